"""Times the slab ocean's training front end on the full-size contexts (1152 atmo regions,
their sst regions' slab reservoirs).

  * sml_slab_train_series over T steps (default 1460, one year) at (window, divisor) =
    (29, 28) and (169, 168), against what a caller could do before it, in the same
    process, pairs alternating: sml_res_tile_series over the series in batches, a torch
    index_select with the slab's atmo_training_data_idx into a [T, slab feedback] buffer,
    then `window` shifted in-order adds and a division.  Both medians, their ratio, and the
    new call's achieved bytes/s against its algorithmic bytes -- (T + window - 1) * tot * 8
    read + T * tot * 8 written -- as a share of 8 TB/s.  The two results are compared bit
    for bit.
  * with --train: one full train_slab_from_grids at that size, with its split into series /
    drive / Gram / solve (device events around the stages of the same loop).

Every figure is the median of --repeats device-event timings after warm-up, with the
smallest and largest beside it.  The atmo context holds no weights: the series call reads
none.  Writes JSON lines to stdout and a markdown table to --out.

    python tools/probe_slab_series.py --out profiles/slab_train.md
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speedy-ml-1_amd"))

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1460)
    ap.add_argument("--forms", type=int, nargs="+", default=[29, 28, 169, 168], help="window divisor pairs")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--batch", type=int, default=64, help="steps per sml_res_tile_series call of the comparison")
    ap.add_argument("--regions", type=int, default=1152, help="the first regions only (a rehearsal, not a measurement)")
    ap.add_argument("--train", action="store_true", help="also time one train_slab_from_grids")
    ap.add_argument("--n-override", type=int, default=None, help="reduced slab n for --train (a rehearsal)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from speedy_ml_amd import domain
    from speedy_ml_amd.reservoir import Reservoirs
    from speedy_ml_amd.synthetic import slab_weights
    from speedy_ml_amd.training import Trainer, fit_standardisation, slab_series, tile_series

    if not torch.cuda.is_available():
        sys.exit("probe_slab_series needs the GPU")
    dev = torch.device("cuda", 0)
    mask = domain.load_sst_mask()
    regions = list(range(args.regions))
    atmo = Reservoirs(regions, [mask[r] for r in regions], [64] * len(regions), [128] * len(regions), weight_dtype="f32")
    sreg = [r for r in regions if mask[r]]
    geo = [domain.region_geometry(r) for r in sreg]
    ninp = [7 * g.inx * g.iny for g in geo]
    if args.train:
        sws = [slab_weights(r, n_override=args.n_override) for r in sreg]
        sn, sk = [w.n for w in sws], [w.k for w in sws]
    else:
        sn, sk = [2 * p for p in ninp], [8] * len(sreg)
    slab = Reservoirs(sreg, [0] * len(sreg), sn, sk, chunk_speedy=0, nout=4, ninp=ninp, out_index=[35] * 4)
    tot_a, tot = int(atmo.fb_offsets[-1]), int(slab.fb_offsets[-1])
    T = args.steps
    gen = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64, device=dev)  # noqa: E731
    g4 = rnd(T, 8, 48, 96, 4) * 8.0 + 250.0
    g2, pr, sst, tisr = rnd(T, 48, 96), rnd(T, 48, 96).abs(), rnd(T, 48, 96) * 5.0 + 285.0, rnd(T, 48, 96).abs() * 300.0
    fit_standardisation(atmo, g4[:32], g2[:32], pr[:32], sst[:32], tisr[:32])  # a table that is not (0, 1)
    # atmo_training_data_idx of every slab reservoir, in the atmo feedback
    row = {r: i for i, r in enumerate(regions)}
    src = []
    for r, g in zip(sreg, geo):
        in2d, o = g.inx * g.iny, int(atmo.fb_offsets[row[r]])
        natmo = 32 * in2d
        src += [o + np.arange(natmo - 4 * in2d, natmo + in2d), o + np.arange(natmo + 2 * in2d, natmo + 4 * in2d)]
    ring_src = torch.from_numpy(np.concatenate(src)).to(dev)
    assert ring_src.numel() == tot
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def summary(ms):
        return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))

    out = torch.zeros(T * tot, dtype=torch.float64, device=dev)
    blocks = torch.zeros(args.batch * tot_a, dtype=torch.float64, device=dev)
    z = torch.zeros((T, tot), dtype=torch.float64, device=dev)
    acc = torch.zeros((T, tot), dtype=torch.float64, device=dev)
    lines = ["# Slab ocean training front end on the MI355X (`tools/probe_slab_series.py`)", "",
             f"Median of {args.repeats} device-event timings after warm-up, smallest .. largest.  The comparison is what a "
             "caller could do before `sml_slab_train_series`, in the same process, pairs alternating: `sml_res_tile_series` "
             f"over the series in batches of {args.batch}, a torch `index_select` with the slabs' `atmo_training_data_idx`, "
             "`window` shifted in-order adds and one division by a tensor.  Algorithmic bytes: (T + window - 1) tot 8 read "
             "+ T tot 8 written.  The accuracy figures and the kernel's earlier form are in DESIGN.md section 3.10.", "",
             f"{len(regions)} atmo regions, {len(sreg)} slab reservoirs, slab feedback {tot} doubles "
             f"({tot * 8 / 1e6:.2f} MB a step), atmo feedback {tot_a} doubles, T = {T}", "",
             "| (window, divisor) | sml_slab_train_series median ms (min .. max) | tile_series + index_select + shifted adds "
             "median ms (min .. max) | ratio | algorithmic bytes | achieved | of 8 TB/s | same bits |",
             "|---|---|---|---|---|---|---|---|"]
    for window, divisor in zip(args.forms[::2], args.forms[1::2]):
        def new():
            slab_series(atmo, slab, g4, g2, pr, sst, tisr, window, divisor, out=out)

        def old():
            for t0 in range(0, T, args.batch):
                m = min(args.batch, T - t0)
                tile_series(atmo, g4[t0:t0 + m], g2[t0:t0 + m], pr[t0:t0 + m], sst[t0:t0 + m], tisr[t0:t0 + m],
                            inputs=blocks)
                torch.index_select(blocks[:m * tot_a].view(m, tot_a), 1, ring_src, out=z[t0:t0 + m])
            acc.zero_()
            for k in range(min(window, T) - 1, -1, -1):  # ascending step order: the oldest term first
                acc[k:] += z[:T - k]
            acc.div_(den)  # (by a tensor: a division by a Python scalar is a multiplication by its reciprocal)

        ramp = min(window - 1, T)
        den = torch.cat([torch.arange(1, ramp + 1, dtype=torch.float64, device=dev),
                         torch.full((T - ramp,), float(divisor), dtype=torch.float64, device=dev)])[:, None]
        for _ in range(2):
            timed(new), timed(old)
        a, b = [], []
        for _ in range(args.repeats):  # pairs alternating
            a.append(timed(new))
            b.append(timed(old))
        same = bool(torch.equal(out.view(T, tot), acc))
        sa, sb = summary(a), summary(b)
        nbytes = (T + window - 1) * tot * 8 + T * tot * 8
        rate = nbytes / (sa["median_ms"] * 1e-3)
        rec = dict(what="slab_series", window=window, divisor=divisor, T=T, new=sa, old=sb,
                   ratio=sb["median_ms"] / sa["median_ms"], bytes=nbytes, bytes_per_s=rate, share_of_8TBs=rate / HBM_PEAK,
                   same_bits=same)
        print(json.dumps(rec), flush=True)
        lines.append(f"| ({window}, {divisor}) | {sa['median_ms']:.3f} ({sa['min_ms']:.3f} .. {sa['max_ms']:.3f}) | "
                     f"{sb['median_ms']:.3f} ({sb['min_ms']:.3f} .. {sb['max_ms']:.3f}) | {rec['ratio']:.1f} x | "
                     f"{nbytes / 1e9:.2f} GB | {rate / 1e12:.3f} TB/s | {100 * rate / HBM_PEAK:.1f} % | {same} |")
    del z, acc, blocks

    if args.train:
        # train_slab_from_grids' loop with events around its stages: (29, 28), 28 phases
        window, divisor, S, discard, nb = 29, 28, 28, 2, 2
        batch = (T // S - discard) // nb
        for j, w in enumerate(sws):
            slab.load_region_weights(j, w)
        slab.set_target_index(np.stack([slab.slab_target_index(j) for j in range(slab.nlocal)]))
        naug = [int(n) for n in slab.n]
        tr = Trainer(naug, 4)
        tr.reset()
        states = torch.empty(sum(naug) * batch, dtype=torch.float64, device=dev)
        targets = torch.empty(len(naug) * batch * 4, dtype=torch.float64, device=dev)
        print("train: weights loaded, trainer created", flush=True)
        wall = time.perf_counter()
        t_series = timed(lambda: slab_series(atmo, slab, g4, g2, pr, sst, tisr, window, divisor, out=out))
        t_drive = t_gram = 0.0
        for i in range(S):
            for j, n in enumerate(naug):
                slab.set_state(j, np.zeros(n))
            t_drive += timed(lambda: slab.synchronize(out[i * tot:], discard, stride=S * tot))
            for b in range(nb):
                col = i + (discard + b * batch) * S
                t_drive += timed(lambda: slab.train_drive(out[col * tot:], batch, None, states, targets, stride=S * tot))
                t_gram += timed(lambda: tr.accumulate(states, targets, batch))
            print(f"train: phase {i + 1} of {S} enqueued and run", flush=True)
        t_solve = timed(lambda: tr.solve(ncs=0, beta_res=1e-4, using_prior=False))
        wall = time.perf_counter() - wall
        tr.close()
        rec = dict(what="train_slab_from_grids", T=T, phases=S, discard_cols=discard, batch=batch, nbatches=nb,
                   n=int(max(naug)), series_ms=t_series, drive_ms=t_drive, gram_ms=t_gram, solve_ms=t_solve,
                   total_ms=t_series + t_drive + t_gram + t_solve, wall_s=wall)
        print(json.dumps(rec), flush=True)
        lines += ["", f"train_slab_from_grids' stages, (29, 28), {S} phases of {discard} + {nb} x {batch} columns, n up to "
                      f"{max(naug)} (one run, device events around each stage; the wall time holds the host's per-phase state resets too):",
                  "", "| series ms | drive ms | Gram ms | solve ms | sum ms | wall s |", "|---|---|---|---|---|---|",
                  f"| {t_series:.1f} | {t_drive:.1f} | {t_gram:.1f} | {t_solve:.1f} | {rec['total_ms']:.1f} | {wall:.2f} |"]
    else:
        lines += ["", "train_slab_from_grids' stages: not run (`--train`)."]
    atmo.close()
    slab.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
