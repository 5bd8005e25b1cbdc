"""Times the training front end on the full-size 1152-region context.

  * sml_res_series_stats at T steps (default 1460, one year): the call's device time and the
    achieved bytes/s against two streaming reads of the series, as a share of 8 TB/s;
  * sml_res_tile_series at batch = 16, 64, 256 against what the library offered before it for
    the same work -- batch x (sml_res_tile_feedback, sml_res_tile_tisr_field,
    sml_res_tile_local_model) -- in the same process, pairs alternating.

Every figure is the median of --repeats device-event timings after warm-up, with the
smallest and largest beside it.  The context holds no weights: neither call reads them.
Writes JSON lines to stdout and a markdown table to --out.

    python tools/probe_train_series.py --out profiles/train_series.md
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speedy-ml-1_amd"))

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1460)
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--n-override", type=int, default=None, help="reduced n (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from speedy_ml_amd import domain
    from speedy_ml_amd._lib import check, lib, ptr, stream_ptr
    from speedy_ml_amd.reservoir import Reservoirs
    from speedy_ml_amd.training import fit_standardisation, series_stats, tile_series

    if not torch.cuda.is_available():
        sys.exit("probe_train_series needs the GPU")
    dev = torch.device("cuda", 0)
    mask = domain.load_sst_mask()
    regions = list(range(1152))
    sizes = [domain.reservoir_sizes(r, bool(mask[r])) for r in regions]
    n = [s.n if args.n_override is None else args.n_override for s in sizes]
    k = [s.k if args.n_override is None else 2 * args.n_override for s in sizes]
    res = Reservoirs(regions, [mask[r] for r in regions], n, k, weight_dtype="f32")
    tot, nmod = int(res.fb_offsets[-1]), res.nlocal * res.ncs
    T, bmax = args.steps, max(args.batches)
    if T < bmax:
        sys.exit("--steps must cover the largest batch")
    gen = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64, device=dev)  # noqa: E731
    g4 = rnd(T, 8, 48, 96, 4) * 8.0 + 250.0
    g2, pr, sst, tisr = rnd(T, 48, 96), rnd(T, 48, 96).abs(), rnd(T, 48, 96) * 5.0 + 285.0, rnd(T, 48, 96).abs() * 300.0
    fc4, fc2 = g4[:bmax] + 0.5, g2[:bmax] + 0.01
    fit_standardisation(res, g4[:32], g2[:32], pr[:32], sst[:32], tisr[:32])  # a table that is not (0, 1)
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

    rows, lines = [], []
    # --- the statistics
    stats = lambda: series_stats(res, g4, g2, pr, sst, tisr)  # noqa: E731
    for _ in range(2):
        timed(stats)
    s = summary([timed(stats) for _ in range(args.repeats)])
    nbytes = 2 * T * (147456 + 4 * 4608) * 8
    rate = nbytes / (s["median_ms"] * 1e-3)
    row = dict(what="series_stats", T=T, bytes=nbytes, bytes_per_s=rate, share_of_8TBs=rate / HBM_PEAK, **s)
    rows.append(row)
    print(json.dumps(row), flush=True)
    lines += ["| call | T | median ms | min .. max ms | bytes (two reads of the series) | achieved | of 8 TB/s |",
              "|---|---|---|---|---|---|---|",
              f"| series_stats | {T} | {s['median_ms']:.3f} | {s['min_ms']:.3f} .. {s['max_ms']:.3f} | {nbytes / 1e9:.2f} GB "
              f"| {rate / 1e12:.2f} TB/s | {100 * rate / HBM_PEAK:.0f} % |", ""]
    # --- the tilings
    inputs = torch.zeros(bmax * tot, dtype=torch.float64, device=dev)
    model = torch.zeros(bmax * nmod, dtype=torch.float64, device=dev)
    L, st = lib(), stream_ptr(None)
    lines += ["| batch | tile_series median ms (min .. max) | batch x 3 single-grid launches median ms (min .. max) | ratio |",
              "|---|---|---|---|"]
    for B in args.batches:
        def series():
            tile_series(res, g4[:B], g2[:B], pr[:B], sst[:B], tisr[:B], fc4[:B], fc2[:B], inputs=inputs, model=model)

        def per_grid():
            for t in range(B):
                fb, lm = inputs[t * tot:], model[t * nmod:]
                check(L.sml_res_tile_feedback(res.handle, ptr(g4[t]), ptr(g2[t]), ptr(pr[t]), None, ptr(fb), st))
                check(L.sml_res_tile_tisr_field(res.handle, ptr(tisr[t]), ptr(fb), st))
                check(L.sml_res_tile_local_model(res.handle, ptr(fc4[t]), ptr(fc2[t]), ptr(lm), st))

        for _ in range(2):
            timed(series), timed(per_grid)
        a, b = [], []
        for _ in range(args.repeats):  # pairs alternating
            a.append(timed(series))
            b.append(timed(per_grid))
        sa, sb = summary(a), summary(b)
        row = dict(what="tile_series", batch=B, series=sa, per_grid=sb, ratio=sb["median_ms"] / sa["median_ms"],
                   written_bytes=B * (tot + nmod) * 8)
        rows.append(row)
        print(json.dumps(row), flush=True)
        lines.append(f"| {B} | {sa['median_ms']:.3f} ({sa['min_ms']:.3f} .. {sa['max_ms']:.3f}) | {sb['median_ms']:.3f} "
                     f"({sb['min_ms']:.3f} .. {sb['max_ms']:.3f}) | {row['ratio']:.2f} x |")
    res.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
