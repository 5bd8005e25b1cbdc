#!/usr/bin/env python
"""Ensemble members against E single-member steps (profiles/members.md).

A configs[1]-shaped context (every region of the decomposition at its own n, fp32 storage,
built from the pieces bench.py builds its reservoirs from) is stepped two ways, alternating
in one process:
  members : predict_members with the context set to E members (one call advances all)
  looped  : the context set to one member, E back-to-back predict calls -- sml_res_step's
            own kernels, i.e. what E forecasts cost without members
Each window is timed with device events after a warm-up and holds enough calls to last
--window seconds; the alternation is repeated --repeats times for the spread.  Then, per
E, the update / readout split (kernel_times) of the members form, the readout's
algorithmic bytes (W_out once per stream of ceil(E / readout_tile), plus E times what is
not weights: x in, local model in, outvec out) as a share of the HBM peak, and its fp64
FMAs over the vector peak.  Prints one JSON line per E and a markdown table.
Needs the GPU; there is no CPU path.
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

HBM_PEAK = 8.0e12          # bytes / s
F64_VALU_PEAK = 78.6e12    # flop / s: 256 CUs x 4 SIMDs x 64 lanes x 2 flop / 4 clk x 2.4 GHz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=1152)
    ap.add_argument("--members", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timed window (>= 0.2)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n-override", type=int, default=None, help="reduced n (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    args = ap.parse_args()

    import torch

    from speedy_ml_amd import domain
    from speedy_ml_amd.reservoir import Reservoirs
    from speedy_ml_amd.synthetic import initial_state, region_weights

    if not torch.cuda.is_available():
        sys.exit("probe_members needs the GPU")
    dev = torch.device("cuda", 0)
    mask = domain.load_sst_mask()
    regions = domain.processor_decomposition(args.regions, 1, 0)
    t0 = time.time()

    def weights(r):
        return region_weights(r, bool(mask[r]), climatology=True, n_override=args.n_override)

    # as bench.py: the sizes first, a region's weights when it is loaded
    if args.n_override is None:
        sizes = [domain.reservoir_sizes(r, bool(mask[r])) for r in regions]
        ws_n, ws_k = [s.n for s in sizes], [s.k for s in sizes]
    else:  # (the reduced n and k are the generator's)
        ws_n, ws_k = (list(v) for v in zip(*((w.n, w.k) for w in map(weights, regions))))
    res = Reservoirs(regions, [mask[r] for r in regions], ws_n, ws_k, weight_dtype="f32")
    for i, r in enumerate(regions):
        w = weights(r)
        res.load_region_weights(i, w)
        res.set_state(i, initial_state(r, w.n))
        if i % 144 == 0:
            print(f"loaded {i}/{len(regions)} regions ({time.time() - t0:.1f}s)", flush=True)
    nl, ncs, nout = res.nlocal, res.ncs, res.nout
    tot = int(res.fb_offsets[-1])
    emax = max(args.members)
    g = torch.Generator(device="cpu").manual_seed(5)
    fb = torch.randn((emax, tot), dtype=torch.float64, generator=g).to(dev)
    lm = torch.randn((emax, nl, ncs), dtype=torch.float64, generator=g).to(dev)
    ov = torch.zeros((emax, nl, nout), dtype=torch.float64, device=dev)
    x0 = [initial_state(r, n) for r, n in zip(regions, ws_n)]

    def set_members(E):
        res.set_members(E)
        for e in range(1, E):  # perturbed copies of member 0's start
            for i in range(nl):
                res.set_state(i, x0[i] * (1.0 - 0.01 * e), member=e)

    def call_members(E):
        res.predict_members(fb[:E], lm[:E], ov[:E])

    def call_looped(E):
        for e in range(E):
            res.predict(fb[e], lm[e], ov[e])

    def window(fn, E, ncalls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ncalls):
            fn(E)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / ncalls  # ms per call

    def calls_for(fn, E):
        for _ in range(5):
            fn(E)
        torch.cuda.synchronize()
        ms = window(fn, E, 10)
        return max(20, int(np.ceil(args.window * 1e3 / ms)))

    wout_bytes = sum(4 * nout * (ncs + n) for n in ws_n)
    rest_bytes = sum(8 * n + 8 * ncs + 8 * nout for n in ws_n)  # x in, local model in, outvec out
    fma = sum(nout * (ncs + n) for n in ws_n)
    weight_bytes, algo_bytes = res.footprint()
    lines = []
    for E in args.members:
        mem_ms, loop_ms = [], []
        for _ in range(args.repeats):
            set_members(E)
            mem_ms.append(window(call_members, E, calls_for(call_members, E)))
            res.set_members(1)
            loop_ms.append(window(call_looped, E, calls_for(call_looped, E)))
        # the update / readout split of the members form, in a window of its own
        set_members(E)
        tile = res.member_tile()
        res.enable_timing(30)
        for _ in range(30):
            call_members(E)
        upd, rd = res.kernel_times()
        res.enable_timing(0)
        res.set_members(1)
        streams = -(-E // max(tile["readout_tile"], 1))
        rd_bytes = streams * wout_bytes + E * rest_bytes
        rd_ms = float(np.median(rd))
        t_bytes, t_flop = rd_bytes / HBM_PEAK * 1e3, 2.0 * fma * E / F64_VALU_PEAK * 1e3
        rec = dict(E=E, tile=tile, members_ms=[round(v, 4) for v in mem_ms], looped_ms=[round(v, 4) for v in loop_ms],
                   members_ms_median=float(np.median(mem_ms)), looped_ms_median=float(np.median(loop_ms)),
                   members_ms_per_member=float(np.median(mem_ms)) / E, spread_ms=float(
                       max(max(mem_ms) - min(mem_ms), max(loop_ms) - min(loop_ms))),
                   update_ms=float(np.median(upd)), readout_ms=rd_ms, readout_streams=streams,
                   readout_algo_bytes=rd_bytes, readout_share_of_hbm_peak=t_bytes / rd_ms,
                   readout_fma=fma * E, readout_fma_ms_at_peak=t_flop, readout_bytes_ms_at_peak=t_bytes,
                   readout_bound="bytes" if t_bytes >= t_flop else "fp64 FMA",
                   footprint_weight_bytes=weight_bytes, footprint_algo_bytes=algo_bytes)
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    print("\n| E | members ms / call | ms / member | E x single ms | spread ms | update ms | readout ms | W_out streams "
          "| readout bytes / 8 TB/s | FMA ms at peak | bound |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in lines:
        print(f"| {r['E']} | {r['members_ms_median']:.3f} | {r['members_ms_per_member']:.3f} | "
              f"{r['looped_ms_median']:.3f} | {r['spread_ms']:.3f} | {r['update_ms']:.3f} | {r['readout_ms']:.3f} | "
              f"{r['readout_streams']} | {r['readout_share_of_hbm_peak']:.2f} | {r['readout_fma_ms_at_peak']:.3f} | "
              f"{r['readout_bound']} |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
