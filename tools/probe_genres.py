#!/usr/bin/env python3
"""Times the spectral radius of all 1152 full-size atmosphere reservoirs and one
genres.generate end to end (profiles/genres.md).

  python tools/probe_genres.py [--regions 1152] [--generate 16] [--seed 20241]

Part 1: the raw draws of `--regions` regions (sizes of domain.reservoir_sizes with the
sst mask) loaded into one context; sml_res_spectral_radius once to warm up, then three
calls timed with HIP events on the call's stream.  The iteration reads A alone, so the
context is a generic one with a single input and output per region: the 38 MB dense
W_in of a real load would only slow the host side of the probe.
Part 2: genres.generate on a real context of the first `--generate` regions at full
size (draw, load, radius, scale, reload), wall clock, and the radius it leaves loaded.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speedy-ml-1_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=1152)
    ap.add_argument("--generate", type=int, default=16)
    ap.add_argument("--seed", type=int, default=20241)
    args = ap.parse_args()

    import torch

    from speedy_ml_amd.domain import load_sst_mask, radius_by_region, reservoir_sizes
    from speedy_ml_amd.genres import generate, generate_region
    from speedy_ml_amd.reservoir import Reservoirs
    from speedy_ml_amd.synthetic import climatology_mean_std

    assert torch.cuda.is_available(), "needs the GPU"
    mask = load_sst_mask()
    regions = list(range(args.regions))
    sz = [reservoir_sizes(r, bool(mask[r])) for r in regions]
    out = {"regions": args.regions, "seed": args.seed}

    # --- part 1: the batched radius
    t0 = time.perf_counter()
    res = Reservoirs(regions, [0] * len(regions), [z.n for z in sz], [z.k for z in sz], chunk_speedy=0, nout=1,
                     ninp=[1] * len(regions), out_index=[-1])
    for i, z in enumerate(sz):
        rows, cols, vals, _, _ = generate_region(z.n, z.k, 1, args.seed, regions[i], 0.5)
        res.load_region(i, rows, cols, vals, np.ones((1, z.n), dtype=np.float32), np.zeros((z.n, 1), dtype=np.float32),
                        np.zeros(36), np.ones(36))
    out["draw_and_load_s"] = round(time.perf_counter() - t0, 3)
    lo, hi, iters, info = res.spectral_radius()  # warm-up
    assert (info == 0).all(), info
    ms = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res.spectral_radius()
        b.record()
        b.synchronize()
        ms.append(round(a.elapsed_time(b), 3))
    res.set_reference_paths(radius_global=True)
    res.spectral_radius()
    gms = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        glo, ghi, git, _ = res.spectral_radius()
        b.record()
        b.synchronize()
        gms.append(round(a.elapsed_time(b), 3))
    assert np.array_equal(glo, lo) and np.array_equal(ghi, hi) and np.array_equal(git, iters)
    rho = (lo + hi) / 2
    out.update(radius_ms_lds=ms, radius_ms_global=gms, iters_min=int(iters.min()), iters_max=int(iters.max()),
               iters_mean=round(float(iters.mean()), 2), rho_min=float(rho.min()), rho_max=float(rho.max()),
               width_max=float(((hi - lo) / hi).max()),
               n_classes=sorted({(z.n, z.k) for z in sz}))
    res.close()

    # --- part 2: generate end to end on a real context
    g = regions[:args.generate]
    gsz = sz[:args.generate]
    res = Reservoirs(g, [int(mask[r]) for r in g], [z.n for z in gsz], [z.k for z in gsz])
    mean, std = climatology_mean_std()
    radius = [radius_by_region(r) for r in g]
    t0 = time.perf_counter()
    ws, raw = generate(res, args.seed, radius, 0.5, mean, std)
    out["generate_regions"] = len(g)
    out["generate_s"] = round(time.perf_counter() - t0, 3)
    lo, hi, _, info = res.spectral_radius()
    assert (info == 0).all()
    out["generate_dev_max"] = float(np.abs((lo + hi) / 2 / np.asarray(radius) - 1).max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
