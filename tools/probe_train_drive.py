#!/usr/bin/env python
"""Times the training drive on one MI355X: 144 full-size regions, m = 1024 columns.

Three paths, each timed with HIP events after a warm-up call, best and median of
--reps calls:
  persistent   sml_res_train_drive, one launch per batch (k_res_drive)
  stepwise     the same call with SML_RES_PATH_STEPWISE_DRIVE (column writer + update
               launch per column)
  synchronize  sml_res_synchronize(length = m): the update alone, nothing recorded
With SML_LIB pointing at a build without the drive (an earlier commit's library) only
the synchronize figure is taken: that is the yardstick the persistent kernel is held
to (profiles/train_drive.md).  Not part of bench.py.

    python tools/probe_train_drive.py [--regions 144] [--m 1024] [--reps 3] [--n-override N]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speedy-ml-1_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=144)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n-override", type=int, default=None, help="reduced reservoirs (a quick check of the tool)")
    args = ap.parse_args()

    import torch

    from speedy_ml_amd import _lib
    from speedy_ml_amd.domain import load_sst_mask, reservoir_sizes
    from speedy_ml_amd.reservoir import Reservoirs
    from speedy_ml_amd.synthetic import region_weights

    dev = torch.device("cuda:0")
    have_drive = hasattr(_lib.lib(), "sml_res_train_drive")
    sst = load_sst_mask()
    regions = list(range(args.regions))
    # one synthetic weight set per shape class (ninp, sst), shared by the regions of the class
    classes, ws = {}, []
    for r in regions:
        key = (reservoir_sizes(r, bool(sst[r])).ninp, bool(sst[r]))
        if key not in classes:
            classes[key] = region_weights(r, bool(sst[r]), n_override=args.n_override)
        ws.append(classes[key])
    res = Reservoirs(regions, [int(sst[r]) for r in regions], [w.n for w in ws], [w.k for w in ws])
    for i, w in enumerate(ws):
        res.load_region_weights(i, w)
    m, tot, ncs = args.m, int(res.fb_offsets[-1]), res.ncs
    naug = int(res.n.sum()) + res.nlocal * ncs
    g = torch.Generator(device=dev).manual_seed(3)
    d_in = torch.randn((m, tot), dtype=torch.float64, device=dev, generator=g)
    d_mo = torch.rand((m, res.nlocal * ncs), dtype=torch.float64, device=dev, generator=g) * 2.0 - 1.0
    d_s = torch.empty(naug * m, dtype=torch.float64, device=dev)
    d_t = torch.empty(res.nlocal * m * res.nout, dtype=torch.float64, device=dev)

    def zero_states():
        for i, n in enumerate(res.n):
            res.set_state(i, np.zeros(int(n)))

    def timed(fn):
        zero_states()
        fn()  # warm-up (first-use tables, code load)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            zero_states()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return {"best_ms": min(ms), "median_ms": float(np.median(ms))}

    out = {"regions": args.regions, "m": m, "n_total": int(res.n.sum()), "state_bytes": naug * m * 8,
           "target_bytes": res.nlocal * m * res.nout * 8, "have_drive": have_drive,
           "lib": os.environ.get("SML_LIB") or "tree"}
    out["synchronize"] = timed(lambda: res.synchronize(d_in, m))
    if have_drive:
        res.set_reference_paths(stepwise_drive=False)
        out["persistent"] = timed(lambda: res.train_drive(d_in, m, d_mo, d_s, d_t))
        res.set_reference_paths(stepwise_drive=True)
        out["stepwise"] = timed(lambda: res.train_drive(d_in, m, d_mo, d_s, d_t))
        res.set_reference_paths()
        for k in ("persistent", "stepwise"):
            out[k]["state_GBps"] = out["state_bytes"] / (out[k]["best_ms"] * 1e-3) / 1e9
    print(json.dumps(out))


if __name__ == "__main__":
    main()
