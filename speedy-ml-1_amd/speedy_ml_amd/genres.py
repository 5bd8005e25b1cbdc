"""Reservoir generation: A drawn and scaled to a spectral radius, W_in drawn.

The stage between the data and the W_out fit (training.train_wout), the reference's
gen_res and the W_in fill of train_reservoir (src/mod_reservoir.f90:180-210, :260-278):

  generate_region(...)  <- makesparse + the W_in fill, on the host (sml_gen_region):
                           a counter-based generator keyed by (seed, region), so a
                           region's draw does not depend on the rank that owns it
  generate(res, ...)    <- gen_res for every local region of a Reservoirs: the raw A
                           loaded, one batched Reservoirs.spectral_radius call (the
                           GPU's power iteration in place of ARPACK), then
                           vals = (vals / rho) * radius (:193) loaded in its place

The draws differ from the reference's RANDOM_NUMBER stream, which is seeded from
system_clock and was never reproducible.  synthetic.py's draws are a different,
unscaled family kept for the bench and the existing tests.
"""
from __future__ import annotations

import numpy as np

from ._lib import check, lib, ptr
from .synthetic import RegionWeights


def generate_region(n: int, k: int, ninp: int, seed: int, region: int, sigma: float):
    """The raw draw of one region (sml_gen_region): rows, cols (int32, 1-based, (k,)),
    vals (float32 (k,), in [0, 1)), win_col (int32 (n,), 0-based), win_val (float32 (n,))."""
    rows, cols = np.zeros(max(k, 0), dtype=np.int32), np.zeros(max(k, 0), dtype=np.int32)
    vals = np.zeros(max(k, 0), dtype=np.float32)
    win_col, win_val = np.zeros(max(n, 0), dtype=np.int32), np.zeros(max(n, 0), dtype=np.float32)
    check(lib().sml_gen_region(int(n), int(k), int(ninp), int(seed) & 0xFFFFFFFFFFFFFFFF, int(region), float(sigma),
                               ptr(rows), ptr(cols), ptr(vals), ptr(win_col), ptr(win_val)))
    return rows, cols, vals, win_col, win_val


def generate(res, seed: int, radius, sigma: float, mean, std):
    """Draw and load A and W_in of every local region of `res` (either kind of context),
    A scaled to spectral radius `radius` (a number, or one per local region); W_out is
    loaded as zero, mean / std ((36,), or one row per local region) as given.  The
    atmosphere's reservoirs use domain.radius_by_region and sigma 0.5, the slab ocean's
    radius 0.9 and sigma 0.6.

    Returns (weights, rho): the RegionWeights of each local region as loaded -- ready for
    training.train_wout and write_region_netcdf once its wout is set -- and the raw draws'
    spectral radii, the midpoints of the GPU's enclosures.  vals are float32 (the file's
    precision), float64 for a context that holds its weights as f64.  A region whose
    iteration does not close (info != 0) raises."""
    nl = res.nlocal
    radius = np.broadcast_to(np.asarray(radius, dtype=np.float64), (nl,))
    mean = np.broadcast_to(np.asarray(mean, dtype=np.float64), (nl, 36))
    std = np.broadcast_to(np.asarray(std, dtype=np.float64), (nl, 36))
    ws = []
    for i in range(nl):
        n, k, ninp, region = int(res.n[i]), int(res.k[i]), res.ninp(i), int(res.region_ids[i])
        rows, cols, vals, wcol, wval = generate_region(n, k, ninp, seed, region, sigma)
        win = np.zeros((ninp, n), dtype=np.float32)
        win[wcol, np.arange(n)] = wval
        wout = np.zeros((res.ncs + n, res.nout), dtype=np.float32)
        w = RegionWeights(region, bool(res.sst[i]), n, ninp, k, rows, cols, vals, win, wout, mean[i].copy(),
                          std[i].copy())
        res.load_region_weights(i, w)
        ws.append(w)
    lo, hi, iters, info = res.spectral_radius()
    if (info != 0).any():
        bad = np.flatnonzero(info != 0)
        raise RuntimeError(f"spectral radius not found for local regions {bad.tolist()}: info {info[bad].tolist()}, "
                           f"lo {lo[bad].tolist()}, hi {hi[bad].tolist()} after {iters[bad].tolist()} iterations")
    rho = (lo + hi) / 2
    for i, w in enumerate(ws):
        scaled = (w.vals.astype(np.float64) / rho[i]) * radius[i]
        w.vals = scaled if res.weight_dtype == "f64" else scaled.astype(np.float32)
        res.load_region_weights(i, w)
    return ws, rho
