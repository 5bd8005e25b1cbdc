"""oracle/oracle.py -- TEST INFRASTRUCTURE ONLY (ctypes wrapper of liboracle.so).

The checker for the SPEEDY-ML hot path.  Only tests/, __graft_entry__.smoke()
and bench.py's cpu_baseline leg import this module.  It never ships in the
product path (speedy-ml-1_amd/ never imports it).

Every function mirrors one routine of speedy_oracle.c, which in turn cites the
reference file:line it restates.  Arrays are numpy float64, laid out exactly as
the reference's Fortran arrays (column-major), i.e. a spectral field
v(mx2=62,nx=32) is a C array of shape (32, 62) and a grid field g(96,48) is a C
array of shape (48, 96).
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "liboracle.so")
REF_SPECTRAL_PATH = os.path.join(HERE, "_ref", "libspeedy_ref_spectral.so")

MX, NX, MX2, IX, IY, IL = 31, 32, 62, 96, 24, 48
EARTH_RADIUS = 6.371e6  # mod_dyncon1.f90: rearth

_lib = None
_init_radius = None


def build() -> None:
    """Compile liboracle.so (gcc).  Cheap; called by __graft_entry__.build()."""
    subprocess.run(["make", "-s", "-C", HERE], check=True)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        _lib = ctypes.CDLL(LIB_PATH)
        _declare(_lib)
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _declare(L):
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.orc_spectral_init.argtypes = [d]
    L.orc_get_tables.argtypes = [vp, vp, vp, vp]
    for name in ("orc_gridy", "orc_specy", "orc_specx", "orc_spec", "orc_lap", "orc_invlap"):
        getattr(L, name).argtypes = [vp, vp]
    L.orc_gridx.argtypes = [vp, vp, i]
    L.orc_grid.argtypes = [vp, vp, i]
    L.orc_vds.argtypes = [vp, vp, vp, vp]
    L.orc_uvspec.argtypes = [vp, vp, vp, vp]
    L.orc_grad.argtypes = [vp, vp, vp]
    L.orc_vdspec.argtypes = [vp, vp, vp, vp, i]
    L.orc_trunct.argtypes = [vp]
    L.orc_region_geometry_ints.argtypes = [i, i, i, vp]
    L.orc_radius_by_region.argtypes = [i, i]
    L.orc_radius_by_region.restype = d
    L.orc_reservoir_sizes.argtypes = [i, i, i, i, vp]
    L.orc_predict.argtypes = [i, i, i, vp, vp, vp, vp, vp, i, i, d, vp, vp, vp, vp, vp, vp, i]
    L.orc_predict_f32.argtypes = [i, i, i, vp, vp, vp, vp, vp, vp, i, i, d, vp, vp, vp, vp, vp, vp, i]
    L.orc_predict_regions.argtypes = [i, i, vp, vp, vp, vp, vp, vp, vp, vp, i, i, d, vp, vp, vp, vp, vp, vp]
    L.orc_predict_f32_regions.argtypes = [i, i, vp, vp, vp] + [vp] * 6 + [i, i, d] + [vp] * 6
    L.orc_predict_slab_ml_f32.argtypes = [i, i, vp, vp, vp, vp, vp, vp, i, d, vp, vp, vp, d, d]
    L.orc_unstandardize_res.argtypes = [vp, i, i, i, vp, vp, i, i, i, i]
    L.orc_assemble.argtypes = [i, vp, i, vp, vp, vp]
    L.orc_tile_feedback.argtypes = [i, i, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orc_tile_local_model.argtypes = [i, i, vp, vp, vp, vp, vp]
    L.orc_dyn_init.argtypes = []
    L.orc_dyn_impint.argtypes = [d, d]
    L.orc_dyn_step.argtypes = [vp] * 9 + [i, i, d, d, d, d, vp, vp]
    L.orc_iogrid30.argtypes = [vp] * 8
    L.orc_iogrid31.argtypes = [vp] * 7
    L.orc_train_accumulate.argtypes = [i, i, i, vp, vp, vp, vp]
    L.orc_phys_init.argtypes = [vp, vp]
    L.orc_phys_tables.argtypes = [vp, vp, vp]
    L.orc_sol_oz.argtypes = [d, vp, vp, vp, vp, vp]
    L.orc_sflset.argtypes = [vp, vp]
    L.orc_phypar_grid.argtypes = [vp] * 11 + [i, vp]
    L.orc_phypar_grid_census.argtypes = [vp] * 11 + [i, vp, vp]
    L.orc_phys_census_size.argtypes = []
    L.orc_phys_inputs.argtypes = [vp] * 12
    L.orc_train_solve.argtypes = [i, i, i, d, d, i, d, vp, vp, vp]
    L.orc_newdate.argtypes = [i, i, vp, vp]
    L.orc_forint.argtypes = [i, d, vp, vp]
    L.orc_forin5.argtypes = [i, d, vp, vp]
    L.orc_coupler.argtypes = [i, i] + [vp] * 7
    L.orc_fordate.argtypes = [d] + [vp] * 15


def spectral_init(radius: float = EARTH_RADIUS) -> None:
    global _init_radius
    if _init_radius != radius:
        lib().orc_spectral_init(radius)
        _init_radius = radius


def tables():
    spectral_init()
    sia = np.zeros(IY)
    wt = np.zeros(IY)
    cpol = np.zeros((IY, NX, MX2))
    nsh2 = np.zeros(NX, dtype=np.int32)
    lib().orc_get_tables(_p(sia), _p(wt), _p(cpol), _p(nsh2))
    return {"sia": sia, "wt": wt, "cpol": cpol, "nsh2": nsh2}


def _f64(a, shape):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.shape == shape, (a.shape, shape)
    return a


def gridy(v):
    spectral_init()
    v = _f64(v, (NX, MX2))
    out = np.zeros((IL, MX2))
    lib().orc_gridy(_p(v), _p(out))
    return out


def gridx(varm, kcos=1):
    spectral_init()
    varm = _f64(varm, (IL, MX2))
    out = np.zeros((IL, IX))
    lib().orc_gridx(_p(varm), _p(out), kcos)
    return out


def specx(g):
    spectral_init()
    g = _f64(g, (IL, IX))
    out = np.zeros((IL, MX2))
    lib().orc_specx(_p(g), _p(out))
    return out


def specy(varm):
    spectral_init()
    varm = _f64(varm, (IL, MX2))
    out = np.zeros((NX, MX2))
    lib().orc_specy(_p(varm), _p(out))
    return out


def grid(v, kcos=1):
    spectral_init()
    v = _f64(v, (NX, MX2))
    out = np.zeros((IL, IX))
    lib().orc_grid(_p(v), _p(out), kcos)
    return out


def spec(g):
    spectral_init()
    g = _f64(g, (IL, IX))
    out = np.zeros((NX, MX2))
    lib().orc_spec(_p(g), _p(out))
    return out


def vdspec(ug, vg, kcos=2):
    spectral_init()
    ug = _f64(ug, (IL, IX))
    vg = _f64(vg, (IL, IX))
    vor = np.zeros((NX, MX2))
    div = np.zeros((NX, MX2))
    lib().orc_vdspec(_p(ug), _p(vg), _p(vor), _p(div), kcos)
    return vor, div


def uvspec(vor, div):
    spectral_init()
    vor = _f64(vor, (NX, MX2))
    div = _f64(div, (NX, MX2))
    u = np.zeros((NX, MX2))
    v = np.zeros((NX, MX2))
    lib().orc_uvspec(_p(vor), _p(div), _p(u), _p(v))
    return u, v


def vds(ucos, vcos):
    spectral_init()
    ucos = _f64(ucos, (NX, MX2))
    vcos = _f64(vcos, (NX, MX2))
    vor = np.zeros((NX, MX2))
    div = np.zeros((NX, MX2))
    lib().orc_vds(_p(ucos), _p(vcos), _p(vor), _p(div))
    return vor, div


def grad(psi):
    spectral_init()
    psi = _f64(psi, (NX, MX2))
    dx = np.zeros((NX, MX2))
    dy = np.zeros((NX, MX2))
    lib().orc_grad(_p(psi), _p(dx), _p(dy))
    return dx, dy


def lap(s):
    spectral_init()
    s = _f64(s, (NX, MX2))
    out = np.zeros((NX, MX2))
    lib().orc_lap(_p(s), _p(out))
    return out


def invlap(s):
    spectral_init()
    s = _f64(s, (NX, MX2))
    out = np.zeros((NX, MX2))
    lib().orc_invlap(_p(s), _p(out))
    return out


def trunct(s):
    spectral_init()
    s = _f64(s, (NX, MX2)).copy()
    lib().orc_trunct(_p(s))
    return s


# ---------------------------------------------------------------- domain
GEOM_FIELDS = ("res_xstart", "res_xend", "res_ystart", "res_yend", "resxchunk", "resychunk",
               "input_xstart", "input_xend", "input_ystart", "input_yend", "inputxchunk", "inputychunk",
               "pole", "periodic", "tdata_xstart", "tdata_xend", "tdata_ystart", "tdata_yend")


def region_geometry(region: int, numregions: int = 1152, overlap: int = 1) -> dict:
    out = np.zeros(len(GEOM_FIELDS), dtype=np.int32)
    lib().orc_region_geometry_ints(numregions, region, overlap, _p(out))
    return dict(zip(GEOM_FIELDS, (int(v) for v in out)))


def radius_by_region(region: int, numregions: int = 1152) -> float:
    return float(lib().orc_radius_by_region(numregions, region))


def reservoir_sizes(region: int, sst: bool, numregions: int = 1152, m_nodes: int = 6000) -> dict:
    out = np.zeros(5, dtype=np.int32)
    lib().orc_reservoir_sizes(numregions, region, int(bool(sst)), m_nodes, _p(out))
    return dict(zip(("ninp", "n", "k", "chunk_pred", "chunk_speedy"), (int(v) for v in out)))


# ---------------------------------------------------------------- reservoir
def _check_unstandardize(unstandardize, nout):
    # orc_unstandardize_res walks the 2x2 region's 136 outputs: on a shorter outvec it
    # would run past the array
    if unstandardize and nout != 136:
        raise ValueError(f"unstandardize=True needs the 2x2 region's 136 outputs, not {nout}")


def predict(rows, cols, vals, win_dense, wout, feedback, local_model, x, mean, std,
            chunk_speedy=132, leakage=1.0, unstandardize=True):
    """Reference predict (mod_reservoir.f90:1416-1487).  win_dense: (ninp, n) C array
    == Fortran win(n, ninp); wout: (ncs+n, nout) C array == Fortran wout(nout, ncs+n).
    Returns (outvec, x_new)."""
    ninp, n = win_dense.shape
    k = len(rows)
    nout = wout.shape[1]
    _check_unstandardize(unstandardize, nout)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    win_dense = np.ascontiguousarray(win_dense, dtype=np.float64)
    wout = np.ascontiguousarray(wout, dtype=np.float64)
    feedback = np.ascontiguousarray(feedback, dtype=np.float64)
    lm = np.ascontiguousarray(local_model if local_model is not None else np.zeros(1), dtype=np.float64)
    xx = np.array(x, dtype=np.float64, copy=True)
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    std = np.ascontiguousarray(std, dtype=np.float64)
    out = np.zeros(nout)
    lib().orc_predict(n, ninp, k, _p(rows), _p(cols), _p(vals), _p(win_dense), _p(wout), nout,
                      chunk_speedy, leakage, _p(feedback), _p(lm), _p(xx), _p(out), _p(mean), _p(std),
                      int(bool(unstandardize)))
    return out, xx


def predict_regions(regions, feedbacks, local_models, xs, nthreads=1, chunk_speedy=132, leakage=1.0):
    """orc_predict over many regions with OpenMP (the CPU baseline's reservoir leg).
    regions: list of dicts with rows, cols, vals, win (ninp, n), wout (ncs+n, nout),
    mean, std as contiguous float64 / int32 arrays; xs updated in place.  Returns
    outvecs [nreg, nout]."""
    nreg = len(regions)
    nout = regions[0]["wout"].shape[1]

    def table(arrs):
        return (ctypes.c_void_p * nreg)(*[a.ctypes.data for a in arrs])

    n = np.array([r["win"].shape[1] for r in regions], dtype=np.int32)
    ninp = np.array([r["win"].shape[0] for r in regions], dtype=np.int32)
    k = np.array([len(r["rows"]) for r in regions], dtype=np.int32)
    out = np.zeros((nreg, nout))
    keys = ("rows", "cols", "vals", "win", "wout")
    tabs = [table([r[key] for r in regions]) for key in keys]
    lib().orc_predict_regions(nreg, int(nthreads), _p(n), _p(ninp), _p(k), *tabs, nout, chunk_speedy, leakage,
                              table(feedbacks), table(local_models), table(xs), _p(out),
                              table([r["mean"] for r in regions]), table([r["std"] for r in regions]))
    return out


def predict_f32(rows, cols, vals_f32, win_col, win_val_f32, wout_f32, feedback, local_model, x, mean, std,
                chunk_speedy=132, leakage=1.0, unstandardize=True):
    """Same arithmetic with the compressed W_in (one entry per row) and fp32 weights."""
    n = len(win_col)
    nout = wout_f32.shape[1]
    _check_unstandardize(unstandardize, nout)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    vals_f32 = np.ascontiguousarray(vals_f32, dtype=np.float32)
    win_col = np.ascontiguousarray(win_col, dtype=np.int32)
    win_val_f32 = np.ascontiguousarray(win_val_f32, dtype=np.float32)
    wout_f32 = np.ascontiguousarray(wout_f32, dtype=np.float32)
    feedback = np.ascontiguousarray(feedback, dtype=np.float64)
    lm = np.ascontiguousarray(local_model if local_model is not None else np.zeros(1), dtype=np.float64)
    xx = np.array(x, dtype=np.float64, copy=True)
    out = np.zeros(nout)
    lib().orc_predict_f32(n, len(feedback), len(rows), _p(rows), _p(cols), _p(vals_f32), _p(win_col),
                          _p(win_val_f32), _p(wout_f32), nout, chunk_speedy, leakage, _p(feedback), _p(lm),
                          _p(xx), _p(out), _p(np.ascontiguousarray(mean, dtype=np.float64)),
                          _p(np.ascontiguousarray(std, dtype=np.float64)), int(bool(unstandardize)))
    return out, xx


def predict_f32_regions(regs, feedbacks, local_models, xs, nthreads=8, chunk_speedy=132, leakage=1.0):
    """predict_f32 over many regions with OpenMP.  regs: dicts with rows, cols, vals
    (f32), win_col (i32), win_val (f32), wout (f32, (ncs+n, nout)), mean, std; xs
    (float64 arrays) updated in place.  Returns outvecs [nreg, nout]."""
    nreg = len(regs)
    nout = regs[0]["wout"].shape[1]

    def table(arrs):
        return (ctypes.c_void_p * nreg)(*[a.ctypes.data for a in arrs])

    n = np.array([len(r["win_col"]) for r in regs], dtype=np.int32)
    ninp = np.array([len(f) for f in feedbacks], dtype=np.int32)
    k = np.array([len(r["rows"]) for r in regs], dtype=np.int32)
    fbs = [np.ascontiguousarray(f, dtype=np.float64) for f in feedbacks]
    lms = [np.ascontiguousarray(m if m is not None else np.zeros(1), dtype=np.float64) for m in local_models]
    out = np.zeros((nreg, nout))
    tabs = [table([r[key] for r in regs]) for key in ("rows", "cols", "vals", "win_col", "win_val", "wout")]
    lib().orc_predict_f32_regions(nreg, int(nthreads), _p(n), _p(ninp), _p(k), *tabs, nout, chunk_speedy, leakage,
                                  table(fbs), table(lms), table(xs), _p(out), table([r["mean"] for r in regs]),
                                  table([r["std"] for r in regs]))
    return out


# ---------------------------------------------------------------- slab ocean
def predict_slab_ml_f32(rows, cols, vals_f32, win_col, win_val_f32, wout_f32, feedback, x, mean_sst, std_sst,
                        leakage=1.0):
    """predict_slab_ml (mod_slab_ocean_reservoir.f90:1251-1296).  Returns (outvec, x_new)."""
    n = len(win_col)
    nout = wout_f32.shape[1]
    xx = np.array(x, dtype=np.float64, copy=True)
    out = np.zeros(nout)
    lib().orc_predict_slab_ml_f32(n, len(rows), _p(np.ascontiguousarray(rows, dtype=np.int32)),
                                  _p(np.ascontiguousarray(cols, dtype=np.int32)),
                                  _p(np.ascontiguousarray(vals_f32, dtype=np.float32)),
                                  _p(np.ascontiguousarray(win_col, dtype=np.int32)),
                                  _p(np.ascontiguousarray(win_val_f32, dtype=np.float32)),
                                  _p(np.ascontiguousarray(wout_f32, dtype=np.float32)), nout, leakage,
                                  _p(np.ascontiguousarray(feedback, dtype=np.float64)), _p(xx), _p(out),
                                  float(mean_sst), float(std_sst))
    return out, xx


def slab_input_index(region, numregions=1152):
    """atmo_training_data_idx (mod_slab_ocean_reservoir.f90:1550-1563), 0-based, into
    the bottom-level atmo feedback of a region with an sst input: the lowest level's
    4 variables (the last 4*in2d of atmo3d), logp, then sst, then tisr."""
    geo = region_geometry(region, numregions)
    in2d = geo["inputxchunk"] * geo["inputychunk"]
    natmo = 4 * in2d * 8
    return np.concatenate([np.arange(natmo - 4 * in2d, natmo + in2d), np.arange(natmo + 2 * in2d, natmo + 4 * in2d)])


def tile_2d(region, grid2d, numregions=1152):
    """tileoverlapgrid of one 2-D field (res_domain.f90:348-420): the region's
    overlap input tile, x fastest (tile_4d_and_logp_to_local_state_input_slab)."""
    geo = region_geometry(region, numregions)
    ix, iy = geo["inputxchunk"], geo["inputychunk"]
    xs = [(geo["input_xstart"] - 1 + lx) % 96 for lx in range(ix)]  # periodic wrap in x
    ys = [geo["input_ystart"] - 1 + ly for ly in range(iy)]
    return np.array([grid2d[y, x] for y in ys for x in xs])


def sst_grid(sst_rows, base_sst, sea_mask, numregions=1152):
    """sendrecievegrid's wholegrid_sst (mpires.f90:288-319, 458-472): base_sst_grid,
    every region's sst (its slab outvec, or 272 K without one) tiled on its resolved
    points (tile_full_2d_grid_with_local_res), base_sst_grid where sea_mask > 0, then
    a 272 K floor (train_on_sst_anomalies off).  sst_rows [numregions][resx*resy];
    grids (48, 96) == Fortran (96, 48)."""
    g = np.array(base_sst, dtype=np.float64, copy=True)
    for r in range(numregions):
        geo = region_geometry(r, numregions)
        rx, ry = geo["resxchunk"], geo["resychunk"]
        g[geo["res_ystart"] - 1:geo["res_ystart"] - 1 + ry, geo["res_xstart"] - 1:geo["res_xstart"] - 1 + rx] = \
            np.asarray(sst_rows[r]).reshape(ry, rx)
    g = np.where(sea_mask > 0.0, base_sst, g)
    return np.where(g < 272.0, 272.0, g)


def hybrid_sst_am(sst_cpl, sst_hybrid, sice, tice, bias=0.0):
    """ini_sea's hybrid block (cpl_sea.f90:38-46) on the coupler's (ice-blended) sst_am."""
    s = np.where(sst_cpl - sst_hybrid < 6.0, sst_hybrid, sst_cpl)
    s = s + bias
    d = tice - s
    return s + sice * d


# ---------------------------------------------------------------- exchange / tiling
def assemble(outvecs):
    outvecs = np.ascontiguousarray(outvecs, dtype=np.float64)
    nreg, outlen = outvecs.shape
    g4 = np.zeros((8, 48, 96, 4))
    g2 = np.zeros((48, 96))
    pr = np.zeros((48, 96))
    lib().orc_assemble(nreg, _p(outvecs), outlen, _p(g4), _p(g2), _p(pr))
    return g4, g2, pr


def tile_feedback(region, g4, g2, pr, mean, std, tisr_std, sst_std=None, numregions=1152):
    geo = region_geometry(region, numregions)
    in2d = geo["inputxchunk"] * geo["inputychunk"]
    ninp = 4 * in2d * 8 + 3 * in2d + (in2d if sst_std is not None else 0)
    fb = np.zeros(ninp)
    sst_ptr = None
    if sst_std is not None:
        sst_std = np.ascontiguousarray(sst_std, dtype=np.float64)
        sst_ptr = _p(sst_std)
    lib().orc_tile_feedback(numregions, region, _p(np.ascontiguousarray(g4)), _p(np.ascontiguousarray(g2)),
                            _p(np.ascontiguousarray(pr)), _p(np.ascontiguousarray(mean, dtype=np.float64)),
                            _p(np.ascontiguousarray(std, dtype=np.float64)),
                            _p(np.ascontiguousarray(tisr_std, dtype=np.float64)), sst_ptr, _p(fb))
    return fb


def tile_local_model(region, fc4d, fc2d, mean, std, numregions=1152):
    lm = np.zeros(132)
    lib().orc_tile_local_model(numregions, region, _p(np.ascontiguousarray(fc4d)), _p(np.ascontiguousarray(fc2d)),
                               _p(np.ascontiguousarray(mean, dtype=np.float64)),
                               _p(np.ascontiguousarray(std, dtype=np.float64)), _p(lm))
    return lm


# ---------------------------------------------------------------- dynamics
KX = 8
DYN_FIELDS = ("vor", "div", "t", "tr", "ps")


def dyn_state_copy(st):
    """Contiguous complex128 copies: vor/div/t/tr (2, kx, nx, mx), ps (2, nx, mx)."""
    return {f: np.ascontiguousarray(st[f], dtype=np.complex128).copy() for f in DYN_FIELDS}


def dyn_step(state, phis, tcorh, qcorh, phys, j1, j2, dt, alph, rob=0.05, wil=0.53):
    """One SPEEDY `step` (dyn_step.f90:1-128) on `state` (updated in place).

    impint(dt, alph) is evaluated first, as stepone/stloop do before their steps.
    phys: physics grid tendencies (4, kx, 48, 96) = u, v, t, q, or None.
    Returns (phi = geop(j4) (kx, nx, mx) complex, tendencies before timint
    (4*kx+1, nx, mx) complex: vordt | divdt | tdt | trdt | psdt)."""
    spectral_init()
    L = lib()
    L.orc_dyn_init()
    L.orc_dyn_impint(dt, alph)
    for f in DYN_FIELDS:
        a = state[f]
        assert a.dtype == np.complex128 and a.flags.c_contiguous
    cplx = lambda a: np.ascontiguousarray(a, dtype=np.complex128)
    phis, tcorh, qcorh = cplx(phis), cplx(tcorh), cplx(qcorh)
    ph = None if phys is None else np.ascontiguousarray(phys, dtype=np.float64)
    phi = np.zeros((KX, NX, MX), np.complex128)
    tend = np.zeros((4 * KX + 1, NX, MX), np.complex128)
    L.orc_dyn_step(_p(state["vor"]), _p(state["div"]), _p(state["t"]), _p(state["ps"]), _p(state["tr"]),
                   _p(phis), _p(tcorh), _p(qcorh), None if ph is None else _p(ph), j1, j2, dt, alph, rob, wil,
                   _p(phi), _p(tend))
    return phi, tend


def iogrid30(state, grid4d, logp):
    """iogrid(30): window entry into level 1 of `state` (in place); returns
    (minmax[8], is_safe).  grid4d: variables3d (4, 96, 48, 8) Fortran order ==
    C (8, 48, 96, 4); logp (48, 96)."""
    spectral_init()
    g = np.ascontiguousarray(grid4d, dtype=np.float64)
    lp = np.ascontiguousarray(logp, dtype=np.float64)
    mm = np.zeros(8)
    safe = lib().orc_iogrid30(_p(g), _p(lp), _p(state["vor"]), _p(state["div"]), _p(state["t"]), _p(state["ps"]),
                              _p(state["tr"]), _p(mm))
    return mm, bool(safe)


def iogrid31(state):
    """iogrid(31): level 1 of `state` -> (grid4d (8, 48, 96, 4), logp (48, 96))."""
    spectral_init()
    g = np.zeros((KX, IL, IX, 4))
    lp = np.zeros((IL, IX))
    lib().orc_iogrid31(_p(state["vor"]), _p(state["div"]), _p(state["t"]), _p(state["ps"]), _p(state["tr"]),
                       _p(g), _p(lp))
    return g, lp


# ---------------------------------------------------------------- training
def train_accumulate(S, T, G, B):
    """chunking_matmul: G += S S^T, B += T S^T.  S (naug, m) / T (nout, m) Fortran
    order == C arrays (m, naug) / (m, nout); G (naug, naug) as C (naug, naug)
    transposed-symmetric; B (nout, naug) Fortran == C (naug, nout)."""
    S = np.ascontiguousarray(S, dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.float64)
    m, naug = S.shape
    nout = T.shape[1]
    assert T.shape[0] == m and G.shape == (naug, naug) and B.shape == (naug, nout)
    lib().orc_train_accumulate(naug, nout, m, _p(S), _p(T), _p(G), _p(B))


def train_solve(G, B, ncs, beta_res, beta_model, using_prior=True, prior_val=0.0):
    """fit_chunk_hybrid + mldivide; returns (wout as C (naug, nout) == Fortran
    wout(nout, naug), info).  G, B are consumed (copies are made)."""
    G = np.array(G, dtype=np.float64, order="C")
    B = np.ascontiguousarray(B, dtype=np.float64)
    naug, nout = B.shape
    w = np.zeros((naug, nout))
    info = lib().orc_train_solve(naug, nout, ncs, beta_res, beta_model, int(using_prior), prior_val, _p(G), _p(B),
                                 _p(w))
    return w, info


# ---------------------------------------------------------------- physics
NGP = IX * IL
PHYS_BC = ("fmask1", "phis0", "stl_am", "sst_am", "soilw_am", "alb_l", "alb_s", "albsfc", "snowc",
           "fsol", "ozone", "ozupp", "zenit", "stratz", "forog")
HSG = np.array([0.000, 0.050, 0.140, 0.260, 0.420, 0.600, 0.770, 0.900, 1.000])


def radang():
    """radang(il) of indyns (ini_indyns.f90:49-56) from the Gaussian latitudes."""
    sia = tables()["sia"]
    r = np.zeros(IL)
    r[:IY] = -np.arcsin(sia)
    r[IL - 1:IY - 1:-1] = np.arcsin(sia)
    return r


def phys_init():
    """inphys(hsg, ppl, radang) + radset."""
    spectral_init()
    lib().orc_phys_init(_p(np.ascontiguousarray(HSG)), _p(np.ascontiguousarray(radang())))


def sol_oz(tyear):
    phys_init()
    out = [np.zeros(NGP) for _ in range(5)]
    lib().orc_sol_oz(tyear, *[_p(o) for o in out])
    return dict(zip(("fsol", "ozone", "ozupp", "zenit", "stratz"), out))


def sflset(phi0):
    forog = np.zeros(NGP)
    lib().orc_sflset(_p(np.ascontiguousarray(phi0, dtype=np.float64).ravel()), _p(forog))
    return forog


def phys_inputs(state, phis):
    """phypar's grid inputs of level 1 of `state` (geop(1), uvspec, grid):
    (ug1, vg1, tg1, qg1, phig1 (kx, ngp), pslg1 (ngp,))."""
    spectral_init()
    L = lib()
    L.orc_dyn_init()
    outs = [np.zeros((KX, NGP)) for _ in range(5)] + [np.zeros(NGP)]
    ph = np.ascontiguousarray(phis, dtype=np.complex128)
    L.orc_phys_inputs(_p(state["vor"]), _p(state["div"]), _p(state["t"]), _p(state["ps"]), _p(state["tr"]), _p(ph),
                      *[_p(o) for o in outs])
    return outs


def dyn_step_physics(state, phis, tcorh, qcorh, bc, rad, lradsw, j1, j2, dt, alph, rob=0.05, wil=0.53):
    """step with phypar evaluated on level 1 first (dyn_step.f90:45 -> grtend(.., 1, j2)
    -> phypar, dyn_grtend.f90:223-226); rad (phys_state()) is updated in place."""
    tend = phypar_grid(*phys_inputs(state, phis), bc, rad, lradsw)
    return dyn_step(state, phis, tcorh, qcorh, tend.reshape(4, KX, IL, IX), j1, j2, dt, alph, rob, wil)


def phys_state():
    """Radiation state kept between physics calls: tau2 (4, kx, ngp), stratc
    (2, ngp), tt_rsw (kx, ngp), ssrd (ngp)."""
    return {"tau2": np.zeros((4, KX, NGP)), "stratc": np.zeros((2, NGP)), "tt_rsw": np.zeros((KX, NGP)),
            "ssrd": np.zeros(NGP)}


# The branch census of orc_phys_column (the CEN_* enum of speedy_oracle_phys.c, in
# order): what each column decided; -1 = the decision was not reached.
CENSUS = ("cnv_psg", "cnv_ktop1", "cnv_ktop2", "cnv_lqthr", "cnv_itop", "cnv_precnv", "cnv_fqmax", "cnv_fpsa",
          "cnv_delq", "lsc_levels", "lsc_dqmax", "cld_rhnl1", "cld_strtop", "cld_itoplt", "cld_icltop",
          "cld_cl1cap", "cld_pr1cap", "cld_abscl2", "cld_fst", "lw_cold", "lw_hot", "lw_tshot", "sfl_tgrad",
          "sfl_dthl", "sfl_dths", "sfl_evap1", "sfl_evap2n", "vdi_shc", "vdi_qdif", "vdi_dryadj", "qclip",
          "cld_clccap")


def phypar_grid(ug1, vg1, tg1, qg1, phig1, pslg1, bc, state, lradsw, census=False):
    """phypar's physics tendencies (4, kx, ngp) = u, v, t, q from grid inputs
    (kx, ngp) / (ngp,); bc: dict of PHYS_BC arrays (ngp,); state updated in place.
    census=True: returns (tendencies, int32 (ngp, len(CENSUS)) branch census)."""
    phys_init()
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    bcs = np.ascontiguousarray(np.stack([np.asarray(bc[k], dtype=np.float64).ravel() for k in PHYS_BC]))
    tend = np.zeros((4, KX, NGP))
    ins = [f(x) for x in (ug1, vg1, tg1, qg1, phig1, pslg1)]
    if census:
        assert lib().orc_phys_census_size() == len(CENSUS)
        cen = np.zeros((NGP, len(CENSUS)), dtype=np.int32)
        lib().orc_phypar_grid_census(*[_p(x) for x in ins], _p(bcs), _p(state["tau2"]), _p(state["stratc"]),
                                     _p(state["tt_rsw"]), _p(state["ssrd"]), int(bool(lradsw)), _p(tend), _p(cen))
        return tend, cen
    lib().orc_phypar_grid(*[_p(x) for x in ins], _p(bcs), _p(state["tau2"]), _p(state["stratc"]),
                          _p(state["tt_rsw"]), _p(state["ssrd"]), int(bool(lradsw)), _p(tend))
    return tend


# ---------------------------------------------------------------- per-window forcing
CLIMATOLOGY = ("stl12", "snowd12", "soilw12", "sst12", "sice12")


def _leap(y):
    return (y % 4 == 0 and y % 100 != 0) or y % 400 == 0


def calendar_delta_hour(startyear, hours, state):
    """get_current_time_delta_hour (mod_calendar.f90:24-92), statement by statement:
    (year, month, day, hour) after `hours` from startyear; state["ncal"] is the
    routine's SAVEd month table (February set to 29 once a leap year is met)."""
    years = hours // 8760
    year = years + startyear
    leap_days = sum(1 for i in range(years) if _leap(startyear + i))
    ncal = state.setdefault("ncal", [31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31])
    if _leap(year):
        ncal[1] = 29
    c = (hours % 8760) // 24 - leap_days
    month = 1
    while c > 0:
        c -= ncal[month - 1]
        month += 1
    month -= 1
    if month <= 0:
        month = 12
        year -= 1
    return year, month, ncal[month - 1] + c, hours % 24


def newdate(imonth, iday):
    """newdate(0), iseasc = 1 (mod_date.f90:17-79): (tmonth, tyear)."""
    tm, ty = np.zeros(1), np.zeros(1)
    lib().orc_newdate(int(imonth), int(iday), _p(tm), _p(ty))
    return float(tm[0]), float(ty[0])


def forint(imon, fmon, for12):
    out = np.zeros(NGP)
    lib().orc_forint(int(imon), float(fmon), _p(np.ascontiguousarray(for12, dtype=np.float64)), _p(out))
    return out


def forin5(imon, fmon, for12):
    out = np.zeros(NGP)
    lib().orc_forin5(int(imon), float(fmon), _p(np.ascontiguousarray(for12, dtype=np.float64)), _p(out))
    return out


def coupler(imonth, iday, clim):
    """ini_coupler(2) at the date (cpl_land.f90, cpl_sea.f90; icland 1, icsea 0,
    icice 1): dict stl_am, snowd_am, soilw_am, sst_am (ice-blended), sice_am, tice_am.
    clim: dict of CLIMATOLOGY (12, ngp) arrays."""
    c = np.ascontiguousarray(np.stack([np.asarray(clim[k], dtype=np.float64).reshape(12, NGP)
                                       for k in CLIMATOLOGY]))
    names = ("stl_am", "snowd_am", "soilw_am", "sst_am", "sice_am", "tice_am")
    out = {k: np.zeros(NGP) for k in names}
    lib().orc_coupler(int(imonth), int(iday), _p(c), *[_p(out[k]) for k in names])
    return out


def fordate(tyear, surf, phis0, stl_am, sst_am, sice_am, snowd_am=None, snowc=None):
    """fordate(0) (ini_fordate.f90:1-115): dict snowc, alb_l, alb_s, albsfc, fsol,
    ozone, ozupp, zenit, stratz (ngp,) and tcorh, qcorh complex (nx, mx).
    surf: dict fmask_l, fmask_s, alb0.  Without snowd_am, snowc is the input."""
    phys_init()
    f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel())  # noqa: E731
    sc = f(snowc) if snowd_am is None else np.zeros(NGP)
    out = {k: np.zeros(NGP) for k in ("alb_l", "alb_s", "albsfc")}
    sol = np.zeros((5, NGP))
    tq = [np.zeros((NX, MX), np.complex128) for _ in range(2)]
    ins = [f(surf["fmask_l"]), f(surf["fmask_s"]), f(surf["alb0"]), f(phis0), f(stl_am), f(sst_am)]
    sn = None if snowd_am is None else f(snowd_am)
    lib().orc_fordate(float(tyear), *[_p(x) for x in ins], None if sn is None else _p(sn), _p(f(sice_am)), _p(sc),
                      _p(out["alb_l"]), _p(out["alb_s"]), _p(out["albsfc"]), _p(sol), _p(tq[0]), _p(tq[1]))
    out["snowc"] = sc
    out.update(zip(("fsol", "ozone", "ozupp", "zenit", "stratz"), sol))
    out["tcorh"], out["qcorh"] = tq
    return out


def window_forcing(imonth, iday, surf, bc, clim=None, sice=None, tice=None, sst_hybrid=None, bias=0.0):
    """The whole per-window forcing as sml_dyn_fordate applies it: the coupler at the
    date (clim) or bc's coupler fields, ini_sea's hybrid SST, fordate.  Returns
    (bc', tcorh, qcorh, sice, tice) with bc' the boundary fields of the window."""
    b = {k: np.array(v, dtype=np.float64, copy=True).ravel() for k, v in bc.items()}
    snowd = None
    if clim is not None:
        c = coupler(imonth, iday, clim)
        b["stl_am"], b["soilw_am"], snowd = c["stl_am"], c["soilw_am"], c["snowd_am"]
        sst_cpl, sice, tice = c["sst_am"], c["sice_am"], c["tice_am"]
    else:  # bc's sst_am is the coupler's (sml_dyn_set_physics)
        sst_cpl = b["sst_am"]
        sice = np.zeros(NGP) if sice is None else np.asarray(sice, dtype=np.float64).ravel()
        tice = np.zeros(NGP) if tice is None else np.asarray(tice, dtype=np.float64).ravel()
    b["sst_am"] = sst_cpl if sst_hybrid is None else hybrid_sst_am(sst_cpl, sst_hybrid, sice, tice, bias)
    _, tyear = newdate(imonth, iday)
    fd = fordate(tyear, surf, b["phis0"], b["stl_am"], b["sst_am"], sice, snowd_am=snowd,
                 snowc=None if snowd is not None else b["snowc"])
    for k in ("snowc", "alb_l", "alb_s", "albsfc", "fsol", "ozone", "ozupp", "zenit", "stratz"):
        b[k] = fd[k]
    return b, fd["tcorh"], fd["qcorh"], sice, tice


# ---------------------------------------------------------------- reference (pinning only)
def ref_spectral():
    """ctypes handle on the reference's own spectral Fortran (oracle/_ref), or None."""
    if not os.path.exists(REF_SPECTRAL_PATH):
        return None
    return ctypes.CDLL(REF_SPECTRAL_PATH)
