"""Seeded physics inputs that reach every branch of phypar's column physics, with the
oracle's branch census (oracle.phypar_grid(..., census=True)) to prove it.  NumPy and
the oracle only: the CPU tests check the fixtures (tests/test_oracle_physics_edges.py),
the GPU tests run the kernels on them (tests/test_physics_edges_gpu.py).

Two fixtures:

 * direct(): grid inputs (ug1, vg1, tg1, qg1, phig1, pslg1) and boundary fields for all
   4608 columns, as two input sets A and B for a shortwave call followed by a
   longwave-only call on A's radiation state.  Bands of latitude rows of a synthetic
   state are overwritten with per-column random draws (low surface pressure, cold top,
   hot surface, super-adiabatic layers, negative humidity, nint ties, ...).  B has the
   bands on other rows, so every column's longwave-only call reads a radiation state
   that another kind of column made.
 * state(): two spectral states S_A, S_B (oracle.spec of smooth crafted grid fields)
   for the reference's own phypar and the step kernels, with their boundary fields.

Rules of both: temperatures stay within 150..350 K (the reference and the oracle index
fband(100:400) without a clamp), and no threshold is set exactly on a computed value
(exp differs by an ulp between libms); exact values are only given to inputs that the
physics compares as they are (q = 0, fmask1 = 0 or 1, soilw_am = 0, equal
temperatures, T = n + 0.5).
"""
import os

import numpy as np

import oracle

NGP, KX, IL, IX = oracle.NGP, oracle.KX, oracle.IL, oracle.IX
CEN = {k: i for i, k in enumerate(oracle.CENSUS)}
INS = ("ug1", "vg1", "tg1", "qg1", "phig1", "pslg1")

# Every state of every census entry that a fixture must reach (-1, "not reached", is
# never required).  Bit entries: every listed bit must occur set and clear.
STATES = {
    "cnv_psg": (0, 1), "cnv_ktop1": (0, 1), "cnv_ktop2": (0, 1), "cnv_lqthr": (0, 1),
    "cnv_itop": (3, 4, 5, 9), "cnv_precnv": (0, 1), "cnv_fqmax": (0, 1), "cnv_fpsa": (0, 1),
    "cnv_delq": (0, 1), "lsc_dqmax": (0, 1), "cld_rhnl1": (0, 1), "cld_strtop": (3, 4, 5, 6, 7, 9),
    "cld_itoplt": (0, 1), "cld_icltop": (2, 3, 4, 5, 6, 7, 9), "cld_cl1cap": (0, 1), "cld_pr1cap": (0, 1),
    "cld_abscl2": (0, 1), "cld_fst": (0, 1, 2), "cld_clccap": (0, 1), "lw_cold": (0, 1), "lw_hot": (0, 1),
    "lw_tshot": (0, 1), "sfl_tgrad": (0, 1), "sfl_dthl": (0, 1, 2, 3), "sfl_dths": (0, 1, 2, 3),
    "sfl_evap1": (0, 1), "sfl_evap2n": (0, 1), "vdi_shc": (0, 1, 2, 3, 4, 5), "qclip": (0, 1),
}
BITS = {"lsc_levels": tuple(range(2, 9)), "vdi_qdif": (5, 6), "vdi_dryadj": tuple(range(1, 8))}
# hydrostatic phi would need T near 140 K for these: not asked of the state fixture
STATE_FIXTURE_EXEMPT = {("vdi_dryadj", 1), ("vdi_dryadj", 2)}

SIG = 0.5 * (oracle.HSG[1:] + oracle.HSG[:-1])
CP = 1004.0


def golden(name):
    from conftest import REPO

    return dict(np.load(os.path.join(REPO, "tests", "golden", name)))


def qsat(ta, ps, sig):
    """shtorh's saturation specific humidity (g/kg), for placing humidity bands."""
    e0, c1, c2, t0, t1, t2 = 6.108e-3, 17.269, 21.875, 273.16, 35.86, 7.66
    q = np.where(ta >= t0, e0 * np.exp(c1 * (ta - t0) / (ta - t1)), e0 * np.exp(c2 * (ta - t0) / (ta - t2)))
    return 622.0 * q / (sig * ps - 0.378 * q)


def coverage(cens):
    """{(entry, state): number of columns} over a list of census arrays; bit entries
    as (entry, k) for set and (entry, -k) for clear."""
    out = {}
    for name, states in STATES.items():
        col = np.concatenate([c[:, CEN[name]] for c in cens])
        for s in states:
            out[(name, s)] = int((col == s).sum())
    for name, bits in BITS.items():
        col = np.concatenate([c[:, CEN[name]] for c in cens])
        for k in bits:
            out[(name, k)] = int(((col >> k) & 1 == 1).sum())
            out[(name, -k)] = int(((col >> k) & 1 == 0).sum())
    return out


def describe(cen_row):
    """One column's census as text, for assertion messages."""
    return ", ".join(f"{k}={int(v)}" for k, v in zip(oracle.CENSUS, cen_row))


def perturb(rng, a, ulps=2):
    """`a` moved by up to +-ulps ulp of its level's largest magnitude (last axis = columns)."""
    a = np.asarray(a, dtype=np.float64)
    scale = np.spacing(np.abs(a).max(axis=-1, keepdims=True))
    return a + rng.integers(-ulps, ulps + 1, a.shape) * scale


def near_tie(tg, tol=1e-6):
    """Columns with a temperature within tol of a nint tie (n + 0.5)."""
    return (np.abs(np.abs(tg - np.floor(tg)) - 0.5) < tol).any(axis=0)


# ------------------------------------------------------------------ direct fixture
DIRECT_SEED = 31
NBAND, BAND_ROWS = 16, 3


def _direct_set(pg, seed, shift):
    from speedy_ml_amd.synthetic import dyn_state
    from test_oracle_physics import _bc

    st, forcing = dyn_state(seed)
    ug, vg, tg, qg, phig, psl = [np.array(x) for x in oracle.phys_inputs(oracle.dyn_state_copy(st), forcing["phis"])]
    bc = {k: np.array(v, dtype=np.float64).copy() for k, v in _bc(pg).items()}
    rng = np.random.default_rng(1000 + seed)
    row = np.repeat(np.arange(IL), IX)
    band_of = ((row + shift) % IL) // BAND_ROWS

    def band(b):
        m = band_of == b
        return m, int(m.sum())

    U = rng.uniform
    m, n = band(0)  # high ground: no convection
    psl[m] = np.log(U(0.55, 0.80, n))
    m, n = band(1)  # the fpsa ramp
    psl[m] = np.log(U(0.80, 0.90, n))
    m, n = band(2)  # cold top: fband rows below 200 K
    tg[0][m] = U(182.0, 205.0, n)
    tg[1][m] = U(182.0, 205.0, n)
    m, n = band(3)  # hot surface and lowest levels: fband rows above 320 K
    tg[7][m] = U(312.0, 335.0, n)
    tg[6][m] = U(312.0, 335.0, n)
    bc["stl_am"][m] = U(318.0, 340.0, n)
    bc["sst_am"][m] = U(300.0, 325.0, n)
    m, n = band(4)  # one super-adiabatic layer k | k+1 per column, k = 1..7 (phi is an input here)
    k = rng.integers(1, 8, n)
    cols = np.flatnonzero(m)
    dphi = U(1000.0, 5000.0, n)
    phig[k - 1, cols] = phig[k, cols] + dphi
    tg[k - 1, cols] = tg[k, cols] - 0.9 * dphi / CP - U(1.0, 8.0, n)
    m, n = band(5)  # q exactly 0 and negative
    r = rng.random((KX, n))
    qg[:, m] = np.where(r < 0.3, 0.0, np.where(r < 0.6, -rng.random((KX, n)), qg[:, m]))
    qg[rng.integers(0, KX, n), np.flatnonzero(m)] = -rng.random(n) - 0.01  # at least one negative level each
    m, n = band(6)  # nint ties
    tg[:, m] = np.round(tg[:, m]) + 0.5
    m, n = band(7)  # dry: no cloud
    qg[:, m] *= U(0.005, 0.05, n)
    m, n = band(8)  # all sea
    bc["fmask1"][m] = 0.0
    m, n = band(9)  # all land, dry soil
    bc["fmask1"][m] = 1.0
    bc["soilw_am"][m] = 0.0
    m, n = band(10)  # surface air colder than the level above; in 6 columns ta(nlev) == ta(nl1) exactly
    tg[7][m] = tg[6][m] - U(0.5, 10.0, n)
    cols = np.flatnonzero(m)[:6]
    tg[7][cols] = tg[6][cols]
    m, n = band(11)  # one level around saturation per column, others dry: lscond level by level
    k = rng.integers(1, KX, n)
    cols = np.flatnonzero(m)
    ps = np.exp(psl[cols])
    qg[:, cols] *= 0.3
    qg[k, cols] = qsat(tg[k, cols], ps, SIG[k]) * U(0.85, 1.6, n)
    m, n = band(12)  # moist, warm boundary layer under a cool dry mid-troposphere: deep convection
    tg[7][m] += U(0.0, 12.0, n)
    tg[6][m] += U(0.0, 8.0, n)
    ps = np.exp(psl[m])
    qg[7][m] = qsat(tg[7][m], ps, SIG[7]) * U(0.6, 1.05, n)
    qg[6][m] = qsat(tg[6][m], ps, SIG[6]) * U(0.3, 1.05, n)
    for kk in (2, 3, 4, 5):
        tg[kk][m] -= U(0.0, 10.0, n)
        qg[kk][m] *= U(0.0, 1.5, n)
    m, n = band(13)  # cloud at one chosen level 3..7 per column; surface warmer or colder than the air
    k = rng.integers(2, 7, n)
    cols = np.flatnonzero(m)
    ps = np.exp(psl[cols])
    qg[:, cols] *= U(0.02, 0.4, n)
    tg[2, cols] = np.where(k == 2, U(236.0, 250.0, n), tg[2, cols])  # warm enough for q > qacl below saturation
    qg[k, cols] = qsat(tg[k, cols], ps, SIG[k]) * U(0.4, 0.85, n)
    bc["stl_am"][m] = tg[7][m] + U(-12.0, 12.0, n)
    bc["sst_am"][m] = tg[7][m] + U(-12.0, 12.0, n)
    m, n = band(14)  # convection that reaches a warm, dry layer and does not precipitate (precnv clipped at 0):
    # a saturated boundary layer (the lqthr entry) under levels 5 and 6 as warm as the surface air, their
    # geopotential set low enough for the saturation moist static energy to stay below the surface air's
    ps = np.exp(psl[m])
    qg[7][m] = qsat(tg[7][m], ps, SIG[7]) * U(0.92, 1.0, n)
    qg[6][m] = qsat(tg[6][m], ps, SIG[6]) * U(0.92, 1.0, n)
    mss8 = CP * tg[7][m] + phig[7][m] + 2501.0 * qsat(tg[7][m], ps, SIG[7])
    for kk in (4, 5):
        tg[kk][m] = tg[7][m] + U(-3.0, 6.0, n)
        phig[kk][m] = mss8 - U(500.0, 5000.0, n) - CP * tg[kk][m] - 2501.0 * qsat(tg[kk][m], ps, SIG[kk])
        qg[kk][m] *= U(0.0, 0.3, n)
    return {"ins": [ug, vg, tg, qg, phig, psl], "bc": bc}


_cache = {}


def direct():
    """{"A": {"ins", "bc"}, "B": ...}: built once, never modified by the tests."""
    if "direct" not in _cache:
        pg = golden("phys_ref.npz")
        _cache["direct"] = {"A": _direct_set(pg, DIRECT_SEED, 0), "B": _direct_set(pg, DIRECT_SEED + 1, 20)}
    return _cache["direct"]


def run_sequence(sets, perturb_seed=None):
    """The oracle on set A with lradsw, then on B without, on A's radiation state.
    Returns [(tend, census, rad-after-call)], inputs perturbed when a seed is given."""
    rad = oracle.phys_state()
    out = []
    rng = None if perturb_seed is None else np.random.default_rng(perturb_seed)
    for s, lradsw in zip(sets, (True, False)):
        ins = s["ins"] if rng is None else [perturb(rng, x) for x in s["ins"]]
        tend, cen = oracle.phypar_grid(*ins, s["bc"], rad, lradsw, census=True)
        out.append((tend, cen, {k: v.copy() for k, v in rad.items()}))
    return out


PERTURB_SEEDS = (101, 102, 103, 104, 105)


def fragility(sets):
    """(base runs, fragile[ncall][ngp] bool, floor[ncall][4][kx]): columns whose census
    changes under any of the 5 perturbed draws, and per (variable, level) the largest
    change of the tendency over the other columns / that level's maximum."""
    if ("frag", id(sets[0])) in _cache:
        return _cache[("frag", id(sets[0]))]
    base = run_sequence(sets)
    draws = [run_sequence(sets, s) for s in PERTURB_SEEDS]
    fragile = []
    for c in range(len(base)):
        f = np.zeros(NGP, bool)
        for d in draws:
            f |= (d[c][1] != base[c][1]).any(axis=1)
        fragile.append(f)
    # the longwave-only call reads the state the shortwave call made in the same column
    fragile[1] = fragile[1] | fragile[0]
    _cache[("frag", id(sets[0]))] = (base, fragile, draws)
    return _cache[("frag", id(sets[0]))]


def level_rel(got, ref, keep=None):
    """max |got - ref| over the kept columns / max |ref| of the level, per leading index."""
    got, ref = np.asarray(got), np.asarray(ref)
    den = np.abs(ref).max(axis=-1)
    if keep is not None:
        got, ref = got[..., keep], ref[..., keep]
    return np.abs(got - ref).max(axis=-1) / np.where(den > 0, den, 1.0)


def floor_table(base, draws, exclude):
    """[ncall][4][kx]: noise floor of the tendencies (see fragility)."""
    out = []
    for c in range(len(base)):
        keep = ~exclude[c]
        out.append(np.max([level_rel(d[c][0], base[c][0], keep) for d in draws], axis=0))
    return np.array(out)


def noise_floor(sets):
    """floor_table over the columns that are neither fragile nor within 1e-6 K of a nint
    tie (a tie moved by an ulp changes the fband row: 1.4e-3 of a level's maximum)."""
    base, fragile, draws = fragility(sets)
    return floor_table(base, draws, [f | near_tie(s["ins"][2]) for f, s in zip(fragile, sets)])


def level_bounds(sets, tol):
    """[ncall][4][kx] bound on the per-level norm: tol, or 8 x the level's noise floor
    where that floor is above tol / 8."""
    floor = noise_floor(sets)
    return np.where(floor > tol / 8, 8.0 * floor, tol)


# ------------------------------------------------------------------ state fixture
STATE_SEED = 9
RD = 287.0
SEL = np.arange(NGP)[np.arange(NGP) % 4 == 0]  # the columns the golden stores: every 4th longitude


def _grid(c):
    return oracle.grid(np.ascontiguousarray(c, dtype=np.complex128).view(np.float64))


def _spec(g):
    return oracle.spec(g).view(np.complex128)


HUM_T = (280.0, 280.0, 310.0, 320.0, 318.5, 325.5, 316.0, 334.0)
HUM_RH = (0.2, 0.2, 0.2, 0.2, 0.2, 0.1, 0.95, 0.95)


def _bump(lat0, lon0, width):
    """exp(-(d / width)^2) of the great-circle distance d to (lat0, lon0), degrees: (il, ix)."""
    lat = oracle.radang()[:, None]
    lon = (np.arange(IX) * 2 * np.pi / IX)[None, :]
    la0, lo0 = np.deg2rad(lat0), np.deg2rad(lon0)
    c = np.sin(lat) * np.sin(la0) + np.cos(lat) * np.cos(la0) * np.cos(lon - lo0)
    return np.exp(-(np.rad2deg(np.arccos(np.clip(c, -1.0, 1.0))) / width) ** 2)


def _state_set(pg, seed, rot):
    """One spectral state with its forcing and boundary fields; the features sit `rot`
    degrees of longitude further east (S_B against S_A)."""
    from speedy_ml_amd.synthetic import dyn_state
    from test_oracle_physics import _bc

    st, forcing = dyn_state(seed)
    st = oracle.dyn_state_copy(st)
    bc = {k: np.array(v, dtype=np.float64).copy() for k, v in _bc(pg).items()}
    tg = np.stack([_grid(st["t"][0, k]) for k in range(KX)])
    qg = np.stack([_grid(st["tr"][0, k]) for k in range(KX)])
    lnps = _grid(st["ps"][0])
    phis0 = _grid(forcing["phis"])
    B = lambda lat0, lon0, w: _bump(lat0, lon0 + rot, w)  # noqa: E731

    # a polar cap and a plateau with psg near 0.6, on orography that balances them
    high = np.minimum(1.0, 1.15 * B(-90.0, 0.0, 24.0)) + np.minimum(1.0, 1.15 * B(35.0, 90.0, 17.0))
    lnps = lnps - 0.52 * high
    phis0 = phis0 + RD * 262.0 * 0.52 * high
    # a cold top
    cold = B(0.0, 180.0, 26.0)
    tg[0] -= 21.0 * cold
    tg[1] -= 18.0 * cold
    # a hot surface with hot lowest levels
    hot = np.minimum(1.0, 1.2 * B(20.0, 0.0, 18.0))
    for k, a in enumerate((0.0, 0.0, 0.0, 4.0, 12.0, 27.0, 47.0, 44.0)):
        tg[k] += a * hot
    stl = bc["stl_am"].reshape(IL, IX) + 50.0 * hot
    sst = bc["sst_am"].reshape(IL, IX) + 30.0 * hot
    # a dry region
    qg *= 1.0 - 1.03 * B(-32.0, 270.0, 20.0)
    # a very hot, saturated boundary layer on a moist adiabat up to level 5 under a warm dry cap: hydrostatic
    # columns convect without precipitating (precnv clipped at 0) only with surface air above about 331 K
    hum = np.minimum(1.0, 1.3 * B(55.0, 250.0, 20.0))
    for k, a in enumerate(HUM_T):
        tg[k] += hum * (a + 0.2 * (tg[k] - tg[k].mean()) - tg[k])
    # saturated regions, one level each
    ps = np.exp(lnps)
    for k, f in enumerate(HUM_RH):
        qg[k] += hum * (f * qsat(tg[k], ps, SIG[k]) - qg[k])
    for k in range(1, KX):
        w = np.minimum(1.0, 1.3 * B(-20.0 + 8.0 * (k % 3), 100.0 + 45.0 * k, 11.0))
        if k == 2:
            tg[k] += 26.0 * w  # warm enough for q > qacl below saturation
        qg[k] += w * (1.35 * qsat(tg[k], ps, SIG[k]) - qg[k])
    bc["stl_am"], bc["sst_am"] = stl.ravel(), sst.ravel()
    for k in range(KX):
        st["t"][1, k] += _spec(tg[k]) - st["t"][0, k]
        st["t"][0, k] = _spec(tg[k])
        st["tr"][1, k] += _spec(qg[k]) - st["tr"][0, k]
        st["tr"][0, k] = _spec(qg[k])
    st["ps"][1] += _spec(lnps) - st["ps"][0]
    st["ps"][0] = _spec(lnps)
    forcing = dict(forcing, phis=_spec(phis0))
    bc["phis0"] = _grid(forcing["phis"]).ravel()
    bc["forog"] = oracle.sflset(bc["phis0"])
    ins = oracle.phys_inputs(st, forcing["phis"])
    return {"state": st, "forcing": forcing, "bc": bc, "ins": ins}


def state():
    """{"A": {"state", "forcing", "bc", "ins"}, "B": ...}; "ins" = oracle.phys_inputs of
    the state: what the physics sees after truncation."""
    if "state" not in _cache:
        pg = golden("phys_ref.npz")
        _cache["state"] = {"A": _state_set(pg, STATE_SEED, 0.0), "B": _state_set(pg, STATE_SEED + 1, 140.0)}
    return _cache["state"]


def state_sets():
    s = state()
    return [s["A"], s["B"]]
