"""Generate tests/golden/dyn_edges_*.npz from the reference's own dynamical core, on a
"white" state that loads every wavenumber of the T30 triangle alike.

Run in the survey/build container (needs /root/reference and flang):

    make -C oracle ref          # builds oracle/_ref/libspeedy_ref_dyn.so
    python tests/golden/make_dyn_edges_golden.py

Same driver as make_dyn_golden.py (its Ref class, initialisation, surface forcing and
physics call are reused), another state and one more case.  dyn_ref.npz's spectra decay
as (1 + m + n)^-1 or ^-1.5 around a large mean, so a relative error of 1e-9 in a
coefficient at the truncation edge is 1e-12 of the field's maximum and passes; here the
outputs are compared wave by wave (tests/_dyn_measure.py).

Input state, inputs() (pure numpy, rebuilt from SEED wherever it is needed, not stored):

 - vor, div, t, tr on each of the 8 levels and ps: every coefficient of the triangle
   (m + n <= 30) is amp x a seeded complex normal value, m = 0 real, (0,0) the mean of
   make_dyn_golden.py (tref for t, 12 fsg^3 for tr, 0 else).  One amplitude per field
   and level, AMP[f] x (1 - k/32) (tr: of its level mean), no decay with wavenumber: a
   mix-up of levels changes the numbers.
 - lift_rows(): t and tr sit on a mean 10^3 to 10^4 times the admissible white
   amplitude (the grid image of t has to stay inside 160..330 K, which caps the
   amplitude near 0.3 K where the floor of the measure, 1e-3 of the level's maximum, is
   0.3 to 0.4 K), so chance leaves the largest coefficient of a short row (m = 30 is one
   coefficient) under that floor, or one step moves it there.  Where the largest
   coefficient of a row of level 1 is under NEAR x the floor it is scaled, phase kept, to
   LIFT x the floor.  The rule is applied to every field, level and row; it fires on 124
   rows of t and 4 of tr (whose physics tendencies move a coefficient by several floors
   in a step, hence LIFTS["tr"]).  Everything else stays as drawn.
 - time level 2 = level 1 + a white perturbation of 1e-3 of the amplitude.
 - phis, tcorh, qcorh: those of dyn_ref.npz plus FORCING_EDGE at n = 0 and n = 30 - m
   of every m ((0,0) left alone), as make_spec_kernel.py's edge variant loads a state;
   sst, stl, fmask1: those of dyn_ref.npz.

Checked here, on the reference alone (main() asserts each):

 - the grid images of level 1 lie inside the iogrid safety ranges |u| < 150, |v| < 120,
   160 < T < 330 (uvspec + grid(kcos = 2), grid(kcos = 1) of the reference);
 - phypar on it (geop(1), lradsw off) is finite and repeats bit for bit;
 - every output is finite; level 1 is unchanged where j1 = 1;
 - outside the triangle every output is exactly zero, and so are the imaginary parts
   of m = 0 of level 2 -- the zero masks are stored, not assumed;
 - the measure's floor is active on no row of any state output.

Cases, each from that state after impint(dt, alph):

    fwd    step(1,1, delt/2, 0.5, ROB, WIL)
    lf0    step(1,2, delt,   0.5, ROB, WIL)
    lf     step(2,2, 2 delt, 0.5, ROB, WIL)     (+ phi = geop(j4))
    expl   step(1,1, delt/2, 0.0, ROB, WIL)
    lf_rw  step(2,2, 2 delt, 0.75, 0.1, 0.3)    every parameter off its default

Files (each under 1 MiB): dyn_edges_j1.npz (fwd, lf0, expl: level 2), dyn_edges_lf.npz,
dyn_edges_lf_rw.npz (both levels), dyn_edges_phys.npz (P = u, v, t, q tendencies of
phypar on level 1, the same for every case).  Each stores, beside an output, the packed
mask of its exactly zero real and imaginary parts (<name>_zero).
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from make_dyn_golden import DELT, IL, IX, KX, MX, NX, ROB, WIL, Ref, _dbl, _int, _p  # noqa: E402

SEED = 20251020
FIELDS = ("vor", "div", "t", "tr", "ps")
# white amplitude per real and imaginary part on the top level; tr: as a fraction of the
# level mean.  Chosen so that the reference's own grid images stay inside the iogrid
# ranges with room to spare (main() prints the extremes).
AMP = {"vor": 8e-7, "div": 2e-7, "t": 0.32, "tr": 1e-2, "ps": 1e-3}
PERT = 1e-3       # time level 2 - time level 1, as a fraction of the amplitude
FLOOR = 1e-3      # the measure's floor (tests/_dyn_measure.py), a share of the level maximum
# lift_rows(): a row under NEAR x the floor gets LIFT x the floor; (NEAR, LIFT) per field
LIFTS = {"tr": (6.0, 8.0)}
NEAR, LIFT = 2.0, 3.0
FORCING_EDGE = {"phis": 300.0, "tcorh": 0.3, "qcorh": 0.03}
CASES = {"fwd": (1, 1, 0.5 * DELT, 0.5, ROB, WIL), "lf0": (1, 2, DELT, 0.5, ROB, WIL),
         "lf": (2, 2, 2 * DELT, 0.5, ROB, WIL), "expl": (1, 1, 0.5 * DELT, 0.0, ROB, WIL),
         "lf_rw": (2, 2, 2 * DELT, 0.75, 0.1, 0.3)}
FILES = {"j1": ("fwd", "lf0", "expl"), "lf": ("lf",), "lf_rw": ("lf_rw",)}

HSG = np.array([0.000, 0.050, 0.140, 0.260, 0.420, 0.600, 0.770, 0.900, 1.000])
FSG = 0.5 * (HSG[1:] + HSG[:-1])
TRI = (np.arange(NX)[:, None] + np.arange(MX)[None, :]) <= 30  # (n, m): inside the triangle


def path(name: str) -> str:
    return os.path.join(HERE, f"dyn_edges_{name}.npz")


def white(rng, amp, mean=0.0):
    """complex (nx, mx): amp x complex normal on the triangle, m = 0 real, (0,0) the mean."""
    c = np.zeros((NX, MX), np.complex128)
    c[TRI] = (rng.standard_normal(TRI.sum()) + 1j * rng.standard_normal(TRI.sum())) * amp
    c[:, 0] = c[:, 0].real
    c[0, 0] = mean * np.sqrt(2.0)  # P_00 = sqrt(1/2)
    return c


def lift_rows(c, near=NEAR, lift=LIFT):
    """Where the largest |coefficient| of a row m is under near x FLOOR x the level's
    maximum, scale it to lift x that floor (in place); returns the rows lifted."""
    a = np.abs(c)
    floor = FLOOR * a.max()
    rows = []
    for m in range(MX):
        n = int(np.argmax(a[:MX - m, m]))
        if 0.0 < a[n, m] < near * floor:
            c[n, m] *= lift * floor / a[n, m]
            rows.append(m)
    return rows


def inputs():
    """The white state and its forcing: vor/div/t/tr (2, kx, nx, mx), ps (2, nx, mx),
    phis/tcorh/qcorh (nx, mx), sst/stl/fmask1 (ngp,), lifted = [(field, level, m)]."""
    rng = np.random.default_rng(SEED)
    rgam = (2.0 / 7.0) * 1004.0 * 6.0 / (1000.0 * 9.81)
    tref = 288.0 * np.maximum(0.2, FSG) ** rgam
    st = {f: np.zeros((2, KX, NX, MX), np.complex128) for f in FIELDS[:4]}
    st["ps"] = np.zeros((2, NX, MX), np.complex128)
    amp = {f: np.zeros(KX) for f in FIELDS[:4]}
    lifted = []
    for k in range(KX):
        s = 1.0 - k / 32.0
        qm = 12.0 * FSG[k] ** 3
        amp["vor"][k], amp["div"][k], amp["t"][k], amp["tr"][k] = (AMP["vor"] * s, AMP["div"] * s, AMP["t"] * s,
                                                                   AMP["tr"] * s * qm)
        st["vor"][0, k] = white(rng, amp["vor"][k])
        st["div"][0, k] = white(rng, amp["div"][k])
        st["t"][0, k] = white(rng, amp["t"][k], mean=tref[k])
        st["tr"][0, k] = white(rng, amp["tr"][k], mean=qm)
        for f in FIELDS[:4]:
            lifted += [(f, k, m) for m in lift_rows(st[f][0, k], *LIFTS.get(f, (NEAR, LIFT)))]
    st["ps"][0] = white(rng, AMP["ps"])
    lifted += [("ps", -1, m) for m in lift_rows(st["ps"][0])]
    for f in FIELDS[:4]:
        for k in range(KX):
            st[f][1, k] = st[f][0, k] + white(rng, PERT * amp[f][k])
    st["ps"][1] = st["ps"][0] + white(rng, PERT * AMP["ps"])
    base = np.load(os.path.join(HERE, "dyn_ref.npz"))
    out = dict(st)
    for f, a in FORCING_EDGE.items():
        c = base[f].copy()
        for m in range(MX):
            for n in {0, 30 - m}:
                if m == 0 and n == 0:
                    continue
                c[n, m] += a * (1.0 if m == 0 else 1.0 + 1.0j)  # m = 0 is real
        out[f] = c
    for f in ("sst", "stl", "fmask1"):
        out[f] = base[f].copy()
    out["lifted"] = lifted
    return out


def golden():
    """Every fixture file merged into one dict (the zero masks unpacked to bool)."""
    g = {}
    for name in tuple(FILES) + ("phys",):
        g.update(np.load(path(name)))
    for k in [k for k in g if k.endswith("_zero")]:
        ref = g[k[:-5]]
        g[k] = np.unpackbits(g[k])[:2 * ref.size].astype(bool).reshape(ref.shape + (2,))
    return g


def floor_active(ref):
    """(..., nx, mx) complex -> bool (..., mx): rows whose largest coefficient is under
    FLOOR x the level's maximum (the same rule as tests/_dyn_measure.py)."""
    a = np.abs(ref) * TRI
    return a.max(axis=-2) < FLOOR * a.max(axis=(-2, -1))[..., None]


def main():
    R = Ref()
    L = R.L
    x = inputs()
    print("rows lifted:", x["lifted"])
    # 1. initialisation (make_dyn_golden.py)
    L.inifft_()
    L.indyns_()
    hsg = R.var("mod_dyncon1", "hsg", (KX + 1,))
    fsg = R.var("mod_dyncon1", "fsg", (KX,))
    radang = R.var("mod_dyncon1", "radang", (IL,))
    assert np.allclose(hsg, HSG, rtol=0, atol=1e-15) and np.allclose(fsg, FSG, rtol=0, atol=1e-15)
    ppl = np.ascontiguousarray(fsg.copy())
    L.inphys_(_p(hsg), _p(ppl), _p(radang))
    L.radset_()
    R.scalar_logical("mod_lflags", "lradsw", False)

    vor = R.var("mod_dynvar", "vor", (MX, NX, KX, 2), np.complex128)
    div = R.var("mod_dynvar", "div", (MX, NX, KX, 2), np.complex128)
    t = R.var("mod_dynvar", "t", (MX, NX, KX, 2), np.complex128)
    ps = R.var("mod_dynvar", "ps", (MX, NX, 2), np.complex128)
    tr = R.var("mod_dynvar", "tr", (MX, NX, KX, 2, 1), np.complex128)
    phi = R.var("mod_dynvar", "phi", (MX, NX, KX), np.complex128)
    phis = R.var("mod_dynvar", "phis", (MX, NX), np.complex128)
    tcorh = R.var("mod_hdifcon", "tcorh", (MX, NX), np.complex128)
    qcorh = R.var("mod_hdifcon", "qcorh", (MX, NX), np.complex128)

    def load_state():
        vor[...] = x["vor"].transpose(3, 2, 1, 0)
        div[...] = x["div"].transpose(3, 2, 1, 0)
        t[...] = x["t"].transpose(3, 2, 1, 0)
        tr[..., 0] = x["tr"].transpose(3, 2, 1, 0)
        ps[...] = x["ps"].transpose(2, 1, 0)
        phis[...] = x["phis"].T
        tcorh[...] = x["tcorh"].T
        qcorh[...] = x["qcorh"].T

    def grid(c, kcos):
        g = np.zeros((IL, IX))
        L.grid_(_p(np.ascontiguousarray(c).view(np.float64)), _p(g), _int(kcos))
        return g

    # 2. the grid images of level 1 inside the iogrid safety ranges
    ext = np.zeros((KX, 4))
    for k in range(KX):
        uc, vc = np.zeros((NX, MX), np.complex128), np.zeros((NX, MX), np.complex128)
        L.uvspec_(_p(np.ascontiguousarray(x["vor"][0, k])), _p(np.ascontiguousarray(x["div"][0, k])), _p(uc), _p(vc))
        tg = grid(x["t"][0, k], 1)
        ext[k] = np.abs(grid(uc, 2)).max(), np.abs(grid(vc, 2)).max(), tg.min(), tg.max()
    print("level 1 grid images, per level: max |u|, max |v|, min T, max T\n", ext.round(1))
    assert ext[:, 0].max() < 150.0 and ext[:, 1].max() < 120.0 and ext[:, 2].min() > 160.0 and ext[:, 3].max() < 330.0

    # 3. surface forcing and the physics tendencies of level 1 (make_dyn_golden.py)
    ngp = IX * IL
    load_state()
    phis0 = R.var("mod_surfcon", "phis0", (IX, IL))
    g = grid(x["phis"], 1)
    phis0[...] = g.T
    R.var("mod_surfcon", "fmask1", (IX, IL))[...] = x["fmask1"].reshape(IL, IX).T
    L.sflset_(_p(np.ascontiguousarray(g)))
    R.var("mod_var_sea", "sst_am", (ngp,))[...] = x["sst"]
    R.var("mod_var_sea", "ssti_om", (ngp,))[...] = x["sst"]
    R.var("mod_var_land", "stl_am", (ngp,))[...] = x["stl"]
    R.var("mod_var_land", "soilw_am", (ngp,))[...] = 0.4
    R.var("mod_radcon", "alb_l", (ngp,))[...] = 0.25
    R.var("mod_radcon", "alb_s", (ngp,))[...] = 0.07
    R.var("mod_radcon", "snowc", (ngp,))[...] = 0.0

    def physics():
        load_state()
        L.geop_(_int(1))
        tend = [np.zeros((KX, IL, IX)) for _ in range(4)]
        L.phypar_(_p(vor), _p(div), _p(t), _p(tr), _p(phi), _p(ps), *[_p(a) for a in tend])
        return np.stack(tend)

    phys = physics()
    assert np.array_equal(phys, physics()), "reference physics is not repeatable"
    assert np.all(np.isfinite(phys))

    # 4. the cases
    out = {name: {} for name in FILES}
    active = []
    for name, members in FILES.items():
        for case in members:
            j1, j2, dt, alph, rob, wil = CASES[case]
            load_state()
            L.impint_(_dbl(dt), _dbl(alph))
            L.step_(_int(j1), _int(j2), _dbl(dt), _dbl(alph), _dbl(rob), _dbl(wil))
            res = {"vor": vor.transpose(3, 2, 1, 0).copy(), "div": div.transpose(3, 2, 1, 0).copy(),
                   "t": t.transpose(3, 2, 1, 0).copy(), "tr": tr[..., 0].transpose(3, 2, 1, 0).copy(),
                   "ps": ps.transpose(2, 1, 0).copy()}
            levels = [0, 1] if j1 == 2 else [1]
            if case == "lf":
                res["phi"] = phi.transpose(2, 1, 0).copy()
            for f, a in res.items():
                if f != "phi":
                    if j1 == 1:  # eps = 0: level 1 is returned unchanged, store level 2 only
                        assert np.array_equal(a[0], x[f][0]), f"{case}: level 1 of {f} changed"
                    a = a[levels]
                assert np.all(np.isfinite(a.view(np.float64))), (case, f)
                zero = a.view(np.float64).reshape(a.shape + (2,)) == 0.0
                assert zero[..., ~TRI, :].all(), f"{case} {f}: the reference left something outside the triangle"
                if f != "phi":  # Im of m = 0: zero on the level the step wrote (timint truncates it)
                    assert zero[-1][..., :, 0, 1].all(), (case, f)
                    act = floor_active(a)
                    active += [(case, f) + tuple(i) for i in np.argwhere(act).tolist()]
                out[name][f"{case}_{f}"] = a
                out[name][f"{case}_{f}_zero"] = np.packbits(zero)
            out[name][f"{case}_case"] = np.array([j1, j2, dt, alph, rob, wil])
    assert not active, f"the floor is active on (case, field, time level, level, m) {active}"
    out["phys"] = {"phys": phys}
    for name, arrays in out.items():
        np.savez_compressed(path(name), **arrays)
        size = os.path.getsize(path(name))
        print("wrote", path(name), size, "bytes")
        assert size < 1 << 20, "fixture over 1 MiB"


if __name__ == "__main__":
    main()
