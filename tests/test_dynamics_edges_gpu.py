"""The fused dynamics step (k_st_inv, k_st_rows, k_st_gridspec_p, k_st_spec) and the
unfused one against the reference's `step` on the white, edge-loaded state
(tests/golden/make_dyn_edges_golden.py), wave by wave: per field, time level, level and
zonal wavenumber m (tests/_dyn_measure.py), every case through both forms, T30L8 single
steps.

Tolerances, none of them taken from what the GPU returned:

 - state, per (case, field): tol() of test_oracle_dynamics_edges.py = 10 x the oracle's
   own worst error against the reference under the same measure, rounded up to one
   significant digit (2e-15 ... 6e-14; the table and its reason are in that file's
   docstring and DESIGN.md section 5);
 - outside the triangle, and Im of m = 0: exactly zero where the reference and the oracle
   are both exactly zero, else tol() x the level's maximum;
 - phi of lf (PHI_TOL = 1e-14): the oracle's equals the reference's bit for bit, so 10 x
   its error is no bound.  geop adds two terms xgeop * t per level to phis, 16 fp64
   operations at most, each rounded at 1.1e-16 of a partial sum, and the partial sums
   of the level-independent white coefficients stay within a few row maxima: 1e-14 is
   the most rounding can give, FMA contraction included;
 - tendencies of step(2, 2, 0) against the oracle's (TEND_TOL = 1e-12): the reference
   does not hand out its tendencies, so there is no oracle-against-reference noise to
   multiply; 1e-12 is the bound test_dynamics_gpu.py already puts on this comparison,
   applied here to every row instead of the whole array;
 - the GPU's own physics (lf): tol() + what a physics error of the physics suite's
   bound (1e-12 of a level's largest tendency, test_physics_gpu.py) does to each row,
   taken from the oracle by linearity: D = step(P + d) - step(P) for a grid perturbation
   d of random sign and 1e-6 of each level's maximum, scaled by 1e-6.
"""
import os
import sys

import numpy as np
import pytest

import _dyn_measure as dm
import oracle
from conftest import REPO
from test_oracle_dynamics_edges import CASES, levels, oracle_step, tol, white_bc

sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
import make_dyn_edges_golden as mk  # noqa: E402

pytestmark = pytest.mark.gpu

PHI_TOL = 1e-14
TEND_TOL = 1e-12
SPEC_TOL = 1e-12  # test_spectral_gpu.py's TOL
PHYS_REL = 1e-12  # test_physics_gpu.py's TOL
FORMS = ("fused", "unfused")
TEND_SLICES = {"vor": slice(0, 8), "div": slice(8, 16), "t": slice(16, 24), "tr": slice(24, 32), "ps": slice(32, 33)}


@pytest.fixture(scope="module")
def white():
    return mk.inputs()


@pytest.fixture(scope="module")
def edges():
    return mk.golden()


@pytest.fixture(scope="module")
def dyns(cuda):
    from speedy_ml_amd.dynamics import Dynamics

    d = {}
    for form in FORMS:
        d[form] = Dynamics()
        d[form].set_fused(form == "fused")
    yield d
    for x in d.values():
        x.close()


def _load(d, x):
    d.set_forcing(x["phis"], x["tcorh"], x["qcorh"])
    d.set_state({f: x[f] for f in mk.FIELDS})


def _run(d, x, g, case, **override):
    """The state after one step of `case` with the reference's P handed in."""
    j1, j2, dt, alph, rob, wil = g[f"{case}_case"]
    p = dict(alph=float(alph), rob=float(rob), wil=float(wil))
    p.update(override)
    _load(d, x)
    d.step(int(j1), int(j2), float(dt), p["alph"], p["rob"], p["wil"], phys=g["phys"])
    return d.get_state()


@pytest.fixture(scope="module")
def oracle_steps(white, edges):
    """The oracle's output of every case (for the zero masks), computed once."""
    return {case: oracle_step(white, edges, case)[0] for case in CASES}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES)
def test_step_matches_reference_per_wavenumber(dyns, white, edges, oracle_steps, case, form):
    x, g = white, edges
    st = _run(dyns[form], x, g, case)
    lv = levels(g[f"{case}_case"][0])
    worst = {}
    for f in mk.FIELDS:
        worst[f] = dm.worst(st[f][lv], g[f"{case}_{f}"])
    print(f"{form} {case}: " + " ".join(f"{f} {worst[f]:.2e}/{tol(case, f):.0e}" for f in mk.FIELDS))
    for f in mk.FIELDS:
        ref = g[f"{case}_{f}"]
        err, _ = dm.per_m(st[f][lv], ref)
        assert err.max() <= tol(case, f), (form, case, f, err.max(), np.unravel_index(err.argmax(), err.shape))
        dm.check_zeros(st[f][lv], ref, g[f"{case}_{f}_zero"], oracle_steps[case][f][lv], tol(case, f))
        if lv == [1]:
            np.testing.assert_array_equal(st[f][0], x[f][0])


@pytest.mark.parametrize("form", FORMS)
def test_leapfrog_geopotential_per_wavenumber(dyns, white, edges, form):
    _run(dyns[form], white, edges, "lf")
    err, _ = dm.per_m(dyns[form].get_phi(), edges["lf_phi"])
    print(f"{form} lf phi: worst per level", " ".join(f"{e:.1e}" for e in err.max(axis=-1)))
    assert err.max() <= PHI_TOL, err.max()


@pytest.mark.parametrize("form", FORMS)
def test_tendencies_only_per_wavenumber(dyns, white, edges, form):
    """step(2, 2, 0, alph): the tendencies against the oracle's per field, level and m;
    the state is bitwise untouched."""
    x, g, d = white, edges, dyns[form]
    _load(d, x)
    d.step(2, 2, 0.0, 0.5, phys=g["phys"])
    tend = d.get_tendencies()
    st = oracle.dyn_state_copy(x)
    _, otend = oracle.dyn_step(st, x["phis"], x["tcorh"], x["qcorh"], g["phys"], 2, 2, 0.0, 0.5)
    err, active = dm.per_m(tend, otend)
    print(f"{form} tendencies: " + " ".join(f"{f} {err[sl].max():.2e}" for f, sl in TEND_SLICES.items()),
          f"floor active on {active.sum()} of {active.size} rows")
    assert active.mean() < 0.05
    for f, sl in TEND_SLICES.items():
        assert err[sl].max() <= TEND_TOL, (form, f, err[sl].max())
    got = d.get_state()
    for f in mk.FIELDS:
        np.testing.assert_array_equal(got[f], x[f])


@pytest.mark.parametrize("form", FORMS)
def test_step_parameters_reach_the_kernels(dyns, white, edges, form):
    """lf_rw passes with its own alph, rob, wil (the case test above) and fails under the
    measure with any one of them, or all three, at the default: a constant baked into a
    kernel where the argument belongs cannot pass both."""
    from speedy_ml_amd.dynamics import ALPH, ROB, WIL

    x, g, d = white, edges, dyns[form]
    own = _run(d, x, g, "lf_rw")
    for f in mk.FIELDS:
        assert dm.worst(own[f], g[f"lf_rw_{f}"]) <= tol("lf_rw", f), f
    for name, override in (("alph", dict(alph=ALPH)), ("rob", dict(rob=ROB)), ("wil", dict(wil=WIL)),
                           ("all", dict(alph=ALPH, rob=ROB, wil=WIL))):
        st = _run(d, x, g, "lf_rw", **override)
        ratio = {f: dm.worst(st[f], g[f"lf_rw_{f}"]) / tol("lf_rw", f) for f in mk.FIELDS}
        print(f"{form} lf_rw with default {name}: err / tolerance " + " ".join(f"{f} {r:.1e}" for f, r in ratio.items()))
        # rob and wil enter every field's filter; alph only the gravity-wave fields
        for f in (("div", "t", "ps") if name == "alph" else mk.FIELDS):
            assert ratio[f] > 1.0, (name, f, ratio[f])
            assert dm.worst(st[f], own[f]) > tol("lf_rw", f), (name, f)


@pytest.mark.parametrize("form", FORMS)
def test_gpu_physics_on_the_white_state(dyns, white, edges, form):
    """One lf step with the GPU's own phypar (lradsw off) against the oracle's
    dyn_step_physics.  test_oracle_dynamics_edges.py shows the oracle's physics
    tendencies equal the reference's P on this state (no branch flips)."""
    x, g, d = white, edges, dyns[form]
    j1, j2, dt, alph, rob, wil = g["lf_case"]
    bc = white_bc(x)
    st = oracle.dyn_state_copy(x)
    ptend = oracle.phypar_grid(*oracle.phys_inputs(st, x["phis"]), bc, oracle.phys_state(), False)
    ptend = ptend.reshape(4, oracle.KX, 48, 96)
    ref, _, _ = oracle_step(x, g, "lf", phys=ptend)
    rng = np.random.default_rng(7)
    delta = 1e-6 * np.abs(ptend).max(axis=(2, 3), keepdims=True) * rng.choice([-1.0, 1.0], size=ptend.shape)
    pert, _, _ = oracle_step(x, g, "lf", phys=ptend + delta)
    try:
        _load(d, x)
        d.set_physics(bc)
        d.set_rad_state(None)
        d.set_clock(1, False)
        d.step(int(j1), int(j2), float(dt), float(alph), float(rob), float(wil))
        got = d.get_state()
    finally:
        d.set_physics(None)
    for f in mk.FIELDS:
        a = np.abs(ref[f])
        den = np.maximum((a * dm.TRI).max(axis=-2), dm.FLOOR * a.max(axis=(-2, -1))[..., None])
        allowed = tol("lf", f) + PHYS_REL * (np.abs(pert[f] - ref[f]) * dm.TRI).max(axis=-2) / 1e-6 / den
        err, _ = dm.per_m(got[f], ref[f])
        print(f"{form} lf with GPU physics, {f}: worst err {err.max():.2e}, worst err / allowed {(err / allowed).max():.2e}, "
              f"allowed {allowed.min():.1e} .. {allowed.max():.1e}")
        assert (err <= allowed).all(), (form, f, (err / allowed).max())


def _impulses():
    """One field per coefficient of the triangle and part (Im of m = 0 left out, gridx
    drops it): (961, 32, 62) in the transforms' layout [n, 2 m + part]."""
    e = []
    for m in range(31):
        for n in range(31 - m):
            for part in range(2):
                if m == 0 and part == 1:
                    continue
                a = np.zeros((32, 62))
                a[n, 2 * m + part] = 1.0
                e.append(a)
    return np.stack(e)


def test_transform_impulses(cuda):
    """Each column of pinv and pfwd on its own instead of inside a random sum:
    grid(e) against oracle.grid per field, spec(grid(e)) = e within the spectral suite's
    TOL.  The reference's spec is no projection on the triangle -- it also fills the
    waves m + n = 31, to rounding, and so does the oracle -- so outside the triangle the
    rule of _dyn_measure.check_zeros holds: exactly zero where the oracle's spec is
    exactly zero whatever the field (m + n > 31, and n = 31 of m = 0), within TOL on
    m + n = 31.  (Where the oracle is zero on m + n = 31 for one impulse only, it is the
    parity of that impulse cancelling bit for bit in its folded hemispheres; the MFMA sum
    over all 48 latitudes leaves rounding there, as it does inside the triangle.)"""
    import torch

    from speedy_ml_amd.spectral import Spectral

    sp = Spectral()
    e = _impulses()
    assert e.shape == (961, 32, 62)
    tri = (np.arange(62)[None, :] // 2 + np.arange(32)[:, None]) <= 30
    g = sp.grid(torch.from_numpy(e).to(cuda))
    back = sp.spec(g).cpu().numpy()
    g = g.cpu().numpy()
    og = np.stack([oracle.grid(a, 1) for a in e])
    gerr = np.abs(g - og).max(axis=(1, 2)) / np.abs(og).max(axis=(1, 2))
    print(f"grid(e) vs oracle: worst {gerr.max():.2e} at field {gerr.argmax()}")
    assert gerr.max() < SPEC_TOL
    rerr = np.abs(back - e).max(axis=(1, 2))
    print(f"spec(grid(e)) - e: worst {rerr.max():.2e} at field {rerr.argmax()}; inside the triangle "
          f"{np.abs(back - e)[:, tri].max():.2e}, outside {np.abs(back[:, ~tri]).max():.2e}")
    assert rerr.max() < SPEC_TOL
    # structural zeros: where the oracle's spec is exactly zero for every impulse
    ozero = (np.stack([oracle.spec(a) for a in og]) == 0.0).all(axis=0) & ~tri
    total = (np.arange(62)[None, :] // 2 + np.arange(32)[:, None])
    assert ozero.sum() == (~tri).sum() - 60 and (total[~tri & ~ozero] == 31).all()  # all but m + n = 31, m >= 1
    bad = np.argwhere(back[:, ozero] != 0.0)
    print(f"structural zeros: {ozero.sum()} positions x {len(e)} fields, {len(bad)} values not zero; "
          f"on m + n = 31: max |spec| {np.abs(back[:, ~tri & ~ozero]).max():.2e}")
    assert len(bad) == 0, (len(bad), np.abs(back[:, ozero]).max(), sorted(set(total[ozero][bad[:, 1]].tolist())))
    assert np.abs(back[:, ~tri]).max() < SPEC_TOL
