"""Conditions on the physics edge fixtures (tests/_phys_edges.py), on the CPU: the
oracle's branch census leaves its results bitwise alone; both fixtures reach every
state of every census entry; few (direct fixture) or no (state fixture) columns sit so
close to a threshold that +-2 ulp on the inputs flips a decision; the noise floor of the
tendencies under that perturbation; and the oracle against the reference's own phypar on
the state fixture (tests/golden/phys_edges_ref.npz, phys_edges_ref_b.npz), per variable
and per level.

Norm: max |err| over the compared columns / max |reference| of that level, per variable
and level (a norm over all levels hides the upper levels, whose tendencies are 100 to
1000 times smaller than the largest).  Tolerance: TOL = 1e-12 of test_oracle_physics.py,
per level."""
import numpy as np
import pytest

import oracle
import _phys_edges as pe
from test_oracle_physics import TOL, _fill

MIN_DIRECT = 24        # columns per state over A and B, direct fixture
MIN_STATE = 16         # columns per state over S_A and S_B
MIN_STATE_GOLDEN = 4   # of them among the columns the golden stores
MAX_FRAGILE = 23       # 0.5 % of 4608
VARS = ("u", "v", "t", "q")


@pytest.fixture(scope="module")
def direct_sets():
    d = pe.direct()
    return [d["A"], d["B"]]


@pytest.fixture(scope="module")
def state_sets():
    return pe.state_sets()


def _in_range(sets):
    for s in sets:
        for x in s["ins"]:
            assert np.isfinite(x).all()
        for a in (s["ins"][2], s["bc"]["stl_am"], s["bc"]["sst_am"]):
            assert 150.0 <= a.min() and a.max() <= 350.0, (a.min(), a.max())


def _coverage(cens, need, exempt=()):
    cov = pe.coverage(cens)
    missing = {k: v for k, v in cov.items() if v < need and k not in exempt}
    assert not missing, missing
    return cov


def test_census_leaves_the_oracle_bitwise(direct_sets):
    for lradsw in (True, False):
        a, b = oracle.phys_state(), oracle.phys_state()
        for s in direct_sets:  # B after A, so that lradsw False reads a made radiation state
            ta = oracle.phypar_grid(*s["ins"], s["bc"], a, lradsw)
            tb, cen = oracle.phypar_grid(*s["ins"], s["bc"], b, lradsw, census=True)
            assert cen.shape == (oracle.NGP, len(oracle.CENSUS)) and cen.dtype == np.int32
            np.testing.assert_array_equal(ta, tb)
            for k in a:
                np.testing.assert_array_equal(a[k], b[k])
            assert ((cen[:, pe.CEN["cld_icltop"]] == -1) == (not lradsw)).all()


def test_census_agrees_with_the_inputs(direct_sets):
    """The entries that can be restated from the inputs alone, and the ties between entries."""
    C = pe.CEN
    for (tend, cen, rad), s in zip(pe.run_sequence(direct_sets), direct_sets):
        ug, vg, tg, qg, phig, psl = s["ins"]
        nint = np.where(tg >= 0, np.floor(tg + 0.5), -np.floor(-tg + 0.5))  # half away from zero
        np.testing.assert_array_equal(cen[:, C["lw_cold"]], (nint < 200).any(axis=0))
        np.testing.assert_array_equal(cen[:, C["lw_hot"]], (nint > 320).any(axis=0))
        np.testing.assert_array_equal(cen[:, C["qclip"]], (qg < 0).any(axis=0))
        np.testing.assert_array_equal(cen[:, C["sfl_tgrad"]], tg[7] > tg[6])
        np.testing.assert_array_equal(cen[:, C["cnv_psg"]], np.exp(psl) > 0.8)
        se = pe.CP * tg + phig
        dry = np.zeros(oracle.NGP, np.int32)
        for k in range(1, 8):
            dry |= (se[k - 1] < se[k] + 0.1 * (phig[k - 1] - phig[k])).astype(np.int32) << k
        np.testing.assert_array_equal(cen[:, C["vdi_dryadj"]], dry)
        none = cen[:, C["cnv_itop"]] == 9
        assert none[cen[:, C["cnv_psg"]] == 0].all()
        for k in ("cnv_precnv", "cnv_fqmax", "cnv_fpsa", "cnv_delq"):
            assert ((cen[:, C[k]] == -1) == none).all(), k
        assert ((cen[:, C["lsc_levels"]] == 0) == (cen[:, C["lsc_dqmax"]] == -1)).all()
        if (cen[:, C["cld_icltop"]] >= 0).all():  # the shortwave call: icltop = min(cloud top, convmf's and lscond's itop)
            lsc = cen[:, C["lsc_levels"]]
            lsc_top = np.full(oracle.NGP, 9)
            for k in range(8, 1, -1):
                lsc_top = np.where((lsc >> k) & 1 == 1, k, lsc_top)
            itop = np.minimum(cen[:, C["cnv_itop"]], lsc_top)
            np.testing.assert_array_equal(cen[:, C["cld_icltop"]], np.minimum(itop, cen[:, C["cld_strtop"]]))
            np.testing.assert_array_equal(cen[:, C["cld_itoplt"]], itop < cen[:, C["cld_strtop"]])


def test_direct_fixture_reaches_every_branch_state(direct_sets):
    _in_range(direct_sets)
    runs = pe.run_sequence(direct_sets)
    for tend, _, rad in runs:
        assert np.isfinite(tend).all() and all(np.isfinite(v).all() for v in rad.values())
    cov = _coverage([r[1] for r in runs], MIN_DIRECT)
    print("direct fixture, columns per state:", cov)
    # what the bands are for, beyond the census: exact inputs and the longwave-only call on another band's state
    a, b = direct_sets
    for s in direct_sets:
        ug, vg, tg, qg, phig, psl = s["ins"]
        assert ((qg == 0.0).any(axis=0)).sum() >= MIN_DIRECT and ((qg < 0.0).any(axis=0)).sum() >= MIN_DIRECT
        assert (tg - np.floor(tg) == 0.5).any(axis=0).sum() >= MIN_DIRECT
        assert (tg[7] == tg[6]).sum() >= 4
        for v in (0.0, 1.0):
            assert (s["bc"]["fmask1"] == v).sum() >= MIN_DIRECT
        assert (s["bc"]["soilw_am"] == 0.0).sum() >= MIN_DIRECT
        psg = np.exp(psl)
        assert (psg < 0.8).sum() >= MIN_DIRECT and ((psg > 0.8) & (psg < 0.9)).sum() >= MIN_DIRECT
    changed = (np.exp(a["ins"][5]) < 0.9) != (np.exp(b["ins"][5]) < 0.9)
    assert changed.sum() >= 10 * MIN_DIRECT  # B's bands lie on other rows than A's


def test_direct_fixture_has_few_fragile_columns(direct_sets):
    base, fragile, draws = pe.fragility(direct_sets)
    print("direct fixture, fragile columns per call:", [int(f.sum()) for f in fragile])
    for f in fragile:
        assert f.sum() <= MAX_FRAGILE, int(f.sum())


def test_state_fixture_reaches_every_branch_state(state_sets):
    _in_range(state_sets)
    runs = pe.run_sequence(state_sets)
    for tend, _, rad in runs:
        assert np.isfinite(tend).all() and all(np.isfinite(v).all() for v in rad.values())
    exempt = set(pe.STATE_FIXTURE_EXEMPT)
    cov = _coverage([r[1] for r in runs], MIN_STATE, exempt)
    print("state fixture, columns per state:", cov)
    _coverage([r[1][pe.SEL] for r in runs], MIN_STATE_GOLDEN, exempt)
    a = state_sets[0]["ins"]
    psg = np.exp(a[5])
    assert psg.min() < 0.62 and ((psg > 0.8) & (psg < 0.9)).sum() >= MIN_STATE
    assert ((a[2][:2].min(axis=0) > 190.0) & (a[2][:2].min(axis=0) < 199.0)).sum() >= MIN_STATE
    assert ((a[2][6] > 321.0) & (a[2][7] > 321.0)).sum() >= MIN_STATE


def test_state_fixture_has_no_fragile_column(state_sets):
    """A flipped column cannot be cut out of a spectral comparison: none may flip, and
    none may sit within 1e-6 K of a nint tie."""
    base, fragile, draws = pe.fragility(state_sets)
    for f, s in zip(fragile, state_sets):
        assert f.sum() == 0, np.flatnonzero(f)
        assert pe.near_tie(s["ins"][2]).sum() == 0


@pytest.mark.parametrize("which", ["direct", "state"])
def test_noise_floor_of_the_tendencies(direct_sets, state_sets, which):
    """Largest change of the oracle's tendency under +-2 ulp on the inputs, over columns
    that are neither fragile nor on a nint tie, / the level's maximum: the table of
    DESIGN.md (SPEEDY window numerics).  It has to stay below TOL / 8 for TOL to be the
    bound of every level (tests/test_physics_edges_gpu.py takes 8 x the floor otherwise)."""
    sets = direct_sets if which == "direct" else state_sets
    floor = pe.noise_floor(sets)
    for c, name in enumerate("AB"):
        for v in range(4):
            print(f"{which} {name} {VARS[v]} floor per level:", " ".join(f"{x:.1e}" for x in floor[c][v]))
    assert np.isfinite(floor).all() and floor.max() < TOL
    bounds = pe.level_bounds(sets, TOL)
    assert (bounds >= TOL).all() and (bounds <= 8 * TOL).all()


def test_oracle_matches_reference_phypar_on_state_fixture(state_sets):
    """S_A with lradsw, then S_B without on the kept radiation state, as
    make_phys_edges_golden.py ran the reference's phypar."""
    g = dict(pe.golden("phys_edges_ref.npz"), **pe.golden("phys_edges_ref_b.npz"))
    sel = g["sel"]
    assert np.array_equal(sel, pe.SEL) and int(g["seed"]) == pe.STATE_SEED
    rad = oracle.phys_state()
    for case, s, lradsw in (("a", state_sets[0], True), ("b", state_sets[1], False)):
        # the golden is this fixture's: what the oracle's transforms give for the state is what phypar saw
        for name, x in zip(pe.INS, s["ins"]):
            ref = g[f"{case}_{name}"]
            if name == "qg1":  # phypar clips its qg1 in place (phy_phypar.f90:87): the golden holds max(q, 0)
                assert (ref >= 0.0).all() and (x < 0.0).any()
                x = np.maximum(x, 0.0)
            rel = pe.level_rel(x[..., sel], ref)
            assert (rel <= TOL).all(), (case, name, rel)
        ins = [_fill(g[f"{case}_{name}"], sel) for name in pe.INS]
        tend, cen = oracle.phypar_grid(*ins, s["bc"], rad, lradsw, census=True)
        own = oracle.phypar_grid(*s["ins"], s["bc"], {k: v.copy() for k, v in rad.items()}, lradsw, census=True)[1]
        own[:, pe.CEN["qclip"]] = cen[:, pe.CEN["qclip"]]  # (the clip is already applied in the golden's q)
        np.testing.assert_array_equal(cen[sel], own[sel])  # no column near a threshold: the same decisions
        ref = g[f"{case}_tend"]
        for v in range(4):
            rel = pe.level_rel(tend[v][:, sel], ref[v])
            print(f"oracle vs reference, {case} {VARS[v]} per level:", " ".join(f"{x:.1e}" for x in rel))
            k = int(rel.argmax())
            j = int(np.abs(tend[v][k, sel] - ref[v][k]).argmax())
            assert (rel <= TOL).all(), (case, VARS[v], rel, pe.describe(cen[sel[j]]))
        if case == "a":
            np.testing.assert_allclose(rad["tau2"][..., sel], g["a_tau2"], rtol=1e-13, atol=0)
            np.testing.assert_allclose(rad["stratc"][:, sel], g["a_stratc"], rtol=1e-13, atol=0)
            np.testing.assert_allclose(rad["ssrd"][sel], g["a_ssrd"], rtol=1e-13, atol=1e-12)
            rel = pe.level_rel(rad["tt_rsw"][:, sel], g["a_tt_rsw"])
            assert (rel <= TOL).all(), rel
