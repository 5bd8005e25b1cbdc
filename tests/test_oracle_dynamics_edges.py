"""The oracle's `step` against the reference's on the white, edge-loaded state
(tests/golden/make_dyn_edges_golden.py), wave by wave (tests/_dyn_measure.py), and the
proof that this measure sees what the suite's max |err| / max |field| cannot.

The noise floor measured here is where the GPU tolerances of
test_dynamics_edges_gpu.py come from: NOISE[case][field] is the oracle's worst
err(field, time level, level, m) against the reference, as this file printed it when
the fixtures were written; tol() = 10 x that, rounded up to one significant digit (the
ratio between the suite's oracle bounds and its GPU bounds: fordate, 1e-13 and 1e-12).
Both sides are fp64 reorderings of the same sums -- the oracle's Fourier stage is a
long-double DFT, the reference's FFTPACK -- and the GPU adds the MFMA K-block order and
FMA contraction.  Every value is far inside the suite's one-step bound of 1e-12, so no
cancellation in the chosen amplitudes had to be looked for.  The test below asserts
oracle <= tol() / 10, so the table cannot drift from what the oracle does.

  worst per (case, field)   vor      div      t        tr       ps
  fwd                       3.2e-16  3.0e-16  1.8e-16  2.0e-16  1.1e-16
  lf0                       3.6e-16  4.6e-16  2.1e-16  2.4e-16  1.7e-16
  lf                        6.6e-16  8.5e-16  3.4e-16  1.0e-15  3.3e-16
  expl                      3.2e-16  1.7e-16  2.0e-16  2.0e-16  1.9e-16
  lf_rw                     6.3e-16  5.2e-15  3.5e-16  1.2e-15  4.1e-16

lf's phi = geop(j4) equals the reference's bit for bit.
"""
import math
import os
import sys

import numpy as np
import pytest

import _dyn_measure as dm
import oracle
from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
import make_dyn_edges_golden as mk  # noqa: E402

CASES = tuple(mk.CASES)
NOISE = {
    "fwd": {"vor": 3.24e-16, "div": 2.97e-16, "t": 1.84e-16, "tr": 2.02e-16, "ps": 1.08e-16},
    "lf0": {"vor": 3.59e-16, "div": 4.63e-16, "t": 2.11e-16, "tr": 2.37e-16, "ps": 1.72e-16},
    "lf": {"vor": 6.57e-16, "div": 8.49e-16, "t": 3.40e-16, "tr": 1.00e-15, "ps": 3.32e-16},
    "expl": {"vor": 3.24e-16, "div": 1.71e-16, "t": 1.99e-16, "tr": 2.02e-16, "ps": 1.92e-16},
    "lf_rw": {"vor": 6.26e-16, "div": 5.24e-15, "t": 3.54e-16, "tr": 1.15e-15, "ps": 4.07e-16},
}
OLD_TOL = 1e-12  # test_dynamics_gpu.py's TOL, on its global _rel
PHYS_TOL = 1e-12  # test_oracle_physics_step.py's TOL


def tol(case, field):
    """The GPU tolerance: 10 x NOISE, rounded up to one significant digit."""
    v = 10.0 * NOISE[case][field]
    e = 10.0 ** math.floor(math.log10(v))
    return math.ceil(v / e - 1e-9) * e


def levels(j1):
    return [0, 1] if int(j1) == 2 else [1]


def white_bc(x):
    """phypar's boundary fields of the white state (test_oracle_physics_step.dyn_bc)."""
    from test_oracle_physics_step import dyn_bc

    return dyn_bc(x)


@pytest.fixture(scope="module")
def white():
    return mk.inputs()


@pytest.fixture(scope="module")
def edges():
    return mk.golden()


def oracle_step(x, g, case, phys=None):
    """(state, phi, tendencies) of the oracle's step of `case`; phys: its P, default the reference's."""
    j1, j2, dt, alph, rob, wil = g[f"{case}_case"]
    st = oracle.dyn_state_copy(x)
    phi, tend = oracle.dyn_step(st, x["phis"], x["tcorh"], x["qcorh"], g["phys"] if phys is None else phys,
                                int(j1), int(j2), float(dt), float(alph), float(rob), float(wil))
    return st, phi, tend


def test_inputs_are_white_and_the_cases_are_the_generators(white, edges):
    x, g = white, edges
    for case, args in mk.CASES.items():
        np.testing.assert_array_equal(g[f"{case}_case"], np.array(args))
    assert mk.CASES["lf_rw"][3:] != mk.CASES["lf"][3:]
    for f in mk.FIELDS:
        a = np.abs(x[f])
        assert (a[..., ~dm.TRI] == 0.0).all() and (x[f][..., :, 0].imag == 0.0).all()
        inside = a[..., dm.TRI]
        assert (inside[..., 1:] > 0.0).all(), f  # every wave but (0,0) carries data
    lifted = x["lifted"]
    print(f"{len(lifted)} rows lifted to the floor, fields {sorted({f for f, _, _ in lifted})}")
    assert {f for f, _, _ in lifted} <= {"t", "tr"}


@pytest.mark.parametrize("case", CASES)
def test_step_matches_reference_per_wavenumber(white, edges, case):
    x, g = white, edges
    st, phi, _ = oracle_step(x, g, case)
    lv = levels(g[f"{case}_case"][0])
    for f in mk.FIELDS:
        ref = g[f"{case}_{f}"]
        err, active = dm.per_m(st[f][lv], ref)
        assert not active.any(), (case, f)  # the generator's condition, on the stored reference
        print(f"oracle vs reference, {case} {f}: worst err {err.max():.2e} (global {dm.global_rel(st[f][lv], ref):.1e})")
        assert err.max() <= tol(case, f) / 10.0, (case, f, err.max())
        n = dm.check_zeros(st[f][lv], ref, g[f"{case}_{f}_zero"], st[f][lv], tol(case, f))
        assert n >= ref.size  # at least everything outside the triangle
        if lv == [1]:
            np.testing.assert_array_equal(st[f][0], x[f][0])
    if case == "lf":
        np.testing.assert_array_equal(phi, g["lf_phi"])


def test_tendency_rows_rarely_reach_the_floor(white, edges):
    """The reference's step keeps its tendencies to itself, so the share of tendency rows
    on which the floor is active is checked on the oracle's: under 5 %."""
    x, g = white, edges
    st = oracle.dyn_state_copy(x)
    _, tend = oracle.dyn_step(st, x["phis"], x["tcorh"], x["qcorh"], g["phys"], 2, 2, 0.0, 0.5)
    _, active = dm.per_m(tend, tend)
    print(f"tendency rows with the floor active: {active.sum()} of {active.size} ({100.0 * active.mean():.2f} %)")
    assert active.mean() < 0.05
    for f in mk.FIELDS:
        np.testing.assert_array_equal(st[f], x[f])


# (field, time level, level, n, m): the truncation edge of the longest and of the
# shortest row on a middle level, and the top level, whose humidity is 1e-5 of the bottom's
EDITS = {"m30_n0": ("tr", 1, 3, 0, 30), "m0_n30": ("tr", 1, 3, 30, 0), "tr_level1": ("tr", 1, 0, 7, 9)}


@pytest.mark.parametrize("edit", sorted(EDITS))
def test_measure_rejects_what_the_global_norm_accepts(edges, edit):
    """One coefficient of the reference's lf output scaled by 1 + 1e-9: the per-wavenumber
    measure fails it at lf's tolerance, test_dynamics_gpu.py's _rel at 1e-12 does not.
    (On t the rows lift_rows() raised hold a coefficient of 1e-3 of the mean, which the
    global norm sees at 2e-12; everywhere else, and on every level of tr but the lowest,
    it is blind to 1e-9.)"""
    f, j, k, n, m = EDITS[edit]
    ref = edges[f"lf_{f}"]
    got = ref.copy()
    assert got[j, k, n, m] != 0.0
    got[j, k, n, m] *= 1.0 + 1e-9
    new, old = dm.worst(got, ref), dm.global_rel(got, ref)
    print(f"{edit}: per-wavenumber {new:.2e} (tolerance {tol('lf', f):.0e}), global {old:.2e} (tolerance {OLD_TOL:.0e})")
    assert new > tol("lf", f)
    assert old < OLD_TOL
    assert dm.worst(ref, ref) == 0.0


def test_oracle_physics_is_the_references_on_the_white_state(white, edges):
    """phys_inputs -> phypar_grid of the oracle against the reference's P within the
    physics suite's bound, per variable and (printed and asserted) per level: no branch
    flips between them at any column, so test_dynamics_edges_gpu.py may compare the
    GPU's own physics with the oracle's on this state."""
    x, g = white, edges
    st = oracle.dyn_state_copy(x)
    tend = oracle.phypar_grid(*oracle.phys_inputs(st, x["phis"]), white_bc(x), oracle.phys_state(), False)
    ref = g["phys"].reshape(4, oracle.KX, oracle.NGP)
    for v in range(4):
        den = np.abs(ref[v]).max(axis=-1)
        lv = np.abs(tend[v] - ref[v]).max(axis=-1) / np.where(den > 0, den, 1.0)
        print(f"oracle physics vs reference P, variable {v} per level:", " ".join(f"{e:.1e}" for e in lv))
        assert dm.global_rel(tend[v], ref[v]) < PHYS_TOL, v
        assert (lv < PHYS_TOL).all(), (v, lv)
