"""The per-m spectral kernels (k_st_spec, k_io_entry, k_st_inv, and k_dyn_tail of the
unfused step, which share tail_coef / inv_inputs / uvspec_sel / gridy_m / gridy_io) with
the level index held wave-uniform, the level loops ended at the wave's level and
specy's MFMA operand guards dropped compute what the branch-free form computed, bit for
bit.

Cases and inputs: tests/golden/make_spec_kernel.py -- run_model from a grid with
GPU physics (a), the window without GPU physics launched step by step and as a graph
through the fused (b) and the unfused (c) path, and single fused steps followed by a
tendencies-only step (d: the fused path fills get_tendencies() only for dt <= 0, so the
tendencies compared are that third step's), each from dyn_state(1425) and from its
variant with data at the truncation edge of every m on the top and bottom level.  All at
T30L8 with two leapfrog steps.

 - bitwise: every array of every run equals the golden tests/golden/spec_kernel.npz,
   written by the build of the commit before the change (SHA-256 per array; ps and the
   forecast logp are stored in full and compared first, so a mismatch is sized);
 - rounding: cases a and b agree with the unfused path at
   test_row_kernel_shortwave_gpu.py's FUSED_TOL.
"""
import os
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
import make_spec_kernel as mk  # noqa: E402

pytestmark = pytest.mark.gpu

FUSED_TOL = 1e-11  # test_row_kernel_shortwave_gpu.py, test_physics_gpu.py
RUNS = ("a", "b_nograph", "b_graph", "c_nograph", "c_graph", "d")


@pytest.fixture(scope="module")
def golden_spec():
    return dict(np.load(mk.PATH))


@pytest.fixture(scope="module")
def all_runs(cuda):
    """Every pinned run of every variant, computed once."""
    return {v: mk.runs(v) for v in mk.VARIANTS}


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("variant", mk.VARIANTS)
def test_per_m_kernels_are_bitwise_the_golden(all_runs, golden_spec, variant, run):
    g = golden_spec
    assert int(g["seed"]) == mk.SEED and int(g["nleap"]) == mk.NLEAP and tuple(g["variants"]) == mk.VARIANTS
    made_with = str(g["hipcc_version"]).splitlines()[0]
    arrays = all_runs[variant][run]
    for k in mk.FULL:
        if k in arrays:
            diff = np.abs(arrays[k] - g[f"{variant}_{run}_{k}"]).max()
            print(f"{variant} {run}: max |{k} - golden| {diff:.3e}")
            assert diff == 0.0, (k, diff, made_with)
    for k, a in arrays.items():
        assert mk.digest(a) == str(g[f"{variant}_{run}_sha_{k}"]), (k, made_with)


def _close(x, y):
    x, y = np.asarray(x), np.asarray(y)
    assert np.abs(x - y).max() <= FUSED_TOL * max(np.abs(y).max(), 1e-300), np.abs(x - y).max()


@pytest.mark.parametrize("variant", mk.VARIANTS)
def test_run_model_agrees_with_unfused_path_to_rounding(all_runs, variant):
    """Case a, per variable and level (fc4d is (level, lat, lon, var))."""
    a = all_runs[variant]["a"]
    u = mk.run_a(variant, fused=False)
    for v in range(4):
        for k in range(8):
            _close(a["fc4d"][k, :, :, v], u["fc4d"][k, :, :, v])
    _close(a["logp"], u["logp"])
    for f in mk.STATE:
        for lev in range(2):
            if f == "ps":
                _close(a[f][lev], u[f][lev])
            else:
                for k in range(8):
                    _close(a[f][lev, k], u[f][lev, k])


@pytest.mark.parametrize("graph", ["nograph", "graph"])
@pytest.mark.parametrize("variant", mk.VARIANTS)
def test_window_agrees_with_unfused_path_to_rounding(all_runs, variant, graph):
    """Case b against case c, per variable, time level and level."""
    b, c = all_runs[variant][f"b_{graph}"], all_runs[variant][f"c_{graph}"]
    for f in mk.STATE:
        for lev in range(2):
            if f == "ps":
                _close(b[f][lev], c[f][lev])
            else:
                for k in range(8):
                    _close(b[f][lev, k], c[f][lev, k])
    for k in range(8):
        _close(b["phi"][k], c["phi"][k])
