"""The row kernel's shortwave steps (k_st_gridspec_p with sml_physics_pair.hpp: the pair
lanes run the part of the shortwave path that needs neither the moist side's hand-over
nor the cloud BEFORE the hand-over barrier, the rest after it) compute what the one-stage
form computed, bit for bit.

Cases (tests/golden/make_row_kernel_sw.py): the seeded dyn_state with its spectral
humidity scaled by 0.25, 1 and 2.5, stepone + 6 leapfrog steps with physics through the
fused path at T30L8 (48 x 96 columns); stepone's two steps and the leapfrog steps 1 and 4
are shortwave steps.  On the CPU oracle the first case has 27 % of its columns without
cloud and stratiform tops at the levels 4, 5, 6 and 7 (= nl1) and at or above 3; the
other two are cloudy everywhere, mostly with tops at or above level 3 (convective, or
the stratiform loop's first level), some at 4..7.

 - bitwise: the final spectral state and radiation state equal the golden
   tests/golden/row_kernel_sw.npz, written by the build before the split (SHA-256 per
   array; ps and ssrd are stored in full and compared first, so a mismatch is sized);
 - rounding: each case agrees with the unfused path (sml_dyn_set_fused off: k_phys, the
   one-lane phys_column) at test_fused_step_agrees_with_unfused_step_to_rounding's
   FUSED_TOL.
"""
import os
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
import make_row_kernel_sw as mk  # noqa: E402

pytestmark = pytest.mark.gpu

FUSED_TOL = 1e-11  # test_physics_gpu.py


@pytest.fixture(scope="module")
def golden_sw():
    return dict(np.load(mk.PATH))


@pytest.fixture(scope="module")
def fused_runs(cuda):
    """The fused path's (state, rad) per case, computed once."""
    return [mk.run_case(scale) for scale in mk.SCALES]


@pytest.mark.parametrize("c", range(len(mk.SCALES)))
def test_shortwave_steps_are_bitwise_the_golden(fused_runs, golden_sw, c):
    g = golden_sw
    assert tuple(g["scales"]) == mk.SCALES and int(g["seed"]) == mk.SEED and int(g["nleap"]) == mk.NLEAP
    state, rad = fused_runs[c]
    made_with = str(g["hipcc_version"]).splitlines()[0]
    dps = np.abs(state["ps"] - g[f"c{c}_ps"]).max()
    dss = np.abs(rad["ssrd"] - g[f"c{c}_ssrd"]).max()
    print(f"scale {mk.SCALES[c]}: max |ps - golden| {dps:.3e}, max |ssrd - golden| {dss:.3e}")
    assert dps == 0.0 and dss == 0.0, (dps, dss, made_with)
    for k in mk.STATE:
        assert mk.digest(state[k]) == str(g[f"c{c}_sha_{k}"]), (k, made_with)
    for k in mk.RAD:
        assert mk.digest(rad[k]) == str(g[f"c{c}_sha_{k}"]), (k, made_with)


@pytest.mark.parametrize("c", range(len(mk.SCALES)))
def test_shortwave_steps_agree_with_unfused_path_to_rounding(fused_runs, c):
    state, rad = fused_runs[c]
    ustate, urad = mk.run_case(mk.SCALES[c], fused=False)

    def close(x, y):
        x, y = np.asarray(x), np.asarray(y)
        assert np.abs(x - y).max() <= FUSED_TOL * max(np.abs(y).max(), 1e-300), np.abs(x - y).max()

    for k in mk.STATE:
        for j in range(state[k].shape[0]):
            close(state[k][j], ustate[k][j])
    for k in mk.RAD:
        close(rad[k], urad[k])
