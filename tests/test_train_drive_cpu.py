"""sml_region_target_index (host only): the positions of a region's training targets
inside its feedback vector, against an index list built in numpy from the oracle's
restatement of get_trainingdataindices (res_domain.f90:547-574) and the layout
tile_full_input_to_target_data2d reads (:602-651)."""
import ctypes

import numpy as np
import pytest

import oracle
from speedy_ml_amd import _lib

NUMREGIONS = 1152
NOUT = 136


def _numpy_index(region):
    g = oracle.region_geometry(region, NUMREGIONS)
    ix, iy = g["inputxchunk"], g["inputychunk"]
    in2d = ix * iy
    xs = slice(g["tdata_xstart"] - 1, g["tdata_xend"])
    ys = slice(g["tdata_ystart"] - 1, g["tdata_yend"])
    # Fortran temp5d(4, ix, iy, 8) / temp3d(ix, iy) == C arrays with the axes reversed
    atmo = np.arange(4 * in2d * 8).reshape(8, iy, ix, 4)[:, ys, xs, :]
    logp = 4 * in2d * 8 + np.arange(in2d).reshape(iy, ix)[ys, xs]
    precip = logp + in2d
    return np.concatenate([atmo.ravel(), logp.ravel(), precip.ravel()]), g


def _lib_index(region, sst):
    idx = np.full(NOUT + 8, -7, dtype=np.int32)
    cnt = ctypes.c_int()
    _lib.check(_lib.lib().sml_region_target_index(NUMREGIONS, region, sst, _lib.ptr(idx), ctypes.byref(cnt)))
    assert (idx[cnt.value:] == -7).all()  # nothing written past the count
    return idx[:cnt.value]


@pytest.mark.parametrize("sst", [0, 1])
def test_target_index_matches_the_oracle_geometry(sst):
    polar = 0
    for region in range(NUMREGIONS):
        ref, g = _numpy_index(region)
        got = _lib_index(region, sst)
        assert len(got) == NOUT, region
        np.testing.assert_array_equal(got, ref, err_msg=f"region {region}")
        in2d = g["inputxchunk"] * g["inputychunk"]
        assert got.max() < 4 * in2d * 8 + 2 * in2d  # before the sst / tisr blocks
        polar += bool(g["pole"])
    assert polar == 96


def test_target_index_rejects_a_bad_region():
    idx = np.zeros(NOUT, dtype=np.int32)
    cnt = ctypes.c_int()
    assert _lib.lib().sml_region_target_index(NUMREGIONS, NUMREGIONS, 0, _lib.ptr(idx), ctypes.byref(cnt)) != 0
    assert _lib.lib().sml_region_target_index(NUMREGIONS, 0, 0, None, ctypes.byref(cnt)) != 0
