"""sml_slab_train_series / sml_res_set_target_index / sml_slab_target_index: the symbols, and
the argument checks that need no device -- SML_ERR_ARG with a message on null and
out-of-range arguments, before anything touches a context."""
import ctypes
import os

import numpy as np

from speedy_ml_amd import _lib

SML_ERR_ARG = -1


def test_slab_series_symbols_are_declared():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "speedy_ml.h")).read()
    fortran = open(os.path.join(root, "speedy-ml-1_amd", "fortran", "sml_hip.f90")).read()
    for name in ("sml_slab_train_series", "sml_res_set_target_index", "sml_slab_target_index"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib(), name)
        assert getattr(_lib.lib(), name).argtypes is not None
        assert f"int {name}(" in header
        assert f"bind(C, name='{name}')" in fortran


def test_slab_series_refuses_without_a_device():
    L = _lib.lib()
    buf = (ctypes.c_double * 4)()  # 16-byte aligned, never dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)
    ctx = ctypes.cast(buf, ctypes.c_void_p)  # a non-null "context": every case below is refused before it is read

    def series(atmo=ctx, slab=ctx, g4=p, s4=147456, g2=p, pr=p, sst=p, s2=4608, T=4, window=2, divisor=1, t0=0, ncols=4,
               out=p, out_stride=1 << 40):
        return L.sml_slab_train_series(atmo, slab, g4, s4, g2, pr, sst, None, s2, T, window, divisor, t0, ncols, out,
                                       out_stride, None)

    cases = ((dict(T=0), b"T = 0"), (dict(T=-3), b"T = -3"),
             (dict(window=0), b"window = 0"), (dict(window=1025), b"window = 1025"),
             (dict(divisor=0), b"divisor = 0"), (dict(divisor=-2), b"divisor = -2"),
             (dict(t0=-1), b"t0 = -1"), (dict(ncols=-1), b"ncols = -1"), (dict(t0=2, ncols=3), b"leave the series"),
             (dict(t0=5, ncols=0), b"leave the series"),
             (dict(s4=147455), b"g4_stride"), (dict(s4=0), b"g4_stride"), (dict(s2=4607), b"g2_stride"),
             (dict(s4=147457), b"16-byte"),
             (dict(atmo=None), b"null reservoir context"), (dict(slab=None), b"null reservoir context"),
             (dict(g4=None), b"null argument"), (dict(g2=None), b"null argument"), (dict(pr=None), b"null argument"),
             (dict(sst=None), b"null argument"), (dict(out=None), b"null argument"),
             (dict(g4=ctypes.c_void_p(p.value + 8)), b"not 16-byte aligned"))
    for kw, word in cases:
        assert series(**kw) == SML_ERR_ARG, kw
        assert word in L.sml_last_error(), (kw, L.sml_last_error())


def test_target_index_calls_refuse_without_a_device():
    L = _lib.lib()
    idx = np.zeros(4, dtype=np.int32)
    assert L.sml_res_set_target_index(None, _lib.ptr(idx)) == SML_ERR_ARG
    assert b"null reservoir context" in L.sml_last_error()
    cnt = ctypes.c_int()
    assert L.sml_slab_target_index(1152, 0, None, ctypes.byref(cnt)) == SML_ERR_ARG
    assert b"null argument" in L.sml_last_error()
    assert L.sml_slab_target_index(1152, 0, _lib.ptr(idx), None) == SML_ERR_ARG
    assert L.sml_slab_target_index(1152, 1152, _lib.ptr(idx), ctypes.byref(cnt)) == SML_ERR_ARG
    assert b"does not decompose" in L.sml_last_error()
    assert L.sml_slab_target_index(1000, 0, _lib.ptr(idx), ctypes.byref(cnt)) == SML_ERR_ARG


def test_slab_target_index_is_the_inner_tile_of_the_sst_section():
    """Host arithmetic: entry 5 * in2d + the input-tile position of resolved point o, for a
    pole region (no halo row on the pole side), a wrap region and an interior one."""
    from speedy_ml_amd import domain

    L = _lib.lib()
    for region in (0, 23, 5, 500, 1151):
        g = domain.region_geometry(region)
        idx = np.full(5, -7, dtype=np.int32)
        cnt = ctypes.c_int()
        assert L.sml_slab_target_index(1152, region, _lib.ptr(idx), ctypes.byref(cnt)) == 0
        assert cnt.value == g.resx * g.resy == 4 and idx[4] == -7
        in2d = g.inx * g.iny
        y0 = 0 if region % 24 == 0 else 1  # the south-pole row of regions has no halo row below it
        want = [5 * in2d + (1 + o % 2) + g.inx * (y0 + o // 2) for o in range(4)]
        assert idx[:4].tolist() == want, (region, idx, want)
