"""The ensemble's slab ocean and member tilings in the C ABI (include/speedy_ml.h): the built
library exports the new entry points, the header declares them with their member strides,
the Fortran module binds them, and the ABI version is unchanged.  CPU-only: no compute call
is made."""
import os
import re
import subprocess

from speedy_ml_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SLAB = ("sml_slab_create", "sml_slab_destroy", "sml_slab_info", "sml_slab_start", "sml_slab_predict",
        "sml_slab_sst", "sml_slab_ring", "sml_slab_buffers")
TILING = ("sml_res_tile_feedback_members", "sml_res_tile_tisr_field_members")
NEW = SLAB + TILING


def _header():
    txt = open(os.path.join(REPO, "include", "speedy_ml.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"\s+", " ", txt)


def _args(flat, name):
    m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", flat)
    assert m, name
    return m.group(1)


def test_library_exports_the_ensemble_slab():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (sml_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in exported, name
        assert hasattr(L, name), name
        assert name in _lib.EXPORTED, name
        assert getattr(L, name).argtypes is not None, name
    assert L.sml_abi_version() == 1


def test_header_declares_the_ensemble_slab():
    flat = _header()
    assert "typedef struct sml_slab sml_slab;" in flat
    # the strides are part of the signatures: member e's data at e * stride doubles
    want = {
        "sml_slab_create": ("sml_reservoirs *atmo", "sml_reservoirs *slab", "const double *d_base_sst",
                            "const double *d_sea_mask", "int timestep", "int timestep_slab", "double sst_bias",
                            "sml_slab **out"),
        "sml_slab_destroy": ("sml_slab *s",),
        "sml_slab_start": ("int member", "int64_t ov_stride"),
        "sml_slab_predict": ("int64_t t_next", "int64_t ov_stride", "int *predicted"),
        "sml_slab_sst": ("int64_t ov_stride", "int64_t fb_stride", "int *wrote"),
        "sml_slab_ring": ("int64_t t", "int64_t fb_stride"),
        "sml_slab_buffers": ("int64_t *sst_stride", "int64_t *ring_stride", "int64_t *fb_stride",
                             "int64_t *ov_stride"),
        "sml_slab_info": ("int *members", "int *exchange_width"),
        "sml_res_tile_feedback_members": ("int64_t g4_stride", "int64_t g2_stride", "const double *d_tisr",
                                          "int64_t fb_stride", "void *stream"),
        "sml_res_tile_tisr_field_members": ("const double *d_tisr_grid", "int64_t fb_stride", "void *stream"),
    }
    assert set(want) == set(NEW)
    for name, parts in want.items():
        args = _args(flat, name)
        for p in parts:
            assert p in args, (name, p)


def test_binding_signatures_match_the_header():
    """One ctypes argument per declared parameter, 64-bit where the header says int64_t."""
    import ctypes

    flat = _header()
    L = _lib.lib()
    for name in NEW:
        params = [p.strip() for p in _args(flat, name).split(",")]
        argtypes = getattr(L, name).argtypes
        assert len(argtypes) == len(params), name
        for p, a in zip(params, argtypes):
            if p.startswith("int64_t ") and "*" not in p:
                assert a is ctypes.c_int64, (name, p)
            elif p.startswith("int ") and "*" not in p:
                assert a is ctypes.c_int, (name, p)
            elif p.startswith("double ") and "*" not in p:
                assert a is ctypes.c_double, (name, p)


def test_fortran_binding_has_the_ensemble_slab():
    src = open(os.path.join(_lib.PKG_ROOT, "fortran", "sml_hip.f90")).read()
    bound = set(re.findall(r"bind\(C, name='(sml_[a-z0-9_]+)'\)", src))
    assert set(NEW) <= bound, set(NEW) - bound
