"""The ensemble products in the C ABI (include/speedy_ml.h): the built library exports the
sml_ens_* entry points, the header declares them with their member strides, the ctypes
binding's signatures match the header, the Fortran module binds them, and the ABI version is
unchanged.  CPU-only: the one call made is the host-only sml_ens_weights."""
import ctypes
import os
import re
import subprocess

import numpy as np

from speedy_ml_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("sml_ens_create", "sml_ens_destroy", "sml_ens_info", "sml_ens_reset", "sml_ens_moments", "sml_ens_scores",
       "sml_ens_read", "sml_ens_weights")


def _header():
    txt = open(os.path.join(REPO, "include", "speedy_ml.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"\s+", " ", txt)


def _args(flat, name):
    m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", flat)
    assert m, name
    return m.group(1)


def test_library_exports_the_ensemble_products():
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


def test_header_declares_the_ensemble_products():
    flat = _header()
    assert "typedef struct sml_ens sml_ens;" in flat
    members = ("const double *d_g4", "int64_t g4_stride", "const double *d_g2", "const double *d_pr",
               "int64_t g2_stride")
    want = {
        "sml_ens_create": ("int members", "int capacity_steps", "sml_ens **out"),
        "sml_ens_destroy": ("sml_ens *e",),
        "sml_ens_info": ("int *members", "int *capacity_steps", "int *fields", "int *scores_per_field",
                         "int *rank_bins"),
        "sml_ens_reset": ("sml_ens *e", "void *stream"),
        "sml_ens_moments": members + ("double *d_mean4", "double *d_mean2", "double *d_meanpr", "double *d_spread4",
                                      "double *d_spread2", "double *d_spreadpr", "void *stream"),
        "sml_ens_scores": members + ("const double *d_truth4", "const double *d_truth2", "const double *d_truthpr",
                                     "int t", "void *stream"),
        "sml_ens_read": ("int t0", "int count", "double *scores", "int32_t *ranks"),
        "sml_ens_weights": ("double *w48",),
    }
    assert set(want) == set(NEW)
    for name, parts in want.items():
        args = _args(flat, name)
        for p in parts:
            assert p in args, (name, p)
    assert "#define SML_RES_MAX_MEMBERS 32" in flat


def test_binding_signatures_match_the_header():
    """One ctypes argument per declared parameter, 64-bit where the header says int64_t."""
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
            elif "*" in p:
                assert a is not ctypes.c_int and a is not ctypes.c_int64, (name, p)


def test_fortran_binding_has_the_ensemble_products():
    src = open(os.path.join(_lib.PKG_ROOT, "fortran", "sml_hip.f90")).read()
    bound = set(re.findall(r"bind\(C, name='(sml_[a-z0-9_]+)'\)", src))
    assert set(NEW) <= bound, set(NEW) - bound


def test_weights_on_the_host():
    """sml_ens_weights needs no GPU: 48 row weights, 96 of each summing to 1, symmetric,
    growing from the poles to the equator; a NULL pointer is refused with its message."""
    L = _lib.lib()
    w = np.zeros(48)
    assert L.sml_ens_weights(w.ctypes.data_as(ctypes.c_void_p)) == 0
    assert abs(96.0 * w.sum() - 1.0) <= 48 * 2.0 ** -52
    assert np.array_equal(w, w[::-1])
    assert np.all(np.diff(w[:24]) > 0)
    assert L.sml_ens_weights(None) == -1
    assert b"null argument" in L.sml_last_error()
