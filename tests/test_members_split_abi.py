"""The members' split step in the C ABI (include/speedy_ml.h): the built library exports
the five new entry points, the header declares them, and the ABI version is unchanged.
CPU-only: no compute call is made."""
import os
import re
import subprocess

from speedy_ml_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("sml_res_step_begin_members", "sml_res_step_finish_members", "sml_res_step_finish_grid_members",
       "sml_res_step_finish_assemble_members", "sml_res_member_finish_tile")


def test_library_exports_the_members_split():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (sml_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in exported, name
        assert hasattr(L, name), name
        assert name in _lib.EXPORTED, name
    assert L.sml_abi_version() == 1


def test_header_declares_the_members_split():
    txt = open(os.path.join(REPO, "include", "speedy_ml.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    flat = re.sub(r"\s+", " ", txt)
    for name in NEW:
        assert re.search(r"\bint " + name + r"\s*\(", flat), name
    # the strides are part of the signatures: member e's data at e * stride doubles
    m = re.search(r"sml_res_step_finish_assemble_members\s*\(([^;]*)\);", flat)
    for stride in ("fc4_stride", "fc2_stride", "lm_stride", "ov_stride", "g4_stride", "g2_stride"):
        assert "int64_t " + stride in m.group(1), stride
    assert "int64_t fb_stride" in re.search(r"sml_res_step_begin_members\s*\(([^;]*)\);", flat).group(1)


def test_fortran_binding_has_the_members_split():
    src = open(os.path.join(_lib.PKG_ROOT, "fortran", "sml_hip.f90")).read()
    bound = set(re.findall(r"bind\(C, name='(sml_[a-z0-9_]+)'\)", src))
    assert set(NEW[:4]) <= bound
