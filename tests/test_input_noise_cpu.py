"""The input noise's definition on a CPU: sml_noise_bits -- the
device's own integer functions, host side -- against the NumPy uint64 restatement; the
stand-alone check program of the index packing, the refusals and the uniforms' ranges (plain
and under ASan/UBSan, nothing preloaded, nothing loaded into Python); sml_gen_region unchanged
by the generator's move into the shared header; the argument errors of the new calls that
need no device; and the moments of the restated normals at the seed the GPU test uses."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _noise_ref as nref
import _series_ref as ref
from speedy_ml_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "speedy-ml-1_amd", "csrc")
SML_ERR_ARG = -1

SEEDS = (0, 2 ** 64 - 1, 0x0123456789ABCDEF)
REGIONS = (0, 1151)
STEPS = (0, 1, 2 ** 43 - 1)
ENTRIES = (0, 2 ** 20 - 1)


def _lib_bits(seed, region, t, e):
    b1, b2 = ctypes.c_uint64(), ctypes.c_uint64()
    rc = _lib.lib().sml_noise_bits(seed, region, t, e, ctypes.byref(b1), ctypes.byref(b2))
    assert rc == 0, _lib.lib().sml_last_error()
    return b1.value, b2.value


def test_noise_bits_equal_the_numpy_restatement():
    seen = set()
    for seed in SEEDS:
        for region in REGIONS:
            for t in STEPS:
                for e in ENTRIES:
                    want = tuple(int(b[0]) for b in nref.bits(seed, region, t, e))
                    assert _lib_bits(seed, region, t, e) == want, (seed, region, t, e)
                    assert want[0] < 2 ** 53 and want[1] < 2 ** 53
                    seen.add(want)
    assert len(seen) == len(SEEDS) * len(REGIONS) * len(STEPS) * len(ENTRIES)  # no two corners collide
    # a block, vectorised, against the scalar calls
    b1, b2 = nref.block_bits(77, [245, 7], [5, 3], 10, 3)
    assert b1.shape == (3, 8)
    for c in range(3):
        for j, (r, e) in enumerate([(245, k) for k in range(5)] + [(7, k) for k in range(3)]):
            assert (int(b1[c, j]), int(b2[c, j])) == _lib_bits(77, r, 10 + c, e)


VARIANTS = {
    "O2": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_noise_bits_check(tmp_path, variant):
    """tests/noise_bits_check.cpp: the index packing, the refusals, the bits against a
    restatement in C++, u1 > 0 at b1 = 0 and u2 < 1 at b2 = 2^53 - 1."""
    exe = tmp_path / ("noise_bits_check_" + variant)
    cmd = ["g++", "-std=gnu++17", "-ffp-contract=off", "-Wall", *VARIANTS[variant], "-I" + CSRC,
           os.path.join(HERE, "noise_bits_check.cpp"), os.path.join(CSRC, "sml_genres.cpp"),
           os.path.join(CSRC, "sml_tables.cpp"), "-o", str(exe), "-lquadmath"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and variant == "sanitized":
        for src in cmd[-6:-3]:  # compiling alone must pass: only a failure of the sanitised *link* may skip
            subprocess.run(cmd[:-6] + ["-c", src, "-o", str(tmp_path / (os.path.basename(src) + ".o"))], check=True)
        pytest.skip("the sanitised link itself failed (no ASan/UBSan runtime for g++?): " + b.stderr[-400:])
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith(" 0 failed"), r.stdout[-2000:]


def test_gen_region_is_unchanged_by_the_shared_header():
    """Against arrays recorded from the commit before the generator moved (tests/golden/genres_seed.npz)."""
    z = np.load(os.path.join(HERE, "golden", "genres_seed.npz"))
    n, k, ninp, region = (int(v) for v in z["params"])
    rows, cols, vals = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.float32)
    wc, wv = np.zeros(n, np.int32), np.zeros(n, np.float32)
    rc = _lib.lib().sml_gen_region(n, k, ninp, int(z["seed"][0]), region, float(z["sigma"][0]), _lib.ptr(rows),
                                   _lib.ptr(cols), _lib.ptr(vals), _lib.ptr(wc), _lib.ptr(wv))
    assert rc == 0
    for name, got in (("rows", rows), ("cols", cols), ("vals", vals), ("win_col", wc), ("win_val", wv)):
        assert got.tobytes() == z[name].tobytes(), name


def test_new_calls_refuse_without_a_device():
    L = _lib.lib()
    buf = (ctypes.c_double * 4)()  # never dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in ("sml_res_train_drive_from", "sml_res_set_input_noise", "sml_res_input_noise", "sml_noise_bits"):
        assert name in _lib.EXPORTED and hasattr(L, name)
    # the setter: the magnitudes before the context
    for mag, word in ((-0.5, b"noisemag"), (float("nan"), b"noisemag"), (float("inf"), b"noisemag")):
        assert L.sml_res_set_input_noise(None, mag, 1, 0.0, None) == SML_ERR_ARG
        assert word in L.sml_last_error(), L.sml_last_error()
    for eps in (-1e-3, float("nan")):
        assert L.sml_res_set_input_noise(None, 0.1, 1, eps, None) == SML_ERR_ARG
        assert b"precip_epsilon" in L.sml_last_error()
    assert L.sml_res_set_input_noise(None, 0.1, 1, 0.0, None) == SML_ERR_ARG
    assert b"null reservoir context" in L.sml_last_error()
    # the launcher: m and the steps before the context
    for kw, word in ((dict(m=-1), b"m = -1"), (dict(t0=-1), b"2^43"), (dict(t0=2 ** 43), b"2^43"),
                     (dict(t0=2 ** 43 - 3, m=4), b"2^43"), (dict(), b"null reservoir context")):
        a = dict(t0=0, m=2)
        a.update(kw)
        assert L.sml_res_input_noise(None, p, 1 << 30, p, 1 << 30, a["t0"], a["m"], None) == SML_ERR_ARG, kw
        assert word in L.sml_last_error(), (kw, L.sml_last_error())
    # the drive
    assert L.sml_res_train_drive_from(None, p, 2, 1 << 30, p, 1 << 30, p, 1 << 30, p, p, None) == SML_ERR_ARG
    assert L.sml_res_train_drive_from(None, p, -1, 1 << 30, p, 1 << 30, p, 1 << 30, p, p, None) == SML_ERR_ARG
    # the bits
    b1, b2 = ctypes.c_uint64(), ctypes.c_uint64()
    for args, word in (((1, -1, 0, 0), b"region"), ((1, 0, -1, 0), b"2^43"), ((1, 0, 2 ** 43, 0), b"2^43"),
                       ((1, 0, 0, 2 ** 20), b"2^20"), ((1, 0, 0, -1), b"2^20")):
        assert L.sml_noise_bits(*args, ctypes.byref(b1), ctypes.byref(b2)) == SML_ERR_ARG, args
        assert word in L.sml_last_error(), (args, L.sml_last_error())
    assert L.sml_noise_bits(1, 0, 0, 0, None, ctypes.byref(b2)) == SML_ERR_ARG


def test_restated_normals_meet_the_moment_conditions_at_the_tests_seed():
    """The caps are conditions on the definition at a fixed seed, not chances: the NumPy
    restatement alone meets them here, and tests/test_input_noise_gpu.py asserts the same of
    the device's draws (which differ from these by the transcendental error only)."""
    ids = [r for r, _ in ref.CASES]
    off = ref.feedback_offsets(ref.CASES)
    ninps = np.diff(off)
    b1, b2 = nref.block_bits(nref.MOMENT_SEED, ids, ninps, nref.MOMENT_T0, nref.MOMENT_M)
    g, R = nref.normals_ld(b1, b2)
    N = g.size
    assert N >= 2 ** 18
    assert np.isfinite(g).all() and float(np.abs(g).max()) <= nref.G_MAX
    mean, var, re, rt = nref.moments(g.astype(np.float64), ninps)
    cm, cv, cr = nref.moment_caps(N)
    print(f"N {N}: mean {mean:+.3e} (cap {cm:.3e}), var - 1 {var - 1:+.3e} (cap {cv:.3e}), "
          f"lag-1 along e {re:+.3e}, along t {rt:+.3e} (cap {cr:.3e})")
    assert abs(mean) <= cm and abs(var - 1.0) <= cv and abs(re) <= cr and abs(rt) <= cr
