"""The ensemble products' host unit (csrc/sml_ens_layout.cpp) on a CPU:
tests/ens_layout_check.cpp, a stand-alone program, checks the area weights, the field table,
the score tables' rows and every refusal -- built plain and as an ASan/UBSan executable
(nothing preloaded, nothing loaded into Python)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "speedy-ml-1_amd", "csrc")

VARIANTS = {
    "O2": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_ens_layout_check(tmp_path, variant):
    """The 48 row weights sum to 1 over the 4608 points within 48 ulp, are symmetric about the
    equator and grow from the pole to the equator as the cosine of sia's latitudes does; the
    34 fields' offsets cover every element of grid4d, logp and precip exactly once; the score
    and rank tables' row offsets at t = 0 and capacity - 1; and each refusal (members 0 and
    33, capacity 0, a short stride of each kind, t out of range, rows past the table, a truth
    half given, null grids) with its message."""
    exe = tmp_path / ("ens_layout_check_" + variant)
    srcs = [os.path.join(HERE, "ens_layout_check.cpp"), os.path.join(CSRC, "sml_ens_layout.cpp"),
            os.path.join(CSRC, "sml_tables.cpp")]
    flags = ["g++", "-std=gnu++17", "-ffp-contract=off", "-Wall", *VARIANTS[variant], "-I" + CSRC]
    b = subprocess.run(flags + srcs + ["-o", str(exe), "-lquadmath"], capture_output=True, text=True)
    if b.returncode != 0 and variant == "sanitized":
        for src in srcs:  # compiling alone must pass: only a failure of the sanitised *link* may skip
            subprocess.run(flags + ["-c", src, "-o", str(tmp_path / (os.path.basename(src) + ".o"))], check=True)
        pytest.skip("the sanitised link itself failed (no ASan/UBSan runtime for g++?): " + b.stderr[-400:])
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith(" 0 failed"), r.stdout[-2000:]
