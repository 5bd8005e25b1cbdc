"""The slab ocean's host table unit (csrc/sml_slab_layout.cpp) on a CPU:
tests/slab_layout_check.cpp, a stand-alone program, builds the tables and compares every one
with its plain definition -- built plain and as an ASan/UBSan executable (nothing preloaded,
nothing loaded into Python)."""
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
def test_slab_layout_check(tmp_path, variant):
    """ring_src (the atmo_training_data_idx subset of the atmo feedback), row, the feedback's
    sst entries with their grid points and slab reservoirs, and the 48 x 96 table from a grid
    point to its region's exchange row and sst column, for single regions at both poles, at
    both ends of the longitude wrap and in the interior, a region without sst, a mixed list,
    the whole 1152 decomposition and a 288-region one; every grid point is covered exactly
    once; and each refusal (cadence, decomposition, ML-only, nout, the slab reservoirs' order,
    count, inputs and offsets, a region id out of range, null arguments) with its message."""
    exe = tmp_path / ("slab_layout_check_" + variant)
    srcs = [os.path.join(HERE, "slab_layout_check.cpp"), os.path.join(CSRC, "sml_slab_layout.cpp"),
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
