"""The reservoir context's host layout unit (csrc/sml_reservoir_layout.cpp) on a CPU:
tests/reservoir_layout_check.cpp, a stand-alone program, packs regions, plans pools and
builds the index tables, and compares every vector with its plain definition -- built
plain and as an ASan/UBSan executable (nothing preloaded, nothing loaded into Python)."""
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
def test_reservoir_layout_check(tmp_path, variant):
    """A's ELL / overflow layout against its CSR rows and a byte count of the test's own,
    W_in's ELL / implicit-column choice and its CSR copy, W_out transposed and padded, the
    pool offsets, the balanced update's block table and the tile tables of a pole, a wrap
    and an interior region -- n = 1, the overflow words' edges, every width 1..9, k = 0,
    duplicates, four W_in forms, fp32 / fp64 storage from both sources, and the rejected
    loads' messages.  (Blocks of one row, q = 1, have no 32-bit magic -- ceil(2^32 / 1)
    wraps to 0 -- so the check pins that such a region keeps its stored columns.)
    Then step_shape (which kernel form each stage of a step takes, and its LDS) against
    the predicates as the launchers spelt them, with their numbers written out: maxn 7168 /
    7169, maxninp 1024 / 1025, the balanced and the drive LDS at max_lds (65536, 163840)
    and one row over, the per-region LDS at 64 KiB and 8 bytes over, nout_pad 136 / 153 /
    144, the grouped finish at ncs 133 / 134 / 0, nout_pad 144 / 148 and its switch, parts
    at nlocal 1 / 512 / 513, every begin mode, each reference-path flag alone, and 6000
    random inputs."""
    exe = tmp_path / ("reservoir_layout_check_" + variant)
    cmd = ["g++", "-std=gnu++17", "-ffp-contract=off", "-Wall", *VARIANTS[variant], "-I" + CSRC,
           os.path.join(HERE, "reservoir_layout_check.cpp"), os.path.join(CSRC, "sml_reservoir_layout.cpp"),
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
