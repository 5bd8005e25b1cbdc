"""member_finish (csrc/sml_reservoir_layout.cpp), the tile of the members' grid finish, on a
CPU: tests/reservoir_members_split_check.cpp, a stand-alone program, built plain and as an
ASan/UBSan executable exactly as test_reservoir_members_cpu.py builds its program (nothing
preloaded, nothing loaded into Python)."""
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
def test_reservoir_members_split_check(tmp_path, variant):
    """member_finish against its definition with the numbers written out: every E of
    1 .. 32 at the build's tile and at each tile a measurement may choose (1: the looped
    single-member kernel), E on both sides of the build's tile, the block's LDS per member
    (10112 bytes) within the 64 KiB of static LDS, 2000 random inputs."""
    exe = tmp_path / ("reservoir_members_split_check_" + variant)
    cmd = ["g++", "-std=gnu++17", "-ffp-contract=off", "-Wall", *VARIANTS[variant], "-I" + CSRC,
           os.path.join(HERE, "reservoir_members_split_check.cpp"), os.path.join(CSRC, "sml_reservoir_layout.cpp"),
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
