"""The series tables of the reservoir context's host layout unit (build_series_tables,
series_split in csrc/sml_reservoir_layout.cpp) on a CPU: tests/series_layout_check.cpp, a
stand-alone program, builds them and compares every entry with its plain definition --
built plain and as an ASan/UBSan executable (nothing preloaded, nothing loaded into Python)."""
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
def test_series_layout_check(tmp_path, variant):
    """Every feedback entry's source in the series' index space and its mean / std slot --
    the sst and tisr entries included -- and each region's input-tile points, for the
    regions of the GPU tests (both poles, both longitude wraps, interior with and without
    sst, neighbours) and for every region of the 1152-, 288- and 72-region decompositions;
    where the single-grid tables hold an entry the two agree.  Then the statistics' split of
    T = 1 .. 5000 steps into chunks."""
    exe = tmp_path / ("series_layout_check_" + variant)
    cmd = ["g++", "-std=gnu++17", "-ffp-contract=off", "-Wall", *VARIANTS[variant], "-I" + CSRC,
           os.path.join(HERE, "series_layout_check.cpp"), os.path.join(CSRC, "sml_reservoir_layout.cpp"),
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
