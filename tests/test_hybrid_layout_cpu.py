"""The hybrid loop's host arithmetic (csrc/sml_hybrid_layout.cpp) on a CPU:
tests/hybrid_layout_check.cpp, a stand-alone program, checks the calendar, the loop's
calendar, the exchange plan and the step's schedule -- built plain and as an ASan/UBSan
executable (nothing preloaded, nothing loaded into Python)."""
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
def test_hybrid_layout_check(tmp_path, variant):
    """The calendar: the known answers of tests/test_calendar.py with their dates, a month
    boundary, the February latch, and mod_calendar.f90 restated statement by statement over
    30 years from 1981, 1990 and 2000 at every 6 h step.  LoopCalendar: 6000 steps against
    direct calls in the loop's order with one latch, the two resets, the table's range
    refusal.  The exchange plan for 1, 6, 7, 288 and 1152 regions at every world up to 16 and
    at world = numregions, with its refusals.  LoopSchedule: all 384 combinations of its
    inputs against the loop's former inline expressions and the properties that make the
    in-kernel waits safe."""
    exe = tmp_path / ("hybrid_layout_check_" + variant)
    srcs = [os.path.join(HERE, "hybrid_layout_check.cpp"), os.path.join(CSRC, "sml_hybrid_layout.cpp"),
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
