"""The slab training series' host table (build_slab_series_tables, slab_target_index:
csrc/sml_slab_layout.cpp) on a CPU: tests/slab_series_layout_check.cpp, a stand-alone
program, builds the table and compares every entry with its plain definition -- built plain
and as an ASan/UBSan executable (nothing preloaded, nothing loaded into Python)."""
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
def test_slab_series_layout_check(tmp_path, variant):
    """Every slab feedback entry's source in the series' index space, its mean / std slot and
    its local atmo row against the plain definition: single regions at both poles, at both
    ends of the longitude wrap and in the interior, a region without sst, a mixed list, all
    1152 regions, the shares of 8 and of 7 ranks, a 288-region decomposition; the slab's
    target positions for every region; and each refusal of build_slab_tables carried
    through, with the table's own (short or null series tables, null out)."""
    exe = tmp_path / ("slab_series_layout_check_" + variant)
    srcs = [os.path.join(HERE, "slab_series_layout_check.cpp"), os.path.join(CSRC, "sml_slab_layout.cpp"),
            os.path.join(CSRC, "sml_reservoir_layout.cpp"), os.path.join(CSRC, "sml_tables.cpp")]
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
