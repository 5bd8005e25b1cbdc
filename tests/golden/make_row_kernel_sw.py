"""Generate tests/golden/row_kernel_sw.npz: this project's own output of the fused step
with GPU physics (the row kernel k_st_gridspec_p: grid-point dynamics, phypar's moist
part, and the longwave / surface chain with the shortwave on lane pairs) over a run
that holds shortwave steps, pinned bit for bit.

Run on the MI355X with the library built from the tree:

    python tests/golden/make_row_kernel_sw.py [output.npz]

The golden is NOT a reference result: it records what the row kernel computed when the
file was written, so that a change which only reorders the kernel's work (the same
operations on the same values) can be shown to leave every bit alone.  It was written
with the build of the commit BEFORE the pair lanes' shortwave path was split at the
moist side's hand-over barrier.  The device's exp / log / sqrt and the contraction of
a*b + c come from the compiler, so a toolchain change may move bits in both the old
and the new kernel: the file stores the `hipcc --version` string it was made with, and
after a toolchain change it has to be regenerated from a build WITHOUT the successor
edits of that split (check the split's commit out, revert the split in
sml_physics_pair.hpp / sml_dyn_fused.hpp, build, run this script), never from the
kernel under test.

A case (run_case): the seeded synthetic state dyn_state(SEED) with its spectral
humidity (both time levels) scaled by a factor of SCALES, synthetic boundary fields
(phys_boundary), zero radiation state, lradsw = .true.; then stepone (two steps, both
shortwave) and 6 leapfrog steps with stloop's clock (istep 1 and 4 are shortwave
steps), launched step by step.  The three factors give columns without cloud,
stratiform cloud tops at every level 3..7 and convective tops (the CPU oracle's count
per factor is in profiles/row_kernel_shortwave.md).

Stored per case c (0, 1, 2): the SHA-256 of every array of the final spectral state
(vor, div, t, tr, ps: both time levels) and of the radiation state (tau2, stratc,
tt_rsw, ssrd) -- the bitwise pin; the arrays themselves are 2.6 MB per case, past what
a committed fixture may hold -- and ps and ssrd in full, so that a mismatch can be
sized.
"""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(REPO, "speedy-ml-1_amd"),):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SEED = 1425
SCALES = (0.25, 1.0, 2.5)
NLEAP = 6
STATE = ("vor", "div", "t", "tr", "ps")
RAD = ("tau2", "stratc", "tt_rsw", "ssrd")
PATH = os.path.join(HERE, "row_kernel_sw.npz")


def case_inputs(scale: float):
    """(state, forcing) of the case with humidity factor `scale`."""
    from speedy_ml_amd.synthetic import dyn_state

    st, forcing = dyn_state(SEED)
    st["tr"] = st["tr"] * scale
    return st, forcing


def run_case(scale: float, fused: bool = True):
    """Final (state, radiation state) of the case on the GPU."""
    import torch

    from speedy_ml_amd.dynamics import Dynamics
    from speedy_ml_amd.synthetic import phys_boundary

    st, forcing = case_inputs(scale)
    d = Dynamics()
    try:
        d.set_fused(fused)
        d.set_forcing(**forcing)
        d.set_state(st)
        d.set_physics(phys_boundary(d, forcing["phis"]))
        d.set_rad_state(None)
        d.set_clock(1, True)
        d.window(NLEAP, graph=False)  # stepone, then NLEAP leapfrog steps from istep = 1
        torch.cuda.synchronize()
        assert d.get_clock() == (NLEAP + 1, False)
        state = d.get_state()
        rad = {k: np.array(v) for k, v in d.get_rad_state().items()}
    finally:
        d.close()
    return state, rad


def digest(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    out = {"hipcc_version": np.array(subprocess.run(["/opt/rocm/bin/hipcc", "--version"], check=True,
                                                    capture_output=True, text=True).stdout),
           "scales": np.array(SCALES), "seed": np.int64(SEED), "nleap": np.int64(NLEAP)}
    for c, scale in enumerate(SCALES):
        state, rad = run_case(scale)
        for k in STATE:
            assert np.all(np.isfinite(state[k].view(np.float64))), (scale, k)
            out[f"c{c}_sha_{k}"] = np.array(digest(state[k]))
        for k in RAD:
            assert np.all(np.isfinite(rad[k])), (scale, k)
            out[f"c{c}_sha_{k}"] = np.array(digest(rad[k]))
        out[f"c{c}_ps"] = state["ps"]
        out[f"c{c}_ssrd"] = rad["ssrd"]
        print(f"scale {scale}: ps {out[f'c{c}_sha_ps'].item()[:16]} tau2 {out[f'c{c}_sha_tau2'].item()[:16]} "
              f"ssrd max {rad['ssrd'].max():.3f}", flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
