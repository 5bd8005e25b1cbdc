"""Generate tests/golden/spec_kernel.npz: this project's own output of the per-m
spectral kernels (k_st_spec, k_io_entry, k_st_inv and the unfused k_dyn_tail, which
share tail_coef / inv_inputs / uvspec_sel / gridy_m / gridy_io), pinned bit for bit on
the paths tests/golden/row_kernel_sw.npz does not reach.

Run on the MI355X with the library built from the tree:

    python tests/golden/make_spec_kernel.py [output.npz]

The golden is NOT a reference result: it records what these kernels computed when the
file was written, so that a change which only decides differently WHICH statements run
(the level index held wave-uniform, the level loops ended at the wave's level, specy's
operand guards dropped) can be shown to leave every bit alone.  It was written with the build of
the commit BEFORE that change, never by the kernels under test.  The contraction of
a*b + c comes from the compiler, so a toolchain change may move bits in both forms: the
file stores the `hipcc --version` string it was made with, and after a toolchain change
it has to be regenerated from a build of that earlier commit.

All cases are T30L8 (the tables fix the grid); the small dimension is the number of
steps.  Inputs (VARIANTS): dyn_state(SEED) as it is, and a variant with a fixed amplitude
added to the coefficients at the truncation edge of every m (n = 30 - m, the last n
inside the triangle, and n = 0; (m, n) = (0, 0), the global mean, is left alone) on
levels 1 and 8 of every variable and on ps, both time levels -- so the m == 0, first-n,
last-n, top-level and bottom-level branches all carry data of their own.  Case a, which
starts from a grid, takes another synthetic grid for the variant too.

 a  run_model from a grid, nleap = 2, GPU physics on: k_io_entry, the chained k_st_spec,
    the last step's next_j2 <= 0 path with io_varm (io_prep_m + gridy_io) and the exit.
    Stored: the forecast grids and the spectral state.
 b  window(2, graph=False) and window(2, graph=True), GPU physics off: nin == kNInv
    (inv_inputs without the level-1 fields), the last step without io_varm.
    Stored: the state and get_phi().
 c  b through the unfused path (set_fused(False)): k_dyn_tail's tail_coef.
 d  one step(1, 1, delt / 2), one step(2, 2, 2 delt), GPU physics on, launched alone
    through the fused path (k_state_to_m + k_st_inv in front, next_j2 = 0), then a
    step(2, 2, 0): the fused path fills the tendencies only for dt <= 0, so that third
    step is what get_tendencies() reads.  Stored: the state, phi and the tendencies.

Stored per run: the SHA-256 of every array (the bitwise pin), and ps of the final state
(both time levels) and the forecast logp in full, so that a mismatch can be sized.
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
VARIANTS = ("plain", "edge")
GRID_SEEDS = {"plain": 11, "edge": 5}
NLEAP = 2
STATE = ("vor", "div", "t", "tr", "ps")
# the edge variant's amplitude per variable: about the size of the state's largest
# wave coefficients
EDGE_AMP = {"vor": 2e-6, "div": 2e-7, "t": 0.5, "tr": 0.05, "ps": 2e-3}
PATH = os.path.join(HERE, "spec_kernel.npz")


def case_inputs(variant: str):
    """(state, forcing) of a variant, built on the CPU."""
    from speedy_ml_amd.synthetic import dyn_state

    st, forcing = dyn_state(SEED)
    if variant == "edge":
        for m in range(31):
            for n in {0, 30 - m}:
                if m == 0 and n == 0:
                    continue
                for f in STATE:
                    a = EDGE_AMP[f] * (1.0 if m == 0 else 1.0 + 1.0j)  # m = 0 is real
                    if f == "ps":
                        st[f][:, n, m] += a
                    else:
                        st[f][:, 0, n, m] += a
                        st[f][:, 7, n, m] += a
    else:
        assert variant == "plain"
    return st, forcing


def case_grids(variant: str):
    """run_model's input grid of a variant (a dry stratosphere, as tests/test_run_model_gpu.py)."""
    from speedy_ml_amd.synthetic import synthetic_grids

    g4, g2, _ = synthetic_grids(GRID_SEEDS[variant])
    g4[:2, ..., 3] = 0.0
    return g4, g2


def _context(variant: str, physics: bool, fused: bool):
    from speedy_ml_amd.dynamics import Dynamics
    from speedy_ml_amd.synthetic import phys_boundary

    st, forcing = case_inputs(variant)
    d = Dynamics()
    d.set_fused(fused)
    d.set_forcing(**forcing)
    d.set_state(st)
    if physics:
        d.set_physics(phys_boundary(d, forcing["phis"]))
        d.set_rad_state(None)
    d.set_clock(1, True)
    return d


def run_a(variant: str, fused: bool = True):
    """Case a: {fc4d, logp, state arrays} of run_model(nleap = NLEAP) with GPU physics."""
    import torch

    dev = torch.device("cuda:0")
    g4, g2 = case_grids(variant)
    d = _context(variant, True, fused)
    try:
        i4 = torch.from_numpy(np.ascontiguousarray(g4)).to(dev)
        i2 = torch.from_numpy(np.ascontiguousarray(g2)).to(dev)
        f4, f2 = torch.zeros_like(i4), torch.zeros_like(i2)
        d.run_model(i4, i2, f4, f2, nleap=NLEAP)
        safe, mm = d.last_safe()
        torch.cuda.synchronize()
        assert safe, mm
        out = {"fc4d": f4.cpu().numpy(), "logp": f2.cpu().numpy()}
        out.update(d.get_state())
    finally:
        d.close()
    return out


def run_b(variant: str, graph: bool, fused: bool = True):
    """Cases b (fused) and c (unfused): {state arrays, phi} of window(NLEAP), no GPU physics."""
    import torch

    d = _context(variant, False, fused)
    try:
        d.window(NLEAP, graph=graph)
        torch.cuda.synchronize()
        out = dict(d.get_state())
        out["phi"] = d.get_phi()
    finally:
        d.close()
    return out


def run_d(variant: str):
    """Case d: {state arrays, phi, tend} of single fused steps with GPU physics."""
    import torch

    from speedy_ml_amd.dynamics import DELT

    d = _context(variant, True, True)
    try:
        d.step(1, 1, 0.5 * DELT)
        d.step(2, 2, 2 * DELT)
        d.step(2, 2, 0.0)  # tendencies only
        torch.cuda.synchronize()
        out = dict(d.get_state())
        out["phi"] = d.get_phi()
        out["tend"] = d.get_tendencies()
    finally:
        d.close()
    return out


def runs(variant: str):
    """Every pinned run of a variant: {run name: {array name: array}}."""
    return {"a": run_a(variant), "b_nograph": run_b(variant, False), "b_graph": run_b(variant, True),
            "c_nograph": run_b(variant, False, fused=False), "c_graph": run_b(variant, True, fused=False),
            "d": run_d(variant)}


FULL = ("ps", "logp")  # stored in full beside their digests


def digest(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    out = {"hipcc_version": np.array(subprocess.run(["/opt/rocm/bin/hipcc", "--version"], check=True,
                                                    capture_output=True, text=True).stdout),
           "seed": np.int64(SEED), "nleap": np.int64(NLEAP), "variants": np.array(VARIANTS)}
    for variant in VARIANTS:
        for run, arrays in runs(variant).items():
            for k, a in arrays.items():
                a = np.asarray(a)
                real = a.view(np.float64) if np.iscomplexobj(a) else a
                assert np.all(np.isfinite(real)), (variant, run, k)
                assert np.any(real != 0.0), (variant, run, k)
                out[f"{variant}_{run}_sha_{k}"] = np.array(digest(a))
                if k in FULL:
                    out[f"{variant}_{run}_{k}"] = a
            print(f"{variant} {run}: " + " ".join(f"{k} {digest(a)[:12]}" for k, a in arrays.items()), flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
