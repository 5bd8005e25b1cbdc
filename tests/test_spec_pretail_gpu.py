"""k_st_spec with the tail in two halves: tail_pre (the stage that reads the state and
the tables only) runs from the state staged in LDS ahead of specy -- beside the other
waves' loads of specy's Fourier operands -- and tail_post after the combine; specy's
Legendre columns and weights reach the waves through LDS.  tests/test_spec_kernel_gpu.py
pins the bits against the golden; this file checks what the new order could break.

 - repeatability: tail_pre reads every level's div and t straight from the LDS state
   that tail_post's timint later overwrites.  A read racing a later writer shows as a
   run-to-run difference, not as a fixed error, so the fused window (launched step by
   step and as a graph) is repeated 10 times from the same state and must give the same
   bits every time;
 - the stamped build (SML_DYN_STAMPS=1 at creation: extra block-wide barriers at the
   stamps) gives the bits of the unstamped one, and the per-m kernel's stamps are
   non-decreasing in every block that ran (chained steps 0..6, the last step 0..4);
 - the fused path (tail_pre + tail_post in k_st_spec) against the unfused one
   (set_fused(False): k_dyn_tail's tail_coef, whole) per variable and level at the
   project's FUSED_TOL, over step(1, 1, delt / 2), step(1, 2, delt), step(2, 2, 2 delt),
   a tendencies-only step(2, 2, 0) after them, and an explicit step (alph = 0).

All at T30L8 (the tables fix the grid) with two or three steps, from both inputs of
tests/golden/make_spec_kernel.py: the edge variant carries data at m == 0, n = 0,
n = 30 - m and on the top and bottom level.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
import make_spec_kernel as mk  # noqa: E402

pytestmark = pytest.mark.gpu

FUSED_TOL = 1e-11  # test_spec_kernel_gpu.py, test_row_kernel_shortwave_gpu.py, test_physics_gpu.py
REPEATS = 10
KX = 8


def _context(variant, fused=True, stamps=False):
    from speedy_ml_amd.dynamics import Dynamics

    st, forcing = mk.case_inputs(variant)
    if stamps:
        os.environ["SML_DYN_STAMPS"] = "1"
    try:
        d = Dynamics()
    finally:
        if stamps:
            del os.environ["SML_DYN_STAMPS"]
    d.set_fused(fused)
    d.set_forcing(**forcing)
    d.set_clock(1, True)
    return d, st


def _window(d, st, nleap, graph):
    import torch

    d.set_state(st)
    d.set_clock(1, True)
    d.window(nleap, graph=graph)
    torch.cuda.synchronize()
    out = dict(d.get_state())
    out["phi"] = d.get_phi()
    return out


@pytest.mark.parametrize("graph", [False, True], ids=["launched", "graph"])
def test_fused_window_repeats_bit_for_bit(cuda, graph):
    d, st = _context("edge")
    try:
        first = _window(d, st, 2, graph)
        for f, a in first.items():
            assert np.all(np.isfinite(a.view(np.float64))) and np.any(a != 0), f
        for rep in range(1, REPEATS):
            again = _window(d, st, 2, graph)
            for f, a in first.items():
                assert a.tobytes() == again[f].tobytes(), (f, rep, np.abs(a - again[f]).max())
    finally:
        d.close()


def test_stamped_context_same_bits_and_ordered_stamps(cuda):
    from speedy_ml_amd._lib import lib

    plain, st = _context("edge")
    stamped, _ = _context("edge", stamps=True)
    try:
        a = _window(plain, st, 3, True)
        b = _window(stamped, st, 3, True)
        for f in a:
            assert a[f].tobytes() == b[f].tobytes(), (f, np.abs(a[f] - b[f]).max())
        buf = np.zeros((4, 96, 8), dtype=np.int64)
        L = lib()
        L.sml_dbg_dyn_stamps.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        assert L.sml_dbg_dyn_stamps(stamped._h, buf.ctypes.data) == 0
    finally:
        plain.close()
        stamped.close()
    # kernel 1: the chained k_st_spec (stamps 0..6); kernel 3: the window's last (0..4)
    for kern, last in ((1, 6), (3, 4)):
        ran = buf[kern, :, 0] > 0
        assert int(ran.sum()) == 31, (kern, int(ran.sum()))  # the lead block of every m
        s = buf[kern, ran, :last + 1]
        assert np.all(np.diff(s, axis=1) >= 0), (kern, s[np.any(np.diff(s, axis=1) < 0, axis=1)])


def _close(x, y, what):
    x, y = np.asarray(x), np.asarray(y)
    err, bound = np.abs(x - y).max(), FUSED_TOL * max(np.abs(y).max(), 1e-300)
    assert err <= bound, (what, err, bound)


def _compare(f, u, what, tend):
    sf, su = f.get_state(), u.get_state()
    for v in mk.STATE:
        for lev in range(2):
            if v == "ps":
                _close(sf[v][lev], su[v][lev], (what, v, lev))
            else:
                for k in range(KX):
                    _close(sf[v][lev, k], su[v][lev, k], (what, v, lev, k))
    pf, pu = f.get_phi(), u.get_phi()
    for k in range(KX):
        _close(pf[k], pu[k], (what, "phi", k))
    if tend:  # [vor 8 | div 8 | t 8 | tr 8 | ps]; the fused path fills them for dt <= 0 only
        tf, tu = f.get_tendencies(), u.get_tendencies()
        for i in range(4 * KX + 1):
            assert np.any(tu[i] != 0), i
            _close(tf[i], tu[i], (what, "tend", i))


def _steps(variant, steps):
    import torch

    f, st = _context(variant, fused=True)
    u, _ = _context(variant, fused=False)
    try:
        for d in (f, u):
            d.set_state(st)
        for what, args, kw in steps:
            for d in (f, u):
                d.step(*args, **kw)
            torch.cuda.synchronize()
            _compare(f, u, what, tend=args[2] == 0.0)
    finally:
        f.close()
        u.close()


@pytest.mark.parametrize("variant", mk.VARIANTS)
def test_fused_steps_agree_with_whole_tail_coef(cuda, variant):
    from speedy_ml_amd.dynamics import DELT

    _steps(variant, [("forward half step", (1, 1, 0.5 * DELT), {}), ("first leapfrog", (1, 2, DELT), {}),
                     ("leapfrog", (2, 2, 2 * DELT), {}), ("tendencies only", (2, 2, 0.0), {})])


@pytest.mark.parametrize("variant", mk.VARIANTS)
def test_fused_explicit_steps_agree_with_whole_tail_coef(cuda, variant):
    """alph = 0: tail_post without implic (and without its barriers)."""
    from speedy_ml_amd.dynamics import DELT

    _steps(variant, [("explicit forward", (1, 1, 0.5 * DELT), {"alph": 0.0}),
                     ("explicit leapfrog", (2, 2, 2 * DELT), {"alph": 0.0}),
                     ("explicit tendencies only", (2, 2, 0.0), {"alph": 0.0})])
