"""The native loop's slab ocean as a piece of state (sml_hybrid_set_slab / _start_slab /
_slab_buffers over the shared slab context, csrc/sml_slab.hip): the order refusals with their
messages, a restart that is bit for bit a fresh loop (also after new slab weights with another
sst mean / std), and create / destroy rounds that leave the device memory as it was.

The world is tests/test_ensemble_slab_gpu.py's (all 1152 regions at n 96, the 1027 slab
reservoirs at n 200, nleap 2, timestep_slab 24 h against 6 h: the 4th of five steps is a slab
step), on the overlapped loop with its default CU split and hops.  No tolerance anywhere.
The fresh loop's five steps are computed once and never modified."""
import ctypes

import numpy as np
import pytest

from test_ensemble_slab_gpu import CAL, KEYS, World

pytestmark = pytest.mark.gpu

STEPS = 5


@pytest.fixture(scope="module")
def world(cuda):
    w = World(cuda)
    w.fresh = None
    yield w
    w.close()


def _loop(w, dyn, slab=True):
    from speedy_ml_amd.exchange import OutvecExchange
    from speedy_ml_amd.hybrid import HybridLoop

    return HybridLoop(w.single, dyn, OutvecExchange(1152, 1, 0, device=w.cuda), w.cuda, tisr=w.tisr, nleap=2,
                      slab=w.ocean(w.sslab) if slab else None)


def _start(w, loop, slab=True):
    """The first inputs and the reservoirs' first states; the calendar (and with it the slab
    cadence's step count) from the beginning.  The feedback is the host's buffer: the start
    tiles all of it but the sst entries, which the first step's exchange writes after the
    first predict has read them, so the host hands them over as it did the first time, zero."""
    w.set_states(w.single, w.sslab, 0, member=0)
    loop.fb.zero_()
    loop.set_calendar(CAL[0], CAL[1], 6)
    loop.start(*w.grids(0))
    if slab:
        loop.start_slab(w.slab_start(0))


def _steps(loop, n=STEPS, slab=True):
    import torch

    snaps = []
    for _ in range(n):
        loop.step()
        loop.sync()
        torch.cuda.synchronize()
        assert loop.run_speedy()
        snap = {k: getattr(loop, k).cpu().numpy().copy() for k in KEYS}
        if slab:
            snap.update(loop.slab_state())
        snaps.append(snap)
    return snaps


def _fresh_run(w):
    import torch

    dyn = w.dynamics()
    loop = _loop(w, dyn)
    assert loop.exchange_width == 140
    _start(w, loop)
    snaps = _steps(loop)
    loop.close()
    dyn.close()
    torch.cuda.synchronize()
    return snaps


def _fresh(w):
    if w.fresh is None:
        w.fresh = _fresh_run(w)
        # a slab step falls inside: the slab outvecs are the start's until the 4th step
        ov = [s["outvec"] for s in w.fresh]
        assert np.array_equal(ov[0], ov[2]) and not np.array_equal(ov[2], ov[3]) and np.array_equal(ov[3], ov[4])
        assert np.isfinite(w.fresh[-1]["f4"]).all() and np.abs(w.fresh[-1]["f4"]).max() > 0
    return w.fresh


def _same(got, want, what, restarted=False):
    """Every buffer of every step.  The slab feedback is the slab step's scratch: written there
    before it is read, and until then whatever was left in it -- zero in a fresh loop, the last
    run's mean after a restart -- so after a restart it is compared from the slab step on."""
    assert len(got) == len(want)
    for s, (a, b) in enumerate(zip(got, want)):
        assert sorted(a) == sorted(b)
        for k in b:
            if k != "feedback" or not restarted or s >= 3:
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: step {s} {k}")


def _set_slab(w, h, timestep=6, timestep_slab=24):
    from speedy_ml_amd._lib import check, lib, ptr

    check(lib().sml_hybrid_set_slab(h, w.sslab.handle, ptr(w.d_base), ptr(w.d_mask), timestep, timestep_slab, 0.0))


def test_order_refusals_of_a_loop_with_a_slab(world):
    """sml_hybrid_set_slab twice, sml_hybrid_start_slab before sml_hybrid_start, a step before
    sml_hybrid_start_slab: each refused with its message; the loop then runs the fresh loop's
    five steps bit for bit."""
    import torch

    from speedy_ml_amd._lib import SmlError

    w = world
    want = _fresh(w)
    dyn = w.dynamics()
    loop = _loop(w, dyn)
    with pytest.raises(SmlError, match="the slab ocean is set already"):
        _set_slab(w, loop._h)
    with pytest.raises(SmlError, match="sml_hybrid_start first"):
        loop.start_slab(w.slab_start(0))
    _start(w, loop, slab=False)
    with pytest.raises(SmlError, match="sml_hybrid_start_slab first"):
        loop.step()
    with pytest.raises(SmlError, match="sml_hybrid_start_slab first"):
        loop.predict()
    _start(w, loop)
    _same(_steps(loop), want, "after the refusals")
    loop.close()
    dyn.close()
    torch.cuda.synchronize()


def test_order_refusals_of_a_loop_without_a_slab(world):
    """sml_hybrid_set_slab after sml_hybrid_set_buffers and sml_hybrid_slab_buffers without a
    slab are refused with their messages; the rows keep their 136 columns and the loop steps
    bit for bit as one that was never asked."""
    import torch

    from speedy_ml_amd._lib import SmlError, check, lib

    w = world
    w.single.set_outvec_ld(136)  # (the loops with a slab left the rows at 140)
    runs = []
    for ask in (False, True):
        dyn = w.dynamics()
        loop = _loop(w, dyn, slab=False)
        if ask:
            with pytest.raises(SmlError, match="must precede sml_hybrid_set_buffers"):
                _set_slab(w, loop._h)
            with pytest.raises(SmlError, match="no slab ocean in this loop"):
                check(lib().sml_hybrid_slab_buffers(loop._h, None, None, None, None, None))
        assert loop.exchange_width == 136
        _start(w, loop, slab=False)
        runs.append(_steps(loop, 2, slab=False))
        loop.close()
        dyn.close()
        torch.cuda.synchronize()
    _same(runs[1], runs[0], "after the refusals")
    assert np.isfinite(runs[0][-1]["f4"]).all() and np.abs(runs[0][-1]["ov"]).max() > 0


def test_a_refused_cadence_leaves_the_loop_without_a_slab(world):
    """A sml_hybrid_set_slab refused for its cadence leaves no slab behind (the rows keep 136
    columns, sml_hybrid_slab_buffers is refused); a correct call then succeeds and the rows
    widen to 140."""
    import torch

    from speedy_ml_amd._lib import SmlError, check, lib
    from speedy_ml_amd.dynamics import ALPH, DELT, ROB, WIL

    w, L = world, lib()
    dyn = w.dynamics()
    h, width = ctypes.c_void_p(), ctypes.c_int()
    check(L.sml_hybrid_create(w.single.handle, dyn._h, None, 2, DELT, ALPH, ROB, WIL, 1, 64, ctypes.byref(h)))
    try:
        for ts, tslab in ((6, 20), (6, 6), (0, 24)):
            with pytest.raises(SmlError, match="must be a multiple >= 2 of timestep"):
                _set_slab(w, h, ts, tslab)
            check(L.sml_hybrid_exchange_width(h, ctypes.byref(width)))
            assert width.value == 136
            with pytest.raises(SmlError, match="no slab ocean in this loop"):
                check(L.sml_hybrid_slab_buffers(h, None, None, None, None, None))
        _set_slab(w, h)
        check(L.sml_hybrid_exchange_width(h, ctypes.byref(width)))
        assert width.value == 140
        n = ctypes.c_int()
        check(L.sml_hybrid_slab_buffers(h, None, None, ctypes.byref(n), None, None))
        assert n.value > 0
        with pytest.raises(SmlError, match="the slab ocean is set already"):
            _set_slab(w, h)
    finally:
        check(L.sml_hybrid_destroy(h))
        w.single.set_outvec_ld(136)
        dyn.close()
        torch.cuda.synchronize()


def _second_run(w, fresh, between=lambda: None):
    """Five steps, `between`, then the first inputs again and five more steps: on the same loop
    (a restart) or, with `fresh`, on a new loop after the first is destroyed.  Both second runs
    meet the SPEEDY model where the same first five steps left it: a Dynamics carries state of
    its own from window to window, which is its host's and which neither a restart of the loop
    nor a new loop resets.  Returns the snapshots of both runs."""
    import torch

    dyn = w.dynamics()
    loop = _loop(w, dyn)
    _start(w, loop)
    first = _steps(loop)
    between()
    if fresh:
        loop.close()
        torch.cuda.synchronize()
        loop = _loop(w, dyn)
    _start(w, loop)
    second = _steps(loop)
    loop.close()
    dyn.close()
    torch.cuda.synchronize()
    return first, second


def test_restart_is_bitwise_a_fresh_loop(world):
    """Five steps across a slab step, then sml_hybrid_start and sml_hybrid_start_slab again
    with the first inputs and the reservoirs' first states: the next five steps give the
    outvecs, grids, feedback, forecasts, SST grid, ring, slab feedback and slab outvecs of a
    fresh loop.  The restart clears the ring and brings the slab outvecs back to the start's."""
    w = world
    want = _fresh(w)
    first, got = _second_run(w, fresh=False)
    _same(first, want, "the first run")
    first_b, fresh = _second_run(w, fresh=True)
    _same(first_b, want, "the first run of the other loop")
    _same(got, fresh, "after the restart", restarted=True)
    assert first[-1]["ring"][1:].any() and not got[0]["ring"][1:].any()
    np.testing.assert_array_equal(got[0]["outvec"], want[0]["outvec"])
    np.testing.assert_array_equal(got[0]["ov"], want[0]["ov"])  # (the first outvecs do not depend on a window)
    assert not np.array_equal(got[0]["outvec"], first[-1]["outvec"])


def test_restart_reads_the_slab_mean_and_std_again(world):
    """New weights with another sst mean and std for one slab reservoir, loaded between two
    starts: the restarted loop is bit for bit a fresh loop built with those weights, and its
    feedback's sst entries follow the new mean / std from the first step on."""
    import copy

    w = world
    j = w.sprobe[1]
    old = w.sws[j]
    new = copy.deepcopy(old)
    new.mean[35] += 1.5
    new.std[35] *= 1.25
    try:
        first, got = _second_run(w, fresh=False, between=lambda: w.sslab.load_region_weights(j, new))
        w.sslab.load_region_weights(j, old)
        _, fresh = _second_run(w, fresh=True, between=lambda: w.sslab.load_region_weights(j, new))
    finally:
        w.sslab.load_region_weights(j, old)
    _same(first, _fresh(w), "the first run")
    _same(got, fresh, "after new slab weights", restarted=True)
    # (the first step's feedback and SST grid do not depend on a window: the same tiles and
    # the same sst, standardized with another mean / std for that region's overlap tile)
    np.testing.assert_array_equal(got[0]["sst"], first[0]["sst"])
    differ = np.flatnonzero(got[0]["fb"] != first[0]["fb"])
    assert 1 <= len(differ) <= 16, len(differ)


def test_create_destroy_rounds_leave_the_device_memory(world):
    """The loop with a slab created, started, stepped and destroyed three times in one process:
    the device memory in use after the third destroy is what it was after the first."""
    import torch

    w = world
    dyn = w.dynamics()
    grids, sov = w.grids(0), w.slab_start(0)
    used = []
    for _ in range(3):
        loop = _loop(w, dyn)
        w.set_states(w.single, w.sslab, 0, member=0)
        loop.start(*grids)
        loop.start_slab(sov)
        loop.step()
        loop.sync()
        assert loop.run_speedy()
        loop.close()
        del loop
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info(w.cuda)
        used.append(total - free)
    dyn.close()
    assert used[2] == used[0] and used[1] == used[0], used
