"""The split step of the ensemble members (sml_res_step_begin_members, _finish_members,
_finish_grid_members, _finish_assemble_members; csrc/sml_res_members.hpp): every member's
update and v_ml in the begin, every member's v_p in one of three finishes.

References, for every member e:
  * predict_members (the one-pass step) on a twin context: outvecs and states bit for bit;
  * a single-member context of the same weights, started from member e's state and fed
    member e's inputs through predict_begin + predict_finish / _finish_grid /
    _finish_assemble: outvecs, local models, grids and states bit for bit;
  * oracle.predict_f32 chained per member, within the project's tolerances as
    tests/test_reservoir_members_gpu.py applies them (state 1e-14 (t + 1) (1 + |x|),
    outvec 1e-11 (1 + |outvec|)).
The members' buffers are strided past the minimum, the padding holding a sentinel that
must survive.
"""
import ctypes
import functools

import numpy as np
import pytest

from speedy_ml_amd import SmlError, domain
from speedy_ml_amd._lib import check, lib, ptr
from speedy_ml_amd.synthetic import region_weights, synthetic_grids
from test_reservoir_edges_gpu import CASES, _generic, _region_weights, _regular, _weights
from test_reservoir_members_gpu import (SENTINEL, STEPS, _check_members, _inputs, _oracle_member, _run_members,
                                        _states, _tile_sizes)

pytestmark = pytest.mark.gpu

N4, N2 = 8 * 48 * 96 * 4, 48 * 96


def _dev(a, cuda):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _set_states(res, x0, E):
    for e in range(E):
        for i in range(res.nlocal):
            res.set_state(i, x0[e][i], member=e)


# ------------------------------------------------------------------------------- forms
def _run_split(res, E, x0, fbs, lms, cuda, stream=None):
    """_run_members' layout (every stride above its minimum, outvec rows 4 columns wider)
    through chained begin_members + finish_members.  seq[t] = (outvecs, states[e][i])."""
    import torch

    nl, nout, ncs, ld = res.nlocal, res.nout, res.ncs, res.nout + 4
    tot = int(res.fb_offsets[-1])
    res.set_members(E)
    res.set_outvec_ld(ld)
    _set_states(res, x0, E)
    fb_back = torch.zeros((E, tot + 3), dtype=torch.float64, device=cuda)
    lm_back = torch.zeros((E, nl + 1, max(ncs, 1)), dtype=torch.float64, device=cuda)
    ov_back = torch.full((E, nl + 1, ld), SENTINEL, dtype=torch.float64, device=cuda)
    d_lm = lm_back[:, :nl, :ncs] if ncs else None
    d_ov = ov_back[:, :nl]
    if E > 1:
        assert fb_back.stride(0) > tot and d_ov.stride(0) > nl * ld
        assert d_lm is None or d_lm.stride(0) > nl * ncs
    seq = []
    for t in range(len(fbs)):
        fb_back[:, :tot] = _dev(fbs[t], cuda)
        if ncs:
            lm_back[:, :nl, :ncs] = _dev(lms[t, :, :, :ncs], cuda)
        torch.cuda.synchronize()
        assert not res.step_begun()
        res.begin_members(fb_back, stream=stream)
        assert res.step_begun()
        res.finish_members(d_lm, d_ov, stream=stream)
        assert not res.step_begun()
        if stream is not None:
            stream.synchronize()
        torch.cuda.synchronize()
        ov = ov_back.cpu().numpy()
        assert (ov[:, nl:, :] == SENTINEL).all() and (ov[:, :, nout:] == SENTINEL).all(), \
            f"step {t}: the outvecs' padding was written"
        assert not (ov[:, :nl, :nout] == SENTINEL).any()
        seq.append((ov[:, :nl, :nout].copy(), _states(res, E)))
    return seq


def _run_single_split(res, x0e, fbs_e, lms_e, cuda):
    """The reference: chained predict_begin + predict_finish on a single-member context
    from one member's state and inputs.  seq[t] = (outvecs, states[i])."""
    import torch

    assert res.members == 1
    for i in range(res.nlocal):
        res.set_state(i, x0e[i])
    ov = torch.full((res.nlocal, res.nout), float("nan"), dtype=torch.float64, device=cuda)
    seq = []
    for t in range(len(fbs_e)):
        dlm = _dev(lms_e[t][:, :res.ncs], cuda) if res.ncs else None
        res.predict_begin(_dev(fbs_e[t], cuda))
        res.predict_finish(dlm, ov)
        torch.cuda.synchronize()
        seq.append((ov.cpu().numpy().copy(), [res.get_state(i) for i in range(res.nlocal)]))
    return seq


def _same_members(a, b, E, what):
    for t, ((ov, xs), (bov, bxs)) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(ov, bov, err_msg=f"{what} step {t} outvecs")
        for e in range(E):
            for i, x in enumerate(xs[e]):
                np.testing.assert_array_equal(x, bxs[e][i], err_msg=f"{what} step {t} member {e} region {i} state")


# --------------------------------------------------------------- A. split equals one pass
# regions (33, 3) and (1025, 11); every pair of chunk_speedy 0 / 5 / 132 and nout 8 / 7 / 136
# (the 8-row readout at nout_pad 8, the 17-row readout at 136), both storage dtypes and
# leakage 1 and 1/3 spread over the pairs
SPLIT = {
    f"ncs{ncs}_nout{nout}_{wdt}_leak{'1' if leak == 1.0 else '3rd'}": dict(ncs=ncs, nout=nout, wdt=wdt, leak=leak)
    for k, (ncs, nout) in enumerate((c, o) for c in (0, 5, 132) for o in (8, 7, 136))
    for wdt, leak in [(("f32", "f64")[k % 2], (1.0, 1 / 3)[(k // 2) % 2])]
}


@pytest.mark.parametrize("case", list(SPLIT))
def test_split_equals_one_pass(cuda, case):
    """Three chained begin_members + finish_members at E = T - 1, T, T + 1, 2 T + 1: bit for
    bit predict_members on a twin context and predict_begin + predict_finish per member on a
    single-member context; within tolerance of the oracle's chain per member."""
    s = SPLIT[case]
    ncs, nout, leak, wdt = s["ncs"], s["nout"], s["leak"], s["wdt"]
    ws = [_weights(n, p, ncs, nout, seed=i) for i, (n, p) in enumerate(((33, 3), (1025, 11)))]
    make = lambda: _generic(ws, ncs, nout, leak, wdt)  # noqa: E731
    T, sizes = _tile_sizes(make())
    single = make()
    for E in sizes:
        x0, fbs, lms = _inputs(ws, ncs, E)
        res = make()
        seq = _run_split(res, E, x0, fbs, lms, cuda)
        assert res.member_tile()["readout_tile"] == min(E, T)
        twin = _run_members(make(), E, x0, fbs, lms, cuda)
        _same_members(seq, twin, E, f"{case} E {E} against predict_members")
        single_of = functools.lru_cache(maxsize=None)(
            lambda e: _run_single_split(single, x0[e], fbs[:, e], lms[:, e], cuda))
        oracle_of = functools.lru_cache(maxsize=None)(
            lambda e: _oracle_member(ws, x0[e], fbs[:, e], lms[:, e], ncs, leak, False))
        _check_members(seq, E, single_of, oracle_of, f"{case} E {E}")
        res.close()


# ------------------------------------------------------------------ B. finish from grids
EMAX_GRID = 9  # 2 TF + 1 at the largest tile the kernel is built for


@functools.lru_cache(maxsize=None)
def _grid_inputs(E):
    """Per member: start states, one feedback, forecast grids of its own."""
    ws = _region_weights(tuple(CASES), 1024)
    x0, fbs, _ = _inputs(ws, 132, E, steps=1, seed=23)
    fc = [synthetic_grids(100 + e)[:2] for e in range(E)]
    f4 = np.stack([np.ascontiguousarray(g4).reshape(8, 48, 96, 4) for g4, _ in fc])
    f2 = np.stack([np.ascontiguousarray(g2).reshape(48, 96) for _, g2 in fc])
    return ws, x0, fbs[0], f4, f2


@functools.lru_cache(maxsize=None)
def _grid_reference(cuda):
    """predict_begin + predict_finish_grid of a single-member context, per member: computed
    once for EMAX_GRID members, shared by every case (member e's inputs do not depend on E)."""
    import torch

    ws, x0, fb, f4, f2 = _grid_inputs(EMAX_GRID)
    res = _regular(ws, 1 / 3)
    out = []
    for e in range(EMAX_GRID):
        for i in range(res.nlocal):
            res.set_state(i, x0[e][i])
        ov = torch.full((res.nlocal, 136), float("nan"), dtype=torch.float64, device=cuda)
        lm = torch.full((res.nlocal, 132), float("nan"), dtype=torch.float64, device=cuda)
        res.predict_begin(_dev(fb[e], cuda))
        res.predict_finish_grid(_dev(f4[e], cuda), _dev(f2[e], cuda), lm, ov)
        torch.cuda.synchronize()
        out.append((ov.cpu().numpy(), lm.cpu().numpy(), [res.get_state(i) for i in range(res.nlocal)]))
        assert not np.isnan(out[-1][0]).any() and not np.isnan(out[-1][1]).any()
    res.close()
    return out


def _finish_tile(res):
    res.set_members(32)
    tf = res.member_finish_tile()
    res.set_members(1)
    return tf


@pytest.mark.parametrize("ungrouped", [False, True], ids=["grouped", "ungrouped"])
def test_finish_from_grids(cuda, ungrouped):
    """finish_grid_members on the T30 regions of CASES at n 1024, forecast grids distinct per
    member, E on both sides of the finish tile: outvecs and the written local models bit for
    bit a single-member predict_finish_grid per member; the same outvecs with d_local_model
    NULL; the grouped finish and SML_RES_PATH_UNGROUPED_FINISH."""
    import torch

    ws, x0, fb, f4, f2 = _grid_inputs(EMAX_GRID)
    ref = _grid_reference(cuda)
    make = lambda: _regular(ws, 1 / 3, ungrouped_finish=True) if ungrouped else _regular(ws, 1 / 3)  # noqa: E731
    res = make()
    TF = _finish_tile(res)
    assert TF >= 2, "the members' grid finish fell back to one member per block"
    assert 2 * TF + 1 <= EMAX_GRID
    nl = res.nlocal
    d_fb, d_f4, d_f2 = _dev(fb, cuda), _dev(f4, cuda), _dev(f2, cuda)
    for E in sorted({e for e in (TF - 1, TF, TF + 1, 2 * TF + 1) if e >= 2}):
        res.set_members(E)
        assert res.member_finish_tile() == min(E, TF)
        for with_lm in (True, False):
            _set_states(res, x0, E)
            ov = torch.full((E, nl + 1, 136), SENTINEL, dtype=torch.float64, device=cuda)
            lm = torch.full((E, nl + 1, 132), SENTINEL, dtype=torch.float64, device=cuda)
            res.begin_members(d_fb[:E])
            res.finish_grid_members(d_f4[:E], d_f2[:E], lm[:, :nl] if with_lm else None, ov[:, :nl])
            torch.cuda.synchronize()
            assert not res.step_begun()
            ovh, lmh = ov.cpu().numpy(), lm.cpu().numpy()
            assert (ovh[:, nl:] == SENTINEL).all(), "the outvecs' padding was written"
            assert (lmh[:, nl:] == SENTINEL).all() and (with_lm or (lmh == SENTINEL).all())
            for e in range(E):
                what = f"E {E} member {e} lm {with_lm}"
                np.testing.assert_array_equal(ovh[e, :nl], ref[e][0], err_msg=what + " outvecs")
                if with_lm:
                    np.testing.assert_array_equal(lmh[e, :nl], ref[e][1], err_msg=what + " local models")
                for i in range(nl):
                    np.testing.assert_array_equal(res.get_state(i, member=e), ref[e][2][i], err_msg=what + " state")
    res.close()


# ---------------------------------------------------- C. finish with assembly, isolation
E_WORLD = 3


@functools.lru_cache(maxsize=None)
def _world_weights():
    mask = domain.load_sst_mask()
    return [region_weights(r, bool(mask[r]), n_override=96, seed=5, climatology=True) for r in range(1152)]


def _world_context():
    from speedy_ml_amd.reservoir import Reservoirs

    ws = _world_weights()
    res = Reservoirs(list(range(1152)), [w.sst for w in ws], [w.n for w in ws], [w.k for w in ws])
    for i, w in enumerate(ws):
        res.load_region_weights(i, w)
    return res


@functools.lru_cache(maxsize=None)
def _world_inputs():
    ws = _world_weights()
    rng = np.random.default_rng(31)
    x0 = [[rng.random(w.n) - 0.5 for w in ws] for _ in range(E_WORLD)]
    fb = rng.standard_normal((E_WORLD, sum(w.ninp for w in ws)))
    fc = [synthetic_grids(200 + e)[:2] for e in range(E_WORLD)]
    f4 = np.stack([np.ascontiguousarray(a).reshape(8, 48, 96, 4) for a, _ in fc])
    f2 = np.stack([np.ascontiguousarray(b).reshape(48, 96) for _, b in fc])
    return x0, fb, f4, f2


def _members_assemble(res, x0, fb, f4, f2, cuda, pad4=7, pad2=5):
    """One begin_members + finish_assemble_members of all 1152 regions at E_WORLD members,
    the members' grids pad4 / pad2 doubles apart beyond their packed sizes.  Host copies of
    (ov, lm, g4, g2, pr) and the backing arrays of the grids."""
    import torch

    E, nl = E_WORLD, res.nlocal
    res.set_members(E)
    _set_states(res, x0, E)
    b4 = torch.full((E, N4 + pad4), SENTINEL, dtype=torch.float64, device=cuda)
    b2 = torch.full((E, N2 + pad2), SENTINEL, dtype=torch.float64, device=cuda)
    bp = torch.full((E, N2 + pad2), SENTINEL, dtype=torch.float64, device=cuda)
    g4 = torch.as_strided(b4, (E, 8, 48, 96, 4), (N4 + pad4, 48 * 96 * 4, 96 * 4, 4, 1))
    g2 = torch.as_strided(b2, (E, 48, 96), (N2 + pad2, 96, 1))
    pr = torch.as_strided(bp, (E, 48, 96), (N2 + pad2, 96, 1))
    ov = torch.full((E, nl, 136), SENTINEL, dtype=torch.float64, device=cuda)
    lm = torch.full((E, nl, 132), SENTINEL, dtype=torch.float64, device=cuda)
    res.begin_members(_dev(fb, cuda))
    res.finish_assemble_members(_dev(f4, cuda), _dev(f2, cuda), lm, ov, g4, g2, pr)
    torch.cuda.synchronize()
    h = lambda a: a.cpu().numpy()  # noqa: E731
    return dict(ov=h(ov), lm=h(lm), g4=h(b4), g2=h(b2), pr=h(bp))


@functools.lru_cache(maxsize=None)
def _world_clean(cuda):
    """The clean members run (kept for the isolation test) and its context."""
    res = _world_context()
    return res, _members_assemble(res, *_world_inputs(), cuda)


def test_finish_with_assembly(cuda):
    """All 1152 regions at n 96 in global order, E = 3: grids, outvecs and local models of
    finish_assemble_members bit for bit predict_finish_assemble of a single-member context per
    member; the sentinel between the members' grids (strides 7 and 5 doubles above the packed
    sizes) survives."""
    import torch

    x0, fb, f4, f2 = _world_inputs()
    _, got = _world_clean(cuda)
    for k, n in (("g4", N4), ("g2", N2), ("pr", N2)):
        assert (got[k][:, n:] == SENTINEL).all(), f"{k}: the padding between the members' grids was written"
        assert not (got[k][:, :n] == SENTINEL).any(), f"{k}: a grid point was not written"
    single = _world_context()
    for e in range(E_WORLD):
        for i in range(single.nlocal):
            single.set_state(i, x0[e][i])
        ov = torch.full((single.nlocal, 136), float("nan"), dtype=torch.float64, device=cuda)
        lm = torch.full((single.nlocal, 132), float("nan"), dtype=torch.float64, device=cuda)
        g4 = torch.full((8, 48, 96, 4), float("nan"), dtype=torch.float64, device=cuda)
        g2 = torch.full((48, 96), float("nan"), dtype=torch.float64, device=cuda)
        pr = torch.full((48, 96), float("nan"), dtype=torch.float64, device=cuda)
        single.predict_begin(_dev(fb[e], cuda))
        single.predict_finish_assemble(_dev(f4[e], cuda), _dev(f2[e], cuda), lm, ov, g4, g2, pr)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got["ov"][e], ov.cpu().numpy(), err_msg=f"member {e} outvecs")
        np.testing.assert_array_equal(got["lm"][e], lm.cpu().numpy(), err_msg=f"member {e} local models")
        np.testing.assert_array_equal(got["g4"][e, :N4], g4.cpu().numpy().ravel(), err_msg=f"member {e} grid4d")
        np.testing.assert_array_equal(got["g2"][e, :N2], g2.cpu().numpy().ravel(), err_msg=f"member {e} logp")
        np.testing.assert_array_equal(got["pr"][e, :N2], pr.cpu().numpy().ravel(), err_msg=f"member {e} precip")
        assert np.isfinite(got["ov"][e]).all()
    single.close()
    # the assembly needs every region on the rank
    part = _regular(_region_weights(tuple(CASES[:2]), 96), 1.0)
    part.set_members(2)
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=cuda)  # noqa: E731
    part.begin_members(z(2, int(part.fb_offsets[-1])))
    with pytest.raises(SmlError, match="error -1: the fused assembly needs every region"):
        part.finish_assemble_members(z(2, 8, 48, 96, 4), z(2, 48, 96), None, z(2, 2, 136), z(2, 8, 48, 96, 4),
                                     z(2, 48, 96), z(2, 48, 96))
    assert part.step_begun()
    part.close()


def test_members_are_isolated(cuda):
    """A NaN in member 1's forecast grid at a point that feeds region r: member 1's outputs
    of the regions that read it are NaN; every other member, and every region of member 1
    that does not read it, is bitwise the clean run."""
    x0, fb, f4, f2 = _world_inputs()
    res, clean = _world_clean(cuda)
    # a level-0 temperature point in the middle of the grid: the regions whose local model
    # reads it are those whose tiled local model changes to NaN
    bad4 = f4.copy()
    bad4[1, 0, 24, 48, 2] = np.nan
    got = _members_assemble(res, x0, fb, bad4, f2, cuda)
    hit = np.isnan(got["lm"][1]).any(axis=1)
    assert 1 <= hit.sum() < res.nlocal, f"{hit.sum()} regions read the point"
    assert np.isnan(got["ov"][1][hit]).any(axis=1).all(), "a region that read the NaN has finite outputs"
    np.testing.assert_array_equal(got["ov"][1][~hit], clean["ov"][1][~hit])
    np.testing.assert_array_equal(got["lm"][1][~hit], clean["lm"][1][~hit])
    for e in (0, 2):
        for k in ("ov", "lm", "g4", "g2", "pr"):
            np.testing.assert_array_equal(got[k][e], clean[k][e], err_msg=f"member {e} {k}")
    # member 1's grids differ only where its NaN outputs were scattered
    for k in ("g4", "g2", "pr"):
        diff = got[k][1] != clean[k][1]
        assert (np.isnan(got[k][1]) | (got[k][1] == clean[k][1]))[diff].all(), k


# ------------------------------------------------------------------- D. state machine
def _small():
    ncs, nout, leak = 5, 13, 1 / 3
    ws = [_weights(n, p, ncs, nout, seed=i) for i, (n, p) in enumerate(((33, 3), (1025, 11)))]
    return ws, ncs, nout, leak


def test_state_machine(cuda):
    """Misuse returns SML_ERR_STATE naming the call; cancel_step and set_state_member discard
    a begun members step; the partial sums follow set_members; E = 1 pairs with the
    single-member calls."""
    import torch

    ws, ncs, nout, leak = _small()
    E = 2
    x0, fbs, lms = _inputs(ws, ncs, 5)
    res = _generic(ws, ncs, nout, leak)
    nl, tot = res.nlocal, int(res.fb_offsets[-1])
    res.set_members(E)
    _set_states(res, x0, E)
    fb, lm = _dev(fbs[0, :E], cuda), _dev(lms[0, :E], cuda)
    ov = torch.zeros((E, nl, nout), dtype=torch.float64, device=cuda)
    with pytest.raises(SmlError, match="error -4: sml_res_step_finish_members without sml_res_step_begin_members"):
        res.finish_members(lm, ov)
    g4, g2 = torch.zeros((E, 8, 48, 96, 4), dtype=torch.float64, device=cuda), torch.zeros(
        (E, 48, 96), dtype=torch.float64, device=cuda)
    # (the grid finishes on a generic context are refused for their tables before the state is looked at:
    # their own state check is on the regular context below)
    res.begin_members(fb)
    with pytest.raises(SmlError, match="error -4: sml_res_step_begin_members called twice"):
        res.begin_members(fb)
    with pytest.raises(SmlError, match="error -4: sml_res_set_members inside a begun step"):
        res.set_members(3)
    with pytest.raises(SmlError, match="error -4: sml_res_step_members inside a begun step"):
        res.predict_members(fb, lm, ov)
    with pytest.raises(SmlError, match="error -4: sml_res_synchronize_members inside a begun step"):
        res.synchronize_members(fb[None], 1)
    # the single-member finishes at E = 2: refused, the step still begun
    with pytest.raises(SmlError, match="error -4: sml_res_step_finish on a context of 2 members"):
        res.predict_finish(lm[0], ov[0])
    assert res.step_begun()
    with pytest.raises(SmlError, match="error -4: sml_res_step_begin on a context of 2 members"):
        res.predict_begin(fb[0])
    assert res.step_begun()
    # --- cancel: every member's state is what it was; the next step equals a twin's
    res.cancel_step()
    assert not res.step_begun()
    for e in range(E):
        for i in range(nl):
            np.testing.assert_array_equal(res.get_state(i, member=e), x0[e][i], err_msg=f"member {e} region {i}")
    res.begin_members(fb)
    res.finish_members(lm, ov)
    torch.cuda.synchronize()
    twin = _generic(ws, ncs, nout, leak)
    twin.set_members(E)
    _set_states(twin, x0, E)
    ov2 = torch.zeros_like(ov)
    twin.begin_members(fb)
    twin.finish_members(lm, ov2)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ov.cpu().numpy(), ov2.cpu().numpy())
    for e in range(E):
        for i in range(nl):
            np.testing.assert_array_equal(res.get_state(i, member=e), twin.get_state(i, member=e))
    # --- set_state_member inside a begun step discards it
    before = _states(res, E)
    res.begin_members(fb)
    res.set_state(1, x0[1][1], member=1)
    assert not res.step_begun()
    np.testing.assert_array_equal(res.get_state(0, member=0), before[0][0])
    np.testing.assert_array_equal(res.get_state(1, member=1), x0[1][1])
    # --- set_members(2), a split step, set_members(5), a split step: members 0 and 1 as a twin's
    a, b = _generic(ws, ncs, nout, leak), _generic(ws, ncs, nout, leak)
    outs = {}
    for name, ctx, sizes in (("grown", a, (2, 5)), ("twin", b, (2, 2))):
        ctx.set_members(2)
        _set_states(ctx, x0, 2)
        outs[name] = []
        for t, n in enumerate(sizes):
            ctx.set_members(n)
            for e in range(2, n):
                for i in range(nl):
                    ctx.set_state(i, x0[e][i], member=e)
            o = torch.zeros((n, nl, nout), dtype=torch.float64, device=cuda)
            ctx.begin_members(_dev(fbs[t, :n], cuda))
            ctx.finish_members(_dev(lms[t, :n], cuda), o)
            torch.cuda.synchronize()
            outs[name].append((o.cpu().numpy()[:2], [[ctx.get_state(i, member=e) for i in range(nl)]
                                                     for e in range(2)]))
    _same_members(outs["grown"], outs["twin"], 2, "members 0 and 1 across set_members(5)")
    assert not np.isnan(outs["grown"][1][0]).any()
    # --- E = 1: the members calls are the single-member calls and pair with them
    want = _generic(ws, ncs, nout, leak)
    fb1, lm1 = _dev(fbs[0, 0], cuda), _dev(lms[0, 0], cuda)
    ov1 = torch.zeros((nl, nout), dtype=torch.float64, device=cuda)
    want.predict(fb1, lm1, ov1)
    torch.cuda.synchronize()
    base = (ov1.cpu().numpy().copy(), [want.get_state(i) for i in range(nl)])
    for mixed in ("begin_members + predict_finish", "predict_begin + finish_members"):
        one = _generic(ws, ncs, nout, leak)
        o = torch.zeros((1, nl, nout), dtype=torch.float64, device=cuda)
        if mixed.startswith("begin_members"):
            one.begin_members(fb1[None])
            assert one.step_begun()
            one.predict_finish(lm1, o[0])
        else:
            one.predict_begin(fb1)
            one.finish_members(lm1[None], o)
        torch.cuda.synchronize()
        assert not one.step_begun()
        np.testing.assert_array_equal(o.cpu().numpy()[0], base[0], err_msg=mixed)
        for i in range(nl):
            np.testing.assert_array_equal(one.get_state(i), base[1][i], err_msg=mixed)
        with pytest.raises(SmlError, match="error -4: sml_res_step_finish_members without"):
            one.finish_members(lm1[None], o)
    # --- the grid finishes: a regular context
    rws = _region_weights(tuple(CASES[:2]), 96)
    reg = _regular(rws, 1.0)
    reg.set_members(E)
    rov = torch.zeros((E, 2, 136), dtype=torch.float64, device=cuda)
    with pytest.raises(SmlError, match="error -4: sml_res_step_finish_grid_members without sml_res_step_begin_members"):
        reg.finish_grid_members(g4, g2, None, rov)
    reg.begin_members(torch.zeros((E, int(reg.fb_offsets[-1])), dtype=torch.float64, device=cuda))
    with pytest.raises(SmlError, match="error -4: sml_res_step_finish_grid on a context of 2 members"):
        reg.predict_finish_grid(g4[0], g2[0], None, rov[0])
    assert reg.step_begun()
    reg.finish_grid_members(g4, g2, None, rov)
    assert not reg.step_begun()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------ E. refusals
def test_refusals(cuda):
    """Each stride one short is SML_ERR_ARG naming it; short or mis-shaped tensors are a
    ValueError from the Python class before the call."""
    import torch

    E = 2
    reg = _regular(_region_weights(tuple(CASES[:2]), 96), 1.0)
    reg.set_members(E)
    nl, ncs, nout, tot = reg.nlocal, reg.ncs, reg.nout, int(reg.fb_offsets[-1])
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=cuda)  # noqa: E731
    fb, lm, ov = z(E, tot), z(E, nl, ncs), z(E, nl, nout)
    f4, f2, g4, g2, pr = z(E, 8, 48, 96, 4), z(E, 48, 96), z(E, 8, 48, 96, 4), z(E, 48, 96), z(E, 48, 96)
    L, st = lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def err(rc, what):
        assert rc == -1 and what.encode() in L.sml_last_error(), (what, rc, L.sml_last_error())

    err(L.sml_res_step_begin_members(reg.handle, ptr(fb), tot - 1, st), "fb_stride")
    assert not reg.step_begun()
    check(L.sml_res_step_begin_members(reg.handle, ptr(fb), tot, st))
    ok = dict(fc4=N4, fc2=N2, lm=nl * ncs, ov=nl * nout, g4=N4, g2=N2)
    for k in ("lm", "ov"):
        s = dict(ok)
        s[k] -= 1
        err(L.sml_res_step_finish_members(reg.handle, ptr(lm), s["lm"], ptr(ov), s["ov"], st), k + "_stride")
    for k in ("fc4", "fc2", "lm", "ov"):
        s = dict(ok)
        s[k] -= 1
        err(L.sml_res_step_finish_grid_members(reg.handle, ptr(f4), s["fc4"], ptr(f2), s["fc2"], ptr(lm), s["lm"],
                                               ptr(ov), s["ov"], st), k + "_stride")
    assert reg.step_begun()  # a refused finish leaves the step begun
    check(L.sml_res_step_finish_grid_members(reg.handle, ptr(f4), N4, ptr(f2), N2, None, 0, ptr(ov), ok["ov"], st))
    assert not reg.step_begun()
    # the assembly's strides on a context that holds every region (checked before the state)
    res, _ = _world_clean(cuda)
    assert res.members == E_WORLD
    wl, wov = z(E_WORLD, 1152, 132), z(E_WORLD, 1152, 136)
    w4, w2 = z(E_WORLD, 8, 48, 96, 4), z(E_WORLD, 48, 96)
    wok = dict(fc4=N4, fc2=N2, lm=1152 * 132, ov=1152 * 136, g4=N4, g2=N2)
    for k in wok:
        s = dict(wok)
        s[k] -= 1
        err(L.sml_res_step_finish_assemble_members(res.handle, ptr(w4), s["fc4"], ptr(w2), s["fc2"], ptr(wl), s["lm"],
                                                   ptr(wov), s["ov"], ptr(w4), s["g4"], ptr(w2), ptr(w2), s["g2"],
                                                   st), k + "_stride")
    # --- the Python class
    for args, msg in (((z(E, tot - 1),), "d_feedback"), ((z(E + 1, tot),), "d_feedback"), ((fb.float(),), "d_feedback"),
                      ((z(tot),), "d_feedback")):
        with pytest.raises(ValueError, match=msg):
            reg.begin_members(*args)
    for args, msg in (((z(E, nl, ncs + 1), ov), "d_local_model"), ((None, ov), "d_local_model"),
                      ((lm, z(E, nl, nout + 1)), "d_outvec"), ((lm, z(E, nl + 1, nout)), "d_outvec"),
                      ((lm, z(E, nout, nl).transpose(1, 2)), "d_outvec")):
        with pytest.raises(ValueError, match=msg):
            reg.finish_members(*args)
    for args, msg in (((z(E, 8, 48, 96, 3), f2, lm, ov), "d_fc4d"), ((z(E, 8, 48, 96), f2, lm, ov), "d_fc4d"),
                      ((f4, z(E, 48, 95), lm, ov), "d_fc2d"), ((f4, z(E + 1, 48, 96), lm, ov), "d_fc2d"),
                      ((f4, f2, z(E, nl, ncs - 1), ov), "d_local_model"), ((f4, f2, lm, z(E, nl, nout - 1)), "d_outvec")):
        with pytest.raises(ValueError, match=msg):
            reg.finish_grid_members(*args)
    for args, msg in (((f4, f2, lm, ov, z(E, 8, 48, 96, 5), g2, pr), "^g4:"), ((f4, f2, lm, ov, g4, z(E, 47, 96), pr), "^g2:"),
                      ((f4, f2, lm, ov, g4, g2, z(E, 48, 97)), "^pr:"),
                      ((f4, f2, lm, ov, g4, g2, z(E, 2, 48, 96)[:, 0]), "^pr:")):  # precip with another member stride
        with pytest.raises(ValueError, match=msg):
            reg.finish_assemble_members(*args)
    assert not reg.step_begun()
    torch.cuda.synchronize()


# --------------------------------------------------------------- F. pacing and streams
def test_pacing_and_streams(cuda):
    """set_read_waves(3) gives bitwise the uncapped results; a side stream gives bitwise the
    default stream's."""
    import torch

    ws, ncs, nout, leak = _small()
    E = 5
    x0, fbs, lms = _inputs(ws, ncs, E)
    base_res = _generic(ws, ncs, nout, leak)
    base_res.set_read_waves(0)
    base = _run_split(base_res, E, x0, fbs, lms, cuda)
    paced = _generic(ws, ncs, nout, leak)
    paced.set_read_waves(3)
    _same_members(_run_split(paced, E, x0, fbs, lms, cuda), base, E, "read_waves 3")
    # the 17-row readout too (nout 136: 8 items a region)
    wide = [_weights(n, p, ncs, 136, seed=i) for i, (n, p) in enumerate(((33, 3), (1025, 11)))]
    x0w, fbw, lmw = _inputs(wide, ncs, 3)
    runs = []
    for waves in (0, 3):
        r = _generic(wide, ncs, 136, leak)
        r.set_read_waves(waves)
        runs.append(_run_split(r, 3, x0w, fbw, lmw, cuda))
    _same_members(runs[1], runs[0], 3, "read_waves 3, wide readout")
    # a stream of the library's own over every CU, destroyed here (as the members test does)
    h = ctypes.c_void_p()
    check(lib().sml_stream_create_cu_range(0, torch.cuda.get_device_properties(cuda).multi_processor_count,
                                           ctypes.byref(h)))
    try:
        side = torch.cuda.ExternalStream(h.value, device=cuda)
        seq = _run_split(_generic(ws, ncs, nout, leak), E, x0, fbs, lms, cuda, stream=side)
        side.synchronize()
    finally:
        check(lib().sml_stream_destroy(h))
    _same_members(seq, base, E, "side stream")
    assert not np.isnan(base[-1][0]).any()
    assert STEPS == len(base)
