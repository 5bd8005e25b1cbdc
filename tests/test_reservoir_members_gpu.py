"""Ensemble members of the reservoir layer (sml_res_set_members, sml_res_step_members,
sml_res_synchronize_members; csrc/sml_res_members.hpp): E states of every region
advanced through one stream of the weights.

References, for every member e:
  * a single-member context of the same weights, started from member e's state and fed
    member e's inputs through sml_res_step / sml_res_synchronize: outvecs and states
    bit for bit;
  * oracle.predict_f32 chained per member, within the project's tolerances
    (tests/test_reservoir_edges_gpu.py): state 1e-14 (t + 1) (1 + |x|), outvec
    1e-11 (1 + |outvec|).
Every case runs 3 chained steps with distinct per-member states, feedback and local
models, at E = T - 1 (when >= 2), T, T + 1 and 2 T + 1 with T from member_tile(); the
members' buffers are strided past the minimum and the outvec rows padded, the padding
holding a sentinel that must survive.  update_tile >= 2 and readout_tile >= 2 are asserted:
a shape that falls back to a tile of one member fails.
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from speedy_ml_amd import SmlError
from speedy_ml_amd._lib import check, lib, ptr
from test_reservoir_edges_gpu import OUT_TOL, X_TOL, _generic, _region_weights, _regular, _scaled, _weights

pytestmark = pytest.mark.gpu

STEPS = 3
SENTINEL = -1234.5678
LDS_MAX = 163840  # the MI355X's LDS per workgroup
REGION_LDS_MAX = 65536  # a per-region update stages x and u in LDS up to this size


# ------------------------------------------------------------------------------ inputs
def _inputs(ws, ncs, E, steps=STEPS, seed=11):
    """Distinct per-member start states x0[e][i], feedback fbs [steps, E, tot_fb] and
    local models lms [steps, E, nlocal, max(ncs, 1)]."""
    rng = np.random.default_rng([seed, E, len(ws), ncs])
    x0 = [[rng.random(w.n) - 0.5 for w in ws] for _ in range(E)]
    fbs = rng.standard_normal((steps, E, sum(w.ninp for w in ws)))
    lms = rng.standard_normal((steps, E, len(ws), max(ncs, 1)))
    return x0, fbs, lms


def _tile_sizes(res):
    """E = T - 1 (when >= 2), T, T + 1, 2 T + 1 for the readout's T at this shape."""
    res.set_members(32)
    T = res.member_tile()["readout_tile"]
    res.set_members(1)
    assert T >= 2, "the members readout fell back to one member per W_out load"
    return T, sorted({e for e in (T - 1, T, T + 1, 2 * T + 1) if e >= 2})


def _states(res, E):
    return [[res.get_state(i, member=e) for i in range(res.nlocal)] for e in range(E)]


# ------------------------------------------------------------------------------- forms
def _run_members(res, E, x0, fbs, lms, cuda, stream=None):
    """set_members(E), the members' states, then chained predict_members with every
    stride above its minimum: feedback rows 3 doubles longer, one spare region row per
    member in the local models and the outvecs, outvec rows 4 columns wider
    (set_outvec_ld).  seq[t] = (outvecs [E, nlocal, nout], states[e][i])."""
    import torch

    nl, nout, ncs, ld = res.nlocal, res.nout, res.ncs, res.nout + 4
    tot = int(res.fb_offsets[-1])
    res.set_members(E)
    assert res.members == E
    tile = res.member_tile()
    assert tile["update_tile"] >= 2 and tile["readout_tile"] >= 2, tile
    res.set_outvec_ld(ld)
    for e in range(E):
        for i in range(nl):
            res.set_state(i, x0[e][i], member=e)
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
        fb_back[:, :tot] = torch.from_numpy(fbs[t].copy()).to(cuda)
        if ncs:
            lm_back[:, :nl, :ncs] = torch.from_numpy(np.ascontiguousarray(lms[t, :, :, :ncs])).to(cuda)
        torch.cuda.synchronize()
        res.predict_members(fb_back, d_lm, d_ov, stream=stream)
        if stream is not None:
            stream.synchronize()
        torch.cuda.synchronize()
        ov = ov_back.cpu().numpy()
        assert (ov[:, nl:, :] == SENTINEL).all() and (ov[:, :, nout:] == SENTINEL).all(), \
            f"step {t}: the outvecs' padding was written"
        assert not (ov[:, :nl, :nout] == SENTINEL).any()
        seq.append((ov[:, :nl, :nout].copy(), _states(res, E)))
    return seq


def _run_single(res, x0e, fbs_e, lms_e, cuda):
    """The reference: chained sml_res_step on a single-member context from one member's
    state and inputs.  seq[t] = (outvecs [nlocal, nout], states[i])."""
    import torch

    assert res.members == 1
    for i in range(res.nlocal):
        res.set_state(i, x0e[i])
    ov = torch.full((res.nlocal, res.nout), float("nan"), dtype=torch.float64, device=cuda)
    seq = []
    for t in range(len(fbs_e)):
        dfb = torch.from_numpy(fbs_e[t].copy()).to(cuda)
        dlm = torch.from_numpy(np.ascontiguousarray(lms_e[t][:, :res.ncs])).to(cuda) if res.ncs else None
        res.predict(dfb, dlm, ov)
        torch.cuda.synchronize()
        seq.append((ov.cpu().numpy().copy(), [res.get_state(i) for i in range(res.nlocal)]))
    return seq


def _oracle_member(ws, x0e, fbs_e, lms_e, ncs, leak, unstandardize):
    offs = np.concatenate([[0], np.cumsum([w.ninp for w in ws])])
    xs = list(x0e)
    seq = []
    for t in range(len(fbs_e)):
        outs = []
        for i, w in enumerate(ws):
            out, xs[i] = oracle.predict_f32(w.rows, w.cols, w.vals, w.wcol, w.wval, w.wout,
                                            fbs_e[t, offs[i]:offs[i + 1]], lms_e[t, i] if ncs else None, xs[i], w.mean,
                                            w.std, chunk_speedy=ncs, leakage=leak, unstandardize=unstandardize)
            outs.append(out)
        seq.append((np.stack(outs), list(xs)))
    return seq


def _check_members(seq, E, single_of, oracle_of, what):
    """Every member of seq bitwise its single-member run, and within tolerance of its
    oracle chain (each figure printed before it is asserted)."""
    worst_x = worst_o = 0.0
    for e in range(E):
        base, ref = single_of(e), oracle_of(e)
        for t, (ov, xs) in enumerate(seq):
            np.testing.assert_array_equal(ov[e], base[t][0], err_msg=f"{what} member {e} step {t} outvecs")
            for i, x in enumerate(xs[e]):
                np.testing.assert_array_equal(x, base[t][1][i], err_msg=f"{what} member {e} step {t} region {i} state")
            eo = _scaled(ov[e], ref[t][0])
            ex = max(_scaled(x, rx) for x, rx in zip(xs[e], ref[t][1]))
            worst_o, worst_x = max(worst_o, eo), max(worst_x, ex / (t + 1))
            print(f"{what} member {e} step {t}: outvec scaled err {eo:.3e}, state {ex:.3e}")
            assert eo <= OUT_TOL, f"{what} member {e} step {t}: outvec scaled err {eo:.3e} > {OUT_TOL:.0e}"
            assert ex <= X_TOL * (t + 1), f"{what} member {e} step {t}: state scaled err {ex:.3e}"
    print(f"{what}: E = {E} bitwise the single-member runs; worst outvec {worst_o:.2e}, state / (t + 1) {worst_x:.2e}")


def _case(make, ws, ncs, leak, cuda, what, unstandardize=False, sizes=None, expect=None):
    """The whole contract for one context shape: at every E of the tile's edges (or the
    sizes given), members against single-member runs and the oracle."""
    T, tile_sizes = _tile_sizes(make())
    single = make()
    for E in sizes or tile_sizes:
        x0, fbs, lms = _inputs(ws, ncs, E)
        res = make()
        seq = _run_members(res, E, x0, fbs, lms, cuda)
        if expect:
            expect(res, E, T)
        single_of = functools.lru_cache(maxsize=None)(
            lambda e: _run_single(single, x0[e], fbs[:, e], lms[:, e], cuda))
        oracle_of = functools.lru_cache(maxsize=None)(
            lambda e: _oracle_member(ws, x0[e], fbs[:, e], lms[:, e], ncs, leak, unstandardize))
        _check_members(seq, E, single_of, oracle_of, f"{what} E {E}")
        res.close()


# ------------------------------------------------------------------ A. generic contexts
GENERIC = {
    # two regions of different n in one context; n across the 1024-row pass
    "n1_33_ncs0_nout8": dict(n=[1, 33], ninp=[3, 11], ncs=0, nout=8, leak=1.0, wdt="f32"),
    "n33_1025_ncs5_nout13": dict(n=[33, 1025], ninp=[3, 11], ncs=5, nout=13, leak=1 / 3, wdt="f32"),
    "n1025_33_ncs132_nout13_f64": dict(n=[1025, 33], ninp=[11, 3], ncs=132, nout=13, leak=1 / 3, wdt="f64"),
    "n1_1025_ncs132_nout8_f64": dict(n=[1, 1025], ninp=[3, 11], ncs=132, nout=8, leak=1.0, wdt="f64"),
    "n33_1025_ncs0_nout13_f64": dict(n=[33, 1025], ninp=[11, 3], ncs=0, nout=13, leak=1 / 3, wdt="f64"),
    "n1025_1_ncs5_nout8": dict(n=[1025, 1], ninp=[11, 3], ncs=5, nout=8, leak=1.0, wdt="f32"),
}


@pytest.mark.parametrize("case", list(GENERIC))
def test_generic_contexts(cuda, case):
    """Two regions of different n (1, 33, 1025: below, at and across the 1024-row pass),
    ninp 3 / 11, chunk_speedy 0 / 5 / 132, nout 8 and 13 (the 8-row readout, nout_pad 8 and
    16), leakage 1 and 1/3, fp32 and fp64 storage; A in ELL with an overflow list where
    n >= 3, W_in with a stored column."""
    s = GENERIC[case]
    ws = [_weights(n, p, s["ncs"], s["nout"], seed=i) for i, (n, p) in enumerate(zip(s["n"], s["ninp"]))]

    def expect(res, E, T):
        assert res.member_tile() == dict(update_tile=min(E, T), update_lds=True, readout_tile=min(E, T))

    _case(lambda: _generic(ws, s["ncs"], s["nout"], s["leak"], s["wdt"]), ws, s["ncs"], s["leak"], cuda, case,
          expect=expect)


def test_update_gathers_from_global_memory(cuda):
    """One region with n + ninp > 8192 (no LDS staging: update_lds == 0) and nout 8."""
    ncs, nout, leak = 5, 8, 1 / 3
    ws = [_weights(8161, 32, ncs, nout, seed=0)]

    def expect(res, E, T):
        assert res.member_tile() == dict(update_tile=min(E, T), update_lds=False, readout_tile=min(E, T))

    _case(lambda: _generic(ws, ncs, nout, leak), ws, ncs, leak, cuda, "n8161", expect=expect)


# ----------------------------------------------------------------------- B. T30 regions
T30 = ((0, False), (5, True), (1151, True))


@pytest.mark.parametrize("csr", [False, True], ids=["ell", "csr"])
def test_t30_regions_wide_readout(cuda, csr):
    """T30 regions (a pole, an sst region with an implicit W_in column, the last region)
    at n 1024: the 17-row readout with nout 136, chunk_speedy 132, every output
    unstandardized; A / W_in in ELL form and from the CSR copies alone."""
    ws = _region_weights(T30, 1024)
    leak = 1 / 3

    def make():
        res = _regular(ws, leak, csr=True) if csr else _regular(ws, leak)
        lay = res.ell_layout(1)
        assert (lay["a_width"] == 0 and not lay["win_ell"]) if csr else (lay["a_width"] > 0 and lay["win_ell"]), lay
        return res

    _case(make, ws, 132, leak, cuda, "T30 " + ("csr" if csr else "ell"), unstandardize=True)


def test_full_size_region_lds_bound_tile(cuda):
    """One region at its own n: the update's tile is what fits the device's LDS per
    workgroup (163840 // lds_region, capped by E and T); E = update_tile + 1 runs a
    second, partial tile."""
    ws = _region_weights(((5, True),), None)
    w = ws[0]
    lds_region = ((w.n + 1) // 2 * 2 + w.ninp) * 8
    assert lds_region <= REGION_LDS_MAX, "the full-size region no longer stages in LDS"
    probe = _regular(ws, 1.0)
    probe.set_members(32)
    tile = probe.member_tile()
    T = tile["readout_tile"]
    want = min(LDS_MAX // lds_region, T)
    assert tile == dict(update_tile=want, update_lds=True, readout_tile=T), (tile, lds_region)
    assert want >= 2
    probe.close()

    def expect(res, E, T):
        assert res.member_tile()["update_tile"] == min(LDS_MAX // lds_region, E, T)

    _case(lambda: _regular(ws, 1.0), ws, 132, 1.0, cuda, "full-size region", unstandardize=True, sizes=[want + 1],
          expect=expect)


# ------------------------------------------------------------------------ C. isolation
def _iso_setup():
    ncs, nout, leak = 5, 13, 1 / 3
    ws = [_weights(n, p, ncs, nout, seed=i) for i, (n, p) in enumerate(((33, 3), (1025, 11)))]
    return ws, ncs, nout, leak


def test_members_are_isolated(cuda):
    """A NaN in member 1's state of region 0 leaves every other member, and region 1 of
    member 1, bitwise the clean run; two members given identical inputs give identical
    bits; permuting the members permutes the results."""
    ws, ncs, nout, leak = _iso_setup()
    E = 3
    x0, fbs, lms = _inputs(ws, ncs, E)
    clean = _run_members(_generic(ws, ncs, nout, leak), E, x0, fbs, lms, cuda)
    bad = [[x.copy() for x in xe] for xe in x0]
    bad[1][0][0] = np.nan
    seq = _run_members(_generic(ws, ncs, nout, leak), E, bad, fbs, lms, cuda)
    for t in range(STEPS):
        for e in (0, 2):
            np.testing.assert_array_equal(seq[t][0][e], clean[t][0][e], err_msg=f"step {t} member {e}")
            for i in range(2):
                np.testing.assert_array_equal(seq[t][1][e][i], clean[t][1][e][i])
        np.testing.assert_array_equal(seq[t][0][1][1], clean[t][0][1][1], err_msg=f"step {t} member 1 region 1")
        np.testing.assert_array_equal(seq[t][1][1][1], clean[t][1][1][1])
        assert np.isnan(seq[t][1][1][0]).any() and np.isnan(seq[t][0][1][0]).any()  # and the NaN did propagate
    # members 0 and 2 given the same state and inputs
    twin_x = [x0[0], x0[1], x0[0]]
    twin_fb, twin_lm = fbs.copy(), lms.copy()
    twin_fb[:, 2], twin_lm[:, 2] = fbs[:, 0], lms[:, 0]
    seq = _run_members(_generic(ws, ncs, nout, leak), E, twin_x, twin_fb, twin_lm, cuda)
    for t in range(STEPS):
        np.testing.assert_array_equal(seq[t][0][2], seq[t][0][0])
        np.testing.assert_array_equal(seq[t][0][0], clean[t][0][0])
        for i in range(2):
            np.testing.assert_array_equal(seq[t][1][2][i], seq[t][1][0][i])
    # a permutation across the tile's edge
    perm = [2, 0, 1]
    seq = _run_members(_generic(ws, ncs, nout, leak), E, [x0[p] for p in perm], fbs[:, perm], lms[:, perm], cuda)
    for t in range(STEPS):
        for e, p in enumerate(perm):
            np.testing.assert_array_equal(seq[t][0][e], clean[t][0][p], err_msg=f"step {t} member {e} <- {p}")
            for i in range(2):
                np.testing.assert_array_equal(seq[t][1][e][i], clean[t][1][p][i])


# ---------------------------------------------------------------- D. synchronize_members
def test_synchronize_members(cuda):
    """4 blocks at member_stride > the packed feedback size: every member's state bitwise
    sml_res_synchronize's on a single-member context; a following predict_members
    continues from there, bitwise the single-member step."""
    import torch

    ws, ncs, nout, leak = _iso_setup()
    E, L = 3, 4
    x0, fbs, lms = _inputs(ws, ncs, E, steps=L + 1)
    res = _generic(ws, ncs, nout, leak)
    tot = int(res.fb_offsets[-1])
    res.set_members(E)
    for e in range(E):
        for i in range(res.nlocal):
            res.set_state(i, x0[e][i], member=e)
    back = torch.zeros((L, E, tot + 5), dtype=torch.float64, device=cuda)
    back[:, :, :tot] = torch.from_numpy(fbs[:L].copy()).to(cuda)
    d_in = back[:, :, :tot + 2]  # member_stride tot + 5, block stride E (tot + 5)
    assert d_in.stride(1) > tot
    res.synchronize_members(d_in, L)
    torch.cuda.synchronize()
    got = _states(res, E)
    single = _generic(ws, ncs, nout, leak)
    after = []
    for e in range(E):
        for i in range(single.nlocal):
            single.set_state(i, x0[e][i])
        single.synchronize(torch.from_numpy(np.ascontiguousarray(fbs[:L, e])).to(cuda), L)
        torch.cuda.synchronize()
        xs = [single.get_state(i) for i in range(single.nlocal)]
        for i in range(single.nlocal):
            np.testing.assert_array_equal(got[e][i], xs[i], err_msg=f"member {e} region {i}")
        ref = _oracle_member(ws, x0[e], fbs[:L, e], lms[:L, e], ncs, leak, False)
        ex = max(_scaled(x, rx) for x, rx in zip(xs, ref[-1][1]))
        print(f"synchronize member {e}: state scaled err {ex:.3e}")
        assert ex <= X_TOL * L
        after.append(_run_single(single, xs, fbs[L:, e], lms[L:, e], cuda)[0])
    seq = _run_members(res, E, got, fbs[L:], lms[L:], cuda)
    for e in range(E):
        np.testing.assert_array_equal(seq[0][0][e], after[e][0], err_msg=f"member {e}: the step after synchronize")
        for i in range(res.nlocal):
            np.testing.assert_array_equal(seq[0][1][e][i], after[e][1][i])


# ----------------------------------------------------------------------- E. the context
def test_set_members_keeps_member_zero_and_zeroes_the_rest(cuda):
    ws, ncs, nout, leak = _iso_setup()
    res = _generic(ws, ncs, nout, leak)
    assert res.members == 1 and res.member_tile() == dict(update_tile=1, update_lds=True, readout_tile=1)
    x0, fbs, lms = _inputs(ws, ncs, 3)
    res.set_members(3)
    for i, w in enumerate(ws):
        np.testing.assert_array_equal(res.get_state(i), w.x0)  # member 0 as loaded
        for e in (1, 2):
            assert (res.get_state(i, member=e) == 0).all()
            res.set_state(i, x0[e][i], member=e)
    res.set_members(2)  # shrinking drops member 2, keeps 0 and 1
    res.set_members(3)  # growing again: zeros
    for i, w in enumerate(ws):
        np.testing.assert_array_equal(res.get_state(i), w.x0)
        np.testing.assert_array_equal(res.get_state(i, member=1), x0[1][i])
        assert (res.get_state(i, member=2) == 0).all()
    # a member started from zero steps like a single-member context started from zero
    zero = [[w.x0 for w in ws], x0[1], [np.zeros(w.n) for w in ws]]
    seq = _run_members(res, 3, zero, fbs, lms, cuda)
    base = _run_single(_generic(ws, ncs, nout, leak), zero[2], fbs[:, 2], lms[:, 2], cuda)
    for t in range(STEPS):
        np.testing.assert_array_equal(seq[t][0][2], base[t][0])
    for bad in (0, -1, 33):
        with pytest.raises(SmlError, match="error -1: members"):
            res.set_members(bad)
    for i in (0, 1):
        with pytest.raises(SmlError, match="member 3 out of range"):
            res.get_state(i, member=3)
        with pytest.raises(SmlError, match="member -1 out of range"):
            res.set_state(i, x0[0][i], member=-1)
    assert res.members == 3


def test_single_member_calls_are_refused_while_members_are_held(cuda):
    """At E = 2 each single-member call that advances the state returns SML_ERR_STATE
    naming sml_res_set_members; after set_members(1) they work again, and the context
    steps bit for bit like one that never held members."""
    import torch

    ncs = nout = 8  # (sml_res_step_slab wants chunk_speedy == nout)
    leak = 1 / 3
    ws = [_weights(n, p, ncs, nout, seed=i) for i, (n, p) in enumerate(((33, 3), (1025, 11)))]
    x0, fbs, lms = _inputs(ws, ncs, 1)
    res = _generic(ws, ncs, nout, leak)
    res.set_members(2)
    tot = int(res.fb_offsets[-1])
    dfb = torch.from_numpy(fbs[0, 0].copy()).to(cuda)
    dlm = torch.from_numpy(np.ascontiguousarray(lms[0, 0])).to(cuda)
    dnext = torch.zeros_like(dlm)
    dov = torch.zeros((2, nout), dtype=torch.float64, device=cuda)
    dst = torch.zeros(3 * (sum(w.n for w in ws) + 2 * ncs), dtype=torch.float64, device=cuda)
    calls = {
        "sml_res_step": lambda: res.predict(dfb, dlm, dov),
        "sml_res_step_begin": lambda: res.predict_begin(dfb),
        "sml_res_step_slab": lambda: res.predict_slab(dfb, dlm, dnext, dov),
        "sml_res_synchronize": lambda: res.synchronize(dfb, 1),
        "sml_res_start_prediction": lambda: res.start_prediction(dfb, 0, torch.zeros(tot, dtype=torch.float64,
                                                                                   device=cuda)),
        "sml_res_train_drive": lambda: res.train_drive(dfb, 1, dlm, dst),
        "sml_res_step_host": lambda: res.predict_host(fbs[0, 0], lms[0, 0]),
    }
    for name, call in calls.items():
        with pytest.raises(SmlError, match=rf"error -4: {name} on a context of 2 members.*sml_res_set_members"):
            call()
    # what does not touch the state stays available
    lo, hi, _, _ = res.spectral_radius(max_iter=50)
    assert (lo <= hi).all() and (hi > 0).all()
    assert res.ell_layout(0)["a_width"] == 6
    res.set_members(1)
    for i in range(res.nlocal):
        res.set_state(i, x0[0][i])
    never = _generic(ws, ncs, nout, leak)
    seq = _run_single(res, x0[0], fbs[:, 0], lms[:, 0], cuda)
    base = _run_single(never, x0[0], fbs[:, 0], lms[:, 0], cuda)
    for t in range(STEPS):
        np.testing.assert_array_equal(seq[t][0], base[t][0])
        for i in range(res.nlocal):
            np.testing.assert_array_equal(seq[t][1][i], base[t][1][i])
    assert not np.isnan(seq[-1][0]).any()
    for call in list(calls.values())[:2]:  # and the others run: step, then begin + finish
        call()
    res.predict_finish(dlm, dov)
    res.synchronize(dfb, 1)
    res.predict_slab(dfb, dlm, dnext, dov)
    res.predict_host(fbs[0, 0], lms[0, 0])
    torch.cuda.synchronize()


def test_refusals(cuda):
    """Short strides and wrong shapes are refused -- by the Python class before the call,
    and by the library (SML_ERR_ARG) when called directly; set_members and
    predict_members inside a begun step are SML_ERR_STATE."""
    import torch

    ws, ncs, nout, leak = _iso_setup()
    res = _generic(ws, ncs, nout, leak)
    E, nl = 2, res.nlocal
    tot = int(res.fb_offsets[-1])
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=cuda)  # noqa: E731
    res.predict_begin(z(tot))
    with pytest.raises(SmlError, match="error -4: sml_res_set_members inside a begun step"):
        res.set_members(E)
    with pytest.raises(SmlError, match="error -4: sml_res_step_members inside a begun step"):
        res.predict_members(z(1, tot), z(1, nl, ncs), z(1, nl, nout))
    with pytest.raises(SmlError, match="error -4: sml_res_synchronize_members inside a begun step"):
        res.synchronize_members(z(1, 1, tot), 1)
    res.predict_finish(z(nl, ncs), z(nl, nout))
    res.set_members(E)
    fb, lm, ov = z(E, tot), z(E, nl, ncs), z(E, nl, nout)
    for args, msg in (((z(E, tot - 1), lm, ov), "d_feedback"), ((z(E + 1, tot), lm, ov), "d_feedback"),
                      ((fb, z(E, nl, ncs + 1), ov), "d_local_model"), ((fb, None, ov), "d_local_model"),
                      ((fb, lm, z(E, nl, nout + 1)), "d_outvec"), ((fb, lm, z(E, nl + 1, nout)), "d_outvec"),
                      ((fb, lm, z(E, nout, nl).transpose(1, 2)), "d_outvec"),
                      ((fb.float(), lm, ov), "d_feedback")):
        with pytest.raises(ValueError, match=msg):
            res.predict_members(*args)
    for d_in, length in ((z(2, E, tot - 1), 2), (z(1, E, tot), 2), (z(2, E + 1, tot), 2)):
        with pytest.raises(ValueError, match="d_inputs"):
            res.synchronize_members(d_in, length)
    L, st = lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = (tot, nl * ncs, nl * nout)
    for k, what in enumerate(("fb_stride", "lm_stride", "ov_stride")):
        strides = list(ok)
        strides[k] -= 1
        rc = L.sml_res_step_members(res.handle, ptr(fb), strides[0], ptr(lm), strides[1], ptr(ov), strides[2], st)
        assert rc == -1 and what.encode() in L.sml_last_error(), (rc, L.sml_last_error())
    assert L.sml_res_synchronize_members(res.handle, ptr(fb), 1, tot - 1, tot, st) == -1
    assert L.sml_res_synchronize_members(res.handle, ptr(fb), 1, 2 * tot, tot - 1, st) == -1
    assert L.sml_res_step_members(res.handle, ptr(fb), ok[0], ptr(lm), ok[1], ptr(ov), ok[2], st) == 0
    torch.cuda.synchronize()
    assert not np.isnan(ov.cpu().numpy()).any()


# ------------------------------------------------------------- F. streams and lifetime
def test_side_stream_and_lifetime(cuda):
    """A side stream gives bitwise the default stream's results; three create /
    set_members / step / destroy rounds run clean and agree."""
    import torch

    ws, ncs, nout, leak = _iso_setup()
    E = 5
    x0, fbs, lms = _inputs(ws, ncs, E)
    base = _run_members(_generic(ws, ncs, nout, leak), E, x0, fbs, lms, cuda)
    # a stream of the library's own over every CU, destroyed here: the process keeps the
    # streams and hardware queues it had (a stream of torch's pool would stay instantiated
    # and shift the queues of the contexts that later tests create)
    h = ctypes.c_void_p()
    check(lib().sml_stream_create_cu_range(0, torch.cuda.get_device_properties(cuda).multi_processor_count,
                                           ctypes.byref(h)))
    try:
        side = torch.cuda.ExternalStream(h.value, device=cuda)
        seq = _run_members(_generic(ws, ncs, nout, leak), E, x0, fbs, lms, cuda, stream=side)
        side.synchronize()
    finally:
        check(lib().sml_stream_destroy(h))
    for t in range(STEPS):
        np.testing.assert_array_equal(seq[t][0], base[t][0])
    for r in range(3):
        res = _generic(ws, ncs, nout, leak)
        res.enable_timing(STEPS)
        seq = _run_members(res, E, x0, fbs, lms, cuda)
        upd, rd = res.kernel_times()
        assert len(upd) == STEPS and len(rd) == STEPS and (upd > 0).all() and (rd > 0).all()
        res.close()
        for t in range(STEPS):
            np.testing.assert_array_equal(seq[t][0], base[t][0], err_msg=f"round {r} step {t}")
            for e in range(E):
                for i in range(2):
                    np.testing.assert_array_equal(seq[t][1][e][i], base[t][1][e][i])
