"""GPU W_out training at its tile, nout and stream edges (csrc/sml_train.hip).

Gram / cross products against the np.longdouble product of the same fp64 inputs, every
element within the derived bound (m_total + batches + 1) 2^-53 (|S|^T |S|)_ij
(tests/_train_ref.py); the padding exactly zero.  Solves against the oracle within
test_training_gpu.py's W_TOL and under the normwise backward-error cap n 2^-53, the
residual in longdouble on the regularised system built in longdouble.  info at block
edges from an exactly zero pivot; a NaN stays in its region; a side stream gives the
default stream's bits.

Measured on the MI355X (profiles/training_edges.md): the Gram at most 0.33 of its bound
(m = 1; 0.04 over the 81 mixed steps), eta at most 1.7e-16 (the oracle's LU: 2.1e-16)
against caps of 1.4e-14 .. 7.1e-14."""
import functools

import numpy as np
import pytest

import _train_ref as ref
import oracle

pytestmark = pytest.mark.gpu

W_TOL = 1e-9  # test_training_gpu.py's: Cholesky against the oracle's LU, well conditioned


def _data(naugs, nout, m, seed=0):
    """test_training_gpu.py's distribution (132 unbounded "model" rows, then tanh of a
    normal), for regions of any naug."""
    rng = np.random.default_rng(seed)
    S, T = [], []
    for n in naugs:
        s = np.tanh(rng.standard_normal((m, n)))
        s[:, :132] = rng.standard_normal((m, min(132, n)))
        S.append(s)
        T.append(rng.standard_normal((m, nout)))
    return S, T


def _pack(arrs, cuda):
    import torch

    return torch.from_numpy(np.concatenate([a.ravel() for a in arrs])).to(cuda)


def _accumulate(tr, S, T, batches, cuda, stream=None):
    """One accumulate per entry of `batches` (time steps each); returns the device
    tensors, to be kept alive until the stream has run."""
    keep, t0 = [], 0
    for b in batches:
        s, t = _pack([x[t0:t0 + b] for x in S], cuda), _pack([x[t0:t0 + b] for x in T], cuda)
        keep.append((s, t))
        t0 += b
    if stream is not None:
        import torch

        torch.cuda.synchronize()  # the uploads (default stream) before the side stream reads them
    for (s, t), b in zip(keep, batches):
        tr.accumulate(s, t, int(b), stream=stream)
    return keep


def _check_gram(tr, S, T, batches, what):
    """Every region's G (lower triangle) and B within the element-wise bound; the padding
    rows and columns -- whole tiles past the region's live blocks among them -- exactly 0."""
    worst = 0.0
    for i, n in enumerate(tr.naug):
        G, B = tr.gram(i)  # G[c, r] = G(r, c), lower triangle (r >= c) valid; B[o, j]
        Gl, Bl, Ga, Ba = ref.products(S[i], T[i])
        low = np.tril(np.ones((n, n), dtype=bool))
        eg = ref.gram_excess(G[:n, :n].T[low], Gl[low], Ga[low], sum(batches), len(batches))
        eb = ref.gram_excess(B[:, :n].T, Bl, Ba, sum(batches), len(batches))
        worst = max(worst, eg, eb)
        assert eg <= 1.0 and eb <= 1.0, (what, i, n, eg, eb)
        assert not G[n:, :].any() and not G[:, n:].any(), (what, i, n)
        assert not B[:, n:].any(), (what, i, n)
        live = -(-n // 128) * 128
        assert not G[live:, :].any() and not G[:, live:].any() and not B[:, live:].any(), (what, i, n)
    print(f"{what}: Gram at {worst:.3f} of the element-wise bound")
    return worst


def _check_solve(tr, w, S, T, params, what):
    """W of every region against the oracle (W_TOL) and under the backward-error cap."""
    ncs = params[0]
    views = tr.wout_views(w)
    for i, n in enumerate(tr.naug):
        Go = np.zeros((n, n))
        Bo = np.zeros((n, tr.nout))
        oracle.train_accumulate(S[i], T[i], Go, Bo)
        wo, oinfo = oracle.train_solve(Go, Bo, *params)
        assert oinfo == 0
        got = views[i].cpu().numpy()
        assert np.abs(got - wo).max() <= W_TOL * np.abs(wo).max(), (what, i, n, np.abs(got - wo).max())
        Gr, Br = ref.regularised(*ref.sums(S[i], T[i]), *params)
        e, eo = ref.eta(Gr, Br, got), ref.eta(Gr, Br, wo)
        print(f"{what} naug {n} ncs {ncs}: eta {e:.3e}, oracle {eo:.3e}, cap {ref.eta_cap(n):.3e}")
        assert e <= ref.eta_cap(n), (what, i, n, e)


# ------------------------------------------------------------------ arguments
@pytest.mark.parametrize("naugs,nout", [([1], 136), ([200], 1), ([200], 145), ([0], 136)])
def test_create_rejects_one_row_operands(cuda, naugs, nout):
    """The Gram kernel loads operand rows in pairs: naug or nout of 1 (and the values
    out of range) are SML_ERR_ARG at sml_train_create, before any launch."""
    from speedy_ml_amd._lib import SmlError
    from speedy_ml_amd.training import Trainer

    with pytest.raises(SmlError):
        Trainer(naugs, nout)


# ------------------------------------------------------------------ Gram
EDGE_NAUGS = [2, 127, 128, 129, 133, 255, 256, 257, 383, 384]


@pytest.mark.parametrize("batches", [(1,), (16,), (48,), (16, 1, 17, 32, 15)], ids=lambda b: "m" + "+".join(map(str, b)))
def test_gram_tile_edges(cuda, batches):
    """Regions ending one short of, on and one past a 128-tile, one launch per batch:
    m = 16, 48 and the 16- and 32-step batches of the mixed run take the LDS-DMA path on
    the full tiles of the even regions, everything else the masked path; m = 1 and the
    1-, 17- and 15-step batches the time clamp; the mixed run changes m, and with it
    every region's offsets, at every call and sums all 81 steps."""
    from speedy_ml_amd.training import Trainer

    nout = 136
    S, T = _data(EDGE_NAUGS, nout, sum(batches), seed=41)
    tr = Trainer(EDGE_NAUGS, nout)
    assert tr.npad == 384
    keep = _accumulate(tr, S, T, batches, cuda)
    _check_gram(tr, S, T, batches, f"tile edges {batches}")
    tr.close()
    del keep


NOUTS = [2, 47, 48, 49, 96, 97, 127, 128, 129, 135, 144]
SWEEP_PARAMS = (100, 0.3, 1.0, True, 0.5)  # ncs, beta_res, beta_model, using_prior, prior_val


@pytest.mark.parametrize("nout", NOUTS)
def test_nout_sweep(cuda, nout):
    """The strip's rows and the solves' three column groups of 48 at their edges: the
    second strip tile row is live above nout = 128, the second and third column groups
    empty or partial at 47 .. 97; nout = 2 < ncs takes the prior's i < nout arm.  G and
    B within the bound at m = 32 (LDS-DMA where the tiles are full) and m = 33 (masked),
    then W against the oracle and under the backward-error cap."""
    from speedy_ml_amd.training import Trainer

    naugs = [130, 257]
    for m in (32, 33):
        S, T = _data(naugs, nout, m, seed=43 + m)
        tr = Trainer(naugs, nout)
        keep = _accumulate(tr, S, T, (m,), cuda)
        _check_gram(tr, S, T, (m,), f"nout {nout} m {m}")
        w, info = tr.solve(*SWEEP_PARAMS)
        assert (info == 0).all()
        _check_solve(tr, w, S, T, SWEEP_PARAMS, f"nout {nout} m {m}")
        tr.close()
        del keep


def test_gram_misaligned_states(cuda):
    """The states one double into their allocation: the LDS-DMA precondition (16-byte
    operand rows) fails on tiles that would take it, and the 8-byte-aligned masked
    path must give the sums within the same bound."""
    import torch

    from speedy_ml_amd.training import Trainer

    naugs, nout, m = [128, 256], 136, 32
    S, T = _data(naugs, nout, m, seed=47)
    flat = np.concatenate([a.ravel() for a in S])
    buf = torch.zeros(flat.size + 1, dtype=torch.float64, device=cuda)
    buf[1:] = torch.from_numpy(flat).to(cuda)
    targets = _pack(T, cuda)
    grams = []
    assert buf[1:].data_ptr() % 16 == 8
    for states in (buf[1:], _pack(S, cuda)):
        tr = Trainer(naugs, nout)
        tr.accumulate(states, targets, m)
        _check_gram(tr, S, T, (m,), f"states at {states.data_ptr() % 16} mod 16")
        grams.append([tr.gram(i) for i in range(len(naugs))])
        tr.close()
    same = all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(*grams))
    print(f"misaligned states: bitwise equal to the aligned run: {same}")


# ------------------------------------------------------------------ solve
LIVE_NAUGS = [128, 129, 133, 256, 383, 384, 640]
LIVE_PARAMS = [(100, 0.3, 1.0, True, 0.5), (0, 0.5, 1.0, False, 0.0), (128, 0.3, 1.0, True, 0.25)]


@functools.lru_cache(maxsize=None)
def _live_data():
    return _data(LIVE_NAUGS, 136, 200, seed=51)


@functools.lru_cache(maxsize=None)
def _live_sums():
    """Per region: the oracle's sums and the longdouble ones (shared by every case)."""
    S, T = _live_data()
    out = []
    for s, t in zip(S, T):
        n = s.shape[1]
        Go = np.zeros((n, n))
        Bo = np.zeros((n, 136))
        oracle.train_accumulate(s, t, Go, Bo)
        out.append((Go, Bo) + ref.sums(s, t))
    return out


@functools.lru_cache(maxsize=None)
def _live_reference(pi):
    """Per region: the oracle's W, the longdouble regularised system, the oracle's eta."""
    out = []
    for Go, Bo, Gl, Bl in _live_sums():
        wo, oinfo = oracle.train_solve(Go, Bo, *LIVE_PARAMS[pi])
        assert oinfo == 0
        Gr, Br = ref.regularised(Gl, Bl, *LIVE_PARAMS[pi])
        out.append((wo, Gr, Br, ref.eta(Gr, Br, wo)))
    return out


@pytest.mark.parametrize("panel", [None, 1, 2])
@pytest.mark.parametrize("pi", range(len(LIVE_PARAMS)), ids=["prior-ncs100", "noprior-ncs0", "prior-ncs128"])
def test_solve_live_blocks(cuda, pi, panel):
    """One to five live blocks in one batch of npad = 640, last blocks of 1, 5 and 127
    rows and whole ones: every skip on live_blocks and every rows mask runs beside a
    region that needs the block.  Panels of 8 (one panel), 1 (right-looking only, every
    trailing update) and 2 (fused in-panel steps, forked forward substitution)."""
    from speedy_ml_amd.training import Trainer

    S, T = _live_data()
    tr = Trainer(LIVE_NAUGS, 136)
    assert tr.npad == 640
    if panel is not None:
        tr.set_panel(panel)
    keep = _accumulate(tr, S, T, (100, 100), cuda)
    w, info = tr.solve(*LIVE_PARAMS[pi])
    assert (info == 0).all(), info
    views = tr.wout_views(w)
    for i, (n, (wo, Gr, Br, eo)) in enumerate(zip(LIVE_NAUGS, _live_reference(pi))):
        got = views[i].cpu().numpy()
        assert np.abs(got - wo).max() <= W_TOL * np.abs(wo).max(), (i, n, np.abs(got - wo).max())
        e = ref.eta(Gr, Br, got)
        print(f"live blocks panel {panel} params {pi} naug {n}: eta {e:.3e}, oracle {eo:.3e}, "
              f"cap {ref.eta_cap(n):.3e}")
        assert e <= ref.eta_cap(n), (i, n, e)
    tr.close()
    del keep


@pytest.mark.parametrize("panel", [None, 1])
def test_info_at_block_edges(cuda, panel):
    """An exactly zero pivot: column j of S zero and no regularisation there (beta_res =
    0, j >= ncs), so column j of G, every L_jk and the pivot are exact zeros, while the
    leading j x j minor is positive definite (m > naug).  info = j + 1 for the last
    pivot of a block, the first of the next, the last row of a partial last block, and
    in a region with fewer live blocks than the batch; the siblings report 0."""
    from speedy_ml_amd.training import Trainer

    naugs = [300, 300, 261, 130, 300, 129]
    zero = [127, 128, 260, 129, None, None]
    nout, m = 136, 400
    S, T = _data(naugs, nout, m, seed=53)
    for s, j in zip(S, zero):
        if j is not None:
            s[:, j] = 0.0
    tr = Trainer(naugs, nout)
    assert tr.npad == 384
    if panel is not None:
        tr.set_panel(panel)
    keep = _accumulate(tr, S, T, (m,), cuda)
    _, info = tr.solve(4, 0.0, 1.0, False, 0.0)
    assert list(info) == [0 if j is None else j + 1 for j in zero], info
    tr.close()
    del keep


def test_nan_stays_in_its_region(cuda):
    """One NaN in one region's states: that region reports info != 0, every other
    region's W is bitwise what it is without the NaN."""
    from speedy_ml_amd.training import Trainer

    naugs, nout, m = [200, 331, 130], 136, 400
    S, T = _data(naugs, nout, m, seed=57)
    ws = []
    for bad in (False, True):
        s1 = S[1].copy()
        if bad:
            s1[5, 7] = np.nan
        tr = Trainer(naugs, nout)
        keep = _accumulate(tr, [S[0], s1, S[2]], T, (m,), cuda)
        w, info = tr.solve(132, 0.3, 1.0, True, 0.5)
        assert info[0] == 0 and info[2] == 0 and (info[1] != 0) == bad, info
        ws.append([v.cpu().numpy().copy() for v in tr.wout_views(w)])
        tr.close()
        del keep
    assert np.array_equal(ws[0][0], ws[1][0]) and np.array_equal(ws[0][2], ws[1][2])
    assert np.isfinite(ws[0][1]).all()


# ------------------------------------------------------------------ streams
def test_side_stream_matches_default_stream(cuda):
    """reset, three accumulates and the solve (panels of two: the forward substitution
    forked to the context's stream and joined back) on a torch side stream -- a
    non-blocking stream -- give the default stream's W and info bit for bit.  The
    batches do not grow (334, 333, 333): see test_table_upload_under_a_running_launch."""
    import torch

    from speedy_ml_amd.training import Trainer

    naugs, nout = [777, 401, 640], 136
    S, T = _data(naugs, nout, 1000, seed=61)
    got = []
    for stream in (None, torch.cuda.Stream()):
        tr = Trainer(naugs, nout)
        tr.set_panel(2)
        torch.cuda.synchronize()  # the constructor's zero fill runs on the default stream
        tr.reset(stream=stream)
        keep = _accumulate(tr, S, T, (334, 333, 333), cuda, stream=stream)
        out = torch.empty(sum(naugs) * nout, dtype=torch.float64, device=cuda)
        torch.cuda.synchronize()
        w, info = tr.solve(132, 0.3, 1.0, True, 0.5, out=out, stream=stream)
        assert (info == 0).all()
        got.append((w.cpu().numpy().copy(), info.copy()))
        tr.close()
        del keep
    assert np.array_equal(got[0][1], got[1][1])
    assert np.array_equal(got[0][0], got[1][0])


def test_table_upload_under_a_running_launch(cuda):
    """accumulate with m = 1024, then at once with m = 256, on a side stream: the first
    launch (48 regions x 18 tiles = 864 workgroups, more than three rounds of what the
    chip holds) is still starting workgroups when the second call is made, and must see
    its own offsets.  Large, then small only: a workgroup that read the later call's
    (smaller) offsets with its own m would still read inside the first call's buffers.
    The reference is the same two calls with the stream synchronised between them."""
    import torch

    from speedy_ml_amd.training import Trainer

    nreg, naug, nout = 48, 512, 136
    gen = torch.Generator(device=cuda)
    gen.manual_seed(67)
    rn = lambda k: torch.randn(k, dtype=torch.float64, device=cuda, generator=gen)  # noqa: E731
    s1, t1, s2, t2 = rn(nreg * naug * 1024), rn(nreg * nout * 1024), rn(nreg * naug * 256), rn(nreg * nout * 256)
    tr = Trainer([naug] * nreg, nout)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    grams = []
    for sync_between in (True, False):
        tr.reset(stream=side)
        tr.accumulate(s1, t1, 1024, stream=side)
        if sync_between:
            side.synchronize()
        tr.accumulate(s2, t2, 256, stream=side)
        side.synchronize()
        grams.append([tr.gram(i) for i in (0, nreg // 2, nreg - 1)])
    tr.close()
    for (Ga, Ba), (Gb, Bb) in zip(*grams):
        assert np.array_equal(Ga, Gb) and np.array_equal(Ba, Bb)
