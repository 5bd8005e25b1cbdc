"""The training drive (sml_res_train_drive, k_res_drive): reservoir states, model rows
and targets for the W_out fit, "record, then advance" (reservoir_layer_chunking_hybrid,
src/mod_reservoir.f90:1065-1173, with chunking_matmul's first lines, :1662-1675).

Column c of a region's state block is [model block c; x~] with x~ the state before
input c, its 0-based odd nodes squared; column c of its targets is the region's own
points of input c; then the state advances on input c.  The state arithmetic is the
update's own row expression, so every comparison with sml_res_synchronize is bitwise;
against the oracle the state tolerance is the project's X_TOL = 1e-14 per update
(tanh: device vs glibc).
"""
import functools

import numpy as np
import pytest

import oracle
from speedy_ml_amd import SmlError
from speedy_ml_amd.synthetic import initial_state, local_model_vector, region_weights

pytestmark = pytest.mark.gpu

X_TOL = 1e-14
OUT_TOL = 1e-11
W_TOL = 1e-9
NCS = 132
NOUT = 136

# the four shape classes (n 5880, 5760, 6048, 6160 at full size), both polar rows
CASES = [(0, False), (5, True), (23, True), (24, False), (30, False)]
M = 7


def _context(cases, n_override=None, weight_dtype="f32", chunk_speedy=NCS, dense_win=None, seed=1234):
    from speedy_ml_amd.reservoir import Reservoirs

    ws = [region_weights(r, s, seed=seed, n_override=n_override, chunk_speedy=chunk_speedy) for r, s in cases]
    if dense_win is not None:  # one region with every W_in entry nonzero (the reference's matmul, :1443)
        rng = np.random.default_rng(4)
        ws[dense_win].win[:] = (0.02 * (2.0 * rng.random(ws[dense_win].win.shape) - 1.0)).astype(np.float32)
    res = Reservoirs([w.region for w in ws], [w.sst for w in ws], [w.n for w in ws], [w.k for w in ws],
                     chunk_speedy=chunk_speedy, weight_dtype=weight_dtype)
    for i, w in enumerate(ws):
        res.load_region_weights(i, w)
        res.set_state(i, initial_state(w.region, w.n))
    return res, ws


def _series(res, m, seed=11, pad_in=3, pad_model=5):
    """m input blocks and m model blocks with padded strides; the padding is NaN, so a
    read past a block shows."""
    tot = int(res.fb_offsets[-1])
    stride, mstride = tot + pad_in, res.nlocal * res.ncs + pad_model
    rng = np.random.default_rng(seed)
    inputs = np.full((m, stride), np.nan)
    inputs[:, :tot] = rng.standard_normal((m, tot))
    model = np.full((m, mstride), np.nan)
    model[:, :res.nlocal * res.ncs] = 2.0 * rng.random((m, res.nlocal * res.ncs)) - 1.0
    return inputs, model


def _drive(res, inputs, model, m, cuda, targets=True, first=0):
    """One drive call over blocks first .. first + m - 1; per region the state block as
    (m, ncs + n) and the target block as (m, nout) (C order of the column-major blocks).
    The buffers start as NaN: an entry the drive does not write shows."""
    import torch

    naug = [res.ncs + int(n) for n in res.n]
    d_in = torch.from_numpy(inputs[first:first + m].copy()).to(cuda)
    d_mo = torch.from_numpy(model[first:first + m].copy()).to(cuda) if res.ncs else None
    d_s = torch.full((sum(naug) * m,), float("nan"), dtype=torch.float64, device=cuda)
    d_t = torch.full((res.nlocal * m * res.nout,), float("nan"), dtype=torch.float64, device=cuda) if targets else None
    res.train_drive(d_in, m, d_mo, d_s, d_t, stride=inputs.shape[1], model_stride=model.shape[1])
    torch.cuda.synchronize()
    s, t = d_s.cpu().numpy(), (d_t.cpu().numpy() if targets else None)
    S, T, off = [], [], 0
    for i, na in enumerate(naug):
        S.append(s[off:off + na * m].reshape(m, na))
        off += na * m
        if targets:
            T.append(t[i * m * res.nout:(i + 1) * m * res.nout].reshape(m, res.nout))
    return S, T


def _stepwise_states(res, inputs, m, cuda):
    """The states before each of the m inputs and after the last, from
    synchronize(length=1) on a context of its own: xs[c][i], c = 0 .. m."""
    import torch

    d_in = torch.from_numpy(inputs.copy()).to(cuda)
    xs = [[res.get_state(i) for i in range(res.nlocal)]]
    for c in range(m):
        res.synchronize(d_in[c], 1, stride=inputs.shape[1])
        xs.append([res.get_state(i) for i in range(res.nlocal)])
    return xs


def _squared(x):
    xt = x.copy()
    xt[1::2] = x[1::2] * x[1::2]
    return xt


@functools.lru_cache(maxsize=None)
def _reference(n_override):
    """Shared by the n_override cases: the series and the stepwise states (read only)."""
    import torch

    res, ws = _context(CASES, n_override=n_override)
    inputs, model = _series(res, M)
    xs = _stepwise_states(res, inputs, M, torch.device("cuda:0"))
    for a in (inputs, model):
        a.setflags(write=False)
    return inputs, model, xs


def _check_columns(res, S, T, inputs, model, xs, m, first=0):
    o = res.fb_offsets
    for i in range(res.nlocal):
        for c in range(m):
            np.testing.assert_array_equal(S[i][c, res.ncs:], _squared(xs[first + c][i]), err_msg=f"region {i} col {c}")
            np.testing.assert_array_equal(S[i][c, :res.ncs], model[first + c, i * res.ncs:(i + 1) * res.ncs])
            if T:
                np.testing.assert_array_equal(T[i][c], inputs[first + c, o[i] + res.target_index(i)])


@pytest.mark.parametrize("n_override", [700, 1500])
def test_drive_is_bitwise_the_stepwise_update(cuda, n_override):
    """One partial 1024-row pass (n_override 700) and two passes (1500), padded strides."""
    inputs, model, xs = _reference(n_override)
    res, ws = _context(CASES, n_override=n_override)
    assert (max(res.n) <= 1024) == (n_override == 700)
    S, T = _drive(res, inputs, model, M, cuda)
    _check_columns(res, S, T, inputs, model, xs, M)
    for i in range(res.nlocal):
        assert len(res.target_index(i)) == NOUT
        np.testing.assert_array_equal(res.get_state(i), xs[M][i])


def test_drive_matches_the_oracle(cuda):
    """Column c against c applications of the oracle's update: X_TOL per update."""
    inputs, model, _ = _reference(700)
    res, ws = _context(CASES, n_override=700)
    S, _ = _drive(res, inputs, model, M, cuda, targets=False)
    o = res.fb_offsets
    for i, w in enumerate(ws):
        col, val = w.win_compressed()
        x = initial_state(w.region, w.n)
        for c in range(M + 1):
            got = S[i][c, NCS:] if c < M else res.get_state(i)
            ref = _squared(x) if c < M else x
            err = np.abs(got - ref) / (1.0 + np.abs(ref))
            print(f"region {w.region} column {c}: scaled err {err.max():.3e}")
            assert err.max() <= X_TOL * (c + 1), (w.region, c, err.max())
            if c < M:
                _, x = oracle.predict_f32(w.rows, w.cols, w.vals, col, val, w.wout, inputs[c, o[i]:o[i + 1]],
                                          np.zeros(NCS), x, w.mean, w.std)


def test_batches_compose(cuda):
    """Calls of 4 then 3 columns = one call of 7, bitwise (columns and final state)."""
    inputs, model, xs = _reference(700)
    res, _ = _context(CASES, n_override=700)
    Sa, Ta = _drive(res, inputs, model, 4, cuda)
    _check_columns(res, Sa, Ta, inputs, model, xs, 4)
    Sb, Tb = _drive(res, inputs, model, 3, cuda, first=4)
    _check_columns(res, Sb, Tb, inputs, model, xs, 3, first=4)
    for i in range(res.nlocal):
        np.testing.assert_array_equal(res.get_state(i), xs[M][i])


def test_stepwise_reference_path(cuda):
    """SML_RES_PATH_STEPWISE_DRIVE: the column writer + the update's own launch per
    column give the persistent kernel's bits (= the shared stepwise reference)."""
    inputs, model, xs = _reference(700)
    res, _ = _context(CASES, n_override=700)
    res.set_reference_paths(stepwise_drive=True)
    S, T = _drive(res, inputs, model, M, cuda)
    _check_columns(res, S, T, inputs, model, xs, M)
    for i in range(res.nlocal):
        np.testing.assert_array_equal(res.get_state(i), xs[M][i])


def _against_synchronize(make, m, cuda, targets=True):
    res, _ = make()
    inputs, model = _series(res, m, seed=23)
    xs = _stepwise_states(make()[0], inputs, m, cuda)
    S, T = _drive(res, inputs, model, m, cuda, targets=targets)
    _check_columns(res, S, T, inputs, model, xs, m)
    for i in range(res.nlocal):
        np.testing.assert_array_equal(res.get_state(i), xs[m][i])
    return res


def test_full_size_regions(cuda):
    """Full-size regions, n 5880 / 6160 / 5760 (ninp 420 / 560 / 576): the LDS ceiling
    (two states + two inputs of the 6160 / 576 maxima) and the six-pass row loop."""
    res = _against_synchronize(lambda: _context([(24, False), (30, False), (5, True)]), 3, cuda)
    assert [int(v) for v in res.n] == [5880, 6160, 5760] and res.ninp(1) == 560


def test_f64_weights(cuda):
    _against_synchronize(lambda: _context(CASES[:3], n_override=400, weight_dtype="f64"), 4, cuda)


def test_dense_win_region(cuda):
    """One region read from the CSR copy of a dense W_in beside two in ELL form."""
    _against_synchronize(lambda: _context(CASES[:3], n_override=400, dense_win=1, seed=9), 4, cuda)


def _generic_context():
    """A slab-ocean shaped context (sml_res_create_generic), chunk_speedy = 0."""
    from speedy_ml_amd.reservoir import Reservoirs

    regions, ninp = [10, 500, 1100], [48, 40, 64]
    n = [600 // p * p for p in ninp]
    res = Reservoirs(regions, [0, 0, 0], n, [6 * v for v in n], chunk_speedy=0, nout=4, ninp=ninp,
                     out_index=[35] * 4)
    for i, (r, p, nn) in enumerate(zip(regions, ninp, n)):
        rng = np.random.default_rng([6, r])
        rows = np.concatenate([rng.permutation(nn) + 1 for _ in range(6)]).astype(np.int32)
        cols = np.concatenate([rng.permutation(nn) + 1 for _ in range(6)]).astype(np.int32)
        vals = (rng.random(6 * nn) * 0.3).astype(np.float32)
        win = np.zeros((p, nn), dtype=np.float32)
        q = nn // p
        for j in range(q):
            win[np.arange(p), np.arange(p) * q + j] = (0.5 * (2 * rng.random(p) - 1)).astype(np.float32)
        wout = ((rng.random((nn, 4)) * 2 - 1) * 0.01).astype(np.float32)
        res.load_region(i, rows, cols, vals, win, wout, np.zeros(36), np.ones(36))
        res.set_state(i, 0.1 * np.random.default_rng(i).random(nn))
    return res, None


def test_generic_context_without_model_rows(cuda):
    """chunk_speedy = 0 on a generic context: columns hold the n state rows only, no
    model buffer, no targets."""
    res = _against_synchronize(_generic_context, 4, cuda, targets=False)
    assert res.ncs == 0


def test_error_paths(cuda):
    import torch

    from speedy_ml_amd.reservoir import Reservoirs

    res, ws = _context(CASES[:2], n_override=300)
    tot, nmod = int(res.fb_offsets[-1]), res.nlocal * NCS
    naug = sum(NCS + int(n) for n in res.n)
    z = lambda k: torch.zeros(k, dtype=torch.float64, device=cuda)  # noqa: E731
    d_in, d_mo, d_s, d_t = z(2 * tot), z(2 * nmod), z(2 * naug), z(2 * res.nlocal * NOUT)
    with pytest.raises(SmlError, match="stride"):
        res.train_drive(d_in, 2, d_mo, d_s, d_t, stride=tot - 1)
    with pytest.raises(SmlError, match="model_stride"):
        res.train_drive(d_in, 2, d_mo, d_s, d_t, model_stride=nmod - 1)
    # m = 0: a no-op -- state and buffers untouched
    before = [res.get_state(i) for i in range(res.nlocal)]
    d_s.fill_(3.0)
    d_t.fill_(4.0)
    res.train_drive(d_in, 0, d_mo, d_s, d_t)
    torch.cuda.synchronize()
    assert (d_s == 3.0).all() and (d_t == 4.0).all()
    for i in range(res.nlocal):
        np.testing.assert_array_equal(res.get_state(i), before[i])
    # inside a begun step
    res.predict_begin(z(tot))
    with pytest.raises(SmlError, match="begun"):
        res.train_drive(d_in, 2, d_mo, d_s, d_t)
    # a region without weights
    w = ws[0]
    empty = Reservoirs([w.region], [w.sst], [w.n], [w.k])
    with pytest.raises(SmlError, match="no weights loaded"):
        empty.train_drive(z(w.ninp), 1, z(NCS), z(NCS + w.n), None)
    # targets need the region geometry
    gen, _ = _generic_context()
    gtot, gn = int(gen.fb_offsets[-1]), int(gen.n.sum())
    with pytest.raises(SmlError, match="generic"):
        gen.train_drive(z(gtot), 1, None, z(gn), z(gen.nlocal * 4))


def _cpu_pipeline(ws, tidx, offs, inputs, model, discard, batch, nbatches, beta_res, beta_model, perturb=None):
    """The training pipeline on the CPU: the oracle's update loop for the states, the
    numpy target gather, oracle.train_accumulate per batch, oracle.train_solve.
    perturb(c, xt) -> xt': the state rows of update count c moved before they are used."""
    wouts = []
    for i, w in enumerate(ws):
        col, val = w.win_compressed()
        u = inputs[:, offs[i]:offs[i + 1]]
        x = np.zeros(w.n)
        for t in range(discard):
            _, x = oracle.predict_f32(w.rows, w.cols, w.vals, col, val, w.wout, u[t], np.zeros(NCS), x, w.mean, w.std)
        naug = NCS + w.n
        G, B = np.zeros((naug, naug)), np.zeros((naug, NOUT))
        for b in range(nbatches):
            S, T = np.zeros((batch, naug)), np.zeros((batch, NOUT))
            for c in range(batch):
                t = discard + b * batch + c
                xt = _squared(x)
                S[c, :NCS] = model[t, i * NCS:(i + 1) * NCS]
                S[c, NCS:] = perturb(t, xt) if perturb else xt
                T[c] = u[t, tidx[i]]
                _, x = oracle.predict_f32(w.rows, w.cols, w.vals, col, val, w.wout, u[t], np.zeros(NCS), x, w.mean,
                                          w.std)
            oracle.train_accumulate(S, T, G, B)
        wo, info = oracle.train_solve(G, B, NCS, beta_res, beta_model, False, 0.0)
        assert info == 0
        wouts.append(wo)
    return wouts


def _numpy_target_index(region):
    g = oracle.region_geometry(region)
    ix, iy = g["inputxchunk"], g["inputychunk"]
    xs, ys = slice(g["tdata_xstart"] - 1, g["tdata_xend"]), slice(g["tdata_ystart"] - 1, g["tdata_yend"])
    atmo = np.arange(32 * ix * iy).reshape(8, iy, ix, 4)[:, ys, xs, :]
    logp = 32 * ix * iy + np.arange(ix * iy).reshape(iy, ix)[ys, xs]
    return np.concatenate([atmo.ravel(), logp.ravel(), (logp + ix * iy).ravel()])


def test_train_wout_end_to_end(cuda, tmp_path):
    """Inputs to a weight file: train_wout (zero states, synchronize(discard), train_drive
    + accumulate per batch, solve) against the same pipeline on the CPU, max |dW| <=
    W_TOL max |W| = 1e-9 max |W|; then the float32 W_out, loaded into a fresh context,
    predicts as the oracle does with the same rounded W_out (OUT_TOL).

    Sensitivity of the tolerance (measured on the CPU with the oracle alone, these
    shapes and betas 0.5 / 1.0): moving every state row by the state tolerance of
    test_drive_matches_the_oracle, 1e-14 (t + 1) (1 + |x~|) with random signs, moves the
    oracle's W by 9e-13 max |W| (both regions) -- 1e-3 of W_TOL, under the tenth of it required
    (the test repeats the measurement and asserts it)."""
    import torch

    from speedy_ml_amd.reservoir import Reservoirs
    from speedy_ml_amd.training import train_wout

    cases, discard, batch, nbatches = [(5, True), (24, False)], 5, 16, 2
    beta_res, beta_model = 0.5, 1.0
    res, ws = _context(cases, n_override=300)
    nblocks = discard + batch * nbatches
    tot = int(res.fb_offsets[-1])
    rng = np.random.default_rng(77)
    inputs = rng.standard_normal((nblocks, tot))
    model = 2.0 * rng.random((nblocks, res.nlocal * NCS)) - 1.0
    tidx = [_numpy_target_index(w.region) for w in ws]
    ref = _cpu_pipeline(ws, tidx, res.fb_offsets, inputs, model, discard, batch, nbatches, beta_res, beta_model)
    # the tolerance's footing: the oracle's own W under a state error of the size test 2 allows
    prng = np.random.default_rng(5)
    moved = _cpu_pipeline(ws, tidx, res.fb_offsets, inputs, model, discard, batch, nbatches, beta_res, beta_model,
                          perturb=lambda t, xt: xt + X_TOL * (t + 1) * (1.0 + np.abs(xt))
                          * prng.choice([-1.0, 1.0], xt.shape))
    for a, b in zip(ref, moved):
        sens = np.abs(a - b).max() / np.abs(a).max()
        print(f"W sensitivity to the state tolerance: {sens:.3e} of max |W|")
        assert sens <= 0.1 * W_TOL
    wouts, info = train_wout(res, torch.from_numpy(inputs).to(cuda), torch.from_numpy(model).to(cuda), discard, batch,
                             nbatches, ncs=NCS, beta_res=beta_res, beta_model=beta_model, using_prior=False)
    assert (info == 0).all()
    for i, w in enumerate(ws):
        assert wouts[i].dtype == np.float32 and wouts[i].shape == (NCS + w.n, NOUT)
    # W_TOL is below float32's rounding (6e-8): the comparison is made on the solve's
    # float64 result, which the float32 arrays must be the rounding of
    res2, _ = _context(cases, n_override=300)
    got64, info = train_wout(res2, torch.from_numpy(inputs).to(cuda), torch.from_numpy(model).to(cuda), discard,
                             batch, nbatches, ncs=NCS, beta_res=beta_res, beta_model=beta_model, using_prior=False,
                             dtype=np.float64)
    assert (info == 0).all()
    for i, w in enumerate(ws):
        err = np.abs(got64[i] - ref[i]).max()
        print(f"region {w.region}: max |dW| {err:.3e} vs {W_TOL * np.abs(ref[i]).max():.3e}")
        assert err <= W_TOL * np.abs(ref[i]).max()
        np.testing.assert_array_equal(wouts[i], got64[i].astype(np.float32))
    # the trained weights predict: a fresh context from the float32 W_out
    fresh = Reservoirs([w.region for w in ws], [w.sst for w in ws], [w.n for w in ws], [w.k for w in ws])
    for i, w in enumerate(ws):
        fresh.load_region(i, w.rows, w.cols, w.vals, w.win, wouts[i], w.mean, w.std)
        fresh.set_state(i, initial_state(w.region, w.n))
    fb = rng.standard_normal(tot)
    lm = np.stack([local_model_vector(w.region) for w in ws])
    out = fresh.predict_host(fb, lm)
    o = res.fb_offsets
    for i, w in enumerate(ws):
        col, val = w.win_compressed()
        want, _ = oracle.predict_f32(w.rows, w.cols, w.vals, col, val, wouts[i], fb[o[i]:o[i + 1]], lm[i],
                                     initial_state(w.region, w.n), w.mean, w.std)
        err = np.abs(out[i] - want) / (1.0 + np.abs(want))
        assert err.max() <= OUT_TOL, (w.region, err.max())
