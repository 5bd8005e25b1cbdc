"""train_slab_from_grids: from a seeded series of global grids to the slab-ocean reservoirs'
W_out on the device -- bit for bit the hand-composed chain of the calls it makes (the phase /
stride bookkeeping), against the oracle chain (the NumPy restatement's averaged series, the
oracle's state update per column from x = 0 per phase, oracle.train_accumulate over all
phases, oracle.train_solve(ncs = 0)) within the project's training tolerances, and the
returned weights loaded and used for one prediction.  The atmo context is the eight regions
of _series_ref.CASES, the slab reservoirs have n = 2 * ninp."""
import numpy as np
import pytest

import _series_ref as ref
import _slab_series_ref as sref
import _train_ref as tref
import oracle
from speedy_ml_amd.synthetic import region_weights, slab_weights

pytestmark = pytest.mark.gpu

T, S, DISCARD, BATCH, NBATCHES = 40, 3, 2, 5, 2
WINDOW, DIVISOR = 3, 2
# W_TOL holds for a well-conditioned system (tests/test_training_gpu.py): 30 columns against
# 224 unknowns leave the regulariser to condition it, so it is of the Gram's own size here,
# as in tests/test_train_from_grids_gpu.py
BETA = 0.5
W_TOL = 1e-9     # W within 1e-9 of max |W|
OUT_TOL = 1e-11  # the reservoir tests' outvec bound: |err| <= 1e-11 (1 + |v|)


def _contexts():
    from speedy_ml_amd.reservoir import Reservoirs

    ws = [region_weights(r, s, n_override=64) for r, s in ref.CASES]
    atmo = Reservoirs([w.region for w in ws], [w.sst for w in ws], [w.n for w in ws], [w.k for w in ws])
    for i, w in enumerate(ws):
        atmo.load_region_weights(i, w)
    return atmo, ws


def _slab():
    from speedy_ml_amd.reservoir import Reservoirs

    sreg = [r for r, s in ref.CASES if s]
    sws = [slab_weights(r, n_override=2 * 7 * 16) for r in sreg]
    slab = Reservoirs(sreg, [0] * len(sreg), [w.n for w in sws], [w.k for w in sws], chunk_speedy=0, nout=4,
                      ninp=[w.ninp for w in sws], out_index=[35] * 4)
    for j, w in enumerate(sws):
        slab.load_region_weights(j, w)
    return slab, sws


def _host(seed=23):
    rng = np.random.default_rng(seed)
    g4 = rng.standard_normal((T, 8, 48, 96, 4)) * np.array([8.0, 6.0, 12.0, 2e-3]) + np.array([3.0, -1.0, 255.0, 4e-3])
    g2, pr = 0.02 * rng.standard_normal((T, 48, 96)) - 0.05, np.abs(rng.standard_normal((T, 48, 96)))
    sst, tisr = 285.0 + 8.0 * rng.standard_normal((T, 48, 96)), 300.0 * rng.random((T, 48, 96))
    return g4, g2, pr, sst, tisr


def _squared(x):
    xt = x.copy()
    xt[1::2] = x[1::2] * x[1::2]
    return xt


def test_end_to_end(cuda):
    import torch

    from speedy_ml_amd.training import Trainer, slab_series, tile_series, train_slab_from_grids

    host = _host()
    dev = tuple(torch.from_numpy(a).to(cuda) for a in host)
    atmo, ws = _contexts()
    slab, sws = _slab()
    kw = dict(beta_res=BETA, dtype=np.float64)
    wouts, info, mean, std = train_slab_from_grids(atmo, slab, dev, WINDOW, DIVISOR, S, DISCARD, BATCH, NBATCHES, **kw)
    assert (info == 0).all()
    rows = [i for i, (_, flag) in enumerate(ref.CASES) if flag]
    for j, i in enumerate(rows):  # the slab's file carries its atmo region's statistics
        assert np.array_equal(mean[j], ws[i].mean) and np.array_equal(std[j], ws[i].std)

    # ---- bit for bit the hand-composed chain, on contexts of its own
    atmo2, _ = _contexts()
    slab2, _ = _slab()
    series = slab_series(atmo2, slab2, *dev, WINDOW, DIVISOR)
    tidx = np.stack([slab2.slab_target_index(j) for j in range(slab2.nlocal)])
    slab2.set_target_index(tidx)
    tot = int(slab2.fb_offsets[-1])
    naug = [int(n) for n in slab2.n]
    tr = Trainer(naug, 4)
    tr.reset()
    states = torch.empty(sum(naug) * BATCH, dtype=torch.float64, device=cuda)
    targets = torch.empty(len(naug) * BATCH * 4, dtype=torch.float64, device=cuda)
    Sg, Tg = [[] for _ in naug], [[] for _ in naug]  # the GPU's own columns, for the backward error
    for i in range(S):
        for j, n in enumerate(naug):
            slab2.set_state(j, np.zeros(n))
        slab2.synchronize(series[i * tot:], DISCARD, stride=S * tot)
        for b in range(NBATCHES):
            col = i + (DISCARD + b * BATCH) * S
            slab2.train_drive(series[col * tot:], BATCH, None, states, targets, stride=S * tot)
            tr.accumulate(states, targets, BATCH)
            torch.cuda.synchronize()
            s, t, off = states.cpu().numpy(), targets.cpu().numpy(), 0
            for j, n in enumerate(naug):
                Sg[j].append(s[off:off + n * BATCH].reshape(BATCH, n).copy())
                Tg[j].append(t[j * BATCH * 4:(j + 1) * BATCH * 4].reshape(BATCH, 4).copy())
                off += n * BATCH
    packed, info2 = tr.solve(ncs=0, beta_res=BETA, using_prior=False)
    assert (info2 == 0).all()
    hand = [v.cpu().numpy() for v in tr.wout_views(packed)]
    tr.close()
    for j in range(len(naug)):
        assert wouts[j].shape == (naug[j], 4) and np.isfinite(wouts[j]).all()
        assert wouts[j].tobytes() == hand[j].tobytes(), j

    # ---- the oracle chain
    blocks, _ = tile_series(atmo2, *dev)
    torch.cuda.synchronize()
    a = sref.averaged(sref.gather(ref.CASES, blocks.cpu().numpy().reshape(T, -1)), WINDOW, DIVISOR)
    assert series.cpu().numpy().tobytes() == a.tobytes()
    soff = sref.slab_offsets(ref.CASES)
    params = (0, BETA, 1.0, False, 0.0)
    for j, w in enumerate(sws):
        col, val = w.win_compressed()
        u = a[:, soff[j]:soff[j + 1]]

        def upd(x, fb):
            return oracle.predict_slab_ml_f32(w.rows, w.cols, w.vals, col, val, w.wout, fb, x, w.mean[35], w.std[35])[1]

        So, To = [], []
        for i in range(S):
            x = np.zeros(w.n)
            for k in range(DISCARD + BATCH * NBATCHES):
                c = i + k * S
                if k >= DISCARD:
                    So.append(_squared(x))
                    To.append(u[c, tidx[j]])
                x = upd(x, u[c])
        So, To = np.array(So), np.array(To)
        Go, Bo = np.zeros((w.n, w.n)), np.zeros((w.n, 4))
        oracle.train_accumulate(So, To, Go, Bo)
        wo, oinfo = oracle.train_solve(Go, Bo, *params)
        assert oinfo == 0
        err = np.abs(wouts[j] - wo).max()
        # the targets are the slab's sst entries of the averaged series, bit for bit
        Sj, Tj = np.concatenate(Sg[j]), np.concatenate(Tg[j])
        assert Tj.tobytes() == To.tobytes(), j
        Gr, Br = tref.regularised(*tref.sums(Sj, Tj), *params)
        e = tref.eta(Gr, Br, wouts[j])
        print(f"slab {w.region}: |W - oracle| {err:.3e} (max |W| {np.abs(wo).max():.3e}), eta {e:.3e}, "
              f"cap {tref.eta_cap(w.n):.3e}, states within {np.abs(Sj - So).max():.1e} of the oracle's")
        assert err <= W_TOL * np.abs(wo).max(), (j, err)
        assert e <= tref.eta_cap(w.n), (j, e)

    # ---- the returned weights, as float32 (the file's NF90_REAL), load and predict
    w32, _, mean32, std32 = train_slab_from_grids(atmo, slab, dev, WINDOW, DIVISOR, S, DISCARD, BATCH, NBATCHES,
                                                 beta_res=BETA)
    slab3, _ = _slab()
    x0 = []
    for j, w in enumerate(sws):
        assert w32[j].dtype == np.float32 and np.array_equal(w32[j], wouts[j].astype(np.float32))
        slab3.load_region(j, w.rows, w.cols, w.vals, w.win, w32[j], mean32[j], std32[j])
        x0.append(0.1 * np.random.default_rng(j).random(w.n))
        slab3.set_state(j, x0[j])
    fb = series[7 * tot:8 * tot].clone()
    ov = torch.zeros((slab3.nlocal, 4), dtype=torch.float64, device=cuda)
    slab3.predict(fb, None, ov)
    torch.cuda.synchronize()
    got = ov.cpu().numpy()
    for j, w in enumerate(sws):
        col, val = w.win_compressed()
        want, _ = oracle.predict_slab_ml_f32(w.rows, w.cols, w.vals, col, val, w32[j], a[7, soff[j]:soff[j + 1]], x0[j],
                                             mean32[j][35], std32[j][35])
        assert (np.abs(got[j] - want) <= OUT_TOL * (1 + np.abs(want))).all(), (j, got[j], want)
    for c in (atmo, slab, atmo2, slab2, slab3):
        c.close()


def test_value_error_on_a_short_series_and_a_foreign_slab(cuda):
    import torch

    from speedy_ml_amd.reservoir import Reservoirs
    from speedy_ml_amd.training import train_slab_from_grids

    Ts = 6
    dev = tuple(torch.from_numpy(np.ascontiguousarray(a[:Ts])).to(cuda) for a in _host())
    atmo, _ = _contexts()
    slab, sws = _slab()
    with pytest.raises(ValueError, match="fewer than phase_stride"):
        train_slab_from_grids(atmo, slab, dev, 3, 2, 2, 2, 2, 1, beta_res=BETA)  # 2 * (2 + 2) = 8 > 6
    sreg = [r for r, s in ref.CASES if s]
    other = Reservoirs(sreg[1:], [0] * 3, [w.n for w in sws[1:]], [w.k for w in sws[1:]], chunk_speedy=0, nout=4,
                       ninp=[w.ninp for w in sws[1:]], out_index=[35] * 4)
    with pytest.raises(ValueError, match="not the ML-only context"):
        train_slab_from_grids(atmo, other, dev, 3, 2, 2, 1, 2, 1, beta_res=BETA)
    # the exact length passes
    wouts, info, _, _ = train_slab_from_grids(atmo, slab, dev, 3, 2, 2, 1, 2, 1, beta_res=BETA)
    assert (info == 0).all() and len(wouts) == 4
    for c in (atmo, slab, other):
        c.close()


def test_a_non_blocking_side_stream_gives_the_default_streams_bits(cuda):
    """Every launch goes to `stream`, and each phase's host-side reset of the states waits for
    it: on a non-blocking stream (torch's own are) the phases still start from x = 0."""
    import torch

    from speedy_ml_amd.training import train_slab_from_grids

    dev = tuple(torch.from_numpy(a).to(cuda) for a in _host())
    torch.cuda.synchronize()
    runs = []
    for stream in (None, torch.cuda.Stream(device=cuda)):
        atmo, _ = _contexts()
        slab, _ = _slab()
        wouts, info, _, _ = train_slab_from_grids(atmo, slab, dev, WINDOW, DIVISOR, S, DISCARD, BATCH, NBATCHES,
                                                  beta_res=BETA, dtype=np.float64, stream=stream)
        torch.cuda.synchronize()
        assert (info == 0).all()
        runs.append(wouts)
        atmo.close()
        slab.close()
    for a, b in zip(*runs):
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes()


def test_a_rank_without_sst_regions_returns_empty_results(cuda):
    import torch

    from speedy_ml_amd.reservoir import Reservoirs
    from speedy_ml_amd.training import train_slab_from_grids

    cases = [(r, s) for r, s in ref.CASES if not s]
    ws = [region_weights(r, s, n_override=64) for r, s in cases]
    atmo = Reservoirs([w.region for w in ws], [w.sst for w in ws], [w.n for w in ws], [w.k for w in ws])
    slab = Reservoirs([], [], [], [], chunk_speedy=0, nout=4, ninp=[], out_index=[35] * 4)
    dev = tuple(torch.from_numpy(np.ascontiguousarray(a[:6])).to(cuda) for a in _host())
    wouts, info, mean, std = train_slab_from_grids(atmo, slab, dev, 3, 2, 2, 1, 2, 1, beta_res=BETA)
    assert wouts == [] and info.shape == (0,) and mean.shape == (0, 36) and std.shape == (0, 36)
    atmo.close()
    slab.close()
