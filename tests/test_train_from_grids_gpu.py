"""train_from_grids: from a seeded series of global grids to W_out on the device -- the
statistics against the restatement, the blocks against the single-grid tilings with the
adopted table, W_out against train_wout on those blocks -- and fit_standardisation's error
on a flagged region whose sst does not vary."""
import numpy as np
import pytest

import _series_ref as ref
from speedy_ml_amd.synthetic import region_weights

pytestmark = pytest.mark.gpu

NCS = 132
CASES = [(0, True), (245, True), (246, False), (1151, False)]
# the discard phase is tiled 8 steps long, the two batches 15 each: an odd length, and one
# that differs from the discard's, through the one reused buffer
T, DISCARD, BATCH, NBATCHES = 40, 8, 15, 2


def _context():
    from speedy_ml_amd.reservoir import Reservoirs

    ws = [region_weights(r, s, n_override=64, chunk_speedy=NCS) for r, s in CASES]
    res = Reservoirs([w.region for w in ws], [w.sst for w in ws], [w.n for w in ws], [w.k for w in ws],
                     chunk_speedy=NCS)
    for i, w in enumerate(ws):
        res.load_region_weights(i, w)
    return res, ws


def _host(seed=21):
    rng = np.random.default_rng(seed)
    g4 = rng.standard_normal((T, 8, 48, 96, 4)) * np.array([8.0, 6.0, 12.0, 2e-3]) + np.array([3.0, -1.0, 255.0, 4e-3])
    g2, pr = 0.02 * rng.standard_normal((T, 48, 96)) - 0.05, np.abs(rng.standard_normal((T, 48, 96)))
    sst, tisr = 285.0 + 8.0 * rng.standard_normal((T, 48, 96)), 300.0 * rng.random((T, 48, 96))
    fc4 = g4 + 0.1 * rng.standard_normal(g4.shape) * np.array([8.0, 6.0, 12.0, 2e-3])
    fc2 = g2 + 0.001 * rng.standard_normal(g2.shape)
    return g4, g2, pr, sst, tisr, fc4, fc2


def test_end_to_end_from_grids(cuda):
    import torch

    from speedy_ml_amd._lib import check, lib, ptr, stream_ptr
    from speedy_ml_amd.training import tile_series, train_from_grids, train_wout

    host = _host()
    g4, g2, pr, sst, tisr, fc4, fc2 = (torch.from_numpy(a).to(cuda) for a in host)
    res, ws = _context()
    kw = dict(ncs=NCS, beta_res=0.5, beta_model=1.0, using_prior=False, dtype=np.float64)
    wouts, info, mean, std = train_from_grids(res, (g4, g2, pr, sst, tisr), (fc4, fc2), DISCARD, BATCH, NBATCHES, **kw)
    assert (info == 0).all()
    # --- the statistics, over the whole series, within their bound
    rmean, rstd, bmean, bstd = ref.stats(CASES, *host[:5])
    em, es = np.abs(mean.astype(np.longdouble) - rmean), np.abs(std.astype(np.longdouble) - rstd)
    print(f"largest error / bound: mean {float((em[bmean > 0] / bmean[bmean > 0]).max()):.3f}, "
          f"std {float((es[bstd > 0] / bstd[bstd > 0]).max()):.3f}")
    assert (em <= bmean).all() and (es <= bstd).all()
    for i in range(res.nlocal):  # adopted
        m, s = np.zeros(36), np.zeros(36)
        check(lib().sml_res_mean_std(res.handle, i, ptr(m), ptr(s)))
        assert np.array_equal(m, mean[i]) and np.array_equal(s, std[i])
    # --- the blocks: the single-grid tilings with the adopted table (sst entries: NumPy)
    nblocks = DISCARD + BATCH * NBATCHES
    tot, nmod = int(res.fb_offsets[-1]), res.nlocal * NCS
    d_in, d_mod = tile_series(res, g4[:nblocks], g2[:nblocks], pr[:nblocks], sst[:nblocks], tisr[:nblocks],
                              fc4[:nblocks], fc2[:nblocks])
    want = torch.zeros((nblocks, tot), dtype=torch.float64, device=cuda)
    wmod = torch.zeros((nblocks, nmod), dtype=torch.float64, device=cuda)
    for t in range(nblocks):
        res.tile_feedback(g4[t], g2[t], pr[t], None, want[t])
        check(lib().sml_res_tile_tisr_field(res.handle, ptr(tisr[t]), ptr(want[t]), stream_ptr(None)))
        res.tile_local_model(fc4[t], fc2[t], wmod[t])
    torch.cuda.synchronize()
    want = want.cpu().numpy()
    off = ref.feedback_offsets(CASES)
    for i, (r, flag) in enumerate(CASES):
        if flag:
            g = ref.geometry(r)
            in2d = g["inx"] * g["iny"]
            at = off[i] + 4 * in2d * 8 + 2 * in2d
            X, Y = ref.tile_points(r)
            want[:, at:at + in2d] = (host[3][:nblocks][:, Y, X].reshape(nblocks, -1) - mean[i, 35]) / std[i, 35]
    assert d_in.cpu().numpy().tobytes() == want.tobytes()
    assert d_mod.cpu().numpy().tobytes() == wmod.cpu().numpy().tobytes()
    # --- W_out: train_wout on those blocks, a context of its own
    res2, _ = _context()
    wref, info2 = train_wout(res2, d_in, d_mod, DISCARD, BATCH, NBATCHES, **kw)
    assert (info2 == 0).all()
    for i, w in enumerate(ws):
        assert wouts[i].shape == (NCS + w.n, 136) and np.isfinite(wouts[i]).all()
        assert wouts[i].tobytes() == wref[i].tobytes(), w.region
    res.close()
    res2.close()


def test_flagged_region_with_a_constant_sst_raises(cuda):
    import torch

    from speedy_ml_amd.training import fit_standardisation

    g4, g2, pr, sst, tisr, _, _ = _host()
    sst = sst[:6].copy()
    X, Y = ref.tile_points(245)
    sst[:, Y, X] = 271.35  # region 245 (local 1): a frozen patch; region 0 keeps a varying sst
    res, ws = _context()
    before = [w.mean.copy() for w in ws]
    dev = [torch.from_numpy(np.ascontiguousarray(a[:6])).to(cuda) for a in (g4, g2, pr)] + \
          [torch.from_numpy(sst).to(cuda), torch.from_numpy(np.ascontiguousarray(tisr[:6])).to(cuda)]
    with pytest.raises(ValueError, match=r"local regions \[1\] \(ids \[245\]\)"):
        fit_standardisation(res, *dev)
    # nothing was adopted
    from speedy_ml_amd._lib import check, lib, ptr

    m, s = np.zeros(36), np.zeros(36)
    check(lib().sml_res_mean_std(res.handle, 1, ptr(m), ptr(s)))
    assert np.array_equal(m, np.asarray(before[1], dtype=np.float64))
    res.close()
