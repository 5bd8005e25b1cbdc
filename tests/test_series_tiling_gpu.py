"""sml_res_tile_series: T input blocks and T model blocks in one launch each, bit for bit
the loop of the single-grid calls; the sst entries against NumPy; padding untouched.  The
eight regions of _series_ref.CASES, n = 64, the mean / std the regions were loaded with."""
import functools

import numpy as np
import pytest

import _series_ref as ref
from speedy_ml_amd.synthetic import region_weights

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
PAD_IN, PAD_MODEL = 3, 5


def _context(chunk_speedy):
    from speedy_ml_amd.reservoir import Reservoirs

    ws = [region_weights(r, s, n_override=64, chunk_speedy=chunk_speedy) for r, s in ref.CASES]
    res = Reservoirs([w.region for w in ws], [w.sst for w in ws], [w.n for w in ws], [w.k for w in ws],
                     chunk_speedy=chunk_speedy)
    for i, w in enumerate(ws):
        res.load_region_weights(i, w)
    return res, ws


@functools.lru_cache(maxsize=None)
def _host(T):
    rng = np.random.default_rng(100 + T)
    g4 = rng.standard_normal((T, 8, 48, 96, 4)) * np.array([8.0, 6.0, 12.0, 2e-3]) + np.array([3.0, -1.0, 255.0, 4e-3])
    g2, pr = 0.02 * rng.standard_normal((T, 48, 96)), np.abs(rng.standard_normal((T, 48, 96)))
    sst, tisr = 285.0 + 8.0 * rng.standard_normal((T, 48, 96)), 300.0 * rng.random((T, 48, 96))
    fc4 = g4 + 0.1 * rng.standard_normal(g4.shape)
    fc2 = g2 + 0.001 * rng.standard_normal(g2.shape)
    return g4, g2, pr, sst, tisr, fc4, fc2


@pytest.mark.parametrize("ncs", [0, 132])
@pytest.mark.parametrize("T", [1, 3, 5, 37])
def test_series_is_the_loop_of_the_single_grid_calls(cuda, T, ncs):
    import torch

    from speedy_ml_amd.training import tile_series

    res, ws = _context(ncs)
    host = _host(T)
    g4, g2, pr, sst, tisr, fc4, fc2 = (torch.from_numpy(a).to(cuda) for a in host)
    tot, nmod = int(res.fb_offsets[-1]), res.nlocal * ncs
    ins, mos = tot + PAD_IN, nmod + PAD_MODEL
    inputs = torch.full((T, ins), SENTINEL, dtype=torch.float64, device=cuda)
    model = torch.full((T, mos), SENTINEL, dtype=torch.float64, device=cuda) if ncs else None
    tile_series(res, g4, g2, pr, sst, tisr, fc4 if ncs else None, fc2 if ncs else None, inputs=inputs.view(-1),
                model=model.view(-1) if ncs else None, in_stride=ins, model_stride=mos)
    # the loop of the single-grid calls, on buffers that start as the sentinel
    want = torch.full((T, tot), SENTINEL, dtype=torch.float64, device=cuda)
    wmod = torch.full((T, max(nmod, 1)), SENTINEL, dtype=torch.float64, device=cuda)
    for t in range(T):
        res.tile_feedback(g4[t], g2[t], pr[t], None, want[t])
        check_tisr(res, tisr[t], want[t])
        if ncs:
            res.tile_local_model(fc4[t], fc2[t], wmod[t])
    torch.cuda.synchronize()
    got, want = inputs.cpu().numpy(), want.cpu().numpy()
    off = ref.feedback_offsets(ref.CASES)
    assert off[-1] == tot
    sst_entry = np.zeros(tot, bool)
    for i, (r, flag) in enumerate(ref.CASES):
        w = ws[i]
        g = ref.geometry(r)
        in2d = g["inx"] * g["iny"]
        if flag:
            at = off[i] + 4 * in2d * 8 + 2 * in2d
            sst_entry[at:at + in2d] = True
            # the sst entries, which the single-grid call leaves to the slab stage: NumPy float64
            X, Y = ref.tile_points(r)
            for t in range(T):
                x = host[3][t][Y, X].ravel()
                assert np.array_equal(got[t, at:at + in2d], (x - np.float64(w.mean[35])) / np.float64(w.std[35])), (r, t)
    assert (want[:, sst_entry] == SENTINEL).all() and not (want[:, ~sst_entry] == SENTINEL).any()
    assert got[:, :tot][:, ~sst_entry].tobytes() == want[:, ~sst_entry].tobytes()
    assert (got[:, tot:] == SENTINEL).all()  # the padding between blocks is untouched
    if ncs:
        gm, wm = model.cpu().numpy(), wmod.cpu().numpy()
        assert gm[:, :nmod].tobytes() == wm.tobytes() and not (wm == SENTINEL).any()
        assert (gm[:, nmod:] == SENTINEL).all()
    res.close()


def check_tisr(res, field, fb):
    from speedy_ml_amd._lib import check, lib, ptr, stream_ptr

    check(lib().sml_res_tile_tisr_field(res.handle, ptr(field), ptr(fb), stream_ptr(None)))


def test_absent_fields_and_argument_checks(cuda):
    """sst / tisr None leave their entries untouched; model blocks are refused at
    chunk_speedy 0, a short in_stride and fc4 without d_model are refused."""
    import torch

    from speedy_ml_amd._lib import lib, ptr, stream_ptr
    from speedy_ml_amd.training import tile_series

    T = 3
    res, _ = _context(0)
    g4, g2, pr, sst, tisr, fc4, fc2 = (torch.from_numpy(a).to(cuda) for a in _host(T))
    tot = int(res.fb_offsets[-1])
    full = torch.full((T * tot,), SENTINEL, dtype=torch.float64, device=cuda)
    part = torch.full((T * tot,), SENTINEL, dtype=torch.float64, device=cuda)
    tile_series(res, g4, g2, pr, sst, tisr, inputs=full)
    tile_series(res, g4, g2, pr, None, None, inputs=part)
    torch.cuda.synchronize()
    f, p = full.cpu().numpy(), part.cpu().numpy()
    kept = p == SENTINEL
    nsst = sum(ref.geometry(r)["inx"] * ref.geometry(r)["iny"] for r, flag in ref.CASES if flag)
    ntisr = sum(ref.geometry(r)["inx"] * ref.geometry(r)["iny"] for r, _ in ref.CASES)
    assert kept.sum() == T * (nsst + ntisr) and not (f == SENTINEL).any()
    assert np.array_equal(f[~kept], p[~kept])
    L, st = lib(), stream_ptr(None)

    def call(in_stride=tot, f4=None, f2=None, mod=None):
        return L.sml_res_tile_series(res.handle, ptr(g4), 147456, ptr(g2), ptr(pr), None, None, 4608, ptr(f4), 147456,
                                     ptr(f2), 4608, T, ptr(part), in_stride, ptr(mod), 8, st)

    assert call(in_stride=tot - 1) == -1 and b"in_stride" in L.sml_last_error()
    assert call(f4=fc4, f2=fc2) == -1 and b"together" in L.sml_last_error()
    assert call(f4=fc4, f2=fc2, mod=full) == -1 and b"chunk_speedy" in L.sml_last_error()
    res.close()
