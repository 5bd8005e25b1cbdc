"""sml_res_series_stats / sml_res_set_mean_std_device: the standardisation statistics of a
series of global grids against the longdouble restatement (tests/_series_ref.py), on the
eight regions of _series_ref.CASES (poles, both longitude wraps, sst and no sst, neighbours
sharing halo points) with n = 64."""
import ctypes
import functools

import numpy as np
import pytest

import _series_ref as ref
from speedy_ml_amd.synthetic import region_weights

pytestmark = pytest.mark.gpu

NCS = 132
T_ODD = 37  # three chunks of 13, 13 and 11 steps: no multiple of the time tile (8), more than one chunk


def _context(cases=ref.CASES, chunk_speedy=NCS):
    from speedy_ml_amd.reservoir import Reservoirs

    ws = [region_weights(r, s, n_override=64, chunk_speedy=chunk_speedy) for r, s in cases]
    res = Reservoirs([w.region for w in ws], [w.sst for w in ws], [w.n for w in ws], [w.k for w in ws],
                     chunk_speedy=chunk_speedy)
    return res, ws


@functools.lru_cache(maxsize=None)
def _host(T, seed=3, ratio=None):
    """A seeded series: every slot with a scale and an offset of its own (temperature and
    logp far from zero), a field that varies in space and time.  ratio: every field's
    mean / std forced to it."""
    rng = np.random.default_rng(seed)
    g4 = rng.standard_normal((T, 8, 48, 96, 4))
    lvl = 1.0 + 0.1 * np.arange(8)[:, None, None, None]
    g4 = g4 * np.array([8.0, 6.0, 12.0, 2e-3]) * lvl + np.array([3.0, -1.0, 255.0, 4e-3])
    g2 = 0.02 * rng.standard_normal((T, 48, 96)) - 0.05
    pr = np.log1p(np.abs(rng.standard_normal((T, 48, 96))))
    sst = 285.0 + 8.0 * rng.standard_normal((T, 48, 96))
    tisr = 300.0 * rng.random((T, 48, 96))
    if ratio is not None:
        g4 = rng.standard_normal((T, 8, 48, 96, 4)) + ratio
        g2, pr, sst, tisr = (rng.standard_normal((T, 48, 96)) + ratio for _ in range(4))
    return tuple(np.ascontiguousarray(a) for a in (g4, g2, pr, sst, tisr))


@functools.lru_cache(maxsize=None)
def _reference(T, ratio=None):
    return ref.stats(ref.CASES, *_host(T, ratio=ratio))


def _device(arrs, cuda, pad4=0, pad2=0, fill=9.5):
    """The series on the device; with padding, steps pad4 / pad2 doubles apart from packed."""
    import torch

    out = []
    for a, pad in zip(arrs, (pad4, pad2, pad2, pad2, pad2)):
        T = a.shape[0]
        flat = torch.from_numpy(a.reshape(T, -1)).to(cuda)
        if pad:
            buf = torch.full((T, flat.shape[1] + pad), fill, dtype=torch.float64, device=cuda)
            buf[:, :flat.shape[1]] = flat
            flat = buf[:, :flat.shape[1]]
        out.append(flat.unflatten(1, a.shape[1:]))
    return out


def _stats(res, dev, stream=None, sst=True, tisr=True):
    import torch

    from speedy_ml_amd.training import series_stats

    table, change = series_stats(res, dev[0], dev[1], dev[2], dev[3] if sst else None, dev[4] if tisr else None,
                                 stream=stream)
    torch.cuda.synchronize()
    return table.cpu().numpy(), change.cpu().numpy()


def _check(table, T, ratio=None, what=""):
    mean, std, bmean, bstd = _reference(T, ratio)
    em = np.abs(table[:, :36].astype(np.longdouble) - mean)
    es = np.abs(table[:, 36:].astype(np.longdouble) - std)
    worst = max(float((em[bmean > 0] / bmean[bmean > 0]).max()), float((es[bstd > 0] / bstd[bstd > 0]).max()))
    print(f"series stats {what} T={T}: largest error / bound {worst:.3f}")
    assert (em <= bmean).all(), np.argwhere(em > bmean)
    assert (es <= bstd).all(), np.argwhere(es > bstd)
    return worst


@pytest.mark.parametrize("T", [1, 2, 3, T_ODD])
def test_statistics_match_the_restatement(cuda, T):
    """Mean and std of every region and slot within the bound derived from the kernels'
    operation counts (DESIGN, the series section), with packed and with padded strides;
    slot 35 of the regions without sst is the default (0, 1)."""
    res, _ = _context()
    for pads in ((0, 0), (6, 5)):
        table, change = _stats(res, _device(_host(T), cuda, *pads))
        _check(table, T, what=f"pads {pads}")
        for i, (_, flag) in enumerate(ref.CASES):
            if not flag:
                assert table[i, 35] == 0.0 and table[i, 71] == 1.0 and change[i] == 0
            else:
                assert change[i] == 1  # (the sst of _host varies by 8 K in space and time)
    res.close()


def test_absent_tisr_keeps_the_defaults(cuda):
    res, _ = _context()
    table, _ = _stats(res, _device(_host(3), cuda), tisr=False)
    assert (table[:, 33] == 0.0).all() and (table[:, 36 + 33] == 1.0).all()
    full, _ = _stats(res, _device(_host(3), cuda))
    keep = np.delete(np.arange(72), [33, 69])
    assert table[:, keep].tobytes() == full[:, keep].tobytes()
    res.close()


def test_conditioning_separates_two_pass_from_one_pass(cuda):
    """Fields with mean / std = 1e6 (temperature and logp are the real cases) still pass
    their bound; the reference's one-pass precipitation form, in float64 on the same input,
    does not -- the case separates the two forms."""
    T, ratio = T_ODD, 1e6
    res, _ = _context()
    table, _ = _stats(res, _device(_host(T, ratio=ratio), cuda))
    _check(table, T, ratio, what="mean/std 1e6")
    _, std, _, bstd = _reference(T, ratio)
    arrs = _host(T, ratio=ratio)
    fails = 0
    for i, (r, flag) in enumerate(ref.CASES):
        for l in (2 * 8 + 3, 32, 34):
            one = ref.one_pass_std(ref.slot_values(r, l, *arrs))
            fails += abs(np.longdouble(one) - std[i, l]) > bstd[i, l]
    print(f"one-pass float64 outside the bound: {fails} of {3 * len(ref.CASES)}")
    assert fails >= 3 * len(ref.CASES) - 2  # (a one-pass value may land inside by chance: two at the most)
    res.close()


def test_sst_change_on_both_sides_of_the_threshold(cuda):
    """sst_change = 1 iff sum (x - mean)^2 > 0 and std > 0.2: a series with std 0.25, one with
    0.15, one constant; regions without the flag report 0 throughout."""
    T = 5
    g4, g2, pr, _, tisr = _host(T)
    rng = np.random.default_rng(8)
    unit = rng.standard_normal((T, 48, 96))
    res, _ = _context()
    flagged = np.array([f for _, f in ref.CASES])
    for amp, want in ((0.25, 1), (0.15, 0), (0.0, 0)):
        sst = np.ascontiguousarray(271.35 + amp * unit)
        table, change = _stats(res, _device((g4, g2, pr, sst, tisr), cuda))
        std = ref.stats(ref.CASES, g4, g2, pr, sst, tisr)[1][:, 35]
        assert (np.abs(std[flagged] - 0.2) > 0.02).all() or amp == 0.0  # well off the threshold
        assert (change[flagged] == want).all(), (amp, change)
        assert (change[~flagged] == 0).all()
        if amp == 0.0:
            bstd = ref.stats(ref.CASES, g4, g2, pr, sst, tisr)[3][:, 35]
            assert (table[flagged, 71] <= bstd[flagged]).all()  # a constant field: std 0 up to the sums' rounding
    res.close()


def test_bit_for_bit_across_calls_streams_masks_and_strides(cuda):
    import torch

    from speedy_ml_amd._lib import check, lib

    res, _ = _context()
    packed, padded = _device(_host(T_ODD), cuda), _device(_host(T_ODD), cuda, 6, 5)
    # both streams are the library's and are destroyed below: the test leaves the process's
    # streams, and with them their share of its few hardware queues, as it found them
    h, hs = ctypes.c_void_p(), ctypes.c_void_p()
    ncu = torch.cuda.get_device_properties(cuda).multi_processor_count
    check(lib().sml_stream_create_cu_range(ncu // 2, 24, ctypes.byref(h)))
    check(lib().sml_stream_create_cu_range(0, ncu, ctypes.byref(hs)))
    masked = torch.cuda.ExternalStream(h.value, device=cuda)
    side = torch.cuda.ExternalStream(hs.value, device=cuda)
    torch.cuda.synchronize()
    runs = [_stats(res, packed), _stats(res, packed), _stats(res, packed, stream=side),
            _stats(res, packed, stream=masked), _stats(res, padded)]
    res.close()
    check(lib().sml_stream_destroy(h))
    check(lib().sml_stream_destroy(hs))
    assert np.isfinite(runs[0][0]).all()
    for t in range(1, len(runs)):
        assert runs[t][0].tobytes() == runs[0][0].tobytes(), t
        assert runs[t][1].tobytes() == runs[0][1].tobytes(), t


def test_nan_reaches_exactly_the_tiles_that_hold_the_point(cuda):
    """A NaN at one point of one step of one (variable, level): exactly that slot of the
    regions whose input tile holds the point is NaN."""
    T, v, z = 5, 2, 3
    X, Y = ref.tile_points(245)
    x, y = int(X[1, 3]), int(Y[1, 3])  # in 245's halo column: 269's own point
    holders = [i for i, (r, _) in enumerate(ref.CASES)
               if ((ref.tile_points(r)[0] == x) & (ref.tile_points(r)[1] == y)).any()]
    assert len(holders) >= 2 and len(holders) < len(ref.CASES)
    arrs = [a.copy() for a in _host(T)]
    arrs[0][2, z, y, x, v] = np.nan
    res, _ = _context()
    table, _ = _stats(res, _device(arrs, cuda))
    res.close()
    want = np.zeros((len(ref.CASES), 72), bool)
    want[holders, v * 8 + z] = want[holders, 36 + v * 8 + z] = True
    assert np.array_equal(np.isnan(table), want)


def test_refusals(cuda):
    """SML_ERR_ARG with a message, nothing enqueued: T = 0, short strides, a misaligned 4-d
    pointer or stride, a generic context, a NULL d_sst with sst regions;
    set_mean_std_device under a begun step and with members."""
    import torch

    from speedy_ml_amd._lib import lib, ptr, stream_ptr
    from speedy_ml_amd.reservoir import Reservoirs

    L = lib()
    res, ws = _context()
    for i, w in enumerate(ws):
        res.load_region_weights(i, w)
    d4, d2, dp, ds, dt = _device(_host(2), cuda)
    table = torch.full((res.nlocal, 72), 7.0, dtype=torch.float64, device=cuda)
    st = stream_ptr(None)

    def stats(c=res.handle, g4=d4, s4=147456, s2=4608, T=2, sst=ds):
        return L.sml_res_series_stats(c, ptr(g4), s4, ptr(d2), ptr(dp), ptr(sst), ptr(dt), s2, T, ptr(table), None, st)

    for kw, word in ((dict(T=0), b"T = 0"), (dict(s4=147454), b"g4_stride"), (dict(s2=4607), b"g2_stride"),
                     (dict(s4=147457), b"16-byte"), (dict(g4=d4.reshape(-1)[1:]), b"16-byte"),
                     (dict(sst=None), b"d_sst")):
        rc = stats(**kw)
        assert rc == -1 and word in L.sml_last_error(), (rc, word, L.sml_last_error())
    gen = Reservoirs([0, 1], [0, 0], [64, 64], [128, 128], chunk_speedy=0, nout=4, ninp=[8, 8], out_index=[0, 1, 2, 3])
    assert stats(c=gen.handle) == -1 and b"generic" in L.sml_last_error()
    inputs = torch.zeros(2 * int(res.fb_offsets[-1]), dtype=torch.float64, device=cuda)
    rc = L.sml_res_tile_series(gen.handle, ptr(d4), 147456, ptr(d2), ptr(dp), None, None, 4608, None, 0, None, 0, 2,
                               ptr(inputs), inputs.numel() // 2, None, 0, st)
    assert rc == -1 and b"generic" in L.sml_last_error()
    gen.close()
    torch.cuda.synchronize()
    assert (table == 7.0).all()  # nothing was enqueued
    # set_mean_std_device: refused inside a begun step and with members
    fb, _, _ = res.alloc_io(cuda)
    res.predict_begin(fb)
    assert res.step_begun()
    assert L.sml_res_set_mean_std_device(res.handle, ptr(table), st) == -1 and b"begun" in L.sml_last_error()
    res.cancel_step()
    res.set_members(2)
    assert L.sml_res_set_mean_std_device(res.handle, ptr(table), st) == -1 and b"members" in L.sml_last_error()
    res.set_members(1)
    assert L.sml_res_set_mean_std_device(res.handle, ptr(table), st) == 0
    res.close()


def test_adoption(cuda):
    """After set_mean_std_device the host copy sml_res_mean_std returns is the table, and
    sml_res_tile_feedback standardises with it."""
    import torch

    from speedy_ml_amd._lib import check, lib, ptr
    from speedy_ml_amd.training import fit_standardisation

    res, _ = _context()
    arrs = _host(3)
    dev = _device(arrs, cuda)
    mean, std, change = fit_standardisation(res, *dev)
    table, _ = _stats(res, dev)
    assert np.array_equal(mean, table[:, :36]) and np.array_equal(std, table[:, 36:])
    for i in range(res.nlocal):
        m, s = np.zeros(36), np.zeros(36)
        check(lib().sml_res_mean_std(res.handle, i, ptr(m), ptr(s)))
        assert np.array_equal(m, mean[i]) and np.array_equal(s, std[i])
    fb = torch.zeros(int(res.fb_offsets[-1]), dtype=torch.float64, device=cuda)
    res.tile_feedback(dev[0][1], dev[1][1], dev[2][1], None, fb)
    torch.cuda.synchronize()
    got, off = fb.cpu().numpy(), ref.feedback_offsets(ref.CASES)
    assert off[-1] == int(res.fb_offsets[-1])
    for i, (r, flag) in enumerate(ref.CASES):
        want = ref.tile_feedback(r, flag, arrs[0][1], arrs[1][1], arrs[2][1], None, None, mean[i], std[i])
        there = ~np.isnan(want)  # the sst and tisr entries are not this call's
        assert np.array_equal(got[off[i]:off[i + 1]][there], want[there]), r
        assert (got[off[i]:off[i + 1]][~there] == 0.0).all()
    res.close()
