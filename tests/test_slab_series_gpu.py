"""sml_slab_train_series: the slab reservoirs' rolling-mean input series from a series of
global grids -- bit for bit against the NumPy restatement (tests/_slab_series_ref.py) over
tile_series's own blocks, within the derived bound against longdouble from the raw grids,
and bit for bit across column ranges, strides, streams and CU masks.  The atmo context is
the eight regions of _series_ref.CASES (four with sst: poles, wraps, neighbours sharing halo
points), n = 64; the slab reservoirs have n = 2 * ninp."""
import ctypes
import functools

import numpy as np
import pytest

import _series_ref as ref
import _slab_series_ref as sref
from speedy_ml_amd.synthetic import region_weights, slab_weights

pytestmark = pytest.mark.gpu

CHUNK = 64       # kSlabSerChunk (csrc/sml_slab_series.hpp): the columns one thread serves
LANES_64_MAX = 121  # slab_series_threads: the largest window served by blocks of 64 lanes; 122 .. 249 take 32, 250 .. 16
T_LONG = 2 * CHUNK + 2  # three chunks: columns CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK - 1, 2 CHUNK, 2 CHUNK + 1
FORMS = [(1, 1), (2, 1), (3, 2), (28, 27), (29, 28)]
SENTINEL = -77.25


def _contexts(cases=ref.CASES, load=True):
    from speedy_ml_amd.reservoir import Reservoirs

    ws = [region_weights(r, s, n_override=64) for r, s in cases]
    atmo = Reservoirs([w.region for w in ws], [w.sst for w in ws], [w.n for w in ws], [w.k for w in ws])
    if load:
        for i, w in enumerate(ws):
            atmo.load_region_weights(i, w)
    sreg = [r for r, s in cases if s]
    sws = [slab_weights(r, n_override=2 * 7 * 16) for r in sreg]
    slab = Reservoirs(sreg, [0] * len(sreg), [w.n for w in sws], [w.k for w in sws], chunk_speedy=0, nout=4,
                      ninp=[w.ninp for w in sws], out_index=[35] * 4)
    for j, w in enumerate(sws):
        assert w.n == 2 * w.ninp
    return atmo, slab, ws


@functools.lru_cache(maxsize=None)
def _host(T, seed=5):
    rng = np.random.default_rng(seed + T)
    g4 = rng.standard_normal((T, 8, 48, 96, 4)) * np.array([8.0, 6.0, 12.0, 2e-3]) + np.array([3.0, -1.0, 255.0, 4e-3])
    g2, pr = 0.02 * rng.standard_normal((T, 48, 96)) - 0.05, np.abs(rng.standard_normal((T, 48, 96)))
    sst, tisr = 285.0 + 8.0 * rng.standard_normal((T, 48, 96)), 300.0 * rng.random((T, 48, 96))
    return tuple(np.ascontiguousarray(a) for a in (g4, g2, pr, sst, tisr))


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


def _z(atmo, dev):
    """z [T, slab feedback]: tile_series's own blocks gathered through slab_input_index."""
    import torch

    from speedy_ml_amd.training import tile_series

    T = dev[0].shape[0]
    blocks, _ = tile_series(atmo, *dev)
    torch.cuda.synchronize()
    return sref.gather(ref.CASES, blocks.cpu().numpy().reshape(T, -1))


def _series(atmo, slab, dev, window, divisor, tisr=True, **kw):
    import torch

    from speedy_ml_amd.training import slab_series

    out = slab_series(atmo, slab, dev[0], dev[1], dev[2], dev[3], dev[4] if tisr else None, window, divisor, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("window,divisor", FORMS)
def test_bit_for_bit_with_the_restatement(cuda, window, divisor):
    """T = 1, window - 1, window, window + 1: the ramp-up columns (d = the number of terms),
    the first full window, the first column that drops a step."""
    atmo, slab, _ = _contexts()
    tot = int(slab.fb_offsets[-1])
    assert tot == sref.slab_offsets(ref.CASES)[-1]
    for T in sorted({1, window - 1, window, window + 1} - {0}):
        dev = _device(_host(T), cuda)
        want = sref.averaged(_z(atmo, dev), window, divisor)
        got = _series(atmo, slab, dev, window, divisor).reshape(T, tot)
        assert np.isfinite(got).all()
        assert got.tobytes() == want.tobytes(), (T, np.argwhere(got != want)[:4])
    atmo.close()
    slab.close()


@functools.lru_cache(maxsize=None)
def _long(cuda):
    """The three-chunk series on the device, with its z (shared: computed once)."""
    atmo, slab, _ = _contexts()
    dev = _device(_host(T_LONG), cuda)
    z = _z(atmo, dev)
    atmo.close()
    slab.close()
    return dev, z


@pytest.mark.parametrize("window,divisor", [(3, 2), (7, 7), (8, 7), (9, 8), (29, 28), (LANES_64_MAX, LANES_64_MAX - 1),
                                            (LANES_64_MAX + 1, LANES_64_MAX), (250, 249)])
def test_three_chunks_and_every_block_size(cuda, window, divisor):
    """T_LONG columns span three of the kernel's chunks (columns CHUNK - 1, CHUNK, CHUNK + 1
    of the first edge, and the second edge's); windows below, on and above the tile of 8
    columns summed together; windows LANES_64_MAX and LANES_64_MAX + 1 are the last served by
    64 lanes a block and the first by 32, 250 the first by 16."""
    dev, z = _long(cuda)
    atmo, slab, _ = _contexts()
    tot = int(slab.fb_offsets[-1])
    want = sref.averaged(z, window, divisor)
    got = _series(atmo, slab, dev, window, divisor).reshape(T_LONG, tot)
    for t in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1):
        assert got[t].tobytes() == want[t].tobytes(), t
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:4]
    atmo.close()
    slab.close()


@pytest.mark.parametrize("window,divisor", [(3, 2), (29, 28)])
def test_within_the_bound_of_longdouble_from_the_raw_grids(cuda, window, divisor):
    """|a^ - a| <= 1.01 (w + 2) u sum|z| / d: 2u per standardised value, (w - 1) u sum|z| for
    the ordered sum, u for the division (tests/_slab_series_ref.py)."""
    T = 40
    atmo, slab, ws = _contexts()
    host = _host(T)
    got = _series(atmo, slab, _device(host, cuda), window, divisor).reshape(T, -1)
    mean, std = np.stack([w.mean for w in ws]), np.stack([w.std for w in ws])
    a, bound = sref.averaged_ld(sref.standardised_ld(ref.CASES, *host, mean, std), window, divisor)
    err = np.abs(got.astype(np.longdouble) - a)
    assert (bound > 0).all()
    print(f"slab series ({window}, {divisor}) T={T}: largest error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), np.argwhere(err > bound)[:4]
    atmo.close()
    slab.close()


def test_ranges_strides_streams_and_masks_give_the_same_bits(cuda):
    import torch

    from speedy_ml_amd._lib import check, lib

    window, divisor = 29, 28
    dev, _ = _long(cuda)
    atmo, slab, _ = _contexts()
    tot = int(slab.fb_offsets[-1])
    whole = _series(atmo, slab, dev, window, divisor).reshape(T_LONG, tot)
    again = _series(atmo, slab, dev, window, divisor).reshape(T_LONG, tot)
    assert again.tobytes() == whole.tobytes()
    # column ranges: t0 inside a chunk, on a chunk's edge, one column short of an edge; ncols < T - t0
    for t0, ncols in ((7, 20), (CHUNK, CHUNK + 1), (CHUNK - 1, 3), (CHUNK + 5, CHUNK - 10), (T_LONG - 1, 1), (3, 0)):
        part = _series(atmo, slab, dev, window, divisor, t0=t0, ncols=ncols).reshape(ncols, tot)
        assert part.tobytes() == whole[t0:t0 + ncols].tobytes(), (t0, ncols)
    # a padded out_stride: the columns are the same, the words between them untouched
    pad = 5
    out = torch.full((T_LONG, tot + pad), SENTINEL, dtype=torch.float64, device=cuda)
    got = _series(atmo, slab, dev, window, divisor, out=out.view(-1), out_stride=tot + pad).reshape(T_LONG, tot + pad)
    assert got[:, :tot].tobytes() == whole.tobytes() and (got[:, tot:] == SENTINEL).all()
    # padded series strides
    padded = _device(_host(T_LONG), cuda, 6, 5)
    assert _series(atmo, slab, padded, window, divisor).tobytes() == whole.tobytes()
    del padded
    # a side stream and a CU mask (the library's streams, destroyed below)
    h, hs = ctypes.c_void_p(), ctypes.c_void_p()
    ncu = torch.cuda.get_device_properties(cuda).multi_processor_count
    check(lib().sml_stream_create_cu_range(ncu // 2, 24, ctypes.byref(h)))
    check(lib().sml_stream_create_cu_range(0, ncu, ctypes.byref(hs)))
    masked = torch.cuda.ExternalStream(h.value, device=cuda)
    side = torch.cuda.ExternalStream(hs.value, device=cuda)
    torch.cuda.synchronize()
    runs = [_series(atmo, slab, dev, window, divisor, stream=side), _series(atmo, slab, dev, window, divisor, stream=masked)]
    atmo.close()
    slab.close()
    check(lib().sml_stream_destroy(h))
    check(lib().sml_stream_destroy(hs))
    for k, r in enumerate(runs):
        assert r.tobytes() == whole.tobytes(), k


def test_a_nan_reaches_its_entries_for_window_columns(cuda):
    """A NaN at one logp point of step t*: exactly the slab entries whose source is that
    point, exactly in columns t* .. t* + window - 1; every other double keeps its bits."""
    T, window, divisor, ts = 12, 3, 2, 4
    X, Y = ref.tile_points(245)
    x, y = int(X[1, 3]), int(Y[1, 3])  # in 245's halo column: 269's own point
    host = _host(T)
    bad = [a.copy() for a in host]
    bad[1][ts, y, x] = np.nan
    atmo, slab, ws = _contexts()
    clean = _series(atmo, slab, _device(host, cuda), window, divisor).reshape(T, -1)
    got = _series(atmo, slab, _device(bad, cuda), window, divisor).reshape(T, -1)
    atmo.close()
    slab.close()
    # the entries whose source is the point, from the restatement's own geometry
    mean, std = np.stack([w.mean for w in ws]), np.stack([w.std for w in ws])
    entries = np.isnan(sref.standardised_ld(ref.CASES, *[a[ts:ts + 1] for a in bad], mean, std)[0])
    assert entries.sum() >= 2  # 245 and 269 both hold the point
    want = np.zeros(got.shape, bool)
    want[ts:ts + window, entries] = True
    assert np.array_equal(np.isnan(got), want)
    assert got[~want].tobytes() == clean[~want].tobytes()


def test_a_null_tisr_gives_zeros_at_the_tisr_entries(cuda):
    T, window, divisor = 9, 3, 2
    atmo, slab, _ = _contexts()
    dev = _device(_host(T), cuda)
    full = _series(atmo, slab, dev, window, divisor).reshape(T, -1)
    none = _series(atmo, slab, dev, window, divisor, tisr=False).reshape(T, -1)
    atmo.close()
    slab.close()
    m = sref.tisr_entries(ref.CASES)
    assert m.any() and (none[:, m] == 0.0).all() and not np.signbit(none[:, m]).any()
    assert none[:, ~m].tobytes() == full[:, ~m].tobytes()


def test_device_side_refusals(cuda):
    """SML_ERR_ARG with a message and nothing enqueued: a slab context of other regions, in
    another order, with other input counts or hybrid; an atmo context with members or
    generic; an out_stride below the slab's packed feedback."""
    import torch

    from speedy_ml_amd._lib import lib, ptr, stream_ptr
    from speedy_ml_amd.reservoir import Reservoirs

    L = lib()
    atmo, slab, _ = _contexts()
    d4, d2, dp, ds, dt = _device(_host(3), cuda)
    tot = int(slab.fb_offsets[-1])
    out = torch.full((3 * tot,), SENTINEL, dtype=torch.float64, device=cuda)

    def call(a=atmo, s=slab, out_stride=tot):
        return L.sml_slab_train_series(a.handle, s.handle, ptr(d4), 147456, ptr(d2), ptr(dp), ptr(ds), ptr(dt), 4608, 3, 2,
                                       1, 0, 3, ptr(out), out_stride, stream_ptr(None))

    sreg = [r for r, s in ref.CASES if s]
    mk = lambda regs, ninp, ncs=0, nout=4: Reservoirs(regs, [0] * len(regs), [2 * v for v in ninp], [8] * len(regs),  # noqa: E731
                                                      chunk_speedy=ncs, nout=nout, ninp=ninp, out_index=[35] * nout)
    ninp = [int(slab.ninp(j)) for j in range(slab.nlocal)]
    others = [(mk(sreg[:-1], ninp[:-1]), b"is not the rank's sst region"),
              (mk(sreg + [500], ninp + [112]), b"5 slab reservoirs for 4 sst regions"),
              (mk([sreg[1], sreg[0]] + sreg[2:], [ninp[1], ninp[0]] + ninp[2:]), b"is not the rank's sst region"),
              (mk(sreg, [ninp[0] + 7] + ninp[1:]), b"the atmo subset has"),
              (mk(sreg, ninp, nout=6), b"predict the sst of the region's 4 points")]
    for other, word in others:
        assert call(s=other) == -1 and word in L.sml_last_error(), (word, L.sml_last_error())
        other.close()
    assert call(a=slab) == -1 and b"generic" in L.sml_last_error()
    assert call(out_stride=tot - 1) == -1 and b"out_stride" in L.sml_last_error()
    atmo.set_members(2)
    assert call() == -1 and b"members" in L.sml_last_error()
    atmo.set_members(1)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()  # nothing was enqueued
    assert call() == 0
    torch.cuda.synchronize()
    assert not (out == SENTINEL).any()
    atmo.close()
    slab.close()
