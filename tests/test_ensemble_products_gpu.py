"""Ensemble products on the GPU (csrc/sml_ensemble.hip, speedy_ml_amd.ensemble.EnsembleProducts):
per-point mean and spread of E members' grids, and per step the area-weighted rmse, spread,
fair CRPS, bias and rank histogram of each of the 34 fields against a truth.

Members are synthetic_grids(100 + e), the truth synthetic_grids(7); E runs over 1, 2, 3, 4, 5, 8,
9, 32: both sides of the 4-member load tile, and the maximum.  The host arrays and the
longdouble references are built once per E and never modified.

Moments: a float64 NumPy restatement of the kernel's operations in their order.
  s = x_0; s = s + x_e; mean = s / E                      -- the device's within 1 ulp
  q = 0; d = x_e - mean; q = q + d * d; var = q / (E - 1)  -- from the *returned* mean, so that
  the chain up to the last division is restated bit for bit and var is within 1 ulp;
  spread = sqrt(var) within 1 ulp of np.sqrt of that variance.  The ABI returns the spread, not
  the variance, so the two statements are checked together: the returned spread must be within
  1 ulp of np.sqrt(v) for a v within 1 ulp of the restated variance.

Scores: against np.longdouble on the same fp64 inputs (u = 2^-53, N = 4608 points, w the row
weights, A = mean_e |x_e|, terms >= 0 unless said).  A sum of n fp64 terms added in any order
carries at most (n - 1) u sum|terms| to first order, each term's own roundings add their count
times u |term|, and c = 8 covers the constant per-point operations (the subtraction of the
mean or the truth, the square, the division, the weight) and the second-order remainders:
  S  = sum w var:    E squares summed per point            -> B_S = (N + E + c) u S
       (var is insensitive to the mean's error to first order: sum_e (x_e - m') ^ 2 =
       sum_e (x_e - m) ^ 2 + E (m - m') ^ 2)
  R  = sum w (m - y)^2                                      -> B_R = (N + c) u R + sum 2 w |m - y| dm
  Bi = sum w (m - y), signed                                -> B_b = (N + c) u sum w |m - y| + sum w dm
       with dm = E u A the first-order image of the mean's error (E - 1 additions of
       magnitude <= sum|x_e|, one division)
  C  = sum w [a / E - 2 p / (2 E (E - 1))], a = sum_e |x_e - y|, p = sum_{e<f} |x_e - x_f|
                                                            -> B_C = (N + E (E - 1) / 2 + E + c) u sum w (a / E + pair)
  rmse = sqrt(R), spread = sqrt(S): one more rounding       -> B / (2 sqrt(.)) + u sqrt(.)
The largest ratio of error to bound is printed (DESIGN.md section 3.8 records it).

Measured on the MI355X: the mean and the spread are the restatement bit for bit at every E; the
largest error / bound is 0.0011 (rmse), 0.0014 (spread), 0.0009 (crps), 0.0003 (bias): the
bounds count a serial sum of 4608 terms, the kernels add a lane tree and 48 row partials."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ES = (1, 2, 3, 4, 5, 8, 9, 32)
N, F, U, C = 4608, 34, 2.0 ** -53, 8
RMSE, SPREAD, CRPS, BIAS = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def _host(E):
    """(g4 [E, 8, 48, 96, 4], g2 [E, 48, 96], pr [E, 48, 96]) and the truth triple."""
    from speedy_ml_amd.synthetic import synthetic_grids

    gs = [synthetic_grids(100 + e) for e in range(E)]
    out = tuple(np.ascontiguousarray(np.stack([g[i] for g in gs])) for i in range(3)) + (synthetic_grids(7),)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def _fields(g4, g2, pr):
    """[..., 34, 4608]: field 4 k + v, then logp, then precip."""
    lead = g4.shape[:-4]
    a = np.moveaxis(g4, -1, -3).reshape(lead + (32, N))
    return np.concatenate([a, g2.reshape(lead + (1, N)), pr.reshape(lead + (1, N))], axis=-2)


def _weights():
    from speedy_ml_amd.ensemble import EnsembleProducts

    return np.repeat(EnsembleProducts.weights(), 96)  # [4608], row j * 96 + i


def _reference(x, y, w):
    """Longdouble scores [34, 4] and their bounds, and the rank histogram [34, 33], of members
    x [E, 34, 4608] against y [34, 4608]."""
    E = x.shape[0]
    L = np.longdouble
    xl, yl, wl = x.astype(L), y.astype(L), w.astype(L)
    m = xl.sum(0) / E
    d = xl - m
    var = (d * d).sum(0) / (E - 1) if E > 1 else np.zeros_like(m)
    a = np.abs(xl - yl).sum(0)
    p = np.zeros_like(m)
    for e in range(E):
        for f in range(e + 1, E):
            p += np.abs(xl[e] - xl[f])
    pair = 2 * p / (2 * E * (E - 1)) if E > 1 else p
    A = np.abs(xl).sum(0) / E
    dm = E * U * A
    S, R = (wl * var).sum(1), (wl * (m - yl) ** 2).sum(1)
    sc, bd = np.zeros((F, 4), L), np.zeros((F, 4), L)
    B_S = (N + E + C) * U * S
    B_R = (N + C) * U * R + (2 * wl * np.abs(m - yl) * dm).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc[:, SPREAD], bd[:, SPREAD] = np.sqrt(S), np.where(S > 0, B_S / (2 * np.sqrt(S)), 0) + U * np.sqrt(S)
        sc[:, RMSE], bd[:, RMSE] = np.sqrt(R), B_R / (2 * np.sqrt(R)) + U * np.sqrt(R)
    sc[:, BIAS] = (wl * (m - yl)).sum(1)
    bd[:, BIAS] = (N + C) * U * (wl * np.abs(m - yl)).sum(1) + (wl * dm).sum(1)
    sc[:, CRPS] = (wl * (a / E - pair)).sum(1)
    bd[:, CRPS] = (N + E * (E - 1) // 2 + E + C) * U * (wl * (a / E + pair)).sum(1)
    r = (x < y).sum(0)
    hist = np.stack([np.bincount(r[f], minlength=33) for f in range(F)]).astype(np.int32)
    return sc, bd, hist


@functools.lru_cache(maxsize=None)
def _ref(E):
    g4, g2, pr, truth = _host(E)
    return _reference(_fields(g4, g2, pr), _fields(*truth), _weights())


def _dev(cuda, *arrays):
    import torch

    return [None if a is None else torch.from_numpy(np.array(a, order="C")).to(cuda) for a in arrays]


def _ulps(a, b):
    """Distance in units in the last place between float64 arrays of one sign pattern."""
    ia, ib = a.view(np.int64).astype(np.int64), b.view(np.int64).astype(np.int64)
    ia = np.where(ia < 0, np.int64(-2 ** 63) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2 ** 63) - ib, ib)
    return np.abs(ia - ib)


def _run(cuda, E, capacity=1, t=0, truth=True, pr=True):
    """moments + scores of the E synthetic members; host (moments [6], scores, ranks)."""
    import torch

    from speedy_ml_amd.ensemble import EnsembleProducts

    g4, g2, p, tr = _host(E)
    d4, d2, dp = _dev(cuda, g4, g2, p if pr else None)
    dt = tuple(_dev(cuda, *tr)) if truth else None
    prod = EnsembleProducts(E, capacity, cuda)
    mom = prod.moments(d4, d2, dp)
    prod.scores(d4, d2, dp, dt, t)
    torch.cuda.synchronize()
    sc, rk = prod.read()
    out = [None if m is None else m.cpu().numpy() for m in mom], sc, rk
    prod.close()
    return out


@pytest.mark.parametrize("E", ES)
def test_moments_against_the_restatement(cuda, E):
    g4, g2, pr, _ = _host(E)
    mom, _, _ = _run(cuda, E)
    x = _fields(g4, g2, pr)
    mean, spread = _fields(mom[0], mom[1], mom[2]), _fields(mom[3], mom[4], mom[5])
    s = x[0].copy()
    for e in range(1, E):
        s = s + x[e]
    want = s / E
    du = _ulps(mean, want)
    print(f"E {E}: mean exactly the restatement at {(du == 0).mean():.6f} of the points, worst {du.max()} ulp"
          f" (the device's division is {'' if du.max() == 0 else 'not '}correctly rounded here)")
    assert du.max() <= 1
    if E == 1:
        np.testing.assert_array_equal(mean, x[0])
        assert np.array_equal(spread, np.zeros_like(spread)) and not np.signbit(spread).any()
        return
    q = np.zeros_like(mean)
    for e in range(E):
        d = x[e] - mean
        q = q + d * d
    var = q / (E - 1)
    # the returned spread is within 1 ulp of np.sqrt(v) for a v within 1 ulp of the restated variance
    ok = np.zeros(var.shape, bool)
    for v in (var, np.nextafter(var, np.inf), np.nextafter(var, -np.inf)):
        ok |= _ulps(spread, np.sqrt(v)) <= 1
    print(f"E {E}: spread exactly sqrt(restated variance) at {(spread == np.sqrt(var)).mean():.6f} of the points")
    assert ok.all(), int((~ok).sum())
    assert (spread > 0).all()


def test_equal_members_have_no_spread(cuda):
    """Four equal members: x + x + x + x and the division by 4 are exact, so the mean is the
    member bit for bit and every deviation, the variance and the spread are exactly 0."""
    from speedy_ml_amd.ensemble import EnsembleProducts

    g4, g2, pr, _ = _host(1)
    d4, d2, dp = _dev(cuda, np.repeat(g4, 4, 0), np.repeat(g2, 4, 0), np.repeat(pr, 4, 0))
    prod = EnsembleProducts(4, 1, cuda)
    mom = [m.cpu().numpy() for m in prod.moments(d4, d2, dp)]
    prod.scores(d4, d2, dp, None, 0)
    sc, _ = prod.read()
    prod.close()
    for got, want in zip(mom[:3], (g4[0], g2[0], pr[0])):
        np.testing.assert_array_equal(got, want)
    for got in mom[3:]:
        np.testing.assert_array_equal(got, 0.0)
    np.testing.assert_array_equal(sc[0, :, SPREAD], 0.0)


@pytest.mark.parametrize("E", ES)
def test_scores_and_ranks_against_longdouble(cuda, E):
    sc, bd, hist = _ref(E)
    _, got, ranks = _run(cuda, E)
    err = np.abs(got[0].astype(np.longdouble) - sc)
    ratio = np.where(bd > 0, err / np.where(bd > 0, bd, 1), np.where(err == 0, 0, np.inf))
    for k, name in enumerate(("rmse", "spread", "crps", "bias")):
        print(f"E {E}: {name:6s} largest error / bound {float(ratio[:, k].max()):.4f} (field {int(ratio[:, k].argmax())})")
    assert np.isfinite(got[0]).all()
    assert (ratio <= 1).all(), np.argwhere(ratio > 1)
    if E == 1:  # no spread, and the fair CRPS is the absolute error
        np.testing.assert_array_equal(got[0][:, SPREAD], 0.0)
    np.testing.assert_array_equal(ranks[0], hist)
    assert (ranks[0].sum(1) == N).all()
    assert (ranks[0][:, E + 1:] == 0).all()


def test_ties_are_not_below_and_permutations_change_nothing(cuda):
    """The truth equal to member 2 at every point of fields 5 and 33, and at chosen points of
    field 32: that member is not counted as below itself, so the top bin E stays empty there
    and the histogram is NumPy's.  Then the members permuted: the same histograms, and the
    scores within the bounds of the same reference."""
    import torch

    from speedy_ml_amd.ensemble import EnsembleProducts

    E = 5
    g4, g2, pr, truth = _host(E)
    t4, t2, tp = (a.copy() for a in truth)
    t4[1, :, :, 1] = g4[2, 1, :, :, 1]  # field 5 = level 1, variable 1
    tp[:] = pr[2]
    chosen = (np.array([0, 0, 23, 47, 47]), np.array([0, 95, 40, 0, 95]))
    t2[chosen] = g2[2][chosen]
    x, y = _fields(g4, g2, pr), _fields(t4, t2, tp)
    sc, bd, hist = _reference(x, y, _weights())
    assert (hist[[5, 33], E] == 0).all() and hist[5].sum() == N
    prod = EnsembleProducts(E, 2, cuda)
    d4, d2, dp, dt4, dt2, dtp = _dev(cuda, g4, g2, pr, t4, t2, tp)
    prod.scores(d4, d2, dp, (dt4, dt2, dtp), 0)
    perm = [3, 0, 4, 2, 1]
    p4, p2, pp = _dev(cuda, g4[perm], g2[perm], pr[perm])
    prod.scores(p4, p2, pp, (dt4, dt2, dtp), 1)
    torch.cuda.synchronize()
    got, ranks = prod.read()
    prod.close()
    np.testing.assert_array_equal(ranks[0], hist)
    np.testing.assert_array_equal(ranks[1], hist)
    r2 = (g2 < t2).sum(0)[chosen]  # member 2 itself is not below: at most E - 1
    assert (r2 == (np.delete(g2, 2, 0) < t2).sum(0)[chosen]).all() and r2.max() <= E - 1
    for row in (0, 1):
        err = np.abs(got[row].astype(np.longdouble) - sc)
        assert (err <= bd).all(), (row, np.argwhere(err > bd))


def test_bit_for_bit_across_calls_streams_masks_and_strides(cuda):
    """Scores, ranks and moments of E = 9: a second call, a side stream, a CU-masked stream
    (sml_stream_create_cu_range), member strides larger than packed, and scores without a
    moments call before it, all against the first call on the default stream."""
    import torch

    from speedy_ml_amd._lib import check, lib
    from speedy_ml_amd.ensemble import EnsembleProducts

    E = 9
    g4, g2, pr, truth = _host(E)
    d4, d2, dp = _dev(cuda, g4, g2, pr)
    dt = tuple(_dev(cuda, *truth))
    pad = lambda a, extra: torch.cat([a.reshape(E, -1), torch.full((E, extra), 9.5, dtype=torch.float64, device=cuda)], 1)  # noqa: E731
    b4, b2, bp = pad(d4, 24), pad(d2, 9), pad(dp, 9)
    s4 = b4[:, :147456].unflatten(1, (8, 48, 96, 4))
    s2, sp = b2[:, :4608].unflatten(1, (48, 96)), bp[:, :4608].unflatten(1, (48, 96))
    assert s4.stride(0) == 147456 + 24 and s2.stride(0) == 4608 + 9 and s4.data_ptr() == b4.data_ptr()
    # both streams are the library's and are destroyed below: the test leaves the process's
    # streams, and with them their share of its few hardware queues, as it found them
    h, hs = ctypes.c_void_p(), ctypes.c_void_p()
    ncu = torch.cuda.get_device_properties(cuda).multi_processor_count
    check(lib().sml_stream_create_cu_range(ncu // 2, 24, ctypes.byref(h)))
    check(lib().sml_stream_create_cu_range(0, ncu, ctypes.byref(hs)))
    masked = torch.cuda.ExternalStream(h.value, device=cuda)
    side = torch.cuda.ExternalStream(hs.value, device=cuda)
    prod = EnsembleProducts(E, 6, cuda)
    torch.cuda.synchronize()
    runs = [(d4, d2, dp, None), (d4, d2, dp, None), (d4, d2, dp, side), (d4, d2, dp, masked), (s4, s2, sp, None)]
    moms = []
    for t, (a4, a2, ap, st) in enumerate(runs):
        mom = prod.moments(a4, a2, ap, stream=st)
        prod.scores(a4, a2, ap, dt, t, stream=st)
        torch.cuda.synchronize()
        moms.append([m.cpu().numpy() for m in mom])
    prod.scores(d4, d2, dp, dt, 5)  # no moments call before it on a fresh stream of work
    torch.cuda.synchronize()
    sc, rk = prod.read()
    prod.close()
    check(lib().sml_stream_destroy(h))
    check(lib().sml_stream_destroy(hs))
    assert np.isfinite(sc).all()
    for t in range(1, 6):
        assert sc[t].tobytes() == sc[0].tobytes(), t
        np.testing.assert_array_equal(rk[t], rk[0])
    for t in range(1, 5):
        for a, b in zip(moms[t], moms[0]):
            assert a.tobytes() == b.tobytes(), t
    assert (b4[:, 147456:] == 9.5).all() and (b2[:, 4608:] == 9.5).all()  # the padding is only skipped


def test_containment(cuda):
    """E = 5.  A NaN in member 3 at one point of field 9 (level 2, variable 1): a NaN mean and
    spread at that point only and NaN scores for that field only -- everything else is the
    clean run's bit for bit.  A NULL precip leaves field 33's rows as reset left them; no
    truth leaves rmse, crps and bias NaN, the ranks 0 and the spread that of the run with
    truth; rows t - 1 and t + 1 stay as reset left them."""
    import torch

    from speedy_ml_amd.ensemble import EnsembleProducts

    E = 5
    g4, g2, pr, truth = _host(E)
    clean_mom, clean_sc, clean_rk = _run(cuda, E, capacity=3, t=1)
    assert np.isnan(clean_sc[[0, 2]]).all() and (clean_rk[[0, 2]] == 0).all()  # the neighbouring rows
    assert np.isfinite(clean_sc[1]).all()
    bad = g4.copy()
    bad[3, 2, 10, 20, 1] = np.nan
    d4, d2, dp = _dev(cuda, bad, g2, pr)
    dt = tuple(_dev(cuda, *truth))
    prod = EnsembleProducts(E, 3, cuda)
    mom = [m.cpu().numpy() for m in prod.moments(d4, d2, dp)]
    prod.scores(d4, d2, dp, dt, 1)
    sc, rk = prod.read()
    for k in (0, 3):
        nan = np.argwhere(np.isnan(mom[k]))
        assert nan.tolist() == [[2, 10, 20, 1]], nan
        keep = np.ones(mom[k].shape, bool)
        keep[2, 10, 20, 1] = False
        assert mom[k][keep].tobytes() == clean_mom[k][keep].tobytes()
    for k in (1, 2, 4, 5):
        assert mom[k].tobytes() == clean_mom[k].tobytes()
    assert np.isnan(sc[1, 9]).all()
    others = [f for f in range(F) if f != 9]
    assert sc[1, others].tobytes() == clean_sc[1, others].tobytes()
    np.testing.assert_array_equal(rk[1, others], clean_rk[1, others])
    assert rk[1, 9].sum() == N  # the NaN is not below the truth: the point is still counted
    # NULL precip, then no truth, in rows of their own
    prod.reset()
    e4, e2, ep = _dev(cuda, g4, g2, pr)
    prod.scores(e4, e2, None, dt, 0)
    prod.scores(e4, e2, ep, None, 2)
    mom2 = prod.moments(e4, e2, None)
    torch.cuda.synchronize()
    assert mom2[2] is None and mom2[5] is None
    assert mom2[0].cpu().numpy().tobytes() == clean_mom[0].tobytes()
    sc, rk = prod.read()
    prod.close()
    assert np.isnan(sc[1]).all() and (rk[1] == 0).all()  # reset, and untouched by rows 0 and 2
    assert np.isnan(sc[0, 33]).all() and (rk[0, 33] == 0).all()
    assert sc[0, :33].tobytes() == clean_sc[1, :33].tobytes()
    np.testing.assert_array_equal(rk[0, :33], clean_rk[1, :33])
    assert np.isnan(sc[2][:, [RMSE, CRPS, BIAS]]).all() and (rk[2] == 0).all()
    assert sc[2][:, SPREAD].tobytes() == clean_sc[1][:, SPREAD].tobytes()
    # the quiet NaN of reset, bit for bit
    assert sc[1].view(np.uint64).tolist() == [[0x7FF8000000000000] * 4] * F


def test_truth_without_precip(cuda):
    """A truth without precip beside members with precip: field 33 is scored as without truth
    (its spread only), the other fields as with the whole truth."""
    import torch

    from speedy_ml_amd.ensemble import EnsembleProducts

    E = 3
    g4, g2, pr, truth = _host(E)
    _, full, full_rk = _run(cuda, E)
    d4, d2, dp = _dev(cuda, g4, g2, pr)
    t4, t2, _ = _dev(cuda, *truth)
    prod = EnsembleProducts(E, 1, cuda)
    prod.scores(d4, d2, dp, (t4, t2, None), 0)
    torch.cuda.synchronize()
    sc, rk = prod.read()
    prod.close()
    assert sc[0, :33].tobytes() == full[0, :33].tobytes()
    np.testing.assert_array_equal(rk[0, :33], full_rk[0, :33])
    assert sc[0, 33, SPREAD] == full[0, 33, SPREAD] and np.isnan(sc[0, 33, [RMSE, CRPS, BIAS]]).all()
    assert (rk[0, 33] == 0).all()


def test_refusals_through_the_abi(cuda):
    """Every refusal arrives as SML_ERR_ARG with sml_last_error naming the argument; nothing
    is launched (the tables stay as reset left them)."""
    import torch

    from speedy_ml_amd._lib import SmlError, check, lib, ptr
    from speedy_ml_amd.ensemble import EnsembleProducts

    L = lib()
    h = ctypes.c_void_p()
    for members, capacity, msg in ((0, 4, r"members 0 out of range \[1, 32\]"), (33, 4, "members 33 out of range"),
                                   (4, 0, "capacity_steps 0")):
        with pytest.raises(SmlError, match=msg):
            check(L.sml_ens_create(members, capacity, ctypes.byref(h)))
        assert not h.value
    E = 3
    g4, g2, pr, truth = _host(E)
    d4, d2, dp = _dev(cuda, g4, g2, pr)
    t4, t2, tp = _dev(cuda, *truth)
    prod = EnsembleProducts(E, 2, cuda)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    info = [ctypes.c_int() for _ in range(5)]
    check(L.sml_ens_info(prod._h, *[ctypes.byref(x) for x in info]))
    assert [x.value for x in info] == [E, 2, 34, 4, 33]
    m = [torch.empty_like(d4[0]), torch.empty_like(d2[0]), torch.empty_like(d2[0])]
    for s4, s2, msg in ((147455, 4608, "g4_stride 147455 smaller"), (147456, 4607, "g2_stride 4607 smaller"),
                        (147457, 4608, "g4_stride 147457 odd")):
        with pytest.raises(SmlError, match=msg):
            check(L.sml_ens_moments(prod._h, ptr(d4), s4, ptr(d2), ptr(dp), s2, ptr(m[0]), ptr(m[1]), ptr(m[2]), None,
                                    None, None, st))
        with pytest.raises(SmlError, match=msg):
            check(L.sml_ens_scores(prod._h, ptr(d4), s4, ptr(d2), ptr(dp), s2, ptr(t4), ptr(t2), ptr(tp), 0, st))
    args = (prod._h, ptr(d4), 147456, ptr(d2), ptr(dp), 4608)
    for t, msg in ((-1, r"t -1 out of range \[0, 2\)"), (2, r"t 2 out of range \[0, 2\)")):
        with pytest.raises(SmlError, match=msg):
            check(L.sml_ens_scores(*args, ptr(t4), ptr(t2), ptr(tp), t, st))
    for tr, msg in (((t4, None, None), "truth half given"), ((None, t2, tp), "truth half given"),
                    ((None, None, tp), "d_truthpr set")):
        with pytest.raises(SmlError, match=msg):
            check(L.sml_ens_scores(*args, *[ptr(x) for x in tr], 0, st))
    with pytest.raises(SmlError, match="null members' grid"):
        check(L.sml_ens_scores(prod._h, None, 147456, ptr(d2), ptr(dp), 4608, None, None, None, 0, st))
    with pytest.raises(SmlError, match=r"rows \[1, 1 \+ 2\) outside \[0, 2\)"):
        prod.read(1, 2)
    with pytest.raises(ValueError, match="3 members expected"):
        prod.scores(d4[:2], d2[:2], dp[:2], None, 0)
    sc, rk = prod.read()
    prod.close()
    assert np.isnan(sc).all() and (rk == 0).all()
