"""The reference's input noise on the device (sml_res_set_input_noise, sml_res_input_noise,
sml_res_train_drive_from) and noise=InputNoise(...) on the training
functions.  Every assertion is exact (integer bits; one or two fp64 operations, contraction
off) or a derived bound against NumPy longdouble on the device's own draws.

The bounds.  U = 2^-53.  The ROCm device library's ulp figures are not documented in this
tree's toolchain, so (as the issue sets for that case) C_NORMAL is 4 x the largest ratio
|g - g_ld| / (U max(sqrt(-2 log u1), 1)) measured on this file's draws against the longdouble
value, 2.60 (printed by test_normals; DESIGN.md section 3.11 records it).  The precipitation
bound is first-order error propagation through the branch's eleven operations with K_FN ulp
for exp and log (test_precip_entries' docstring)."""
import ctypes
import functools

import numpy as np
import pytest

import _noise_ref as nref
import _series_ref as ref
from speedy_ml_amd.synthetic import region_weights, slab_weights

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
C_NORMAL = 10.5  # 4 x 2.603, the measured largest ratio (m = 17; 2.564 at m = 3), rounded up
K_FN = 4.0      # ulp allowed to the device's exp and log in the precip bound (2^-52 relative each)
NCS = 132
IDS = [r for r, _ in ref.CASES]
SEED = 0xC0FFEE


@functools.lru_cache(maxsize=None)
def _layout(cases=tuple(ref.CASES)):
    off = ref.feedback_offsets(list(cases))
    return off, [int(v) for v in np.diff(off)]


def _atmo(cases=ref.CASES, ncs=NCS, load=True):
    from speedy_ml_amd.reservoir import Reservoirs

    ws = [region_weights(r, s, n_override=64, chunk_speedy=ncs) for r, s in cases]
    res = Reservoirs([w.region for w in ws], [w.sst for w in ws], [w.n for w in ws], [w.k for w in ws], chunk_speedy=ncs)
    if load:
        for i, w in enumerate(ws):
            res.load_region_weights(i, w)
    return res, ws


def _precip_mask(cases=ref.CASES):
    """The precipitation entries of the packed layout, from the documented feedback layout
    [atmo(4, inx, iny, 8) | logp | precip | sst? | tisr] alone, and each entry's local region."""
    off, ninp = _layout(tuple(cases))
    mask, reg = np.zeros(off[-1], bool), np.zeros(off[-1], int)
    for i, (r, _) in enumerate(cases):
        g = ref.geometry(r)
        in2d = g["inx"] * g["iny"]
        mask[off[i] + 33 * in2d:off[i] + 34 * in2d] = True
        reg[off[i]:off[i + 1]] = i
    return mask, reg


def _noise(res, x, t0, m, cuda, in_stride=None, out_stride=None, stream=None, in_place=False):
    """input_noise on host blocks x [m, in_stride] (None: the draws themselves): [m, tot] of the output,
    whose buffer starts as NaN."""
    import torch

    tot = int(res.fb_offsets[-1])
    out_stride = tot if out_stride is None else out_stride
    d_in = None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(cuda).reshape(-1)
    if in_place:
        d_out = d_in
    else:
        d_out = torch.full((max(m, 1) * out_stride,), float("nan"), dtype=torch.float64, device=cuda)
    torch.cuda.synchronize()
    res.input_noise(d_in, d_out, t0, m, in_stride=in_stride, out_stride=out_stride, stream=stream)
    (stream if stream is not None else torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    full = d_out.cpu().numpy()[:m * out_stride].reshape(m, out_stride)
    if not in_place and out_stride > tot:
        assert np.isnan(full[:, tot:]).all(), "a write between the blocks"
    return full[:, :tot].copy()


def _blocks(m, tot, seed=3, pad=0):
    rng = np.random.default_rng(seed)
    x = np.full((m, tot + pad), np.nan)
    x[:, :tot] = rng.standard_normal((m, tot))
    return x


# ------------------------------------------------------------------ 1. the normals
@pytest.mark.parametrize("m", [3, 17])
def test_normals(cuda, m):
    res, _ = _atmo(load=False)
    off, ninp = _layout()
    res.set_input_noise(0.05, SEED)
    t0 = 5
    g = _noise(res, None, t0, m, cuda)
    want, R = nref.normals_ld(*nref.block_bits(SEED, IDS, ninp, t0, m))
    scale = U * np.maximum(R, 1).astype(np.float64)
    ratio = np.abs(g.astype(LD) - want).astype(np.float64) / scale
    print(f"m {m}: largest |g - g_ld| / (2^-53 max(sqrt(-2 log u1), 1)) = {ratio.max():.3f} (C_NORMAL {C_NORMAL})")
    assert np.isfinite(g).all()
    assert (ratio <= C_NORMAL).all(), ratio.max()
    assert (np.abs(g) <= nref.G_MAX + C_NORMAL * scale).all()
    res.close()


# ------------------------------------------------------------------ 2. plain entries
@pytest.mark.parametrize("mag", [0.05, 1e-300])
def test_plain_entries_are_exact(cuda, mag):
    res, _ = _atmo(load=False)
    tot = int(res.fb_offsets[-1])
    res.set_input_noise(mag, SEED)
    t0, m = 11, 5
    x = _blocks(m, tot, pad=3)
    g = _noise(res, None, t0, m, cuda)
    got = _noise(res, x, t0, m, cuda, in_stride=tot + 3)
    want = x[:, :tot] + (g * mag) * x[:, :tot]
    assert got.tobytes() == want.tobytes()
    assert mag < 1e-100 or (got != x[:, :tot]).mean() > 0.99
    res.close()


def test_zero_magnitude_copies_the_block(cuda):
    res, _ = _atmo(load=False)
    tot = int(res.fb_offsets[-1])
    res.set_input_noise(0.0, SEED, precip_epsilon=0.001)
    x = _blocks(3, tot)
    x[0, :7] = [-0.0, 0.0, np.inf, -np.inf, 5e-324, -1e308, np.nan]
    got = _noise(res, x, 2, 3, cuda)
    assert got.tobytes() == x.tobytes()
    assert _noise(res, x, 2, 3, cuda, in_place=True).tobytes() == x.tobytes()
    # the draws themselves do not depend on the magnitude
    g0 = _noise(res, None, 2, 3, cuda)
    res.set_input_noise(0.3, SEED)
    assert _noise(res, None, 2, 3, cuda).tobytes() == g0.tobytes()
    res.close()


# ------------------------------------------------------------------ 3. precip entries
def _adopt(res, cuda, seed=8):
    """Adopt statistics of the context's own: returns (mean, std) [nlocal, 36]."""
    import torch

    from speedy_ml_amd._lib import check, lib, ptr, stream_ptr

    rng = np.random.default_rng(seed)
    mean, std = rng.standard_normal((res.nlocal, 36)), 0.5 + rng.random((res.nlocal, 36))
    mean[:, 34], std[:, 34] = -2.0 + 0.5 * rng.standard_normal(res.nlocal), 1.0 + rng.random(res.nlocal)
    table = torch.from_numpy(np.concatenate([mean, std], axis=1)).to(cuda)
    check(lib().sml_res_set_mean_std_device(res.handle, ptr(table), stream_ptr(None)))
    return mean, std


def test_precip_entries(cuda):
    """precip_epsilon = 0.001, adopted statistics.  Slot-34 entries against the longdouble
    restatement on the device's own g.  The bound, per entry, to first order with u = 2^-53
    (one rounding) and k = K_FN 2^-52 (exp, log), every quantity the longdouble one:
        a1 = x s            a2 = a1 + m         E = exp(a2)      relative error of E: rE = u (|a1| + |a2|) + k
        d = E - 1           dd  = E rE + u |d|                   (the cancellation: E's absolute error stays
        p0 = eps d          dp0 = eps dd + u |p0|                 when d is small, so the bound is absolute)
        gm = g mag          dgm = u |gm|
        p1 = p0 + gm        dp1 = dp0 + dgm + u |p1|             (|.| changes no error)
        q = |p1| / eps      dq  = dp1 / eps + u q
        r = 1 + q           dr  = dq + u r
        L = log(r)          dL  = dr / r + k |L|                 (r >= 1)
        t = L - m           dt  = dL + u |t|
        y = t / s           dy  = dt / |s| + u |y|
    and the test allows 1.01 dy for the second-order terms.  Every other entry is plain, bit for
    bit; with precip_epsilon = 0 slot 34 is plain too."""
    res, _ = _atmo(load=False)
    tot = int(res.fb_offsets[-1])
    mean, std = _adopt(res, cuda)
    mask, reg = _precip_mask()
    assert mask.sum() == sum(ref.geometry(r)["inx"] * ref.geometry(r)["iny"] for r in IDS)
    mag, eps, t0, m = 0.05, 0.001, 4, 6
    x = _blocks(m, tot, seed=9)
    x[0, np.flatnonzero(mask)[:3]] = [0.0, -mean[reg[mask][0], 34] / std[reg[mask][0], 34], 30.0]  # E = 1 twice, a large one
    res.set_input_noise(mag, SEED, precip_epsilon=eps)
    g = _noise(res, None, t0, m, cuda)
    got = _noise(res, x, t0, m, cuda)
    plain = x + (g * mag) * x
    assert got[:, ~mask].tobytes() == plain[:, ~mask].tobytes()
    s, mu = std[reg[mask], 34].astype(LD), mean[reg[mask], 34].astype(LD)
    xl, gl = x[:, mask].astype(LD), g[:, mask].astype(LD)
    u, k = LD(U), LD(K_FN * 2.0 ** -52)
    a1 = xl * s
    a2 = a1 + mu
    E = np.exp(a2)
    d = E - 1
    dd = E * (u * (np.abs(a1) + np.abs(a2)) + k) + u * np.abs(d)
    p0 = eps * d
    dp0 = eps * dd + u * np.abs(p0)
    gm = gl * LD(mag)
    p1 = p0 + gm
    dp1 = dp0 + u * np.abs(gm) + u * np.abs(p1)
    q = np.abs(p1) / eps
    dq = dp1 / eps + u * q
    r = 1 + q
    dr = dq + u * r
    L = np.log(r)
    dL = dr / r + k * np.abs(L)
    t = L - mu
    dt = dL + u * np.abs(t)
    y = t / s
    dy = 1.01 * (dt / np.abs(s) + u * np.abs(y))
    err = np.abs(got[:, mask].astype(LD) - y)
    print(f"precip entries: largest error / bound {float((err / dy).max()):.3f}, largest bound {float(dy.max()):.2e}, "
          f"values within [{float(y.min()):.2f}, {float(y.max()):.2f}]")
    assert np.isfinite(got).all() and (err <= dy).all()
    assert (np.abs(got[:, mask] - plain[:, mask]) > 1e-6).mean() > 0.9  # the branch is on
    # precip_epsilon = 0: the reference's precip_bool = .false.
    res.set_input_noise(mag, SEED, precip_epsilon=0.0)
    assert _noise(res, x, t0, m, cuda).tobytes() == plain.tobytes()
    res.close()


# ------------------------------------------------------------------ 4. cutting and sharing
def test_cutting_strides_streams_and_contexts(cuda):
    import torch

    from speedy_ml_amd._lib import check, lib, ptr, stream_ptr
    from speedy_ml_amd.reservoir import Reservoirs

    res, _ = _atmo(load=False)
    off, ninp = _layout()
    tot = off[-1]
    _adopt(res, cuda)
    mag, eps = 0.05, 0.001
    res.set_input_noise(mag, SEED, precip_epsilon=eps)
    x = _blocks(8, tot, seed=13)
    whole = _noise(res, x, 0, 8, cuda)
    assert np.isfinite(whole).all()
    parts = np.concatenate([_noise(res, x[:3], 0, 3, cuda), _noise(res, x[3:], 3, 5, cuda)])
    assert parts.tobytes() == whole.tobytes()
    assert _noise(res, x, 0, 8, cuda, in_place=True).tobytes() == whole.tobytes()
    xp = np.full((8, tot + 5), np.nan)
    xp[:, :tot] = x
    assert _noise(res, xp, 0, 8, cuda, in_stride=tot + 5, out_stride=tot + 2).tobytes() == whole.tobytes()
    assert _noise(res, xp, 0, 8, cuda, in_stride=tot + 5, out_stride=tot + 5, in_place=True).tobytes() == whole.tobytes()
    # a side stream and a CU mask (the library's streams, destroyed below)
    h, hs = ctypes.c_void_p(), ctypes.c_void_p()
    ncu = torch.cuda.get_device_properties(cuda).multi_processor_count
    check(lib().sml_stream_create_cu_range(ncu // 2, 24, ctypes.byref(h)))
    check(lib().sml_stream_create_cu_range(0, ncu, ctypes.byref(hs)))
    try:
        for handle in (hs, h):
            st = torch.cuda.ExternalStream(handle.value, device=cuda)
            assert _noise(res, x, 0, 8, cuda, stream=st).tobytes() == whole.tobytes()
    finally:
        torch.cuda.synchronize()
        check(lib().sml_stream_destroy(h))
        check(lib().sml_stream_destroy(hs))
    # a context holding a subset of the regions: the matching rows of the full context
    pick = [1, 3, 5, 6]
    cols = np.concatenate([np.arange(off[i], off[i + 1]) for i in pick])
    sub, _ = _atmo([ref.CASES[i] for i in pick], load=False)
    full_ms = np.zeros((res.nlocal, 72))
    for i in range(res.nlocal):
        check(lib().sml_res_mean_std(res.handle, i, ptr(full_ms[i, :36]), ptr(full_ms[i, 36:])))
    check(lib().sml_res_set_mean_std_device(sub.handle, ptr(torch.from_numpy(full_ms[pick].copy()).to(cuda)),
                                            stream_ptr(None)))
    sub.set_input_noise(mag, SEED, precip_epsilon=eps)
    assert _noise(sub, x[:, cols], 0, 8, cuda).tobytes() == whole[:, cols].tobytes()
    # a generic context with ids: the geometry context's rows of those ids, plain entries
    res.set_input_noise(mag, SEED)
    plain = _noise(res, x, 0, 8, cuda)
    gn = [ninp[i] for i in pick]
    gen = Reservoirs([10, 11, 12, 13], [0] * 4, gn, [2 * v for v in gn], chunk_speedy=0, nout=4, ninp=gn,
                     out_index=[35] * 4)
    gen.set_input_noise(mag, SEED, precip_epsilon=eps, ids=[IDS[i] for i in pick])  # eps: no geometry, no precip branch
    assert _noise(gen, x[:, cols], 0, 8, cuda).tobytes() == plain[:, cols].tobytes()
    gen.set_input_noise(mag, SEED)  # ids None on a generic context: the local index
    own = _noise(gen, x[:, cols], 0, 8, cuda)
    g_own = nref.normals_ld(*nref.block_bits(SEED, [0, 1, 2, 3], gn, 0, 8))[0].astype(np.float64)
    assert np.abs(own - (x[:, cols] + (g_own * mag) * x[:, cols])).max() < 1e-13 and own.tobytes() != plain[:, cols].tobytes()
    for c in (res, sub, gen):
        c.close()


def test_setter_and_launcher_refusals(cuda):
    import torch

    from speedy_ml_amd import SmlError

    res, _ = _atmo(ref.CASES[:2])
    tot = int(res.fb_offsets[-1])
    z = torch.zeros(2 * tot, dtype=torch.float64, device=cuda)
    with pytest.raises(SmlError, match="before sml_res_set_input_noise"):
        res.input_noise(z, z, 0, 2)
    with pytest.raises(SmlError, match="negative"):
        res.set_input_noise(0.1, 1, ids=[3, -1])
    res.set_input_noise(0.1, 1)
    with pytest.raises(SmlError, match="out_stride"):
        res.input_noise(z, torch.zeros(4 * tot, dtype=torch.float64, device=cuda), 0, 2, out_stride=tot - 1)
    with pytest.raises(SmlError, match="in place"):
        res.input_noise(z, z, 0, 1, in_stride=tot + 1, out_stride=tot)
    z.fill_(2.0)
    res.input_noise(z, z, 0, 0)  # m = 0: a no-op
    torch.cuda.synchronize()
    assert (z == 2.0).all()
    res.predict_begin(z[:tot])
    with pytest.raises(SmlError, match="begun"):
        res.set_input_noise(0.1, 1)
    res.cancel_step()
    res.set_members(2)
    with pytest.raises(SmlError, match="members"):
        res.set_input_noise(0.1, 1)
    with pytest.raises(SmlError, match="members"):
        res.input_noise(z, z, 0, 1)
    res.close()


# ------------------------------------------------------------------ 5. NaN
def test_a_nan_stays_at_its_own_entry(cuda):
    res, _ = _atmo(load=False)
    tot = int(res.fb_offsets[-1])
    _adopt(res, cuda)
    mask, _ = _precip_mask()
    res.set_input_noise(0.05, SEED, precip_epsilon=0.001)
    x = _blocks(5, tot, seed=17)
    clean = _noise(res, x, 0, 5, cuda)
    assert np.isfinite(clean).all()
    for at in (int(np.flatnonzero(~mask)[100]), int(np.flatnonzero(mask)[5])):  # a plain entry, a precip entry
        y = x.copy()
        y[2, at] = np.nan
        got = _noise(res, y, 0, 5, cuda)
        assert np.isnan(got[2, at])
        got[2, at] = clean[2, at]
        assert got.tobytes() == clean.tobytes()
    res.close()


# ------------------------------------------------------------------ 6. moments
def test_moments_at_the_fixed_seed(cuda):
    """The conditions tests/test_input_noise_cpu.py asserts of the NumPy restatement at this
    seed, asserted of the device's draws."""
    res, _ = _atmo(load=False)
    off, ninp = _layout()
    res.set_input_noise(1.0, nref.MOMENT_SEED)
    g = _noise(res, None, nref.MOMENT_T0, nref.MOMENT_M, cuda)
    N = g.size
    assert N >= 2 ** 18 and np.isfinite(g).all()
    mean, var, re, rt = nref.moments(g, ninp)
    cm, cv, cr = nref.moment_caps(N)
    print(f"N {N}: mean {mean:+.3e} (cap {cm:.3e}), var - 1 {var - 1:+.3e} (cap {cv:.3e}), "
          f"lag-1 along e {re:+.3e}, along t {rt:+.3e} (cap {cr:.3e})")
    assert abs(mean) <= cm and abs(var - 1.0) <= cv and abs(re) <= cr and abs(rt) <= cr
    res.close()


# ------------------------------------------------------------------ 7. the drive
def _wide_generic():
    """A generic context with a target table: ninp 48 and 1040 (past the drive's one-register
    input path, ninp > 1024)."""
    from speedy_ml_amd.reservoir import Reservoirs

    regions, ninp = [10, 500], [48, 1040]
    n = [96, 1040]
    res = Reservoirs(regions, [0, 0], n, [6 * v for v in n], chunk_speedy=0, nout=4, ninp=ninp, out_index=[35] * 4)
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
    res.set_target_index(np.array([[3, 47, 0, 20], [1039, 1024, 5, 600]], dtype=np.int32))
    return res


def _geometry_ctx():
    from speedy_ml_amd.synthetic import initial_state

    res, ws = _atmo(ref.CASES[:4])
    for i, w in enumerate(ws):
        res.set_state(i, initial_state(w.region, w.n))
    return res


def _drive(make, stepwise, inputs, model, m, cuda, target_inputs=None, pad=0, tpad=0):
    """(states, targets, final states) of one drive over m blocks on a fresh context; the
    buffers start as NaN."""
    import torch

    res = make()
    if stepwise:
        res.set_reference_paths(stepwise_drive=True)
    tot = int(res.fb_offsets[-1])
    naug = sum(res.ncs + int(n) for n in res.n)

    def dev(a, p):
        b = np.full((m, a.shape[1] + p), np.nan)
        b[:, :a.shape[1]] = a[:m]
        return torch.from_numpy(b).to(cuda).reshape(-1)

    d_s = torch.full((naug * m,), float("nan"), dtype=torch.float64, device=cuda)
    d_t = torch.full((res.nlocal * m * res.nout,), float("nan"), dtype=torch.float64, device=cuda)
    kw = {}
    if target_inputs is not None:
        kw = dict(target_inputs=dev(target_inputs, tpad), target_stride=tot + tpad)
    res.train_drive(dev(inputs, pad), m, torch.from_numpy(model[:m].copy()).to(cuda) if res.ncs else None, d_s, d_t,
                    stride=tot + pad, **kw)
    torch.cuda.synchronize()
    out = d_s.cpu().numpy(), d_t.cpu().numpy(), np.concatenate([res.get_state(i) for i in range(res.nlocal)])
    res.close()
    return out


@pytest.mark.parametrize("stepwise", [False, True])
@pytest.mark.parametrize("ctx", ["geometry", "generic"])
def test_drive_from(cuda, ctx, stepwise):
    """target_inputs = inputs is train_drive bit for bit; with distinct series the states are
    the driving series' and the targets the target series', bit for bit."""
    make = _geometry_ctx if ctx == "geometry" else _wide_generic
    probe = make()
    tot, nmod = int(probe.fb_offsets[-1]), probe.nlocal * probe.ncs
    assert (max(probe.ninp(i) for i in range(probe.nlocal)) > 1024) == (ctx == "generic")
    probe.close()
    rng = np.random.default_rng(31)
    noisy, clean = rng.standard_normal((17, tot)), rng.standard_normal((17, tot))
    model = 2.0 * rng.random((17, max(nmod, 1))) - 1.0
    for m in (1, 2, 17):
        base = _drive(make, stepwise, noisy, model, m, cuda)
        assert all(np.isfinite(a).all() for a in base)
        same = _drive(make, stepwise, noisy, model, m, cuda, target_inputs=noisy)
        for a, b in zip(base, same):
            assert a.tobytes() == b.tobytes(), (m, "target_inputs = inputs")
        tbase = _drive(make, stepwise, clean, model, m, cuda)
        two = _drive(make, stepwise, noisy, model, m, cuda, target_inputs=clean, pad=3, tpad=7)
        assert two[0].tobytes() == base[0].tobytes() and two[2].tobytes() == base[2].tobytes(), (m, "states")
        assert two[1].tobytes() == tbase[1].tobytes() and two[1].tobytes() != base[1].tobytes(), (m, "targets")


# ------------------------------------------------------------------ 8. end to end
W_TOL = 1e-9  # tests/test_train_drive_gpu.py: max |dW| <= 1e-9 max |W| against the oracle chain


def _squared(x):
    xt = x.copy()
    xt[1::2] = x[1::2] * x[1::2]
    return xt


def test_train_wout_with_noise_against_the_oracle_chain(cuda):
    """train_wout(noise=...) on the shapes of tests/test_train_drive_gpu.py's end-to-end test
    (whose tolerance this is): the oracle's update loop driven by the noised blocks read back
    from the device, its targets from the clean blocks.  noise=None: the chain of public calls
    as it was, bit for bit.  Two seeds differ, one seed repeats its bits."""
    import torch

    import oracle
    from test_train_drive_gpu import _numpy_target_index
    from speedy_ml_amd.reservoir import Reservoirs
    from speedy_ml_amd.training import InputNoise, Trainer, train_wout

    cases, discard, batch, nbatches = [(5, True), (24, False)], 5, 16, 2
    kw = dict(ncs=NCS, beta_res=0.5, beta_model=1.0, using_prior=False, dtype=np.float64)

    def context():
        ws = [region_weights(r, s, n_override=300) for r, s in cases]
        res = Reservoirs([w.region for w in ws], [w.sst for w in ws], [w.n for w in ws], [w.k for w in ws])
        for i, w in enumerate(ws):
            res.load_region_weights(i, w)
        return res, ws

    res, ws = context()
    nblocks, tot = discard + batch * nbatches, int(res.fb_offsets[-1])
    rng = np.random.default_rng(77)
    inputs = rng.standard_normal((nblocks, tot))
    model = 2.0 * rng.random((nblocks, res.nlocal * NCS)) - 1.0
    d_in, d_mod = torch.from_numpy(inputs).to(cuda), torch.from_numpy(model).to(cuda)
    noise = InputNoise(0.05, 11, precip_epsilon=0.001)
    got, info = train_wout(res, d_in, d_mod, discard, batch, nbatches, noise=noise, **kw)
    assert (info == 0).all()
    # the noised blocks, read back: one call over the series with the same configuration
    noisy = res.input_noise(d_in.reshape(-1), torch.empty(nblocks * tot, dtype=torch.float64, device=cuda), 0, nblocks)
    torch.cuda.synchronize()
    noisy = noisy.cpu().numpy().reshape(nblocks, tot)
    assert np.isfinite(noisy).all() and (noisy != inputs).mean() > 0.99
    offs = res.fb_offsets
    for i, w in enumerate(ws):
        col, val = w.win_compressed()
        u, uc = noisy[:, offs[i]:offs[i + 1]], inputs[:, offs[i]:offs[i + 1]]
        tidx = _numpy_target_index(w.region)
        x = np.zeros(w.n)

        def upd(x, fb):
            return oracle.predict_f32(w.rows, w.cols, w.vals, col, val, w.wout, fb, np.zeros(NCS), x, w.mean, w.std)[1]

        for t in range(discard):
            x = upd(x, u[t])
        naug = NCS + w.n
        G, B = np.zeros((naug, naug)), np.zeros((naug, 136))
        for b in range(nbatches):
            S, T = np.zeros((batch, naug)), np.zeros((batch, 136))
            for c in range(batch):
                t = discard + b * batch + c
                S[c, :NCS], S[c, NCS:], T[c] = model[t, i * NCS:(i + 1) * NCS], _squared(x), uc[t, tidx]
                x = upd(x, u[t])
            oracle.train_accumulate(S, T, G, B)
        wo, oinfo = oracle.train_solve(G, B, NCS, 0.5, 1.0, False, 0.0)
        assert oinfo == 0
        err = np.abs(got[i] - wo).max()
        print(f"region {w.region}: max |dW| {err:.3e} vs {W_TOL * np.abs(wo).max():.3e}")
        assert err <= W_TOL * np.abs(wo).max()
    # the same seed again: the same bits; another seed: other weights
    res2, _ = context()
    again, _ = train_wout(res2, d_in, d_mod, discard, batch, nbatches, noise=noise, **kw)
    res3, _ = context()
    other, _ = train_wout(res3, d_in, d_mod, discard, batch, nbatches, noise=InputNoise(0.05, 12, 0.001), **kw)
    for a, b, c in zip(got, again, other):
        assert a.tobytes() == b.tobytes() and np.abs(a - c).max() > 1e-6 * np.abs(a).max()
    # noise=None: the chain as it was
    res4, _ = context()
    plain, _ = train_wout(res4, d_in, d_mod, discard, batch, nbatches, **kw)
    res5, _ = context()
    naug = [NCS + int(n) for n in res5.n]
    for i, n in enumerate(res5.n):
        res5.set_state(i, np.zeros(int(n)))
    flat, fmod = d_in.reshape(-1), d_mod.reshape(-1)
    res5.synchronize(flat, discard)
    tr = Trainer(naug, 136)
    tr.reset()
    states = torch.empty(sum(naug) * batch, dtype=torch.float64, device=cuda)
    targets = torch.empty(len(naug) * batch * 136, dtype=torch.float64, device=cuda)
    for b in range(nbatches):
        t0 = discard + b * batch
        res5.train_drive(flat[t0 * tot:], batch, fmod[t0 * res5.nlocal * NCS:], states, targets)
        tr.accumulate(states, targets, batch)
    packed, _ = tr.solve(ncs=NCS, beta_res=0.5, beta_model=1.0, using_prior=False)
    for a, v, g in zip(plain, tr.wout_views(packed), got):
        assert a.tobytes() == v.cpu().numpy().tobytes() and np.abs(a - g).max() > 1e-6 * np.abs(a).max()
    tr.close()
    for c in (res, res2, res3, res4, res5):
        c.close()


T, DISCARD, BATCH, NBATCHES = 40, 8, 15, 2


def _host(seed=21):
    rng = np.random.default_rng(seed)
    g4 = rng.standard_normal((T, 8, 48, 96, 4)) * np.array([8.0, 6.0, 12.0, 2e-3]) + np.array([3.0, -1.0, 255.0, 4e-3])
    g2, pr = 0.02 * rng.standard_normal((T, 48, 96)) - 0.05, np.abs(rng.standard_normal((T, 48, 96)))
    sst, tisr = 285.0 + 8.0 * rng.standard_normal((T, 48, 96)), 300.0 * rng.random((T, 48, 96))
    fc4 = g4 + 0.1 * rng.standard_normal(g4.shape) * np.array([8.0, 6.0, 12.0, 2e-3])
    fc2 = g2 + 0.001 * rng.standard_normal(g2.shape)
    return g4, g2, pr, sst, tisr, fc4, fc2


def test_train_from_grids_with_noise_is_the_chain_of_public_calls(cuda):
    import torch

    from speedy_ml_amd.training import InputNoise, Trainer, fit_standardisation, tile_series, train_from_grids

    cases = [(0, True), (245, True), (246, False), (1151, False)]
    g4, g2, pr, sst, tisr, fc4, fc2 = (torch.from_numpy(a).to(cuda) for a in _host())
    kw = dict(ncs=NCS, beta_res=0.5, beta_model=1.0, using_prior=False, dtype=np.float64)
    noise = InputNoise(0.05, 5, precip_epsilon=0.001)
    res, ws = _atmo(cases)
    got, info, mean, std = train_from_grids(res, (g4, g2, pr, sst, tisr), (fc4, fc2), DISCARD, BATCH, NBATCHES, noise=noise,
                                            **kw)
    assert (info == 0).all() and all(np.isfinite(w).all() for w in got)
    # by hand
    res2, _ = _atmo(cases)
    fit_standardisation(res2, g4, g2, pr, sst, tisr)
    res2.set_input_noise(0.05, 5, 0.001)
    tot = int(res2.fb_offsets[-1])
    naug = [NCS + int(n) for n in res2.n]
    for i, n in enumerate(res2.n):
        res2.set_state(i, np.zeros(int(n)))
    noisy = torch.empty(BATCH * tot, dtype=torch.float64, device=cuda)

    def tiled(t0, m):
        return tile_series(res2, g4[t0:t0 + m], g2[t0:t0 + m], pr[t0:t0 + m], sst[t0:t0 + m], tisr[t0:t0 + m],
                           fc4[t0:t0 + m], fc2[t0:t0 + m])

    clean, _ = tiled(0, DISCARD)
    res2.synchronize(res2.input_noise(clean, noisy, 0, DISCARD), DISCARD)
    tr = Trainer(naug, 136)
    tr.reset()
    states = torch.empty(sum(naug) * BATCH, dtype=torch.float64, device=cuda)
    targets = torch.empty(len(naug) * BATCH * 136, dtype=torch.float64, device=cuda)
    for b in range(NBATCHES):
        t0 = DISCARD + b * BATCH
        clean, mod = tiled(t0, BATCH)
        res2.input_noise(clean, noisy, t0, BATCH)
        res2.train_drive(noisy, BATCH, mod, states, targets, target_inputs=clean)
        tr.accumulate(states, targets, BATCH)
    packed, info2 = tr.solve(ncs=NCS, beta_res=0.5, beta_model=1.0, using_prior=False)
    assert (info2 == 0).all()
    for a, v in zip(got, tr.wout_views(packed)):
        assert a.tobytes() == v.cpu().numpy().tobytes()
    tr.close()
    # the noise changes the weights; the precip branch is part of it
    res3, _ = _atmo(cases)
    plain, _, _, _ = train_from_grids(res3, (g4, g2, pr, sst, tisr), (fc4, fc2), DISCARD, BATCH, NBATCHES, **kw)
    res4, _ = _atmo(cases)
    noeps, _, _, _ = train_from_grids(res4, (g4, g2, pr, sst, tisr), (fc4, fc2), DISCARD, BATCH, NBATCHES,
                                      noise=InputNoise(0.05, 5), **kw)
    for a, b, c in zip(got, plain, noeps):
        assert a.tobytes() != b.tobytes() and a.tobytes() != c.tobytes()
    for c in (res, res2, res3, res4):
        c.close()


def test_train_slab_from_grids_with_noise(cuda):
    """Bit for bit the chain of public calls (the averaged series noised whole, t = the column's
    index, ids = the sst regions' global ids); against the oracle chain run on the noised series
    read back, targets from the clean one, within tests/test_slab_train_gpu.py's W_TOL."""
    import torch

    import _slab_series_ref as sref
    import oracle
    from speedy_ml_amd.reservoir import Reservoirs
    from speedy_ml_amd.training import InputNoise, Trainer, slab_series, train_slab_from_grids

    S, discard, batch, nbatches, window, divisor, beta = 3, 2, 5, 2, 3, 2, 0.5
    dev = tuple(torch.from_numpy(a).to(cuda) for a in _host(23)[:5])

    def contexts():
        atmo, ws = _atmo(ncs=NCS)
        sreg = [r for r, s in ref.CASES if s]
        sws = [slab_weights(r, n_override=2 * 7 * 16) for r in sreg]
        slab = Reservoirs(sreg, [0] * len(sreg), [w.n for w in sws], [w.k for w in sws], chunk_speedy=0, nout=4,
                          ninp=[w.ninp for w in sws], out_index=[35] * 4)
        for j, w in enumerate(sws):
            slab.load_region_weights(j, w)
        return atmo, slab, sws

    noise = InputNoise(0.05, 9, precip_epsilon=0.001)
    atmo, slab, sws = contexts()
    got, info, _, _ = train_slab_from_grids(atmo, slab, dev, window, divisor, S, discard, batch, nbatches, beta_res=beta,
                                            dtype=np.float64, noise=noise)
    assert (info == 0).all()
    # by hand
    atmo2, slab2, _ = contexts()
    series = slab_series(atmo2, slab2, *dev, window, divisor)
    tidx = np.stack([slab2.slab_target_index(j) for j in range(slab2.nlocal)])
    slab2.set_target_index(tidx)
    slab2.set_input_noise(0.05, 9, 0.001, ids=slab2.region_ids)
    noisy = slab2.input_noise(series, torch.empty_like(series), 0, T)
    tot = int(slab2.fb_offsets[-1])
    naug = [int(n) for n in slab2.n]
    tr = Trainer(naug, 4)
    tr.reset()
    states = torch.empty(sum(naug) * batch, dtype=torch.float64, device=cuda)
    targets = torch.empty(len(naug) * batch * 4, dtype=torch.float64, device=cuda)
    for i in range(S):
        torch.cuda.synchronize()
        for j, n in enumerate(naug):
            slab2.set_state(j, np.zeros(n))
        slab2.synchronize(noisy[i * tot:], discard, stride=S * tot)
        for b in range(nbatches):
            col = i + (discard + b * batch) * S
            slab2.train_drive(noisy[col * tot:], batch, None, states, targets, stride=S * tot,
                              target_inputs=series[col * tot:], target_stride=S * tot)
            tr.accumulate(states, targets, batch)
    packed, info2 = tr.solve(ncs=0, beta_res=beta, using_prior=False)
    assert (info2 == 0).all()
    for a, v in zip(got, tr.wout_views(packed)):
        assert np.isfinite(a).all() and a.tobytes() == v.cpu().numpy().tobytes()
    tr.close()
    # the noised series is the plain formula on the clean one, ids = the sst regions' global ids
    a, an = series.cpu().numpy().reshape(T, tot), noisy.cpu().numpy().reshape(T, tot)
    soff = sref.slab_offsets(ref.CASES)
    sids = [int(r) for r in slab2.region_ids]
    g = nref.normals_ld(*nref.block_bits(9, sids, [int(v) for v in np.diff(soff)], 0, T))[0].astype(np.float64)
    assert np.abs(an - (a + (g * 0.05) * a)).max() <= 1e-13 * (1 + np.abs(a).max())
    # the oracle chain
    for j, w in enumerate(sws):
        col, val = w.win_compressed()
        u, uc = an[:, soff[j]:soff[j + 1]], a[:, soff[j]:soff[j + 1]]

        def upd(x, fb):
            return oracle.predict_slab_ml_f32(w.rows, w.cols, w.vals, col, val, w.wout, fb, x, w.mean[35], w.std[35])[1]

        So, To = [], []
        for i in range(S):
            x = np.zeros(w.n)
            for k in range(discard + batch * nbatches):
                c = i + k * S
                if k >= discard:
                    So.append(_squared(x))
                    To.append(uc[c, tidx[j]])
                x = upd(x, u[c])
        Go, Bo = np.zeros((w.n, w.n)), np.zeros((w.n, 4))
        oracle.train_accumulate(np.array(So), np.array(To), Go, Bo)
        wo, oinfo = oracle.train_solve(Go, Bo, 0, beta, 1.0, False, 0.0)
        assert oinfo == 0
        err = np.abs(got[j] - wo).max()
        print(f"slab {w.region}: |W - oracle| {err:.3e} (max |W| {np.abs(wo).max():.3e})")
        assert err <= W_TOL * np.abs(wo).max(), (j, err)
    # noise=None: the same call without it gives other weights, and what it gave before
    atmo3, slab3, _ = contexts()
    plain, _, _, _ = train_slab_from_grids(atmo3, slab3, dev, window, divisor, S, discard, batch, nbatches, beta_res=beta,
                                           dtype=np.float64)
    assert all(p.tobytes() != q.tobytes() for p, q in zip(plain, got))
    for c in (atmo, slab, atmo2, slab2, atmo3, slab3):
        c.close()
