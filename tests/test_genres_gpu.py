"""The spectral radius of every region's A on the GPU (sml_res_spectral_radius,
k_res_radius) and reservoir generation on top of it (speedy_ml_amd.genres).

Gate 1: the GPU's enclosure [lo, hi] holds the longdouble radius of
tests/test_genres_cpu.py within g = (L + 2) 2^-53 (derived there), is no wider than
tol hi, and reports info 0 -- on every shape of GPU_SHAPES, at tol 2e-14 and 1e-10.
Gate 2: lo, hi and iters are the same bits whatever the context, the held precision,
the place of x and y (LDS or the context's scratch), the call and the stream.
After genres.generate the loaded A has rho = radius within 2^-24 + 3 tol (f32 weights:
an entrywise relative perturbation eps of a non-negative matrix moves its Perron root
by at most eps, and the rounding to float32 is eps <= 2^-24; the 3 tol covers the two
enclosures' half widths and the scaling's own roundings) or 3 tol + 4 2^-53 (f64).
"""
import functools

import numpy as np
import pytest

from speedy_ml_amd import SmlError
from speedy_ml_amd.domain import radius_by_region, reservoir_sizes
from speedy_ml_amd.synthetic import climatology_mean_std, initial_state, local_model_vector
from test_genres_cpu import GPU_SHAPES, SEED, check_enclosure, gpu_matrix, reference_radius

pytestmark = pytest.mark.gpu

TOL = 2e-14
F32_BOUND = 2.0 ** -24 + 3 * TOL
F64_BOUND = 3 * TOL + 4 * 2.0 ** -53


def _context(mats, weight_dtype="f32"):
    """A generic context (one input, one output, no local model) holding the matrices
    (n, k, rows, cols, vals) as its regions' A."""
    from speedy_ml_amd.reservoir import Reservoirs

    nl = len(mats)
    res = Reservoirs(list(range(nl)), [0] * nl, [m[0] for m in mats], [m[1] for m in mats], chunk_speedy=0, nout=1,
                     weight_dtype=weight_dtype, ninp=[1] * nl, out_index=[-1])
    for i in range(nl):
        _load(res, i, mats[i])
    return res


def _load(res, i, mat):
    n, k, rows, cols, vals = mat
    dt = np.float32 if res.weight_dtype == "f32" else np.float64
    res.load_region(i, rows, cols, np.asarray(vals, dtype=dt), np.ones((1, n), dtype=dt), np.zeros((n, 1), dtype=dt),
                    np.zeros(36), np.ones(36))


def _bits(r):
    lo, hi, iters, info = r
    return lo.view(np.uint64).tolist(), hi.view(np.uint64).tolist(), iters.tolist(), info.tolist()


@functools.lru_cache(maxsize=None)
def _shapes_context(weight_dtype="f32"):
    return _context([gpu_matrix(j) for j in range(len(GPU_SHAPES))], weight_dtype)


@functools.lru_cache(maxsize=None)
def _shapes_result(tol=TOL):
    """The default form's result on the GPU_SHAPES context (read only)."""
    return _shapes_context().spectral_radius(tol=tol)


@pytest.mark.parametrize("tol", [2e-14, 1e-10])
def test_enclosure_holds_the_longdouble_radius(cuda, tol):
    lo, hi, iters, info = _shapes_result(tol)
    for j, (n, k) in enumerate(GPU_SHAPES):
        rho_ref, L = reference_radius(j)
        print(f"n {n} k {k} L {L} tol {tol:g}: iters {iters[j]} info {info[j]} lo {lo[j]!r} hi {hi[j]!r} "
              f"rho_ref {rho_ref!r}")
    for j in range(len(GPU_SHAPES)):
        rho_ref, L = reference_radius(j)
        check_enclosure(lo[j], hi[j], info[j], tol, rho_ref, L)


def _small_matrix(i):
    from speedy_ml_amd.genres import generate_region

    n = (1, 2, 7, 63, 64, 65, 300, 777, 1023, 1025, 2000)[i % 11]
    rows, cols, vals, _, _ = generate_region(n, 6 * n, 1, SEED, 100 + i, 0.5)
    return n, 6 * n, rows, cols, vals


def test_alone_and_inside_a_mixed_context(cuda):
    """96 regions of mixed n whose blocks finish at different iterations; regions of
    the GPU_SHAPES context, computed there, sit among them."""
    inside = {5: 2, 17: 7, 40: 11, 41: 9, 77: 12, 95: 0}  # position in the 96 -> GPU_SHAPES index
    mats = [gpu_matrix(inside[i]) if i in inside else _small_matrix(i) for i in range(96)]
    lo, hi, iters, info = _context(mats).spectral_radius()
    assert (info == 0).all()
    assert len(set(iters.tolist())) > 5
    blo, bhi, bit, _ = _shapes_result()
    for i, j in inside.items():
        assert (lo[i].view(np.uint64), hi[i].view(np.uint64), iters[i]) == \
            (blo[j].view(np.uint64), bhi[j].view(np.uint64), bit[j]), GPU_SHAPES[j]
    for i in (0, 8, 30, 43):  # small regions alone
        alone = _context([mats[i]]).spectral_radius()
        assert _bits(alone) == _bits((lo[i:i + 1], hi[i:i + 1], iters[i:i + 1], info[i:i + 1])), mats[i][0]


def test_f64_held_context_gives_the_same_bits(cuda):
    assert _bits(_shapes_context("f64").spectral_radius()) == _bits(_shapes_result())


def test_global_scratch_form_gives_the_same_bits(cuda):
    res = _shapes_context()
    res.set_reference_paths(radius_global=True)
    try:
        forced = res.spectral_radius()
    finally:
        res.set_reference_paths()
    assert _bits(forced) == _bits(_shapes_result())
    assert _bits(res.spectral_radius()) == _bits(_shapes_result())  # and back in LDS


def test_successive_calls_and_a_side_stream(cuda):
    import torch

    res = _shapes_context()
    assert _bits(res.spectral_radius()) == _bits(_shapes_result())
    side = torch.cuda.Stream()
    assert _bits(res.spectral_radius(stream=side)) == _bits(_shapes_result())


def test_known_answers(cuda):
    rng = np.random.default_rng(3)
    n = 100
    halves = (n, 6 * n, np.repeat(np.arange(1, n + 1), 6), rng.integers(1, n + 1, 6 * n), np.full(6 * n, 0.5))
    perm = (50, 50, np.arange(1, 51), rng.permutation(50) + 1, np.ones(50))
    cyc = (2, 2, np.array([1, 2]), np.array([2, 1]), np.array([2.0, 1.0]))  # [[0, 2], [1, 0]]: imprimitive
    zero = (9, 12, rng.integers(1, 10, 12), rng.integers(1, 10, 12), np.zeros(12))
    lo, hi, iters, info = _context([halves, perm, cyc, zero]).spectral_radius(max_iter=50)
    assert (lo[0], hi[0], iters[0], info[0]) == (3.0, 3.0, 1, 0)
    assert (lo[1], hi[1], iters[1], info[1]) == (1.0, 1.0, 1, 0)
    assert (lo[2], hi[2], iters[2], info[2]) == (1.0, 2.0, 50, 1)  # bounded: nothing loops past max_iter
    assert (lo[3], hi[3], info[3]) == (0.0, 0.0, 2)
    # one negative entry: that region alone is refused
    neg = list(_small_matrix(6))
    neg[4] = neg[4].copy()
    neg[4][123] = -0.5
    lo, hi, iters, info = _context([_small_matrix(7), tuple(neg), _small_matrix(6)]).spectral_radius()
    assert np.isnan(lo[1]) and np.isnan(hi[1]) and info[1] == 3
    for i, j in ((0, 7), (2, 6)):
        alone = _context([_small_matrix(j)]).spectral_radius()
        assert info[i] == 0 and _bits(alone) == _bits((lo[i:i + 1], hi[i:i + 1], iters[i:i + 1], info[i:i + 1]))


def test_error_paths(cuda):
    from speedy_ml_amd.reservoir import Reservoirs

    m = _small_matrix(2)
    res = Reservoirs([0, 1], [0, 0], [m[0], m[0]], [m[1], m[1]], chunk_speedy=0, nout=1, ninp=[1, 1], out_index=[-1])
    _load(res, 0, m)
    with pytest.raises(SmlError, match="error -4"):  # SML_ERR_STATE: region 1 not loaded
        res.spectral_radius()
    _load(res, 1, m)
    for kw in (dict(tol=0.0), dict(tol=-1e-3), dict(tol=float("nan")), dict(max_iter=0)):
        with pytest.raises(SmlError, match="error -1"):
            res.spectral_radius(**kw)
    assert (res.spectral_radius()[3] == 0).all()


# ------------------------------------------------------------------------ generate
T30_CASES = [(0, False), (5, True), (23, True), (24, False), (30, False), (600, True), (601, False), (1151, False)]


def _t30_context(cases, full=False):
    """Atmosphere reservoirs: at n_override = 96 a region has one node per input
    (n = ninp, k = 6 n, as synthetic.region_weights shrinks it); full = the real sizes."""
    from speedy_ml_amd.reservoir import Reservoirs

    sz = [reservoir_sizes(r, s) for r, s in cases]
    n = [z.n if full else z.ninp for z in sz]
    k = [z.k if full else 6 * z.ninp for z in sz]
    return Reservoirs([r for r, _ in cases], [s for _, s in cases], n, k)


def _check_generated(res, ws, radius, bound):
    lo, hi, _, info = res.spectral_radius()
    assert (info == 0).all()
    rho = (lo + hi) / 2
    for i, w in enumerate(ws):
        dev = abs(rho[i] / radius[i] - 1)
        print(f"region {w.region} n {w.n}: rho / radius - 1 = {rho[i] / radius[i] - 1:.3e} (bound {bound:.3e})")
        assert dev <= bound
        # the block-diagonal W_in is found: its column computed from the row (win_q = q);
        # at one node per input the layout keeps the column list (its 32-bit multiplier
        # cannot express q = 1) in the one-entry-per-row form
        q, lay = w.n // w.ninp, res.ell_layout(i)
        assert lay["win_ell"] and lay["win_q"] == (q if q >= 2 else 0)
        if w.n <= 1025:
            a = np.zeros((w.n, w.n))
            np.add.at(a, (w.rows - 1, w.cols - 1), w.vals.astype(np.float64))
            eig = np.abs(np.linalg.eigvals(a)).max()
            print(f"region {w.region} n {w.n}: eigvals rho / radius - 1 = {eig / radius[i] - 1:.3e}")
            assert abs(eig / radius[i] - 1) <= bound + 1e-12


@functools.lru_cache(maxsize=None)
def _generated_eight():
    from speedy_ml_amd.genres import generate

    res = _t30_context(T30_CASES)
    mean, std = climatology_mean_std()
    radius = [radius_by_region(r) for r, _ in T30_CASES]
    ws, rho = generate(res, SEED, radius, 0.5, mean, std)
    return res, ws, rho, radius


def test_generate_scales_to_the_radius(cuda):
    res, ws, rho, radius = _generated_eight()
    assert {bool(w.sst) for w in ws} == {True, False}
    assert ((rho > 2.3) & (rho < 3.3)).all()
    for w in ws:
        assert w.vals.dtype == np.float32 and not w.wout.any()
    _check_generated(res, ws, radius, F32_BOUND)


def test_generate_at_full_size(cuda):
    from speedy_ml_amd.genres import generate

    res = _t30_context([(30, False)], full=True)
    assert (int(res.n[0]), int(res.k[0]), res.ninp(0)) == (6160, 37945, 560)
    mean, std = climatology_mean_std()
    ws, rho = generate(res, SEED, radius_by_region(30), 0.5, mean, std)
    _check_generated(res, ws, [radius_by_region(30)], F32_BOUND)


@pytest.mark.parametrize("weight_dtype,bound", [("f32", F32_BOUND), ("f64", F64_BOUND)])
def test_generate_on_a_generic_context(cuda, weight_dtype, bound):
    """The slab ocean's shape of context (radius 0.9, sigma 0.6), small enough for
    numpy.linalg.eigvals of the dense matrix."""
    from speedy_ml_amd.genres import generate
    from speedy_ml_amd.reservoir import Reservoirs

    n, ninp = [96, 504], [12, 63]
    res = Reservoirs([7, 8], [0, 0], n, [6 * v for v in n], chunk_speedy=0, nout=4, weight_dtype=weight_dtype,
                     ninp=ninp, out_index=[35] * 4)
    mean, std = climatology_mean_std()
    ws, rho = generate(res, SEED, 0.9, 0.6, mean, std)
    assert ws[0].vals.dtype == (np.float32 if weight_dtype == "f32" else np.float64)
    assert all(np.abs(w.win).max() <= 0.6 for w in ws)
    _check_generated(res, ws, [0.9] * 2, bound)


def test_generate_does_not_depend_on_the_context(cuda):
    """Regions 5 and 600 drawn in a context of two and in the context of eight."""
    from speedy_ml_amd.genres import generate

    _, ws8, rho8, _ = _generated_eight()
    cases = [(5, True), (600, True)]
    res = _t30_context(cases)
    mean, std = climatology_mean_std()
    ws2, rho2 = generate(res, SEED, [radius_by_region(r) for r, _ in cases], 0.5, mean, std)
    for w2, r2 in zip(ws2, rho2):
        i8 = [w.region for w in ws8].index(w2.region)
        assert r2.view(np.uint64) == rho8[i8].view(np.uint64)
        for name in ("rows", "cols", "vals", "win"):
            np.testing.assert_array_equal(getattr(w2, name), getattr(ws8[i8], name), err_msg=name)


def test_generate_train_write_read_predict(cuda, tmp_path):
    """From nothing but a series to a weight file: generate, train_wout, write, read, and
    the file's weights in a fresh context predict bit for bit what the trained context does."""
    import torch

    from speedy_ml_amd.genres import generate
    from speedy_ml_amd.reservoir import read_region_netcdf, write_region_netcdf
    from speedy_ml_amd.training import train_wout

    cases, discard, batch, nbatches = [(5, True), (24, False)], 5, 16, 2
    radius = [radius_by_region(r) for r, _ in cases]
    res = _t30_context(cases)
    mean, std = climatology_mean_std()
    ws, _ = generate(res, SEED, radius, 0.5, mean, std)
    nblocks, tot = discard + batch * nbatches, int(res.fb_offsets[-1])
    rng = np.random.default_rng(77)
    inputs = rng.standard_normal((nblocks, tot))
    model = 2.0 * rng.random((nblocks, res.nlocal * res.ncs)) - 1.0
    wouts, info = train_wout(res, torch.from_numpy(inputs).to(cuda), torch.from_numpy(model).to(cuda), discard, batch,
                             nbatches, ncs=res.ncs, beta_res=0.5, beta_model=1.0, using_prior=False)
    assert (info == 0).all()
    fresh = _t30_context(cases)
    for i, w in enumerate(ws):
        w.wout = wouts[i]
        assert w.wout.any() and np.isfinite(w.wout).all()
        res.load_region_weights(i, w)
        path = str(tmp_path / f"worker_{w.region:04d}_level_1_gen.nc")
        write_region_netcdf(path, w.win, w.wout, w.rows, w.cols, w.vals, w.mean, w.std)
        d = read_region_netcdf(path)
        for name in ("rows", "cols", "vals", "win", "wout"):
            np.testing.assert_array_equal(d[name], getattr(w, name), err_msg=name)
        fresh.load_netcdf(i, path)
    lo, hi, _, info = fresh.spectral_radius()
    assert (info == 0).all()
    for i in range(len(cases)):
        assert abs((lo[i] + hi[i]) / 2 / radius[i] - 1) <= F32_BOUND
    fb = rng.standard_normal(tot)
    lm = np.stack([local_model_vector(w.region) for w in ws])
    for ctx in (res, fresh):
        for i, w in enumerate(ws):
            ctx.set_state(i, initial_state(w.region, w.n))
    np.testing.assert_array_equal(fresh.predict_host(fb, lm), res.predict_host(fb, lm))
