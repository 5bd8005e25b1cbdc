"""Reservoir generation on the host (sml_gen_region) and the yardstick of the GPU's
spectral radius (tests/test_genres_gpu.py).  No GPU: the library loads without one.

The generator's recipe (csrc/sml_genres.cpp's header comment) is restated here in NumPy
uint64 arithmetic and must match bit for bit.  The float64 model of the power iteration
(sml_res_spectral_radius, include/speedy_ml.h) lives here too, and is held to a
longdouble run of the same iteration on every matrix the GPU tests use: the enclosure
lo (1 - g) <= rho_ref <= hi (1 + g), g = (L + 2) 2^-53 with L the longest row -- each
y_i is a sum of at most L non-negative products (relative error <= L 2^-53), one more
rounding for the division, and the Collatz-Wielandt bounds are exact for exact ratios
while x > 0, which the model checks at every iteration.
"""
import ctypes
import functools

import numpy as np
import pytest

from speedy_ml_amd import _lib
from speedy_ml_amd.genres import generate_region

U = np.uint64
GOLDEN = U(0x9E3779B97F4A7C15)
SEED = 20241

# (n, k): the shapes of tests/test_genres_gpu.py -- small and edge n, one on each side of
# the LDS switch (2 n doubles against 160 KiB), the 16-bit column limit, the full-size
# atmosphere and slab reservoirs
GPU_SHAPES = [(n, 6 * n) for n in (1, 2, 7, 63, 64, 65, 1023, 1025, 10240, 10241, 65535)] + [(6160, 37945),
                                                                                           (4032, 24385)]


# ------------------------------------------------------------------ the recipe in NumPy
def _mix(z):
    z = z ^ (z >> U(30))
    z = z * U(0xBF58476D1CE4E5B9)
    z = z ^ (z >> U(27))
    z = z * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def _key(seed, region, stream):
    return _mix(_mix(np.array([seed], dtype=U) + GOLDEN) ^ U(8 * region + stream))


def _draw(key, index):
    return _mix(key + (np.asarray(index, dtype=U) + U(1)) * GOLDEN)


def _shuffle(n, count, key, first):
    d = _draw(key, first + np.arange(count))
    t = (((d >> U(32)) * (n - np.arange(count)).astype(U)) >> U(32)).astype(np.int64)
    choices = list(range(1, n + 1))
    out = np.empty(count, dtype=np.int32)
    for j in range(count):
        m = n - j
        tmp = choices[t[j]]
        out[j] = tmp
        choices[t[j]] = choices[m - 1]
        choices[m - 1] = tmp
    return out


def numpy_region(n, k, ninp, seed, region, sigma):
    rows, cols = np.empty(k, dtype=np.int32), np.empty(k, dtype=np.int32)
    for first in range(0, k, n):
        count = min(n, k - first)
        rows[first:first + count] = _shuffle(n, count, _key(seed, region, 0), first)
        cols[first:first + count] = _shuffle(n, count, _key(seed, region, 1), first)
    vals = ((_draw(_key(seed, region, 2), np.arange(k)) >> U(40)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    u = ((_draw(_key(seed, region, 3), np.arange(n)) >> U(40)).astype(np.float64) + 0.5) * 2.0 ** -24
    q = n // ninp
    return rows, cols, vals, (np.arange(n) // q).astype(np.int32), (sigma * (2.0 * u - 1.0)).astype(np.float32)


CPU_SHAPES = [(1, 6, 1), (7, 42, 7), (96, 576, 12), (6160, 37945, 1540), (1500, 2250, 3), (64, 40, 8)]


@pytest.mark.parametrize("n,k,ninp", CPU_SHAPES)
def test_generator_is_the_numpy_restatement(n, k, ninp):
    got = generate_region(n, k, ninp, SEED, 17, 0.5)
    want = numpy_region(n, k, ninp, SEED, 17, 0.5)
    for name, a, b in zip(("rows", "cols", "vals", "win_col", "win_val"), got, want):
        assert a.dtype == b.dtype, name
        np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                      b.view(np.uint32) if b.dtype == np.float32 else b, err_msg=name)


@pytest.mark.parametrize("n,k,ninp", CPU_SHAPES)
@pytest.mark.parametrize("sigma", [0.5, 0.6])
def test_structure(n, k, ninp, sigma):
    rows, cols, vals, wcol, wval = generate_region(n, k, ninp, SEED, 3, sigma)
    full, left = divmod(k, n)
    for a in (rows, cols):
        for b in range(full):
            np.testing.assert_array_equal(np.sort(a[b * n:(b + 1) * n]), np.arange(1, n + 1))
        tail = a[full * n:]
        assert tail.size == left and np.unique(tail).size == left
        assert left == 0 or (tail.min() >= 1 and tail.max() <= n)
    assert (vals >= 0).all() and (vals < 1).all()
    scaled = vals.astype(np.float64) * 2.0 ** 24
    np.testing.assert_array_equal(scaled, np.floor(scaled))
    assert (np.abs(wval.astype(np.float64)) <= sigma).all() and (wval != 0).all()
    np.testing.assert_array_equal(wcol, np.arange(n) // (n // ninp))


def test_keying():
    a = generate_region(96, 576, 12, SEED, 5, 0.5)
    b = generate_region(96, 576, 12, SEED, 5, 0.5)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    for other in (generate_region(96, 576, 12, SEED, 6, 0.5), generate_region(96, 576, 12, SEED + 1, 5, 0.5)):
        for j in (0, 1, 2, 4):  # rows, cols, vals, win_val (win_col is the fixed block structure)
            assert not np.array_equal(a[j], other[j])


@pytest.mark.parametrize("n,k,ninp", [(10, 20, 3), (0, 5, 1), (-4, 5, 1), (8, -1, 2), (65536, 10, 1)])
def test_argument_errors(n, k, ninp):
    L = _lib.lib()
    buf = np.zeros(16, dtype=np.int32)
    fbuf = np.zeros(16, dtype=np.float32)
    rc = L.sml_gen_region(n, k, ninp, ctypes.c_uint64(1), 0, 0.5, _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(fbuf),
                          _lib.ptr(buf), _lib.ptr(fbuf))
    assert rc == -1  # SML_ERR_ARG
    assert b"sml_gen_region" in L.sml_last_error()
    assert not buf.any() and not fbuf.any()


# ------------------------------------------------------------------ the iteration's model
def csr_slots(n, rows, cols, vals):
    """A's entries grouped by their position within their row, rows in entry order (the
    CSR copy's order: COO semantics, duplicates add): a list over slots of (row, col,
    val), each row at most once per slot.  Also the longest row L."""
    order = np.argsort(rows, kind="stable")
    r, c, v = rows[order].astype(np.int64) - 1, cols[order].astype(np.int64) - 1, np.asarray(vals)[order]
    counts = np.bincount(r, minlength=n)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    slot = np.arange(r.size) - start[r]
    L = int(counts.max()) if r.size else 0
    return [(r[slot == s], c[slot == s], v[slot == s]) for s in range(L)], L


def power_iteration(n, slots, tol, max_iter, dtype=np.float64):
    """sml_res_spectral_radius's iteration for one region in `dtype` arithmetic.
    Returns (lo, hi, iters, info, the smallest x entry met)."""
    x = np.ones(n, dtype=dtype)
    xmin = dtype(1)
    slots = [(r, c, v.astype(dtype)) for r, c, v in slots]
    if any(((v < 0) | ~np.isfinite(v)).any() for _, _, v in slots):
        return dtype(np.nan), dtype(np.nan), 0, 3, xmin
    t = 0
    while True:
        t += 1
        y = np.zeros(n, dtype=dtype)
        for r, c, v in slots:
            y[r] = y[r] + v * x[c]
        pos = x > 0
        q = y[pos] / x[pos]
        lo, hi, m = q.min(), q.max(), y.max()
        if m == 0:
            return dtype(0), dtype(0), t, 2, xmin
        if hi - lo <= dtype(tol) * hi:
            return lo, hi, t, 0, xmin
        if t == max_iter:
            return lo, hi, t, 1, xmin
        x = y / m
        xmin = min(xmin, x.min())


def gpu_matrix(j):
    """Matrix j of the GPU tests: (n, k, rows, cols, vals), raw draws with W_in unused."""
    n, k = GPU_SHAPES[j]
    rows, cols, vals, _, _ = generate_region(n, k, 1, SEED, j, 0.5)
    return n, k, rows, cols, vals


@functools.lru_cache(maxsize=None)
def reference_radius(j):
    """rho_ref of GPU matrix j: the longdouble iteration closed to a relative width of
    1e-18, its midpoint; also the longest row L."""
    assert np.finfo(np.longdouble).eps < 2e-19, "the reference needs an 80-bit long double"
    n, k, rows, cols, vals = gpu_matrix(j)
    slots, L = csr_slots(n, rows, cols, vals)
    lo, hi, iters, info, xmin = power_iteration(n, slots, 1e-18, 200, dtype=np.longdouble)
    assert info == 0 and xmin > 0, (GPU_SHAPES[j], info, iters)
    return (lo + hi) / 2, L


def check_enclosure(lo, hi, info, tol, rho_ref, L):
    """Gate 1 of the issue, in longdouble so that the bounds themselves do not round."""
    ld = np.longdouble
    g = ld(L + 2) * ld(2.0) ** -53
    assert info == 0
    assert ld(lo) * (1 - g) <= rho_ref <= ld(hi) * (1 + g), (lo, hi, rho_ref)
    assert hi - lo <= tol * hi


@pytest.mark.parametrize("j", range(len(GPU_SHAPES)))
def test_float64_model_encloses_the_longdouble_radius(j):
    n, k, rows, cols, vals = gpu_matrix(j)
    rho_ref, L = reference_radius(j)
    slots, _ = csr_slots(n, rows, cols, vals)
    for tol in (2e-14, 1e-10):
        lo, hi, iters, info, xmin = power_iteration(n, slots, tol, 1000)
        print(f"n {n} k {k} L {L} tol {tol:g}: iters {iters} lo {lo!r} hi {hi!r} rho_ref {rho_ref!r} xmin {xmin:.3e}")
        assert xmin > 0
        check_enclosure(lo, hi, info, tol, rho_ref, L)


def test_model_known_answers():
    s, _ = csr_slots(2, np.array([1, 2]), np.array([2, 1]), np.array([2.0, 1.0]))
    lo, hi, iters, info, _ = power_iteration(2, s, 2e-14, 50)
    assert (lo, hi, iters, info) == (1.0, 2.0, 50, 1)
    s, _ = csr_slots(3, np.array([1, 2]), np.array([2, 3]), np.array([0.0, 0.0]))
    assert power_iteration(3, s, 2e-14, 50)[:4] == (0.0, 0.0, 1, 2)
    s, _ = csr_slots(3, np.array([1, 2]), np.array([2, 3]), np.array([0.5, -0.5]))
    assert power_iteration(3, s, 2e-14, 50)[3] == 3
