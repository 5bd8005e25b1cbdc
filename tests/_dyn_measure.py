"""The per-wavenumber error measure of the dynamics-step edge tests
(test_oracle_dynamics_edges.py, test_dynamics_edges_gpu.py) on spectral arrays
(..., nx = 32, mx = 31), complex, index (n, m), triangle m + n <= 30.

For one level (the last two axes) and one zonal wavenumber m:

    err(m) = max over n <= 30 - m of |got - ref|
             / max( max over n <= 30 - m of |ref| ,  FLOOR x max over the whole level of |ref| )

so a coefficient is held to its own row, not to the level's mean: the suite's
max |err| / max |field| lets a relative error of 1e-9 at the truncation edge through
wherever a large (0,0) mean sits in the same array.  The floor is a condition, not a
tolerance: it keeps a row that cancels by chance (m = 30 is a single coefficient) from
asking more than an fp64 sum can give.  make_dyn_edges_golden.py asserts it active on
no row of any state output of the reference.

Outside the triangle (and the imaginary parts of m = 0) nothing is relative:
check_zeros() wants exact zeros where both the reference and the oracle have them, and
|got| <= tol x the level's maximum elsewhere outside the triangle."""
import numpy as np

NX, MX = 32, 31
FLOOR = 1e-3
TRI = (np.arange(NX)[:, None] + np.arange(MX)[None, :]) <= 30  # (n, m)


def per_m(got, ref):
    """(err, active): err (..., mx) as above, active (..., mx) = the floor set the denominator."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and ref.shape[-2:] == (NX, MX), (got.shape, ref.shape)
    num = (np.abs(got - ref) * TRI).max(axis=-2)
    a = np.abs(ref)
    row = (a * TRI).max(axis=-2)
    floor = FLOOR * a.max(axis=(-2, -1))[..., None]
    return num / np.maximum(np.maximum(row, floor), 1e-300), row < floor


def worst(got, ref):
    """max of err over every level and m."""
    return float(per_m(got, ref)[0].max())


def global_rel(got, ref):
    """The suite's present measure (test_dynamics_gpu.py's _rel), for comparison."""
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)


def parts(a):
    """complex (...) -> float64 (..., 2) real and imaginary parts (a copy)."""
    a = np.ascontiguousarray(a, dtype=np.complex128)
    return a.view(np.float64).reshape(a.shape + (2,)).copy()


def check_zeros(got, ref, ref_zero, orc, tol):
    """Exact zeros where the reference (its stored mask ref_zero, bool (..., 2)) and the
    oracle (the array orc) are both exactly zero; elsewhere outside the triangle
    |got| <= tol x the level's max |ref|.  Returns the number of exact zeros checked."""
    g = parts(got)
    both = ref_zero & (parts(orc) == 0.0)
    assert both[..., ~TRI, :].all(), "reference and oracle are both zero outside the triangle"
    bad = np.argwhere(both & (g != 0.0))
    assert bad.size == 0, f"{len(bad)} values not exactly zero, first at {bad[0].tolist()}: {g[tuple(bad[0])]!r}"
    lev = np.abs(ref).max(axis=(-2, -1))[..., None]
    out = (np.abs(got) * ~TRI).max(axis=-2)
    assert (out <= tol * lev).all(), (out / lev).max()
    return int(both.sum())
