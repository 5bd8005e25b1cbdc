"""np.longdouble references for the W_out training tests (x87 80-bit, eps 1.08e-19).

Gram / cross products.  Each element of G = S^T S (B = S^T T) is one fp64 FMA chain
over a batch's m products, added once to the running sum per batch, so against the
exact product of the same fp64 inputs

    |G - G_ref|_ij <= (m_total + batches + 1) 2^-53 (|S|^T |S|)_ij

and likewise for B with |S|^T |T|: m_total roundings of the chains, one per batch's
add, one for the reference's own rounding to spare.  Derived, not measured.

Solve.  The normwise backward error of a Cholesky solution, per output column o, with
the residual taken in longdouble on the regularised system built in longdouble:

    eta_o = ||G w_o - b_o||_inf / (||G||_inf ||w_o||_inf + ||b_o||_inf) <= n 2^-53

(n = naug; the first-order bound for Cholesky with substitution carries a small
multiple of n u; the cap is that order of magnitude, not a measurement)."""
import numpy as np

L = np.longdouble
U = L(2.0) ** -53


def cross(S, T):
    """B = S^T T in longdouble for S (m, naug), T (m, nout) fp64."""
    return np.asarray(S, dtype=L).T @ np.asarray(T, dtype=L)


def sums(S, T):
    """(G, B) = (S^T S, S^T T) in longdouble."""
    return cross(S, S), cross(S, T)


def products(S, T):
    """(G, B, |S|^T |S|, |S|^T |T|): the sums and the magnitudes their bound scales by."""
    return sums(S, T) + sums(np.abs(S), np.abs(T))


def gram_excess(got, ref, mag, m_total, batches):
    """max over the elements of |got - ref| / bound (<= 1 passes); exact zeros of the
    bound must be met exactly."""
    err = np.abs(np.asarray(got, dtype=L) - ref)
    bound = L(m_total + batches + 1) * U * mag
    if (err[bound == 0] != 0).any():
        return float("inf")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def regularised(G, B, ncs, beta_res, beta_model, using_prior, prior_val):
    """fit_chunk_hybrid's system on longdouble sums G (naug, naug), B (naug, nout)."""
    n, nout = B.shape
    bm, br = L(beta_model), L(beta_res)
    add = np.where(np.arange(n) < ncs, bm * bm if using_prior else bm, br * br if using_prior else br)
    Gr = G + np.diag(add)
    Br = B.copy()
    if using_prior:
        for i in range(min(ncs, nout)):
            Br[i, i] += L(prior_val) * bm * bm
    return Gr, Br


def eta(Gr, Br, W):
    """max over the output columns of the normwise backward error of W (naug, nout)."""
    w = np.asarray(W, dtype=L)
    res = np.abs(Gr @ w - Br).max(axis=0)
    den = np.abs(Gr).sum(axis=1).max() * np.abs(w).max(axis=0) + np.abs(Br).max(axis=0)
    return float((res / den).max())


def eta_cap(n):
    return float(L(n) * U)
