"""Oracle W_out training (chunking_matmul + fit_chunk_hybrid + mldivide).

mldivide calls LAPACK dgesv, which the reference does not vendor; the oracle
restates dgesv's published algorithm (LU with partial pivoting) and is checked
here against numpy.linalg.solve (LAPACK gesv).  No reference test or fixture
covers training: parity unpinned beyond the cited call sites."""
import numpy as np
import pytest

import oracle


def _data(naug, nout, m, seed=0):
    rng = np.random.default_rng(seed)
    S = np.tanh(rng.standard_normal((m, naug)))  # C (m, naug) == Fortran augmented_states(naug, m)
    S[:, :32] = rng.standard_normal((m, 32))      # "imperfect model" rows
    T = rng.standard_normal((m, nout))
    return S, T


def test_accumulate_matches_numpy_and_batches_add():
    S, T = _data(90, 20, 70)
    G = np.zeros((90, 90))
    B = np.zeros((90, 20))
    oracle.train_accumulate(S[:40], T[:40], G, B)
    oracle.train_accumulate(S[40:], T[40:], G, B)
    np.testing.assert_allclose(G, S.T @ S, rtol=1e-13, atol=1e-12)
    np.testing.assert_allclose(B, S.T @ T, rtol=1e-13, atol=1e-12)


@pytest.mark.parametrize("using_prior,prior_val", [(False, 0.0), (True, 0.0), (True, 0.3)])
def test_solve_matches_lapack(using_prior, prior_val):
    naug, nout, ncs = 120, 24, 32
    S, T = _data(naug, nout, 400, seed=1)
    G = S.T @ S
    B = S.T @ T
    bm, br = 1.0, 0.05
    w, info = oracle.train_solve(G, B, ncs, br, bm, using_prior, prior_val)
    assert info == 0
    add = np.where(np.arange(naug) < ncs, bm ** 2 if using_prior else bm, br ** 2 if using_prior else br)
    Greg = G + np.diag(add)
    rhs = B.copy()
    if using_prior:
        for i in range(min(ncs, nout)):
            rhs[i, i] += prior_val * bm ** 2
    ref = np.linalg.solve(Greg.T, rhs)
    np.testing.assert_allclose(w, ref, rtol=0, atol=1e-10 * np.abs(ref).max())


# ---- the oracle on the GPU edge tests' ground, against np.longdouble (tests/_train_ref.py)
def _edge_data(naug, nout, m, seed):
    """tests/test_training_gpu.py's _data for one region."""
    rng = np.random.default_rng(seed)
    S = np.tanh(rng.standard_normal((m, naug)))
    S[:, :132] = rng.standard_normal((m, min(132, naug)))
    return S, rng.standard_normal((m, nout))


@pytest.mark.parametrize("nout", [2, 49, 136, 144])
@pytest.mark.parametrize("naug", [2, 129, 257])
def test_accumulate_within_the_elementwise_bound(naug, nout):
    """Batches of 16, 1 and 17 steps into the same sums: every element of G and B within
    (m_total + batches + 1) 2^-53 (|S|^T |S|)_ij of the longdouble product."""
    import _train_ref as ref

    batches = (16, 1, 17)
    S, T = _edge_data(naug, nout, sum(batches), seed=31)
    G = np.zeros((naug, naug))
    B = np.zeros((naug, nout))
    t0 = 0
    for b in batches:
        oracle.train_accumulate(S[t0:t0 + b], T[t0:t0 + b], G, B)
        t0 += b
    Gl, Bl, Ga, Ba = ref.products(S, T)
    eg = ref.gram_excess(G, Gl, Ga, sum(batches), len(batches))
    eb = ref.gram_excess(B, Bl, Ba, sum(batches), len(batches))
    print(f"naug {naug} nout {nout}: G at {eg:.3f}, B at {eb:.3f} of the bound")
    assert eg <= 1.0 and eb <= 1.0


@pytest.mark.parametrize("ncs,using_prior,beta_res,beta_model,prior_val",
                         [(100, True, 0.3, 1.0, 0.5), (0, False, 0.5, 1.0, 0.0), (128, True, 0.3, 1.0, 0.25)])
@pytest.mark.parametrize("naug", [129, 384])
def test_solve_backward_error_under_the_cap(naug, ncs, using_prior, beta_res, beta_model, prior_val):
    """The LU restatement's normwise backward error on the longdouble system <= n 2^-53."""
    import _train_ref as ref

    nout, m = 136, 200
    S, T = _edge_data(naug, nout, m, seed=33)
    G = np.zeros((naug, naug))
    B = np.zeros((naug, nout))
    oracle.train_accumulate(S, T, G, B)
    w, info = oracle.train_solve(G, B, ncs, beta_res, beta_model, using_prior, prior_val)
    assert info == 0
    Gl, Bl = ref.sums(S, T)
    e = ref.eta(*ref.regularised(Gl, Bl, ncs, beta_res, beta_model, using_prior, prior_val), w)
    print(f"naug {naug} ncs {ncs}: eta {e:.3e} (cap {ref.eta_cap(naug):.3e})")
    assert e <= ref.eta_cap(naug)
