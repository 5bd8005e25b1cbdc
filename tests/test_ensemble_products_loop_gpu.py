"""Ensemble products inside the E-member hybrid loop (EnsembleLoop.set_products): the loop with
products on computes, in every buffer and after every step, exactly what it computes with
products off; what it reports is what EnsembleProducts gives when called directly on the
step's assembled grids; a step past the capacity refuses before anything is enqueued.

E = 3, all 1152 regions at n 96, three steps, built as tests/test_ensemble_loop_gpu.py builds
its ensemble; one more case with the slab ocean and the calendar on, as
tests/test_ensemble_slab_gpu.py sets them up, for two steps.  No tolerance anywhere."""
import numpy as np
import pytest

import test_ensemble_loop_gpu as plain
import test_ensemble_slab_gpu as slabbed

pytestmark = pytest.mark.gpu

E, STEPS = 3, 3
KEYS = ("ov", "g4", "g2", "pr", "fb", "f4", "f2", "lm")


def _truth(cuda, steps):
    import torch

    from speedy_ml_amd.synthetic import synthetic_grids

    gs = [synthetic_grids(70 + s) for s in range(steps)]
    return tuple(torch.from_numpy(np.ascontiguousarray(np.stack([g[i] for g in gs]))).to(cuda) for i in range(3))


def _snapshot(ens):
    return {k: getattr(ens, k).cpu().numpy().copy() for k in KEYS}


def _direct(ens, direct, truth, s):
    """EnsembleProducts called on the loop's grids after step s: (moments, score row, rank row)."""
    import torch

    mom = direct.moments(ens.g4, ens.g2, ens.pr)
    direct.scores(ens.g4, ens.g2, ens.pr, None if truth is None else tuple(a[s] for a in truth), s)
    torch.cuda.synchronize()
    return [m.cpu().numpy() for m in mom]


def _compare_products(ens, direct, truth, s):
    want = _direct(ens, direct, truth, s)
    got = [getattr(ens, k).cpu().numpy() for k in ("mean4", "mean2", "meanpr", "spread4", "spread2", "spreadpr")]
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.tobytes() == b.tobytes(), (s, k)
        assert np.isfinite(a).all()
    sc, rk = ens.products()
    dsc, drk = direct.read(0, s + 1)
    assert sc.shape == (s + 1, 34, 4) and sc.tobytes() == dsc.tobytes(), s
    np.testing.assert_array_equal(rk, drk)
    if truth is not None:
        assert np.isfinite(sc).all() and (rk.sum(2) == 4608).all() and (rk[:, :, E + 1:] == 0).all()


def test_products_in_the_loop(cuda):
    """Three steps with set_products(3, truth) against the same loop without products: ov, g4,
    g2, pr, fb, f4, f2 and lm are bit for bit the same after every step; mean, spread and the
    score rows are EnsembleProducts' on the step's g4, g2, pr; a fourth step refuses with the
    loop untouched, and goes through after a larger capacity (no truth: only the spread is
    scored) and after set_products(None)."""
    import torch

    from speedy_ml_amd import domain
    from speedy_ml_amd.ensemble import EnsembleLoop, EnsembleProducts
    from speedy_ml_amd.synthetic import initial_state, region_weights

    mask = domain.load_sst_mask()
    ws = [region_weights(r, bool(mask[r]), n_override=96, seed=5, climatology=True) for r in range(1152)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    tisr = t(np.random.default_rng(13).standard_normal((1152, 16)))
    x0 = [initial_state(w.region, w.n) for w in ws]
    truth = _truth(cuda, STEPS)
    res = plain._context(ws, mask)
    res.set_members(E)
    snaps = {}
    for on in (False, True):
        for e in range(E):
            for i in range(1152):
                res.set_state(i, x0[i], member=e)
        dyns = [plain._dynamics() for _ in range(E)]
        ens = EnsembleLoop(res, dyns, cuda, tisr=tisr)
        direct = EnsembleProducts(E, STEPS + 1, cuda)
        if on:
            with pytest.raises(ValueError, match="truth"):
                ens.set_products(STEPS + 1, truth)  # fewer truth steps than rows
            ens.set_products(STEPS, truth)
        else:
            with pytest.raises(RuntimeError, match="no products"):
                ens.products()
        for e in range(E):
            ens.start(e, *(t(a) for a in plain._start_grids(e)))
        snaps[on] = []
        for s in range(STEPS):
            ens.step()
            ens.sync()
            torch.cuda.synchronize()
            assert ens.run_speedy() == [True] * E
            snaps[on].append(_snapshot(ens))
            if on:
                _compare_products(ens, direct, truth, s)
        if on:
            for s in range(STEPS):
                for k in KEYS:
                    np.testing.assert_array_equal(snaps[True][s][k], snaps[False][s][k], err_msg=f"step {s} {k}")
            before = _snapshot(ens)
            with pytest.raises(RuntimeError, match="3 rows are full"):
                ens.step()
            ens.sync()
            assert ens.t == STEPS and res.step_begun()
            after = _snapshot(ens)
            for k in KEYS:
                np.testing.assert_array_equal(after[k], before[k])
            ens.set_products(2, None)  # a new table: its rows start again, nothing to verify against
            ens.step()
            ens.sync()
            sc, rk = ens.products()
            assert sc.shape == (1, 34, 4) and np.isfinite(sc[0, :, 1]).all() and (sc[0, :, 1] > 0).all()
            assert np.isnan(sc[0][:, [0, 2, 3]]).all() and (rk == 0).all()
            ens.set_products(None)
            assert ens.mean4 is None
            ens.step()
            ens.step()
            ens.sync()
            assert ens.t == STEPS + 3 and ens.run_speedy() == [True] * E
        direct.close()
        ens.cancel_step()
        ens.close()
        for d in dyns:
            d.close()
        torch.cuda.synchronize()
    res.close()


def test_products_in_the_loop_with_slab_and_calendar(cuda):
    """Two steps with the slab ocean and run_model's calendar on: every loop buffer and every
    member's slab state is bit for bit that of the same loop without products, and the
    products are EnsembleProducts' on the step's grids."""
    import torch

    from speedy_ml_amd.ensemble import EnsembleLoop, EnsembleProducts

    w = slabbed.World(cuda)
    truth = _truth(cuda, 2)
    snaps = {}
    for on in (False, True):
        for e in range(E):
            w.set_states(w.res, w.slab, e, member=e)
        dyns = [w.dynamics() for _ in range(E)]
        ens = EnsembleLoop(w.res, dyns, cuda, tisr=w.tisr, nleap=2, slab=w.ocean(w.slab))
        ens.set_calendar(slabbed.CAL[0], slabbed.CAL[1], 6)
        direct = EnsembleProducts(E, 2, cuda)
        if on:
            ens.set_products(2, truth)
        for e in range(E):
            ens.start(e, *w.grids(e))
            ens.start_slab(e, w.slab_start(e))
        snaps[on] = []
        for s in range(2):
            ens.step()
            ens.sync()
            torch.cuda.synchronize()
            assert ens.run_speedy() == [True] * E
            snap = _snapshot(ens)
            for e in range(E):
                snap.update({f"{k}{e}": v for k, v in ens.slab_state(e).items() if k != "feedback"})
            snaps[on].append(snap)
            if on:
                _compare_products(ens, direct, truth, s)
        direct.close()
        ens.cancel_step()
        ens.close()
        for d in dyns:
            d.close()
        torch.cuda.synchronize()
    for s in range(2):
        assert set(snaps[True][s]) == set(snaps[False][s])
        for k in snaps[True][s]:
            np.testing.assert_array_equal(snaps[True][s][k], snaps[False][s][k], err_msg=f"step {s} {k}")
    w.close()
