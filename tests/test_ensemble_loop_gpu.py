"""An E-member hybrid forecast (speedy_ml_amd.ensemble.EnsembleLoop: begin_members beside E
SPEEDY windows, finish_assemble_members behind them) against E single-member hybrid loops.

E = 3, all 1152 regions at n 96, three steps; states, fixed tisr and forcing as
tests/test_hybrid_gpu.py::_loop builds them, the weights built once and shared, every member
started from synthetic grids of its own.  The reference of member e is a one-stream
HybridLoop(overlap=False) of its own -- the one-pass readout, the assembly, run_model and the
re-tiling issued one after the other -- and every buffer of the ensemble loop is compared bit
for bit with it."""
import numpy as np
import pytest

from speedy_ml_amd import domain
from speedy_ml_amd.synthetic import initial_state, region_weights

pytestmark = pytest.mark.gpu

E, STEPS = 3, 3
KEYS = ("ov", "g4", "g2", "pr", "fb", "f4", "f2", "lm")
PROBE = (0, 500, 1151)


def _dynamics():
    from speedy_ml_amd.dynamics import Dynamics
    from speedy_ml_amd.synthetic import dyn_state, phys_boundary

    st0, forcing = dyn_state()
    dyn = Dynamics()
    dyn.set_forcing(**forcing)
    dyn.set_state(st0)
    dyn.set_physics(phys_boundary(dyn, forcing["phis"]))
    return dyn


def _context(ws, mask):
    from speedy_ml_amd.reservoir import Reservoirs

    res = Reservoirs(list(range(1152)), mask, [w.n for w in ws], [w.k for w in ws])
    for i, w in enumerate(ws):
        res.load_region_weights(i, w)
    return res


def _start_grids(e):
    from speedy_ml_amd.synthetic import synthetic_grids

    g4, g2, pr = synthetic_grids(11 + 10 * e)
    f4, f2, _ = synthetic_grids(12 + 10 * e)
    return g4, g2, pr, f4, f2


def test_ensemble_loop_is_bitwise_the_single_member_loops(cuda):
    """After every step member e's ov, g4, g2, pr, fb, f4 and f2 are those of a serial
    HybridLoop of its own after the same step; its lm (written by the next finish) after step
    t + 1 is that loop's after step t; after cancel_step the states are that loop's; every
    run_speedy flag is True and the last forecast is finite and nonzero."""
    import torch

    from speedy_ml_amd.ensemble import EnsembleLoop
    from speedy_ml_amd.exchange import OutvecExchange
    from speedy_ml_amd.hybrid import HybridLoop

    mask = domain.load_sst_mask()
    ws = [region_weights(r, bool(mask[r]), n_override=96, seed=5, climatology=True) for r in range(1152)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    tisr = t(np.random.default_rng(13).standard_normal((1152, 16)))
    x0 = [initial_state(w.region, w.n) for w in ws]

    # --- the references: one serial loop per member, one after the other on one context
    single = _context(ws, mask)
    ref, ref_x = [], []
    for e in range(E):
        for i in range(1152):
            single.set_state(i, x0[i])
        dyn = _dynamics()
        loop = HybridLoop(single, dyn, OutvecExchange(1152, 1, 0, device=cuda), cuda, tisr=tisr, overlap=False)
        loop.start(*(t(a) for a in _start_grids(e)))
        loop.sync()
        snaps = []
        for _ in range(STEPS):
            loop.step()
            loop.sync()
            torch.cuda.synchronize()
            assert loop.run_speedy()
            snaps.append({k: getattr(loop, k).cpu().numpy().copy() for k in KEYS})
        ref.append(snaps)
        ref_x.append([single.get_state(i) for i in PROBE])
        loop.close()
        dyn.close()
        torch.cuda.synchronize()
    single.close()

    # --- the ensemble
    res = _context(ws, mask)
    res.set_members(E)
    for e in range(E):
        for i in range(1152):
            res.set_state(i, x0[i], member=e)
    dyns = [_dynamics() for _ in range(E)]
    ens = EnsembleLoop(res, dyns, cuda, tisr=tisr)
    assert ens.run_speedy() == [True] * E
    for e in range(E):
        assert not res.step_begun()
        ens.start(e, *(t(a) for a in _start_grids(e)))
    assert res.step_begun()
    for s in range(STEPS):
        ens.step()
        ens.sync()
        torch.cuda.synchronize()
        assert ens.run_speedy() == [True] * E, f"step {s}: {ens.run_speedy()}"
        got = {k: getattr(ens, k).cpu().numpy() for k in KEYS}
        for e in range(E):
            for k in KEYS[:-1]:
                np.testing.assert_array_equal(got[k][e], ref[e][s][k], err_msg=f"step {s} member {e} {k}")
            if s >= 1:
                np.testing.assert_array_equal(got["lm"][e], ref[e][s - 1]["lm"], err_msg=f"step {s} member {e} lm")
    # the states run one update ahead; rolled back they are the serial loops'
    assert res.step_begun()
    ens.cancel_step()
    assert not res.step_begun()
    for e in range(E):
        for j, i in enumerate(PROBE):
            np.testing.assert_array_equal(res.get_state(i, member=e), ref_x[e][j], err_msg=f"member {e} region {i}")
    last = got["f4"]
    assert np.isfinite(last).all() and np.isfinite(got["f2"]).all() and np.isfinite(got["ov"]).all()
    assert all(np.abs(last[e]).max() > 0 for e in range(E))
    # the members' forecasts differ (each started from its own grids)
    assert not np.array_equal(last[0], last[1]) and not np.array_equal(last[1], last[2])
    ens.close()
    for d in dyns:
        d.close()
    res.close()
    torch.cuda.synchronize()
