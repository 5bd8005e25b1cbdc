"""sml_res_set_target_index: training targets on a generic (slab-ocean shaped) context.
After the call sml_res_train_drive writes u_c[idx] per column through both drive forms
(k_res_drive, and k_drive_record under SML_RES_PATH_STEPWISE_DRIVE); the state columns and
the final state are bitwise those of the call without targets; before the call the
refusal stays."""
import numpy as np
import pytest

from speedy_ml_amd import SmlError

pytestmark = pytest.mark.gpu

REGIONS, NINP = [10, 500, 1100], [48, 40, 64]
NOUT = 4
PAD = 3


def _context(stepwise=False):
    """A slab-ocean shaped context (sml_res_create_generic), chunk_speedy = 0, n ~ 600."""
    from speedy_ml_amd.reservoir import Reservoirs

    n = [600 // p * p for p in NINP]
    res = Reservoirs(REGIONS, [0, 0, 0], n, [6 * v for v in n], chunk_speedy=0, nout=NOUT, ninp=NINP,
                     out_index=[35] * NOUT)
    for i, (r, p, nn) in enumerate(zip(REGIONS, NINP, n)):
        rng = np.random.default_rng([6, r])
        rows = np.concatenate([rng.permutation(nn) + 1 for _ in range(6)]).astype(np.int32)
        cols = np.concatenate([rng.permutation(nn) + 1 for _ in range(6)]).astype(np.int32)
        vals = (rng.random(6 * nn) * 0.3).astype(np.float32)
        win = np.zeros((p, nn), dtype=np.float32)
        q = nn // p
        for j in range(q):
            win[np.arange(p), np.arange(p) * q + j] = (0.5 * (2 * rng.random(p) - 1)).astype(np.float32)
        wout = ((rng.random((nn, NOUT)) * 2 - 1) * 0.01).astype(np.float32)
        res.load_region(i, rows, cols, vals, win, wout, np.zeros(36), np.ones(36))
    if stepwise:
        res.set_reference_paths(stepwise_drive=True)
    return res


def _reset(res):
    for i, n in enumerate(res.n):
        res.set_state(i, 0.1 * np.random.default_rng(i).random(int(n)))


def _index():
    """Positions spread over each region's feedback: the first, the last, two in between."""
    return np.array([[0, p - 1, p // 3, 2 * p // 3 + 1] for p in NINP], dtype=np.int32)


def _drive(res, inputs, m, cuda, targets):
    import torch

    d_in = torch.from_numpy(inputs[:m].copy()).to(cuda)
    d_s = torch.full((int(res.n.sum()) * m,), float("nan"), dtype=torch.float64, device=cuda)
    d_t = torch.full((res.nlocal * m * NOUT,), float("nan"), dtype=torch.float64, device=cuda) if targets else None
    res.train_drive(d_in, m, None, d_s, d_t, stride=inputs.shape[1])
    torch.cuda.synchronize()
    final = [res.get_state(i) for i in range(res.nlocal)]
    return d_s.cpu().numpy(), (d_t.cpu().numpy() if targets else None), final


@pytest.mark.parametrize("stepwise", [False, True])
@pytest.mark.parametrize("m", [1, 7])
def test_targets_are_the_indexed_inputs_and_change_nothing_else(cuda, stepwise, m):
    """m = 1 and m = 7 (a multiple of nothing), an input stride padded with NaN."""
    res = _context(stepwise)
    tot = int(res.fb_offsets[-1])
    rng = np.random.default_rng(31)
    inputs = np.full((m, tot + PAD), np.nan)
    inputs[:, :tot] = rng.standard_normal((m, tot))
    idx = _index()
    _reset(res)
    s0, _, x0 = _drive(res, inputs, m, cuda, targets=False)
    res.set_target_index(idx)
    _reset(res)
    s1, t1, x1 = _drive(res, inputs, m, cuda, targets=True)
    assert np.isfinite(s0).all() and s1.tobytes() == s0.tobytes()
    for a, b in zip(x0, x1):
        assert a.tobytes() == b.tobytes()
    o = res.fb_offsets
    for i in range(res.nlocal):
        T = t1[i * m * NOUT:(i + 1) * m * NOUT].reshape(m, NOUT)
        for c in range(m):
            assert T[c].tobytes() == inputs[c, o[i] + idx[i]].tobytes(), (i, c)
    # without targets the call still works on the context that has an index
    _reset(res)
    s2, _, x2 = _drive(res, inputs, m, cuda, targets=False)
    assert s2.tobytes() == s0.tobytes()
    res.close()


def test_a_generic_context_without_the_call_still_refuses_targets(cuda):
    import torch

    res = _context()
    tot = int(res.fb_offsets[-1])
    z = lambda k: torch.zeros(k, dtype=torch.float64, device=cuda)  # noqa: E731
    with pytest.raises(SmlError, match=r"a generic \(slab\) context has no target geometry: d_targets must be NULL"):
        res.train_drive(z(2 * tot), 2, None, z(2 * int(res.n.sum())), z(2 * res.nlocal * NOUT))
    res.close()


def test_refusals_leave_the_context_usable(cuda):
    import torch

    from speedy_ml_amd._lib import lib, ptr
    from speedy_ml_amd.reservoir import Reservoirs
    from speedy_ml_amd.synthetic import region_weights

    L = lib()
    # a context with a geometry keeps its own table
    w = region_weights(5, True, n_override=64)
    geo = Reservoirs([w.region], [w.sst], [w.n], [w.k])
    assert L.sml_res_set_target_index(geo.handle, ptr(np.zeros(136, dtype=np.int32))) == -1
    assert b"stays the only one" in L.sml_last_error()
    geo.close()
    res = _context()
    idx = _index()
    assert L.sml_res_set_target_index(res.handle, None) == -1 and b"idx is null" in L.sml_last_error()
    for bad, at in ((-1, (0, 0)), (NINP[1], (1, 3)), (NINP[2] + 100, (2, 1))):
        wrong = idx.copy()
        wrong[at] = bad
        assert L.sml_res_set_target_index(res.handle, ptr(wrong)) == -1
        assert b"outside [0," in L.sml_last_error(), L.sml_last_error()
    # nothing was adopted: targets are still refused, then accepted with a good index
    tot, m = int(res.fb_offsets[-1]), 2
    inputs = np.random.default_rng(2).standard_normal((m, tot))
    _reset(res)
    with pytest.raises(SmlError, match="no target geometry"):
        _drive(res, inputs, m, cuda, targets=True)
    res.set_target_index(idx)
    # a rejected index after a good one leaves the good one in place
    wrong = idx.copy()
    wrong[0, 0] = NINP[0]
    assert L.sml_res_set_target_index(res.handle, ptr(wrong)) == -1
    _reset(res)
    _, t, _ = _drive(res, inputs, m, cuda, targets=True)
    o = res.fb_offsets
    for i in range(res.nlocal):
        assert t[i * m * NOUT:(i + 1) * m * NOUT].reshape(m, NOUT).tobytes() == inputs[:, o[i] + idx[i]].tobytes()
    # with members, and inside a begun step
    res.set_members(2)
    assert L.sml_res_set_target_index(res.handle, ptr(idx)) == -1 and b"members" in L.sml_last_error()
    res.set_members(1)
    fb = torch.zeros(tot, dtype=torch.float64, device=cuda)
    res.predict_begin(fb)
    assert L.sml_res_set_target_index(res.handle, ptr(idx)) != 0 and b"begun" in L.sml_last_error()
    res.cancel_step()
    assert L.sml_res_set_target_index(res.handle, ptr(idx)) == 0
    res.close()
