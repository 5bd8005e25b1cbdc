"""The reservoir forward (sml_reservoir.hip) outside the shape box of
test_reservoir_gpu.py: leakage != 1 through every update form, odd and tiny n, n at
the 1024-row pass, at the balanced update's 7168 bound, past the LDS-staged update
(n + ninp > 8192) and at the 16-bit column limit, chunk_speedy not a multiple of 4,
nout not a multiple of 8 (and padded wide rows, nout_pad 144), ninp > 1024 and > n,
W_in with a stored column, the paced readout and a padded outvec stride; and the
context itself: eight create / use / destroy rounds through every lazy allocation, the
reported update and begin forms against the reference paths, refused creates.

Reference: the oracle's predict (oracle.predict / predict_f32 with leakage= and
chunk_speedy=), pinned at these shapes against a longdouble restatement by
tests/test_oracle_reservoir.py.  Tolerances are the project's (test_reservoir_gpu.py):
  state x : |err| <= 1e-14 (t + 1) (1 + |x|) after t + 1 chained steps
  outvec  : |err| <= 1e-11 (1 + |outvec|)
Bitwise assertions between the library's own forms come on top of the oracle
comparison.  Where the library reports the form it takes (update_balanced, begin_fused,
ell_layout) the test asserts it, so a dispatch change cannot move a case off its path.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
from speedy_ml_amd import SmlError
from speedy_ml_amd.synthetic import initial_state, region_weights, synthetic_grids

pytestmark = pytest.mark.gpu

X_TOL = 1e-14
OUT_TOL = 1e-11

CASES = [(0, False), (5, True), (23, True), (24, False), (600, True), (1127, False), (1151, True)]
WORST = {"x": 0.0, "out": 0.0}  # the largest scaled errors against the oracle seen so far (printed)


# ----------------------------------------------------------------------------- weights
@functools.lru_cache(maxsize=None)
def _weights(n, ninp, ncs, nout, seed=0, win="random"):
    """One reservoir of any shape.  A: 6 n + n // 3 entries from per-block permutations,
    so rows hold 6 or 7 entries (a 6-slot ELL with an overflow list; one width where
    n < 3).  W_in: one entry per row, in a random column or block-diagonal (row i reads
    input i // (n / ninp))."""
    rng = np.random.default_rng([seed, n, ninp, ncs, nout])
    blocks = [n] * 6 + [n // 3]
    rows = np.concatenate([rng.permutation(n)[:b] + 1 for b in blocks]).astype(np.int32)
    cols = np.concatenate([rng.permutation(n)[:b] + 1 for b in blocks]).astype(np.int32)
    vals = (0.3 * rng.random(len(rows))).astype(np.float32)
    if win == "block":
        assert n % ninp == 0
        wcol = (np.arange(n) // (n // ninp)).astype(np.int32)
    else:
        wcol = rng.integers(0, ninp, n).astype(np.int32)
    wval = (rng.random(n) - 0.5).astype(np.float32)
    wval[wval == 0] = 0.25
    dense = np.zeros((ninp, n), dtype=np.float32)
    dense[wcol, np.arange(n)] = wval
    wout = (0.01 * (2.0 * rng.random((ncs + n, nout)) - 1.0)).astype(np.float32)
    mean = rng.standard_normal(36)
    std = 0.5 + rng.random(36)
    w = SimpleNamespace(n=n, ninp=ninp, k=len(rows), rows=rows, cols=cols, vals=vals, win=dense, wcol=wcol,
                        wval=wval, wout=wout, mean=mean, std=std, x0=rng.random(n) - 0.5, region=0, sst=0)
    for a in (rows, cols, vals, dense, wcol, wval, wout, mean, std, w.x0):
        a.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _region_weights(cases, n_override):
    """T30 regions (synthetic.region_weights) in the same record."""
    out = []
    for region, sst in cases:
        r = region_weights(region, sst, n_override=n_override)
        wcol, wval = r.win_compressed()
        out.append(SimpleNamespace(n=r.n, ninp=r.ninp, k=r.k, rows=r.rows, cols=r.cols, vals=r.vals, win=r.win,
                                   wcol=wcol, wval=wval, wout=r.wout, mean=r.mean, std=r.std,
                                   x0=initial_state(region, r.n), region=region, sst=sst))
    return out


def _load(res, ws, wdt="f32"):
    for i, w in enumerate(ws):
        if wdt == "f64":
            res.load_region(i, w.rows, w.cols, w.vals.astype(np.float64), w.win.astype(np.float64),
                            w.wout.astype(np.float64), w.mean, w.std)
        else:
            res.load_region(i, w.rows, w.cols, w.vals, w.win, w.wout, w.mean, w.std)
        res.set_state(i, w.x0)
    return res


def _generic(ws, ncs, nout, leak, wdt="f32", out_index=None, **paths):
    from speedy_ml_amd.reservoir import Reservoirs

    res = Reservoirs(list(range(len(ws))), [0] * len(ws), [w.n for w in ws], [w.k for w in ws], chunk_speedy=ncs,
                     nout=nout, weight_dtype=wdt, leakage=leak, ninp=[w.ninp for w in ws],
                     out_index=[-1] * nout if out_index is None else out_index)
    if paths:
        res.set_reference_paths(**paths)
    return _load(res, ws, wdt)


def _regular(ws, leak, wdt="f32", **paths):
    from speedy_ml_amd.reservoir import Reservoirs

    res = Reservoirs([w.region for w in ws], [w.sst for w in ws], [w.n for w in ws], [w.k for w in ws],
                     weight_dtype=wdt, leakage=leak)
    if paths:
        res.set_reference_paths(**paths)
    return _load(res, ws, wdt)


def _series(ws, ncs, steps, seed=5):
    rng = np.random.default_rng(seed)
    fbs = rng.standard_normal((steps, sum(w.ninp for w in ws)))
    lms = rng.standard_normal((steps, len(ws), max(ncs, 1)))
    return fbs, lms


# --------------------------------------------------------------------------- reference
def _oracle_chain(ws, fbs, lms, ncs, leak, unstandardize=False):
    """seq[t] = (outvecs [nlocal][nout], states) after t + 1 chained oracle steps."""
    offs = np.concatenate([[0], np.cumsum([w.ninp for w in ws])])
    xs = [w.x0 for w in ws]
    seq = []
    for t in range(len(fbs)):
        outs = []
        for i, w in enumerate(ws):
            out, xs[i] = oracle.predict_f32(w.rows, w.cols, w.vals, w.wcol, w.wval, w.wout, fbs[t, offs[i]:offs[i + 1]],
                                            lms[t, i] if ncs else None, xs[i], w.mean, w.std, chunk_speedy=ncs,
                                            leakage=leak, unstandardize=unstandardize)
            outs.append(out)
        seq.append((np.stack(outs), list(xs)))
    return seq


def _scaled(a, b):
    return float((np.abs(np.asarray(a) - np.asarray(b)) / (1.0 + np.abs(np.asarray(b)))).max())


def _near(seq, ref, what):
    """Every step of seq within the project's tolerances of the oracle's chain."""
    for t, ((ov, xs), (rov, rxs)) in enumerate(zip(seq, ref)):
        if ov is not None:
            e = _scaled(ov, rov)
            WORST["out"] = max(WORST["out"], e)
            assert e <= OUT_TOL, f"{what} step {t}: outvec scaled err {e:.3e} > {OUT_TOL:.0e}"
        for i, (x, rx) in enumerate(zip(xs, rxs)):
            e = _scaled(x, rx)
            WORST["x"] = max(WORST["x"], e)
            assert e <= X_TOL * (t + 1), f"{what} step {t} region {i}: state scaled err {e:.3e}"
    print(f"{what}: within tolerance; worst so far x {WORST['x']:.2e} outvec {WORST['out']:.2e}")


def _same(seq, base, what, outvecs=True):
    for t, ((ov, xs), (bov, bxs)) in enumerate(zip(seq, base)):
        if outvecs:
            np.testing.assert_array_equal(ov, bov, err_msg=f"{what} step {t} outvecs")
        for i, (x, bx) in enumerate(zip(xs, bxs)):
            np.testing.assert_array_equal(x, bx, err_msg=f"{what} step {t} region {i} state")


# ------------------------------------------------------------------------------- forms
def _states(res):
    return [res.get_state(i) for i in range(res.nlocal)]


def _run(res, fbs, lms, cuda, split=False, ld=None):
    """Chained steps (sml_res_step, or begin + finish): seq[t] = (outvecs, states).  The
    outvec buffer starts as NaN; with ld the rows are ld wide."""
    import torch

    ov = torch.full((res.nlocal, ld or res.nout), float("nan"), dtype=torch.float64, device=cuda)
    seq = []
    for t in range(len(fbs)):
        dfb = torch.from_numpy(fbs[t].copy()).to(cuda)
        dlm = torch.from_numpy(lms[t, :, :res.ncs].copy()).to(cuda) if res.ncs else None
        if split:
            res.predict_begin(dfb)
            res.predict_finish(dlm, ov)
        else:
            res.predict(dfb, dlm, ov)
        torch.cuda.synchronize()
        seq.append((ov.cpu().numpy().copy(), _states(res)))
    return seq


def _squared(x):
    xt = x.copy()
    xt[1::2] = x[1::2] * x[1::2]
    return xt


def _drive(res, fbs, lms, cuda, targets):
    """train_drive over the blocks of fbs: per region the state block (m, ncs + n), the
    target block (m, nout) or None; buffers start as NaN."""
    import torch

    m = len(fbs)
    naug = [res.ncs + int(n) for n in res.n]
    d_in = torch.from_numpy(fbs.copy()).to(cuda)
    d_mo = torch.from_numpy(np.ascontiguousarray(lms[:, :, :res.ncs]).reshape(m, -1)).to(cuda) if res.ncs else None
    d_s = torch.full((sum(naug) * m,), float("nan"), dtype=torch.float64, device=cuda)
    d_t = torch.full((res.nlocal * m * res.nout,), float("nan"), dtype=torch.float64, device=cuda) if targets else None
    res.train_drive(d_in, m, d_mo, d_s, d_t)
    torch.cuda.synchronize()
    s = d_s.cpu().numpy()
    S, T, off = [], [], 0
    for i, na in enumerate(naug):
        S.append(s[off:off + na * m].reshape(m, na))
        off += na * m
        if targets:
            T.append(d_t.cpu().numpy()[i * m * res.nout:(i + 1) * m * res.nout].reshape(m, res.nout))
    return S, T


def _check_drive(res, ws, fbs, lms, cuda, base, ref, what, targets=False):
    """The drive's columns and final state: bitwise the step forms' states (base), and
    within the state tolerance of the oracle's (ref)."""
    S, T = _drive(res, fbs, lms, cuda, targets)
    m, ncs = len(fbs), res.ncs
    o = res.fb_offsets
    for i, w in enumerate(ws):
        for c in range(m):
            before = w.x0 if c == 0 else base[c - 1][1][i]
            rbefore = w.x0 if c == 0 else ref[c - 1][1][i]
            np.testing.assert_array_equal(S[i][c, ncs:], _squared(before), err_msg=f"{what} region {i} column {c}")
            e = _scaled(S[i][c, ncs:], _squared(rbefore))
            assert e <= X_TOL * (c + 1), f"{what} region {i} column {c}: scaled err {e:.3e}"
            np.testing.assert_array_equal(S[i][c, :ncs], lms[c, i, :ncs])
            if targets:
                np.testing.assert_array_equal(T[i][c], fbs[c, o[i] + res.target_index(i)])
    end = [(None, _states(res))]
    _same(end, [base[m - 1]], what + " final", outvecs=False)
    for i in range(res.nlocal):
        e = _scaled(end[0][1][i], ref[m - 1][1][i])
        assert e <= X_TOL * m, f"{what} region {i} final state: scaled err {e:.3e}"


def _check_synchronize(res, fbs, cuda, base, ref, what):
    import torch

    res.synchronize(torch.from_numpy(fbs.copy()).to(cuda), len(fbs))
    torch.cuda.synchronize()
    xs = _states(res)
    for i, x in enumerate(xs):
        np.testing.assert_array_equal(x, base[-1][1][i], err_msg=f"{what} region {i}")
        e = _scaled(x, ref[-1][1][i])
        assert e <= X_TOL * len(fbs), f"{what} region {i}: scaled err {e:.3e}"


# ------------------------------------------------------- A. leakage, every update form
@pytest.mark.parametrize("wdt", ["f32", "f64"])
@pytest.mark.parametrize("leak", [1 / 3, 1 / 12, 0.0, 1.0], ids=["third", "twelfth", "zero", "one"])
def test_leakage_through_every_update_form(cuda, wdt, leak):
    """x = (1 - leak) x + leak tanh(.) in k_res_update_bal (ell_row_value), k_res_update
    in ELL and CSR form (row_value), k_res_begin and k_res_drive, over 3 chained steps of
    4 regions at n = 700, chunk_speedy 132: each form against the oracle, states and
    outvecs bitwise across forms.  leak 0 must leave the state bit for bit; 1 is the
    control the rest of the suite runs."""
    ws = _region_weights(tuple(CASES[:4]), 700)
    fbs, lms = _series(ws, 132, 3)
    ref = _oracle_chain(ws, fbs, lms, 132, leak, unstandardize=True)

    res = _regular(ws, leak, wdt)
    assert res.update_balanced()
    base = _run(res, fbs, lms, cuda)
    _near(base, ref, "sml_res_step")
    if leak == 0.0:
        for _, xs in base:
            for x, w in zip(xs, ws):
                np.testing.assert_array_equal(x, w.x0)
    for mode in (0, 1, 2):
        res = _regular(ws, leak, wdt)
        res.set_begin_mode(mode)
        assert res.begin_fused == (mode > 0)
        seq = _run(res, fbs, lms, cuda, split=True)
        _near(seq, ref, f"begin mode {mode} + finish")
        _same(seq, base, f"begin mode {mode} + finish")
    res = _regular(ws, leak, wdt, per_region=True)
    assert not res.update_balanced() and res.ell_layout(0)["a_width"] > 0
    seq = _run(res, fbs, lms, cuda)
    _near(seq, ref, "per-region update")
    _same(seq, base, "per-region update")
    res = _regular(ws, leak, wdt, csr=True, per_region=True)
    assert not res.update_balanced() and res.ell_layout(0)["a_width"] == 0 and not res.ell_layout(0)["win_ell"]
    seq = _run(res, fbs, lms, cuda)
    _near(seq, ref, "CSR update")
    _same(seq, base, "CSR update")
    _check_synchronize(_regular(ws, leak, wdt), fbs, cuda, base, ref, "synchronize")
    _check_drive(_regular(ws, leak, wdt), ws, fbs, lms, cuda, base, ref, "train_drive", targets=True)
    _check_drive(_regular(ws, leak, wdt, stepwise_drive=True), ws, fbs, lms, cuda, base, ref, "stepwise drive",
                 targets=True)


# ---------------------------------------------------------------------------- B. sizes
# (n, ninp) per region, chunk_speedy, nout, whether the balanced update takes the context
SIZES = {
    # ncs + n = 1 (mod 32) twice; 1089 rows over a block per CU: blocks share regions
    "n1_63_1025": dict(n=[1, 63, 1025], ninp=[1, 5, 33], ncs=0, nout=9, balanced=True, drive=True),
    # the 1024-row pass boundary; ncs + n = 0 and 31 (mod 32)
    "n1024_1023_65": dict(n=[1024, 1023, 65], ninp=[33, 7, 5], ncs=32, nout=17, balanced=True),
    # the last n the balanced update takes (kStageX * 1024)
    "n7168_2049": dict(n=[7168, 2049], ninp=[64, 33], ncs=5, nout=9, balanced=True),
    # the first it refuses: 8 parts per region, the 2-row region's later parts empty
    "n7169_2": dict(n=[7169, 2], ninp=[33, 1], ncs=5, nout=9, balanced=False),
    # the last shape whose x and feedback are staged in LDS: lds_x + ninp = 8160 + 32 = 8192 doubles
    "n8159": dict(n=[8159], ninp=[32], ncs=5, nout=9, balanced=False),
    # the first that is not (k_res_update<kLds = false>), beside a small region
    "n8161_65": dict(n=[8161, 65], ninp=[32, 32], ncs=5, nout=9, balanced=False, drive=True),
    # the largest n sml_res_create admits (16-bit column indices)
    "n65535": dict(n=[65535], ninp=[33], ncs=5, nout=9, balanced=False),
}


@pytest.mark.parametrize("leak", [1.0, 1 / 3], ids=["one", "third"])
@pytest.mark.parametrize("case", list(SIZES))
def test_sizes(cuda, case, leak):
    """2 chained steps as sml_res_step and as begin + finish against the oracle
    (predict_f32, compressed W_in), the two forms bitwise; for two contexts also
    train_drive with m = 3 against synchronize, bitwise."""
    s = SIZES[case]
    ncs, nout = s["ncs"], s["nout"]
    ws = [_weights(n, p, ncs, nout, seed=i) for i, (n, p) in enumerate(zip(s["n"], s["ninp"]))]
    fbs, lms = _series(ws, ncs, 3)
    ref = _oracle_chain(ws, fbs, lms, ncs, leak)
    res = _generic(ws, ncs, nout, leak)
    assert res.update_balanced() == s["balanced"]
    for i, w in enumerate(ws):
        lay = res.ell_layout(i)
        assert lay["a_width"] == 6 and lay["a_overflow"] == (w.n >= 3) and lay["win_ell"], (i, lay)
    base = _run(res, fbs[:2], lms[:2], cuda)
    _near(base, ref, f"{case} sml_res_step")
    seq = _run(_generic(ws, ncs, nout, leak), fbs[:2], lms[:2], cuda, split=True)
    _near(seq, ref, f"{case} begin + finish")
    _same(seq, base, f"{case} begin + finish")
    if s.get("drive"):
        import torch

        sync = _generic(ws, ncs, nout, leak)
        chain = []
        for t in range(3):
            sync.synchronize(torch.from_numpy(fbs[t].copy()).to(cuda), 1)
            chain.append((None, _states(sync)))
        _near(chain, ref, f"{case} synchronize")
        _check_drive(_generic(ws, ncs, nout, leak), ws, fbs, lms, cuda, chain, ref, f"{case} train_drive")


def test_sizes_outside_the_column_index_are_refused(cuda):
    from speedy_ml_amd.reservoir import Reservoirs

    for n in (65536, 0):
        with pytest.raises(SmlError, match="65535"):
            Reservoirs([0], [0], [n], [6], chunk_speedy=0, nout=4, ninp=[3], out_index=[-1] * 4)


# ------------------------------------------------------------ C. chunk and output sizes
@pytest.mark.parametrize("ncs,nout", [(1, 1), (5, 9), (31, 17), (33, 130), (133, 137), (7, 136)])
def test_chunk_and_output_sizes(cuda, ncs, nout):
    """chunk_speedy not a multiple of 4 (odd: the column parity and the state-index
    parity of the readout's squaring differ), nout not a multiple of 8 in the narrow
    readout, padded rows in the wide one (nout_pad 136: the fused begin is taken), and
    nout_pad 144; two regions of n = 257, leakage 1/3, 2 chained steps.  sml_res_step
    and begin + finish at every begin mode: against oracle.predict (dense W_in, no
    unstandardize) and bitwise each other."""
    leak = 1 / 3
    ws = [_weights(257, p, ncs, nout, seed=i) for i, p in enumerate((5, 33))]
    fbs, lms = _series(ws, ncs, 2)
    offs = [0, 5, 38]
    xs = [w.x0 for w in ws]
    ref = []
    for t in range(2):
        outs = []
        for i, w in enumerate(ws):
            out, xs[i] = oracle.predict(w.rows, w.cols, w.vals.astype(np.float64), w.win.astype(np.float64),
                                        w.wout.astype(np.float64), fbs[t, offs[i]:offs[i + 1]], lms[t, i], xs[i],
                                        w.mean, w.std, chunk_speedy=ncs, leakage=leak, unstandardize=False)
            outs.append(out)
        ref.append((np.stack(outs), list(xs)))
    base = _run(_generic(ws, ncs, nout, leak), fbs, lms, cuda)
    _near(base, ref, f"ncs {ncs} nout {nout} sml_res_step")
    wide = (nout + 7) // 8 * 8 % 17 == 0
    assert wide == ((ncs, nout) in ((33, 130), (7, 136)))
    for mode in (0, 1, 2):
        res = _generic(ws, ncs, nout, leak)
        res.set_begin_mode(mode)
        assert res.begin_fused == (mode > 0 and wide)
        seq = _run(res, fbs, lms, cuda, split=True)
        _near(seq, ref, f"ncs {ncs} nout {nout} begin mode {mode} + finish")
        _same(seq, base, f"ncs {ncs} nout {nout} begin mode {mode} + finish")


def test_mixed_output_slots(cuda):
    """out_index with some outputs raw (-1) and the others on distinct mean / std
    slots: outvec = raw * std + mean of its own slot."""
    ncs, nout, leak = 5, 9, 1 / 3
    oidx = [-1, 3, -1, 35, 0, 17, -1, 8, 33]
    ws = [_weights(257, p, ncs, nout, seed=i) for i, p in enumerate((5, 33))]
    fbs, lms = _series(ws, ncs, 2)
    raw = _oracle_chain(ws, fbs, lms, ncs, leak)
    sel = np.array(oidx)
    ref = []
    for ov, xs in raw:
        un = ov.copy()
        for i, w in enumerate(ws):
            un[i, sel >= 0] = ov[i, sel >= 0] * w.std[sel[sel >= 0]] + w.mean[sel[sel >= 0]]
        ref.append((un, xs))
    base = _run(_generic(ws, ncs, nout, leak, out_index=oidx), fbs, lms, cuda)
    _near(base, ref, "mixed out_index sml_res_step")
    seq = _run(_generic(ws, ncs, nout, leak, out_index=oidx), fbs, lms, cuda, split=True)
    _near(seq, ref, "mixed out_index begin + finish")
    _same(seq, base, "mixed out_index begin + finish")


def _slab_steps(res, ws, fbs, lm0, cuda, ld=None):
    """Chained sml_res_step_slab: per step (outvecs, raw outvecs, states)."""
    import torch

    d_lm = torch.from_numpy(lm0.copy()).to(cuda)
    d_next = torch.zeros_like(d_lm)
    d_ov = torch.full((len(ws), ld or res.nout), float("nan"), dtype=torch.float64, device=cuda)
    got = []
    for t in range(len(fbs)):
        res.predict_slab(torch.from_numpy(fbs[t].copy()).to(cuda), d_lm, d_next, d_ov)
        torch.cuda.synchronize()
        got.append((d_ov.cpu().numpy().copy(), d_next.cpu().numpy().copy(), _states(res)))
        d_lm, d_next = d_next, d_lm
    return got


def test_slab_step_with_five_outputs(cuda):
    """sml_res_step_slab at chunk_speedy = nout = 5 over 3 steps, the raw outvec fed
    back as the next local model (test_predict_slab_matches_oracle runs 4)."""
    ncs = nout = 5
    leak = 1 / 3
    ws = [_weights(257, p, ncs, nout, seed=i) for i, p in enumerate((5, 33))]
    fbs, lms = _series(ws, ncs, 3)
    offs = [0, 5, 38]
    got = _slab_steps(_generic(ws, ncs, nout, leak, out_index=[35] * nout), ws, fbs, lms[0, :, :ncs], cuda)
    lm = lms[0, :, :ncs].copy()
    xs = [w.x0 for w in ws]
    for t, (ov, raw, states) in enumerate(got):
        for i, w in enumerate(ws):
            want, xs[i] = oracle.predict_f32(w.rows, w.cols, w.vals, w.wcol, w.wval, w.wout, fbs[t, offs[i]:offs[i + 1]],
                                             lm[i], xs[i], w.mean, w.std, chunk_speedy=ncs, leakage=leak,
                                             unstandardize=False)
            assert _scaled(raw[i], want) <= OUT_TOL
            assert _scaled(ov[i], want * w.std[35] + w.mean[35]) <= OUT_TOL
            assert _scaled(states[i], xs[i]) <= X_TOL * (t + 1)
            lm[i] = want


# -------------------------------------------------------------------- D. W_in shapes
WIN = {
    # ninp > 1024: no balanced update, the drive's next input not through one register per thread
    "ninp1500": dict(n=3000, ninp=1500, win="random", balanced=False, q=0),
    "ninp_above_n": dict(n=63, ninp=200, win="random", balanced=True, q=0),
    # n not a multiple of ninp: the column is stored
    "stored_column": dict(n=257, ninp=5, win="random", balanced=True, q=0),
    # block-diagonal with n odd and past one pass: the column is i / q
    "block_odd_n": dict(n=1035, ninp=45, win="block", balanced=True, q=23),
}


@pytest.mark.parametrize("case", list(WIN))
def test_win_shapes(cuda, case):
    """2 chained steps and train_drive with m = 3: against the oracle, and bitwise the
    CSR copies' results (SML_RES_PATH_CSR)."""
    s = WIN[case]
    ncs, nout, leak = 5, 9, 1 / 3
    ws = [_weights(s["n"], s["ninp"], ncs, nout, seed=3, win=s["win"])]
    fbs, lms = _series(ws, ncs, 3)
    ref = _oracle_chain(ws, fbs, lms, ncs, leak)
    res = _generic(ws, ncs, nout, leak)
    lay = res.ell_layout(0)
    assert res.update_balanced() == s["balanced"]
    assert lay["win_ell"] and lay["win_q"] == s["q"], lay
    base = _run(res, fbs, lms, cuda)
    _near(base, ref, f"{case} sml_res_step")
    csr = _generic(ws, ncs, nout, leak, csr=True)
    assert csr.ell_layout(0)["a_width"] == 0 and not csr.ell_layout(0)["win_ell"] and not csr.update_balanced()
    seq = _run(csr, fbs, lms, cuda)
    _near(seq, ref, f"{case} CSR")
    _same(seq, base, f"{case} CSR")
    _check_drive(_generic(ws, ncs, nout, leak), ws, fbs, lms, cuda, base, ref, f"{case} train_drive")
    _check_drive(_generic(ws, ncs, nout, leak, csr=True), ws, fbs, lms, cuda, base, ref, f"{case} CSR train_drive")


# ------------------------------------------------------------ E. the two untested knobs
@pytest.mark.parametrize("shape", ["nout136", "nout9"])
def test_paced_readout_is_bitwise_the_unpaced(cuda, shape):
    """sml_res_set_read_waves 1, 3 and nitems - 1 (every wave takes a run of items)
    against 0 (a wave per item) in begin + finish: outvecs and states bitwise, each
    within tolerance of the oracle."""
    leak = 1 / 3
    if shape == "nout136":  # 5 regions x 8 wide items
        ws, ncs, nitems = _region_weights(tuple(CASES[:5]), 700), 132, 40
        make = lambda: _regular(ws, leak)  # noqa: E731
    else:  # 3 regions x 2 narrow items
        ncs, nitems = 5, 6
        ws = [_weights(n, p, ncs, 9, seed=i) for i, (n, p) in enumerate(((257, 5), (63, 7), (1025, 33)))]
        make = lambda: _generic(ws, ncs, 9, leak)  # noqa: E731
    fbs, lms = _series(ws, ncs, 2)
    ref = _oracle_chain(ws, fbs, lms, ncs, leak, unstandardize=shape == "nout136")
    outs = {}
    for waves in (0, 1, 3, nitems - 1):
        res = make()
        res.set_read_waves(waves)
        assert not res.begin_fused
        outs[waves] = _run(res, fbs, lms, cuda, split=True)
        _near(outs[waves], ref, f"{shape} read_waves {waves}")
        _same(outs[waves], outs[0], f"{shape} read_waves {waves}")


def _padded_equals_packed(padded, packed, nout, what):
    np.testing.assert_array_equal(padded[:, :nout], packed, err_msg=what)
    assert np.isnan(padded[:, nout:]).all(), f"{what}: the row padding was written"
    assert not np.isnan(packed).any()


@pytest.mark.parametrize("ld", [139, 140])
def test_outvec_stride_regular_context(cuda, ld):
    """sml_res_set_outvec_ld on a 136-output context: sml_res_step, step_finish and
    step_finish_grid write rows ld apart, the first 136 columns bitwise the packed
    result, the padding untouched; the packed results against the oracle."""
    import torch

    leak = 1 / 3
    ws = _region_weights(tuple(CASES[:3]), 700)
    fbs, lms = _series(ws, 132, 2)
    ref = _oracle_chain(ws, fbs, lms, 132, leak, unstandardize=True)
    packed = {}
    for split in (False, True):
        packed[split] = _run(_regular(ws, leak), fbs, lms, cuda, split=split)
        _near(packed[split], ref, "packed")
        res = _regular(ws, leak)
        res.set_outvec_ld(ld)
        wide = _run(res, fbs, lms, cuda, split=split, ld=ld)
        for t in range(2):
            _padded_equals_packed(wide[t][0], packed[split][t][0], 136, f"split {split} step {t}")
        _same([(None, xs) for _, xs in wide], packed[split], "strided", outvecs=False)
    # the finish from the forecast grids
    g4, g2, _ = synthetic_grids(7)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    got = {}
    for stride in (136, ld):
        res = _regular(ws, leak)
        res.set_outvec_ld(stride)
        ov = torch.full((len(ws), stride), float("nan"), dtype=torch.float64, device=cuda)
        lm = torch.zeros((len(ws), 132), dtype=torch.float64, device=cuda)
        res.predict_begin(dev(fbs[0]))
        res.predict_finish_grid(dev(g4), dev(g2), lm, ov)
        torch.cuda.synchronize()
        got[stride] = (ov.cpu().numpy(), lm.cpu().numpy(), _states(res))
    _padded_equals_packed(got[ld][0], got[136][0], 136, "step_finish_grid")
    np.testing.assert_array_equal(got[ld][1], got[136][1])
    want = _oracle_chain(ws, fbs[:1], got[136][1][None], 132, leak, unstandardize=True)  # the tiled local model
    _near([(got[136][0], got[136][2])], want, "step_finish_grid packed")


def test_outvec_stride_generic_context(cuda):
    """The same on a 9-output generic context (stride nout + 3), sml_res_step_slab
    included; a stride below nout, or a change inside a begun step, is refused."""
    import torch

    ncs = nout = 9
    leak, ld = 1 / 3, 12
    ws = [_weights(257, p, ncs, nout, seed=i) for i, p in enumerate((5, 33))]
    fbs, lms = _series(ws, ncs, 2)
    ref = _oracle_chain(ws, fbs, lms, ncs, leak)
    for split in (False, True):
        packed = _run(_generic(ws, ncs, nout, leak), fbs, lms, cuda, split=split)
        _near(packed, ref, "packed")
        res = _generic(ws, ncs, nout, leak)
        res.set_outvec_ld(ld)
        wide = _run(res, fbs, lms, cuda, split=split, ld=ld)
        for t in range(2):
            _padded_equals_packed(wide[t][0], packed[t][0], nout, f"split {split} step {t}")
    slab = {}
    for stride in (nout, ld):
        res = _generic(ws, ncs, nout, leak, out_index=[35] * nout)
        res.set_outvec_ld(stride)
        slab[stride] = _slab_steps(res, ws, fbs, lms[0, :, :ncs], cuda, ld=stride)
    for t in range(2):
        _padded_equals_packed(slab[ld][t][0], slab[nout][t][0], nout, f"step_slab step {t}")
        np.testing.assert_array_equal(slab[ld][t][1], slab[nout][t][1])  # the raw outvecs stay packed
    for i, w in enumerate(ws):  # step 1's raw outvec is predict's
        assert _scaled(slab[nout][0][1][i], ref[0][0][i]) <= OUT_TOL
        assert _scaled(slab[nout][0][0][i], ref[0][0][i] * w.std[35] + w.mean[35]) <= OUT_TOL
    res = _generic(ws, ncs, nout, leak)
    with pytest.raises(SmlError, match="stride"):
        res.set_outvec_ld(nout - 1)
    res.predict_begin(torch.from_numpy(fbs[0].copy()).to(cuda))
    with pytest.raises(SmlError, match="begun"):
        res.set_outvec_ld(ld)
    res.predict_finish(torch.from_numpy(lms[0, :, :ncs].copy()).to(cuda),
                       torch.zeros((2, nout), dtype=torch.float64, device=cuda))
    torch.cuda.synchronize()


# ------------------------------------------- F. the context's memory, shape and refusals
def _lifetime_round(cuda, ncu):
    """One context through every allocation it makes after create: a W_in pool re-laid for
    a second entry per row, the spectral radius's three buffers, the host step's staging
    at two outvec strides, the balanced update's block tables at three grid sizes (8 and
    16 share the first buffer, sized for the device; ncu + 8 grows it), timing events."""
    import torch

    ncs, nout, leak = 5, 9, 1 / 3
    ws = [_weights(257, p, ncs, nout, seed=i) for i, p in enumerate((5, 33))]
    fbs, lms = _series(ws, ncs, 5)
    res = _generic(ws, ncs, nout, leak)
    w = ws[0]
    win2 = w.win.copy()
    win2[(w.wcol + 1) % w.ninp, np.arange(w.n)] = 0.25
    res.load_region(0, w.rows, w.cols, w.vals, win2, w.wout, w.mean, w.std)  # grow_win_pool
    assert not res.ell_layout(0)["win_ell"] and not res.update_balanced()
    got = {}
    res.set_reference_paths(radius_global=True)
    lo, hi, iters, info = res.spectral_radius()
    assert (info == 0).all(), info
    got["lo"], got["hi"], got["iters"] = lo, hi, iters
    got["host"] = res.predict_host(fbs[0], lms[0, :, :ncs])
    res.set_outvec_ld(nout + 3)  # the staging is re-sized for the stride
    got["host_ld"] = res.predict_host(fbs[1], lms[1, :, :ncs])
    res.load_region(0, w.rows, w.cols, w.vals, w.win, w.wout, w.mean, w.std)  # ELL form again
    assert res.update_balanced()
    res.enable_timing(2)
    ov = torch.full((res.nlocal, nout + 3), float("nan"), dtype=torch.float64, device=cuda)
    for t, cus in enumerate((8, 16, ncu + 8)):
        res.set_update_cus(cus)
        res.predict_begin(torch.from_numpy(fbs[2 + t].copy()).to(cuda))
        res.predict_finish(torch.from_numpy(lms[2 + t, :, :ncs].copy()).to(cuda), ov)
        torch.cuda.synchronize()
        got[f"ov{t}"] = ov.cpu().numpy().copy()
    upd, rd = res.kernel_times()
    assert len(upd) == 2 and len(rd) == 2
    for i in range(res.nlocal):
        got[f"x{i}"] = res.get_state(i)
    res.close()
    return got


def test_context_create_destroy_repeats(cuda):
    """Eight contexts in one process, each taken through every lazy allocation, growth and
    release (_lifetime_round) and destroyed: every round's outvecs, states and radius
    enclosure are bitwise the first round's."""
    import torch

    ncu = torch.cuda.get_device_properties(cuda).multi_processor_count
    first = _lifetime_round(cuda, ncu)
    assert not any(np.isnan(v[:, :9]).any() for k, v in first.items() if k.startswith("ov"))
    assert (first["lo"] <= first["hi"]).all() and (first["lo"] > 0).all()
    for r in range(1, 8):
        got = _lifetime_round(cuda, ncu)
        assert sorted(got) == sorted(first)
        for k in first:
            np.testing.assert_array_equal(got[k], first[k], err_msg=f"round {r} {k}")


# n / ninp per region, chunk_speedy, nout; what the context must report with begin mode 1
# (step_shape's values, pinned on the CPU by tests/reservoir_layout_check.cpp)
REPORTED = {
    "n7168": dict(n=[7168, 2049], ninp=[64, 33], ncs=5, nout=9, balanced=True, fused=False),
    "n7169": dict(n=[7169, 2], ninp=[33, 1], ncs=5, nout=9, balanced=False, fused=False),
    "nout136": dict(n=[257, 257], ninp=[5, 33], ncs=7, nout=136, balanced=True, fused=True),
    "nout137": dict(n=[257, 257], ninp=[5, 33], ncs=133, nout=137, balanced=True, fused=False),
}


@pytest.mark.parametrize("case", list(REPORTED))
def test_reported_path_is_the_launched_path(cuda, case):
    """On each side of the balanced update's edge (n 7168 / 7169) and of the fused
    begin's (nout_pad 136 / 144): sml_res_update_balanced and sml_res_begin_fused report
    the shape's value, and two begin + finish steps are bitwise those of the same context
    with the per-region update forced and begin mode 0 -- so the form reported is a form
    that ran, and it computes what the reference path computes."""
    s = REPORTED[case]
    ncs, nout, leak = s["ncs"], s["nout"], 1 / 3
    ws = [_weights(n, p, ncs, nout, seed=i) for i, (n, p) in enumerate(zip(s["n"], s["ninp"]))]
    fbs, lms = _series(ws, ncs, 2)
    res = _generic(ws, ncs, nout, leak)
    res.set_begin_mode(1)
    assert res.update_balanced() == s["balanced"]
    assert res.begin_fused == s["fused"]
    seq = _run(res, fbs, lms, cuda, split=True)
    ref = _generic(ws, ncs, nout, leak, per_region=True)
    ref.set_begin_mode(0)
    assert not ref.update_balanced() and not ref.begin_fused
    _same(seq, _run(ref, fbs, lms, cuda, split=True), f"{case} against the reference paths")
    assert not any(np.isnan(ov).any() for ov, _ in seq)


@functools.lru_cache(maxsize=None)
def _fresh_process_steps(tmp):
    """_refused_create_child.py's two steps from a process that has done nothing else."""
    import os
    import subprocess
    import sys

    out = os.path.join(tmp, "fresh.npz")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_refused_create_child.py")
    p = subprocess.run([sys.executable, "-u", child, out], timeout=100, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return dict(np.load(out))


def test_refused_creates_leave_a_usable_process(cuda, tmp_path):
    """A sml_train_create refused for naug[1] = 1 and a sml_res_create refused for a
    region id out of range (each after the context object exists, so each takes the
    bail-out), then a good create and one step of each: bitwise a fresh process's."""
    import _refused_create_child as child
    from speedy_ml_amd.training import Trainer

    fresh = _fresh_process_steps(str(tmp_path))
    with pytest.raises(SmlError, match=r"naug\[1\] = 1"):
        Trainer([130, 1], child.TRAIN_NOUT)
    np.testing.assert_array_equal(child.train_step(cuda), fresh["wout"])
    with pytest.raises(SmlError, match="region id 1152 out of range"):
        child.res_create(child.res_weights(), region_ids=(0, 1152))
    ov, x0, x1 = child.res_step(cuda)
    np.testing.assert_array_equal(ov, fresh["ov"])
    np.testing.assert_array_equal(x0, fresh["x0"])
    np.testing.assert_array_equal(x1, fresh["x1"])
    assert not np.isnan(ov).any() and np.abs(fresh["wout"]).max() > 0
