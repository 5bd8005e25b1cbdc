"""One good sml_train_create + accumulate + solve, and one good sml_res_create + load +
sml_res_step, each with fixed inputs: run by test_reservoir_edges_gpu.py in its own
process after a refused create, and here in a fresh process (python _refused_create_child.py
OUT.npz), for the bitwise comparison of the two."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, "speedy-ml-1_amd") not in sys.path:
    sys.path.insert(0, os.path.join(REPO, "speedy-ml-1_amd"))

NAUGS, TRAIN_NOUT, TRAIN_M = [130, 257], 136, 32
RES_N, RES_NINP, RES_NCS, RES_NOUT = [65, 33], [5, 7], 5, 9


def train_step(cuda):
    """W_out of two regions from one batch of 32 columns."""
    import torch
    from speedy_ml_amd.training import Trainer

    rng = np.random.default_rng(71)
    S = [np.tanh(rng.standard_normal((TRAIN_M, n))) for n in NAUGS]
    T = [rng.standard_normal((TRAIN_M, TRAIN_NOUT)) for _ in NAUGS]
    states = torch.from_numpy(np.concatenate([a.ravel() for a in S])).to(cuda)
    targets = torch.from_numpy(np.concatenate([a.ravel() for a in T])).to(cuda)
    tr = Trainer(NAUGS, TRAIN_NOUT)
    tr.accumulate(states, targets, TRAIN_M)
    w, info = tr.solve(4, 0.001, 1.0, True, 0.0)
    out = w.cpu().numpy().copy()
    tr.close()
    assert (info == 0).all(), info
    return out


def res_weights():
    """Two small regions: A with 3 entries per row, W_in one entry per row, all exact in float."""
    rng = np.random.default_rng(73)
    ws = []
    for n, ninp in zip(RES_N, RES_NINP):
        rows = np.concatenate([rng.permutation(n) + 1 for _ in range(3)]).astype(np.int32)
        cols = np.concatenate([rng.permutation(n) + 1 for _ in range(3)]).astype(np.int32)
        vals = (0.3 * rng.random(len(rows))).astype(np.float32)
        win = np.zeros((ninp, n), dtype=np.float32)
        win[rng.integers(0, ninp, n), np.arange(n)] = (rng.random(n) - 0.5).astype(np.float32) + 1.0
        wout = (0.01 * (2.0 * rng.random((RES_NCS + n, RES_NOUT)) - 1.0)).astype(np.float32)
        ws.append(dict(n=n, ninp=ninp, k=len(rows), rows=rows, cols=cols, vals=vals, win=win, wout=wout,
                       mean=rng.standard_normal(36), std=0.5 + rng.random(36), x0=rng.random(n) - 0.5))
    return ws


def res_create(ws, region_ids=(0, 1)):
    from speedy_ml_amd.reservoir import Reservoirs

    return Reservoirs(list(region_ids), [0] * len(ws), [w["n"] for w in ws], [w["k"] for w in ws],
                      chunk_speedy=RES_NCS, nout=RES_NOUT, leakage=1 / 3, ninp=[w["ninp"] for w in ws],
                      out_index=[-1] * RES_NOUT)


def res_step(cuda):
    """The outvecs and states after one sml_res_step."""
    import torch

    ws = res_weights()
    res = res_create(ws)
    for i, w in enumerate(ws):
        res.load_region(i, w["rows"], w["cols"], w["vals"], w["win"], w["wout"], w["mean"], w["std"])
        res.set_state(i, w["x0"])
    rng = np.random.default_rng(79)
    fb = torch.from_numpy(rng.standard_normal(sum(RES_NINP))).to(cuda)
    lm = torch.from_numpy(rng.standard_normal((len(ws), RES_NCS))).to(cuda)
    ov = torch.full((len(ws), RES_NOUT), float("nan"), dtype=torch.float64, device=cuda)
    res.predict(fb, lm, ov)
    torch.cuda.synchronize()
    out = [ov.cpu().numpy().copy()] + [res.get_state(i) for i in range(len(ws))]
    res.close()
    return out


if __name__ == "__main__":
    import torch

    dev = torch.device("cuda:0")
    r = res_step(dev)
    np.savez(sys.argv[1], wout=train_step(dev), ov=r[0], x0=r[1], x1=r[2])
