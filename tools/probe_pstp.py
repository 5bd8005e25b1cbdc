"""Diagnostic: the pair row kernel's roles (k_st_gridspec_p) from the profiling build's
stamps (-DSML_PSTAMPS: tools/build_variant.sh pst ...), us from the physics phase start,
for a window ending on a longwave-only step (nleap 24) and on a shortwave step (nleap 22).
Eight windows from the same state, the first two dropped; per stamp: the median over the
48 row blocks of each block's median over the windows, [the range of the windows' medians
over blocks], and the slowest block (its row).
    SML_LIB=abx/pst/speedy-ml-1_amd/lib/libspeedyml.so python tools/probe_pstp.py"""
import ctypes
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speedy-ml-1_amd"))
from speedy_ml_amd._lib import lib  # noqa: E402
from speedy_ml_amd.dynamics import Dynamics  # noqa: E402
from speedy_ml_amd.synthetic import dyn_state, phys_boundary  # noqa: E402

STAMPS = ((9, "dynamics (wave 0) done"), (11, "moist (wave 2): thermo"), (12, "moist: convmf + lscond, hand-over"),
          (21, "pairs (wave 4): shortwave first stage"), (13, "moist: vdifsc done"), (15, "pairs: sw / prefetch"),
          (16, "pairs: lw down"), (17, "pairs: suflux"), (18, "pairs: wave 4 done"), (19, "pairs: wave 6 done"),
          (20, "sums' barrier passed"))

L = lib()
L.sml_dbg_pst.argtypes = [ctypes.c_void_p]
st, forcing = dyn_state()
d = Dynamics()
d.set_forcing(**forcing)
d.set_state(st)
d.set_physics(phys_boundary(d, forcing["phis"]))
for nleap, name in ((24, "longwave-only step"), (22, "shortwave step")):
    acc = []
    for rep in range(8):
        d.set_state(st)
        d.set_rad_state(None)
        d.set_clock(1, True)
        d.window(nleap)
        torch.cuda.synchronize()
        buf = np.zeros((48, 32), dtype=np.int64)
        assert L.sml_dbg_pst(buf.ctypes.data) == 0
        b = buf.astype(np.float64) / 100.0  # wall_clock64 at 100 MHz -> us
        acc.append(b - b[:, 8:9])
    a = np.array(acc[2:])  # (window, row, stamp)
    med = np.median(a, axis=0)
    print(f"== {name} (nleap {nleap})")
    for s, what in STAMPS:
        if not buf[:, s].any() or (s == 21 and nleap == 24):  # (not written by this build / kind of step)
            continue
        pw = np.median(a[:, :, s], axis=1)
        print(f"  {what:38s} {np.median(med[:, s]):6.2f} [{pw.min():.2f}..{pw.max():.2f}]  slowest block "
              f"{med[:, s].max():.2f} (row {int(med[:, s].argmax())})")
d.close()
