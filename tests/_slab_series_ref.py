"""NumPy restatement of the slab training series (sml_slab_train_series).

For slab reservoir s (a local sst region of the atmo context) and its feedback entry e
(7 * in2d entries: the lowest level's 4 variables, logp, sst, tisr over the input tile),
z_t[e] is the standardised atmo feedback entry slab_input_index[e] of step t, and
    a_t[e] = (z_lo[e] + ... + z_t[e]) / d,   lo = max(0, t - window + 1),
summed from 0.0 in ascending step order, one add a term, then one division; d = the number
of terms while t + 1 < window, `divisor` afterwards.

averaged():    float64, operation for operation (an explicit loop of adds: np.sum is pairwise),
               over blocks of standardised feedback -- bit for bit what the kernel writes.
averaged_ld(): longdouble from the raw grids, with the bound of the float64 value's error:
               each z errs by at most 2u |z| (a subtraction and a division), the ordered sum
               of w terms by at most (w - 1) u sum|z|, the division by u:
                   |a^ - a| <= 1.01 (w + 2) u sum|z| / d,   u = 2^-53.
Nothing here reads the library's index tables: the entries come from the oracle's
slab_input_index and _series_ref's geometry.
"""
from __future__ import annotations

import numpy as np

import _series_ref as ref

U = np.longdouble(2.0) ** -53


def slab_cases(cases):
    """(local atmo row, region) of the slab reservoirs: the sst regions, in order."""
    return [(i, r) for i, (r, flag) in enumerate(cases) if flag]


def slab_offsets(cases):
    off = [0]
    for _, r in slab_cases(cases):
        g = ref.geometry(r)
        off.append(off[-1] + 7 * g["inx"] * g["iny"])
    return off


def gather(cases, blocks):
    """z [T, slab feedback] from blocks [T, atmo feedback] through slab_input_index."""
    import oracle

    off = ref.feedback_offsets(cases)
    cols = np.concatenate([off[i] + oracle.slab_input_index(r) for i, r in slab_cases(cases)])
    return np.ascontiguousarray(blocks[:, cols])


def tisr_entries(cases):
    """Mask [slab feedback] of the tisr entries (the last in2d of each reservoir)."""
    soff = slab_offsets(cases)
    m = np.zeros(soff[-1], bool)
    for j, (_, r) in enumerate(slab_cases(cases)):
        g = ref.geometry(r)
        m[soff[j + 1] - g["inx"] * g["iny"]:soff[j + 1]] = True
    return m


def averaged(z, window: int, divisor: int, t0: int = 0, ncols: int | None = None):
    """Columns t0 .. t0 + ncols - 1 of the rolling mean of z [T, n] (float64), the kernel's
    operations in the kernel's order."""
    z = np.asarray(z, dtype=np.float64)
    T = z.shape[0]
    ncols = T - t0 if ncols is None else ncols
    out = np.zeros((ncols, z.shape[1]))
    for t in range(t0, t0 + ncols):
        lo = max(0, t - window + 1)
        s = np.zeros(z.shape[1])
        for k in range(lo, t + 1):
            s = s + z[k]
        out[t - t0] = s / np.float64(t + 1 - lo if t + 1 < window else divisor)
    return out


def standardised_ld(cases, g4, g2, pr, sst, tisr, mean, std):
    """z [T, slab feedback] in longdouble from the raw grids (not through tile_series):
    mean / std [nlocal, 36] the atmo context's."""
    L = np.longdouble
    T = g4.shape[0]
    cols = []
    for i, r in slab_cases(cases):
        X, Y = ref.tile_points(r)
        m, s = np.asarray(mean[i], L), np.asarray(std[i], L)
        low = g4[:, ref.ZGRID - 1][:, Y, X, :].astype(L)  # [T, iny, inx, v]: the lowest level, v fastest
        slot = np.arange(ref.NVARS) * ref.ZGRID + (ref.ZGRID - 1)
        cols.append(((low - m[slot]) / s[slot]).reshape(T, -1))
        for f, l in ((g2, 32), (sst, 35), (tisr, 33)):
            if f is None:
                cols.append(np.zeros((T, X.size), L))
            else:
                cols.append(((f[:, Y, X].astype(L) - m[l]) / s[l]).reshape(T, -1))
    return np.concatenate(cols, axis=1)


def averaged_ld(zl, window: int, divisor: int):
    """(a, bound) [T, n]: the rolling mean of the longdouble z and the bound on the float64
    value's distance from it."""
    L = np.longdouble
    T = zl.shape[0]
    a, bound = np.zeros(zl.shape, L), np.zeros(zl.shape, L)
    absz = np.abs(zl)
    for t in range(T):
        lo = max(0, t - window + 1)
        w = t + 1 - lo
        d = L(w if t + 1 < window else divisor)
        a[t] = zl[lo:t + 1].sum(axis=0) / d
        bound[t] = L(1.01) * (w + 2) * U * absz[lo:t + 1].sum(axis=0) / d
    return a, bound
