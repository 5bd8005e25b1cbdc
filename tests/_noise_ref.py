"""NumPy restatement of the input noise's definition, from the text
alone -- none of it through the library:

    mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
    key(stream)         = mix(mix(seed + 0x9E3779B97F4A7C15) ^ (8 * region + stream))
    draw(stream, index) = mix(key(stream) + (index + 1) * 0x9E3779B97F4A7C15)
    index = (t << 20) | e;  b1 = draw(4, index) >> 11;  b2 = draw(5, index) >> 11
    u1 = (b1 + 1) 2^-53;  u2 = b2 2^-53;  g = sqrt(-2 log u1) cos(2 pi u2)

in uint64 arrays (wrapping) and, for g, in longdouble on the exact u1, u2.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
LD = np.longdouble
# pi beyond float64 (longdouble(np.pi) is only the float64 value): pi = np.pi + _PI_LO
_PI_LO = LD("1.2246467991473531772e-16")
G_MAX = float(np.sqrt(106.0 * np.log(LD(2))))  # sqrt(-2 log 2^-53)


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def mix(z):
    z = _u64(z).copy()
    z ^= z >> np.uint64(30)
    z *= M1
    z ^= z >> np.uint64(27)
    z *= M2
    z ^= z >> np.uint64(31)
    return z


def stream_key(seed: int, region: int, stream: int):
    return mix(mix(_u64(seed) + GOLDEN) ^ _u64(8 * int(region) + int(stream)))


def draw(key, index):
    return mix(_u64(key) + (_u64(index) + np.uint64(1)) * GOLDEN)


def bits(seed: int, region: int, t, e):
    """b1, b2 of (t, e), broadcast against each other (uint64 arrays)."""
    t, e = np.broadcast_arrays(_u64(t), _u64(e))
    index = (t << np.uint64(20)) | e
    return draw(stream_key(seed, region, 4), index) >> np.uint64(11), draw(stream_key(seed, region, 5), index) >> np.uint64(11)


def block_bits(seed: int, ids, ninps, t0: int, m: int):
    """b1, b2 [m, sum(ninps)] of blocks t0 .. t0 + m - 1 of a context whose local regions
    have noise ids `ids` and feedback lengths `ninps`, in the packed layout."""
    t = np.arange(t0, t0 + m, dtype=np.uint64)[:, None]
    parts = [bits(seed, r, t, np.arange(n, dtype=np.uint64)[None, :]) for r, n in zip(ids, ninps)]
    return np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)


def uniforms_ld(b1, b2):
    """The exact u1 in (0, 1], u2 in [0, 1) as longdouble (64-bit mantissa: b + 1 <= 2^53 is exact)."""
    return (b1.astype(LD) + 1) * LD(U), b2.astype(LD) * LD(U)


def normals_ld(b1, b2):
    """(g, R): g = R cos(2 pi u2), R = sqrt(-2 log u1), in longdouble."""
    u1, u2 = uniforms_ld(b1, b2)
    R = np.sqrt(-2 * np.log(u1))
    return R * np.cos(2 * LD(np.pi) * u2 + 2 * _PI_LO * u2), R


def moments(g, region_lengths):
    """Of g [m, sum(region_lengths)] in float64: the sample mean, the variance about it, and
    the lag-1 correlations along e (neighbouring entries of one region, one block) and along
    t (one entry, neighbouring blocks): mean((a - mean)(b - mean)) / variance over the pairs."""
    g = np.asarray(g, dtype=np.float64)
    mean = g.mean()
    d = g - mean
    var = (d * d).mean()
    off = np.concatenate([[0], np.cumsum(region_lengths)])
    pe = np.concatenate([(d[:, a:b - 1] * d[:, a + 1:b]).ravel() for a, b in zip(off[:-1], off[1:])])
    pt = (d[:-1] * d[1:]).ravel()
    return mean, var, pe.mean() / var, pt.mean() / var


def moment_caps(N: int):
    """The issue's conditions: |mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N), |lag-1| <= 5 / sqrt(N)."""
    return 5.0 / np.sqrt(N), 5.0 * np.sqrt(2.0 / N), 5.0 / np.sqrt(N)


# The moments' sample (tests/test_input_noise_cpu.py and _gpu.py): the 8-region context of
# _series_ref.CASES, MOMENT_M blocks from step MOMENT_T0: N = 64 * 4120 = 263680 >= 2^18
MOMENT_SEED, MOMENT_T0, MOMENT_M = 2024, 1000, 64
