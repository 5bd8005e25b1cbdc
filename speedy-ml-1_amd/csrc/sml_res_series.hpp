// sml_res_series.hpp -- the training front end on a series of global grids: the
// standardisation statistics of every local region (k_series_sum, k_series_m2,
// k_series_combine) and the tiling of T steps in one launch (k_tile_series,
// k_tile_series_model).
//
// Statistics.  For local region i and slot l of the 36, P is the multiset of grid sources
// of the region's feedback entries of that slot (its input tile: SeriesTables::pt_grid),
// N = T |P|, and
//     mean = (sum_t sum_p x_t[p]) / N,   std = sqrt(sum_t sum_p (x_t[p] - mean)^2 / N):
// the population form, the reference's two-pass form (standardize_data_5d_logp_tisr,
// mod_utilities.f90:1137-1186).  A deliberate difference: the reference's precipitation
// statistic (standardize_data_3d, :887-905) is the one-pass sqrt((sum x^2 - (sum x)^2 / N) / N),
// equal mathematically and ill-conditioned; here every slot, precipitation included, takes
// the two-pass value.  There are no guards: a constant field gives the std its rounding
// leaves (0 where the sums are exact), as in the reference.
//
// Regions overlap, so the series is not gathered per region.  It is streamed twice, per
// grid point, and the regions combine their points' moments afterwards:
//   k_series_sum      chunk c of point p:  s_c[p] = x_t0[p]; s_c[p] = s_c[p] + x_t[p]
//   k_series_m2       mu[p] = (s_0[p] + s_1[p] + ...) / T;  q_c[p] = 0; d = x_t[p] - mu[p]; q_c[p] = q_c[p] + d * d
//   k_series_combine  m = (sum_p mu[p]) / |P|;  Q = sum_p ((q_0[p] + q_1[p] + ...) + T * (d * d)), d = mu[p] - m;
//                     mean = m, std = sqrt(Q / N)
// since sum_t (x - m)^2 = sum_t (x - mu_p)^2 + T (mu_p - m)^2 for the point's own mean mu_p.
// The chunks (series_split) are a function of T alone, every sum above runs in index order
// in one thread, and nothing is shared between threads but the workspace across the launch
// boundaries: no floating-point atomics, no waits, the same bits on any stream.
// A thread of the two streaming kernels owns one (k, j, i) quad of the 4-d grid (32 bytes,
// two 16-byte loads) or one point of a 2-d field and keeps kSerTile steps' loads in
// flight.  The unit is built with -ffp-contract=off: no product is fused into a sum.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sml_internal.hpp"
#include "sml_reservoir_layout.hpp"

namespace {
using namespace sml;

constexpr int kSerTile = 8;      // steps whose loads one thread of the statistics issues together
constexpr int kSerThreads = 64;  // threads per block of the streaming kernels
constexpr int kSerQuadBlocks = kGrid4d / kVars / kSerThreads;  // 576
constexpr int kSerPointBlocks = kGrid2d / kSerThreads;         // 72 per 2-d field
static_assert(kSerQuadBlocks * kSerThreads * kVars == kGrid4d && kSerPointBlocks * kSerThreads == kGrid2d,
              "the streaming kernels' blocks tile the grids exactly");

// the series' pointers: step t of the 4-d grid at g4 + t * g4s, of 2-d field f at f2[f] + t * g2s
struct SeriesIn {
    const double *g4;
    const double *f2[kSerFields2d];  // kSerLogp, kSerPrecip, kSerSst, kSerTisr; NULL: the field is absent
    int64_t g4s, g2s;
};

// the statistics' workspace: sum [S][kSerPoints], mu [kSerPoints], m2 [S][kSerPoints]
struct SeriesWork {
    double *sum, *mu, *m2;
};

template <int NV>
__device__ __forceinline__ void ser_load(const double *__restrict__ p, double (&v)[NV]) {
    if constexpr (NV == 1) {
        v[0] = *p;
    } else {
#pragma unroll
        for (int c = 0; c < NV; c += 2) {
            const double2 t = *reinterpret_cast<const double2 *>(p + c);
            v[c] = t.x;
            v[c + 1] = t.y;
        }
    }
}
template <int NV>
__device__ __forceinline__ void ser_store(double *__restrict__ p, const double (&v)[NV]) {
    if constexpr (NV == 1) {
        *p = v[0];
    } else {
#pragma unroll
        for (int c = 0; c < NV; c += 2) *reinterpret_cast<double2 *>(p + c) = make_double2(v[c], v[c + 1]);
    }
}

// (selected, not indexed: a dynamic index into the argument's array would go through scratch)
__device__ __forceinline__ const double *ser_field(const SeriesIn &in, int f) {
    return f == kSerLogp ? in.f2[kSerLogp] : f == kSerPrecip ? in.f2[kSerPrecip]
         : f == kSerSst  ? in.f2[kSerSst]  : in.f2[kSerTisr];
}

// this block's item: the series pointer of its NV values at step 0 (NULL: an absent field),
// its stride, and the values' place in the workspace
struct SerItem {
    const double *x;
    int64_t stride;
    int at;
};
__device__ __forceinline__ SerItem ser_item(const SeriesIn &in, int b, int tid) {
    if (b < kSerQuadBlocks) {
        const int o = (b * kSerThreads + tid) * kVars;
        return {in.g4 + o, in.g4s, o};
    }
    const int f = (b - kSerQuadBlocks) / kSerPointBlocks;
    const int o = ((b - kSerQuadBlocks) % kSerPointBlocks) * kSerThreads + tid;
    const double *x = ser_field(in, f);
    return {x ? x + o : nullptr, in.g2s, kGrid4d + f * kGrid2d + o};
}

// steps [t0, t1) of NV neighbouring values, summed in step order
template <int NV>
__device__ __forceinline__ void ser_sum(const double *__restrict__ x, int64_t stride, int t0, int t1,
                                        double *__restrict__ out) {
    double s[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) s[c] = 0.0;
    for (int a = t0; a < t1; a += kSerTile) {
        double v[kSerTile][NV];
#pragma unroll
        for (int k = 0; k < kSerTile; ++k)
            if (a + k < t1) ser_load<NV>(x + (size_t)(a + k) * stride, v[k]);
#pragma unroll
        for (int k = 0; k < kSerTile; ++k)
            if (a + k < t1) {
#pragma unroll
                for (int c = 0; c < NV; ++c) s[c] = a + k == t0 ? v[k][c] : s[c] + v[k][c];
            }
    }
    ser_store<NV>(out, s);
}

// the point's mean from the S chunk sums, then steps [t0, t1) of (x - mu)^2 in step order
template <int NV>
__device__ __forceinline__ void ser_m2(const double *__restrict__ x, int64_t stride, int t0, int t1, int T, int S,
                                       const double *__restrict__ sum, double *__restrict__ mu_out,
                                       double *__restrict__ out) {
    double mu[NV], q[NV];
    ser_load<NV>(sum, mu);
    for (int c = 1; c < S; ++c) {
        double p[NV];
        ser_load<NV>(sum + (size_t)c * kSerPoints, p);
#pragma unroll
        for (int k = 0; k < NV; ++k) mu[k] = mu[k] + p[k];
    }
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        mu[c] = mu[c] / (double)T;
        q[c] = 0.0;
    }
    if (mu_out) ser_store<NV>(mu_out, mu);
    for (int a = t0; a < t1; a += kSerTile) {
        double v[kSerTile][NV];
#pragma unroll
        for (int k = 0; k < kSerTile; ++k)
            if (a + k < t1) ser_load<NV>(x + (size_t)(a + k) * stride, v[k]);
#pragma unroll
        for (int k = 0; k < kSerTile; ++k)
            if (a + k < t1) {
#pragma unroll
                for (int c = 0; c < NV; ++c) {
                    const double d = v[k][c] - mu[c];
                    q[c] = q[c] + d * d;
                }
            }
    }
    ser_store<NV>(out, q);
}

// grid (kSerQuadBlocks + kSerFields2d * kSerPointBlocks, S): blocks [0, 576) the quads of the
// 4-d grid, then 72 per 2-d field; blockIdx.y the chunk of steps [y * len, min(T, (y + 1) * len))
__global__ __launch_bounds__(kSerThreads) void k_series_sum(SeriesIn in, SeriesWork w, int T, int len) {
    const SerItem it = ser_item(in, blockIdx.x, threadIdx.x);
    if (!it.x) return;
    const int t0 = blockIdx.y * len, t1 = min(T, t0 + len);
    double *out = w.sum + (size_t)blockIdx.y * kSerPoints + it.at;
    if (blockIdx.x < kSerQuadBlocks) ser_sum<kVars>(it.x, it.stride, t0, t1, out);
    else ser_sum<1>(it.x, it.stride, t0, t1, out);
}

__global__ __launch_bounds__(kSerThreads) void k_series_m2(SeriesIn in, SeriesWork w, int T, int len, int S) {
    const SerItem it = ser_item(in, blockIdx.x, threadIdx.x);
    if (!it.x) return;
    const int t0 = blockIdx.y * len, t1 = min(T, t0 + len);
    double *mu = blockIdx.y == 0 ? w.mu + it.at : nullptr;
    double *out = w.m2 + (size_t)blockIdx.y * kSerPoints + it.at;
    if (blockIdx.x < kSerQuadBlocks) ser_m2<kVars>(it.x, it.stride, t0, t1, T, S, w.sum + it.at, mu, out);
    else ser_m2<1>(it.x, it.stride, t0, t1, T, S, w.sum + it.at, mu, out);
}

// one thread per (local region, slot): the region's points in the tile's order.  A slot
// the region lacks (sst unflagged, or the field absent) keeps the context's defaults,
// mean 0 and std 1.  sst_change[i] = 1 iff Q > 0 and std > 0.2 (standardize_sst_data_3d,
// mod_utilities.f90:846-885); 0 for a region without the sst slot.
__global__ void k_series_combine(const int32_t *__restrict__ pt_off, const int32_t *__restrict__ pt_grid,
                                 const unsigned char *__restrict__ sst_flag, SeriesWork w, int has_sst,
                                 int has_tisr, int T, int S, int nlocal, double *__restrict__ meanstd,
                                 int *__restrict__ sst_change) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nlocal * kMeanStd) return;
    const int i = e / kMeanStd, l = e % kMeanStd;
    double *ms = meanstd + (size_t)i * 2 * kMeanStd;
    int base, step = 1;  // the slot's value of 2-d point p at base + step * p of the series' index space
    bool have = true;
    if (l < 32) {
        base = l / kZGrid + kVars * kGrid2d * (l % kZGrid);
        step = kVars;
    } else if (l == 32) {
        base = kGrid4d + kSerLogp * kGrid2d;
    } else if (l == 34) {
        base = kGrid4d + kSerPrecip * kGrid2d;
    } else if (l == 35) {
        base = kGrid4d + kSerSst * kGrid2d;
        have = has_sst && sst_flag[i];
    } else {
        base = kGrid4d + kSerTisr * kGrid2d;
        have = has_tisr;
    }
    const int p0 = pt_off[i], p1 = pt_off[i + 1];
    if (!have || p1 <= p0) {
        ms[l] = 0.0;
        ms[kMeanStd + l] = 1.0;
        if (l == 35 && sst_change) sst_change[i] = 0;
        return;
    }
    const double np = (double)(p1 - p0);
    double s = 0.0;
    for (int p = p0; p < p1; ++p) {
        const double mu = w.mu[base + step * pt_grid[p]];
        s = p == p0 ? mu : s + mu;
    }
    const double m = s / np;
    double Q = 0.0;
    for (int p = p0; p < p1; ++p) {
        const int at = base + step * pt_grid[p];
        double q = w.m2[at];
        for (int c = 1; c < S; ++c) q = q + w.m2[(size_t)c * kSerPoints + at];
        const double d = w.mu[at] - m;
        Q = Q + (q + (double)T * (d * d));
    }
    const double sd = sqrt(Q / ((double)T * np));
    ms[l] = m;
    ms[kMeanStd + l] = sd;
    if (l == 35 && sst_change) sst_change[i] = (Q > 0.0 && sd > 0.2) ? 1 : 0;
}

// ---- the series tilings.  A thread reads its table entries and its mean / std once and
// serves every step with them, kTileMem steps' gathers in flight together; per element
// the two operations are k_tile_feedback's: t = x - mean; t / std.  An entry whose field
// is absent (NULL) is left untouched, as the single-grid call leaves it.
__global__ void k_tile_series(const int32_t *__restrict__ src, const uint8_t *__restrict__ lidx,
                              const uint16_t *__restrict__ reg, const double *__restrict__ meanstd, SeriesIn in,
                              double *__restrict__ inputs, int64_t in_stride, int total, int T) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int s = src[e];
    const double *g;
    int64_t gs;
    if (s < kGrid4d) {
        g = in.g4 + s;
        gs = in.g4s;
    } else {
        const int f = (s - kGrid4d) / kGrid2d;
        const double *b = ser_field(in, f);
        if (!b) return;
        g = b + (s - kGrid4d - f * kGrid2d);
        gs = in.g2s;
    }
    const double *ms = meanstd + (size_t)reg[e] * 2 * kMeanStd;
    const int l = lidx[e];
    const double mean = ms[l], stdv = ms[kMeanStd + l];
    double *out = inputs + e;
    for (int t0 = 0; t0 < T; t0 += kTileMem) {
        double v[kTileMem];
#pragma unroll
        for (int k = 0; k < kTileMem; ++k)
            if (t0 + k < T) v[k] = g[(size_t)(t0 + k) * gs];
#pragma unroll
        for (int k = 0; k < kTileMem; ++k)
            if (t0 + k < T) {
                const double t = v[k] - mean;
                out[(size_t)(t0 + k) * in_stride] = t / stdv;
            }
    }
}

// the T model blocks [nlocal][ncs] from the forecast series: per step k_tile_local_model's
__global__ void k_tile_series_model(const int32_t *__restrict__ src, const uint8_t *__restrict__ lidx,
                                    const double *__restrict__ meanstd, const double *__restrict__ fc4, int64_t fc4s,
                                    const double *__restrict__ fc2, int64_t fc2s, double *__restrict__ model,
                                    int64_t model_stride, int ncs, int total, int T) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int s = src[e];
    const double *g = s < kGrid4d ? fc4 + s : fc2 + (s - kGrid4d);
    const int64_t gs = s < kGrid4d ? fc4s : fc2s;
    const double *ms = meanstd + (size_t)(e / ncs) * 2 * kMeanStd;
    const int l = lidx[e];
    const double mean = ms[l], stdv = ms[kMeanStd + l];
    double *out = model + e;
    for (int t0 = 0; t0 < T; t0 += kTileMem) {
        double v[kTileMem];
#pragma unroll
        for (int k = 0; k < kTileMem; ++k)
            if (t0 + k < T) v[k] = g[(size_t)(t0 + k) * gs];
#pragma unroll
        for (int k = 0; k < kTileMem; ++k)
            if (t0 + k < T) {
                const double t = v[k] - mean;
                out[(size_t)(t0 + k) * model_stride] = t / stdv;
            }
    }
}

}  // namespace
