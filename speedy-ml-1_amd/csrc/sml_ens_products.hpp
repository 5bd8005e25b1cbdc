// sml_ens_products.hpp -- the ensemble products' kernels: per-point mean and spread of the E
// members' assembled grids, and the area-weighted scores of a step against a verifying
// analysis (rmse of the mean, spread, fair CRPS, bias, rank histogram) for each of the 34
// fields.  The only kernels of the library that reduce over the member dimension.
//
// Member e's part of every input starts e * stride doubles into it.  A thread owns one
// (k, j, i) quad of the 4-d grid (32 bytes, read as 16-byte loads) or one point of a 2-d
// grid, and issues the members' loads a tile of kEnsTile members at a time, as the slab
// stages do (sml_slab.hpp).  Per point, in member order:
//   s = x_0; s = s + x_e;  mean = s / E
//   q = 0;   d = x_e - mean; q = q + d * d;  var = q / (E - 1)  (q itself at E = 1: 0)
// -- the same two functions (ens_mean, ens_var) in both kernels.  The unit is built with
// -ffp-contract=off: no product is fused into a sum.
//
// The scores are sums over the 4608 points of a field in a fixed order that depends on
// nothing but the block shape: k_ens_rows, one block per (level, latitude row), reduces its
// 96 points by a lane tree (shuffles), the two waves' partials through LDS, and stores row
// partials; k_ens_fields, one block per field in a launch behind it, adds the 48 row
// partials in row order.  No floating-point atomics, no waits, nothing shared between
// blocks but the row partials across the launch boundary; the rank counts use LDS integer
// atomics inside a block and plain stores.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sml_ens_layout.hpp"
#include "sml_internal.hpp"

namespace {
using namespace sml;

constexpr int kEnsTile = 4;           // members whose loads one thread issues together
constexpr int kEnsRowThreads = 128;   // k_ens_rows: two waves, 96 lanes own a point of the row
constexpr int kEnsMomentThreads = 64;
constexpr int kEnsRows4d = kZGrid * kYGrid;  // 384 (level, row) blocks, then 48 of logp, 48 of precip
constexpr int kEnsQuadBlocks = kGrid4d / kVars / kEnsMomentThreads;  // 576
constexpr int kEnsPointBlocks = kGrid2d / kEnsMomentThreads;         // 72

template <int NV>
__device__ __forceinline__ void ens_load(const double *__restrict__ p, double (&v)[NV]) {
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
__device__ __forceinline__ void ens_store(double *__restrict__ p, const double (&v)[NV]) {
    if constexpr (NV == 1) {
        *p = v[0];
    } else {
#pragma unroll
        for (int c = 0; c < NV; c += 2) *reinterpret_cast<double2 *>(p + c) = make_double2(v[c], v[c + 1]);
    }
}

__device__ __forceinline__ double ens_mean(double s, int E) { return s / (double)E; }
__device__ __forceinline__ double ens_var(double q, int E) { return E > 1 ? q / (double)(E - 1) : q; }

// mean and spread of NV neighbouring values per member; x: member 0's
template <int NV>
__device__ __forceinline__ void ens_moments_point(const double *__restrict__ x, int64_t stride, int E,
                                                  double *__restrict__ mean_out, double *__restrict__ spread_out) {
    double s[NV], mean[NV], q[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) s[c] = q[c] = 0.0;
    for (int e0 = 0; e0 < E; e0 += kEnsTile) {
        double v[kEnsTile][NV];
#pragma unroll
        for (int k = 0; k < kEnsTile; ++k)
            if (e0 + k < E) ens_load<NV>(x + (size_t)(e0 + k) * stride, v[k]);
#pragma unroll
        for (int k = 0; k < kEnsTile; ++k)
            if (e0 + k < E) {
#pragma unroll
                for (int c = 0; c < NV; ++c) s[c] = e0 + k == 0 ? v[k][c] : s[c] + v[k][c];
            }
    }
#pragma unroll
    for (int c = 0; c < NV; ++c) mean[c] = ens_mean(s[c], E);
    if (mean_out) ens_store<NV>(mean_out, mean);
    if (!spread_out) return;
    for (int e0 = 0; e0 < E; e0 += kEnsTile) {
        double v[kEnsTile][NV];
#pragma unroll
        for (int k = 0; k < kEnsTile; ++k)
            if (e0 + k < E) ens_load<NV>(x + (size_t)(e0 + k) * stride, v[k]);
#pragma unroll
        for (int k = 0; k < kEnsTile; ++k)
            if (e0 + k < E) {
#pragma unroll
                for (int c = 0; c < NV; ++c) {
                    const double d = v[k][c] - mean[c];
                    q[c] = q[c] + d * d;
                }
            }
    }
    double sp[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) sp[c] = sqrt(ens_var(q[c], E));
    ens_store<NV>(spread_out, sp);
}

// blocks [0, 576): the quads of the 4-d grid; [576, 648): logp; [648, 720): precip
__global__ __launch_bounds__(kEnsMomentThreads) void k_ens_moments(
    const double *__restrict__ g4, int64_t g4_stride, const double *__restrict__ g2, const double *__restrict__ pr,
    int64_t g2_stride, double *__restrict__ mean4, double *__restrict__ mean2, double *__restrict__ meanpr,
    double *__restrict__ spread4, double *__restrict__ spread2, double *__restrict__ spreadpr, int E) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b < kEnsQuadBlocks) {
        if (!mean4 && !spread4) return;
        const size_t o = (size_t)(b * kEnsMomentThreads + tid) * kVars;
        ens_moments_point<kVars>(g4 + o, g4_stride, E, mean4 ? mean4 + o : nullptr, spread4 ? spread4 + o : nullptr);
    } else if (b < kEnsQuadBlocks + kEnsPointBlocks) {
        if (!mean2 && !spread2) return;
        const size_t o = (size_t)(b - kEnsQuadBlocks) * kEnsMomentThreads + tid;
        ens_moments_point<1>(g2 + o, g2_stride, E, mean2 ? mean2 + o : nullptr, spread2 ? spread2 + o : nullptr);
    } else {
        if (!pr || (!meanpr && !spreadpr)) return;
        const size_t o = (size_t)(b - kEnsQuadBlocks - kEnsPointBlocks) * kEnsMomentThreads + tid;
        ens_moments_point<1>(pr + o, g2_stride, E, meanpr ? meanpr + o : nullptr, spreadpr ? spreadpr + o : nullptr);
    }
}

// One row of 96 points, NV neighbouring fields per point: the four weighted row sums of
// each field into part[f][j][4] and, with a truth, its rank counts into rpart[f][j][33].
// x / y: member 0's and the truth's values of this thread's point (y NULL: no truth);
// xs: the thread's own column of the members' values, [E][96 * NV] in LDS.
template <int NV>
__device__ __forceinline__ void ens_row(const double *__restrict__ x, int64_t stride, const double *__restrict__ y,
                                        double w, int E, int f0, int j, double *__restrict__ xs,
                                        double (*red)[2][kEnsScores], int (*hist)[kEnsRankBins],
                                        double *__restrict__ part, int32_t *__restrict__ rpart) {
    const int tid = threadIdx.x;
    const bool act = tid < kXGrid;
    if (tid < NV * kEnsRankBins) hist[tid / kEnsRankBins][tid % kEnsRankBins] = 0;
    __syncthreads();
    double term[NV][kEnsScores];
#pragma unroll
    for (int c = 0; c < NV; ++c)
#pragma unroll
        for (int sc = 0; sc < kEnsScores; ++sc) term[c][sc] = 0.0;
    if (act) {
        double *col = xs + tid * NV;
        double s[NV], mean[NV], q[NV], a[NV], p[NV], yv[NV];
        int r[NV];
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            s[c] = q[c] = a[c] = p[c] = yv[c] = 0.0;
            r[c] = 0;
        }
        if (y) ens_load<NV>(y, yv);
        for (int e0 = 0; e0 < E; e0 += kEnsTile) {
            double v[kEnsTile][NV];
#pragma unroll
            for (int k = 0; k < kEnsTile; ++k)
                if (e0 + k < E) ens_load<NV>(x + (size_t)(e0 + k) * stride, v[k]);
#pragma unroll
            for (int k = 0; k < kEnsTile; ++k)
                if (e0 + k < E) {
                    ens_store<NV>(col + (e0 + k) * (kXGrid * NV), v[k]);
#pragma unroll
                    for (int c = 0; c < NV; ++c) s[c] = e0 + k == 0 ? v[k][c] : s[c] + v[k][c];
                }
        }
#pragma unroll
        for (int c = 0; c < NV; ++c) mean[c] = ens_mean(s[c], E);
        for (int e = 0; e < E; ++e) {
            double v[NV];
            ens_load<NV>(col + e * (kXGrid * NV), v);
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                const double d = v[c] - mean[c];
                q[c] = q[c] + d * d;
                a[c] = a[c] + fabs(v[c] - yv[c]);
                r[c] += v[c] < yv[c] ? 1 : 0;
            }
        }
        if (y) {  // the fair CRPS's pair term over e < f, doubled below
            for (int e = 0; e + 1 < E; ++e) {
                double v[NV];
                ens_load<NV>(col + e * (kXGrid * NV), v);
                for (int f = e + 1; f < E; ++f) {
                    double u[NV];
                    ens_load<NV>(col + f * (kXGrid * NV), u);
#pragma unroll
                    for (int c = 0; c < NV; ++c) p[c] = p[c] + fabs(v[c] - u[c]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            term[c][kEnsSpread] = w * ens_var(q[c], E);
            if (y) {
                const double dm = mean[c] - yv[c];
                const double pair = E > 1 ? (p[c] + p[c]) / (double)(2 * E * (E - 1)) : 0.0;
                term[c][kEnsRmse] = w * (dm * dm);
                term[c][kEnsCrps] = w * (a[c] / (double)E - pair);
                term[c][kEnsBias] = w * dm;
                atomicAdd(&hist[c][r[c]], 1);
            }
        }
    }
    // the lane tree: lane l takes lane l + 32, 16, .., 1 (the idle lanes of the second wave hold 0)
#pragma unroll
    for (int c = 0; c < NV; ++c)
#pragma unroll
        for (int sc = 0; sc < kEnsScores; ++sc) {
            double v = term[c][sc];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off);
            if ((tid & 63) == 0) red[tid >> 6][c][sc] = v;
        }
    __syncthreads();
    if (tid < NV * kEnsScores) {
        const int c = tid / kEnsScores, sc = tid % kEnsScores;
        part[((size_t)(f0 + c) * kYGrid + j) * kEnsScores + sc] = red[0][c][sc] + red[1][c][sc];
    }
    if (y && tid < NV * kEnsRankBins) {
        const int c = tid / kEnsRankBins, b = tid % kEnsRankBins;
        rpart[((size_t)(f0 + c) * kYGrid + j) * kEnsRankBins + b] = hist[c][b];
    }
    __syncthreads();
}

// blocks [0, 384): row j of level k of the 4-d grid, its quads in two halves of two fields;
// [384, 432): logp's rows; [432, 480): precip's
__global__ __launch_bounds__(kEnsRowThreads) void k_ens_rows(
    const double *__restrict__ g4, int64_t g4_stride, const double *__restrict__ g2, const double *__restrict__ pr,
    int64_t g2_stride, const double *__restrict__ t4, const double *__restrict__ t2, const double *__restrict__ tpr,
    const double *__restrict__ w48, int E, double *__restrict__ part, int32_t *__restrict__ rpart) {
    __shared__ __attribute__((aligned(16))) double xs[SML_RES_MAX_MEMBERS * kXGrid * 2];
    __shared__ double red[2][2][kEnsScores];
    __shared__ int hist[2][kEnsRankBins];
    const int b = blockIdx.x;
    const int tid = threadIdx.x < kXGrid ? threadIdx.x : 0;  // (the idle lanes form no address of their own)
    if (b < kEnsRows4d) {
        const int j = b % kYGrid;
        const double w = w48[j];
        for (int h = 0; h < 2; ++h) {
            const size_t o = ((size_t)b * kXGrid + tid) * kVars + 2 * h;
            ens_row<2>(g4 + o, g4_stride, t4 ? t4 + o : nullptr, w, E, (b / kYGrid) * kVars + 2 * h, j, xs, red, hist,
                       part, rpart);
        }
    } else if (b < kEnsRows4d + kYGrid) {
        const int j = b - kEnsRows4d;
        const size_t o = (size_t)j * kXGrid + tid;
        ens_row<1>(g2 + o, g2_stride, t2 ? t2 + o : nullptr, w48[j], E, kVars * kZGrid, j, xs, red, hist, part, rpart);
    } else {
        if (!pr) return;
        const int j = b - kEnsRows4d - kYGrid;
        const size_t o = (size_t)j * kXGrid + tid;
        ens_row<1>(pr + o, g2_stride, tpr ? tpr + o : nullptr, w48[j], E, kVars * kZGrid + 1, j, xs, red, hist, part,
                   rpart);
    }
}

// field f's row of the tables from its 48 row partials, added in row order; without a
// truth only the spread is written, and field 33 not at all without the members' precip
__global__ __launch_bounds__(64) void k_ens_fields(const double *__restrict__ part, const int32_t *__restrict__ rpart,
                                                   bool truth, bool has_pr, bool truth_pr,
                                                   double *__restrict__ scores, int32_t *__restrict__ ranks) {
    const int f = blockIdx.x, tid = threadIdx.x;
    if (f == kEnsFields - 1 && !has_pr) return;
    const bool tr = f == kEnsFields - 1 ? truth_pr : truth;
    if (tid < kEnsScores && (tr || tid == kEnsSpread)) {
        const double *p = part + (size_t)f * kYGrid * kEnsScores + tid;
        double s = p[0];
        for (int j = 1; j < kYGrid; ++j) s = s + p[j * kEnsScores];
        if (tid == kEnsRmse || tid == kEnsSpread) s = sqrt(s);
        scores[f * kEnsScores + tid] = s;
    }
    if (tr && tid < kEnsRankBins) {
        const int32_t *p = rpart + (size_t)f * kYGrid * kEnsRankBins + tid;
        int32_t n = 0;
        for (int j = 0; j < kYGrid; ++j) n += p[j * kEnsRankBins];
        ranks[f * kEnsRankBins + tid] = n;
    }
}

// sml_ens_reset: quiet NaN in every score, 0 in every rank bin
__global__ void k_ens_reset(double *__restrict__ scores, int64_t nscores, int32_t *__restrict__ ranks, int64_t nranks) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nscores) scores[i] = __longlong_as_double(0x7ff8000000000000LL);
    if (i < nranks) ranks[i] = 0;
}

// ---- the launches (each checks nothing: the callers have checked pointers and strides)
inline void launch_ens_moments(const double *g4, int64_t g4_stride, const double *g2, const double *pr,
                               int64_t g2_stride, double *mean4, double *mean2, double *meanpr, double *spread4,
                               double *spread2, double *spreadpr, int E, hipStream_t st) {
    hipLaunchKernelGGL(k_ens_moments, dim3(kEnsQuadBlocks + 2 * kEnsPointBlocks), dim3(kEnsMomentThreads), 0, st, g4,
                       g4_stride, g2, pr, g2_stride, mean4, mean2, meanpr, spread4, spread2, spreadpr, E);
}
inline void launch_ens_rows(const double *g4, int64_t g4_stride, const double *g2, const double *pr, int64_t g2_stride,
                            const double *t4, const double *t2, const double *tpr, const double *w48, int E,
                            double *part, int32_t *rpart, hipStream_t st) {
    hipLaunchKernelGGL(k_ens_rows, dim3(kEnsRows4d + 2 * kYGrid), dim3(kEnsRowThreads), 0, st, g4, g4_stride, g2, pr,
                       g2_stride, t4, t2, tpr, w48, E, part, rpart);
}
inline void launch_ens_fields(const double *part, const int32_t *rpart, bool truth, bool has_pr, bool truth_pr,
                              double *scores, int32_t *ranks, hipStream_t st) {
    hipLaunchKernelGGL(k_ens_fields, dim3(kEnsFields), dim3(64), 0, st, part, rpart, truth, has_pr, truth_pr, scores,
                       ranks);
}
inline void launch_ens_reset(double *scores, int64_t nscores, int32_t *ranks, int64_t nranks, hipStream_t st) {
    const int64_t n = nscores > nranks ? nscores : nranks;
    hipLaunchKernelGGL(k_ens_reset, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, scores, nscores, ranks, nranks);
}

}  // namespace
