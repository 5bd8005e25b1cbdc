// sml_slab_series.hpp -- the slab ocean reservoirs' training inputs from a series of global
// grids (sml_slab_train_series): column t of slab feedback entry e is
//     a_t[e] = (z_lo[e] + z_lo+1[e] + ... + z_t[e]) / d,   lo = max(0, t - window + 1),
// z_k[e] the standardised atmo feedback entry ring_src[e] of step k -- sml_res_tile_series's
// value, t = x - mean; t / std -- summed from 0.0 in ascending step order, one add a term,
// then one division; d = the number of terms while t + 1 < window, `divisor` afterwards
// (rolling_average_over_a_period_2d, mod_utilities.f90:1766-1804, is (window, divisor) =
// (P + 1, P); the loop's ring at prediction is (P, P)).
//
// A thread owns one entry over one chunk of kSlabSerChunk columns (chunk c: columns
// [c * kSlabSerChunk, (c + 1) * kSlabSerChunk) of the series, cut to the call's range).  It
// reads its table entry and its mean / std once and standardises each step it needs once
// (window - 1 steps of history, then the chunk's) into a ring of its own in LDS: step k at
// [(k % cap) * blockDim.x + lane], cap = window + kSlabSerTile - 1.  The columns are served
// kSlabSerTile at a time: the tile's steps are loaded together and written to the ring,
// then the ring is walked once in step order, each value added to the sums of the tile's
// columns whose window holds it -- every column's sum still runs from 0.0 over its own
// steps in ascending order, one add a term (a running add / subtract is not the defined
// value); the tile's sums are independent chains, and a ring value is read once for all of
// them.  Which columns hold step k is the same for every lane, so the tests are scalar.
// The block is as many lanes as keep the ring within kSlabSerLds (slab_series_threads: 64
// up to window 121, 32 up to 249, 16 up to 505, 8 up to 1017, 4 up to the largest window,
// 1024): no window takes another path.  Nothing is shared between threads, no block waits
// for another, no atomics: a column's bits depend on the series alone, not on the range,
// the stream or the CUs.  The unit is built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "sml_internal.hpp"
#include "sml_reservoir_layout.hpp"

namespace {
using namespace sml;

constexpr int kSlabSerChunk = 64;   // columns a thread serves: a constant, so the split depends on (t0, ncols) alone
constexpr int kSlabSerTile = 8;     // columns summed together; steps whose gathers one thread issues together
constexpr int kSlabSerLds = 65536;  // the ring's bytes a block: the LDS a launch gets without asking for more
constexpr int kSlabSerWindowMax = 1024;

// lanes of a block: the largest power of two up to a wave whose rings fit kSlabSerLds
inline int slab_series_threads(int window) {
    const int cap = window + kSlabSerTile - 1;
    int bt = 64;
    while (bt > 1 && (size_t)cap * bt * sizeof(double) > (size_t)kSlabSerLds) bt /= 2;
    return bt;
}
static_assert((kSlabSerWindowMax + kSlabSerTile - 1) * 4 * sizeof(double) <= kSlabSerLds, "the largest window's ring fits");

// the series' pointers: step t of the 4-d grid at g4 + t * g4s, of a 2-d field at its pointer
// + t * g2s (NULL: the field is absent).  The kernel takes the members as arguments of
// their own: a lane selects its field by value, and a selection among the members of one
// by-value argument becomes an indexed load of a copy in scratch.
struct SlabSeriesIn {
    const double *g4, *logp, *precip, *sst, *tisr;
    int64_t g4s, g2s;
};

// the entry's source: its pointer at step 0 (NULL: an absent field, whose z is 0) and stride
struct SlabSerSrc {
    const double *g;
    int64_t gs;
};
__device__ __forceinline__ SlabSerSrc slab_ser_src(const double *g4, const double *logp, const double *precip,
                                                   const double *sst, const double *tisr, int64_t g4s, int64_t g2s,
                                                   int s) {
    if (s < kGrid4d) return {g4 + s, g4s};
    const int f = (s - kGrid4d) / kGrid2d;
    const double *b = f == kSerLogp ? logp : f == kSerPrecip ? precip : f == kSerSst ? sst : tisr;
    return {b ? b + (s - kGrid4d - f * kGrid2d) : nullptr, g2s};
}

// grid (ceil(tot / blockDim.x), chunks): blockIdx.y + c_first is the chunk.  Dynamic LDS:
// (window + kSlabSerTile - 1) * blockDim.x doubles.
__global__ __launch_bounds__(64) void k_slab_series(
    const int32_t *__restrict__ src, const uint8_t *__restrict__ lidx, const uint16_t *__restrict__ row,
    const double *__restrict__ meanstd, const double *__restrict__ g4, const double *__restrict__ logp,
    const double *__restrict__ precip, const double *__restrict__ sst, const double *__restrict__ tisr, int64_t g4s,
    int64_t g2s, int tot, int window, int divisor, int t0, int t1, int c_first, double *__restrict__ out,
    int64_t out_stride) {
    extern __shared__ __attribute__((aligned(16))) double ring[];
    const int bt = blockDim.x;
    const int e = blockIdx.x * bt + threadIdx.x;
    if (e >= tot) return;
    const SlabSerSrc sp = slab_ser_src(g4, logp, precip, sst, tisr, g4s, g2s, src[e]);
    const double *ms = meanstd + (size_t)row[e] * 2 * kMeanStd;
    const int l = lidx[e];
    const double mean = ms[l], stdv = ms[kMeanStd + l];
    const int c = c_first + blockIdx.y;
    const int a0 = max(t0, c * kSlabSerChunk), a1 = min(t1, (c + 1) * kSlabSerChunk);  // this thread's columns
    const int cap = window + kSlabSerTile - 1;
    double *mine = ring + threadIdx.x;
    const int p0 = max(0, a0 - window + 1);
    int wslot = p0 % cap;  // the slot of the next step written: step k at k % cap
    int lo_step = p0, lo_slot = wslot;  // the oldest step the next tile reads, and its slot
    for (int a = p0; a < a0; a += kSlabSerTile) {  // the history: steps [p0, a0)
        double v[kSlabSerTile];
#pragma unroll
        for (int k = 0; k < kSlabSerTile; ++k)
            if (a + k < a0) v[k] = sp.g ? sp.g[(size_t)(a + k) * sp.gs] : 0.0;
#pragma unroll
        for (int k = 0; k < kSlabSerTile; ++k)
            if (a + k < a0) {
                const double d = v[k] - mean;
                mine[wslot * bt] = sp.g ? d / stdv : 0.0;
                wslot = wslot + 1 == cap ? 0 : wslot + 1;
            }
    }
    double *o = out + e;
    for (int a = a0; a < a1; a += kSlabSerTile) {
        const int nc = min(kSlabSerTile, a1 - a);  // the tile's columns a .. a + nc - 1
        double v[kSlabSerTile];
#pragma unroll
        for (int k = 0; k < kSlabSerTile; ++k)
            if (k < nc) v[k] = sp.g ? sp.g[(size_t)(a + k) * sp.gs] : 0.0;
#pragma unroll
        for (int k = 0; k < kSlabSerTile; ++k)
            if (k < nc) {
                const double d = v[k] - mean;
                mine[wslot * bt] = sp.g ? d / stdv : 0.0;
                wslot = wslot + 1 == cap ? 0 : wslot + 1;
            }
        // column a + i sums steps max(0, a + i - window + 1) .. a + i; the walk covers the union
        const int first = max(0, a - window + 1);
        lo_slot += first - lo_step;  // (at most kSlabSerTile further on)
        if (lo_slot >= cap) lo_slot -= cap;
        lo_step = first;
        const int all_lo = max(0, a + nc - window), all_hi = a;  // steps every column of the tile holds
        double s[kSlabSerTile];
#pragma unroll
        for (int i = 0; i < kSlabSerTile; ++i) s[i] = 0.0;
        int k = first, r = lo_slot;
        const int last = a + nc - 1;
        auto some = [&](int kk, double z) {  // the columns whose window holds step kk: the same for every lane
#pragma unroll
            for (int i = 0; i < kSlabSerTile; ++i)
                if (i < nc && kk <= a + i && kk >= a + i - window + 1) s[i] = s[i] + z;
        };
        for (; k <= last && k < all_lo; ++k) {
            some(k, mine[r * bt]);
            r = r + 1 == cap ? 0 : r + 1;
        }
        if (nc == kSlabSerTile)
            for (; k <= all_hi; ++k) {
                const double z = mine[r * bt];
#pragma unroll
                for (int i = 0; i < kSlabSerTile; ++i) s[i] = s[i] + z;
                r = r + 1 == cap ? 0 : r + 1;
            }
        for (; k <= last; ++k) {
            some(k, mine[r * bt]);
            r = r + 1 == cap ? 0 : r + 1;
        }
#pragma unroll
        for (int i = 0; i < kSlabSerTile; ++i)
            if (i < nc) {
                const int t = a + i;
                o[(size_t)(t - t0) * out_stride] = s[i] / (double)(t + 1 < window ? t + 1 : divisor);
            }
    }
}

// columns [t0, t1) of the series; tot > 0, t1 > t0 (the caller has checked every argument)
inline void launch_slab_series(const int32_t *src, const uint8_t *lidx, const uint16_t *row, const double *meanstd,
                               const SlabSeriesIn &in, int tot, int window, int divisor, int t0, int t1, double *out,
                               int64_t out_stride, hipStream_t st) {
    const int c_last = (t1 - 1) / kSlabSerChunk;
    const int bt = slab_series_threads(window);
    const size_t lds = (size_t)(window + kSlabSerTile - 1) * bt * sizeof(double);
    constexpr int kGridY = 65535;  // the launch's limit on gridDim.y: longer ranges take several launches
    for (int c_first = t0 / kSlabSerChunk; c_first <= c_last; c_first += kGridY) {
        const dim3 grid((tot + bt - 1) / bt, std::min(kGridY, c_last - c_first + 1));
        hipLaunchKernelGGL(k_slab_series, grid, dim3(bt), lds, st, src, lidx, row, meanstd, in.g4, in.logp, in.precip,
                           in.sst, in.tisr, in.g4s, in.g2s, tot, window, divisor, t0, t1, c_first, out, out_stride);
    }
}

}  // namespace
