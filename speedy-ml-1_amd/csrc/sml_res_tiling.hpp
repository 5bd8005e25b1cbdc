// sml_res_tiling.hpp -- the device-side exchange: the regions' outvecs into the global
// grids with the root's clips (assemble_one, k_assemble), and the grids back into each
// region's feedback, tisr entries and local-model vector, standardized (k_tile_*).
// (A timeline build, SML_TL, needs the unit's SML_TL_DEFINE ahead of this header.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sml_internal.hpp"
#include "sml_reservoir_layout.hpp"
#include "sml_timeline.hpp"

namespace {
using namespace sml;

// one output into the global grids with the root's clips (k_assemble, and the finish
// that assembles in its own launch: k_res_finish_grid<kAsm>)
__device__ inline void assemble_one(int d, double v, double *__restrict__ g4, double *__restrict__ g2,
                                    double *__restrict__ pr) {
    if (d < 0) return;
    if (d < kGrid4d) {
        if ((d & 3) == 3 && v < 0.000001) v = 0.000001;  // mpires.f90:448-450
        g4[d] = v;
    } else if (d < kGrid4d + kGrid2d) {
        g2[d - kGrid4d] = v;
    } else {
        if (v < 0.00001) v = 0.0;  // mpires.f90:474-478
        pr[d - kGrid4d - kGrid2d] = v;
    }
}

// assemble: all regions' outvecs -> global grids, with the root's clips
__global__ void k_assemble(const int32_t *__restrict__ dst, const double *__restrict__ ov, double *__restrict__ g4,
                           double *__restrict__ g2, double *__restrict__ pr, int total, int nout, int ov_ld) {
    SML_TL_SCOPE(sml::tl::kAssemble);
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int d = dst[e];
    if (d < 0) return;
    assemble_one(d, ov_ld == nout ? ov[e] : ov[(size_t)(e / nout) * ov_ld + e % nout], g4, g2, pr);
}

__device__ inline double grid_at(int src, const double *g4, const double *g2, const double *pr) {
    if (src < kGrid4d) return g4[src];
    if (src < kGrid4d + kGrid2d) return g2[src - kGrid4d];
    return pr[src - kGrid4d - kGrid2d];
}

// tile feedback: overlap tiles of the global grids, standardized (x-mean)/std
__global__ void k_tile_feedback(const int32_t *__restrict__ src, const uint8_t *__restrict__ lidx,
                                const uint16_t *__restrict__ reg, const double *__restrict__ meanstd,
                                const double *__restrict__ g4, const double *__restrict__ g2,
                                const double *__restrict__ pr, const double *__restrict__ tisr,
                                double *__restrict__ feedback, int total) {
    SML_TL_SCOPE(sml::tl::kTileFeedback);
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int s = src[e];
    if (s == kSrcKeep) return;
    if (s < kSrcKeep) {  // tisr entry: -2 - packed index
        if (tisr) feedback[e] = tisr[-2 - s];
        return;
    }
    const double *ms = meanstd + (size_t)reg[e] * 2 * kMeanStd;
    const int l = lidx[e];
    const double t = grid_at(s, g4, g2, pr) - ms[l];
    feedback[e] = t / ms[kMeanStd + l];
}

// tisr entries from one hour's global tisr field (96, 48): get_tisr_by_date's
// full_tisr(:, :, hour) of the region's overlap tile (read_3d_file_parallel over the
// input extent), standardized with the region's tisr mean / std (l = 34,
// get_full_tisr, mod_reservoir.f90:888-906)
__global__ void k_tile_tisr(const int32_t *__restrict__ fbi, const int32_t *__restrict__ gi,
                            const uint16_t *__restrict__ reg, const double *__restrict__ meanstd,
                            const double *__restrict__ G, double *__restrict__ feedback, int total) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const double *ms = meanstd + (size_t)reg[e] * 2 * kMeanStd;
    const double t = G[gi[e]] - ms[33];
    feedback[fbi[e]] = t / ms[kMeanStd + 33];
}

// ---- the two feedback tilings for the E members of an ensemble, one launch each: member
// e's grids, precipitation and feedback start e * g4s / g2s / fbs doubles into their
// arrays.  A thread reads its table entries and its mean / std once and serves every
// member with them, kTileMem members' gathers in flight together; per member the two
// operations are k_tile_feedback's / k_tile_tisr's.
constexpr int kTileMem = 4;

__global__ void k_tile_feedback_mem(const int32_t *__restrict__ src, const uint8_t *__restrict__ lidx,
                                    const uint16_t *__restrict__ reg, const double *__restrict__ meanstd,
                                    const double *__restrict__ g4, const double *__restrict__ g2,
                                    const double *__restrict__ pr, const double *__restrict__ tisr,
                                    double *__restrict__ feedback, int total, int E, int64_t g4s, int64_t g2s,
                                    int64_t fbs) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int s = src[e];
    if (s == kSrcKeep) return;
    if (s < kSrcKeep) {  // tisr entry: -2 - packed index; the vector is the members' common one
        if (tisr) {
            const double v = tisr[-2 - s];
            for (int m = 0; m < E; ++m) feedback[(size_t)m * fbs + e] = v;
        }
        return;
    }
    const double *ms = meanstd + (size_t)reg[e] * 2 * kMeanStd;
    const int l = lidx[e];
    const double mean = ms[l], stdv = ms[kMeanStd + l];
    // which grid, and where in it: the same for every member
    const double *g = s < kGrid4d ? g4 : s < kGrid4d + kGrid2d ? g2 : pr;
    const int64_t gs = s < kGrid4d ? g4s : g2s;
    const int at = s < kGrid4d ? s : s < kGrid4d + kGrid2d ? s - kGrid4d : s - kGrid4d - kGrid2d;
    for (int m0 = 0; m0 < E; m0 += kTileMem) {
        double v[kTileMem];
#pragma unroll
        for (int k = 0; k < kTileMem; ++k)
            if (m0 + k < E) v[k] = g[(size_t)(m0 + k) * gs + at];
#pragma unroll
        for (int k = 0; k < kTileMem; ++k)
            if (m0 + k < E) {
                const double t = v[k] - mean;
                feedback[(size_t)(m0 + k) * fbs + e] = t / stdv;
            }
    }
}

// one hour's tisr field into the E feedbacks (the members share the date)
__global__ void k_tile_tisr_mem(const int32_t *__restrict__ fbi, const int32_t *__restrict__ gi,
                                const uint16_t *__restrict__ reg, const double *__restrict__ meanstd,
                                const double *__restrict__ G, double *__restrict__ feedback, int total, int E,
                                int64_t fbs) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const double *ms = meanstd + (size_t)reg[e] * 2 * kMeanStd;
    const double t = G[gi[e]] - ms[33];
    const double v = t / ms[kMeanStd + 33];
    const int d = fbi[e];
    for (int m = 0; m < E; ++m) feedback[(size_t)m * fbs + d] = v;
}

// tile local_model: SPEEDY forecast at the region's own points, standardized
__global__ void k_tile_local_model(const int32_t *__restrict__ src, const uint8_t *__restrict__ lidx,
                                   const double *__restrict__ meanstd, const double *__restrict__ fc4,
                                   const double *__restrict__ fc2, double *__restrict__ lm, int ncs, int total) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int s = src[e];
    const double v = s < kGrid4d ? fc4[s] : fc2[s - kGrid4d];
    const double *ms = meanstd + (size_t)(e / ncs) * 2 * kMeanStd;
    const int l = lidx[e];
    const double t = v - ms[l];
    lm[e] = t / ms[kMeanStd + l];
}

}  // namespace
