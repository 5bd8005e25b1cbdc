// sml_slab.hpp -- the slab ocean's stage kernels (sendrecievegrid's sst half,
// mpires.f90:288-478, 575-767) with a member dimension: each stage is one launch for the E
// members of an ensemble.  Member e's part of every array starts e * stride doubles into
// it (the hosts check each stride against the packed size).  A thread reads its table
// entries once and serves every member with them, a tile of kSlabTile members at a time:
// the tile's loads are independent, so they are in flight together.  The arithmetic per
// member is the single-member loop's, operation for operation; that loop runs these
// kernels at E = 1 (through sml_slab.hip).  Plain vector loads and stores only: no block waits
// for another, and nothing is shared between threads.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sml_internal.hpp"

namespace {
using namespace sml;

constexpr int kSlabTile = 4;  // members whose loads one thread issues together

// the slab feedback: the mean of the ring of the last timestep_slab/timestep - 1 atmo
// feedback subsets, summed column by column as Fortran's sum(.., dim=2) (mpires.f90:757),
// then one division.  ring [E][ncol][tot], fb [E][tot]
__global__ void k_slab_avg(const double *__restrict__ ring, int64_t ring_stride, int ncol, int tot,
                           double *__restrict__ fb, int64_t fb_stride, int E) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= tot) return;
    for (int e0 = 0; e0 < E; e0 += kSlabTile) {
        double s[kSlabTile];
#pragma unroll
        for (int k = 0; k < kSlabTile; ++k) s[k] = 0.0;
        for (int c = 0; c < ncol; ++c) {
#pragma unroll
            for (int k = 0; k < kSlabTile; ++k)
                if (e0 + k < E) s[k] = s[k] + ring[(size_t)(e0 + k) * ring_stride + (size_t)c * tot + i];
        }
#pragma unroll
        for (int k = 0; k < kSlabTile; ++k)
            if (e0 + k < E) fb[(size_t)(e0 + k) * fb_stride + i] = s[k] / (double)ncol;
    }
}

// averaged_atmo_input_vec(:, col) = the atmo feedback at atmo_training_data_idx
// (mpires.f90:755; the index list of trained_ocean_reservoir_prediction,
// mod_slab_ocean_reservoir.f90:1550-1563).  fb [E][>= tot_fb], col: the ring's column of member 0
__global__ void k_slab_ring(const double *__restrict__ fb, int64_t fb_stride, const int32_t *__restrict__ src, int tot,
                            double *__restrict__ col, int64_t ring_stride, int E) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= tot) return;
    const int s = src[i];
    for (int e0 = 0; e0 < E; e0 += kSlabTile) {
        double v[kSlabTile];
#pragma unroll
        for (int k = 0; k < kSlabTile; ++k)
            if (e0 + k < E) v[k] = fb[(size_t)(e0 + k) * fb_stride + s];
#pragma unroll
        for (int k = 0; k < kSlabTile; ++k)
            if (e0 + k < E) col[(size_t)(e0 + k) * ring_stride + i] = v[k];
    }
}

// the sst columns of the exchange rows: 272 for a region without a slab prediction
// (mpires.f90:366-372), the slab outvec otherwise.  slab_ov [E][nslab][nsst], ov [E][nlocal][xw]
__global__ void k_slab_rows(const double *__restrict__ slab_ov, int64_t sov_stride, const int32_t *__restrict__ row,
                            int nslab, int nsst, int nlocal, int nout, int xw, bool fill, double *__restrict__ ov,
                            int64_t ov_stride, int E) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (fill) {
        if (i >= nlocal * nsst) return;
        const size_t d = (size_t)(i / nsst) * xw + nout + i % nsst;
        for (int e = 0; e < E; ++e) ov[(size_t)e * ov_stride + d] = 272.0;
        return;
    }
    if (i >= nslab * nsst) return;
    const size_t d = (size_t)row[i / nsst] * xw + nout + i % nsst;
    for (int e0 = 0; e0 < E; e0 += kSlabTile) {
        double v[kSlabTile];
#pragma unroll
        for (int k = 0; k < kSlabTile; ++k)
            if (e0 + k < E) v[k] = slab_ov[(size_t)(e0 + k) * sov_stride + i];
#pragma unroll
        for (int k = 0; k < kSlabTile; ++k)
            if (e0 + k < E) ov[(size_t)(e0 + k) * ov_stride + d] = v[k];
    }
}

// wholegrid_sst from every region's sst columns (tile_full_2d_grid_with_local_res,
// res_domain.f90), land / permanent ice to base_sst_grid, floor 272 K
// (mpires.f90:458-472; train_on_sst_anomalies off).  ov_all [E][numregions][xw], sst [E][96 * 48]
__global__ void k_sst_grid(const double *__restrict__ ov_all, int64_t ov_stride, const int32_t *__restrict__ src,
                           const double *__restrict__ base, const double *__restrict__ mask, double *__restrict__ sst,
                           int64_t sst_stride, int E) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= kGrid2d) return;
    const int s = src[p];
    const bool land = mask[p] > 0.0;
    const double b = base[p];
    for (int e0 = 0; e0 < E; e0 += kSlabTile) {
        double v[kSlabTile];
#pragma unroll
        for (int k = 0; k < kSlabTile; ++k)
            if (e0 + k < E) v[k] = ov_all[(size_t)(e0 + k) * ov_stride + s];
#pragma unroll
        for (int k = 0; k < kSlabTile; ++k)
            if (e0 + k < E) {
                double w = v[k];
                if (land) w = b;
                if (w < 272.0) w = 272.0;
                sst[(size_t)(e0 + k) * sst_stride + p] = w;
            }
    }
}

// the atmo feedback's sst entries: the overlap tile of wholegrid_sst standardized with
// the slab reservoir's sst mean / std (tile_4d_and_logp_to_local_state_input_slab +
// standardize_data_given_pars1d, mpires.f90:575-581, copied over at :733-736): a
// subtraction, then a division.  sst [E][96 * 48], fb [E][>= tot_fb]
__global__ void k_sst_feedback(const double *__restrict__ sst, int64_t sst_stride, const int32_t *__restrict__ fbi,
                               const int32_t *__restrict__ gi, const uint16_t *__restrict__ reg,
                               const double *__restrict__ ms, int n, double *__restrict__ fb, int64_t fb_stride,
                               int E) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int j = reg[i], g = gi[i], d = fbi[i];
    const double mean = ms[2 * j], stdv = ms[2 * j + 1];
    for (int e0 = 0; e0 < E; e0 += kSlabTile) {
        double v[kSlabTile];
#pragma unroll
        for (int k = 0; k < kSlabTile; ++k)
            if (e0 + k < E) v[k] = sst[(size_t)(e0 + k) * sst_stride + g];
#pragma unroll
        for (int k = 0; k < kSlabTile; ++k)
            if (e0 + k < E) {
                const double t = v[k] - mean;
                fb[(size_t)(e0 + k) * fb_stride + d] = t / stdv;
            }
    }
}

// ---- the launches (each checks nothing: the callers have checked sizes and strides)
inline void launch_slab_avg(const double *ring, int64_t ring_stride, int ncol, int tot, double *fb, int64_t fb_stride,
                            int E, hipStream_t st) {
    hipLaunchKernelGGL(k_slab_avg, dim3((tot + 255) / 256), dim3(256), 0, st, ring, ring_stride, ncol, tot, fb,
                       fb_stride, E);
}
inline void launch_slab_ring(const double *fb, int64_t fb_stride, const int32_t *src, int tot, double *col,
                             int64_t ring_stride, int E, hipStream_t st) {
    hipLaunchKernelGGL(k_slab_ring, dim3((tot + 255) / 256), dim3(256), 0, st, fb, fb_stride, src, tot, col,
                       ring_stride, E);
}
inline void launch_slab_fill(int nsst, int nlocal, int nout, int xw, double *ov, int64_t ov_stride, int E,
                             hipStream_t st) {
    hipLaunchKernelGGL(k_slab_rows, dim3((nlocal * nsst + 255) / 256), dim3(256), 0, st, nullptr, 0, nullptr, 0, nsst,
                       nlocal, nout, xw, true, ov, ov_stride, E);
}
inline void launch_slab_rows(const double *slab_ov, int64_t sov_stride, const int32_t *row, int nslab, int nsst,
                             int nlocal, int nout, int xw, double *ov, int64_t ov_stride, int E, hipStream_t st) {
    hipLaunchKernelGGL(k_slab_rows, dim3((nslab * nsst + 255) / 256), dim3(256), 0, st, slab_ov, sov_stride, row, nslab,
                       nsst, nlocal, nout, xw, false, ov, ov_stride, E);
}
inline void launch_sst_grid(const double *ov_all, int64_t ov_stride, const int32_t *src, const double *base,
                            const double *mask, double *sst, int64_t sst_stride, int E, hipStream_t st) {
    hipLaunchKernelGGL(k_sst_grid, dim3((kGrid2d + 255) / 256), dim3(256), 0, st, ov_all, ov_stride, src, base, mask,
                       sst, sst_stride, E);
}
inline void launch_sst_feedback(const double *sst, int64_t sst_stride, const int32_t *fbi, const int32_t *gi,
                                const uint16_t *reg, const double *ms, int n, double *fb, int64_t fb_stride, int E,
                                hipStream_t st) {
    hipLaunchKernelGGL(k_sst_feedback, dim3((n + 255) / 256), dim3(256), 0, st, sst, sst_stride, fbi, gi, reg, ms, n, fb,
                       fb_stride, E);
}

}  // namespace
