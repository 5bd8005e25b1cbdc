// sml_res_noise.hpp -- the reference's input noise (gaussian_noise_1d_function,
// gaussian_noise_1d_function_precip: src/mod_utilities.f90:1380-1402, :1404-1456) on blocks
// of the packed feedback layout (k_input_noise).  DESIGN.md §3.11.
//
// Entry e (0-based, in its region's feedback) of the block of absolute step t of a region
// with noise id `region` draws, from the generator of sml_counter_rng.hpp,
//   u1 = (b1 + 1) 2^-53 in (0, 1],  u2 = b2 2^-53 in [0, 1)      (streams 4 and 5, index (t << 20) | e)
//   g  = sqrt(-2 log(u1)) * cospi(2 u2)                           Box-Muller's cosine branch
// (cospi(2 u2), not cos(twopi * u2): 2 u2 is exact, so the argument carries no rounding), and
//   plain entry    noisy = x + (g * noisemag) * x
//   precip entry   p = eps * (exp(x * std + mean) - 1);  p = |p + g * noisemag|;
//                  noisy = (log(1 + p / eps) - mean) / std       mean, std: the region's slot 34
// one rounding per operation (the unit is built with -ffp-contract=off).  noisemag == 0
// copies x: stated, not computed, so -0.0 keeps its sign.  Without an input (in == NULL)
// the output is g itself.
//
// A thread owns one entry and kTileMem blocks: it reads its table entries, its region's
// keys and (a precip entry) mean / std once and keeps the kTileMem loads in flight
// together, k_tile_series's idiom.  No atomics, no LDS, no scratch; in == out is allowed
// (a thread reads its own words before it writes them, and no other thread touches them).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sml_counter_rng.hpp"
#include "sml_res_tiling.hpp"
#include "sml_reservoir_layout.hpp"

namespace {
using namespace sml;

constexpr int kNoiseThreads = 256;
constexpr int kNoisePrecipSlot = 34;  // the series tables' slot of the precipitation entries

struct NoiseDev {
    const uint16_t *reg;    // [tot_fb] the entry's local region
    const uint64_t *key;    // [nlocal][2] the region's keys of streams 4 and 5
    const uint8_t *slot;    // [tot_fb] the entry's mean / std slot; NULL: every entry is plain
    const double *meanstd;  // [nlocal][2 * kMeanStd] the context's adopted table
    double noisemag, eps;
};

__device__ __forceinline__ double noise_normal(uint64_t k1, uint64_t k2, uint64_t index) {
    const double u1 = noise_u1(noise_bits(k1, index)), u2 = noise_u2(noise_bits(k2, index));
    return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}

// grid (ceil(total / kNoiseThreads), tiles of kTileMem blocks): blocks t0 .. t0 + m - 1, block c
// read at in + c * in_stride and written at out + c * out_stride
__global__ __launch_bounds__(kNoiseThreads) void k_input_noise(const RegionDev *__restrict__ R, NoiseDev nz,
                                                               const double *in, int64_t in_stride, double *out,
                                                               int64_t out_stride, int64_t t0, int m, int total) {
    const int e = blockIdx.x * kNoiseThreads + threadIdx.x;
    if (e >= total) return;
    const int r = nz.reg[e];
    const uint64_t el = (uint64_t)(e - R[r].fb);
    const uint64_t k1 = nz.key[2 * r], k2 = nz.key[2 * r + 1];
    const bool precip = nz.slot && nz.slot[e] == kNoisePrecipSlot;
    double mean = 0.0, stdv = 1.0;
    if (precip) {
        const double *ms = nz.meanstd + (size_t)r * 2 * kMeanStd;
        mean = ms[kNoisePrecipSlot];
        stdv = ms[kMeanStd + kNoisePrecipSlot];
    }
    const double mag = nz.noisemag, eps = nz.eps;
    for (int c0 = blockIdx.y * kTileMem; c0 < m; c0 += gridDim.y * kTileMem) {
        double v[kTileMem];
#pragma unroll
        for (int k = 0; k < kTileMem; ++k) v[k] = (in && c0 + k < m) ? in[(size_t)(c0 + k) * in_stride + e] : 0.0;
#pragma unroll
        for (int k = 0; k < kTileMem; ++k)
            if (c0 + k < m) {
                const double x = v[k];
                double y = x;
                if (!in || mag != 0.0) {
                    const double g = noise_normal(k1, k2, ((uint64_t)(t0 + c0 + k) << kNoiseEntryBits) | el);
                    if (!in) {
                        y = g;
                    } else if (precip) {
                        double p = x * stdv;
                        p = p + mean;
                        p = eps * (exp(p) - 1.0);
                        const double gm = g * mag;
                        p = fabs(p + gm);
                        p = log(1.0 + p / eps);
                        p = p - mean;
                        y = p / stdv;
                    } else {
                        const double gm = g * mag;
                        y = x + gm * x;
                    }
                }
                out[(size_t)(c0 + k) * out_stride + e] = y;
            }
    }
}

}  // namespace
