// sml_res_radius.hpp -- the spectral radius of every local region's A by power
// iteration with a Collatz-Wielandt enclosure (RadiusOut, k_res_radius).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sml_reservoir_layout.hpp"

namespace {
using namespace sml;

// ---------------------------------------------------------------- spectral radius
// sml_res_spectral_radius: gen_res's sparse_eigen (src/mod_reservoir.f90:190) for the
// matrices makesparse builds -- no negative entry, so the dominant eigenvalue is real
// and simple (Perron-Frobenius) and plain power iteration finds it; the
// Collatz-Wielandt ratios min / max of (A x)_i / x_i enclose it at every iteration
// (DESIGN.md "Reservoir generation").  A block per region, the whole iteration in one
// launch: x and y in LDS (or, same body, in the context's scratch), two block barriers
// per iteration, no communication between blocks.  The norm is max |y_i| and the
// enclosure a min and a max: no sum whose order could differ between forms.  The
// waves' partial min / max go through global memory (d_rad_part), because at n = 10240
// x and y take the whole 160 KiB of LDS; __syncthreads orders them within the block.
struct RadiusOut {
    double lo, hi;
    int32_t iters, info;
};

constexpr int kRadWaves = kUpdThreads / 64;

template <typename WT>
__device__ __attribute__((always_inline)) inline void radius_region(const int32_t *__restrict__ rp,
                                                                    const uint16_t *__restrict__ ac,
                                                                    const WT *__restrict__ av, int n, double *x,
                                                                    double *y, double *pw, double tol, int max_iter,
                                                                    RadiusOut *out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // a negative or non-finite entry: Perron-Frobenius does not hold, nothing is iterated
    // (the block's "any" goes through the partials like the min / max below: no
    // __syncthreads_or, whose static LDS would not fit beside 160 KiB of x and y)
    int bad = 0;
    for (int e = tid, e1 = rp[n]; e < e1; e += kUpdThreads) {
        const double v = (double)av[e];
        bad |= !(v >= 0.0 && v <= 1.7976931348623157e308);
    }
    bad = __any(bad);
    if (lane == 0) pw[wave] = bad ? 1.0 : 0.0;
    __syncthreads();
    double anybad = pw[lane % kRadWaves];
    for (int o = kRadWaves / 2; o > 0; o >>= 1) anybad = fmax(anybad, __shfl_xor(anybad, o));
    if (anybad > 0.0) {  // block-uniform
        if (tid == 0) *out = RadiusOut{__builtin_nan(""), __builtin_nan(""), 0, SML_RADIUS_INVALID};
        return;
    }
    for (int i = tid; i < n; i += kUpdThreads) x[i] = 1.0;
    __syncthreads();  // x complete; the flags read by every wave before the partials reuse them
    double lo = 0.0, hi = 0.0;
    int info = SML_RADIUS_MAXITER, t = 1;
    for (;; ++t) {  // (lo, hi, the norm and so every branch below are block-uniform)
        double tlo = __builtin_inf(), thi = 0.0, tm = 0.0;
        for (int i = tid; i < n; i += kUpdThreads) {
            double s = 0.0;
            for (int e = rp[i], e1 = rp[i + 1]; e < e1; ++e) s = s + (double)av[e] * x[ac[e]];
            y[i] = s;
            const double xi = x[i];
            if (xi > 0.0) {
                const double q = s / xi;
                tlo = fmin(tlo, q);
                thi = fmax(thi, q);
            }
            tm = fmax(tm, s);
        }
        for (int o = 32; o > 0; o >>= 1) {
            tlo = fmin(tlo, __shfl_xor(tlo, o));
            thi = fmax(thi, __shfl_xor(thi, o));
            tm = fmax(tm, __shfl_xor(tm, o));
        }
        if (lane == 0) {
            pw[wave] = tlo;
            pw[kRadWaves + wave] = thi;
            pw[2 * kRadWaves + wave] = tm;
        }
        __syncthreads();  // y and the partials complete; every read of x done
        lo = pw[lane % kRadWaves];
        hi = pw[kRadWaves + lane % kRadWaves];
        double m = pw[2 * kRadWaves + lane % kRadWaves];
        for (int o = kRadWaves / 2; o > 0; o >>= 1) {
            lo = fmin(lo, __shfl_xor(lo, o));
            hi = fmax(hi, __shfl_xor(hi, o));
            m = fmax(m, __shfl_xor(m, o));
        }
        if (m == 0.0) {
            lo = hi = 0.0;
            info = SML_RADIUS_ZERO;
            break;
        }
        if (hi - lo <= tol * hi) {
            info = SML_RADIUS_OK;
            break;
        }
        if (t == max_iter) break;
        for (int i = tid; i < n; i += kUpdThreads) x[i] = y[i] / m;
        __syncthreads();  // x complete; the partials read by every wave
    }
    if (tid == 0) *out = RadiusOut{lo, hi, t, info};
}

// lds_limit: the bytes of LDS a region's 2 n doubles may take (0 forces the scratch)
template <typename WT>
__global__ __launch_bounds__(kUpdThreads) void k_res_radius(const RegionDev *__restrict__ R,
                                                            const int32_t *__restrict__ row0,
                                                            const int32_t *__restrict__ a_rp,
                                                            const uint16_t *__restrict__ a_col,
                                                            const WT *__restrict__ a_val, double *xy, double *part,
                                                            RadiusOut *out, double tol, int max_iter,
                                                            size_t lds_limit) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int r = blockIdx.x;
    const RegionDev rg = R[r];
    const int n = rg.n;
    const int32_t *rp = a_rp + rg.a_rp;
    const uint16_t *ac = a_col + rg.a_nz;
    const WT *av = a_val + rg.a_nz;
    double *pw = part + (size_t)r * 3 * kRadWaves;
    if (2 * (size_t)n * sizeof(double) <= lds_limit) {  // block-uniform
        radius_region<WT>(rp, ac, av, n, smem, smem + n, pw, tol, max_iter, out + r);
    } else {
        double *x = xy + 2 * (int64_t)row0[r];
        radius_region<WT>(rp, ac, av, n, x, x + n, pw, tol, max_iter, out + r);
    }
}

}  // namespace
