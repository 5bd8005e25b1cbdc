// sml_dyn_fused.hpp -- the kernels of the fused step: k_state_to_m, k_st_inv, the
// row kernels k_st_rows / k_st_gridspec_p with their FFT row helpers, k_pack_pfwd and
// the per-m k_st_spec, with the MFMA helpers they share with the io entry kernel.
// (A timeline build, SML_TL, needs the unit's SML_TL_DEFINE ahead of this header.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "sml_dyn_gridpoint.hpp"
#include "sml_dyn_layout.hpp"
#include "sml_dyn_spec_math.hpp"
#include "sml_dynamics_tables.hpp"
#include "sml_fft.hpp"
#include "sml_fft_wa96.hpp"
#include "sml_physics.hpp"
#include "sml_physics_pair.hpp"
#include "sml_spectral_internal.hpp"
#include "sml_timeline.hpp"

namespace {
using namespace sml;

// ======================================================= fused step
// The step's stages regrouped at the all-to-all seams of the spectral transform
// (spectral <-> Fourier per zonal wavenumber m, Fourier <-> grid per latitude row):
//   k_st_rows   (latitude row j, no GPU physics): gridx (FFT) -> LDS -> grid-point
//               dynamics -> LDS -> specx (FFT)
//   k_st_gridspec_p (with GPU physics): gridx, the grid-point dynamics beside phypar
//               (its roles on waves of their own), specx, in one launch per row
//   k_st_spec   (zonal wavenumber m, 512 threads = 64 coefficients x 8 levels):
//               the tail's state-only half (tail_pre: sptend's and geop's level
//               chains) -> specy -> combine (vds, lap) -> sptend / implic / hordif /
//               timint -> the NEXT step's inverse-transform inputs from the new
//               state (uvspec, grad, geop) -> gridy
//   k_st_inv    (m): the inverse-transform inputs + gridy from the state in memory,
//               for a step that follows no fused step (window start)
// A leapfrog step is 2 launches (with GPU physics: k_st_gridspec_p + k_st_spec)
// instead of 8 / 9.  Each block first stages everything it reads -- the m's slice of
// the state, the row's Fourier coefficients -- in LDS with coalesced loads: the
// fused step keeps its own m-major copies of the state ([m][var][lev][k][n p],
// k_state_to_m before a run of fused steps; the run's last k_st_spec writes the
// reference layout back) and of the forward Fourier coefficients ([m][lat][f][p]),
// so each block's slice is contiguous.  Every stage keeps the unfused kernels'
// arithmetic, operand order and MFMA tiling: results are bit-identical to them
// (tests/test_physics_gpu.py).
typedef double d4 __attribute__((ext_vector_type(4)));
#define MFMA64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

// one 16-B store of a (Re, Im) pair: the inter-kernel hand-offs of the fused step (vfm,
// the next step's varm and state).  (Stored write-through, sc1, the kernel boundary
// got cheaper but the stores far slower: measured and removed)
__device__ __attribute__((always_inline)) inline void store2(double *base, size_t idx, double a, double b) {
    *reinterpret_cast<double2 *>(base + idx) = double2{a, b};
}

// reference state layout <-> the fused step's m-major copy
__global__ void k_state_to_m(const double *__restrict__ st, double *__restrict__ sm) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= kMX * kSM) return;
    const int m = e / kSM, i = e % kSM;
    const int cc = i % kCW, k = (i / kCW) % kKX, lev = (i / (kCW * kKX)) % 2, var = i / (2 * kKX * kCW);
    const int c = ci(cc & 1, m, cc >> 1);
    double v = 0.0;
    if (var < 4) {
        const size_t off = var == 0 ? kOffVor : var == 1 ? kOffDiv : var == 2 ? kOffT : kOffTr;
        v = st[off + ((size_t)lev * kKX + k) * kSF + c];
    } else if (k == 0) {
        v = st[kOffPs + (size_t)lev * kSF + c];
    }
    sm[e] = v;
}

// element i of m's slice (smi layout) into the reference-layout state
__device__ inline void put_state(double *__restrict__ st, int m, int i, double v) {
    const int cc = i % kCW, k = (i / kCW) % kKX, lev = (i / (kCW * kKX)) % 2, var = i / (2 * kKX * kCW);
    const int c = ci(cc & 1, m, cc >> 1);
    if (var < 4) {
        const size_t off = var == 0 ? kOffVor : var == 1 ? kOffDiv : var == 2 ? kOffT : kOffTr;
        st[off + ((size_t)lev * kKX + k) * kSF + c] = v;
    } else if (k == 0) {
        st[kOffPs + (size_t)lev * kSF + c] = v;
    }
}


// uvspec (spe_spectral.f90:351-387) of coefficient (n, p) at level k, time level lev,
// from an m's state slice Sst (smi layout) -> ucos (u), vcos (v).  Branch-free: every
// case's operands read (neighbour indices clamped) and its expression formed, then the
// case selected -- the reference's n == 1 / n == ntrun+2 / interior values without a
// divergent branch and its dependent LDS round trip per case (n and p vary across a
// wave's lanes)
template <class TB>
__device__ inline void uvspec_sel(const double *Sst, const TB &tb, int lev, int k, int n, int p, double *u,
                                  double *v) {
    static_assert(kNTRUN1 - 1 == kNX - 2, "uvspec's last row reads n - 1");
    const int nm = n > 0 ? n - 1 : 0, np = n < kNX - 1 ? n + 1 : kNX - 1;
    const bool first = n == 0, last = n == kNX - 1;
    const double vor_m = Sst[smi(0, lev, k, 2 * nm + p)], vor_p = Sst[smi(0, lev, k, 2 * np + p)];
    const double div_m = Sst[smi(1, lev, k, 2 * nm + p)], div_p = Sst[smi(1, lev, k, 2 * np + p)];
    const double vor_x = Sst[smi(0, lev, k, 2 * n + 1 - p)], div_x = Sst[smi(1, lev, k, 2 * n + 1 - p)];
    const double ux = tb.uvdx_n(n), uvdym = tb.uvdym_n(n), uvdyp = tb.uvdyp_n(n);
    const double zc = p == 1 ? ux * div_x : -ux * div_x;
    const double u0 = zc - uvdyp * vor_p, ul = uvdym * vor_m, um = uvdym * vor_m - uvdyp * vor_p + zc;
    const double zp = p == 1 ? ux * vor_x : -ux * vor_x;
    const double v0 = zp + uvdyp * div_p, vl = -uvdym * div_m, vm = -uvdym * div_m + uvdyp * div_p + zp;
    *u = first ? u0 : last ? ul : um;
    *v = first ? v0 : last ? vl : vm;
}

// The inverse-transform inputs of one m (k_dyn_prep's fields, same expressions)
// from the m's state slice Sst (smi layout); writes In[f][kCW] for f < nin.  The
// whole block calls it.
template <class TB>
__device__ inline void inv_inputs(const double *Sst, double *In, const double *phis_m, const TB &tb, int m, int j2,
                                  int n1, int nin) {
    // one thread per (coefficient cc = 2 n + p, level k) (512 threads): the fields of
    // level k, in the same expressions as k_dyn_prep
    const bool phys = nin > kNInv;
    // (k wave-uniform, wave_index(): the k == 0 fields, the m == 0 correction and geop's
    // bound below are uniform branches)
    const int cc = threadIdx.x & (kCW - 1), k = wave_index(), n = cc >> 1, p = cc & 1;
    auto sv = [&](int var, int lev, int kk, int c2) { return Sst[smi(var, lev, kk, c2)]; };
    auto put = [&](int f, double v) { In[f * kCW + cc] = v; };
#pragma unroll
    for (int var = 0; var < 4; ++var) put(var * kKX + k, sv(var, j2, k, cc));
    // uvspec of level lev at k -> ucos (field fu), vcos (fv)
    const int nm = n > 0 ? n - 1 : 0, np = n < kNX - 1 ? n + 1 : kNX - 1;
    const bool first = n == 0, last = n == kNX - 1;
    auto uvspec = [&](int lev, int fu, int fv) {
        double u, v;
        uvspec_sel(Sst, tb, lev, k, n, p, &u, &v);
        put(fu, u);
        put(fv, v);
    };
    uvspec(j2, n1 + k, n1 + kKX + k);
    if (k == 0) {  // grad(ps(j2)) (wave-uniform branch; the n cases selected as in uvspec)
        const double ps_x = sv(4, j2, 0, 2 * n + 1 - p), ps_m = sv(4, j2, 0, 2 * nm + p), ps_p = sv(4, j2, 0, 2 * np + p);
        const double gx = tb.gradx_m(), gym = tb.gradym_n(n), gyp = tb.gradyp_n(n);
        put(n1 + 2 * kKX, p == 1 ? gx * ps_x : -gx * ps_x);
        const double v0 = gyp * ps_p, vl = -gym * ps_m, vm = -gym * ps_m + gyp * ps_p;
        put(n1 + 2 * kKX + 1, first ? v0 : last ? vl : vm);
    }
    if (!phys) return;
    // phypar's level-1 inputs: t1, q1, geop(1) (geop_at), ps1, ucos1, vcos1
    put(kPT1 + k, sv(2, 1, k, cc));
    put(kPQ1 + k, sv(3, 1, k, cc));
    // (the sum ends at the wave's level by a uniform branch.  The operands are not pinned
    // in one batch ahead of the branches: the compiler's own placement, each level's
    // reads in its branch, measured faster -- the phase 1.12-1.16 us against 1.28-1.32
    // pinned and 1.24 branch-free, profiles/spec_kernel_uniform.md)
    double t1[kKX], g1[kKX], g2[kKX];
#pragma unroll
    for (int kk = 0; kk < kKX; ++kk) {
        t1[kk] = sv(2, 1, kk, cc);
        g1[kk] = tb.xgeop1(kk);
        g2[kk] = kk > 0 ? tb.xgeop2(kk) : 0.0;  // (xgeop2(1) is not used)
    }
    double phi = phis_m[cc] + g1[kKX - 1] * t1[kKX - 1];
#pragma unroll
    for (int kk = kKX - 2; kk >= 0; --kk) {
        if (kk < k) break;  // (uniform)
        const double nx = phi + g2[kk + 1] * t1[kk + 1] + g1[kk] * t1[kk];
        phi = nx;
    }
    {
        const int km = k > 0 ? k - 1 : 0, kp = k < kKX - 1 ? k + 1 : kKX - 1;
        const double pc = phi + tb.corf(k) * (sv(2, 1, kp, cc) - sv(2, 1, km, cc));
        if (m == 0 && k >= 1 && k <= kKX - 2) phi = pc;
    }
    put(kPPhi1 + k, phi);
    if (k == 0) put(kPPs1, sv(4, 1, 0, cc));
    uvspec(1, n1 + 2 * kKX + 2 + k, n1 + 3 * kKX + 2 + k);
}

// gridy of In[f][kCW] (this m) -> vim[m][lat][f][p] (k_gridy's tiling: one wave per
// 8-field x Re/Im tile, waves of the block stride over the tiles)
// the Legendre operands of gridy_m for this lane (loaded once per wave)
struct GridyB {
    double b00[4], b01[4], b10[4], b11[4];
};
// the same operands from a copy of pinv's m-slice [n][32] (LDS)
__device__ inline GridyB gridy_operands_slice(const double *pm) {
    const int l = threadIdx.x & 63, r = l & 15, kk = l >> 4;
    GridyB g;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int n_odd = 2 * (4 * s + kk), n_even = n_odd + 1;
        g.b00[s] = pm[n_odd * 32 + r];
        g.b01[s] = pm[n_odd * 32 + 16 + r];
        g.b10[s] = pm[n_even * 32 + r];
        g.b11[s] = pm[n_even * 32 + 16 + r];
    }
    return g;
}

__device__ inline GridyB gridy_operands(const double *__restrict__ pinv, int m) {
    const int l = threadIdx.x & 63, r = l & 15, kk = l >> 4;
    const double *pm = pinv + (size_t)m * kNX * 32;
    GridyB g;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int n_odd = 2 * (4 * s + kk), n_even = n_odd + 1;
        g.b00[s] = pm[n_odd * 32 + r];
        g.b01[s] = pm[n_odd * 32 + 16 + r];
        g.b10[s] = pm[n_even * 32 + r];
        g.b11[s] = pm[n_even * 32 + 16 + r];
    }
    return g;
}

__device__ inline void gridy_m(const double *In, const GridyB &gb, double *__restrict__ varm, int m, int nf,
                               int tile0 = 0, int tile1 = -1) {
    const int wave = wave_index(), nw = blockDim.x >> 6;
    const int l = threadIdx.x & 63, r = l & 15, kk = l >> 4;
    const int tend = tile1 < 0 ? (nf + 7) / 8 : tile1;
    // work unit u = (tile, latitude half): half 0 the rows j < 16 (b00 / b10), half 1
    // j >= 16 (b01 / b11).  Whole tiles left the SIMDs uneven (k_st_spec's 6 tiles on
    // 8 waves: 2 tiles on two SIMDs, 1 on the others); half tiles give every SIMD 1.5
    for (int u = wave; u < 2 * (tend - tile0); u += nw) {
        const int tile = tile0 + (u >> 1), half = u & 1;
        const int f0 = tile * 8;
        const int fa = f0 + (r >> 1), p = r & 1;
        const bool ok = fa < nf;
        const double *a = In + (ok ? fa : 0) * kCW + p;
        d4 accS = {0, 0, 0, 0}, accA = accS;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int n_odd = 2 * (4 * s + kk);  // n = 1,3,.. (1-based): symmetric part
            const int n_even = n_odd + 1;        // n = 2,4,..: antisymmetric part
            // (the product does not need the zeroing -- a lane past the last field holds
            // its own column r of the B operand and skips its stores -- but without it
            // the compiler pairs and batches these reads and the phase measured 2.00
            // against 1.68 us: kept, profiles/spec_kernel_uniform.md)
            const double a0 = ok ? a[2 * n_odd] : 0.0;
            const double a1 = ok ? a[2 * n_even] : 0.0;
            // the transposed product (Legendre operand first: the same products summed
            // in the same order), so a lane's outputs are latitude rows kk + 4 q of
            // field-part column r: a store instruction writes 16 consecutive doubles of
            // 4 latitudes (4 lines) instead of 4 of 16 latitudes (16 lines)
            accS = MFMA64(half ? gb.b01[s] : gb.b00[s], a0, accS);
            accA = MFMA64(half ? gb.b11[s] : gb.b10[s], a1, accA);
        }
        if (!ok) continue;
        // m-major inverse Fourier coefficients vim[m][lat][f][p]: column r = 2 (fa - f0) + p
        double *vr = varm + (size_t)m * kVIm + fa * 2 + p;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = 16 * half + kk + 4 * q;
            if (j >= kIY) continue;
            const double sym = accS[q], asym = accA[q];
            vr[(kIL - 1 - j) * kVIl] = sym + asym;
            vr[j * kVIl] = sym - asym;
        }
    }
}

// gridy_m with the spectral module's Fourier layout [f][lat][2 m + p] (k_gridy's
// stores): iogrid(31)'s inverse Legendre of the io fields, fused into the window's
// last per-m kernel (run_model)
__device__ inline void gridy_io(const double *In, const GridyB &gb, double *__restrict__ varm, int m, int nf) {
    const int wave = wave_index(), nw = blockDim.x >> 6;
    const int l = threadIdx.x & 63, r = l & 15, kk = l >> 4;
    for (int tile = wave; tile < (nf + 7) / 8; tile += nw) {
        const int f0 = tile * 8;
        const int fa = f0 + (r >> 1), p = r & 1;
        const bool ok = fa < nf;
        const double *a = In + (ok ? fa : 0) * kCW + p;
        d4 acc00 = {0, 0, 0, 0}, acc01 = acc00, acc10 = acc00, acc11 = acc00;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int n_odd = 2 * (4 * s + kk);
            const int n_even = n_odd + 1;
            // (the zeroing kept as in gridy_m, where dropping it measured slower)
            const double a0 = ok ? a[2 * n_odd] : 0.0;
            const double a1 = ok ? a[2 * n_even] : 0.0;
            acc00 = MFMA64(a0, gb.b00[s], acc00);
            acc01 = MFMA64(a0, gb.b01[s], acc01);
            acc10 = MFMA64(a1, gb.b10[s], acc10);
            acc11 = MFMA64(a1, gb.b11[s], acc11);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = kk + 4 * q;
            const int f = f0 + (row >> 1);
            if (f >= nf) continue;
            double *vr = varm + (size_t)f * kVarmField + 2 * m + (row & 1);
            {
                const int j = r;
                const double sym = acc00[q], asym = acc10[q];
                vr[(kIL - 1 - j) * kMX2] = sym + asym;
                vr[j * kMX2] = sym - asym;
            }
            const int j = 16 + r;
            if (j < kIY) {
                const double sym = acc01[q], asym = acc11[q];
                vr[(kIL - 1 - j) * kMX2] = sym + asym;
                vr[j * kMX2] = sym - asym;
            }
        }
    }
}

// iogrid(31)'s k_io_prep at (coefficient cc, level k) from time level 1 of an m-major
// state slice: uvspec of (vor, div), copies of t, tr, ps -> put(field, value) in the
// io layout [u 8 | v 8 | t 8 | q 8 | ps] (the same expressions as uvspec_at)
template <class TB, class Put>
__device__ inline void io_prep_m(const double *Sst, const TB &tb, int k, int cc, Put put) {
    const int n = cc >> 1, p = cc & 1;
    double a, b;
    uvspec_sel(Sst, tb, 1, k, n, p, &a, &b);
    put(k, a);
    put(kKX + k, b);
    put(2 * kKX + k, Sst[smi(2, 1, k, cc)]);
    put(3 * kKX + k, Sst[smi(3, 1, k, cc)]);
    if (k == 0) put(4 * kKX, Sst[smi(4, 1, 0, cc)]);
}

// stage the m's forcing (phis, tcorh, qcorh: reference layout) into Fm[3][kCW]
__device__ inline void load_forcing_m(double *Fm, const double *__restrict__ phis, const double *__restrict__ tcorh,
                                      const double *__restrict__ qcorh, int m) {
    for (int i = threadIdx.x; i < 3 * kCW; i += blockDim.x) {
        const int which = i / kCW, cc = i % kCW;
        const double *src = which == 0 ? phis : which == 1 ? tcorh : qcorh;
        Fm[i] = src[ci(cc & 1, m, cc >> 1)];
    }
}

constexpr int kSpecThreads = kCW * kKX;  // 512: one thread per (coefficient, level) of one m
constexpr int kSpecBlk = 512;             // k_st_spec's block (768: specy -0.6 us, staging +1.2 us, gridy unchanged)
constexpr int kSpecSplit = 2;             // k_st_spec blocks per m (the next step's gridy tiles split between them)
// k_st_spec's grid: block b takes m = b % kSpecStride, half = b / kSpecStride.  A
// launch on a stream places block b on the same XCD every time, the same for every
// kernel of the stream (tools/probe_xcd_l2.hip: XCD = (b + c) mod 8), so with a
// stride of 32 (two idle blocks) both blocks of an m share the XCD of the lead block
// that wrote the m's state in the previous step (and of k_io_entry's block m): the
// slice and the m's tables are L2 hits for both, and the second block's copy of the
// m's Fourier coefficients merges with the first's in that L2.  Stride 31 (62 blocks):
// the second block's reads cross XCDs; same-box A/B: window 0.822 -> 0.800 ms,
// 1006.6 / 1013.5 -> 1018.9 / 1032.2 steps/s (profiles/r03d).  Speed only: any
// placement gives the same results.
#ifndef SML_SPEC_STRIDE
#define SML_SPEC_STRIDE 32
#endif
constexpr int kSpecStride = SML_SPEC_STRIDE;
static_assert(kSpecStride >= kMX, "k_st_spec grid stride");

// window start: the inverse transforms of step (.., j2) from the m-major state
__global__ __launch_bounds__(kSpecThreads) void k_st_inv(const double *__restrict__ sm, const double *__restrict__ phis,
                                                         const DynTables *__restrict__ T,
                                                         const double *__restrict__ pinv, double *__restrict__ varm,
                                                         int j2, int n1, int nin) {
    __shared__ double Sst[kSM];
    __shared__ double In[kNInvMax * kCW];
    __shared__ double Fm[kCW];
    const int m = blockIdx.x;
    const double *src = sm + (size_t)m * kSM;
    for (int i = threadIdx.x; i < kSM / 2; i += blockDim.x)
        reinterpret_cast<double2 *>(Sst)[i] = reinterpret_cast<const double2 *>(src)[i];
    for (int cc = threadIdx.x; cc < kCW; cc += blockDim.x) Fm[cc] = phis[ci(cc & 1, m, cc >> 1)];
    __syncthreads();
    inv_inputs(Sst, In, Fm, GTab{T, m}, m, j2, n1, nin);
    __syncthreads();
    gridy_m(In, gridy_operands(pinv, m), varm, m, nin);
}

// Fourier stage of one latitude row: FFTPACK's real FFT (sml_fft.hpp, the reference's
// rfftb / rfftf operation order), one transform per thread held in registers; the
// row's grid values meet the column-wise grid-point stage in LDS, element-major
// A[lon][f] (row stride kRowLd, odd: the column threads' reads spread over banks).
constexpr int kRowThreads = 128, kRowLd = 97;
static_assert(kNInvMax <= kRowThreads && kNFwd <= kRowThreads && kIX <= kRowThreads, "one thread per transform");

// gridx of field f, row j (spe_subfft_fftpack.f90:24-45): packing, rfftb, x cosgr(j)
// for kcos = 2; the 96 values into A[lon][f]
__device__ __attribute__((always_inline)) inline void row_gridx(double *A, const double *__restrict__ varm, const double *__restrict__ wa, int f,
                                 int j, bool kcos2, double cj) {
    // the m-major coefficients vim[m][lat][f][p] of (f, j): coefficient c = 2 m + p
    const double *v = varm + (size_t)j * kVIl + f * 2;
    auto V = [&](int c) { return v[(size_t)(c >> 1) * kVIm + (c & 1)]; };
    double x[kFftN];
    x[0] = V(0);
#pragma unroll
    for (int e = 1; e <= kMX2 - 2; ++e) x[e] = V(e + 1);
#pragma unroll
    for (int e = kMX2 - 1; e < kFftN; ++e) x[e] = 0.0;
    fft::rfftb96_reg(x, wa);
#pragma unroll
    for (int e = 0; e < kFftN; ++e) A[e * kRowLd + f] = kcos2 ? x[e] * cj : x[e];
}

// specx of field f, row j from x[96] (already x cosgr(j) where vdspec scales):
// rfftf, varm(1) = fvar(1)/ix, varm(2) = 0, varm(m) = fvar(m-1)/ix, into the m-major
// forward coefficients vfm[m][f][j][p]
__device__ __attribute__((always_inline)) inline void row_specx(double *x, double *__restrict__ vfm, const double *__restrict__ wa, int f, int j) {
    fft::rfftf96_reg(x, wa);
    const double scale = 1. / (double)kIX;
    double *o = vfm + (size_t)j * kVLs + f * 2;
    o[0] = x[0] * scale;
    o[1] = 0.0;
#pragma unroll
    for (int c = 2; c < kMX2; ++c) o[(size_t)(c >> 1) * kVFm + (c & 1)] = x[c - 1] * scale;
}

// The row kernel's transforms on lane pairs (sml_fft.hpp rfftb96_half /
// rfftf96_combine): lane h of a pair does half h of FFTPACK's n = 96 transform, so a
// lane's dependent chain is about half of a whole transform's.
// gridx half h of field f, row j: grid points 2 q + h into A (x cosgr where kcos2)
// FFTPACK's half-complex input of field f, row j: x[0] = a0, x[2m-1] = Re, x[2m] = Im
// (m <= 30), 0 beyond (x(e) is a compile-time zero there)
__device__ __attribute__((always_inline)) inline void row_gridx_load(const double *__restrict__ varm, int f, int j,
                                                                     double (&xi)[kMX2 - 1]) {
    const double *v = varm + (size_t)j * kVIl + f * 2;
    xi[0] = v[0];  // a0 (coefficient c = 0); x[e] = coefficient c = e + 1 for e >= 1
#pragma unroll
    for (int e = 1; e < kMX2 - 1; ++e) xi[e] = v[(size_t)((e + 1) >> 1) * kVIm + ((e + 1) & 1)];
    // every load in flight before the first use: left alone, the scheduler hoisted
    // radb2's first add (x(0) + a zero) between the loads, and its wait cost a
    // whole memory round trip before the remaining loads issued
    __builtin_amdgcn_sched_barrier(0);
}

__device__ __attribute__((always_inline)) inline void row_gridx_half(double *A, const double (&xi)[kMX2 - 1],
                                                                     const double *__restrict__ wa, int f,
                                                                     bool kcos2, double cj, int h) {
    double y[48];
    fft::rfftb96_half([&](int e) { return e <= kMX2 - 2 ? xi[e] : 0.0; }, h, y, wa);
#pragma unroll
    for (int q = 0; q < 48; ++q) A[(2 * q + h) * kRowLd + f] = kcos2 ? y[q] * cj : y[q];
}

// specx of transform f, row j, on a lane pair: lane h holds its rfftf48 result of the
// samples 2 i + h in x48; the pair meets in LDS (E = half 0, O = half 1, rows
// [48 h, 48 h + 48) of S, column f) for radf2(48, 1) (spe_subfft_fftpack2.f90:741-789)
// of the outputs m <= 30 (lane 0: m <= 15, lane 1: 16..30), scale 1/ix, into the
// m-major forward coefficients vfm[m][f][j][p].  The whole block calls it (barrier).
__device__ __attribute__((always_inline)) inline void row_specx_pair(const double *x48, double *S, bool act,
                                                                     double *__restrict__ vfm,
                                                                     const double *__restrict__ wa, int f, int j,
                                                                     int h) {
    if (act) {
#pragma unroll
        for (int i = 0; i < 48; ++i) S[(48 * h + i) * kRowLd + f] = x48[i];
    }
    __syncthreads();
    if (!act) return;
    auto E = [&](int i) { return S[i * kRowLd + f]; };
    auto O = [&](int i) { return S[(48 + i) * kRowLd + f]; };
    const double scale = 1. / (double)kIX;
    // lane h does m = 16 h + i, i = 0..15, with the operands of its m selected per lane
    // (the halves' different m ranges were divergent branches: each wave ran both);
    // every m's expressions are rfftf96_combine's: E(2s-1) +- tr2, ti2 +- E(2s) with
    // the sign taken as an exact negation, m = 0 and 24 special
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int m0 = i, m1 = 16 + i;  // lane h = 0 / 1
        const int s0 = m0, s1 = m1 < 24 ? m1 : 48 - m1;
        const int m = h ? m1 : m0, sv = h ? s1 : s0;
        if (m >= kMX) continue;  // (h = 1, i = 15)
        const int sa = sv > 0 ? sv : 1;  // (m = 0: operands unused)
        const double c = h ? wa[2 * (s1 > 0 ? s1 : 1) - 2] : wa[2 * (s0 > 0 ? s0 : 1) - 2];
        const double sn = h ? wa[2 * (s1 > 0 ? s1 : 1) - 1] : wa[2 * (s0 > 0 ? s0 : 1) - 1];
        const double e1 = E(2 * sa - 1), e2 = E(2 * sa), o1 = O(2 * sa - 1), o2 = O(2 * sa);
        const double tr2 = c * o1 + sn * o2;
        const double ti2 = c * o2 - sn * o1;
        const bool lo = m < 24;
        double re = lo ? e1 + tr2 : e1 - tr2;
        double im = lo ? e2 + ti2 : ti2 - e2;
        if (m == 0) {  // ch(1, 1) = cc(1, 1) + cc(1, 2); varm(2) = 0
            re = E(0) + O(0);
            im = 0.0;
        } else if (m == 24) {  // ido even: ch(ido, 1) = cc(ido, 1), ch(1, 2) = -cc(ido, 2)
            re = E(47);
            im = -O(47);
        }
        store2(vfm, (size_t)j * kVLs + f * 2 + (size_t)m * kVFm, re * scale, im * scale);
    }
}

// one latitude row without GPU physics: gridx of the 50 inverse transforms, grid-
// point dynamics of the row's 96 columns (+ a host's physics tendencies Pext
// [u|v|t|q][kx][ngp] if given) into LDS, specx straight to the m-major coefficients.
__global__ __launch_bounds__(kRowThreads) void k_st_rows(const double *__restrict__ varm, double *__restrict__ vfm,
                                                         const double *__restrict__ wa,
                                                         const double *__restrict__ cosgr,
                                                         const DynTables *__restrict__ T,
                                                         const double *__restrict__ Pext, long long *dbg) {
    __shared__ double A[kFftN * kRowLd], B[kFftN * kRowLd], was[kFftWa];
    constexpr int n1 = kNInv1, nin = kNInv;
    const int j = blockIdx.x, tid = threadIdx.x;
    if (tid < kFftWa) was[tid] = wa[tid];
    __syncthreads();
    const double cj = cosgr[j];
    stamp(dbg, 0, 0);
    stamp(dbg, 0, 1);
    // gridx: one field per thread
    if (tid < nin) row_gridx(A, varm, was, tid, j, tid >= n1, cj);
    __syncthreads();
    stamp(dbg, 0, 2);
    // one thread per grid column: grid-point dynamics, the forward-transform inputs into B
    if (tid < kIX) {
        const int i = tid, pt = j * kIX + i;
        auto g = [&](int f) { return A[i * kRowLd + f]; };
        double pu[kKX], pv[kKX], ptt[kKX], pq[kKX];
        if (Pext) {
#pragma unroll
            for (int k = 0; k < kKX; ++k) {
                pu[k] = Pext[(size_t)k * kGF + pt];
                pv[k] = Pext[(size_t)(kKX + k) * kGF + pt];
                ptt[k] = Pext[(size_t)(2 * kKX + k) * kGF + pt];
                pq[k] = Pext[(size_t)(3 * kKX + k) * kGF + pt];
            }
        }
        gridpoint_column(j, n1, g, Pext != nullptr, pu, pv, ptt, pq, [&](int f, double v) { B[i * kRowLd + f] = v; },
                         T);
    }
    __syncthreads();
    stamp(dbg, 0, 3);
    // specx: vdspec's x cosgr(j) on its inputs (spe_spectral.f90:430-445), rfftf
    if (tid < kNFwd) {
        double x[kFftN];
#pragma unroll
        for (int e = 0; e < kFftN; ++e) x[e] = tid < kNFwdScaled ? B[e * kRowLd + tid] * cj : B[e * kRowLd + tid];
        row_specx(x, vfm, was, tid, j);
    }
    __syncthreads();
    stamp(dbg, 0, 4);
}

// With GPU physics, one latitude row per block: the row kernel.  8 waves, two per SIMD.
// gridx of the row's 91 inverse transforms (the 50 level-j2 dynamics fields and
// phypar's 41 level-1 fields) on lane pairs; then waves 0-1 run the grid-point dynamics
// and products (one column per thread, F -> B), waves 2-3 phypar's moist part and
// vdifsc (one column per lane, its results handed over in B's spare columns), waves 4-6
// the longwave / surface chain -- on a shortwave step after the shortwave, whose cloud-free
// part they run while the moist side works, the rest after its hand-over -- on two lanes
// per column (sml_physics_pair.hpp), which then sum the
// tendencies into F (phys_column's sums, four levels per lane); then specx of the 73
// forward transforms (F + P where grtend adds it, x cosgr(j) for vdspec's inputs) on
// lane pairs straight into the m-major coefficients.  Every expression and sum order is
// phys_column's (the one-lane-per-column form it replaced bit for bit, r05).
constexpr int kGpThreads = 512;
__global__ __launch_bounds__(kGpThreads) void k_st_gridspec_p(
    const double *__restrict__ varm, double *__restrict__ vfm, const double *__restrict__ wa,
    const double *__restrict__ cosgr, const DynTables *__restrict__ T, const double *__restrict__ bc,
    double *__restrict__ rad, const PhysTables *__restrict__ PT, int lradsw, const uint64_t *__restrict__ go_src,
    uint64_t *__restrict__ go_dst, long long *dbg) {
    SML_TL_SCOPE(sml::tl::kRow);
    // the window's first row kernel in a graph that holds the entry: the entry's outputs
    // (the safety check's inputs) were released by k_io_entry's end, so the check may go
    // (a relaxed agent-scope vector store, as k_hop_signal)
    if (go_dst && blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_store(go_dst, *go_src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __shared__ double A[kFftN * kRowLd], B[kFftN * kRowLd];
    const double *was = kFftWa96;
    (void)wa;
    constexpr int kPtS = (int)(offsetof(PhysTables, fband) / sizeof(double)), kGpS = (int)(sizeof(GpTab) / 8);
    static_assert(kPtS + kGpS <= kGpThreads, "table staging: one value per thread");
    static_assert(kRowLd - kNFwd >= 24, "moist-side hand-over: 24 spare slots per column in B");
    __shared__ double ptl[kPtS];
    __shared__ GpTab gpt;
    __shared__ double fsr[4 * kIX];  // radlw(1)'s surface row per (column, band), sfc_fband
    constexpr int kMh = 3 + kKX;
    // a shortwave step's moist-part hand-over (precnv, precls, itop, rh); then the pair lanes' tt_rsw
    __shared__ double mhs[kIX * kMh];
    constexpr int n1 = kNInv1P;
    constexpr int nphys = (n1 - kPT1) + (kNInvP - (n1 + 2 * kKX + 2));  // 25 + 16 = 41
    const int j = blockIdx.x, tid = threadIdx.x;
    const bool isp = tid >= 256 && tid < 256 + 2 * kIX;  // the longwave side's pairs
    const int pi = isp ? (tid - 256) >> 1 : 0, ph_ = tid & 1, ppt = j * kIX + pi;
    // a longwave-only step's radiation state of the pair lane (bands 2h, 2h + 1, its levels)
    auto pair_pre_load = [&](PairPre &pre) {
        if (lradsw) return;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int k = 0; k < kKX; ++k)
                pre.tau[b][k] = rad[kRadTau2 + ((size_t)(2 * ph_ + b) * kKX + k) * kNGP + ppt];
        pre.strat0 = rad[kRadStratc + ppt];
        pre.strat1 = rad[kRadStratc + kNGP + ppt];
        pre.ssrd = rad[kRadSsrd + ppt];
#pragma unroll
        for (int s = 0; s < 4; ++s) pre.ttrsw[s] = rad[kRadTtRsw + (size_t)(4 * ph_ + s) * kNGP + ppt];
    };
    stamp(dbg, 0, 0);
    double rtab = 0.0;
    if (tid < kPtS) {
        rtab = reinterpret_cast<const double *>(PT)[tid];
    } else if (tid < kPtS + kGpS) {
        const int e = tid - kPtS, k = e % kKX;
        const int w = e / kKX;
        rtab = w == 0 ? T->dhs[k] : w == 1 ? T->dhsr[k] : w == 2 ? T->fsgr[k] : w == 3 ? T->tref[k]
             : w == 4 ? T->tref3[k] : T->coriol[e - 5 * kKX];
    }
    {
        const int t = tid >> 1, h = tid & 1;
        const bool act = t < kNInv + nphys;
        const int f = t < kNInv ? (t < kNInv1 ? t : n1 + (t - kNInv1))
                                : (t - kNInv < n1 - kPT1 ? kPT1 + (t - kNInv)
                                                         : n1 + 2 * kKX + 2 + (t - kNInv - (n1 - kPT1)));
        double xi[kMX2 - 1];
        if (act) row_gridx_load(varm, f, j, xi);
        if (tid < kPtS) ptl[tid] = rtab;
        else if (tid < kPtS + kGpS) reinterpret_cast<double *>(&gpt)[tid - kPtS] = rtab;
        __syncthreads();
        if (act) row_gridx_half(A, xi, was, f, false, 1.0, h);
        // the surface rows (two dependent loads), by the lanes gridx leaves idle
        for (int e = tid - 192; e >= 0 && e < 4 * kIX; e += kGpThreads - 192)
            fsr[e] = sfc_fband(bc, &PT->fband[0][0], j * kIX + (e >> 2), e & 3);
    }
    __syncthreads();
    stamp(dbg, 0, 1);
    const PhysTables *PTl = reinterpret_cast<const PhysTables *>(ptl);  // (fband stays in PT)
    const double cj = cosgr[j];
    PairOut po;
    SML_PST_T(8, 0);
    SML_PST_T(10, 128);
    SML_PST_T(14, 256);
    if (tid < kIX) {  // grid-point dynamics of column i -> F in B[i][f], then its products
        const int i = tid;
        auto g = [&](int f) { return f >= n1 ? A[i * kRowLd + f] * cj : A[i * kRowLd + f]; };
        double dummy[kKX];
        gridpoint_column(j, n1, g, false, dummy, dummy, dummy, dummy, [&](int f, double v) { B[i * kRowLd + f] = v; },
                         &gpt, false);
        // (the products below kNFwdScaled are vdspec inputs: x cosgr(j) here, not in specx)
        gridpoint_products(n1, g, [&](int f, double v) { B[i * kRowLd + f] = f < kNFwdScaled ? v * cj : v; }, &gpt);
        SML_PST_T(9, 0);
    }
    // the moist / diffusion part of column i's phypar (waves 2-3); on a shortwave step its
    // moist part's results go to the longwave side through mhs at a block barrier
    const bool ism = tid >= 128 && tid < 128 + kIX;
    const int mi = ism ? tid - 128 : 0;
    PhysThermo mth;
    double mtt[kKX], mqt[kKX], mph[kKX];
    int micnv = 0;
    if (ism) {
        const double *Ai = A + mi * kRowLd;
        double ta[kKX], qa[kKX];
#pragma unroll
        for (int k = 0; k < kKX; ++k) {
            ta[k] = Ai[kPT1 + k];
            qa[k] = Ai[kPQ1 + k];
            mph[k] = Ai[kPPhi1 + k];
        }
        phys_thermo(ta, qa, mph, Ai[kPPs1], PTl, mth);
        SML_PST_T(11, 128);
        double precnv, precls;
        int itop;
        phys_moist(mth, PTl, mtt, mqt, precnv, precls, itop, micnv);
        SML_PST_T(12, 128);
        if (lradsw) {
            double *m = mhs + mi * kMh;
            m[0] = precnv;
            m[1] = precls;
            m[2] = (double)itop;
#pragma unroll
            for (int k = 0; k < kKX; ++k) m[3 + k] = mth.rh[k];
        }
    }
    // a shortwave step's pair lanes, while the moist side works: what needs neither its
    // hand-over nor the cloud (they reached the barrier idle: 2.2 us of the step, 3.0 on
    // the tropical rows)
    PairSw psw;
    if (isp && lradsw) {
        phys_pair_sw_pre<kPT1, kPQ1, kPPhi1, kPPs1>(ph_, ppt, A + pi * kRowLd, bc, PTl, psw);
        SML_PST_T(21, 256);
    }
    if (lradsw) __syncthreads();
    if (ism) {
        double ttv[kKX], qtv[kKX];
        phys_vdif(mth, mph, micnv, PTl, ttv, qtv);
        double *Bh = B + mi * kRowLd + kNFwd;
        // tt[0] is +0 always (convection and condensation leave the top level alone)
#pragma unroll
        for (int k = 1; k < kKX; ++k) Bh[k - 1] = mtt[k];
#pragma unroll
        for (int k = 0; k < kKX; ++k) Bh[7 + k] = ttv[k];
#pragma unroll
        for (int k = 0; k < kKX - 1; ++k) Bh[15 + k] = mqt[k] + qtv[k];  // final above the surface layer
        Bh[22] = mqt[kKX - 1];
        Bh[23] = qtv[kKX - 1];
        SML_PST_T(13, 128);
    } else if (isp) {  // the longwave / surface chain (and the shortwave) of column pi, two lanes
        // (pair_pre_load before gridx instead: the gridx lanes' registers spilled, gridx 3.3 -> 3.9 us)
        const double *Ai = A + pi * kRowLd;
        const double u7 = Ai[n1 + 2 * kKX + 2 + kKX - 1] * cj, v7 = Ai[n1 + 3 * kKX + 2 + kKX - 1] * cj;
        const double fs2[2] = {fsr[4 * pi + 2 * ph_], fsr[4 * pi + 2 * ph_ + 1]};
        phys_pair<kPT1, kPQ1, kPPhi1, kPPs1>(ph_, ppt, j, Ai, u7, v7, pair_pre_load, bc, rad, PTl,
                                             &PT->fband[0][0], fs2, mhs + pi * kMh, lradsw != 0, psw, po);
        SML_PST_T(18, 256);
        SML_PST_T(19, 384);
    }
    __syncthreads();
    SML_PST_T(20, 256);
    if (isp) {  // phys_column's sums (phy_phypar.f90:174-196), the pair lane's four levels
        const double *Bh = B + pi * kRowLd + kNFwd;
        const double *Mh = mhs + pi * kMh;  // the lane's levels of the shortwave heating (phys_pair)
        double *Bi = B + pi * kRowLd;
        const double rps = po.rps;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = 4 * ph_ + s;
            const double ttk = (k == 0 ? 0.0 : Bh[k > 0 ? k - 1 : 0]) + Mh[4 * ph_ + s] + po.rlw[s];
            double ttv = Bh[7 + k], utv = 0., vtv = 0.;
            double qtk;
            if (k == kKX - 1) {
                utv = utv + po.ust * rps * PTl->grdsig[kKX - 1];
                vtv = vtv + po.vst * rps * PTl->grdsig[kKX - 1];
                ttv = ttv + po.shf * rps * PTl->grdscp[kKX - 1];
                const double qtv = Bh[23] + po.evp * rps * PTl->grdsig[kKX - 1];
                qtk = Bh[22] + qtv;
            } else {
                qtk = Bh[15 + k];
            }
            // F + P where grtend adds phypar's tendencies (u 0..7, v 24..31, t 56..63, q 64..71)
            Bi[k] = (Bi[k] + (0. + utv)) * cj;  // (x cosgr(j): a vdspec input, scaled here for specx)
            Bi[3 * kKX + k] = (Bi[3 * kKX + k] + (0. + vtv)) * cj;
            Bi[7 * kKX + k] = Bi[7 * kKX + k] + (ttk + ttv);
            Bi[8 * kKX + k] = Bi[8 * kKX + k] + qtk;
        }
    }
    __syncthreads();
    stamp(dbg, 0, 2);
    // specx: transform f on lanes 2 f, 2 f + 1, lane h on the samples 2 i + h
    {
        const int f = tid >> 1, h = tid & 1;
        const bool act = f < kNFwd;
        double x[48];
        if (act) {
            const double *fr = B + f + h * kRowLd;
#pragma unroll
            for (int i = 0; i < 48; ++i) x[i] = fr[2 * i * kRowLd];
            fft::rfftf48_reg(x, was);
        }
        __syncthreads();  // A's P columns are read: A becomes the pairs' meeting place
        row_specx_pair(x, A, act, vfm, was, f, j, h);
    }
    stamp(dbg, 0, 3);
}

// specy's MFMA B operands in lane order: lane l = 16 kk + r of k-step s takes
// pfwd[m][n][j] at n = 2 r (S) and 2 r + 1 (D), j = 4 s + kk ([m][n 32][lat 24], the
// spectral context's forward Legendre table) -> pfl[m][s][l][2]
__global__ void k_pack_pfwd(const double *__restrict__ pfwd, double *__restrict__ pfl) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= kMX * (kIY / 4) * 64) return;
    const int l = e % 64, s = (e / 64) % (kIY / 4), m = e / (64 * (kIY / 4));
    const int r = l & 15, kk = l >> 4, j = 4 * s + kk;
    const double *pm = pfwd + (size_t)m * kNX * kIY;
    pfl[2 * (size_t)e] = pm[(2 * r) * kIY + j];
    pfl[2 * (size_t)e + 1] = pm[(2 * r + 1) * kIY + j];
}

// one zonal wavenumber m: specy of the 73 forward transforms, combine and tail of
// the m's 64 real coefficients x 8 levels (one thread each) on the m's state slice
// in LDS; with next_j2 > 0 the new state feeds the next step's inverse transforms
__global__ __launch_bounds__(kSpecBlk) void k_st_spec(
    const double *__restrict__ vfm, const double *__restrict__ pfl, const double *__restrict__ wt,
    const double *__restrict__ sm, double *__restrict__ sm_out, double *__restrict__ Td, double *__restrict__ phi_out,
    const double *__restrict__ phis,
    const double *__restrict__ tcorh, const double *__restrict__ qcorh, const DynTables *__restrict__ T, int j1,
    int j4, double dt, double alph, double rob, double wil, const double *__restrict__ pinv,
    double *__restrict__ varm_next, int next_j2, int n1, int nin, const double *__restrict__ tabm,
    double *__restrict__ state_out, double *__restrict__ io_varm, long long *dbg) {
    SML_TL_SCOPE(sml::tl::kSpec);
    __shared__ double V[kVFm];            // this m's tables (TabM)
    __shared__ double S[kNInvMax * kCW];  // specy output [f][2 n + p]; then the next step's inputs
    __shared__ double sh[3][kKX][kCW];
    __shared__ double Sst[kSM];           // this m's state, updated in place
    __shared__ double Fm[3 * kCW];        // phis, tcorh, qcorh of this m
    // kSpecSplit blocks per m: each repeats the m's specy, combine and tail (on CUs that
    // would idle), and takes its share of the next step's gridy tiles; the lead block
    // (half 0) alone writes the state, phi and the stamps
    const int m = blockIdx.x % kSpecStride, half = blockIdx.x / kSpecStride;
    if (m >= kMX) return;  // (block-uniform: the grid's idle blocks)
    const bool lead = half == 0;
    if (!lead) dbg = nullptr;
    const int wave = wave_index(), l = threadIdx.x & 63, r = l & 15, kk = l >> 4;
    const int sk = next_j2 > 0 ? 1 : 3;
    stamp(dbg, sk, 0);
    // a) specy (k_specy's tiling: 8 fields x Re/Im per wave), the wave's A operands
    // read from vfm [lat][f][p] (per instruction 4 latitudes x 128 contiguous bytes)
    const double *vm = vfm + (size_t)m * kVFm;
    // at most two tiles per wave (10 tiles, 8 waves): both tiles' loads are issued
    // before the first MFMA, so the second tile costs no memory round trip of its own
    constexpr int kTiles = (kNFwd + 7) / 8, kWaves = kSpecBlk / 64;
    static_assert(kTiles <= 2 * kWaves, "specy: two tiles per wave at most");
    static_assert(kTiles - kWaves <= kWaves / 2, "specy: the waves with two tiles are among those that load first");
    auto tile_load = [&](int tile, double (&vn)[kIY / 4], double (&vs)[kIY / 4]) {
        const int fa = tile * 8 + (r >> 1);
        const double *vr = vm + (fa < kNFwd ? fa : 0) * 2 + (r & 1);
#pragma unroll
        for (int s = 0; s < kIY / 4; ++s) {
            const int j = 4 * s + kk;
            vn[s] = vr[(kIL - 1 - j) * kVLs];
            vs[s] = vr[j * kVLs];
        }
    };
    double vn0[kIY / 4], vs0[kIY / 4], vn1[kIY / 4], vs1[kIY / 4];
    const bool two = wave + kWaves < kTiles;  // wave-uniform
    constexpr int RT = (kTabMDoubles / 2 + kSpecBlk - 1) / kSpecBlk;
    // three named registers, not an array: held across specy, an array was kept in scratch
    static_assert((RT == 2 || RT == 3) && 2 * RT * kSpecBlk <= kVFm && 2 * RT * kSpecBlk - kTabMDoubles <= kTabMPad,
                  "TabM staging");
    double2 rt0, rt1, rt2 = {0.0, 0.0};
    // Load order.  The m's state slice, tables and forcing and specy's B operands -- all
    // same-XCD L2 hits -- are issued first, the pinv slice after them.  Vector loads return
    // in order, so the kernel waits on the first group alone (a counted vmcnt), stages it
    // in LDS and runs the state-only half of the tail (tail_pre) before specy.  The
    // prologue is bound by the issue of its loads -- the CU takes one vector-memory
    // instruction of a wave per about 16 clocks; the Fourier tiles alone are 120 per
    // block, 0.8 us -- and a wave that issues does nothing else.  So the row kernel's
    // Fourier coefficients (tile_load) are issued behind the staging barrier in two
    // orders: waves 0..3 load their tiles and then run tail_pre, waves 4..7 (the other
    // wave of each SIMD) run tail_pre and then load: one half's f64 chains fill the other
    // half's issue time.  (Every wave loading first, in front of the barrier or behind
    // it: the kernel 0.2 us slower than / as long as with the tail in one piece,
    // profiles/spec_kernel_pretail.md.)
    constexpr int NS = kSM / 2, RS = (NS + kSpecBlk - 1) / kSpecBlk;
    static_assert(RS == 5 && NS % kSpecBlk == 0, "state staging: five whole rows of the block");
    double2 rs0, rs1, rs2, rs3, rs4;  // named registers (an array held across specy went to scratch)
    {
        const double2 *ss = reinterpret_cast<const double2 *>(sm + (size_t)m * kSM) + threadIdx.x;
        rs0 = ss[0];
        rs1 = ss[kSpecBlk];
        rs2 = ss[2 * kSpecBlk];
        rs3 = ss[3 * kSpecBlk];
        rs4 = ss[4 * kSpecBlk];
        // this m's tables (into V's space); past the slice: the next m's table or
        // d_tabm's tail pad (unused)
        const double2 *t = reinterpret_cast<const double2 *>(tabm + (size_t)m * kTabMDoubles) + threadIdx.x;
        rt0 = t[0];
        rt1 = t[kSpecBlk];
        if constexpr (RT > 2) rt2 = t[2 * kSpecBlk];
    }
    // the m's forcing (load_forcing_m's elements, one per thread)
    double rf = 0.0;
    if (threadIdx.x < 3 * kCW) {
        const int which = threadIdx.x / kCW, cf = threadIdx.x % kCW;
        const double *src = which == 0 ? phis : which == 1 ? tcorh : qcorh;
        rf = src[ci(cf & 1, m, cf >> 1)];
    }
    // specy's B operands: every wave's tiles use this m's Legendre columns of its lanes,
    // packed in lane order (k_pack_pfwd), and the same Gaussian weights.  They are the same
    // for all eight waves, so the block loads them once -- one 16-B piece of the 6 KB per
    // thread of the first six waves, the 24 weights by 24 lanes -- and stages them in V
    // behind the pinv slice; each wave reads its operands from LDS in front of its MFMAs.
    // (Loaded by every wave they were 96 of the 171 vector-memory instructions in
    // front of the tiles' loads, and the prologue is bound by their issue.)
    constexpr int kPinvM = kNX * 32, kVPinv = 2 * RT * kSpecBlk;
    constexpr int kPflM = 2 * (kIY / 4) * 64, kVPfl = kVPinv + kPinvM, kVWt = kVPfl + kPflM;
    static_assert(kPinvM == 2 * kSpecBlk && kVPinv % 2 == 0, "pinv slice staging in V");
    static_assert(kPflM / 2 <= kSpecBlk && kIY <= 64 && kVWt + kIY <= kVFm, "Legendre columns and weights staged in V");
    double2 rl = {0.0, 0.0};
    double rw = 0.0;
    if (threadIdx.x < kPflM / 2)
        rl = reinterpret_cast<const double2 *>(pfl)[(size_t)m * (kPflM / 2) + threadIdx.x];
    if (threadIdx.x < kIY) rw = wt[threadIdx.x];
    // (the scheduler would otherwise be free to sink these loads below specy's)
    __builtin_amdgcn_sched_barrier(0);
    // gridy's Legendre slice of this m (8 KB, one 16-B load per thread), staged in V
    // behind the tables: each wave then reads its MFMA operands from LDS instead of
    // every wave fetching the same 8 KB from memory in the gridy phase
    const double2 rp = reinterpret_cast<const double2 *>(pinv + (size_t)m * kPinvM)[threadIdx.x];
    // (these loads stay ahead of the first wait)
    __builtin_amdgcn_sched_barrier(0);
    if (dbg) __syncthreads();
    stamp(dbg, sk, 1);
    // (stamps: "load", 0 to 1, is the issue of the loads above; the staging, tail_pre and
    // the tiles' loads fall into "specy", 1 to 2; "tail", 3 to 4, is tail_post alone)
    // state, tables, forcing and specy's B operands into LDS: the wait in front of these
    // stores leaves the pinv slice outstanding
    TabM *tm = reinterpret_cast<TabM *>(V);
    {
        double2 *v2 = reinterpret_cast<double2 *>(V) + threadIdx.x;  // (V holds kVFm >= 2 RT kSpecBlk doubles)
        v2[0] = rt0;
        v2[kSpecBlk] = rt1;
        if constexpr (RT > 2) v2[2 * kSpecBlk] = rt2;
        double2 *s2 = reinterpret_cast<double2 *>(Sst) + threadIdx.x;
        s2[0] = rs0;
        s2[kSpecBlk] = rs1;
        s2[2 * kSpecBlk] = rs2;
        s2[3 * kSpecBlk] = rs3;
        s2[4 * kSpecBlk] = rs4;
        if (threadIdx.x < 3 * kCW) Fm[threadIdx.x] = rf;
        if (threadIdx.x < kPflM / 2) reinterpret_cast<double2 *>(V + kVPfl)[threadIdx.x] = rl;
        if (threadIdx.x < kIY) V[kVWt + threadIdx.x] = rw;
    }
    __syncthreads();  // Sst, Fm, the tables, the Legendre columns and weights complete
    const LTab tb{tm};
    static_assert(kSpecBlk == kSpecThreads, "k_st_spec: one thread per (coefficient, level), none idle in the tail");
    const int cc = threadIdx.x & (kCW - 1), k = wave;
    const int n = cc >> 1, p = cc & 1;
    const int c = ci(p, m, n);
    // c0) the tail's state-only half.  The whole m's state is in LDS, so the other levels'
    // div and t are read from Sst directly: no copy into sh, no second barrier.  Sst is
    // next written by tail_post's timint, behind the barrier that follows specy.
    auto SA = [&](int var, int lev, int kk2) -> double & { return Sst[smi(var, lev, kk2, cc)]; };
    const bool loads_first = wave < kWaves / 2;  // wave-uniform: the two waves of a SIMD take opposite orders
    if (loads_first) {
        tile_load(wave, vn0, vs0);
        if (two) tile_load(wave + kWaves, vn1, vs1);
    }
    __builtin_amdgcn_sched_barrier(0);
    const TailPre pre = tail_pre<true>(SA, [&](int v, int kk2) { return Sst[smi(1 + v, j4, kk2, cc)]; },
                                       lead && next_j2 <= 0 ? phi_out : nullptr, Fm, Fm + kCW, Fm + 2 * kCW, cc, tb, k,
                                       c, m, n, j4);
    // (tail_pre stays ahead of the other waves' loads, of specy's wait and of its MFMAs)
    __builtin_amdgcn_sched_barrier(0);
    if (!loads_first) tile_load(wave, vn0, vs0);  // (one tile: static_assert above)
    __builtin_amdgcn_sched_barrier(0);
    double wv[kIY / 4], bS[kIY / 4], bD[kIY / 4];
#pragma unroll
    for (int s = 0; s < kIY / 4; ++s) {
        const double2 b = reinterpret_cast<const double2 *>(V + kVPfl)[s * 64 + l];
        wv[s] = V[kVWt + 4 * s + kk];
        bS[s] = b.x;
        bD[s] = b.y;
    }
    auto tile_mma = [&](int tile, const double (&vn)[kIY / 4], const double (&vs)[kIY / 4]) {
        const int f0 = tile * 8;
        // the lanes of fields >= kNFwd (the last tile's) loaded field 0 (tile_load: in
        // bounds, finite) and their operands are not zeroed: they are rows of the MFMA's A
        // operand, output row i depends on A's row i alone, and those rows are skipped at
        // the stores below -- they can reach no stored value
        d4 accS = {0, 0, 0, 0}, accD = accS;
#pragma unroll
        for (int s = 0; s < kIY / 4; ++s) {
            const double aS = (vn[s] + vs[s]) * wv[s];
            const double aD = (vn[s] - vs[s]) * wv[s];
            accS = MFMA64(aS, bS[s], accS);
            accD = MFMA64(aD, bD[s], accD);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = kk + 4 * q;
            const int f = f0 + (row >> 1);
            if (f >= kNFwd) continue;
            S[f * kCW + 2 * (2 * r) + (row & 1)] = accS[q];
            S[f * kCW + 2 * (2 * r + 1) + (row & 1)] = accD[q];
        }
    };
    tile_mma(wave, vn0, vs0);
    if (two) tile_mma(wave + kWaves, vn1, vs1);
    reinterpret_cast<double2 *>(V + kVPinv)[threadIdx.x] = rp;  // (behind the tables: no reader before gridy)
    __syncthreads();  // S and the pinv slice complete
    stamp(dbg, sk, 2);
    // b) combine (k_dyn_combine) for coefficient (n, p) at level k: every thread of the
    // block holds one, k the wave's index (wave-uniform)
    auto fl = [&](int f) { return [=](int pp, int nn) { return S[f * kCW + 2 * nn + pp]; }; };
    double vo = 0.0, dv = 0.0, d0 = 0.0, dq = 0.0, dummy;
    vds_gen(fl(k), fl(3 * kKX + k), tb, n, p, &vo, &dv);  // vdspec(utend, vtend)
    const double lapv = -(fl(6 * kKX + k)(p, n) * tb.el2_n(n));
    vds_gen(fl(kKX + k), fl(4 * kKX + k), tb, n, p, &dummy, &d0);      // vdspec(-u tgg, -v tgg)
    vds_gen(fl(2 * kKX + k), fl(5 * kKX + k), tb, n, p, &dummy, &dq);  // vdspec(-u trg, -v trg)
    const double psdt = (m == 0 && n == 0) ? 0.0 : fl(kNFwd - 1)(p, n);
    const double tdt0 = d0 + fl(7 * kKX + k)(p, n), trdt0 = dq + fl(8 * kKX + k)(p, n);
    if (dbg) {
        __syncthreads();
        stamp(dbg, sk, 3);
    }
    // c) the tail's other half: sptend's corrections / implic / diffusion / time
    // integration on the LDS state
    tail_post<kCW>(SA, pre, lead ? Td : nullptr, tb, sh, cc, k, c, m, n, vo, dv - lapv, tdt0, trdt0, psdt, j1, dt, alph,
                   rob, wil);
    __syncthreads();  // S is free, Sst complete
    stamp(dbg, sk, 4);
    if (next_j2 <= 0) {  // the run of fused steps ends: the state straight into the reference layout
        if (!lead) return;  // block-uniform
        for (int i = threadIdx.x; i < kSM; i += kSpecBlk) put_state(state_out, m, i, Sst[i]);
        if (io_varm) {  // run_model: iogrid(31)'s k_io_prep + gridy of this m (block-uniform)
            io_prep_m(Sst, tb, k, cc, [&](int f, double v) { S[f * kCW + cc] = v; });
            __syncthreads();
            gridy_io(S, gridy_operands_slice(V + kVPinv), io_varm, m, kNIo);
        }
        return;  // block-uniform
    }
    if (lead) {  // into the other buffer: this m's second block may still be reading sm
        // (five whole rows of the block, static_assert above: the LDS reads issue together)
        const double2 *src = reinterpret_cast<const double2 *>(Sst) + threadIdx.x;
        double2 v[RS];
#pragma unroll
        for (int q = 0; q < RS; ++q) v[q] = src[q * kSpecBlk];
#pragma unroll
        for (int q = 0; q < RS; ++q)
            store2(sm_out, (size_t)m * kSM + 2 * ((size_t)q * kSpecBlk + threadIdx.x), v[q].x, v[q].y);
    }
    // d) the next step's inverse-transform inputs (k_dyn_prep) and gridy
    inv_inputs(Sst, S, Fm, tb, m, next_j2, n1, nin);
    __syncthreads();
    stamp(dbg, sk, 5);
    {
        const int nt = (nin + 7) / 8, per = (nt + kSpecSplit - 1) / kSpecSplit;
        gridy_m(S, gridy_operands_slice(V + kVPinv), varm_next, m, nin, half * per, min(nt, (half + 1) * per));
    }
    if (dbg) {  // (diagnostics only: the kernel ends here)
        __syncthreads();
        stamp(dbg, sk, 6);
    }
}

}  // namespace
