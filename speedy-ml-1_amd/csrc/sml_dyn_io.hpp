// sml_dyn_io.hpp -- iogrid(30 / 31) and run_model's hand-offs: k_io_combine,
// k_io_prep, the fused window entry k_io_entry, the safety check's k_io_minmax and
// k_check_go, and the one-lane stores k_flag_store*, k_set_xa.
// (A timeline build, SML_TL, needs the unit's SML_TL_DEFINE ahead of this header.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sml_dyn_fused.hpp"
#include "sml_dyn_layout.hpp"
#include "sml_dyn_spec_math.hpp"
#include "sml_dynamics_tables.hpp"
#include "sml_spectral_internal.hpp"
#include "sml_timeline.hpp"

namespace {
using namespace sml;

// ------------------------------------------------------------ iogrid(30/31)
// ppo_iogrid.f90:497-601.  grid4d = variables3d(4, ix, il, kx) (T, u, v, q), logp(ix, il).
// Field-major work layout of both directions: [u 8 | v 8 | t 8 | q 8 | ps] (33 fields).


// entry: vdspec's vds + spec, trunct, into time level 1 (:524-538)
__global__ void k_io_combine(const double *__restrict__ S, double *__restrict__ st, const DynTables *__restrict__ T) {
    const int mn = blockIdx.x * blockDim.x + threadIdx.x;
    if (mn >= kMN) return;
    const int k = blockIdx.y;
    const int m = mn % kMX, n = mn / kMX;
    const double trf = T->trfilt[n][m];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int c = ci(p, m, n);
        double vo, dv;
        vds_at(S + (size_t)k * kSF, S + (size_t)(kKX + k) * kSF, T, m, n, p, &vo, &dv);
        st[kOffVor + (size_t)k * kSF + c] = vo * trf;
        st[kOffDiv + (size_t)k * kSF + c] = dv * trf;
        st[kOffT + (size_t)k * kSF + c] = S[(size_t)(2 * kKX + k) * kSF + c] * trf;
        st[kOffTr + (size_t)k * kSF + c] = S[(size_t)(3 * kKX + k) * kSF + c] * trf;
        if (k == 0) st[kOffPs + c] = S[(size_t)(4 * kKX) * kSF + c] * trf;
    }
}

// both directions: inverse-transform inputs from level 1 (:541-553 / :576-589):
// [ucos 8 | vcos 8 | t 8 | q 8 | ps]
__global__ void k_io_prep(const double *__restrict__ st, double *__restrict__ sin_, const DynTables *__restrict__ T) {
    const int mn = blockIdx.x * blockDim.x + threadIdx.x;
    if (mn >= kMN) return;
    const int k = blockIdx.y;
    const int m = mn % kMX, n = mn / kMX;
    const double *vor = st + kOffVor + (size_t)k * kSF, *div = st + kOffDiv + (size_t)k * kSF;
    uvspec_at(vor, div, T, m, n, sin_ + (size_t)k * kSF, sin_ + (size_t)(kKX + k) * kSF);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int c = ci(p, m, n);
        sin_[(size_t)(2 * kKX + k) * kSF + c] = st[kOffT + (size_t)k * kSF + c];
        sin_[(size_t)(3 * kKX + k) * kSF + c] = st[kOffTr + (size_t)k * kSF + c];
        if (k == 0) sin_[(size_t)(4 * kKX) * kSF + c] = st[kOffPs + c];
    }
}

// run_model's window entry in one launch per zonal wavenumber m (512 threads = 64
// coefficients x 8 levels), after iogrid(30)'s specx: the same operations as
//   specy (k_specy's tiling)  -> k_io_combine (vds / spec + trunct into level 1)
//   -> k_io_prep (the safety check's inputs) -> k_state_to_m -> k_st_inv (the first
//   step's inverse inputs + gridy)
// which all stay inside one m.  vio: the io Fourier coefficients, kNIo fields in the
// spectral module's layout; state: reference layout, level 1 written, level 2 read
// into the m-major slice sm; chk: k_io_prep's output; varm: gridy for step(1, 1).
__global__ __launch_bounds__(kSpecThreads) void k_io_entry(const double *__restrict__ vio,
                                                           const double *__restrict__ pfl,
                                                           const double *__restrict__ wt, double *__restrict__ state,
                                                           double *__restrict__ sm, double *__restrict__ chk,
                                                           const double *__restrict__ phis,
                                                           const double *__restrict__ tabm,
                                                           const double *__restrict__ pinv, double *__restrict__ varm,
                                                           int n1, int nin, uint64_t *__restrict__ xa, uint64_t xa0,
                                                           uint64_t xa1) {
    SML_TL_SCOPE(sml::tl::kIoEntry);
    // a graph-captured exit's per-launch values (sml_dyn_run_model): ordered before the
    // window graph by this kernel's end
    if (xa && blockIdx.x == 0 && threadIdx.x == 0) {
        xa[0] = xa0;
        xa[1] = xa1;
    }
    __shared__ double S[kNIo * kCW];  // specy output [f][2 n + p]
    __shared__ double Sst[kSM];       // this m's state slice
    __shared__ double In[kNInvMax * kCW];
    __shared__ double Fm[kCW];
    constexpr int RT = (kTabMDoubles / 2 + kSpecThreads - 1) / kSpecThreads;
    __shared__ double V[2 * RT * kSpecThreads];  // this m's tables (TabM), staged as k_st_spec does
    const int m = blockIdx.x, tid = threadIdx.x;
    // (wave: also the level k of the thread's coefficient, wave-uniform)
    const int wave = wave_index(), l = tid & 63, r = l & 15, kk = l >> 4;
    // every global load of the entry is issued before the first wait (one memory round
    // trip): level 2 of the slice (k_state_to_m), phis(m), specy's operands and
    // gridy's Legendre columns.  Element i = tid + 512 q of the slice has lev = q % 2,
    // var = q / 2, k = tid / 64, cc = tid % 64.
    constexpr int kSI = kSM / kSpecThreads;
    static_assert(kSM % kSpecThreads == 0 && kSI == 10, "slice staging: ten rows of the block");
    double s2[kSI / 2];
#pragma unroll
    for (int q = 1; q < kSI; q += 2) {  // level 2 (lev index 1); level 1 comes from the combine
        const int cc = tid % kCW, k = wave, var = q / 2;
        const int c = ci(cc & 1, m, cc >> 1);
        double v = 0.0;
        if (var < 4) {
            const size_t off = var == 0 ? kOffVor : var == 1 ? kOffDiv : var == 2 ? kOffT : kOffTr;
            v = state[off + ((size_t)kKX + k) * kSF + c];
        } else if (k == 0) {
            v = state[kOffPs + (size_t)kSF + c];
        }
        s2[q / 2] = v;
    }
    const double phis_m = tid < kCW ? phis[ci(tid & 1, m, tid >> 1)] : 0.0;
    static_assert(2 * RT * kSpecThreads - kTabMDoubles <= kTabMPad, "TabM staging");
    double2 rt[RT];
    {
        const double2 *t = reinterpret_cast<const double2 *>(tabm + (size_t)m * kTabMDoubles) + tid;
#pragma unroll
        for (int q = 0; q < RT; ++q) rt[q] = t[q * kSpecThreads];
    }
    // a) specy of the io fields (k_specy: a wave per 8 fields x Re/Im)
    const bool spw = wave < (kNIo + 7) / 8;  // wave-uniform
    const int f0 = wave * 8, fa = f0 + (r >> 1);
    const bool ok = spw && fa < kNIo;
    double vn[kIY / 4], vs[kIY / 4], wv[kIY / 4], bS[kIY / 4], bD[kIY / 4];
    if (spw) {
        const double *vr = vio + (size_t)(ok ? fa : 0) * kVarmField + 2 * m + (r & 1);
        const double2 *pl = reinterpret_cast<const double2 *>(pfl) + (size_t)m * (kIY / 4) * 64 + l;
#pragma unroll
        for (int s = 0; s < kIY / 4; ++s) {
            const int j = 4 * s + kk;
            vn[s] = vr[(kIL - 1 - j) * kMX2];
            vs[s] = vr[j * kMX2];
            wv[s] = wt[j];
            const double2 b = pl[s * 64];  // the packed B operands (k_pack_pfwd)
            bS[s] = b.x;
            bD[s] = b.y;
        }
    }
    const GridyB gb = gridy_operands(pinv, m);
    __builtin_amdgcn_sched_barrier(0);
    // (the table stores first, in the loads' own block: behind a branch the loads
    // were sunk next to them, after the first wait)
#pragma unroll
    for (int q = 0; q < RT; ++q) reinterpret_cast<double2 *>(V)[tid + q * kSpecThreads] = rt[q];
#pragma unroll
    for (int q = 1; q < kSI; q += 2) Sst[tid + kSpecThreads * q] = s2[q / 2];
    if (tid < kCW) Fm[tid] = phis_m;
    if (spw) {
        d4 accS = {0, 0, 0, 0}, accD = accS;
#pragma unroll
        for (int s = 0; s < kIY / 4; ++s) {
            // (fields >= kNIo: field 0's values, not zeroed -- rows of the A operand whose
            // output rows are skipped at the stores below, as in k_st_spec's specy)
            const double aS = (vn[s] + vs[s]) * wv[s];
            const double aD = (vn[s] - vs[s]) * wv[s];
            accS = MFMA64(aS, bS[s], accS);
            accD = MFMA64(aD, bD[s], accD);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = kk + 4 * q;
            const int f = f0 + (row >> 1);
            if (f >= kNIo) continue;
            S[f * kCW + 2 * (2 * r) + (row & 1)] = accS[q];
            S[f * kCW + 2 * (2 * r + 1) + (row & 1)] = accD[q];
        }
    }
    __syncthreads();
    // b) k_io_combine: vdspec's vds + spec, trunct, into level 1 (ppo_iogrid.f90:524-538)
    const LTab tb{reinterpret_cast<const TabM *>(V)};
    const int cc = tid & (kCW - 1), k = wave, n = cc >> 1, p = cc & 1, c = ci(p, m, n);
    {
        auto fl = [&](int f) { return [=](int pp, int nn) { return S[f * kCW + 2 * nn + pp]; }; };
        const double trf = tb.trfilt_n(n);
        double vo, dv;
        vds_gen(fl(k), fl(kKX + k), tb, n, p, &vo, &dv);
        const double v0 = vo * trf, v1 = dv * trf, v2 = S[(2 * kKX + k) * kCW + cc] * trf,
                     v3 = S[(3 * kKX + k) * kCW + cc] * trf;
        Sst[smi(0, 1, k, cc)] = v0;
        Sst[smi(1, 1, k, cc)] = v1;
        Sst[smi(2, 1, k, cc)] = v2;
        Sst[smi(3, 1, k, cc)] = v3;
        state[kOffVor + (size_t)k * kSF + c] = v0;
        state[kOffDiv + (size_t)k * kSF + c] = v1;
        state[kOffT + (size_t)k * kSF + c] = v2;
        state[kOffTr + (size_t)k * kSF + c] = v3;
        if (k == 0) {
            const double v4 = S[(4 * kKX) * kCW + cc] * trf;
            Sst[smi(4, 1, 0, cc)] = v4;
            state[kOffPs + c] = v4;
        } else {
            Sst[smi(4, 1, k, cc)] = 0.0;  // ps lives at k = 0 only (k_state_to_m)
        }
    }
    __syncthreads();
    // c) k_io_prep: uvspec of level 1 and copies -> the safety check's inputs
    {
        double a, b;
        uvspec_sel(Sst, tb, 1, k, n, p, &a, &b);
        chk[(size_t)k * kSF + c] = a;
        chk[(size_t)(kKX + k) * kSF + c] = b;
        chk[(size_t)(2 * kKX + k) * kSF + c] = Sst[smi(2, 1, k, cc)];
        chk[(size_t)(3 * kKX + k) * kSF + c] = Sst[smi(3, 1, k, cc)];
        if (k == 0) chk[(size_t)(4 * kKX) * kSF + c] = Sst[smi(4, 1, 0, cc)];
    }
    // d) the m-major slice for the window's first k_st_spec (k_state_to_m; whole rows
    // of the block, the LDS reads issued together)
    {
        static_assert(kSM / 2 % kSpecThreads == 0, "slice rows");
        constexpr int R = kSM / 2 / kSpecThreads;
        double2 *dst = reinterpret_cast<double2 *>(sm + (size_t)m * kSM) + tid;
        const double2 *src = reinterpret_cast<const double2 *>(Sst) + tid;
        double2 v[R];
#pragma unroll
        for (int q = 0; q < R; ++q) v[q] = src[q * kSpecThreads];
#pragma unroll
        for (int q = 0; q < R; ++q) dst[q * kSpecThreads] = v[q];
    }
    // e) k_st_inv: step(1, 1)'s inverse inputs (j2 = 1) and gridy
    inv_inputs(Sst, In, Fm, tb, m, 1, n1, nin);
    __syncthreads();
    gridy_m(In, gb, varm, m, nin);
}

// entry safety check (:556-571): min / max of the re-gridded u, v, t, q.  One
// block of 1024 threads per variable.
// NaN-sticky min / max (fmin / fmax would drop a NaN; a blown-up state must not
// pass the check, io_state_safe)
__device__ inline double nmin(double a, double b) { return (a != a || b != b) ? __builtin_nan("") : (b < a ? b : a); }
__device__ inline double nmax(double a, double b) { return (a != a || b != b) ? __builtin_nan("") : (b > a ? b : a); }

// cnt (may be null): the hand-off counter the run_model exit polls -- each block stores
// its min / max sc1, drains its stores and adds 1 (MI355X_MICROARCH.md, inter-workgroup
// visibility: an agent-scope atomic add per storing workgroup, sc1 stores and loads)
// the hybrid loop's forecast hop behind run_model's exit: one relaxed agent-scope
// vector store of the hop's sequence number, xa[1] (the exit's stores were released by
// its kernel's end; as sml_hybrid's k_hop_signal)
__global__ void k_flag_store_value(uint64_t *flag, uint64_t v) {
    SML_TL_SCOPE(sml::tl::kExitStore);
    if (threadIdx.x == 0) __hip_atomic_store(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// a graph-captured run_model's per-launch values (the window graphs, sml_dynamics::d_xa),
// launched right before the graph on its stream: behind the previous window, off the
// chain (the graph's entry waits for its grid anyway)
__global__ void k_set_xa(uint64_t *xa, uint64_t v0, uint64_t v1, uint64_t v2, uint64_t v3) {
    if (threadIdx.x == 0) {
        xa[0] = v0;
        xa[1] = v1;
        xa[2] = v2;
        xa[3] = v3;
    }
}

// the safety check's go on its own stream when the entry is inside the window graph:
// one lane polls *go (stored by the window's first row kernel) and acquires at agent
// scope; the check's kernels follow on the stream.  Never spins forever: on a timeout it
// marks *late with late_value (the exit's target for this check, so sml_dyn_last_safe
// fails this window) and the check reads whatever d_chk holds.  The give-up time is
// tested before each poll, so a zero give-up time gives up at once whichever of this
// kernel and the window's first row kernel -- dispatched side by side -- starts first
// (polled first, it gave up only while the row kernel was the slower one to start, which
// a row kernel without scratch no longer is)
__global__ void k_check_go(const uint64_t *go, uint64_t want, unsigned *late, unsigned late_value, long long timeout) {
    if (threadIdx.x != 0) return;
    const long long t0 = wall_clock64();
    for (;;) {
        if (wall_clock64() - t0 >= timeout) {
            __hip_atomic_store(late, late_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
        if (__hip_atomic_load(go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want) break;
        __builtin_amdgcn_s_sleep(2);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

__global__ void k_flag_store(uint64_t *flag, const uint64_t *xa) {
    SML_TL_SCOPE(sml::tl::kExitStore);
    if (threadIdx.x == 0) __hip_atomic_store(flag, xa[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// late / self: a check whose go hand-off gave up (k_check_go stored self into *late)
// reports NaN, so the exit takes the window as unsafe instead of trusting inputs the
// entry may not have written yet
__global__ __launch_bounds__(1024) void k_io_minmax(const double *__restrict__ G, double *__restrict__ mm,
                                                     unsigned *__restrict__ cnt, const unsigned *__restrict__ late,
                                                     unsigned self) {
    SML_TL_SCOPE(sml::tl::kCheckMinmax);
    __shared__ double smin[16], smax[16];
    const int v = blockIdx.x;
    const double *f = G + (size_t)v * kKX * kGF;
    double lo = f[threadIdx.x], hi = lo;
    for (int i = threadIdx.x; i < kKX * kGF; i += blockDim.x) {
        lo = nmin(lo, f[i]);
        hi = nmax(hi, f[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = nmin(lo, __shfl_xor(lo, o));
        hi = nmax(hi, __shfl_xor(hi, o));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        smin[w] = lo;
        smax[w] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 16; ++i) {
            lo = nmin(lo, smin[i]);
            hi = nmax(hi, smax[i]);
        }
        if (late && __hip_atomic_load(late, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == self)
            lo = hi = __builtin_nan("");
        if (cnt) {
            __hip_atomic_store(mm + 2 * v, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(mm + 2 * v + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            mm[2 * v] = lo;
            mm[2 * v + 1] = hi;
        }
    }
}

}  // namespace
