// sml_res_readout.hpp -- outvec = W_out [local_model; x~], unstandardized: the W_out
// stream (k_res_readout, rows_dot), the fused begin (k_res_begin: a region's update and
// its v_ml in one block) and the v_p finishes (k_res_finish, k_res_finish_grid).
// SML_READ_NT (default 1): W_out streamed with non-temporal loads.
// (A timeline build, SML_TL, needs the unit's SML_TL_DEFINE ahead of this header.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sml_internal.hpp"
#include "sml_res_rows.hpp"
#include "sml_res_tiling.hpp"
#include "sml_reservoir_layout.hpp"
#include "sml_timeline.hpp"

#ifndef SML_READ_NT
#define SML_READ_NT 1
#endif

namespace {
using namespace sml;

template <typename WT>
struct Vec4;
template <>
struct Vec4<float> {
    typedef float4 T;
    typedef float N __attribute__((ext_vector_type(4)));  // native vector (non-temporal loads)
};
template <>
struct Vec4<double> {
    typedef double4 T;
    typedef double N __attribute__((ext_vector_type(4)));
};

// readout: one wave per (region, 8-row group) item, 4 waves per block; blocks are
// remapped so that the items of one region stay on one XCD's L2 (x_aug reuse).
// The product W_out [local_model; x~] is split at column ncs as the reference's
// outvec_component_contribs does (v_p + v_ml, mod_reservoir.f90:1456-1459):
//   kReadML:     part = v_ml = W_out(:, ncs+1:) x~     (needs only this step's feedback)
//   kReadFinish: v = v_p + part, unstandardize (k_res_finish: one thread per output)
//   kReadFull:   v = v_p + v_ml in one pass (sml_res_step)
// v_ml is the wave's per-lane partial sums + butterfly over W_out's rows; v_p is a
// per-output sum over the ncs columns in order from the transposed block
// W_out(:, 1:ncs) = [ncs][nout_pad] (coalesced across outputs), the same code in
// both modes, so the split step and the one-pass step agree bit for bit; the split
// lets the ML part -- ~98 % of the bytes -- run before SPEEDY's local_model exists.
enum ReadMode { kReadML = 0, kReadFinish = 1, kReadFull = 2 };

// dot products of the wave's 8 W_out rows with x over columns [c0, c1) (16-B groups;
// lanes own columns c0 + 4 lane + 256 t), reduced across the wave; x values outside
// [x0, x1) are zero (fma(w, 0, s) == s), which matters only when ncs % 4 != 0
template <int R>
struct Rows {
    double v[R];
};

template <typename WT, int R, int kUnroll = 2, typename XF>
__device__ __attribute__((always_inline)) inline Rows<R> rows_dot(const WT *W, int ld, int lane, int c0, int c1,
                                                               XF xload) {
    typedef typename Vec4<WT>::N V;
    double acc[R];
#pragma unroll
    for (int q = 0; q < R; ++q) acc[q] = 0.0;
#pragma unroll kUnroll
    for (int j = c0 + lane * 4; j < c1; j += 256) {
        const double4 xv = xload(j);
        V w[R];
#pragma unroll
        for (int q = 0; q < R; ++q)  // streamed once per step: non-temporal, so W_out does not evict the
#if SML_READ_NT                          // window's data
            w[q] = __builtin_nontemporal_load(reinterpret_cast<const V *>(W + (size_t)q * ld + j));
#else
            w[q] = *reinterpret_cast<const V *>(W + (size_t)q * ld + j);
#endif
#pragma unroll
        for (int q = 0; q < R; ++q) {
            double s = acc[q];
            s = fma((double)w[q].x, xv.x, s);
            s = fma((double)w[q].y, xv.y, s);
            s = fma((double)w[q].z, xv.z, s);
            s = fma((double)w[q].w, xv.w, s);
            acc[q] = s;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int q = 0; q < R; ++q) acc[q] += __shfl_xor(acc[q], off, 64);
    Rows<R> out;
#pragma unroll
    for (int q = 0; q < R; ++q) out.v[q] = acc[q];
    return out;
}

// v_p = W_out(o, 1:ncs) local_model from the transposed block wl = [ncs][nout_pad] (a
// wave's lanes read neighbouring outputs of a column), summed in kFinGroups groups of
// consecutive columns -- each group a sequential fma chain from 0, the groups added in
// order -- so the finish can run the groups on different threads (k_res_finish_grid)
// and every other form (k_res_finish, the one-pass readout) gets the same bits
__device__ inline int fin_gsz(int ncs) { return (ncs + kFinGroups - 1) / kFinGroups; }

template <typename WT>
__device__ inline double vp_sum(const WT *__restrict__ wl, int nout_pad, const double *__restrict__ lm, int ncs,
                                int o) {
    // the kFinGroups chains advance together; each is still the sequential sum of its
    // own columns.  Every load of a round of kVpU columns per chain is issued before
    // the round's FMAs (indices past a chain's end clamped into the block, those FMAs
    // selected away): one memory round trip per round, not one per column
    constexpr int kVpU = 2;
    const int gsz = fin_gsz(ncs);
    double s[kFinGroups];
#pragma unroll
    for (int g = 0; g < kFinGroups; ++g) s[g] = 0.0;
    for (int jj0 = 0; jj0 < gsz; jj0 += kVpU) {
        double w[kVpU][kFinGroups], x[kVpU][kFinGroups];
#pragma unroll
        for (int u = 0; u < kVpU; ++u)
#pragma unroll
            for (int g = 0; g < kFinGroups; ++g) {
                const int jc = min(g * gsz + jj0 + u, ncs - 1);
                w[u][g] = (double)wl[(size_t)jc * nout_pad + o];
                x[u][g] = lm[jc];
            }
#pragma unroll
        for (int u = 0; u < kVpU; ++u)
#pragma unroll
            for (int g = 0; g < kFinGroups; ++g) {
                const int jj = jj0 + u, j = g * gsz + jj;
                const double t = fma(w[u][g], x[u][g], s[g]);
                s[g] = (jj < gsz && j < ncs) ? t : s[g];
            }
    }
    double v = s[0];
#pragma unroll
    for (int g = 1; g < kFinGroups; ++g) v = v + s[g];
    return v;
}

// unstandardize_state_vec_res: x*std + mean (two roundings) where the output has a slot
__device__ inline double unstd(double v, const double *ms, int l) {
    if (l >= 0) {
        const double t = v * ms[kMeanStd + l];
        v = t + ms[l];
    }
    return v;
}

// x~ over the columns j .. j + 3 of a region's ld-wide row (xr: the row's start; the
// state x sits from column ncs on): x_aug = [local_model; x~], x~ = x with its 1-based
// even entries squared (x_temp(2:n:2)**2, mod_reservoir.f90:1452-1455), the columns
// below ncs zero.  The squares are formed here, where x~ is consumed, instead of in a
// copy written by the update (the same multiply, so the same bits)
__device__ __attribute__((always_inline)) inline double4 rd_x(const double *xr, int j, int ncs) {
    double4 v = *reinterpret_cast<const double4 *>(xr + j);
    auto f = [&](double x, int c) {
        const int i = j + c - ncs;  // 0-based state index
        return i < 0 ? 0.0 : (i & 1) ? x * x : x;
    };
    return double4{f(v.x, 0), f(v.y, 1), f(v.z, 2), f(v.w, 3)};
}

template <typename WT, int kMode, int NR>
__global__ __launch_bounds__(512) void k_res_readout(const RegionDev *__restrict__ R, const WT *__restrict__ wout,
                                                     const WT *__restrict__ wlm,
                                                     const double *__restrict__ xst,
                                                     const double *__restrict__ local_model,
                                                     const double *__restrict__ meanstd,
                                                     const int8_t *__restrict__ outl, double *__restrict__ part,
                                                     double *__restrict__ outvec, int nout, int ov_ld, int nout_pad,
                                                     int ncs, int groups, int nitems, int ipw) {
    SML_TL_SCOPE(sml::tl::kReadout);
    // wave gw takes the items gw, gw + W, gw + 2W, .. (W waves; one item each unless
    // the launch is paced): the waves in flight together work on consecutive items.
    // NR = kRowsWide (17 rows a wave, 8 waves a region of 136 outputs): x_aug is read
    // 8 times per region instead of 17, the waves of a block together; NR = kRows:
    // 17 waves per region.  Either way a region's blocks are neighbours, kept on one
    // XCD's L2 by the remap
    const int bs = xcd_remap(blockIdx.x, gridDim.x);
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    const int gw = bs * wpb + (threadIdx.x >> 6), nw = gridDim.x * wpb;
    (void)ipw;
    for (int item = gw; item < nitems; item += nw) {
        const int r = item / groups, g = item % groups;
        const RegionDev rg = R[r];
        const int ld = rg.ld;
        const WT *W = wout + rg.wout + (size_t)(g * NR) * ld;
        Rows<NR> ml{};
        {   // v_ml: x~ from the state, columns ncs .. ld (zero below ncs from the aligned start)
            const double *xa = xst + rg.xaug;
            ml = rows_dot<WT, NR>(W, ld, lane, ncs & ~(kLdAlign - 1), ld, [=](int j) { return rd_x(xa, j, ncs); });
        }
        const int o0 = g * NR;
        if (kMode == kReadML) {  // every lane holds all 8 sums after the butterfly; lane 0 writes them
            if (lane == 0) {
    #pragma unroll
                for (int q = 0; q < NR; ++q) part[(size_t)r * nout_pad + o0 + q] = ml.v[q];
            }
        } else {  // kReadFull: lane q finishes row o0 + q with v_p (k_res_finish's sum) + v_ml
            const int o = o0 + lane;
            if (lane < NR && o < nout) {
                double vml = ml.v[0];  // static indices only: a lane-indexed pick would put the sums in scratch
    #pragma unroll
                for (int q = 1; q < NR; ++q)
                    if (lane == q) vml = ml.v[q];
                const double vp = vp_sum(wlm + rg.wlm, nout_pad, local_model + (size_t)r * ncs, ncs, o);
                outvec[(size_t)r * ov_ld + o] = unstd(vp + vml, meanstd + (size_t)r * 2 * kMeanStd, outl[o]);
            }
        }
    }
}

// sml_res_step_begin's two launches (k_res_update, then k_res_readout<kReadML>) as
// one, a block per region: the block updates its region's state (update_block, the
// same rows in the same order, kBeginThreads rows per pass) and then each of its
// waves forms one 17-row item of v_ml exactly as k_res_readout does (rows_dot: the
// same lanes, columns and butterfly), reading x~ back from x_aug, which this block
// has just written (same workgroup: visible after the barrier).  The update's
// latency-bound SpMV + tanh of one block then overlaps the W_out stream of the other
// blocks on its CU, instead of running as a grid of its own before the stream.
// Requires the wide readout (nout_pad = 17 g, g <= 8) and the LDS-staged update.
template <typename WT, int kUnroll, int kMinWaves>
__global__ __launch_bounds__(kBeginThreads, kMinWaves) void k_res_begin(
    const RegionDev *__restrict__ R, const int32_t *__restrict__ a_rp, const uint16_t *__restrict__ a_col,
    const WT *__restrict__ a_val, const int32_t *__restrict__ w_rp, const uint16_t *__restrict__ w_col,
    const WT *__restrict__ w_val, Ell ell, const double *__restrict__ x_old, double *__restrict__ x_new,
    const double *__restrict__ feedback, int ncs, double leak, int lds_x, const WT *__restrict__ wout, double *__restrict__ part, int nout_pad, int groups) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int r = blockIdx.x;
    update_block<WT, true, kBeginThreads>(r, smem, R, a_rp, a_col, a_val, w_rp, w_col, w_val, ell, x_old, x_new,
                                          feedback, leak, 1, lds_x);
    __syncthreads();  // the region's new state complete (workgroup scope)
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    if (g >= groups) return;  // wave-uniform
    const RegionDev rg = R[r];
    const int ld = rg.ld;
    const WT *W = wout + rg.wout + (size_t)(g * kRowsWide) * ld;
    const double *xa = x_new + rg.xaug;
    // k_res_readout<kReadML>'s item (r, g): the same x~ loads (zero below ncs)
    const Rows<kRowsWide> ml = rows_dot<WT, kRowsWide, kUnroll>(W, ld, lane, ncs & ~(kLdAlign - 1), ld,
                                                                [=](int j) { return rd_x(xa, j, ncs); });
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < kRowsWide; ++q) part[(size_t)r * nout_pad + g * kRowsWide + q] = ml.v[q];
    }
}

// second half of the split readout (sml_res_step_finish): one thread per (region,
// output): v = v_p + v_ml (v_ml from k_res_readout<kReadML>), unstandardized --
// the same sums, in the same order, as k_res_readout<kReadFull>
// raw (may be NULL): the outputs before unstandardize as well -- predict_slab keeps
// them as its next local model (mod_slab_ocean_reservoir.f90:1235)
template <typename WT>
__global__ __launch_bounds__(256) void k_res_finish(const RegionDev *__restrict__ R, const WT *__restrict__ wlm,
                                                    const double *__restrict__ local_model,
                                                    const double *__restrict__ meanstd,
                                                    const int8_t *__restrict__ outl, const double *__restrict__ part,
                                                    double *__restrict__ outvec, int nout, int ov_ld, int nout_pad,
                                                    int ncs, int nlocal, double *__restrict__ raw = nullptr) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = t / nout_pad, o = t % nout_pad;
    if (r >= nlocal || o >= nout) return;
    const double vp = vp_sum(wlm + R[r].wlm, nout_pad, local_model + (size_t)r * ncs, ncs, o);
    const double v = vp + part[(size_t)r * nout_pad + o];
    if (raw) raw[(size_t)r * nout + o] = v;
    outvec[(size_t)r * ov_ld + o] = unstd(v, meanstd + (size_t)r * 2 * kMeanStd, outl[o]);
}

// sml_res_step_finish_grid: k_tile_local_model + k_res_finish in one launch, one
// block per region.  The region's local-model vector is tiled and standardized
// into LDS (and to d_lm when given) exactly as k_tile_local_model does, then each
// thread finishes one output with vp_sum over the LDS copy: the same values, sums
// and order as the two-launch form, one kernel boundary fewer on the hybrid step's
// critical path
// kAsm (sml_res_step_finish_assemble, one rank holding every region in order): each
// output is also scattered into the global grids with the root's clips, exactly as
// k_assemble does from the outvec (every grid point has one writer), so the
// assembly's own launch leaves the critical path (assemble_one, sml_res_tiling.hpp)
template <typename WT>
struct Quad {
    WT v[4];
};
template <typename WT>
__device__ inline Quad<WT> load_quad(const WT *p) {
    Quad<WT> q;
    if constexpr (sizeof(WT) == 4) {
        const float4 a = *reinterpret_cast<const float4 *>(p);
        q.v[0] = a.x; q.v[1] = a.y; q.v[2] = a.z; q.v[3] = a.w;
    } else {
        const double2 a = *reinterpret_cast<const double2 *>(p), b = *reinterpret_cast<const double2 *>(p + 2);
        q.v[0] = a.x; q.v[1] = a.y; q.v[2] = b.x; q.v[3] = b.y;
    }
    return q;
}

// kGrouped (nout_pad <= 4 * 36, ncs <= kFinGroups * kFinGsz): thread t takes outputs
// 4 (t % nq) .. + 3 over column group t / nq, its W_out loads (one 16-B load per
// column) issued before the local-model gather, so they fly while the forecast is
// read; the kFinGroups partial sums meet in LDS and are added in group order
// (vp_sum's order).  Else one thread per output with vp_sum.
//
// wflag (may be null): the forecast grids come from another stream, whose one-lane
// signal kernel stores a sequence number >= wval behind SPEEDY's exit (SML_HOP_KERNEL;
// sml_hops.hpp k_hop_signal).  The kernel then goes in ahead of the forecast: its
// W_out(:, 1:ncs) block, the gather's tables and mean / std are loaded while the window
// still runs, and only the forecast values wait -- one relaxed poll by one lane,
// one agent-scope acquire by that wave, a barrier (MI355X_MICROARCH.md
// inter-workgroup visibility, the consumer form), then plain loads.  The poll gives
// up after ~4 s, marks *wlate and goes on (sml_hybrid_sync reports it).
template <typename WT, bool kAsm = false, bool kGrouped = true>
__global__ __launch_bounds__(256) void k_res_finish_grid(
    const RegionDev *__restrict__ R, const WT *__restrict__ wlm, const int32_t *__restrict__ src,
    const uint8_t *__restrict__ lidx, const double *__restrict__ fc4, const double *__restrict__ fc2,
    double *__restrict__ lm_out, const double *__restrict__ meanstd, const int8_t *__restrict__ outl,
    const double *__restrict__ part, double *__restrict__ outvec, int nout, int ov_ld, int nout_pad, int ncs,
    const int32_t *__restrict__ asm_dst = nullptr, double *__restrict__ g4 = nullptr, double *__restrict__ g2 = nullptr,
    double *__restrict__ pr = nullptr, const uint64_t *__restrict__ wflag = nullptr, uint64_t wval = 0,
    unsigned *__restrict__ wlate = nullptr, long long wtimeout = 400000000ll) {
    __shared__ double slm[kMaxNcs];
    __shared__ int gave_up;
    __shared__ double red[kGrouped ? kFinGroups * 144 : 1];
    const int r = blockIdx.x, t = threadIdx.x;
    const double *ms = meanstd + (size_t)r * 2 * kMeanStd;
    const WT *wl = wlm + R[r].wlm;
    const int nq = nout_pad / 4, gsz = fin_gsz(ncs);
    const int q = t % nq, g = t / nq;
    const int j0 = g * gsz, j1 = min(ncs, j0 + gsz);
    Quad<WT> w[kFinGsz];
    if constexpr (kGrouped) {
        // every load issued, unpredicated (columns past the group's end clamped into the
        // block and not summed): one memory round trip for all of them
        const int gq = g < kFinGroups ? g : 0;
        const int jlast = max(ncs - 1, 0);
#pragma unroll
        for (int jj = 0; jj < kFinGsz; ++jj)
            w[jj] = load_quad(wl + (size_t)min(gq * gsz + jj, jlast) * nout_pad + 4 * q);
    }
    // the gather's tables and standardization (ncs <= kMaxNcs = blockDim: one entry per thread)
    const bool gj = t < ncs;
    int gs = 0;
    double gmean = 0.0, gstd = 1.0;
    if (gj) {
        const int e = r * ncs + t;
        gs = src[e];
        const int l = lidx[e];
        gmean = ms[l];
        gstd = ms[kMeanStd + l];
    }
    if (wflag) {
        if (t == 0) {
            gave_up = 0;
            const long long c0 = wall_clock64();
            while (__hip_atomic_load(wflag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < wval) {
                __builtin_amdgcn_s_sleep(1);
                if (wall_clock64() - c0 > wtimeout) {  // default ~4 s at wall_clock64's 100 MHz
                    __hip_atomic_store(wlate, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    gave_up = 1;
                    break;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
    }
    SML_TL_SCOPE(sml::tl::kFinish);  // (after the wait: when the forecast arrived)
    if (gj) {
        // a forecast that never arrived reads as NaN: the outvecs, grids and the next
        // window's safety check then refuse it instead of predicting from stale values
        const double v = (wflag && gave_up) ? __builtin_nan("") : (gs < kGrid4d ? fc4[gs] : fc2[gs - kGrid4d]);
        const double d = v - gmean;
        const double x = d / gstd;
        slm[t] = x;
        if (lm_out) lm_out[r * ncs + t] = x;
    }
    __syncthreads();
    if constexpr (kGrouped) {
        // (keep the W_out quads in their storage precision until here: converted early
        // they would hold twice the registers across the gather)
        __builtin_amdgcn_sched_barrier(0);
        if (g < kFinGroups) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int jj = 0; jj < kFinGsz; ++jj)
                if (j0 + jj < j1) {
                    const double x = slm[j0 + jj];
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] = fma((double)w[jj].v[k], x, acc[k]);
                }
#pragma unroll
            for (int k = 0; k < 4; ++k) red[g * nout_pad + 4 * q + k] = acc[k];
        }
        __syncthreads();
    }
    for (int o = t; o < nout; o += blockDim.x) {
        double vp;
        if constexpr (kGrouped) {
            vp = red[o];
#pragma unroll
            for (int gg = 1; gg < kFinGroups; ++gg) vp = vp + red[gg * nout_pad + o];
        } else {
            vp = vp_sum(wl, nout_pad, slm, ncs, o);
        }
        const double v = unstd(vp + part[(size_t)r * nout_pad + o], ms, outl[o]);
        outvec[(size_t)r * ov_ld + o] = v;
        if constexpr (kAsm) assemble_one(asm_dst[(size_t)r * nout + o], v, g4, g2, pr);
    }
}

}  // namespace
