// sml_res_update.hpp -- the state update x <- (1 - a) x + a tanh(A x + W_in u) of every
// local region: k_res_update (a block per (region, part), any layout) and the balanced
// k_res_update_bal (a persistent grid over all the rank's rows, ELL only).
// (A timeline build, SML_TL, needs the unit's SML_TL_DEFINE ahead of this header.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sml_res_rows.hpp"
#include "sml_reservoir_layout.hpp"
#include "sml_timeline.hpp"

namespace {
using namespace sml;

// logical blocks (region, part) = nlog; with a grid smaller than nlog (the paced
// update that runs beside SPEEDY's window) each block takes logical blocks in rounds
// kMinW: waves per SIMD the registers must allow (4: one 1024-thread block per CU; 8:
// two, so one block's x staging and SpMV overlap the other's -- 64 VGPRs)
template <typename WT, bool kLds, int kMinW = 4>
__global__ __launch_bounds__(kUpdThreads, kMinW) void k_res_update(
    const RegionDev *__restrict__ R, const int32_t *__restrict__ a_rp, const uint16_t *__restrict__ a_col,
    const WT *__restrict__ a_val, const int32_t *__restrict__ w_rp, const uint16_t *__restrict__ w_col,
    const WT *__restrict__ w_val, Ell ell, const double *__restrict__ x_old, double *__restrict__ x_new,
    const double *__restrict__ feedback, double leak, int parts, int lds_x, int nlog) {
    SML_TL_SCOPE(sml::tl::kUpdate);
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int off = xcd_remap(blockIdx.x, gridDim.x);
    for (int base = 0; base < nlog; base += gridDim.x) {
        const int lb = base + off;
        if (lb < nlog)  // block-uniform
            update_block<WT, kLds>(lb, smem, R, a_rp, a_col, a_val, w_rp, w_col, w_val, ell, x_old, x_new,
                                   feedback, leak, parts, lds_x);
        if (base + (int)gridDim.x < nlog) __syncthreads();  // the block's LDS, reused next round
    }
}

// ---------------------------------------------------------------- balanced update
// k_res_update_bal: the same rows, the same arithmetic (bitwise k_res_update's ELL
// path), laid out for HBM instead of per region.  k_res_update runs a block per
// (region, part): at 1152 regions on 256 CUs (one 1024-thread block per CU: 71 VGPRs)
// that is 4.5 rounds of blocks -- the fifth a half-empty tail -- each block staging
// its region's x in LDS behind a barrier and then keeping one pass of A rows in
// flight (55 KB per CU: ~0.5 of 8 TB/s at the loaded latency).
// Here a persistent grid of one block per CU takes a contiguous, equal share of all
// the rank's rows (the regions concatenated; r0 of each block from a host table), so
// no block waits on a tail; a pass never straddles regions (a share is a run of
// segments, one per region it touches); the A / W_in rows of the next TWO passes are
// in flight while a pass computes (~110 KB per CU), whatever segment they belong to;
// and the next segment's x / feedback are loaded while the current segment's last
// pass computes and stored into the second of two LDS buffers, so a segment switch
// costs one barrier, not a memory round trip.  Needs every region in ELL form, n <=
// kStageX * 1024, ninp <= 1024 and two buffers in LDS; else k_res_update runs.
struct PassDesc {
    int r, base, end, seg;
    bool live;
};

struct StageRegs {
    double x[kStageX];
    double f;
};

template <typename WT, int NP, bool OVF, int kDepth = 2>
__global__ __launch_bounds__(kUpdThreads, 4) void k_res_update_bal(
    const RegionDev *__restrict__ R, const int32_t *__restrict__ row0, const int32_t *__restrict__ blk_r0, int nlocal,
    int64_t total, Ell ell, const double *__restrict__ x_old, double *__restrict__ x_new,
    const double *__restrict__ feedback, double leak, int lds_x, int lds_buf) {
    SML_TL_SCOPE(sml::tl::kUpdate);
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int G = gridDim.x;
    const int b = xcd_remap(blockIdx.x, G);
    const int g0 = (int)(total * b / G), g1 = (int)(total * (b + 1) / G);
    if (g0 >= g1) return;  // block-uniform
    const int tid = threadIdx.x;
    auto seg_at = [&](int r, int seg) -> PassDesc {
        const int a = row0[r], e = row0[r + 1];
        return PassDesc{r, max(g0, a) - a, min(g1, e) - a, seg, true};
    };
    auto succ = [&](const PassDesc &p) -> PassDesc {
        if (!p.live) return p;
        if (p.base + kUpdThreads < p.end) return PassDesc{p.r, p.base + kUpdThreads, p.end, p.seg, true};
        const int r = p.r + 1;
        if (r >= nlocal || row0[r] >= g1) return PassDesc{r, 0, 0, p.seg + 1, false};
        return seg_at(r, p.seg + 1);
    };
    // a lane past its segment's end loads row 0's data (in range, never used): the
    // same loads in every lane and every pass
    auto load = [&](RowRegs<WT> &q, const PassDesc &p) {
        if (!p.live) return;
        const RegionDev rg = R[p.r];
        const int i = p.base + tid;
        load_row_fixed<WT, NP, OVF>(q, rg, ell, i < p.end ? i : 0);
    };
    auto resolve = [&](RowRegs<WT> &q, const PassDesc &p) {
        q.oh = false;
        if (!OVF || !p.live) return;
        const RegionDev rg = R[p.r];
        if (!rg.a_ov) return;  // pass-uniform
        const int i = p.base + tid;
        resolve_ovf<WT, true>(q, rg, ell, i < p.end ? i : 0);
    };
    auto stage_load = [&](StageRegs &sr, int r) {
        const RegionDev rg = R[r];
        const double *xo = x_old + rg.x;
#pragma unroll
        for (int q = 0; q < kStageX; ++q) {
            const int j = tid + q * kUpdThreads;
            if (j < rg.n) sr.x[q] = xo[j];
        }
        if (tid < rg.ninp) sr.f = feedback[rg.fb + tid];
    };
    auto stage_store = [&](const StageRegs &sr, int r, double *buf) {
        const RegionDev rg = R[r];
#pragma unroll
        for (int q = 0; q < kStageX; ++q) {
            const int j = tid + q * kUpdThreads;
            if (j < rg.n) buf[j] = sr.x[q];
        }
        if (tid < rg.ninp) buf[lds_x + tid] = sr.f;
    };
    // kDepth passes in flight while one computes: L1 .. L{kDepth} (P1 .. P{kDepth})
    static_assert(kDepth == 2 || kDepth == 3, "update pipeline depth");
    PassDesc P0 = seg_at(blk_r0[b], 0);
    RowRegs<WT> L0, L1, L2, L3;
    load(L0, P0);
    resolve(L0, P0);
    PassDesc P1 = succ(P0);
    load(L1, P1);
    PassDesc P2 = succ(P1), P3 = P2;
    if constexpr (kDepth == 3) {
        load(L2, P2);
        P3 = succ(P2);
    }
    {
        StageRegs sr;
        stage_load(sr, P0.r);
        stage_store(sr, P0.r, smem);
    }
    __syncthreads();
    while (P0.live) {  // block-uniform
        // P1's overflow entries before the next pass's loads: compute(P1) then waits for
        // nothing issued after them (the in-order vmcnt), so kDepth passes stay in flight
        resolve(L1, P1);
        if constexpr (kDepth == 3)
            load(L3, P3);
        else
            load(L2, P2);
        const bool newseg = P1.live && P1.seg != P0.seg;
        StageRegs sr;
        if (newseg) stage_load(sr, P1.r);
        {  // the pass: update_block's ELL row, expression for expression
            const RegionDev rg = R[P0.r];
            const double *xs = smem + (size_t)(P0.seg & 1) * lds_buf, *fs = xs + lds_x;
            const int i = P0.base + tid;
            if (i < P0.end) x_new[rg.x + i] = ell_row_value(L0, rg, xs, fs, i, leak);
        }
        if (newseg) {  // the other buffer: its last reader (segment P0.seg - 1) finished before the last barrier
            stage_store(sr, P1.r, smem + (size_t)(P1.seg & 1) * lds_buf);
            __syncthreads();
        }
        P0 = P1;
        L0 = L1;
        P1 = P2;
        L1 = L2;
        if constexpr (kDepth == 3) {
            P2 = P3;
            L2 = L3;
            P3 = succ(P3);
        } else {
            P2 = succ(P2);
        }
    }
}

}  // namespace
