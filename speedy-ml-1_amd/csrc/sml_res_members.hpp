// sml_res_members.hpp -- ensemble members (sml_res_set_members): E states of every
// region advance through one stream of the weights.  k_res_update_mem is the per-region
// update (update_block's structure) with each row's A / W_in loads used for a tile of
// members; k_res_readout_mem is k_res_readout's one-pass form with every 16-byte W_out
// load, and its widening, used for a tile of members.  Member e's state lives at
// e * xstride doubles in both state buffers (xstride = the pool's size, a multiple of
// kLdAlign), so member 0 is where a single-member context keeps its state.
// Per member the arithmetic is the single-member kernels' own -- row_value for a row of
// the update; for the readout the same lanes, columns, per-lane fma order and butterfly
// as rows_dot, then vp_sum and unstd -- so every member's bits are those of sml_res_step
// on a context of its own.
// The split step: k_res_readout_mem's kReadML form leaves every member's v_ml in the
// context's partial sums (sml_res_step_begin_members); k_res_finish_mem and
// k_res_finish_grid_mem are k_res_finish and k_res_finish_grid with a member dimension, the
// latter a block per (region, tile of members) whose gathers fly together.
// (A timeline build, SML_TL, needs the unit's SML_TL_DEFINE ahead of this header.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sml_res_readout.hpp"
#include "sml_res_rows.hpp"
#include "sml_reservoir_layout.hpp"
#include "sml_timeline.hpp"

namespace {
using namespace sml;

// what locates the members of a launch: E members, `tile` of them per block / wave,
// member e's state at e * xs, feedback at e * fbs, local model at e * lms, outvecs at
// e * ovs, the v_ml partial sums of a begun step at e * ps (doubles)
struct MemberArgs {
    int members, tile;
    int64_t xs, fbs, lms, ovs, ps;
};

// logical block = (region, part, tile of members): the tiles of one (region, part) are
// neighbours, so the A / W_in rows a later tile reads again come from the L2.  TM: the
// compile-time bound of the tile (mem.tile <= TM); the members past the tile's count
// are skipped, block-uniformly.  With kLds member m's x and u are staged at
// smem + m * lds_buf (x from 0, u from lds_x, as update_block lays one member out).
template <typename WT, bool kLds, int TM>
__global__ __launch_bounds__(kUpdThreads, 4) void k_res_update_mem(
    const RegionDev *__restrict__ R, const int32_t *__restrict__ a_rp, const uint16_t *__restrict__ a_col,
    const WT *__restrict__ a_val, const int32_t *__restrict__ w_rp, const uint16_t *__restrict__ w_col,
    const WT *__restrict__ w_val, Ell ell, const double *__restrict__ x_old, double *__restrict__ x_new,
    const double *__restrict__ feedback, double leak, int parts, int lds_x, int lds_buf, int ntiles,
    MemberArgs mem) {
    SML_TL_SCOPE(sml::tl::kUpdate);
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int lb = b / ntiles, e0 = (b % ntiles) * mem.tile;
    const int tm = min(mem.tile, mem.members - e0);  // >= 1: ntiles = ceil(members / tile)
    const int r = lb / parts, part = lb % parts;
    const RegionDev rg = R[r];
    const int n = rg.n, tid = threadIdx.x;
    const int per = (n + parts - 1) / parts;
    const int beg = part * per, end = min(n, beg + per);
    if (beg >= end) return;  // block-uniform
    RowRegs<WT> cur, nxt;
    load_row(cur, rg, ell, beg + tid, beg + tid < end);  // once for the tile's members
    const double *xs[TM], *fs[TM];
#pragma unroll
    for (int m = 0; m < TM; ++m) {
        const int e = e0 + min(m, tm - 1);  // (past the tile: a member in range, never used)
        xs[m] = x_old + (size_t)e * mem.xs + rg.x;
        fs[m] = feedback + (size_t)e * mem.fbs + rg.fb;
    }
    if (kLds) {
#pragma unroll
        for (int m = 0; m < TM; ++m) {
            if (m < tm) {
                double *sx = smem + (size_t)m * lds_buf, *sf = sx + lds_x;
                for (int j = tid; j < n; j += kUpdThreads) sx[j] = xs[m][j];
                for (int j = tid; j < rg.ninp; j += kUpdThreads) sf[j] = fs[m][j];
                xs[m] = sx;
                fs[m] = sf;
            }
        }
        __syncthreads();
    }
    const CsrRows<WT> csr{a_rp + rg.a_rp, a_col + rg.a_nz, a_val + rg.a_nz, w_rp + rg.w_rp, w_col + rg.w_nz,
                          w_val + rg.w_nz};
    for (int base = beg; base < end; base += kUpdThreads) {
        const int i = base + tid;
        const bool live = i < end;
        const int inext = i + kUpdThreads;
        if (base + kUpdThreads < end) load_row(nxt, rg, ell, inext, inext < end);
        if (live) {
            // the row's value per member: update_block's expression on that member's x and u
            // (TM independent chains from one row's loads)
            double v[TM];
#pragma unroll
            for (int m = 0; m < TM; ++m)
                if (m < tm) v[m] = row_value(cur, rg, ell, csr, xs[m], fs[m], i, leak);
#pragma unroll
            for (int m = 0; m < TM; ++m)
                if (m < tm) x_new[(size_t)(e0 + m) * mem.xs + rg.x + i] = v[m];
        }
        cur = nxt;
    }
}

// rows_dot for T x-vectors: the wave's R W_out rows over columns [c0, c1), each 16-byte
// load and its widening used T times.  acc[m][q] is rows_dot's acc[q] on member m's x:
// the lane's columns in the same order through one fma chain, the same butterfly.
template <int R, int T>
struct RowsMem {
    double v[T][R];
};

template <typename WT, int R, int T, typename XF>
__device__ __attribute__((always_inline)) inline RowsMem<R, T> rows_dot_mem(const WT *W, int ld, int lane, int c0,
                                                                           int c1, XF xload) {
    typedef typename Vec4<WT>::N V;
    RowsMem<R, T> acc;
#pragma unroll
    for (int m = 0; m < T; ++m)
#pragma unroll
        for (int q = 0; q < R; ++q) acc.v[m][q] = 0.0;
    for (int j = c0 + lane * 4; j < c1; j += 256) {
        double4 xv[T];
#pragma unroll
        for (int m = 0; m < T; ++m) xv[m] = xload(m, j);
        V w[R];
#pragma unroll
        for (int q = 0; q < R; ++q)  // streamed once per tile of members: non-temporal (rows_dot)
#if SML_READ_NT
            w[q] = __builtin_nontemporal_load(reinterpret_cast<const V *>(W + (size_t)q * ld + j));
#else
            w[q] = *reinterpret_cast<const V *>(W + (size_t)q * ld + j);
#endif
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const double wx = (double)w[q].x, wy = (double)w[q].y, wz = (double)w[q].z, ww = (double)w[q].w;
#pragma unroll
            for (int m = 0; m < T; ++m) {
                double s = acc.v[m][q];
                s = fma(wx, xv[m].x, s);
                s = fma(wy, xv[m].y, s);
                s = fma(wz, xv[m].z, s);
                s = fma(ww, xv[m].w, s);
                acc.v[m][q] = s;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int m = 0; m < T; ++m)
#pragma unroll
            for (int q = 0; q < R; ++q) acc.v[m][q] += __shfl_xor(acc.v[m][q], off, 64);
    return acc;
}

// k_res_readout<kReadFull>'s item and wave mapping with a tile of T members per item:
// item = (region, group, stream s), the streams of one (region, group) neighbours (the
// W_out rows a later stream reads again are the ones its neighbour wave is reading).
// T: the compile-time bound of the tile (mem.tile <= T).  The slots of a tile past its
// members read member E - 1's x and write nothing.
// kReadML (sml_res_step_begin_members): v_ml alone, as k_res_readout<kReadML> leaves it --
// lane 0 writes the tile's T x NR sums into their members' partial-sum rows ([nlocal][nout_pad]
// at e * mem.ps); no v_p, no outvec.  Without the epilogue's registers the compiler takes
// the 17-row form to 162 VGPRs for three waves per SIMD and keeps one pass of loads in
// flight; held to two waves per SIMD, as the one-pass form runs, it uses 210 / 248 (fp32 /
// fp64 storage) and the begin is a quarter faster (profiles/members.md).  The other forms
// keep the compiler's default range (1 .. 8).
template <typename WT, int kMode, int NR, int T>
__global__ __launch_bounds__(512)
__attribute__((amdgpu_waves_per_eu(kMode == kReadML && NR == kRowsWide ? 2 : 1,
                                   kMode == kReadML && NR == kRowsWide ? 2 : 8))) void k_res_readout_mem(const RegionDev *__restrict__ R, const WT *__restrict__ wout,
                                                         const WT *__restrict__ wlm, const double *__restrict__ xst,
                                                         const double *__restrict__ local_model,
                                                         const double *__restrict__ meanstd,
                                                         const int8_t *__restrict__ outl, double *__restrict__ part,
                                                         double *__restrict__ outvec, int nout, int ov_ld, int nout_pad, int ncs, int groups,
                                                         int nitems, int nstreams, MemberArgs mem) {
    static_assert(kMode == kReadFull || kMode == kReadML, "the members readout is the one pass or the v_ml half");
    SML_TL_SCOPE(sml::tl::kReadout);
    const int bs = xcd_remap(blockIdx.x, gridDim.x);
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    const int gw = bs * wpb + (threadIdx.x >> 6), nw = gridDim.x * wpb;
    for (int it = gw; it < nitems * nstreams; it += nw) {
        const int item = it / nstreams, e0 = (it % nstreams) * mem.tile;
        const int r = item / groups, g = item % groups;
        const int tm = min(mem.tile, mem.members - e0);  // mem.tile <= T
        const RegionDev rg = R[r];
        const int ld = rg.ld;
        const WT *W = wout + rg.wout + (size_t)(g * NR) * ld;
        const double *xa = xst + rg.xaug;
        const int64_t xs = mem.xs;
        const int elast = mem.members - 1;
        // v_ml of every member of the tile: x~ from that member's state (rd_x)
        const RowsMem<NR, T> ml = rows_dot_mem<WT, NR, T>(W, ld, lane, ncs & ~(kLdAlign - 1), ld, [=](int m, int j) {
            return rd_x(xa + (size_t)min(e0 + m, elast) * xs, j, ncs);
        });
        const int o0 = g * NR, o = o0 + lane;
        if constexpr (kMode == kReadML) {  // every lane holds all the sums after the butterfly; lane 0 writes them
            if (lane == 0) {
#pragma unroll
                for (int m = 0; m < T; ++m) {
                    if (m < tm) {
                        double *p = part + (size_t)(e0 + m) * mem.ps + (size_t)r * nout_pad + o0;
#pragma unroll
                        for (int q = 0; q < NR; ++q) p[q] = ml.v[m][q];
                    }
                }
            }
            continue;
        }
        // lane q finishes row o0 + q of each member with v_p (vp_sum) + v_ml, as k_res_readout does
        // (each member's sum picked before the first v_p, so the T * NR sums are dead by then)
        double vmls[T];
#pragma unroll
        for (int m = 0; m < T; ++m) {
            vmls[m] = ml.v[m][0];  // static indices only (k_res_readout)
#pragma unroll
            for (int q = 1; q < NR; ++q)
                if (lane == q) vmls[m] = ml.v[m][q];
        }
        if (lane < NR && o < nout) {
#pragma unroll
            for (int m = 0; m < T; ++m) {
                if (m < tm) {
                    const double vml = vmls[m];
                    const size_t e = (size_t)(e0 + m);
                    const double vp =
                        vp_sum(wlm + rg.wlm, nout_pad, local_model + e * mem.lms + (size_t)r * ncs, ncs, o);
                    outvec[e * mem.ovs + (size_t)r * ov_ld + o] =
                        unstd(vp + vml, meanstd + (size_t)r * 2 * kMeanStd, outl[o]);
                }
            }
        }
    }
}

// k_res_finish with a member dimension (sml_res_step_finish_members): one thread per
// (member, region, output): vp_sum on member e's local model, plus member e's partial sum,
// then unstd -- k_res_finish's expression on one member's data
template <typename WT>
__global__ __launch_bounds__(256) void k_res_finish_mem(const RegionDev *__restrict__ R, const WT *__restrict__ wlm,
                                                        const double *__restrict__ local_model,
                                                        const double *__restrict__ meanstd,
                                                        const int8_t *__restrict__ outl,
                                                        const double *__restrict__ part, double *__restrict__ outvec,
                                                        int nout, int ov_ld, int nout_pad, int ncs, int nlocal,
                                                        MemberArgs mem) {
    const int per = nlocal * nout_pad;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)per * mem.members) return;
    const int e = (int)(t / per), tr = (int)(t % per);
    const int r = tr / nout_pad, o = tr % nout_pad;
    if (o >= nout) return;
    const double vp = vp_sum(wlm + R[r].wlm, nout_pad, local_model + (size_t)e * mem.lms + (size_t)r * ncs, ncs, o);
    const double v = vp + part[(size_t)e * mem.ps + (size_t)r * nout_pad + o];
    outvec[(size_t)e * mem.ovs + (size_t)r * ov_ld + o] = unstd(v, meanstd + (size_t)r * 2 * kMeanStd, outl[o]);
}

// where the members' forecast grids, local models, outvecs, partial sums and assembled
// grids are: member e at e * stride doubles of each
struct FinMemArgs {
    int members, tile, tiles;
    int64_t fc4s, fc2s, lms, ovs, ps, g4s, g2s;
};

// k_res_finish_grid for a tile of members (sml_res_step_finish_grid_members /
// _assemble_members): one block per (region, tile of TF members at most).  The block loads
// its W_out(:, 1:ncs) quads and the gather's tables, mean and std once, issues the gathers of
// all the tile's members together into slm[m] (their round trips overlap), and after one
// barrier forms each member's grouped sums in red[m] from the same quads -- per member the
// chain k_res_finish_grid runs over the same columns, the groups added in group order --
// then, after a second barrier, each member's outputs: unstd(vp + part) into that member's
// outvec and, with kAsm, assemble_one into that member's grids.  Ungrouped: vp_sum over
// slm[m].  Nothing is summed across members.  No in-kernel forecast wait: that is the
// hybrid loop's.
template <typename WT, bool kAsm, bool kGrouped, int TF>
__global__ __launch_bounds__(256) void k_res_finish_grid_mem(
    const RegionDev *__restrict__ R, const WT *__restrict__ wlm, const int32_t *__restrict__ src,
    const uint8_t *__restrict__ lidx, const double *__restrict__ fc4, const double *__restrict__ fc2,
    double *__restrict__ lm_out, const double *__restrict__ meanstd, const int8_t *__restrict__ outl,
    const double *__restrict__ part, double *__restrict__ outvec, int nout, int ov_ld, int nout_pad, int ncs,
    const int32_t *__restrict__ asm_dst, double *__restrict__ g4, double *__restrict__ g2, double *__restrict__ pr,
    FinMemArgs mem) {
    static_assert(TF >= 1 && TF <= kFinTileMax, "the tile's bound");
    __shared__ double slm[TF][kMaxNcs];
    __shared__ double red[kGrouped ? TF * kFinGroups * kFinOutMax : 1];
    const int r = blockIdx.x / mem.tiles, e0 = (blockIdx.x % mem.tiles) * mem.tile;
    const int tm = min(min(mem.tile, TF), mem.members - e0);  // >= 1: tiles = ceil(members / tile)
    const int t = threadIdx.x;
    const double *ms = meanstd + (size_t)r * 2 * kMeanStd;
    const WT *wl = wlm + R[r].wlm;
    const int nq = nout_pad / 4, gsz = fin_gsz(ncs);
    const int q = t % nq, g = t / nq;
    const int j0 = g * gsz, j1 = min(ncs, j0 + gsz);
    Quad<WT> w[kFinGsz];
    if constexpr (kGrouped) {  // (k_res_finish_grid's loads: every one issued, unpredicated)
        const int gq = g < kFinGroups ? g : 0;
        const int jlast = max(ncs - 1, 0);
#pragma unroll
        for (int jj = 0; jj < kFinGsz; ++jj)
            w[jj] = load_quad(wl + (size_t)min(gq * gsz + jj, jlast) * nout_pad + 4 * q);
    }
    const bool gj = t < ncs;  // ncs <= kMaxNcs = blockDim: one entry per thread
    SML_TL_SCOPE(sml::tl::kFinish);
    if (gj) {
        const int en = r * ncs + t;
        const int gs = src[en];
        const int l = lidx[en];
        const double gmean = ms[l], gstd = ms[kMeanStd + l];
        double v[TF];
#pragma unroll
        for (int m = 0; m < TF; ++m) {  // the tile's gathers, all in flight
            const size_t e = (size_t)(e0 + min(m, tm - 1));
            v[m] = gs < kGrid4d ? fc4[e * mem.fc4s + gs] : fc2[e * mem.fc2s + (gs - kGrid4d)];
        }
#pragma unroll
        for (int m = 0; m < TF; ++m) {
            if (m < tm) {
                const double d = v[m] - gmean;
                const double x = d / gstd;
                slm[m][t] = x;
                if (lm_out) lm_out[(size_t)(e0 + m) * mem.lms + (size_t)r * ncs + t] = x;
            }
        }
    }
    __syncthreads();
    if constexpr (kGrouped) {
        __builtin_amdgcn_sched_barrier(0);  // (the quads stay in their storage precision until here)
        if (g < kFinGroups) {
#pragma unroll 1
            for (int m = 0; m < tm; ++m) {
                double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int jj = 0; jj < kFinGsz; ++jj)
                    if (j0 + jj < j1) {
                        const double x = slm[m][j0 + jj];
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc[k] = fma((double)w[jj].v[k], x, acc[k]);
                    }
                double *rm = red + (size_t)m * kFinGroups * kFinOutMax;
#pragma unroll
                for (int k = 0; k < 4; ++k) rm[g * nout_pad + 4 * q + k] = acc[k];
            }
        }
        __syncthreads();
    }
    for (int o = t; o < nout; o += blockDim.x) {
        const int l = outl[o];
        const int d = kAsm ? asm_dst[(size_t)r * nout + o] : -1;
        for (int m = 0; m < tm; ++m) {
            const size_t e = (size_t)(e0 + m);
            double vp;
            if constexpr (kGrouped) {
                const double *rm = red + (size_t)m * kFinGroups * kFinOutMax;
                vp = rm[o];
#pragma unroll
                for (int gg = 1; gg < kFinGroups; ++gg) vp = vp + rm[gg * nout_pad + o];
            } else {
                vp = vp_sum(wl, nout_pad, slm[m], ncs, o);
            }
            const double v = unstd(vp + part[e * mem.ps + (size_t)r * nout_pad + o], ms, l);
            outvec[e * mem.ovs + (size_t)r * ov_ld + o] = v;
            if constexpr (kAsm) assemble_one(d, v, g4 + e * mem.g4s, g2 + e * mem.g2s, pr + e * mem.g2s);
        }
    }
}

}  // namespace
