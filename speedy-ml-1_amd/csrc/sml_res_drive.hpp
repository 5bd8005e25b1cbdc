// sml_res_drive.hpp -- the training drive: every local region driven by a batch of
// inputs, each state kept as a column of the W_out fit (k_res_drive, one launch per
// batch; k_drive_record, the column writer of the stepwise form).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sml_res_rows.hpp"
#include "sml_reservoir_layout.hpp"

namespace {
using namespace sml;

// ------------------------------------------------------------------ training drive
// reservoir_layer_chunking_hybrid (src/mod_reservoir.f90:1065-1173) with the first lines
// of chunking_matmul (:1662-1675): the reservoirs driven by a batch of m inputs, every
// state kept as one column of the W_out fit's augmented_states.  Column c of a region
// is [model block c (ncs rows); x~ (n rows)] -- x~ the state BEFORE input c with its
// 0-based odd nodes squared (states(2:n:2,:)**2, :1133) -- and column c of its targets
// is the region's own points of input c (tile_full_input_to_target_data2d); then
// x <- (1 - leak) x + leak tanh(A x + W_in u_c).  Region r's block starts at
// m (row0[r] + r ncs) doubles: the layout sml_train_accumulate reads.
//
// Training is teacher-forced -- no exchange, no readout between steps -- so a region's
// whole batch runs in one workgroup: k_res_drive, a block per region, keeps x and u in
// LDS (two copies of each: the SpMV gathers random columns of the old state while the
// new one is written, and input c + 1 lands while input c is read), one barrier per
// column, one launch per batch.  The row is row_value, so the state is bitwise the one
// sml_res_synchronize produces.  The first pass's A / W_in rows of the next column are
// loaded before the barrier that ends the current one.  A block re-reads its region's
// A and W_in every column, so it loads them cached (not the update's streaming loads)
// and streams its columns out instead: 144 full-size regions, 1024 columns 12.8 ms,
// against 17.3 with the update's hints on the same box (profiles/train_drive.md).
//
// The targets of column c are the region's own points of input c: of the driving input
// (TGT_GLOBAL false: read from its LDS copy), or of a second series tinputs, block c at
// tinputs + c * tstride (TGT_GLOBAL true, sml_res_train_drive_from: read from global
// memory) -- the clean series beside a noised driving one (sml_res_input_noise).

// a column is written once and read later by the Gram kernel: streamed past the L2,
// which the region's A rows are to stay in
__device__ inline void drive_store(double *p, double v) { __builtin_nontemporal_store(v, p); }

template <typename WT, bool TGT_GLOBAL>
__global__ __launch_bounds__(kUpdThreads, 4) void k_res_drive(
    const RegionDev *__restrict__ R, const int32_t *__restrict__ row0, const int32_t *__restrict__ a_rp,
    const uint16_t *__restrict__ a_col, const WT *__restrict__ a_val, const int32_t *__restrict__ w_rp,
    const uint16_t *__restrict__ w_col, const WT *__restrict__ w_val, Ell ell, const double *__restrict__ x_old,
    double *__restrict__ x_new, const double *__restrict__ inputs, int64_t stride,
    const double *__restrict__ tinputs, int64_t tstride, const double *__restrict__ model, int64_t model_stride, const int32_t *__restrict__ tgt_idx, double *__restrict__ states,
    double *__restrict__ targets, int m, int ncs, int nout, double leak, int lds_x, int lds_u) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int r = blockIdx.x, tid = threadIdx.x;
    const RegionDev rg = R[r];
    const int n = rg.n, ninp = rg.ninp;
    const CsrRows<WT> csr{a_rp + rg.a_rp, a_col + rg.a_nz, a_val + rg.a_nz, w_rp + rg.w_rp, w_col + rg.w_nz,
                          w_val + rg.w_nz};
    double *sx = smem, *su = smem + 2 * (size_t)lds_x;  // [2][lds_x] states, [2][lds_u] inputs
    const double *u = inputs + rg.fb;
    const double *tu = TGT_GLOBAL ? tinputs + rg.fb : nullptr;
    RowRegs<WT> cur, nxt;
    load_row<WT, false>(cur, rg, ell, tid, tid < n);
    for (int j = tid; j < n; j += kUpdThreads) sx[j] = x_old[rg.x + j];
    for (int j = tid; j < ninp; j += kUpdThreads) su[j] = u[j];
    __syncthreads();
    double *scol = states + (int64_t)m * (row0[r] + (int64_t)r * ncs);
    double *tcol = targets ? targets + (int64_t)m * r * nout : nullptr;
    const int32_t *ti = tgt_idx + (size_t)r * nout;
    const double *lm = model + (size_t)r * ncs;
    const bool ureg = ninp <= kUpdThreads;  // the next input through one register per thread
    int b = 0;
    for (int c = 0; c < m; ++c) {  // (every bound below is block-uniform)
        const double *xs = sx + (size_t)b * lds_x, *fs = su + (size_t)b * lds_u;
        double *xn = sx + (size_t)(1 - b) * lds_x, *un = su + (size_t)(1 - b) * lds_u;
        const bool more = c + 1 < m;
        const double *unext = u + (size_t)(c + 1) * stride;
        double uv = 0.0;
        if (more && ureg && tid < ninp) uv = unext[tid];
        for (int j = tid; j < ncs; j += kUpdThreads) drive_store(scol + j, lm[j]);
        if (tcol) {
            if constexpr (TGT_GLOBAL) {
                const double *tc = tu + (size_t)c * tstride;
                for (int j = tid; j < nout; j += kUpdThreads) drive_store(tcol + j, tc[ti[j]]);
            } else {
                for (int j = tid; j < nout; j += kUpdThreads) drive_store(tcol + j, fs[ti[j]]);
            }
        }
        for (int base = 0; base < n; base += kUpdThreads) {
            const int i = base + tid, inext = i + kUpdThreads;
            if (base + kUpdThreads < n)
                load_row<WT, false>(nxt, rg, ell, inext, inext < n);
            else if (more)
                load_row<WT, false>(nxt, rg, ell, tid, tid < n);  // the next column's first pass
            if (i < n) {
                const double xv = xs[i];
                drive_store(scol + ncs + i, (i & 1) ? xv * xv : xv);
                xn[i] = row_value(cur, rg, ell, csr, xs, fs, i, leak);
            }
            cur = nxt;
        }
        if (more) {
            if (ureg) {
                if (tid < ninp) un[tid] = uv;
            } else {
                for (int j = tid; j < ninp; j += kUpdThreads) un[j] = unext[j];
            }
        }
        __syncthreads();  // x_new and u_{c+1} complete; every read of x and u_c done
        b = 1 - b;
        scol += ncs + n;
        if (tcol) tcol += nout;
        lm += model_stride;
    }
    const double *xs = sx + (size_t)b * lds_x;
    for (int j = tid; j < n; j += kUpdThreads) x_new[rg.x + j] = xs[j];
}

// column c of every region from the state in global memory: the stepwise form of the
// drive (SML_RES_PATH_STEPWISE_DRIVE, or a region past k_res_drive's LDS), followed by
// the update's own launch.  tu: the block the targets are read from (the driving block u,
// or sml_res_train_drive_from's).  grid (nlocal, row chunks of 256)
__global__ __launch_bounds__(256) void k_drive_record(const RegionDev *__restrict__ R,
                                                      const int32_t *__restrict__ row0,
                                                      const double *__restrict__ x, const double *__restrict__ tu,
                                                      const double *__restrict__ lm,
                                                      const int32_t *__restrict__ tgt_idx,
                                                      double *__restrict__ states, double *__restrict__ targets,
                                                      int c, int m, int ncs, int nout) {
    const int r = blockIdx.x, j = blockIdx.y * blockDim.x + threadIdx.x;
    const RegionDev rg = R[r];
    const int naug = ncs + rg.n;
    double *scol = states + (int64_t)m * (row0[r] + (int64_t)r * ncs) + (int64_t)c * naug;
    if (j < ncs) {
        scol[j] = lm[(size_t)r * ncs + j];
    } else if (j < naug) {
        const int i = j - ncs;
        const double xv = x[rg.x + i];
        scol[j] = (i & 1) ? xv * xv : xv;
    }
    if (targets && blockIdx.y == 0) {
        double *tcol = targets + ((int64_t)m * r + c) * nout;
        for (int t = threadIdx.x; t < nout; t += blockDim.x) tcol[t] = tu[rg.fb + tgt_idx[(size_t)r * nout + t]];
    }
}

}  // namespace
