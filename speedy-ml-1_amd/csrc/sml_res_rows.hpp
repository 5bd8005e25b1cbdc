// sml_res_rows.hpp -- what every reservoir kernel that touches A and W_in shares: the
// XCD remap, the ELL pools' pointers (Ell), one row's loads (RowRegs and its loaders),
// the activation, the row's value in each layout (ell_row_value, row_value) and the
// per-region update body (update_block: k_res_update, k_res_begin).
// SML_UPD_NT (default 1): A and W_in streamed with non-temporal loads.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sml_reservoir_layout.hpp"

#ifndef SML_UPD_NT
#define SML_UPD_NT 1
#endif

namespace {
using namespace sml;

// ------------------------------------------------------------------ kernels
// XCD-contiguous remap of a 1-D grid: consecutive hardware blocks are dealt
// round-robin to the 8 XCDs (MI355X_MICROARCH.md, workgroup dispatch); this
// bijection gives each XCD one contiguous range of logical blocks, so all blocks
// of a region share one L2 (speed only, never correctness).
__device__ inline int xcd_remap(int b, int nb) {
    const int q8 = nb / 8, rem = nb % 8, xcd = b % 8, idx = b / 8;
    return xcd * q8 + min(xcd, rem) + idx;
}

struct Ell {
    const uint16_t *a_col;
    const void *a_val;
    const uint16_t *w_col;
    const void *w_val;
    const uint64_t *a_om;  // A's overflow bits / counts / entries (RegionDev::a_ov)
    const uint32_t *a_ob;
    const uint16_t *a_oc;
    const void *a_ov;
    const void *zero;  // 256 zero bytes
};

// Row loads of one pass, issued ahead of their use (software pipelining): A's main
// slots as up to 4 (col, col) / (val, val) pairs, W_in's entry, and -- for a region
// with an overflow list -- the row's overflow word and count, then (resolve_ovf, one
// stage later) its overflow entry.
template <typename WT>
struct RowRegs {
    uint32_t c[kEllA / 2];
    WT v[kEllA];
    uint32_t wc;
    WT wv;
    uint64_t om;
    uint32_t ob;
    uint32_t oc;
    WT ov;
    bool oh;
};

// A and W_in are streamed once per step: non-temporal loads (SML_UPD_NT), like the
// readout's W_out, so they do not evict the data of the SPEEDY window running beside
template <typename T>
__device__ inline T stream_load(const T *p) {
#if SML_UPD_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

template <typename WT>
struct Pair;
template <>
struct Pair<float> {
    typedef float N __attribute__((ext_vector_type(2)));
};
template <>
struct Pair<double> {
    typedef double N __attribute__((ext_vector_type(2)));
};

// pair p of row i (slots 2p, 2p + 1) from the pair-major ELL copy
// kNT = false: plain (cached) loads, for a reader that comes back to the same rows
// (the training drive re-reads its region's A every column)
template <bool kNT, typename T>
__device__ inline T row_load(const T *p) {
    if constexpr (kNT)
        return stream_load(p);
    else
        return *p;
}

template <typename WT, bool kNT = true>
__device__ inline void load_pair(RowRegs<WT> &q, int p, const uint32_t *cp, const WT *vp) {
    typedef typename Pair<WT>::N V2;
    q.c[p] = row_load<kNT>(cp);
    const V2 v = row_load<kNT>(reinterpret_cast<const V2 *>(vp));
    q.v[2 * p] = v.x;
    q.v[2 * p + 1] = v.y;
}

__device__ inline uint32_t win_col_implicit(const RegionDev &rg, int i) {
    return __umulhi((uint32_t)i, rg.w_magic);  // = i / w_q for every i < n (checked at load)
}

// every load of row i, branching on the region's widths (k_res_update, k_res_begin)
template <typename WT, bool kNT = true>
__device__ inline void load_row(RowRegs<WT> &q, const RegionDev &rg, const Ell &ell, int i, bool live) {
    if (live && rg.a_w > 0) {
        const uint32_t *cb = reinterpret_cast<const uint32_t *>(ell.a_col + rg.a_ell);
        const WT *vb = (const WT *)ell.a_val + rg.a_ell;
        const int np = (rg.a_w + 1) >> 1, n = rg.n;
#pragma unroll
        for (int p = 0; p < kEllA / 2; ++p)
            if (p < np) load_pair<WT, kNT>(q, p, cb + (size_t)p * n + i, vb + 2 * ((size_t)p * n + i));
        if (rg.a_ov) {
            q.om = row_load<kNT>(ell.a_om + rg.a_om + (i >> 6));
            q.ob = row_load<kNT>(ell.a_ob + rg.a_om + (i >> 6));
        }
    }
    if (live && rg.w_w > 0) {
        q.wc = rg.w_q > 0 ? win_col_implicit(rg, i) : (uint32_t)row_load<kNT>(ell.w_col + rg.w_ell + i);
        q.wv = row_load<kNT>((const WT *)ell.w_val + rg.w_ell + i);
    }
}

// the same loads for the balanced update: NP pairs from every region (pairs past a
// narrower region's own load the zero bytes, so the pair loads carry no branch); the
// overflow word / count and the stored W_in column only where the region has them --
// a branch uniform across the pass (a pass never straddles regions)
template <typename WT, int NP, bool OVF>
__device__ inline void load_row_fixed(RowRegs<WT> &q, const RegionDev &rg, const Ell &ell, int i) {
    const uint32_t *cb = reinterpret_cast<const uint32_t *>(ell.a_col + rg.a_ell);
    const WT *vb = (const WT *)ell.a_val + rg.a_ell;
    const uint32_t *zc = reinterpret_cast<const uint32_t *>(ell.zero);
    const WT *zv = reinterpret_cast<const WT *>(ell.zero);
    const int np = (rg.a_w + 1) >> 1, n = rg.n;
    if (OVF) {
        q.om = 0;
        q.ob = 0;
        if (rg.a_ov) {
            q.om = stream_load(ell.a_om + rg.a_om + (i >> 6));
            q.ob = stream_load(ell.a_ob + rg.a_om + (i >> 6));
        }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const bool in = p < np;
        load_pair(q, p, in ? cb + (size_t)p * n + i : zc, in ? vb + 2 * ((size_t)p * n + i) : zv);
    }
    if (rg.w_q > 0)
        q.wc = win_col_implicit(rg, i);
    else
        q.wc = stream_load(ell.w_col + rg.w_ell + i);
    q.wv = stream_load((const WT *)ell.w_val + rg.w_ell + i);
}

// row i's overflow entry, if any: its bit in the word, its index = the word's count +
// the bits below it (kFixed: the balanced update's streaming loads)
template <typename WT, bool kFixed>
__device__ inline void resolve_ovf(RowRegs<WT> &q, const RegionDev &rg, const Ell &ell, int i) {
    const int b = i & 63;
    const uint64_t below = b ? q.om << (64 - b) : 0ull;  // the bits of rows i - b .. i - 1
    q.oh = rg.a_ov && ((q.om >> b) & 1ull);
    const int64_t e = rg.a_oe + q.ob + __popcll(below);
    if (q.oh) {  // (the lanes of the rows one longer: 5-16 % of them where a region has any)
        q.oc = kFixed ? stream_load(ell.a_oc + e) : ell.a_oc[e];
        q.ov = kFixed ? stream_load((const WT *)ell.a_ov + e) : ((const WT *)ell.a_ov)[e];
    }
}

// the reservoir's activation, tanh (mod_reservoir.f90:1447).  OCML's tanh(double) is
// ~150 f64 instructions (a double-double exp and a compensated division): in the
// state update that is more VALU time per row than the row's bytes take to stream
// at 8 TB/s.  tanh(x) = em / (em + 2), em = expm1(2|x|), sign restored: expm1 keeps
// small |x| exact to an ulp (no 1 - 2 / (e + 1) cancellation), the division rounds
// once; |x| > 20 gives 1 (tanh(20) = 1 - 8.5e-18 rounds to 1).  Within 3 ulp of
// glibc's tanh (the oracle's; tests bound states at 1e-14), NaN and -0 preserved.
// Every state update form uses it, so they stay bitwise equal to each other.
__device__ __attribute__((always_inline)) inline double res_tanh(double x) {
    double a = fabs(x);
    a = a > 20.0 ? 20.0 : a;  // (NaN stays NaN)
    const double em = expm1(2.0 * a);
    return copysign(em / (em + 2.0), x);
}

template <typename WT>
__device__ inline int ell_col(const RowRegs<WT> &q, int s) {
    return (int)((q.c[s >> 1] >> (16 * (s & 1))) & 0xffffu);
}

// x_new(i) from the row's loads: y = A x over the main slots in order, then the
// overflow entry (the row's file order: makesparse's blocks, CSR-stable), temp =
// W_in u, tanh, leak -- one expression for every ELL form of the update
template <typename WT>
__device__ __attribute__((always_inline)) inline double ell_row_value(const RowRegs<WT> &q, const RegionDev &rg,
                                                                      const double *xs, const double *fs, int i,
                                                                      double leak) {
    double y = 0.0;
#pragma unroll
    for (int s = 0; s < kEllA; ++s)
        if (s < rg.a_w) y = y + (double)q.v[s] * xs[ell_col(q, s)];
    if (q.oh) y = y + (double)q.ov * xs[q.oc];
    double t = 0.0;
    t = t + (double)q.wv * fs[q.wc];
    const double xn = res_tanh(y + t);
    return (1.0 - leak) * xs[i] + leak * xn;
}

// the CSR copies of one region's A and W_in (rows past the ELL slots, a dense W_in)
template <typename WT>
struct CsrRows {
    const int32_t *rp;
    const uint16_t *ac;
    const WT *av;
    const int32_t *wp;
    const uint16_t *wc;
    const WT *wv;
};

// x_new(i) for a region of any form, from the row's ELL loads (load_row) where the
// region has them and from the CSR copies otherwise: the row of update_block, shared
// with the training drive (k_res_drive) so both give the same bits.  The overflow
// entry, when the region has a list, is fetched here.
template <typename WT>
__device__ __attribute__((always_inline)) inline double row_value(RowRegs<WT> &cur, const RegionDev &rg,
                                                                  const Ell &ell, const CsrRows<WT> &csr,
                                                                  const double *xs, const double *fs, int i,
                                                                  double leak) {
    // y = A x, entries of row i in the file's order (COO semantics, duplicates add)
    double y = 0.0;
    if (rg.a_w > 0) {
        cur.oh = false;
        if (rg.a_ov) resolve_ovf<WT, false>(cur, rg, ell, i);
#pragma unroll
        for (int s = 0; s < kEllA; ++s)
            if (s < rg.a_w) y = y + (double)cur.v[s] * xs[ell_col(cur, s)];
        if (cur.oh) y = y + (double)cur.ov * xs[cur.oc];  // the row's last entry (ell_row_value)
    } else {
        for (int e = csr.rp[i], e1 = csr.rp[i + 1]; e < e1; ++e) y = y + (double)csr.av[e] * xs[csr.ac[e]];
    }
    // temp = W_in feedback
    double t = 0.0;
    if (rg.w_w > 0) {
        t = t + (double)cur.wv * fs[cur.wc];
    } else {
        for (int e = csr.wp[i], e1 = csr.wp[i + 1]; e < e1; ++e) t = t + (double)csr.wv[e] * fs[csr.wc[e]];
    }
    const double xn = res_tanh(y + t);
    return (1.0 - leak) * xs[i] + leak * xn;
}

// update: logical block = (region, part); a part is a contiguous range of rows
// walked in passes of 1024 rows.  With kLds the region's state x and feedback u
// are staged once per block in LDS and the SpMV's random column gathers hit LDS
// instead of the L2 (one L2 transaction per gathered double otherwise).  A and
// W_in are read in ELL form when the region's rows are short (pair-major, RegionDev;
// padding slots hold 0 * x[0] after the row's real entries, so the file-order sum
// is unchanged), otherwise from the CSR copy.  The next pass's ELL loads are issued
// before the current pass computes (the overflow entry, when the region has a list,
// is fetched when the row is computed: this form is not the one the loop runs).
template <typename WT, bool kLds, int kThr = kUpdThreads>
__device__ __attribute__((always_inline)) inline void update_block(
    int lb, double *smem, const RegionDev *__restrict__ R, const int32_t *__restrict__ a_rp,
    const uint16_t *__restrict__ a_col, const WT *__restrict__ a_val, const int32_t *__restrict__ w_rp,
    const uint16_t *__restrict__ w_col, const WT *__restrict__ w_val, const Ell &ell,
    const double *__restrict__ x_old, double *__restrict__ x_new,
    const double *__restrict__ feedback, double leak, int parts, int lds_x) {
    const int r = lb / parts, part = lb % parts;
    const RegionDev rg = R[r];
    const int n = rg.n, tid = threadIdx.x;
    const int per = (n + parts - 1) / parts;
    const int beg = part * per, end = min(n, beg + per);
    if (beg >= end) return;  // block-uniform
    RowRegs<WT> cur, nxt;
    load_row(cur, rg, ell, beg + tid, beg + tid < end);
    const double *xo = x_old + rg.x;
    const double *fb = feedback + rg.fb;
    const double *xs = xo, *fs = fb;
    if (kLds) {
        double *sx = smem, *sf = smem + lds_x;
        for (int j = tid; j < n; j += kThr) sx[j] = xo[j];
        for (int j = tid; j < rg.ninp; j += kThr) sf[j] = fb[j];
        __syncthreads();
        xs = sx;
        fs = sf;
    }
    const CsrRows<WT> csr{a_rp + rg.a_rp, a_col + rg.a_nz, a_val + rg.a_nz, w_rp + rg.w_rp, w_col + rg.w_nz,
                          w_val + rg.w_nz};
    for (int base = beg; base < end; base += kThr) {
        const int i = base + tid;
        const bool live = i < end;
        const int inext = i + kThr;
        if (base + kThr < end) load_row(nxt, rg, ell, inext, inext < end);
        if (live)  // (x~ = x with x(2:n:2)**2: squared by the readout's loads, rd_x)
            x_new[rg.x + i] = row_value(cur, rg, ell, csr, xs, fs, i, leak);
        cur = nxt;
    }
}

}  // namespace
