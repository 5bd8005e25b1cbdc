// sml_dyn_spec_math.hpp -- the spectral-space arithmetic of one coefficient (m, n):
// uvspec, geop, the table views (TabM / GTab / LTab), vds and the combine helpers, and
// the step's tail (sptend, geop, implic, hordif, timint) in its two halves.  Device
// functions only; the unfused and the fused kernels share them, which is what keeps the
// two step forms bit-identical.
#pragma once
#include <hip/hip_runtime.h>

#include "sml_dyn_layout.hpp"
#include "sml_dynamics_tables.hpp"

namespace {
using namespace sml;

// uvspec(vor, div) -> (ucos, vcos) at coefficient (m, n), both parts
// (spe_spectral.f90:351-387)
__device__ inline void uvspec_at(const double *vor, const double *div, const DynTables *T, int m, int n, double *uc,
                                 double *vc) {
    const double ux = T->uvdx[n][m];
    double zp[2], zc[2];
    zp[1] = ux * vor[ci(0, m, n)];
    zp[0] = -ux * vor[ci(1, m, n)];
    zc[1] = ux * div[ci(0, m, n)];
    zc[0] = -ux * div[ci(1, m, n)];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        double a, b;
        if (n == 0) {
            a = zc[p] - T->uvdyp[0][m] * vor[ci(p, m, 1)];
            b = zp[p] + T->uvdyp[0][m] * div[ci(p, m, 1)];
        } else if (n == kNX - 1) {
            a = T->uvdym[n][m] * vor[ci(p, m, kNTRUN1 - 1)];
            b = -T->uvdym[n][m] * div[ci(p, m, kNTRUN1 - 1)];
        } else {
            b = -T->uvdym[n][m] * div[ci(p, m, n - 1)] + T->uvdyp[n][m] * div[ci(p, m, n + 1)] + zp[p];
            a = T->uvdym[n][m] * vor[ci(p, m, n - 1)] - T->uvdyp[n][m] * vor[ci(p, m, n + 1)] + zc[p];
        }
        uc[ci(p, m, n)] = a;
        vc[ci(p, m, n)] = b;
    }
}

// geop(1) at level k of one real coefficient c = 2 (m + mx n) + p (dyn_geop.f90:16-32):
// the hydrostatic sum from the bottom, then the free-troposphere lapse-rate
// correction of the zonal-mean row; t = level-1 temperature, all kx levels
__device__ inline double geop_at(const double *t, const double *phis, const DynTables *T, int c, int m, int k) {
    double phi = phis[c] + T->xgeop1[kKX - 1] * t[(size_t)(kKX - 1) * kSF + c];
    for (int kk = kKX - 2; kk >= k; --kk)
        phi = phi + T->xgeop2[kk + 1] * t[(size_t)(kk + 1) * kSF + c] + T->xgeop1[kk] * t[(size_t)kk * kSF + c];
    if (m == 0 && k >= 1 && k <= kKX - 2)
        phi = phi + T->corf[k] * (t[(size_t)(k + 1) * kSF + c] - t[(size_t)(k - 1) * kSF + c]);
    return phi;
}

// Table access for the spectral-space stages of one zonal wavenumber m: GTab reads
// the DynTables in device memory (unfused kernels), LTab a per-m copy staged in LDS
// (TabM, the fused k_st_spec).  Vectors by level k, per-(n, m) tables by n, and
// xj(n, k1, k) = xj[m + n - 1][k1][k] (implic's matrix of ll = m + n).
struct TabM {
    double dhs[kKX], dhsr[kKX], fsgr[kKX], tref[kKX], tref1[kKX], tref2[kKX], tref3[kKX];
    double xgeop1[kKX], xgeop2[kKX], corf[kKX], tcorv[kKX], qcorv[kKX], dhsx[kKX];
    double xc[kKX][kKX], xd[kKX][kKX];
    double el2[kNX], elz[kNX], dmp[kNX], dmp1[kNX], dmpd[kNX], dmp1d[kNX], dmps[kNX], dmp1s[kNX], trfilt[kNX];
    double vddym[kNX], vddyp[kNX], gradym[kNX], gradyp[kNX], uvdx[kNX], uvdym[kNX], uvdyp[kNX];
    double gradx, pad_;
    double xj[kKX][kKX][kNX];  // [k1][k][n]: n fastest, so a wave's lanes (one n each) hit distinct LDS banks
};
constexpr int kTabMDoubles = (int)(sizeof(TabM) / sizeof(double));
constexpr int kTabMPad = 2048;  // d_tabm tail: k_st_spec stages whole 16-B rows of 512 threads
static_assert(kTabMDoubles % 2 == 0, "TabM is copied in 16-B pieces");

#define SML_TAB_VEC(X) \
    X(dhs) X(dhsr) X(fsgr) X(tref) X(tref1) X(tref2) X(tref3) X(xgeop1) X(xgeop2) X(corf) X(tcorv) X(qcorv) X(dhsx)
#define SML_TAB_NM(X)                                                                                       \
    X(el2) X(elz) X(dmp) X(dmp1) X(dmpd) X(dmp1d) X(dmps) X(dmp1s) X(trfilt) X(vddym) X(vddyp) X(gradym) \
        X(gradyp) X(uvdx) X(uvdym) X(uvdyp)

struct GTab {
    const DynTables *T;
    int m;
#define X(name) \
    __device__ double name(int k) const { return T->name[k]; }
    SML_TAB_VEC(X)
#undef X
#define X(name) \
    __device__ double name##_n(int n) const { return T->name[n][m]; }
    SML_TAB_NM(X)
#undef X
    __device__ double gradx_m() const { return T->gradx[m]; }
    __device__ double xc(int k1, int k) const { return T->xc[k1][k]; }
    __device__ double xd(int k1, int k) const { return T->xd[k1][k]; }
    __device__ double xj(int n, int k1, int k) const { return T->xj[m + n - 1][k1][k]; }
};

struct LTab {
    const TabM *t;
#define X(name) \
    __device__ double name(int k) const { return t->name[k]; }
    SML_TAB_VEC(X)
#undef X
#define X(name) \
    __device__ double name##_n(int n) const { return t->name[n]; }
    SML_TAB_NM(X)
#undef X
    __device__ double gradx_m() const { return t->gradx; }
    __device__ double xc(int k1, int k) const { return t->xc[k1][k]; }
    __device__ double xd(int k1, int k) const { return t->xd[k1][k]; }
    __device__ double xj(int n, int k1, int k) const { return t->xj[k1][k][n]; }
};

// the value at flat index i of m's TabM, read from the DynTables (host: the per-slot
// TabM copies built at impint time)
__host__ __device__ inline double tabm_value(const DynTables *__restrict__ T, int m, int i) {
    const TabM *z = nullptr;
    const size_t off = (size_t)i * sizeof(double);
#define X(name)                                                                             \
    {                                                                                       \
        const size_t a = offsetof(TabM, name), b = a + sizeof(z->name);                      \
        if (off >= a && off < b) return T->name[(off - a) / sizeof(double)];                 \
    }
    SML_TAB_VEC(X)
#undef X
#define X(name)                                                                             \
    {                                                                                       \
        const size_t a = offsetof(TabM, name), b = a + sizeof(z->name);                      \
        if (off >= a && off < b) return T->name[(off - a) / sizeof(double)][m];              \
    }
    SML_TAB_NM(X)
#undef X
    if (off >= offsetof(TabM, xc) && off < offsetof(TabM, xc) + sizeof(z->xc))
        return (&T->xc[0][0])[(off - offsetof(TabM, xc)) / sizeof(double)];
    if (off >= offsetof(TabM, xd) && off < offsetof(TabM, xd) + sizeof(z->xd))
        return (&T->xd[0][0])[(off - offsetof(TabM, xd)) / sizeof(double)];
    if (off == offsetof(TabM, gradx)) return T->gradx[m];
    if (off >= offsetof(TabM, xj)) {
        const int q = (int)((off - offsetof(TabM, xj)) / sizeof(double));
        const int k1 = q / (kKX * kNX), k = (q / kNX) % kKX, n = q % kNX;
        return m + n >= 1 ? T->xj[m + n - 1][k1][k] : 0.0;
    }
    return 0.0;
}

// vds (spe_spectral.f90:307-349) divergence / vorticity of one coefficient;
// u(pp, nn), v(pp, nn) read part pp of coefficient (m, nn)
template <class U, class V, class TB>
__device__ inline void vds_gen(U u, V v, const TB &tb, int n, int p, double *vor, double *div) {
    const double gx = tb.gradx_m();
    // zp(2)=gradx*u(1), zp(1)=-gradx*u(2); zc likewise from v
    const double ux = u(1 - p, n), vx = v(1 - p, n);
    const double zp = p == 1 ? gx * ux : -gx * ux;
    const double zc = p == 1 ? gx * vx : -gx * vx;
    // the n == 1 / n == ntrun+2 / interior cases all formed (neighbours clamped into
    // the row), then selected: the reference's values without divergent branches,
    // whose dependent reads cost a round trip per case where u, v live in LDS
    static_assert(kNTRUN1 - 1 == kNX - 2, "vds's last row reads n - 1");
    const int nm = n > 0 ? n - 1 : 0, np = n < kNX - 1 ? n + 1 : kNX - 1;
    const double um = u(p, nm), up = u(p, np), vm = v(p, nm), vp = v(p, np);
    const double dym = tb.vddym_n(n), dyp = tb.vddyp_n(n);
    const double vor0 = zc - dyp * up, div0 = zp + dyp * vp;
    const double vorl = dym * um, divl = -dym * vm;
    const double vori = dym * um - dyp * up + zc, divi = -dym * vm + dyp * vp + zp;
    *vor = n == 0 ? vor0 : n == kNX - 1 ? vorl : vori;
    *div = n == 0 ? div0 : n == kNX - 1 ? divl : divi;
}

__device__ inline void vds_at(const double *u, const double *v, const DynTables *T, int m, int n, int p, double *vor,
                              double *div) {
    vds_gen([&](int pp, int nn) { return u[ci(pp, m, nn)]; }, [&](int pp, int nn) { return v[ci(pp, m, nn)]; },
            GTab{T, m}, n, p, vor, div);
}

// tail: sptend + geop + implic + hordif + drag + timint of one real coefficient c
// (= Re/Im of (m, n)) at level k, given grtend's spectral tendencies of (c, k).
// The CW coefficients x 8 levels of a block share sh[3][kx][CW] (LDS) for the
// vertical couplings (dmeanc, sigdtc, geop, implic's level matrices); every sum
// runs over k in the reference's order.  The whole block must call it (barriers).
// KU: the caller's k is wave-uniform (a scalar: CW == 64, one level per wave).  What
// depends on k alone is then decided by uniform branches -- the level loops end at the
// wave's level instead of forming every level's term and selecting it away.  The
// compiler then places a level's reads in that level's branch; pinning them in one
// batch ahead of the branches measured no faster (profiles/spec_kernel_uniform.md).
// Either way every value stored is formed by the same expression on the same operands.
//
// The tail comes in two halves.  tail_pre is the stage that reads the state and the
// tables only -- sptend's dmeanc and sigdtc chain, geop's phi with lapd, hordif's
// corrected t and tr -- and none of grtend's tendencies: k_st_spec runs it while specy's
// Fourier operands are still in flight.  tail_post is everything from
// psdt = psdt - dmeanc on and holds all of implic's barriers.  Only values that were
// separate values in the one-piece form cross from one half to the other, so
// -ffp-contract=on contracts the same products into the same FMAs.
struct TailPre {
    double dmeanc, sig_k, sig_k1, dumk_k, dumk_k1, lapd, ctmp, cq;
};

// L(v, kk): every level's div (v = 0) and t (v = 1) at time level j4 of this coefficient,
// as the other levels' threads hold them (the caller has made them visible)
template <bool KU, class SA, class LV, class TB>
__device__ inline TailPre tail_pre(SA S, LV L, double *__restrict__ phi_out, const double *__restrict__ phis,
                                   const double *__restrict__ tcorh, const double *__restrict__ qcorh, int fc,
                                   const TB &tb, int k, int c, int m, int n, int j4) {
    TailPre r;
    // ---- sptend(divdt, tdt, psdt, j4)  (dyn_sptend.f90:29-66)
    // every level's operands of sptend (div, dhs) and of geop (t, xgeop1 / 2)
    double d0[kKX], dh[kKX], t1[kKX], g1[kKX], g2[kKX];
#pragma unroll
    for (int kk = 0; kk < kKX; ++kk) {
        d0[kk] = L(0, kk);
        dh[kk] = tb.dhs(kk);
        t1[kk] = L(1, kk);
        g1[kk] = tb.xgeop1(kk);
        g2[kk] = kk > 0 ? tb.xgeop2(kk) : 0.0;  // (xgeop2(1) is not used)
    }
    // (neighbour levels clamped and the edge cases selected: no branch around a read)
    const int km = k > 0 ? k - 1 : 0, kp = k < kKX - 1 ? k + 1 : kKX - 1;
    // the level's own scalars of sptend and geop
    const double trk = tb.tref(k), trm = tb.tref(km), trp = tb.tref(kp), phis_c = phis[fc], corf_k = tb.corf(k);
    double dmeanc = 0.0;
#pragma unroll
    for (int kk = 0; kk < kKX; ++kk) dmeanc = dmeanc + d0[kk] * dh[kk];
    double sig_k = 0.0, sig_k1 = 0.0;  // sigdtc(k), sigdtc(k+1); sigdtc(1) = sigdtc(kxp) = 0
    if constexpr (KU) {
        // the chain ends once sigdtc(k+1) is formed (uniform): sgp, sg = the last two terms
        double sg = 0.0, sgp = 0.0;
#pragma unroll
        for (int kk = 0; kk < kKX - 1; ++kk) {
            if (kk > k) break;
            const double nx_ = sg - dh[kk] * (d0[kk] - dmeanc);
            sgp = sg;
            sg = nx_;
        }
        if (k == kKX - 1) {  // ended at kk = k - 1; sigdtc(kxp) = 0
            sig_k = sg;
        } else {             // ended at kk = k (sgp = sigdtc(1) = 0 at k = 0)
            sig_k = sgp;
            sig_k1 = sg;
        }
    } else {
        double sg = 0.0;
#pragma unroll
        for (int kk = 0; kk < kKX - 1; ++kk) {
            const double nx_ = sg - dh[kk] * (d0[kk] - dmeanc);
            if (kk == k - 1) sig_k = nx_;
            if (kk == k) sig_k1 = nx_;
            sg = nx_;
        }
    }
    r.dmeanc = dmeanc;
    r.sig_k = sig_k;
    r.sig_k1 = sig_k1;
    r.dumk_k = (k == 0) ? 0.0 : sig_k * (trk - trm);
    r.dumk_k1 = (k == kKX - 1) ? 0.0 : sig_k1 * (trp - trk);
    // geop(j4)  (dyn_geop.f90:16-32)
    // (every level's term formed, the ones below k selected away: the sum and its
    // order are the reference's, and the LDS reads issue together instead of one
    // dependent round trip per level of a runtime-bounded loop.  KU: the sum stops at
    // the wave's level by a uniform branch, its operands read above)
    double phi = phis_c + g1[kKX - 1] * t1[kKX - 1];
#pragma unroll
    for (int kk = kKX - 2; kk >= 0; --kk) {
        if constexpr (KU)
            if (kk < k) break;  // (uniform)
        const double nx = phi + g2[kk + 1] * t1[kk + 1] + g1[kk] * t1[kk];
        phi = kk >= k ? nx : phi;
    }
    {
        const double pc = phi + corf_k * (L(1, kp) - L(1, km));
        if (m == 0 && k >= 1 && k <= kKX - 2) phi = pc;
    }
    if (phi_out) phi_out[(size_t)k * kSF + c] = phi;
    {
        const double d1 = phi + kRgas * trk * S(4, j4, 0);
        r.lapd = -(d1 * tb.el2_n(n));
    }
    // hordif's corrected temperature and tracer (dyn_step.f90:60-112)
    r.ctmp = S(2, 1, k) + tcorh[fc] * tb.tcorv(k);
    r.cq = S(3, 1, k) + qcorh[fc] * tb.qcorv(k);
    return r;
}

template <int CW, class SA, class TB>
__device__ inline void tail_post(SA S, const TailPre &pre, double *__restrict__ Td, const TB &tb,
                                 double (*sh)[kKX][CW], int cc, int k, int c, int m, int n, double vordt, double divdt,
                                 double tdt, double trdt, double psdt, int j1, double dt, double alph, double rob,
                                 double wil) {
    const double dmeanc = pre.dmeanc, sig_k = pre.sig_k, sig_k1 = pre.sig_k1, dumk_k = pre.dumk_k,
                 dumk_k1 = pre.dumk_k1, ctmp = pre.ctmp;
    const double dhsr_k = tb.dhsr(k), tref3_k = tb.tref3(k), tref2_k = tb.tref2(k);
    psdt = psdt - dmeanc;
    if (m == 0 && n == 0) psdt = 0.0;  // psdt(1,1) = 0
    tdt = tdt - (dumk_k1 + dumk_k) * dhsr_k + tref3_k * (sig_k1 + sig_k) - tref2_k * dmeanc;
    divdt = divdt - pre.lapd;
    // ---- implic(divdt, tdt, psdt)  (dyn_implic.f90:22-67)
    if (alph != 0.0) {
        // tdt into the third plane: sptend's reads of sh[0] need no barrier of their
        // own before it (sh[1]'s geop reads end at the next one, before yf is written)
        sh[2][k][cc] = tdt;
        __syncthreads();
        double ye = 0.0;
#pragma unroll
        for (int k1 = 0; k1 < kKX; ++k1) ye = ye + tb.xd(k1, k) * sh[2][k1][cc];
        ye = ye + tb.tref1(k) * psdt;
        sh[1][k][cc] = divdt + tb.elz_n(n) * ye;  // yf
        __syncthreads();
        divdt = 0.0;
        const int ll = m + n;
        if (ll != 0) {
#pragma unroll
            for (int k1 = 0; k1 < kKX; ++k1) divdt = divdt + tb.xj(n, k1, k) * sh[1][k1][cc];
        }
        sh[0][k][cc] = divdt;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kKX; ++kk) psdt = psdt - sh[0][kk][cc] * tb.dhsx(kk);
#pragma unroll
        for (int k1 = 0; k1 < kKX; ++k1) tdt = tdt + tb.xc(k1, k) * sh[0][k1][cc];
    }
    // ---- horizontal diffusion (dyn_step.f90:60-112, hordif :130-151)
    const double dmp = tb.dmp_n(n), dmp1 = tb.dmp1_n(n), dmpd = tb.dmpd_n(n), dmp1d = tb.dmp1d_n(n);
    vordt = (vordt - dmp * S(0, 1, k)) * dmp1;
    divdt = (divdt - dmpd * S(1, 1, k)) * dmp1d;
    tdt = (tdt - dmp * ctmp) * dmp1;
    if (k == 0) {
        if (m == 0) {  // stratospheric drag on the zonal mean, top level (:78-82)
            const double sdrag = 1. / (kTdrs * 3600.);
            vordt = vordt - sdrag * S(0, 1, 0);
            divdt = divdt - sdrag * S(1, 1, 0);
        }
        const double dmps = tb.dmps_n(n), dmp1s = tb.dmp1s_n(n);
        vordt = (vordt - dmps * S(0, 1, 0)) * dmp1s;
        divdt = (divdt - dmps * S(1, 1, 0)) * dmp1s;
        tdt = (tdt - dmps * ctmp) * dmp1s;
    }
    trdt = (trdt - dmpd * pre.cq) * dmp1d;
    if (dt <= 0.0) {  // tendencies only (dyn_step.f90:109)
        if (!Td) return;
        Td[kTVor + (size_t)k * kSF + c] = vordt;
        Td[kTDiv + (size_t)k * kSF + c] = divdt;
        Td[kTT + (size_t)k * kSF + c] = tdt;
        Td[kTTr + (size_t)k * kSF + c] = trdt;
        if (k == 0) Td[kTPs + c] = psdt;
        return;
    }
    // ---- timint with the Robert-Williams filter (dyn_step.f90:153-190)
    const double eps = (j1 == 1) ? 0.0 : rob;
    const double trf = tb.trfilt_n(n);
    auto timint = [&](int var, int kk, double fdt) {
        fdt = fdt * trf;  // trunct
        double &f1 = S(var, 1, kk);
        double &f2 = S(var, 2, kk);
        const double fj1_old = (j1 == 1) ? f1 : f2;
        const double fnew = f1 + dt * fdt;
        const double f1new = fj1_old + wil * eps * (f1 - 2 * fj1_old + fnew);
        const double fj1_new = (j1 == 1) ? f1new : fj1_old;
        f2 = fnew - (1 - wil) * eps * (f1new - 2 * fj1_new + fnew);
        f1 = f1new;
    };
    if (k == 0) timint(4, 0, psdt);
    timint(0, k, vordt);
    timint(1, k, divdt);
    timint(2, k, tdt);
    timint(3, k, trdt);
}

// the whole tail (k_dyn_tail): the levels' div and t of time level j4 meet in sh[0] /
// sh[1], then tail_pre and tail_post
template <int CW, bool KU, class SA, class TB>
__device__ inline void tail_coef(SA S, double *__restrict__ Td, double *__restrict__ phi_out,
                                 const double *__restrict__ phis, const double *__restrict__ tcorh,
                                 const double *__restrict__ qcorh, int fc, const TB &tb,
                                 double (*sh)[kKX][CW], int cc, int k, int c, int m, int n, double vordt, double divdt,
                                 double tdt, double trdt, double psdt, int j1, int j4, double dt, double alph,
                                 double rob, double wil) {
    // S(var, lev, kk): the state of coefficient c (var 0..4 = vor, div, t, tr, ps at
    // kk = 0; lev 1 or 2), updated in place; phis / tcorh / qcorh at index fc
    sh[0][k][cc] = S(1, j4, k);
    sh[1][k][cc] = S(2, j4, k);
    __syncthreads();
    const TailPre pre = tail_pre<KU>(S, [&](int v, int kk) { return sh[v][kk][cc]; }, phi_out, phis, tcorh, qcorh, fc,
                                     tb, k, c, m, n, j4);
    tail_post<CW>(S, pre, Td, tb, sh, cc, k, c, m, n, vordt, divdt, tdt, trdt, psdt, j1, dt, alph, rob, wil);
}

}  // namespace
