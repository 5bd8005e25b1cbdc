// sml_physics_pair.hpp -- phypar's longwave / surface side (and, on a shortwave step, its
// shortwave) on two lanes per column: the row kernel whose three roles each have waves
// of their own (k_st_gridspec_p, sml_dyn_fused.hpp).
//
// Reference: phypar (src/phy_phypar.f90:121-179) -- radsw (phy_radiat.f90:154-328), radlw
// (:330-458), suflux (phy_suflux.f90:1-355) -- with the expressions of sml_physics.hpp.
//
// Layout.  Lanes 2i and 2i + 1 own column i; lane h owns the levels 4h .. 4h + 3 (the
// shortwave transmissivities t1 / t2, the heating rates' scaling, the flux divergences)
// and the longwave bands 2h, 2h + 1 (their eight transmissivities, fband rows and flux
// recurrences down and up).  The column-wide chains (on a shortwave step the moist part,
// cloud and radsw's flux chains; suflux) run on both lanes alike.  The partners trade
// values by DPP (one row permutation per double, no LDS), so every level's divergence
// adds the four bands' fluxes in radlw's order: bitwise the one-lane form.
//
// A shortwave step in two stages.  The moist side hands its results (precnv, precls, itop,
// rh) over at a block barrier, and the pair waves have nothing else to do before it: so
// everything of the shortwave path that reads neither the hand-over nor the cloud runs
// before that barrier (phys_pair_sw_pre: the A row, psg, the boundary loads, clstr's
// stability factor, t2, the transmissivities of levels 1, 2 and 8, radlw's blackbody
// terms -- 10 of the lane's 24 exp evaluations and psg's), and phys_pair does the rest
// after it.  Whole statements moved, none split: every exp argument and every contracted
// expression is the same double as in the one-stage form.
#pragma once
#include "sml_physics.hpp"

namespace sml {
#ifdef __HIPCC__

// a longwave-only step's radiation state for lane h: bands 2h, 2h + 1 and its four levels of tt_rsw
struct PairPre {
    double tau[2][kKX];
    double strat0, strat1, ssrd, ttrsw[4];
};

// lane h's share of phys_column's results: its four levels (the shortwave heating: LDS,
// phys_pair's mh), the surface fluxes
struct PairOut {
    double rlw[4];
    double ust, vst, shf, evp, rps;
};

// radlw(1)'s surface emission row fband(nint(tsfc), jb) of column pt (suflux's tsfc =
// sst + fmask (stl - sst), phy_suflux.f90, from the boundary fields alone): the row
// kernel stages it during gridx, off the physics' chain of dependent loads
__device__ __forceinline__ double sfc_fband(const double *__restrict__ bc, const double *__restrict__ fbt, int pt,
                                            int jb) {
    const double tsea = bc[(size_t)kBcSst * kNGP + pt], fmask = bc[(size_t)kBcFmask1 * kNGP + pt];
    const double stl = bc[(size_t)kBcStl * kNGP + pt];
    const double tsfc = tsea + fmask * (stl - tsea);
    return phys::fband_row(fbt, tsfc)[jb];
}

// a shortwave step's values of pair lane h that wait for neither the moist side nor the
// cloud (phys_pair_sw_pre -> phys_pair across the hand-over barrier)
struct PairSw {
    double ta[kKX], qc[kKX], ph7;  // the A row: t, clipped q, the bottom level's phi
    double psg, rps, fst, psaz;    // exp(ps), its inverse, clstr's stability factor, psg x zenit
    double fmask, fsol, ozupp, ozone, albsfc, stratz;  // boundary fields of the shortwave path
    double o2[4];                  // radsw's t2 of the lane's levels
    double tqe[2][3];              // bands 2h, 2h + 1 at levels 1, 2 and 8
    double st4a1[kKX], st4a2[kKX];  // radlw(-1)'s blackbody terms
};

namespace pairx {

// the partner's value (lanes ^ 1: DPP quad permutation 1 0 3 2)
__device__ __forceinline__ double swap(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_mov_dpp((int)b, 0xB1, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), 0xB1, 0xF, 0xF, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// level 4 h + j of a whole-column array (h a lane value, j compile-time)
__device__ __forceinline__ double own(const double (&a)[kKX], int h, int j) { return h ? a[4 + j] : a[j]; }
// level 4 (1 - h) + j (the partner's levels)
__device__ __forceinline__ double oth(const double (&a)[kKX], int h, int j) { return h ? a[j] : a[4 + j]; }

// radlw(-1)'s blackbody terms (phy_radiat.f90:330-413), which need ta alone
__device__ __forceinline__ void blackbody(const double (&ta)[kKX], const PhysTables *P, double (&st4a1)[kKX],
                                          double (&st4a2)[kKX]) {
    using namespace phys;
    constexpr int NL = kKX, nl1 = kKX - 1;
#pragma unroll
    for (int k = 1; k <= nl1; ++k) st4a1[k - 1] = ta[k - 1] + P->wvi[k - 1][1] * (ta[k] - ta[k - 1]);
    st4a2[0] = 0.75 * ta[0] + 0.25 * st4a1[0];
    st4a2[1] = 0.50 * ta[1] + 0.25 * (st4a1[0] + st4a1[1]);
    {
        const double anis = 1.0, anish = 0.5 * anis;
#pragma unroll
        for (int k = 3; k <= nl1; ++k) st4a2[k - 1] = anish * fmax(st4a1[k - 1] - st4a1[k - 2], 0.);
        st4a2[NL - 1] = anis * fmax(ta[NL - 1] - st4a1[nl1 - 1], 0.);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double x = st4a2[k];
        st4a1[k] = sbc * ((x * x) * (x * x));
        st4a2[k] = 0.;
    }
#pragma unroll
    for (int k = 3; k <= NL; ++k) {
        const double t = ta[k - 1];
        const double st3a = sbc * (t * t * t);
        st4a1[k - 1] = st3a * t;
        st4a2[k - 1] = 4. * st3a * st4a2[k - 1];
    }
}

}  // namespace pairx

// The first stage of a shortwave step on pair lane h (column pt, its row Ai in A): what
// phys_pair's shortwave path needs that depends on neither the moist side's hand-over
// nor the cloud, run while the moist side works.
template <int kOT, int kOQ, int kOPhi, int kOPs>
__device__ __forceinline__ void phys_pair_sw_pre(int h, int pt, const double *Ai, const double *__restrict__ bc,
                                                 const PhysTables *P, PairSw &w) {
    using namespace phys;
    using pairx::own;
    constexpr int NL = kKX;
    auto BC = [&](int f) { return bc[(size_t)f * kNGP + pt]; };
    // the boundary loads first: memory round trips that the arithmetic below covers
    w.fmask = BC(kBcFmask1);
    const double zenit = BC(kBcZenit);
    w.fsol = BC(kBcFsol);
    w.ozupp = BC(kBcOzupp);
    w.ozone = BC(kBcOzone);
    w.albsfc = BC(kBcAlbsfc);
    w.stratz = BC(kBcStratz);
    double qa[NL], ph[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        w.ta[k] = Ai[kOT + k];
        qa[k] = Ai[kOQ + k];
        ph[k] = Ai[kOPhi + k];
    }
    const double ps1 = Ai[kOPs];
    w.ph7 = ph[NL - 1];
    const double psg = exp(ps1);
    w.psg = psg;
    w.rps = 1. / psg;
#pragma unroll
    for (int k = 0; k < NL; ++k) w.qc[k] = fmax(qa[k], 0.);
    double se[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) se[k] = cp * w.ta[k] + ph[k];
    const double gse = (se[NL - 2] - se[NL - 1]) / (ph[NL - 2] - ph[NL - 1]);
    {
        const double rgse = 1. / (gse_s1 - gse_s0);
        const double fst = fmax(0., fmin(1., rgse * (gse - gse_s0)));
        w.fst = fst;
    }
    // radsw's t2 of the lane's levels (phy_radiat.f90:190-214; the top level has none)
    const double psaz = psg * zenit;
    w.psaz = psaz;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int L = 4 * h + j, k = L + 1;
        const double qk = own(w.qc, h, j);
        const double e2 = exp(-(psaz * P->dsig[k - 1]) * abswv2 * qk);
        w.o2[j] = L >= 1 ? e2 : 0.0;
    }
    // the longwave transmissivities outside the cloud's levels: k = 1, 2 and 8 of bands
    // 2h, 2h + 1 (phy_radiat.f90:262-300; bands 2 and 3 are 1 at the top level)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int k = i < 2 ? i + 1 : NL;
            const double deltap = psg * P->dsig[k - 1];
            const double qk = w.qc[k - 1];
            double e;
            if (k == 1) {  // bands 0 and 1 (lane 0)
                const double a0 = -deltap * ablwin;
                const double a1 = -deltap * ablco2;
                e = exp(b == 0 ? a0 : a1);
                e = h ? 1. : e;
            } else if (b == 0) {  // band 0 (h = 0) or 2 (h = 1)
                const double a0 = -deltap * ablwin;
                const double a2 = -deltap * ablwv1 * qk;
                e = exp(h ? a2 : a0);
            } else {  // band 1 (h = 0) or 3 (h = 1)
                const double a1 = -deltap * ablco2;
                const double a3 = -deltap * ablwv2 * qk;
                e = exp(h ? a3 : a1);
            }
            w.tqe[b][i] = e;
        }
    }
    pairx::blackbody(w.ta, P, w.st4a1, w.st4a2);
}

// The longwave / surface chain of column pt on pair lane h (and the shortwave before it
// on a lradsw step).  Ai: the column's row in A (t, q, phi at kOT / kOQ / kOPhi + k,
// log ps at kOPs); u7 / v7: the bottom level's wind (x cosgr); fsr: fband(nint(tsfc),
// 2h + b) for b = 0, 1; P: PhysTables (LDS copy); fbt: fband (global); mh: on a
// shortwave step the moist side's precnv, precls, itop and rh of the column (LDS); sw: on
// a shortwave step the first stage's values (phys_pair_sw_pre, before the hand-over);
// pre_load(PairPre &): loads a longwave-only step's radiation state.  The lane's four
// levels of the shortwave heating tt_rsw are not needed before the sums: they wait in LDS,
// mh[4h + j] (the hand-over's slots, read by then), not in registers held through radlw
// and suflux (which went to scratch, on a longwave-only step between its loads).  The two kinds of
// step share no branch but the one below: the first stage's values (sw) and the radiation
// state (PairPre) are never live together (as two branches in a row they were, and the
// longwave-only step spilled loaded values between its loads, +0.2 us).
template <int kOT, int kOQ, int kOPhi, int kOPs, class PreLoad>
__device__ __forceinline__ void phys_pair(int h, int pt, int jlat, const double *Ai, double u7, double v7,
                                          PreLoad &&pre_load, const double *__restrict__ bc, double *__restrict__ rad,
                                          const PhysTables *P, const double *__restrict__ fbt, const double (&fsr)[2],
                                          double *mh, bool lradsw, const PairSw &sw, PairOut &o) {
    using namespace phys;
    using pairx::oth;
    using pairx::own;
    using pairx::swap;
    constexpr int NL = kKX, nl1 = kKX - 1;  // nl1: 1-based index of the level above the bottom
    auto BC = [&](int f) { return bc[(size_t)f * kNGP + pt]; };

    // the A row (on a shortwave step the first stage read it); bands 2h, 2h + 1's fband
    // rows (radlw, both passes): issued as soon as ta is known on a longwave-only step,
    // after the shortwave on a shortwave step (registers)
    double ta[NL], ph7;
    double fbq[2][NL];
    auto load_fbq = [&]() {
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int k = 0; k < NL; ++k) fbq[b][k] = fband_row(fbt, ta[k])[2 * h + b];
    };

    double psg, rps, qc[NL];
    double tq[2][NL], strat0, strat1, ssrd;
    double st4a1[NL], st4a2[NL];  // radlw(-1)'s blackbody terms
    if (lradsw) {
        // the moist part's results from the moist side (mh: precnv, precls, itop, rh(1..8),
        // phys_moist / phys_thermo's values, handed over at the block barrier of a
        // shortwave step), then cloud and radsw (phys_sw) level- and band-split; what
        // needs neither comes from the first stage
        psg = sw.psg;
        rps = sw.rps;
        ph7 = sw.ph7;
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            ta[k] = sw.ta[k];
            qc[k] = sw.qc[k];
            st4a1[k] = sw.st4a1[k];
            st4a2[k] = sw.st4a2[k];
        }
        const double precnv = mh[0], precls = mh[1];
        const int itop = (int)mh[2];
        double rh[NL];
#pragma unroll
        for (int k = 0; k < NL; ++k) rh[k] = mh[3 + k];
        const double *qa_ = qc;
        constexpr int nlp = NL + 1;
        const double rrcl = 1. / (rhcl2 - rhcl1);
        double cloudc, clstr;
        int icltop;
        if (rh[nl1 - 1] > rhcl1) {
            cloudc = rh[nl1 - 1] - rhcl1;
            icltop = nl1;
        } else {
            cloudc = 0.;
            icltop = nlp;
        }
#pragma unroll
        for (int k = 3; k <= NL - 2; ++k) {
            const double drh = rh[k - 1] - rhcl1;
            if (drh > cloudc && qa_[k - 1] > qacl) {
                cloudc = drh;
                icltop = k;
            }
        }
        const double cl1 = fmin(1., cloudc * rrcl);
        const double pr1 = fmin(pmaxcl, 86.4 * (precnv + precls));
        cloudc = fmin(1., wpcl * sqrt(pr1) + cl1 * cl1);
        icltop = (itop < icltop) ? itop : icltop;
        const double qcloud = qa_[nl1 - 1];
        {
            const double clfact = 1.2;
            const double fst = sw.fst;
            clstr = fst * fmax(clsmax - clfact * cloudc, 0.);
            const double clstrl = fmax(clstr, clsminl) * rh[NL - 1];
            clstr = clstr + sw.fmask * (clstrl - clstr);
        }
        // radsw's t1 of the lane's levels (phy_radiat.f90:190-214; t2: the first stage), then
        // the column's
        const double fband2 = 0.05, fband1 = 1. - fband2;
        const double psaz = sw.psaz;
        const double acloud = cloudc * fmin(abscl1 * qcloud, abscl2);
        double t1[NL], t2[NL], t3[NL], dfabs[NL];
        {
            double o1[4], o2[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int L = 4 * h + j, k = L + 1;
                const double qk = own(qc, h, j);
                const double abs1 = absdry + absaer * P->sig[k - 1] * P->sig[k - 1];
                const double deltap = psaz * P->dsig[k - 1];
                const double a0 = -(psaz * P->dsig[k - 1]) * absdry;
                const double ax = -deltap * (abs1 + abswv1 * qk + acloud);
                const double ay = -deltap * (abs1 + abswv1 * qk);
                o1[j] = exp(L == 0 ? a0 : (L < NL - 1 && k >= icltop) ? ax : ay);
                o2[j] = sw.o2[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double w1 = swap(o1[j]), w2 = swap(o2[j]);
                t1[j] = h ? w1 : o1[j];
                t1[4 + j] = h ? o1[j] : w1;
                t2[j] = h ? w2 : o2[j];
                t2[4 + j] = h ? o2[j] : w2;
            }
        }
#pragma unroll
        for (int k = 0; k < NL; ++k) t3[k] = (k + 1 == icltop) ? albcl * cloudc : 0.0;  // icltop <= nlev only
        t3[NL - 1] = albcls * clstr;
        const double fsol = sw.fsol;
        double f1 = fsol * fband1, f2 = fsol * fband2;
        dfabs[0] = f1;
        f1 = t1[0] * (f1 - sw.ozupp * psg);
        dfabs[0] = dfabs[0] - f1;
        dfabs[1] = f1;
        f1 = t1[1] * (f1 - sw.ozone * psg);
        dfabs[1] = dfabs[1] - f1;
#pragma unroll
        for (int k = 3; k <= NL; ++k) {
            t3[k - 1] = f1 * t3[k - 1];
            f1 = f1 - t3[k - 1];
            dfabs[k - 1] = f1;
            f1 = t1[k - 1] * f1;
            dfabs[k - 1] = dfabs[k - 1] - f1;
        }
#pragma unroll
        for (int k = 2; k <= NL; ++k) {
            dfabs[k - 1] = dfabs[k - 1] + f2;
            f2 = t2[k - 1] * f2;
            dfabs[k - 1] = dfabs[k - 1] - f2;
        }
        const double fsfcd = f1 + f2;
        f1 = f1 * sw.albsfc;
#pragma unroll
        for (int k = NL; k >= 1; --k) {
            dfabs[k - 1] = dfabs[k - 1] + f1;
            f1 = t1[k - 1] * f1;
            dfabs[k - 1] = dfabs[k - 1] - f1;
            f1 = f1 + t3[k - 1];
        }
        ssrd = fsfcd;
        // longwave transmissivities of bands 2h, 2h + 1 (phy_radiat.f90:262-300): the levels
        // the cloud reaches, 3 .. nl1 (1, 2 and 8: the first stage)
        const double acl = cloudc * ablcl2;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
            for (int k = 3; k <= nl1; ++k) {
                const double deltap = psg * P->dsig[k - 1];
                const double qk = qc[k - 1];
                double e;
                if (b == 0) {  // band 0 (h = 0) or 2 (h = 1)
                    const double acloud1 = (k < icltop) ? acl : ablcl1 * cloudc;
                    const double a0 = -deltap * (ablwin + acloud1);
                    const double a2 = -deltap * fmax(ablwv1 * qk, acl);
                    e = exp(h ? a2 : a0);
                } else {  // band 1 (h = 0) or 3 (h = 1)
                    const double a1 = -deltap * ablco2;
                    const double a3 = -deltap * fmax(ablwv2 * qk, acl);
                    e = exp(h ? a3 : a1);
                }
                tq[b][k - 1] = e;
            }
            tq[b][0] = sw.tqe[b][0];
            tq[b][1] = sw.tqe[b][1];
            tq[b][NL - 1] = sw.tqe[b][2];
        }
        const double eps1 = epslw / (P->dsig[0] + P->dsig[1]);
        strat0 = sw.stratz * psg;
        strat1 = eps1 * psg;
        double rsw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) rsw[j] = own(dfabs, h, j) * rps * P->grdscp[4 * h + j];
        // the column's state for the steps until the next shortwave step
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int k = 0; k < NL; ++k) rad[kRadTau2 + ((size_t)(2 * h + b) * NL + k) * kNGP + pt] = tq[b][k];
        if (h == 0) {
            rad[kRadStratc + pt] = strat0;
            rad[kRadStratc + kNGP + pt] = strat1;
            rad[kRadSsrd + pt] = fsfcd;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            rad[kRadTtRsw + (size_t)(4 * h + j) * kNGP + pt] = rsw[j];
            mh[4 * h + j] = rsw[j];
        }
        SML_PST_T(15, 256);
        load_fbq();
    } else {  // rad's state; the A row; phys_thermo's psg, rps and clipped q
        PairPre pre;
        pre_load(pre);
        double qa[NL];
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            ta[k] = Ai[kOT + k];
            qa[k] = Ai[kOQ + k];
        }
        ph7 = Ai[kOPhi + NL - 1];
        const double ps1 = Ai[kOPs];
        load_fbq();
        psg = exp(ps1);
        rps = 1. / psg;
#pragma unroll
        for (int k = 0; k < NL; ++k) qc[k] = fmax(qa[k], 0.);
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int k = 0; k < NL; ++k) tq[b][k] = pre.tau[b][k];
        strat0 = pre.strat0;
        strat1 = pre.strat1;
        ssrd = pre.ssrd;
#pragma unroll
        for (int j = 0; j < 4; ++j) mh[4 * h + j] = pre.ttrsw[j];
        SML_PST_T(15, 256);
        pairx::blackbody(ta, P, st4a1, st4a2);
    }

    // 3.2 radlw(-1) (phy_radiat.f90:330-413): the blackbody terms on both lanes (above; a
    // shortwave step's in the first stage), bands 2h, 2h + 1's downward fluxes after each level
    double fo[2][NL];  // band 2h + b's flux after level k
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const double emis = 1. - tq[b][0];
        const double brad = fbq[b][0] * (st4a1[0] + emis * st4a2[0]);
        const double f0 = emis * brad;
        double fl = h == 0 ? f0 : 0.0;  // (bands 3, 4 start at the second level)
        fo[b][0] = fl;
#pragma unroll
        for (int k = 2; k <= NL; ++k) {
            const double tau = tq[b][k - 1];
            const double e = 1. - tau;
            const double br = fbq[b][k - 1] * (st4a1[k - 1] + e * st4a2[k - 1]);
            fl = tau * fl + e * br;
            fo[b][k - 1] = fl;
        }
    }
    // the partner's bands at this lane's levels (and at level 3, and the surface)
    double pr[2][4], pm[2], p7[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int j = 0; j < 4; ++j) pr[b][j] = swap(oth(fo[b], h, j));
        pm[b] = swap(h == 0 ? fo[b][3] : 0.0);
        p7[b] = swap(fo[b][NL - 1]);
    }
    // band jb's flux after level 4h + j (j = -1: level 4h - 1), from this lane or the partner
    auto fdn = [&](int jb, int j) -> double {
        const int b = jb & 1;
        const bool mine = (jb >> 1) == h;
        const double m = j < 0 ? (h ? fo[b][3] : 0.0) : own(fo[b], h, j);
        const double p = j < 0 ? pm[b] : pr[b][j];
        return mine ? m : p;
    };
    double fsfcd = 0.0;
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) fsfcd = fsfcd + emisfc * (((jb >> 1) == h) ? fo[jb & 1][NL - 1] : p7[jb & 1]);
    const double corlw = (epslw * emisfc) * st4a1[NL - 1];
    fsfcd = fsfcd + corlw;
    double dl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int L = 4 * h + j;
        double dg = 0.0;
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
            dg = dg + fdn(jb, j - 1);
            dg = dg - fdn(jb, j);
        }
        double d0 = 0.0;
        d0 = d0 - fo[0][0];
        d0 = d0 - fo[1][0];
        double d = L == 0 ? d0 : dg;
        const double dc = d - corlw;
        dl[j] = L == NL - 1 ? dc : d;
    }
    const double slrd = fsfcd;
    SML_PST_T(16, 256);

    // 3.3 suflux with lfluxland = .true. (phy_suflux.f90:1-355), both lanes
    double ustr3, vstr3, shf3, evap3, slru3;
    {
        constexpr int nlev = NL;
        const double esbc = emisfc * sbc, esbc4 = 4. * esbc, dlambda = clambsn - clambda;
        const double u0 = fwind0 * u7, v0 = fwind0 * v7;
        const double gtemp0 = 1. - ftemp0, rcp = 1. / cp, rdphi0 = -1. / (rd * 288. * P->sigl[nlev - 1]);
        const double phi0 = BC(kBcPhis0), fmask = BC(kBcFmask1), ssrdj = ssrd;
        double t1[2], t2[2], denvvs[3], qsat0[2];
        const double dt1 = P->wvi[nlev - 1][1] * (ta[nlev - 1] - ta[nl1 - 1]);
        t1[0] = ta[nlev - 1] + dt1;
        t1[1] = t1[0] + phi0 * dt1 * rdphi0;
        t2[1] = ta[nlev - 1] + rcp * ph7;
        t2[0] = t2[1] - rcp * phi0;
        if (ta[nlev - 1] > ta[nl1 - 1]) {
            t1[0] = ftemp0 * t1[0] + gtemp0 * t2[0];
            t1[1] = ftemp0 * t1[1] + gtemp0 * t2[1];
        } else {
            t1[0] = ta[nlev - 1];
            t1[1] = ta[nlev - 1];
        }
        const double t0 = t1[1] + fmask * (t1[0] - t1[1]);
        const double prd = p0 / rd, vg2 = vgust * vgust;
        denvvs[0] = (prd * psg / t0) * sqrt(u0 * u0 + v0 * v0 + vg2);
        const double stl = BC(kBcStl), albl = BC(kBcAlbL);
        double tskin = stl + ctday * sqrt(P->clat[jlat]) * ssrdj * (1. - albl) * psg;
        const double rdth = fstab / dtheta, astab = 0.5;
        const double dthl = (tskin > t2[0]) ? fmin(dtheta, tskin - t2[0]) : fmax(-dtheta, astab * (tskin - t2[0]));
        denvvs[1] = denvvs[0] * (1. + dthl * rdth);
        const double cdldv = cdl * denvvs[0] * BC(kBcForog);
        const double ustr1 = -cdldv * u7, vstr1 = -cdldv * v7;
        const double chlcp = chl * cp;
        double shf1 = chlcp * denvvs[1] * (tskin - t1[0]);
        const double q1l = qc[nlev - 1];  // fhum0 = 0
        qsat0[0] = qsat_at(tskin, psg, 1.);
        const double swav = BC(kBcSoilw);
        double evap1 = chl * denvvs[1] * fmax(0., swav * qsat0[0] - q1l);
        const double tsk3 = tskin * tskin * tskin;
        const double dslr = esbc4 * tsk3;
        double slru1 = esbc * tsk3 * tskin;
        double hfl1 = ssrdj * (1. - albl) + slrd - (slru1 + shf1 + alhc * evap1);
        const double clamb = clambda + BC(kBcSnowc) * dlambda;
        hfl1 = hfl1 - clamb * (tskin - stl);
        qsat0[1] = qsat_at(tskin + 1., psg, 1.);
        if (evap1 > 0)
            qsat0[1] = swav * (qsat0[1] - qsat0[0]);
        else
            qsat0[1] = 0.;
        const double dhfdt = clamb + dslr + chl * denvvs[1] * (cp + alhc * qsat0[1]);
        const double dtskin = hfl1 / dhfdt;
        tskin = tskin + dtskin;
        shf1 = shf1 + chlcp * denvvs[1] * dtskin;
        evap1 = evap1 + chl * denvvs[1] * qsat0[1] * dtskin;
        slru1 = slru1 + dslr * dtskin;
        const double tsea = BC(kBcSst);
        const double dths = (tsea > t2[1]) ? fmin(dtheta, tsea - t2[1]) : fmax(-dtheta, astab * (tsea - t2[1]));
        denvvs[2] = denvvs[0] * (1. + dths * rdth);
        const double q1s = qc[nlev - 1];
        const double cdsdv = cds * denvvs[2];
        const double ustr2 = -cdsdv * u7, vstr2 = -cdsdv * v7;
        const double chscp = chs * cp;
        const double shf2 = chscp * denvvs[2] * (tsea - t1[1]);
        const double qs = qsat_at(tsea, psg, 1.);
        const double evap2 = chs * denvvs[2] * (qs - q1s);
        const double ts2 = tsea * tsea;
        const double slru2 = esbc * (ts2 * ts2);
        ustr3 = ustr2 + fmask * (ustr1 - ustr2);
        vstr3 = vstr2 + fmask * (vstr1 - vstr2);
        shf3 = shf2 + fmask * (shf1 - shf2);
        evap3 = evap2 + fmask * (evap1 - evap2);
        slru3 = slru2 + fmask * (slru1 - slru2);
    }

    SML_PST_T(17, 256);
    // 3.4 radlw(1) (phy_radiat.f90:414-458): bands 2h, 2h + 1 upward
    const double refsfc = 1. - emisfc, fsfcu = slru3;
    double fu[2][NL], fs0[2];  // band 2h + b's flux after level k going up; its surface start
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        double fl = fsr[b] * fsfcu + refsfc * fo[b][NL - 1];
        fs0[b] = fl;
#pragma unroll
        for (int k = NL; k >= 2; --k) {
            const double tau = tq[b][k - 1];
            const double e = 1. - tau;
            const double br = fbq[b][k - 1] * (st4a1[k - 1] - e * st4a2[k - 1]);
            fl = tau * fl + e * br;
            fu[b][k - 1] = fl;
        }
        const double tau = tq[b][0];
        const double e = 1. - tau;
        const double br = fbq[b][0] * (st4a1[0] - e * st4a2[0]);
        fu[b][0] = tau * fl + e * br;  // (bands 3, 4: unused)
    }
    // the partner's bands at this lane's levels, and at the level above its top one (4h + 4:
    // level 4, or the surface start for level 7)
    double qr[2][4], qp[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int j = 0; j < 4; ++j) qr[b][j] = swap(oth(fu[b], h, j));
        qp[b] = swap(h == 1 ? fu[b][4] : fs0[b]);
    }
    // band jb's upward flux after level 4h + j (j = 4: level 4h + 4, the surface start at 8)
    auto fup = [&](int jb, int j) -> double {
        const int b = jb & 1;
        const bool mine = (jb >> 1) == h;
        const double m = j > 3 ? (h ? fs0[b] : fu[b][4]) : own(fu[b], h, j);
        const double p = j > 3 ? qp[b] : qr[b][j];
        return mine ? m : p;
    };
    const double corlw1 = P->dsig[0] * strat1 * st4a1[0] + strat0;
    const double corlw2 = P->dsig[1] * strat1 * st4a1[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int L = 4 * h + j;
        double d = dl[j];
        const double ds = d + epslw * fsfcu;
        d = L == NL - 1 ? ds : d;
        double dg = d;
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
            dg = dg + fup(jb, j + 1);
            dg = dg - fup(jb, j);
        }
        double d0 = d;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            d0 = d0 + fu[b][1];
            d0 = d0 - fu[b][0];
        }
        d = L == 0 ? d0 : dg;
        const double c1 = d - corlw1, c2 = d - corlw2;
        d = L == 0 ? c1 : L == 1 ? c2 : d;
        o.rlw[j] = d * rps * P->grdscp[L];
    }
    o.ust = ustr3;
    o.vst = vstr3;
    o.shf = shf3;
    o.evp = evap3;
    o.rps = rps;
}

#endif  // __HIPCC__
}  // namespace sml
