// sml_dyn_unfused.hpp -- the kernels of the unfused step (7 launches, 8 with GPU
// physics, around the spectral unit's batched transforms): k_dyn_prep,
// k_dyn_gridpoint, k_phys, k_dyn_combine, k_dyn_tail.
#pragma once
#include <hip/hip_runtime.h>

#include "sml_dyn_gridpoint.hpp"
#include "sml_dyn_layout.hpp"
#include "sml_dyn_spec_math.hpp"
#include "sml_dynamics_tables.hpp"
#include "sml_physics.hpp"

namespace {
using namespace sml;

// ---------------------------------------------------------------- kernels
// prep: inputs of the inverse transforms from time level j2 (grtend :60-99),
// [vor 8 | div 8 | t 8 | tr 8] then at o2 [ucos 8 | vcos 8 | psdx | psdy]; with
// phys, also the level-1 inputs of phypar (phy_phypar.f90:54-66): t1, q1, geop(1),
// ps1 at kPT1.. and ucos1, vcos1 at o2 + 18.  One thread per (m, n).
__global__ void k_dyn_prep(const double *__restrict__ st, double *__restrict__ sin_, const DynTables *__restrict__ T,
                           const double *__restrict__ phis, int j2, int o2, int phys) {
    const int mn = blockIdx.x * blockDim.x + threadIdx.x;
    if (mn >= kMN) return;
    const int k = blockIdx.y;
    const int m = mn % kMX, n = mn / kMX;
    const size_t lev = (size_t)(j2 - 1) * kKX;
    if (k < kKX) {
        const double *vor = st + kOffVor + (lev + k) * kSF, *div = st + kOffDiv + (lev + k) * kSF;
        const double *t = st + kOffT + (lev + k) * kSF, *tr = st + kOffTr + (lev + k) * kSF;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int c = ci(p, m, n);
            sin_[(size_t)k * kSF + c] = vor[c];
            sin_[(size_t)(kKX + k) * kSF + c] = div[c];
            sin_[(size_t)(2 * kKX + k) * kSF + c] = t[c];
            sin_[(size_t)(3 * kKX + k) * kSF + c] = tr[c];
        }
        uvspec_at(vor, div, T, m, n, sin_ + (size_t)(o2 + k) * kSF, sin_ + (size_t)(o2 + kKX + k) * kSF);
        if (phys) {
            const double *vor1 = st + kOffVor + (size_t)k * kSF, *div1 = st + kOffDiv + (size_t)k * kSF;
            const double *t1 = st + kOffT, *tr1 = st + kOffTr + (size_t)k * kSF;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int c = ci(p, m, n);
                sin_[(size_t)(kPT1 + k) * kSF + c] = t1[(size_t)k * kSF + c];
                sin_[(size_t)(kPQ1 + k) * kSF + c] = tr1[c];
                sin_[(size_t)(kPPhi1 + k) * kSF + c] = geop_at(t1, phis, T, c, m, k);
            }
            uvspec_at(vor1, div1, T, m, n, sin_ + (size_t)(o2 + 2 * kKX + 2 + k) * kSF,
                      sin_ + (size_t)(o2 + 3 * kKX + 2 + k) * kSF);
        }
    } else {
        if (phys) {
#pragma unroll
            for (int p = 0; p < 2; ++p) sin_[(size_t)kPPs1 * kSF + ci(p, m, n)] = st[kOffPs + ci(p, m, n)];
        }
        // grad(ps(j2)) -> (psdx, psdy)  (spe_spectral.f90:271-305)
        const double *ps = st + kOffPs + (size_t)(j2 - 1) * kSF;
        double *dx = sin_ + (size_t)(o2 + 2 * kKX) * kSF, *dy = sin_ + (size_t)(o2 + 2 * kKX + 1) * kSF;
        dx[ci(1, m, n)] = T->gradx[m] * ps[ci(0, m, n)];
        dx[ci(0, m, n)] = -T->gradx[m] * ps[ci(1, m, n)];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            double v;
            if (n == 0)
                v = T->gradyp[0][m] * ps[ci(p, m, 1)];
            else if (n == kNX - 1)
                v = -T->gradym[n][m] * ps[ci(p, m, kNTRUN1 - 1)];
            else
                v = -T->gradym[n][m] * ps[ci(p, m, n - 1)] + T->gradyp[n][m] * ps[ci(p, m, n + 1)];
            dy[ci(p, m, n)] = v;
        }
    }
}

// grid-point dynamics, one thread per grid column; G = the inverse-transformed
// fields, P = optional physics tendencies [u 8 | v 8 | t 8 | q 8] in grid space,
// F = the 73 forward-transform inputs (gridpoint_column)
__global__ __launch_bounds__(256) void k_dyn_gridpoint(const double *__restrict__ G, const double *__restrict__ P,
                                                       double *__restrict__ F, const DynTables *__restrict__ T,
                                                       int o2) {
    const int pt = blockIdx.x * blockDim.x + threadIdx.x;
    if (pt >= kGF) return;
    double pu[kKX], pv[kKX], ptt[kKX], pq[kKX];
    if (P) {
#pragma unroll
        for (int k = 0; k < kKX; ++k) {
            pu[k] = P[(size_t)k * kGF + pt];
            pv[k] = P[(size_t)(kKX + k) * kGF + pt];
            ptt[k] = P[(size_t)(2 * kKX + k) * kGF + pt];
            pq[k] = P[(size_t)(3 * kKX + k) * kGF + pt];
        }
    }
    gridpoint_column(
        pt / kIX, o2, [&](int f) { return G[(size_t)f * kGF + pt]; }, P != nullptr, pu, pv, ptt, pq,
        [&](int f, double v) { F[(size_t)f * kGF + pt] = v; }, T);
}

// phypar's physics, one thread per grid column (sml_physics.hpp): level fields
// [kx][ngp] in, tendencies P = [u 8 | v 8 | t 8 | q 8] x ngp out
__global__ __launch_bounds__(64) void k_phys(const double *__restrict__ ug1, const double *__restrict__ vg1,
                                             const double *__restrict__ tg1, const double *__restrict__ qg1,
                                             const double *__restrict__ phig1, const double *__restrict__ pslg1,
                                             const double *__restrict__ bc, double *__restrict__ rad,
                                             const PhysTables *__restrict__ PT, int lradsw, double *__restrict__ P) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= kNGP) return;
    double ua[kKX], va[kKX], ta[kKX], qa[kKX], phi[kKX], ut[kKX], vt[kKX], tt[kKX], qt[kKX];
#pragma unroll
    for (int k = 0; k < kKX; ++k) {
        ua[k] = ug1[(size_t)k * kNGP + j];
        va[k] = vg1[(size_t)k * kNGP + j];
        ta[k] = tg1[(size_t)k * kNGP + j];
        qa[k] = qg1[(size_t)k * kNGP + j];
        phi[k] = phig1[(size_t)k * kNGP + j];
    }
    phys_column(j, ua, va, ta, qa, phi, pslg1[j], bc, rad, PT, &PT->fband[0][0], lradsw != 0, ut, vt, tt, qt);
#pragma unroll
    for (int k = 0; k < kKX; ++k) {
        P[(size_t)k * kNGP + j] = ut[k];
        P[(size_t)(kKX + k) * kNGP + j] = vt[k];
        P[(size_t)(2 * kKX + k) * kNGP + j] = tt[k];
        P[(size_t)(3 * kKX + k) * kNGP + j] = qt[k];
    }
}

// combine: spectral tendencies of grtend (:229-278) from the 73 forward transforms
__global__ void k_dyn_combine(const double *__restrict__ S, double *__restrict__ Td, const DynTables *__restrict__ T) {
    const int mn = blockIdx.x * blockDim.x + threadIdx.x;
    if (mn >= kMN) return;
    const int k = blockIdx.y;
    const int m = mn % kMX, n = mn / kMX;
    auto fld = [&](int f) { return S + (size_t)f * kSF; };
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int c = ci(p, m, n);
        double vo, dv, d0, dq, dummy;
        vds_at(fld(k), fld(3 * kKX + k), T, m, n, p, &vo, &dv);              // vdspec(utend, vtend)
        const double lapv = -(fld(6 * kKX + k)[c] * T->el2[n][m]);          // lap(spec(0.5(u2+v2)))
        Td[kTVor + (size_t)k * kSF + c] = vo;
        Td[kTDiv + (size_t)k * kSF + c] = dv - lapv;
        vds_at(fld(kKX + k), fld(4 * kKX + k), T, m, n, p, &dummy, &d0);     // vdspec(-u tgg, -v tgg)
        Td[kTT + (size_t)k * kSF + c] = d0 + fld(7 * kKX + k)[c];
        vds_at(fld(2 * kKX + k), fld(5 * kKX + k), T, m, n, p, &dummy, &dq); // vdspec(-u trg, -v trg)
        Td[kTTr + (size_t)k * kSF + c] = dq + fld(8 * kKX + k)[c];
        if (k == 0) Td[kTPs + c] = (m == 0 && n == 0) ? 0.0 : fld(kNFwd - 1)[c];  // psdt(1,1) = 0
    }
}

// tail kernel of the unfused step: a block owns 32 real coefficients x 8 levels
constexpr int kTailC = 32;
__global__ __launch_bounds__(256) void k_dyn_tail(double *__restrict__ st, double *__restrict__ Td,
                                                  double *__restrict__ phi_out, const double *__restrict__ phis,
                                                  const double *__restrict__ tcorh, const double *__restrict__ qcorh,
                                                  const DynTables *__restrict__ T, int j1, int j4, double dt,
                                                  double alph, double rob, double wil) {
    __shared__ double sh[3][kKX][kTailC];
    const int cc = threadIdx.x & (kTailC - 1), k = threadIdx.x / kTailC;
    const int c = blockIdx.x * kTailC + cc;  // 0 .. 1983 = 2 * (m + mx n) + p
    const int mn = c >> 1, m = mn % kMX, n = mn / kMX;
    auto S = [&](int var, int lev, int kk) -> double & {  // reference layout; ps has one level
        if (var == 4) return st[kOffPs + (size_t)(lev - 1) * kSF + c];
        const size_t off = var == 0 ? kOffVor : var == 1 ? kOffDiv : var == 2 ? kOffT : kOffTr;
        return st[off + ((size_t)(lev - 1) * kKX + kk) * kSF + c];
    };
    // (a wave spans two levels at kTailC = 32: k is per lane, the branch-free form)
    tail_coef<kTailC, false>(S, Td, phi_out, phis, tcorh, qcorh, c, GTab{T, m}, sh, cc, k, c, m, n,
                             Td[kTVor + (size_t)k * kSF + c], Td[kTDiv + (size_t)k * kSF + c],
                             Td[kTT + (size_t)k * kSF + c], Td[kTTr + (size_t)k * kSF + c], Td[kTPs + c], j1, j4, dt,
                             alph, rob, wil);
}

}  // namespace
