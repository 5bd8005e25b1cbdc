// sml_dyn_gridpoint.hpp -- the grid-point dynamics of one grid column (grtend's
// products between the inverse and the forward transforms).  Device functions only,
// shared by k_dyn_gridpoint and the fused row kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "sml_dyn_layout.hpp"
#include "sml_dynamics_tables.hpp"

namespace {
using namespace sml;

// the grid-point dynamics' per-level constants and the Coriolis row (the DynTables
// fields gridpoint_column reads), for an LDS copy in the row kernel
struct GpTab {
    double dhs[kKX], dhsr[kKX], fsgr[kKX], tref[kKX], tref3[kKX], coriol[kIL];
};

// grid-point dynamics of one column (grtend :60-217 and the products of :233-275).
// g(f) = inverse-transformed field f at the column (layout of k_dyn_prep, kcos = 2
// group at o2); hasP: add phypar's tendencies pu/pv/pt/pq [kx] where phypar adds
// them (:225); put(f, v) receives the 73 forward-transform inputs
//   [utend 8 | -u*tgg 8 | -u*trg 8 | vtend 8 | -v*tgg 8 | -v*trg 8]  (x 1/cos in specx)
//   [0.5(u^2+v^2) 8 | ttend 8 | trtend 8 | -umean*px - vmean*py]
template <class GetF, class PutF, class TT>
__device__ inline void gridpoint_products(int o2, GetF g, PutF put, const TT *T);

// products = false: the products of :239-271 are left to gridpoint_products (the row
// kernel runs them on the lane that has slack)
template <class GetF, class PutF, class TT>
__device__ inline void gridpoint_column(int j, int o2, GetF g, bool hasP, const double *pu, const double *pv,
                                        const double *pt, const double *pq, PutF put, const TT *T,
                                        bool products = true) {
    double ug[kKX], vg[kKX], vorg[kKX], divg[kKX], tg[kKX], trg[kKX];
#pragma unroll
    for (int k = 0; k < kKX; ++k) {
        vorg[k] = g(k) + T->coriol[j];
        divg[k] = g(kKX + k);
        tg[k] = g(2 * kKX + k);
        trg[k] = g(3 * kKX + k);
        ug[k] = g(o2 + k);
        vg[k] = g(o2 + kKX + k);
    }
    double px = g(o2 + 2 * kKX), py = g(o2 + 2 * kKX + 1);
    double umean = 0.0, vmean = 0.0, dmean = 0.0;
#pragma unroll
    for (int k = 0; k < kKX; ++k) {
        umean = umean + ug[k] * T->dhs[k];
        vmean = vmean + vg[k] * T->dhs[k];
        dmean = dmean + divg[k] * T->dhs[k];
    }
    put(kNFwd - 1, -umean * px - vmean * py);  // psdt source (:95-97)
    double puv[kKX], sigdt[kKXP], sigm[kKXP], tgg[kKX], temp[kKXP];
#pragma unroll
    for (int k = 0; k < kKX; ++k) puv[k] = (ug[k] - umean) * px + (vg[k] - vmean) * py;
    sigdt[0] = 0.0;
    sigm[0] = 0.0;
#pragma unroll
    for (int k = 0; k < kKX; ++k) {
        sigdt[k + 1] = sigdt[k] - T->dhs[k] * (puv[k] + divg[k] - dmean);
        sigm[k + 1] = sigm[k] - T->dhs[k] * puv[k];
    }
#pragma unroll
    for (int k = 0; k < kKX; ++k) tgg[k] = tg[k] - T->tref[k];
    px = kRgas * px;
    py = kRgas * py;
    // zonal wind tendency
    temp[0] = 0.0;
    temp[kKX] = 0.0;
#pragma unroll
    for (int k = 1; k < kKX; ++k) temp[k] = sigdt[k] * (ug[k] - ug[k - 1]);
#pragma unroll
    for (int k = 0; k < kKX; ++k) {
        double u = vg[k] * vorg[k] - tgg[k] * px - (temp[k + 1] + temp[k]) * T->dhsr[k];
        if (hasP) u = u + pu[k];
        put(k, u);
    }
    // meridional wind tendency
#pragma unroll
    for (int k = 1; k < kKX; ++k) temp[k] = sigdt[k] * (vg[k] - vg[k - 1]);
#pragma unroll
    for (int k = 0; k < kKX; ++k) {
        double v = -ug[k] * vorg[k] - tgg[k] * py - (temp[k + 1] + temp[k]) * T->dhsr[k];
        if (hasP) v = v + pv[k];
        put(3 * kKX + k, v);
    }
    // temperature tendency
#pragma unroll
    for (int k = 1; k < kKX; ++k)
        temp[k] = sigdt[k] * (tgg[k] - tgg[k - 1]) + sigm[k] * (T->tref[k] - T->tref[k - 1]);
#pragma unroll
    for (int k = 0; k < kKX; ++k) {
        double tt = tgg[k] * divg[k] - (temp[k + 1] + temp[k]) * T->dhsr[k] +
                    T->fsgr[k] * tgg[k] * (sigdt[k + 1] + sigdt[k]) + T->tref3[k] * (sigm[k + 1] + sigm[k]) +
                    kAkap * (tg[k] * puv[k] - tgg[k] * dmean);
        if (hasP) tt = tt + pt[k];
        put(7 * kKX + k, tt);
    }
    // tracer tendency: no vertical advection between the top three layers (:179-188)
#pragma unroll
    for (int k = 1; k < kKX; ++k) temp[k] = sigdt[k] * (trg[k] - trg[k - 1]);
    temp[1] = 0.0;
    temp[2] = 0.0;
#pragma unroll
    for (int k = 0; k < kKX; ++k) {
        double q = trg[k] * divg[k] - (temp[k + 1] + temp[k]) * T->dhsr[k];
        if (hasP) q = q + pq[k];
        put(8 * kKX + k, q);
    }
    // products for the spectral conversion (:239-271)
    if (products) gridpoint_products(o2, g, put, T);
}

template <class GetF, class PutF, class TT>
__device__ inline void gridpoint_products(int o2, GetF g, PutF put, const TT *T) {
#pragma unroll
    for (int k = 0; k < kKX; ++k) {
        const double ug = g(o2 + k), vg = g(o2 + kKX + k), trg = g(3 * kKX + k);
        const double tgg = g(2 * kKX + k) - T->tref[k];
        put(kKX + k, -ug * tgg);
        put(4 * kKX + k, -vg * tgg);
        put(2 * kKX + k, -ug * trg);
        put(5 * kKX + k, -vg * trg);
        put(6 * kKX + k, 0.5 * (ug * ug + vg * vg));
    }
}

}  // namespace
