// sml_dyn_forcing.hpp -- the per-window forcing kernels: ini_sea's hybrid SST block
// (k_hybrid_sst) and agcm_init's fordate (FordateArgs, k_fordate).  Both switch FMA
// contraction off in their bodies: the unit compiles with -ffp-contract=on.
// (A timeline build, SML_TL, needs the unit's SML_TL_DEFINE ahead of this header.)
#pragma once
#include <hip/hip_runtime.h>

#include "sml_dyn_layout.hpp"
#include "sml_dynamics_tables.hpp"
#include "sml_physics.hpp"
#include "sml_timeline.hpp"

namespace {
using namespace sml;

// ini_sea's hybrid block (cpl_sea.f90:38-46) per grid point: where the coupler's
// (ice-blended) sst_am is less than 6 K above the hybrid SST take the hybrid SST, add
// the bias, blend with the sea ice as sea2atm does (cpl_sea.f90:197)
__global__ void k_hybrid_sst(const double *__restrict__ cpl, const double *__restrict__ hyb,
                             const double *__restrict__ sice, const double *__restrict__ tice, double bias,
                             double *__restrict__ sst_am) {
#pragma clang fp contract(off)  // the reference's separate multiply and add (this file contracts by default)
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= kNGP) return;
    double s = cpl[p];
    if (hyb) {
        const double diff = s - hyb[p];
        if (diff < 6.0) s = hyb[p];
        s = s + bias;
        const double d = tice[p] - s;
        s = s + sice[p] * d;
    }
    sst_am[p] = s;
}

// ------------------------------------------------------ per-window forcing (fordate)
// run_model hands SPEEDY the calendar date of every window (mpires.f90:1545, :1595-1598)
// and agcm_init rebuilds the date's forcing before stepone (ini_agcm_init.f90:57-89):
// newdate(0), ini_coupler(2) and fordate(0); agcm_1day runs fordate(1) again before the
// leapfrog loop (at_gcm.f90:84) with the same inputs (lco2 is .false., mod_lflags.f90:
// 16, so imode 1 changes nothing).  With the coupler flags of the reference
// (icland = 1, icsea = 0, icice = 1, isstan = 0; mod_cpl_flags.f90) and jday = 0:
//   land (cpl_land.f90:1-95)  stl_am = forin5(stl12), snowd_am = forint(snowd12),
//                             soilw_am = forint(soilw12)
//   sea  (cpl_sea.f90:1-200)  sst = forin5(sst12), sice = forint(sice12) adjusted over
//                             sea ice (:96-117, tice), sst_am = sst + sice (tice - sst),
//                             then ini_sea's hybrid block (:38-46, k_hybrid_sst)
//   fordate (ini_fordate.f90:50-113)  sol_oz(tyear), the surface albedo, tcorh =
//                             spec(gamlat phis0), qcorh = spec(refrh1 (qref - qsfc))
//                             from the current stl_am / sst_am
// One thread per grid point; then spec of the two correction fields.

struct FordateArgs {
    double sol[5][kIL];  // sol_oz per latitude row: fsol, ozone, ozupp, zenit, stratz
    int m5[5];
    double w5[5];
    int mi[2];
    double wmon;
    int clim, hyb;
    double bias;
};

__global__ __launch_bounds__(256) void k_fordate(FordateArgs a, const double *__restrict__ surf,
                                                 const double *__restrict__ clim, const double *__restrict__ hyb,
                                                 double *__restrict__ pbc, double *__restrict__ sst_cpl,
                                                 double *__restrict__ sice_am, double *__restrict__ tice_am,
                                                 double *__restrict__ corh) {
#pragma clang fp contract(off)  // the reference's separate multiplies and adds
    SML_TL_SCOPE(sml::tl::kFordate);
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= kNGP) return;
    const int j = p / kIX;
    const double fmask_l = surf[p], fmask_s = surf[kNGP + p], alb0 = surf[2 * kNGP + p];
    double snowc, sice, cpl;
    if (a.clim) {
        auto field = [&](int f, int m) { return clim[((size_t)f * 12 + m) * kNGP + p]; };
        auto forin5 = [&](int f) {
            return a.w5[0] * field(f, a.m5[0]) + a.w5[1] * field(f, a.m5[1]) + a.w5[2] * field(f, a.m5[2]) +
                   a.w5[3] * field(f, a.m5[3]) + a.w5[4] * field(f, a.m5[4]);
        };
        auto forint = [&](int f) {
            const double f0 = field(f, a.mi[0]);
            return f0 + a.wmon * (field(f, a.mi[1]) - f0);
        };
        // land: atm2land(0), stl_lm = stlcl_ob (ini_land, istart 2), land2atm(0)
        const double stl = forin5(0), snowd = forint(1), soilw = forint(2);
        pbc[(size_t)kBcStl * kNGP + p] = stl;
        pbc[(size_t)kBcSoilw * kNGP + p] = soilw;
        snowc = fmin(1., snowd / 60.0);  // fordate: min(1, snowd_am / sd2sc), mod_surfcon sd2sc
        // sea: atm2sea(0) with the sea-ice adjustment of the climatology
        double sst = forin5(3), sic = forint(4), tic;
        const double sstfr = 273.2 - 1.8;
        if (sst > sstfr) {
            sic = fmin(0.5, sic);
            tic = sstfr;
            if (sic > 0.) sst = sstfr + (sst - sstfr) / (1. - sic);
        } else {
            sic = fmax(0.5, sic);
            tic = sstfr + (sst - sstfr) / sic;
            sst = sstfr;
        }
        // ini_sea: the ocean / ice model starts from the climatology; sea2atm(0):
        // icsea 0 -> sst_am = sstcl_ob (+ no anomaly), icice 1 -> the model's ice
        sst = sst + 0.0;
        sst = sst + sic * (tic - sst);
        sice_am[p] = sic;
        tice_am[p] = tic;
        sst_cpl[p] = sst;
        sice = sic;
        cpl = sst;
    } else {
        snowc = pbc[(size_t)kBcSnowc * kNGP + p];
        sice = sice_am[p];
        cpl = sst_cpl[p];
    }
    double sst_am = cpl;
    if (a.hyb) {  // ini_sea's hybrid block, as k_hybrid_sst
        const double h = hyb[p];
        const double diff = sst_am - h;
        if (diff < 6.0) sst_am = h;
        sst_am = sst_am + a.bias;
        sst_am = sst_am + sice * (tice_am[p] - sst_am);
    }
    pbc[(size_t)kBcSst * kNGP + p] = sst_am;
    // fordate 2: daily-mean radiative forcing and the surface albedo
    pbc[(size_t)kBcFsol * kNGP + p] = a.sol[0][j];
    pbc[(size_t)kBcOzone * kNGP + p] = a.sol[1][j];
    pbc[(size_t)kBcOzupp * kNGP + p] = a.sol[2][j];
    pbc[(size_t)kBcZenit * kNGP + p] = a.sol[3][j];
    pbc[(size_t)kBcStratz * kNGP + p] = a.sol[4][j];
    const double albsn = 0.60, albsea = 0.07, albice = 0.60;  // mod_radcon.f90:59-61
    const double alb_l = alb0 + snowc * (albsn - alb0);
    const double alb_s = albsea + sice * (albice - albsea);
    pbc[(size_t)kBcSnowc * kNGP + p] = snowc;
    pbc[(size_t)kBcAlbL * kNGP + p] = alb_l;
    pbc[(size_t)kBcAlbS * kNGP + p] = alb_s;
    pbc[(size_t)kBcAlbsfc * kNGP + p] = alb_s + fmask_l * (alb_l - alb_s);
    // fordate 3-4: the horizontal-diffusion corrections (setgam: gamlat = gamma / (1000 g))
    const double gamlat = 6.0 / (1000. * 9.81), rd = 287., refrh1 = 0.7;
    const double c = gamlat * pbc[(size_t)kBcPhis0 * kNGP + p];
    const double pexp = 1. / (rd * gamlat);
    const double tsfc = fmask_l * pbc[(size_t)kBcStl * kNGP + p] + fmask_s * sst_am;
    const double tref = tsfc + c;
    const double psfc = pow(tsfc / tref, pexp);
    // shtorh(0, .., tref, 1, -1, ..) and shtorh(0, .., tsfc, psfc, 1, ..) (phy_shtorh.f90:27-51)
    auto qsat = [](double ta, double ps) {
        const double e0 = 6.108e-3, c1 = 17.269, c2 = 21.875, t0 = 273.16, t1 = 35.86, t2 = 7.66;
        const double q = (ta >= t0) ? e0 * exp(c1 * (ta - t0) / (ta - t1)) : e0 * exp(c2 * (ta - t0) / (ta - t2));
        return 622. * q / (ps - 0.378 * q);
    };
    const double qref = qsat(tref, 1.0), qsfc = qsat(tsfc, 1. * psfc);
    corh[p] = c;
    corh[kGF + p] = refrh1 * (qref - qsfc);
}

}  // namespace
