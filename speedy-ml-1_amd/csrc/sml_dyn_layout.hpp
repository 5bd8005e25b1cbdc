// sml_dyn_layout.hpp -- the dynamics unit's buffer layouts: field counts and offsets
// of the state, tendency and transform buffers, the coefficient indices, and the fused
// step's m-major layouts and stamp sizes.  Shared by every kernel header of the unit
// and by the host code of sml_dynamics.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "sml_dynamics_tables.hpp"

namespace {
using namespace sml;

constexpr int kSF = kMX2 * kNX;       // 1984 doubles per spectral field
constexpr int kGF = kIX * kIL;        // 4608 doubles per grid field
constexpr int kVF = kMX2 * kIL;       // 2976 doubles per Fourier field
constexpr int kNInv = 6 * kKX + 2;    // 50 inverse transforms per step (dynamics)
constexpr int kNInv1 = 4 * kKX;       // the first 32 are kcos = 1
// with the physics on the GPU: kcos = 1 fields [vor div t tr (j2) | t1 q1 phi1 (8 each) | ps1]
// then kcos = 2 fields [ucos vcos (j2) | psdx psdy | ucos1 vcos1]
constexpr int kNInv1P = kNInv1 + 3 * kKX + 1;  // 57
constexpr int kNInvP = kNInv1P + 4 * kKX + 2;  // 91 (= the reference's 91 grid calls per step)
constexpr int kPT1 = kNInv1, kPQ1 = kNInv1 + kKX, kPPhi1 = kNInv1 + 2 * kKX, kPPs1 = kNInv1 + 3 * kKX;
constexpr int kNInvMax = kNInvP;
constexpr int kNFwdScaled = 6 * kKX;  // 48 vdspec inputs (x 1/cos lat)
constexpr int kNFwd = 9 * kKX + 1;    // 73 forward transforms per step
constexpr int kMN = kMX * kNX;        // 992 complex coefficients
constexpr int kNstrad = 3;            // shortwave radiation every 3rd step (mod_tsteps.f90:65)

// state buffer: vor(mx,nx,kx,2) | div | t | tr(ntr=1) | ps(mx,nx,2) (reference layouts)
constexpr size_t kOffVor = 0, kOffDiv = 2 * kKX * kSF, kOffT = 4 * kKX * kSF, kOffTr = 6 * kKX * kSF,
                 kOffPs = 8 * kKX * kSF, kStateSize = 8 * kKX * kSF + 2 * kSF;
// tendency buffer: vordt | divdt | tdt | trdt (kx fields each) | psdt
constexpr size_t kTVor = 0, kTDiv = kKX * kSF, kTT = 2 * kKX * kSF, kTTr = 3 * kKX * kSF, kTPs = 4 * kKX * kSF,
                 kTendSize = 4 * kKX * kSF + kSF;

__device__ inline int ci(int p, int m, int n) { return p + 2 * (m + kMX * n); }
__device__ inline int mi(int m, int n) { return m + kMX * n; }

constexpr int kCW = 2 * kNX;                  // real coefficients (n, p) of one m
// The per-m kernels run one thread per (coefficient cc, level k), k = threadIdx.x / kCW.
// kCW is the wavefront size, so a wave holds one level and k is the wave's index: read
// through readfirstlane it is a scalar to the compiler, and everything that depends on
// the level alone (edge levels, the level sums' bounds, table and state rows) is decided
// once per wave on the scalar unit instead of per lane with compares and selects.
static_assert(kCW == 64, "one level per 64-lane wave: wave_index() is the level index of the per-m kernels");
__device__ inline int wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
// iogrid's field-major work layout, both directions: [u 8 | v 8 | t 8 | q 8 | ps]
constexpr int kNIo = 4 * kKX + 1;
constexpr int kNIoWind = 2 * kKX;
constexpr int kSM = 5 * 2 * kKX * kCW;        // m-major state slice: [var 5][lev 2][k][cc] (ps at k = 0)
// m-major Fourier coefficients, [m][lat][f][p]: a latitude row's fields are contiguous
// per m (the row kernels' 16-B stores / loads coalesce across the fields' lanes) and
// each m's slice is contiguous (the spectral kernels stage it with coalesced loads)
constexpr int kVLs = 2 * kNFwd;               // forward: latitude stride
constexpr int kVFm = kIL * kVLs;              // forward: per-m slice
constexpr int kVIl = 2 * kNInvMax;            // inverse: latitude stride
constexpr int kVIm = kIL * kVIl;              // inverse: per-m slice
__device__ inline int smi(int var, int lev, int k, int cc) { return ((var * 2 + lev - 1) * kKX + k) * kCW + cc; }

// diagnostic phase stamps (SML_DYN_STAMPS=1 at creation): thread 0 of each block
// writes wall_clock64() (100 MHz) at phase boundaries, [kernel][block][8]
constexpr int kStampKernels = 4, kStampBlocks = 96, kStamps = 8;  // kernels: grid/rows, spec, specx, last spec
__device__ inline void stamp(long long *dbg, int kern, int i) {
    if (dbg && threadIdx.x == 0) dbg[((size_t)kern * kStampBlocks + blockIdx.x) * kStamps + i] = wall_clock64();
}

}  // namespace
