// sml_reservoir_layout.hpp -- the reservoir context's weight layout and index tables:
// what sml_reservoir.hip uploads, computed on the host with no HIP call in between, so
// the index arithmetic runs (and is sanitised) on a CPU: tests/reservoir_layout_check.cpp,
// tests/series_layout_check.cpp.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "sml_internal.hpp"

namespace sml {

constexpr int kLdAlign = 32;    // W_out / x_aug row stride multiple (columns)
constexpr int kRows = 8;        // W_out rows per wave in the readout (nout_pad's multiple)
constexpr int kMeanStd = 36;    // mean/std vector length (mod_reservoir.f90:1815-1846)
constexpr int kTisrStride = 16; // packed tisr input: [nlocal][16]
constexpr int kSrcKeep = -1;    // feedback entry left untouched (sst)

constexpr int kEllA = 8;  // ELL slots reserved per row for A (makesparse rows hold floor(k/n) or +1 <= 8)
constexpr int kEllW = 1;  // ELL slots per row for W_in (the trained W_in has one entry per row)

// A's ELL copy (r04b): a_w "main" slots per row, stored as slot pairs, pair-major
// ([pair][n] of (col, col) u16 pairs and of (val, val) pairs: lane i's row is one
// 4-B + one 8-B load per pair, coalesced across the wave), a_w chosen per region to
// move the fewest bytes.  makesparse rows hold floor(k/n) or floor(k/n) + 1 entries
// (mod_linalg.f90:180-218): with a_ov the rows holding a_w + 1 keep their last entry
// in an overflow list instead of padding every row to the longest -- a bit per row
// (u64 words) + a count per word locate it.  The dominant 4x4+sst region (n 6048,
// 4.8 % of rows one longer) moves 36.5 B of A per row instead of 48.
struct RegionDev {
    int n, ninp, ld;
    int a_w, w_w;  // A's ELL main width in slots (0 = use the CSR copy); W_in ELL (1) or CSR (0)
    int a_ov;      // 1: rows of a_w + 1 entries, the last in the overflow list
    int w_q;       // > 0: W_in's column of row i is i / w_q = umulhi(i, w_magic), not stored
    uint32_t w_magic;
    int64_t a_rp, a_nz, w_rp, w_nz, wout, x, xaug, fb;
    int64_t wlm;  // W_out(:, 1:ncs) transposed, [ncs][nout_pad], in the W_out pool after the row-major blocks
    int64_t a_ell, w_ell;  // offsets into the ELL pools (A: pair-major as above; W_in: [n])
    int64_t a_om;          // overflow bit words / per-word counts: [ceil(n / 64)] each
    int64_t a_oe;          // overflow entries (col, val) in row order: [n] reserved
};

// ELL slots per row reserved for region (n, k): makesparse rows hold floor(k/n) or
// floor(k/n)+1 entries (per-block permutations); none in a CSR-only context
inline int ell_cap_a(int n, int k, bool csr_only) { return !csr_only && k / n + 1 <= kEllA ? kEllA : 0; }
inline int ell_cap_w(bool csr_only) { return csr_only ? 0 : kEllW; }

// W_in's implicit block-diagonal column: i / q == umulhi(i, win_magic(q)) for the rows i
// pack_region verifies (every i < n <= 65535)
inline uint32_t win_magic(int q) { return (uint32_t)((0x100000000ull + q - 1) / q); }

// ------------------------------------------------------------------ pool planning
struct PoolPlanIn {
    int nlocal;
    const int *n, *k, *ninp;
    int ncs, nout_pad;
    bool csr_only;
};

// every region's offsets into the context's pools (elements of the pool's type), and the
// pools' sizes
struct PoolPlan {
    std::vector<RegionDev> rd;
    std::vector<int> ld;
    std::vector<int> a_ell_cap, w_ell_cap;  // ELL slots per row reserved per region
    int64_t tot_a_rp = 0, tot_a_nz = 0, tot_w_rp = 0, tot_w_nz = 0, tot_wout = 0, tot_xaug = 0, tot_fb = 0;
    int64_t tot_wlm = 0;  // elements of the transposed local-model blocks (pool d_wlm)
    int64_t tot_a_ell = 0, tot_w_ell = 0, tot_a_om = 0, tot_a_oe = 0;
    int maxn = 0, maxninp = 0;
};

PoolPlan plan_pools(const PoolPlanIn &in);

// ------------------------------------------------------------------ the launch shape
// constants the kernels (sml_res_*.hpp) and the shape below share
constexpr int kUpdThreads = 1024;  // threads per update block (one row per thread per pass)
constexpr int kStageX = 7;         // the balanced update stages kStageX * kUpdThreads state entries per segment
constexpr int kRowsWide = 17;   // rows per wave when nout_pad = 17 w (w <= 8 waves)
constexpr int kWideWaves = 2;   // waves per readout block with kRowsWide rows (a region = w / 2 blocks;
                                // 2 / 4 / 8 waves measured: one-pass 0.638 / 0.644 / 0.696 ms)
constexpr int kBeginThreads = 512;  // threads per fused-begin block: a wave per wide readout item
constexpr int kWideMax = 8;         // the wide readout's bound on w, one region's items in one begin block
static_assert(kWideMax == kBeginThreads / 64, "the fused begin runs a wave per wide readout item");
constexpr int kMaxNcs = 256;     // local-model length bound of the fused finish (132 in T30L8)
constexpr int kFinGroups = 7;
constexpr int kFinGsz = 19;  // the grouped finish's column-group bound (ncs 132: 6 x 19 + 18)
constexpr int kFinOutMax = 144;  // the grouped finish's outputs (its LDS rows), taken in quads by 256 threads
constexpr size_t kRegionLdsMax = 64 * 1024;  // a per-region block's LDS staging: two blocks per CU

struct StepShapeIn {
    int maxn, maxninp, nout_pad, ncs, nlocal;
    size_t max_lds;  // the device's LDS per workgroup
    bool ell_ok;     // every local region's A and W_in in ELL form
    int begin_mode;  // sml_res_set_begin_mode
    bool per_region, finish_ungrouped, stepwise_drive;  // sml_res_set_reference_paths
};

// Which kernel form each stage of a step takes and with what LDS: all of it host
// arithmetic on the context's sizes and switches, worked out when one of them changes
// (create, a region's load, the setters) and read by the launchers and by the ABI's
// reports (sml_res_update_balanced, sml_res_begin_fused).
struct StepShape {
    int lds_x = 0;          // the update's LDS row count: maxn rounded up to even
    int lds_buf = 0;        // doubles of one staging buffer: lds_x of x, then maxninp of u
    size_t lds_region = 0;  // k_res_update / k_res_begin: x and u of the largest region
    size_t lds_bal = 0;     // k_res_update_bal: two such buffers
    size_t lds_drive = 0;   // k_res_drive: two states and two inputs
    bool region_lds = false;  // the per-region update stages in LDS (else gathers from global memory)
    int parts = 1;            // blocks per region of the per-region update
    bool wide = false;        // the readout kRowsWide rows a wave (nout_pad = 17 w, w <= kWideMax)
    int rows = kRows, groups = 0, wpb = 4;  // rows per wave, items per region, waves per block
    bool balanced = false;        // k_res_update_bal (else k_res_update)
    bool begin_fused = false;     // k_res_begin (else the update grid, then the v_ml readout grid)
    bool finish_grouped = false;  // k_res_finish_grid in column groups (else one thread per output)
    bool drive_fused = false;     // k_res_drive (else a column writer and an update per column)
};

StepShape step_shape(const StepShapeIn &in);

// ------------------------------------------------------------------ ensemble members
// Members (sml_res_set_members): E states advance through one stream of the weights.
// A members kernel (sml_res_members.hpp) serves a tile of members per block (update) or
// per wave (readout); members beyond one tile run as further tiles, each of which reads
// the weights again.
#ifndef SML_MEMBER_TILE
#define SML_MEMBER_TILE 2  // 2 or 4 (profiles/members.md: 4 x 17 sums a wave do not fit the registers)
#endif
constexpr int kMemberTile = SML_MEMBER_TILE;
static_assert(kMemberTile == 2 || kMemberTile == 4, "the members kernels are built for tiles of 2 and 4");
constexpr int kMaxMembers = 32;  // SML_RES_MAX_MEMBERS

struct MemberShapeIn {
    int members;
    size_t lds_region;  // StepShape::lds_region: x and u of the largest region, one member
    bool region_lds;    // StepShape::region_lds: the per-region update stages in LDS
    size_t max_lds;     // the device's LDS per workgroup
};

struct MemberShape {
    int update_tile;      // members a block of k_res_update_mem serves
    bool update_lds;      // their x and u staged side by side in LDS (else gathered from global memory)
    size_t lds;           // the block's LDS: update_tile staging buffers
    int readout_tile;     // members a wave of k_res_readout_mem serves per W_out load
    int readout_streams;  // times W_out is streamed per step: ceil(members / readout_tile)
};

MemberShape member_shape(const MemberShapeIn &in);

// The members' finish from forecast grids (k_res_finish_grid_mem): one block per (region,
// tile of members), the tile's gathers in flight together, about 10 KB of LDS a member.
// kFinTileMax: the compile-time bound of the tile; kFinTile: the tile of the build.  A tile
// of 1 is the single-member kernel once per member on the members' pointers: the same bits.
constexpr int kFinTileMax = 4;
#ifndef SML_MEMBER_FIN_TILE
#define SML_MEMBER_FIN_TILE 4  // profiles/members.md
#endif
constexpr int kFinTile = SML_MEMBER_FIN_TILE;
static_assert(kFinTile >= 1 && kFinTile <= kFinTileMax, "the members finish is built for tiles of 1 .. kFinTileMax");

struct MemberFinish {
    int tile;     // members a block of k_res_finish_grid_mem serves (TF)
    int tiles;    // blocks per region: ceil(members / tile)
    bool looped;  // tile 1 at members > 1: k_res_finish_grid once per member instead
    size_t lds;   // the block's LDS at that tile, in bytes
};

// want: 0 the build's tile, 1 .. kFinTileMax that tile (a measurement's choice)
MemberFinish member_finish(int members, int want = 0);

// ------------------------------------------------------------------ one region's weights
// what sml_res_load_region uploads, in the storage dtype: A and W_in as CSR, W_out
// transposed and padded (wt [nout_pad][ld]) with its local-model block (wl [ncs][nout_pad]),
// and the ELL copies where the region's rows fit them (RegionDev; empty otherwise)
template <typename StoT>
struct PackedRegion {
    std::vector<int32_t> rp, wrp;
    std::vector<uint16_t> acol, wcol;
    std::vector<StoT> aval, wval, wt, wl;
    std::vector<uint16_t> a_ec, w_ec;  // ELL columns: A pair-major, W_in [n]
    std::vector<StoT> a_ev, w_ev;
    std::vector<uint64_t> om;  // A's overflow bits, one word per 64 rows
    std::vector<uint32_t> ob;  // overflow entries before each word
    std::vector<uint16_t> oc;  // overflow entries: column
    std::vector<StoT> ovv;     //                   value
    int a_w = 0, a_ov = 0, w_w = 0, w_q = 0;
    uint32_t w_magic = 0;
    int64_t wnz = 0;
};

struct PackIn {
    int i;  // the region's local index (error messages)
    int k, ncs, nout, nout_pad;
    int a_ell_cap, w_ell_cap;
};

// rows / cols / vals: A as COO, 1-based, k entries; win(n, ninp) and wout(nout, ncs + n)
// column-major.  fp32 storage demands exact representability.
template <typename SrcT, typename StoT>
int pack_region(const PackIn &in, const RegionDev &rg, const int *rows, const int *cols, const SrcT *vals,
                const SrcT *win, const SrcT *wout, PackedRegion<StoT> *out);

// ------------------------------------------------------------------ index tables
struct TablesIn {
    int numregions, nlocal, ncs, nout;
    const RegionGeom *geom;    // [nlocal]
    const unsigned char *sst;  // [nlocal]
    const int *ninp;           // [nlocal]
    const RegionDev *rd;       // [nlocal] (fb)
    int64_t tot_fb;
    const int8_t *out_l;  // generic context: [nout] unstandardise slots (no other table); else null
};

struct RegionTables {
    std::vector<int32_t> asm_dst;  // [numregions*nout] -> concatenated grid index
    std::vector<int32_t> fb_src;   // [tot_fb]
    std::vector<uint8_t> fb_l;
    std::vector<uint16_t> fb_reg;
    std::vector<int32_t> lm_src;  // [nlocal*ncs]
    std::vector<uint8_t> lm_l;
    std::vector<int32_t> tisr_fb, tisr_grid;  // feedback index, grid2d index of the overlap-tile point
    std::vector<uint16_t> tisr_reg;           // local region
    std::vector<int8_t> outl;                 // [nout] mean / std slot of each output
    std::vector<int32_t> tgt_idx;             // [nlocal][nout] the targets' positions in each region's feedback
};

int build_region_tables(const TablesIn &in, RegionTables *out);

// ------------------------------------------------------------------ series tables
// One step of a training series as one index space (sml_res_series_stats,
// sml_res_tile_series): the 4-d grid's kGrid4d doubles, then the four 2-d fields of
// kGrid2d points each in the order of kSer*.  A field has a pointer of its own: the
// index names the field and the point, not an address.
constexpr int kSerLogp = 0, kSerPrecip = 1, kSerSst = 2, kSerTisr = 3, kSerFields2d = 4;
constexpr int kSerPoints = kGrid4d + kSerFields2d * kGrid2d;  // 165888

// the statistics' split of T steps into S chunks of at most `len` steps (none empty):
// a function of T alone, so the summation order depends on nothing else
constexpr int kSerChunkMin = 16;  // steps a chunk holds before T is split further
constexpr int kSerSplitMax = 16;  // chunks at most
struct SeriesSplit {
    int S, len;
};
inline SeriesSplit series_split(int T) {
    const int want = std::min(kSerSplitMax, (T + kSerChunkMin - 1) / kSerChunkMin);
    const int len = (T + std::max(want, 1) - 1) / std::max(want, 1);
    return {len > 0 ? (T + len - 1) / len : 0, len};
}

// what build_region_tables does not hold: every feedback entry's source in the series'
// index space -- the sst and tisr entries included, which the single-grid tables leave to
// other stages -- with its mean / std slot, and each local region's input-tile points
struct SeriesTables {
    std::vector<int32_t> src;     // [tot_fb] series index; an sst entry of an unflagged region does not exist
    std::vector<uint8_t> l;       // [tot_fb] slot: v * 8 + z, 32 logp, 34 precip, 35 sst, 33 tisr
    std::vector<int32_t> pt_off;  // [nlocal + 1] region i's points: pt_grid[pt_off[i] .. pt_off[i + 1])
    std::vector<int32_t> pt_grid; // 2-d grid index of each input-tile point, in the tile's (x fastest) order
};

int build_series_tables(const TablesIn &in, SeriesTables *out);

// mean/std index (0-based) of output o of the bottom-level 2x2 reservoir:
// atmo (var,x,y,z) -> (var-1)*8+z, logp -> 33, precip -> 35 (1-based; :1815-1846)
int out_std_index(int o, const RegionGeom &g);

// the balanced update: the region each of G blocks' share of the rows starts in
// (row0 [nlocal+1] = the regions' rows concatenated)
std::vector<int32_t> block_first_regions(const std::vector<int32_t> &row0, int G);

// sml_res_footprint: unpadded weight bytes, and the minimal traffic of a step
// (wb: bytes per stored weight)
void footprint(int nlocal, const int *n, const int *k, const int *ninp, int ncs, int nout, int64_t wb,
               int64_t *weight_bytes, int64_t *algo_bytes);

}  // namespace sml
