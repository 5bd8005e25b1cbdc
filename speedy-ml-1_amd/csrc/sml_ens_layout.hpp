// sml_ens_layout.hpp -- the ensemble products' host side (sml_ensemble.hip): the table of
// the 34 fields of an assembled grid, the area weights of the 48 Gaussian rows, the layout
// of the score and rank tables, and every argument check of the sml_ens_* entry points.
// No HIP call in between, so all of it runs (and is sanitised) on a CPU:
// tests/ens_layout_check.cpp.
#pragma once

#include <cstdint>

#include "sml_internal.hpp"

namespace sml {

// field f = 4k + v: level k, variable v of grid4d [8, 48, 96, 4]; 32: logp, 33: precip
constexpr int kEnsFields = 4 * kZGrid + 2;  // 34
constexpr int kEnsScores = 4;               // rmse, spread, crps, bias
constexpr int kEnsRankBins = SML_RES_MAX_MEMBERS + 1;  // r = #{e : x_e < y} in 0 .. 32
enum { kEnsRmse = 0, kEnsSpread = 1, kEnsCrps = 2, kEnsBias = 3 };

// where field f lives: array 0 grid4d, 1 grid2d (logp), 2 precip; point p = j * 96 + i of
// the field is element offset + p * step of that array
struct EnsField {
    int array, offset, step;
};
int ens_field(int f, EnsField *out);

// w48[j] = wt[min(j, 47 - j)] / (96 * sum_j wt[min(j, 47 - j)]): the weight of one point of
// row j, wt the Gaussian weights of parmtr (rows j and 47 - j share sia(min(j, 47 - j)),
// index 0 next to the pole).  Refuses tables whose latitudes do not run from pole to
// equator with growing weights.
int ens_weights(double *w48);

// row t of scores [T][34][4] and ranks [T][34][33], in elements
inline int64_t ens_score_offset(int t, int f) { return ((int64_t)t * kEnsFields + f) * kEnsScores; }
inline int64_t ens_rank_offset(int t, int f) { return ((int64_t)t * kEnsFields + f) * kEnsRankBins; }

int check_ens_create(int members, int capacity_steps);
// a 4-d grid (NULL passes) is 16-byte aligned: its quads move as 16-byte accesses
int check_ens_quads(const void *p, const char *name);
// the members' arrays: g4 and g2 given, strides >= the packed grids (precip goes by g2's),
// g4 16-byte aligned with an even stride
int check_ens_members(const void *g4, int64_t g4_stride, const void *g2, int64_t g2_stride);
// truth: all NULL, or grid4d and grid2d given (precip may be NULL beside them)
int check_ens_truth(const void *truth4, const void *truth2, const void *truthpr);
int check_ens_row(int t, int capacity_steps);
int check_ens_read(int t0, int count, int capacity_steps);

}  // namespace sml
