// sml_ens_layout.cpp -- the ensemble products' field table, area weights, table layout and
// argument checks (sml_ens_layout.hpp).  Host only.
#include "sml_ens_layout.hpp"

#include <memory>

#include "sml_spectral_tables.hpp"

namespace sml {

int ens_field(int f, EnsField *out) {
    SML_REQUIRE(out, "null argument");
    SML_REQUIRE(f >= 0 && f < kEnsFields, "field %d out of range [0, %d)", f, kEnsFields);
    if (f < kVars * kZGrid) {
        *out = {0, (f / kVars) * kGrid2d * kVars + f % kVars, kVars};
    } else {
        *out = {f - kVars * kZGrid + 1, 0, 1};
    }
    return SML_OK;
}

int ens_weights(double *w48) {
    SML_REQUIRE(w48, "null argument");
    std::unique_ptr<SpectralTables> t(new SpectralTables);
    build_spectral_tables(1.0, t.get());
    // parmtr pairs sia(j) with the rows j and 49 - j (1-based): index 0 is the row next to
    // the pole, where the weight is smallest
    for (int j = 0; j < kIY; ++j) {
        SML_REQUIRE(t->sia[j] > 0.0 && t->sia[j] < 1.0 && t->wt[j] > 0.0, "Gaussian row %d: sia %g, wt %g", j,
                    t->sia[j], t->wt[j]);
        SML_REQUIRE(j == 0 || (t->sia[j] < t->sia[j - 1] && t->wt[j] > t->wt[j - 1]),
                    "Gaussian rows %d, %d do not run from the pole to the equator", j - 1, j);
    }
    double sum = 0.0;
    for (int j = 0; j < kYGrid; ++j) sum = sum + t->wt[j < kIY ? j : kYGrid - 1 - j];
    for (int j = 0; j < kYGrid; ++j) w48[j] = t->wt[j < kIY ? j : kYGrid - 1 - j] / ((double)kXGrid * sum);
    return SML_OK;
}

int check_ens_create(int members, int capacity_steps) {
    SML_REQUIRE(members >= 1 && members <= SML_RES_MAX_MEMBERS, "members %d out of range [1, %d]", members,
                SML_RES_MAX_MEMBERS);
    SML_REQUIRE(capacity_steps >= 1, "capacity_steps %d: at least one row expected", capacity_steps);
    SML_REQUIRE((int64_t)capacity_steps * kEnsFields * kEnsRankBins < INT32_MAX, "capacity_steps %d too large",
                capacity_steps);
    return SML_OK;
}

int check_ens_members(const void *g4, int64_t g4_stride, const void *g2, int64_t g2_stride) {
    SML_REQUIRE(g4 && g2, "null members' grid (d_g4, d_g2)");
    SML_REQUIRE(g4_stride >= kGrid4d, "g4_stride %lld smaller than the 4-d grid's %d doubles", (long long)g4_stride,
                kGrid4d);
    SML_REQUIRE(g2_stride >= kGrid2d, "g2_stride %lld smaller than the 2-d grid's %d doubles", (long long)g2_stride,
                kGrid2d);
    SML_REQUIRE(g4_stride % 2 == 0, "g4_stride %lld odd: the 4-d grid's quads are read as 16-byte loads",
                (long long)g4_stride);
    return check_ens_quads(g4, "d_g4");
}

int check_ens_quads(const void *p, const char *name) {
    SML_REQUIRE((uintptr_t)p % 16 == 0, "%s not 16-byte aligned: the 4-d grid's quads move as 16-byte accesses", name);
    return SML_OK;
}

int check_ens_truth(const void *truth4, const void *truth2, const void *truthpr) {
    SML_REQUIRE((truth4 && truth2) || (!truth4 && !truth2 && !truthpr),
                "truth half given (d_truth4 %s, d_truth2 %s, d_truthpr %s): all NULL, or d_truth4 and d_truth2",
                truth4 ? "set" : "NULL", truth2 ? "set" : "NULL", truthpr ? "set" : "NULL");
    return SML_OK;
}

int check_ens_row(int t, int capacity_steps) {
    SML_REQUIRE(t >= 0 && t < capacity_steps, "t %d out of range [0, %d)", t, capacity_steps);
    return SML_OK;
}

int check_ens_read(int t0, int count, int capacity_steps) {
    SML_REQUIRE(t0 >= 0 && count >= 0 && t0 <= capacity_steps - count, "rows [%d, %d + %d) outside [0, %d)", t0, t0,
                count, capacity_steps);
    return SML_OK;
}

}  // namespace sml
