// ens_layout_check.cpp -- CPU check of the ensemble products' host unit
// (speedy-ml-1_amd/csrc/sml_ens_layout.cpp): the area weights against the Gaussian table,
// the field table against the grids' plain index arithmetic, the score tables' row
// offsets, and every refusal with its message.  Stand-alone
// (tests/test_ens_layout_cpu.py builds it plain and under ASan/UBSan).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sml_ens_layout.hpp"
#include "sml_spectral_tables.hpp"

using namespace sml;

static int g_fail = 0, g_checks = 0;
static std::string g_case;
#define CHECK(cond, ...)                                              \
    do {                                                              \
        ++g_checks;                                                   \
        if (!(cond)) {                                                \
            if (++g_fail <= 40) {                                     \
                std::printf("FAIL [%s] %s:%d %s -- ", g_case.c_str(), __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                             \
                std::printf("\n");                                    \
            }                                                         \
        }                                                             \
    } while (0)

static void refuse(const char *what, int rc, const char *needle) {
    g_case = what;
    CHECK(rc == SML_ERR_ARG, "rc %d", rc);
    CHECK(std::strstr(sml_last_error(), needle) != nullptr, "message '%s' lacks '%s'", sml_last_error(), needle);
}

int main() {
    // ---- the weights
    g_case = "weights";
    double w[48];
    CHECK(ens_weights(w) == SML_OK, "%s", sml_last_error());
    std::unique_ptr<SpectralTables> t(new SpectralTables);
    build_spectral_tables(1.0, t.get());
    {
        double sum = 0.0;  // over the 4608 points, row by row
        for (int j = 0; j < 48; ++j)
            for (int i = 0; i < 96; ++i) sum += w[j];
        const double ulp = std::ldexp(1.0, -52);
        CHECK(std::fabs(sum - 1.0) <= 48 * ulp, "the weights sum to 1 %+.3e", sum - 1.0);
        double wsum = 0.0;
        for (int j = 0; j < 24; ++j) wsum += 2.0 * t->wt[j];
        CHECK(std::fabs(wsum - 2.0) < 1e-13, "the Gaussian weights sum to %.17g, not 2", wsum);
        for (int j = 0; j < 48; ++j) {
            CHECK(w[j] == w[47 - j], "row %d: not symmetric about the equator", j);
            // the definition, with the table's own weights
            const double want = t->wt[j < 24 ? j : 47 - j] / (96.0 * wsum);
            CHECK(std::fabs(w[j] - want) <= 4 * ulp * want, "row %d: %.17g, want %.17g", j, w[j], want);
        }
        for (int j = 1; j < 24; ++j) {
            // sia runs from the pole (index 0) to the equator: cos(lat) grows, and so does the weight
            const double c0 = std::sqrt(1.0 - t->sia[j - 1] * t->sia[j - 1]), c1 = std::sqrt(1.0 - t->sia[j] * t->sia[j]);
            CHECK(t->sia[j] < t->sia[j - 1] && c1 > c0, "sia(%d) does not run towards the equator", j);
            CHECK(w[j] > w[j - 1] && w[47 - j] > w[48 - j], "row %d: the weight does not grow towards the equator", j);
            // a Gaussian weight is close to cos(lat) * the latitude spacing: the ratio stays near constant
            const double r0 = w[j - 1] / c0, r1 = w[j] / c1;
            CHECK(std::fabs(r1 / r0 - 1.0) < 0.02, "row %d: weight / cos(lat) jumps by %.3f", j, r1 / r0);
        }
    }
    refuse("null weights", ens_weights(nullptr), "null argument");

    // ---- the field table: every element of the three arrays exactly once
    g_case = "fields";
    {
        std::vector<int> hit4(kGrid4d, 0), hit2(kGrid2d, 0), hitp(kGrid2d, 0);
        for (int f = 0; f < kEnsFields; ++f) {
            EnsField fd{};
            CHECK(ens_field(f, &fd) == SML_OK, "field %d: %s", f, sml_last_error());
            for (int j = 0; j < 48; ++j)
                for (int i = 0; i < 96; ++i) {
                    const int el = fd.offset + (j * 96 + i) * fd.step;
                    if (f < 32) {
                        const int k = f / 4, v = f % 4;
                        if (fd.array != 0 || el != ((k * 48 + j) * 96 + i) * 4 + v)
                            CHECK(false, "field %d (%d, %d): array %d element %d", f, j, i, fd.array, el);
                        if (el >= 0 && el < kGrid4d) ++hit4[el];
                    } else {
                        if (fd.array != f - 31 || el != j * 96 + i)
                            CHECK(false, "field %d (%d, %d): array %d element %d", f, j, i, fd.array, el);
                        if (el >= 0 && el < kGrid2d) ++(f == 32 ? hit2 : hitp)[el];
                    }
                }
        }
        int bad = 0;
        for (int h : hit4) bad += h != 1;
        for (int h : hit2) bad += h != 1;
        for (int h : hitp) bad += h != 1;
        CHECK(bad == 0, "%d elements belong to no field or to several", bad);
        CHECK(kEnsFields == 34 && kEnsScores == 4 && kEnsRankBins == 33, "table shape");
        EnsField fd{};
        refuse("field -1", ens_field(-1, &fd), "field -1 out of range [0, 34)");
        refuse("field 34", ens_field(34, &fd), "field 34 out of range [0, 34)");
        refuse("null field", ens_field(0, nullptr), "null argument");
    }

    // ---- the tables' rows
    g_case = "rows";
    for (int cap : {1, 3, 1000}) {
        CHECK(ens_score_offset(0, 0) == 0 && ens_rank_offset(0, 0) == 0, "row 0");
        CHECK(ens_score_offset(cap - 1, 0) == (int64_t)(cap - 1) * 34 * 4, "scores row %d", cap - 1);
        CHECK(ens_rank_offset(cap - 1, 0) == (int64_t)(cap - 1) * 34 * 33, "ranks row %d", cap - 1);
        CHECK(ens_score_offset(cap - 1, 33) + 4 == ens_score_offset(cap, 0), "the last field ends the scores table");
        CHECK(ens_rank_offset(cap - 1, 33) + 33 == ens_rank_offset(cap, 0), "the last field ends the ranks table");
        CHECK(check_ens_row(0, cap) == SML_OK && check_ens_row(cap - 1, cap) == SML_OK, "%s", sml_last_error());
        CHECK(check_ens_read(0, cap, cap) == SML_OK && check_ens_read(cap - 1, 1, cap) == SML_OK &&
                  check_ens_read(cap, 0, cap) == SML_OK,
              "%s", sml_last_error());
    }

    // ---- the refusals
    g_case = "accepted";
    CHECK(check_ens_create(1, 1) == SML_OK && check_ens_create(32, 100000) == SML_OK, "%s", sml_last_error());
    refuse("members 0", check_ens_create(0, 4), "members 0 out of range [1, 32]");
    refuse("members 33", check_ens_create(33, 4), "members 33 out of range [1, 32]");
    refuse("capacity 0", check_ens_create(4, 0), "capacity_steps 0");
    refuse("capacity too large", check_ens_create(4, 2000000), "capacity_steps 2000000 too large");
    alignas(16) const double xa[2] = {0.0, 0.0};
    const double &x = xa[0];
    refuse("an odd g4 stride", check_ens_members(&x, kGrid4d + 1, &x, kGrid2d), "g4_stride 147457 odd");
    refuse("g4 off a 16-byte boundary", check_ens_members(&xa[1], kGrid4d, &x, kGrid2d), "d_g4 not 16-byte aligned");
    refuse("an output off a 16-byte boundary", check_ens_quads(&xa[1], "d_mean4"), "d_mean4 not 16-byte aligned");
    g_case = "accepted";
    CHECK(check_ens_quads(nullptr, "d_mean4") == SML_OK && check_ens_quads(&x, "d_mean4") == SML_OK, "%s", sml_last_error());
    CHECK(check_ens_members(&x, kGrid4d, &x, kGrid2d) == SML_OK && check_ens_members(&x, kGrid4d + 8, &x, kGrid2d + 1) == SML_OK,
          "%s", sml_last_error());
    refuse("a short g4 stride", check_ens_members(&x, kGrid4d - 1, &x, kGrid2d),
           "g4_stride 147455 smaller than the 4-d grid's 147456 doubles");
    refuse("a short g2 stride", check_ens_members(&x, kGrid4d, &x, kGrid2d - 1),
           "g2_stride 4607 smaller than the 2-d grid's 4608 doubles");
    refuse("a negative stride", check_ens_members(&x, -kGrid4d, &x, kGrid2d), "g4_stride -147456 smaller");
    refuse("no g4", check_ens_members(nullptr, kGrid4d, &x, kGrid2d), "null members' grid");
    refuse("no g2", check_ens_members(&x, kGrid4d, nullptr, kGrid2d), "null members' grid");
    refuse("t -1", check_ens_row(-1, 3), "t -1 out of range [0, 3)");
    refuse("t at the capacity", check_ens_row(3, 3), "t 3 out of range [0, 3)");
    refuse("rows past the table", check_ens_read(2, 2, 3), "rows [2, 2 + 2) outside [0, 3)");
    refuse("a negative count", check_ens_read(0, -1, 3), "outside [0, 3)");
    g_case = "accepted";
    CHECK(check_ens_truth(nullptr, nullptr, nullptr) == SML_OK && check_ens_truth(&x, &x, nullptr) == SML_OK &&
              check_ens_truth(&x, &x, &x) == SML_OK,
          "%s", sml_last_error());
    refuse("truth: the 4-d grid alone", check_ens_truth(&x, nullptr, nullptr), "truth half given (d_truth4 set, d_truth2 NULL");
    refuse("truth: the 2-d grid alone", check_ens_truth(nullptr, &x, nullptr), "truth half given (d_truth4 NULL, d_truth2 set");
    refuse("truth: precip alone", check_ens_truth(nullptr, nullptr, &x), "d_truthpr set");
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
