// slab_series_layout_check.cpp -- CPU check of the slab training series' table
// (build_slab_series_tables, speedy-ml-1_amd/csrc/sml_slab_layout.cpp) and of the slab's
// target positions (slab_target_index): every entry's source in the series' index space,
// its mean / std slot and its local atmo row are compared with the plain definition,
// written out here from the regions' geometry and the documented slab feedback
//     [lowest level (4, inx, iny) | logp (inx, iny) | sst (inx, iny) | tisr (inx, iny)]
// without the unit's own index code.  Stand-alone (tests/test_slab_series_layout_cpu.py
// builds it plain and under ASan/UBSan).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sml_reservoir_layout.hpp"
#include "sml_slab_layout.hpp"

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

// a rank's atmo context with its series tables, and its slab context
struct Ctx {
    int numregions = 1152, nout = 136, snum = 1152, sncs = 0, snout = 4;
    std::vector<int> ids, ninp, sids, sninp;
    std::vector<int64_t> off, soff;
    std::vector<unsigned char> sst;
    std::vector<RegionGeom> geom;
    SeriesTables ser;
    SlabLayoutIn in() const {
        return {numregions, (int)ids.size(), nout, ids.data(), ninp.data(), off.data(), snum, (int)sids.size(), sncs,
                snout, sids.data(), sninp.data(), soff.data()};
    }
};

static Ctx make(const std::vector<int> &regions, const std::vector<unsigned char> &sst, int numregions = 1152) {
    Ctx c;
    c.numregions = c.snum = numregions;
    c.soff.push_back(0);
    const int nlocal = (int)regions.size();
    c.geom.resize(nlocal);
    std::vector<int> n(nlocal, 64), k(nlocal, 128);
    for (int i = 0; i < nlocal; ++i) {
        region_geom(numregions, regions[i], &c.geom[i]);
        c.ids.push_back(regions[i]);
        c.sst.push_back(sst[i]);
        c.ninp.push_back(region_ninp(c.geom[i], sst[i] != 0));
        if (sst[i]) {
            c.sids.push_back(regions[i]);
            c.sninp.push_back(7 * c.geom[i].inx * c.geom[i].iny);
            c.soff.push_back(c.soff.back() + c.sninp.back());
        }
    }
    RegionGeom g0{};
    region_geom(numregions, 0, &g0);
    const int resxy = g0.resx * g0.resy;
    c.snout = resxy;
    c.nout = 34 * resxy;
    const int ncs = 33 * resxy;
    // the atmo context's feedback offsets and series tables, as the reservoir unit lays them out
    const PoolPlan plan = plan_pools({nlocal, n.data(), k.data(), c.ninp.data(), ncs, (c.nout + kRows - 1) / kRows * kRows, false});
    for (int i = 0; i < nlocal; ++i) c.off.push_back(plan.rd[i].fb);
    c.off.push_back(plan.tot_fb);
    const TablesIn tin{numregions, nlocal, ncs, c.nout, c.geom.data(), c.sst.data(), c.ninp.data(), plan.rd.data(), plan.tot_fb, nullptr};
    CHECK(build_series_tables(tin, &c.ser) == SML_OK, "build_series_tables: %s", sml_last_error());
    return c;
}

// 0-based global column of 0-based local column lx: in_xstart onwards, wrapping past 96
static int wrap_x(const RegionGeom &g, int lx) { return (g.in_xstart - 1 + lx) % kXGrid; }

static void check_tables(const Ctx &c) {
    SlabSeriesTables t;
    const int rc = build_slab_series_tables(c.in(), c.ser.src.data(), c.ser.l.data(), (int64_t)c.ser.src.size(), &t);
    CHECK(rc == SML_OK, "rc %d: %s", rc, sml_last_error());
    if (rc != SML_OK) return;
    std::vector<int32_t> src;
    std::vector<uint8_t> l;
    std::vector<uint16_t> row;
    for (size_t i = 0; i < c.ids.size(); ++i) {
        if (!c.sst[i]) continue;
        const RegionGeom &g = c.geom[i];
        // the lowest level (the 8th) of the 4 variables, point by point, v fastest ...
        for (int ly = 0; ly < g.iny; ++ly)
            for (int lx = 0; lx < g.inx; ++lx)
                for (int v = 0; v < 4; ++v) {
                    src.push_back(v + 4 * (wrap_x(g, lx) + 96 * ((g.in_ystart - 1 + ly) + 48 * 7)));
                    l.push_back((uint8_t)(v * 8 + 7));
                    row.push_back((uint16_t)i);
                }
        // ... then logp (field 0, slot 32), sst (field 2, slot 35), tisr (field 3, slot 33): not the precipitation
        const int field[3] = {0, 2, 3}, slot[3] = {32, 35, 33};
        for (int b = 0; b < 3; ++b)
            for (int ly = 0; ly < g.iny; ++ly)
                for (int lx = 0; lx < g.inx; ++lx) {
                    src.push_back(147456 + field[b] * 4608 + wrap_x(g, lx) + 96 * (g.in_ystart - 1 + ly));
                    l.push_back((uint8_t)slot[b]);
                    row.push_back((uint16_t)i);
                }
        CHECK(g.in_ystart >= 1 && g.in_ystart - 1 + g.iny <= 48, "region %d: the tile leaves the grid", c.ids[i]);
    }
    CHECK(t.src.size() == src.size() && (int64_t)src.size() == c.soff.back(), "%zu entries, want %zu = the slab feedback's %lld",
          t.src.size(), src.size(), (long long)c.soff.back());
    if (t.src.size() != src.size()) return;
    for (size_t e = 0; e < src.size(); ++e) {
        if (t.src[e] != src[e]) CHECK(false, "src[%zu] = %d, want %d", e, t.src[e], src[e]);
        if (t.l[e] != l[e]) CHECK(false, "l[%zu] = %d, want %d", e, t.l[e], l[e]);
        if (t.row[e] != row[e]) CHECK(false, "row[%zu] = %d, want %d", e, t.row[e], row[e]);
        if (t.src[e] < 0 || t.src[e] >= kSerPoints) CHECK(false, "src[%zu] = %d leaves the series' index space", e, t.src[e]);
    }
    CHECK(t.src == src && t.l == l && t.row == row, "tables");
}

// the slab's targets: the region's own points inside the sst section of the slab feedback
static void check_targets(int numregions, int region) {
    RegionGeom g{};
    CHECK(region_geom(numregions, region, &g), "geometry");
    std::vector<int32_t> idx((size_t)g.resx * g.resy + 1, -7);
    int count = 0;
    CHECK(sml_slab_target_index(numregions, region, idx.data(), &count) == SML_OK, "%s", sml_last_error());
    CHECK(count == g.resx * g.resy && idx.back() == -7, "count %d", count);
    const int in2d = g.inx * g.iny;
    // the region's first point inside its input tile: one halo column, one halo row unless at the south pole
    const int x0 = 1, y0 = g.res_ystart == 1 ? 0 : 1;
    for (int o = 0; o < g.resx * g.resy; ++o) {
        const int lx = x0 + o % g.resx, ly = y0 + o / g.resx;
        CHECK(idx[o] == 5 * in2d + lx + g.inx * ly, "region %d target %d: %d, want %d", region, o, idx[o], 5 * in2d + lx + g.inx * ly);
        // that tile point is the resolved point itself
        CHECK(wrap_x(g, lx) == g.res_xstart - 1 + o % g.resx && g.in_ystart - 1 + ly == g.res_ystart - 1 + o / g.resx,
              "region %d target %d is not its resolved point", region, o);
    }
}

static void refuse(const char *what, int rc, const char *needle) {
    g_case = what;
    CHECK(rc != SML_OK, "accepted");
    CHECK(std::strstr(sml_last_error(), needle) != nullptr, "message '%s' lacks '%s'", sml_last_error(), needle);
}

int main() {
    for (int r : {0, 120, 143, 5, 1133, 500}) {
        g_case = "single region " + std::to_string(r);
        check_tables(make({r}, {1}));
        check_targets(1152, r);
    }
    g_case = "a region without sst";
    {
        Ctx c = make({500}, {0});
        SlabSeriesTables t;
        CHECK(build_slab_series_tables(c.in(), c.ser.src.data(), c.ser.l.data(), (int64_t)c.ser.src.size(), &t) == SML_OK, "%s", sml_last_error());
        CHECK(t.src.empty() && t.l.empty() && t.row.empty(), "not empty");
    }
    g_case = "sst and no sst side by side";
    check_tables(make({0, 1, 23, 24, 500, 501, 1151}, {1, 0, 1, 1, 0, 1, 1}));
    g_case = "the whole 1152 decomposition";
    {
        std::vector<int> all(1152);
        std::vector<unsigned char> sst(1152);
        for (int r = 0; r < 1152; ++r) {
            all[r] = r;
            sst[r] = r % 9 != 4;
            check_targets(1152, r);
        }
        check_tables(make(all, sst));
    }
    // the shares of 8 and of 7 ranks (processor_decomposition: 7 leaves 4 regions over, one each to ranks 1..4)
    for (int np : {8, 7}) {
        int seen = 0;
        for (int rank = 0; rank < np; ++rank) {
            g_case = "rank " + std::to_string(rank) + " of " + std::to_string(np);
            std::vector<int> mine(1152);
            mine.resize(processor_regions(1152, np, rank, mine.data()));
            std::vector<unsigned char> sst(mine.size());
            for (size_t i = 0; i < mine.size(); ++i) sst[i] = mine[i] % 7 != 3;
            seen += (int)mine.size();
            check_tables(make(mine, sst));
        }
        CHECK(seen == 1152, "%d ranks hold %d regions", np, seen);
    }
    g_case = "288 regions of 4 x 4 points";
    {
        std::vector<int> all(288);
        std::vector<unsigned char> sst(288);
        for (int r = 0; r < 288; ++r) {
            all[r] = r;
            sst[r] = r % 5 != 0;
            check_targets(288, r);
        }
        check_tables(make(all, sst, 288));
    }

    // ---- the refusals: build_slab_tables' carry through, then the table's own
    SlabSeriesTables t;
    const Ctx good = make({0, 1, 500}, {1, 0, 1});
    auto build = [&](const Ctx &c) {
        return build_slab_series_tables(c.in(), good.ser.src.data(), good.ser.l.data(), (int64_t)good.ser.src.size(), &t);
    };
    {
        Ctx c = good;
        c.snum = 288;
        refuse("another decomposition", build(c), "must be ML-only (chunk_speedy 0) over the same 1152");
        c = good;
        c.sncs = 132;
        refuse("a hybrid slab context", build(c), "must be ML-only");
        c = good;
        c.snout = 136;
        refuse("nout", build(c), "predict the sst of the region's 4 points, not 136");
        c = good;
        c.sids[1] = 501;
        refuse("another region's slab", build(c), "slab reservoir 1 is not the rank's sst region 500 (local 2)");
        c = good;
        c.sids.pop_back();
        c.sninp.pop_back();
        c.soff.pop_back();
        refuse("a slab missing", build(c), "slab reservoir 1 is not the rank's sst region 500");
        c = good;
        c.sids.push_back(700);
        c.sninp.push_back(7 * 16);
        c.soff.push_back(c.soff.back() + 7 * 16);
        refuse("a slab too many", build(c), "3 slab reservoirs for 2 sst regions");
        c = good;
        c.sninp[1] = 8 * 16;
        refuse("inputs", build(c), "slab reservoir of region 500: 128 inputs, the atmo subset has 112");
        c = good;
        c.ids[2] = 1152;
        refuse("no such region", build(c), "1152 is no region of 1152");
        refuse("null out", build_slab_series_tables(good.in(), good.ser.src.data(), good.ser.l.data(), (int64_t)good.ser.src.size(), nullptr),
               "bad argument");
        refuse("short series tables", build_slab_series_tables(good.in(), good.ser.src.data(), good.ser.l.data(), (int64_t)good.ser.src.size() - 1, &t),
               "the series tables hold");
        refuse("null series tables", build_slab_series_tables(good.in(), nullptr, good.ser.l.data(), (int64_t)good.ser.src.size(), &t),
               "the series tables hold");
        g_case = "a refusal leaves the tables empty";
        CHECK(t.src.empty() && t.l.empty() && t.row.empty(), "not empty");
        int cnt = 0;
        int32_t one[16];
        refuse("target index: no region", sml_slab_target_index(1152, 1152, one, &cnt), "does not decompose the grid");
        refuse("target index: null", sml_slab_target_index(1152, 0, nullptr, &cnt), "null argument");
    }
    std::printf("slab_series_layout_check: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
