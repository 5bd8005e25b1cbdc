// slab_layout_check.cpp -- CPU check of the slab ocean's table unit
// (speedy-ml-1_amd/csrc/sml_slab_layout.cpp): every table is compared with its plain
// definition from the region geometry, written out here without the unit's own code, and
// every refusal's message is provoked.  Stand-alone (tests/test_slab_layout_cpu.py builds
// it plain and under ASan/UBSan).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

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

// a rank's atmo context and its slab context, as the ABI's getters would report them
struct Ctx {
    int numregions = 1152, nout = 136, snum = 1152, sncs = 0, snout = 4;
    std::vector<int> ids, ninp, sids, sninp;
    std::vector<int64_t> off, soff;
    std::vector<char> sst;
    SlabLayoutIn in() const {
        return {numregions, (int)ids.size(), nout, ids.data(), ninp.data(), off.data(), snum, (int)sids.size(), sncs,
                snout, sids.data(), sninp.data(), soff.data()};
    }
};

// the feedback of a region: 4 variables x in2d x 8 levels, logp, precip, [sst], tisr
static int feedback_len(const RegionGeom &g, bool sst) { return (4 * 8 + 2 + (sst ? 1 : 0) + 1) * g.inx * g.iny; }

static Ctx make(const std::vector<int> &regions, const std::vector<char> &sst, int numregions = 1152) {
    Ctx c;
    c.numregions = c.snum = numregions;
    c.off.push_back(0);
    c.soff.push_back(0);
    for (size_t i = 0; i < regions.size(); ++i) {
        RegionGeom g{};
        region_geom(numregions, regions[i], &g);
        c.ids.push_back(regions[i]);
        c.sst.push_back(sst[i]);
        c.ninp.push_back(feedback_len(g, sst[i]));
        c.off.push_back(c.off.back() + c.ninp.back());
        if (sst[i]) {
            c.sids.push_back(regions[i]);
            c.sninp.push_back(7 * g.inx * g.iny);
            c.soff.push_back(c.soff.back() + c.sninp.back());
        }
    }
    RegionGeom g0{};
    region_geom(numregions, 0, &g0);
    c.snout = g0.resx * g0.resy;
    return c;
}

// ---- the plain definitions
static void check_tables(const Ctx &c) {
    SlabTables t;
    const int rc = build_slab_tables(c.in(), &t);
    CHECK(rc == SML_OK, "rc %d: %s", rc, sml_last_error());
    if (rc != SML_OK) return;
    RegionGeom g0{};
    region_geom(c.numregions, 0, &g0);
    const int fx = g0.resx, fy = g0.resy, xw = c.nout + fx * fy;
    CHECK(t.xw == xw, "xw %d, want %d", t.xw, xw);
    // ring_src / row / sfb / sgrid / sreg, region by region
    std::vector<int32_t> ring, row, sfb, sgrid;
    std::vector<uint16_t> sreg;
    int j = 0;
    for (size_t i = 0; i < c.ids.size(); ++i) {
        if (!c.sst[i]) continue;
        RegionGeom g{};
        region_geom(c.numregions, c.ids[i], &g);
        const int in2d = g.inx * g.iny;
        const int64_t o = c.off[i];
        // atmo_training_data_idx: the lowest level (the 8th) of the 4 variables, point by point ...
        for (int y = 0; y < g.iny; ++y)
            for (int x = 0; x < g.inx; ++x)
                for (int v = 0; v < 4; ++v) ring.push_back((int32_t)(o + v + 4 * (x + g.inx * (y + g.iny * 7))));
        // ... logp (block 0 behind the atmo block), not the precipitation (block 1), the sst (2), the tisr (3)
        for (int blk : {0, 2, 3})
            for (int p = 0; p < in2d; ++p) ring.push_back((int32_t)(o + 32 * in2d + blk * in2d + p));
        row.push_back((int32_t)i);
        // the overlap tile's points: one column west of the region (wrapping round the globe),
        // one row south of it unless the region touches the pole
        const int x0 = g.res_xstart - 2, y0 = g.res_ystart == 1 ? 0 : g.res_ystart - 2;
        for (int ly = 0; ly < g.iny; ++ly)
            for (int lx = 0; lx < g.inx; ++lx) {
                sfb.push_back((int32_t)(o + 32 * in2d + 2 * in2d + lx + g.inx * ly));
                sgrid.push_back(((x0 + lx + 96) % 96) + 96 * (y0 + ly));
                sreg.push_back((uint16_t)j);
            }
        CHECK(y0 + g.iny <= 48, "region %d: the tile leaves the grid", c.ids[i]);
        ++j;
    }
    CHECK(t.ring_src == ring, "ring_src: %zu entries, want %zu", t.ring_src.size(), ring.size());
    CHECK(t.row == row, "row");
    CHECK(t.sfb == sfb, "sfb");
    CHECK(t.sgrid == sgrid, "sgrid");
    CHECK(t.sreg == sreg, "sreg");
    CHECK((int64_t)ring.size() == c.soff.back(), "the ring's length %zu is not the slab feedback's %lld", ring.size(),
          (long long)c.soff.back());
    for (size_t e = 0; e < t.ring_src.size(); ++e)
        if (t.ring_src[e] < 0 || t.ring_src[e] >= c.off.back()) CHECK(false, "ring_src[%zu] = %d out of range", e, t.ring_src[e]);
    for (size_t e = 0; e < t.sfb.size(); ++e) {
        if (t.sfb[e] < 0 || t.sfb[e] >= c.off.back()) CHECK(false, "sfb[%zu] = %d out of range", e, t.sfb[e]);
        if (t.sgrid[e] < 0 || t.sgrid[e] >= 96 * 48) CHECK(false, "sgrid[%zu] = %d out of range", e, t.sgrid[e]);
    }
    // src: the point's region from the decomposition (regions run south to north within a
    // column block of fx longitudes, then east), its column within the region
    CHECK((int)t.src.size() == 96 * 48, "src: %zu entries", t.src.size());
    if ((int)t.src.size() != 96 * 48) return;
    const int per_x = 48 / fy;
    std::vector<int> hits((size_t)c.numregions * fx * fy, 0);
    for (int y = 0; y < 48; ++y)
        for (int x = 0; x < 96; ++x) {
            const int r = (x / fx) * per_x + y / fy, col = x % fx + fx * (y % fy);
            const int want = r * xw + c.nout + col;
            if (t.src[x + 96 * y] != want) CHECK(false, "src(%d, %d) = %d, want %d", x, y, t.src[x + 96 * y], want);
            // the region's own extent agrees with that arithmetic
            RegionGeom g{};
            region_geom(c.numregions, r, &g);
            if (!(x + 1 >= g.res_xstart && x + 1 <= g.res_xend && y + 1 >= g.res_ystart && y + 1 <= g.res_yend))
                CHECK(false, "point (%d, %d) is not in region %d", x, y, r);
            const int s = t.src[x + 96 * y];
            if (s >= 0 && s / xw < c.numregions && s % xw >= c.nout) ++hits[(size_t)(s / xw) * fx * fy + s % xw - c.nout];
        }
    // every grid point covered exactly once: 96 * 48 points onto numregions * fx * fy distinct columns
    CHECK((int)hits.size() == 96 * 48, "%zu exchange columns for %d points", hits.size(), 96 * 48);
    int bad = 0;
    for (int h : hits) bad += h != 1;
    CHECK(bad == 0, "%d sst columns are read by no grid point or by several", bad);
}

static void refuse(const char *what, int rc, const char *needle) {
    g_case = what;
    CHECK(rc != SML_OK, "accepted");
    CHECK(std::strstr(sml_last_error(), needle) != nullptr, "message '%s' lacks '%s'", sml_last_error(), needle);
}

int main() {
    // region = 24 * (x block) + (y block) in the 1152 decomposition (2 x 2 points each)
    struct One { const char *name; int region; bool pole, wrap; } ones[] = {
        {"pole and wrap (0)", 0, true, true},     {"south pole (120)", 120, true, false},
        {"north pole (143)", 143, true, false},   {"wrap west (5)", 5, false, true},
        {"wrap east (1133)", 1133, false, true},  {"interior (500)", 500, false, false},
    };
    for (const One &o : ones) {
        g_case = o.name;
        RegionGeom g{};
        CHECK(region_geom(1152, o.region, &g), "geometry");
        CHECK(g.pole == o.pole && g.periodic == o.wrap, "pole %d wrap %d", (int)g.pole, (int)g.periodic);
        check_tables(make({o.region}, {1}));
    }
    g_case = "a region without sst";
    {
        Ctx c = make({500}, {0});
        SlabTables t;
        CHECK(build_slab_tables(c.in(), &t) == SML_OK, "%s", sml_last_error());
        CHECK(t.ring_src.empty() && t.row.empty() && t.sfb.empty() && t.sgrid.empty() && t.sreg.empty(), "not empty");
        check_tables(c);
    }
    g_case = "sst and no sst side by side";
    check_tables(make({0, 1, 23, 24, 500, 501, 1151}, {1, 0, 1, 1, 0, 1, 1}));
    g_case = "the whole 1152 decomposition";
    {
        std::vector<int> all(1152);
        std::vector<char> sst(1152);
        for (int r = 0; r < 1152; ++r) {
            all[r] = r;
            sst[r] = r % 9 != 4;
        }
        check_tables(make(all, sst));
    }
    g_case = "288 regions of 4 x 4 points";
    {
        std::vector<int> all(288);
        std::vector<char> sst(288);
        for (int r = 0; r < 288; ++r) {
            all[r] = r;
            sst[r] = r % 5 != 0;
        }
        Ctx c = make(all, sst, 288);
        CHECK(c.snout == 16, "snout %d", c.snout);
        check_tables(c);
    }

    // ---- the refusals
    refuse("timestep 0", check_slab_cadence(0, 168), "must be a multiple >= 2 of timestep");
    refuse("no multiple", check_slab_cadence(6, 20), "must be a multiple >= 2 of timestep");
    refuse("ratio 1", check_slab_cadence(6, 6), "must be a multiple >= 2 of timestep");
    g_case = "cadences accepted";
    CHECK(check_slab_cadence(6, 168) == SML_OK && check_slab_cadence(6, 12) == SML_OK, "refused");
    SlabTables t;
    const Ctx good = make({0, 1, 500}, {1, 0, 1});
    {
        Ctx c = good;
        c.snum = 288;
        refuse("another decomposition", build_slab_tables(c.in(), &t), "must be ML-only (chunk_speedy 0) over the same 1152");
        c = good;
        c.sncs = 132;
        refuse("a hybrid slab context", build_slab_tables(c.in(), &t), "must be ML-only");
        c = good;
        c.snout = 136;
        refuse("nout", build_slab_tables(c.in(), &t), "predict the sst of the region's 4 points, not 136");
        c = good;
        c.numregions = c.snum = 1000;
        refuse("no decomposition", build_slab_tables(c.in(), &t), "predict the sst of the region's");
        c = good;
        c.sids[1] = 501;
        refuse("another region's slab", build_slab_tables(c.in(), &t), "slab reservoir 1 is not the rank's sst region 500 (local 2)");
        c = good;
        c.sids.pop_back();
        c.sninp.pop_back();
        c.soff.pop_back();
        refuse("a slab missing", build_slab_tables(c.in(), &t), "slab reservoir 1 is not the rank's sst region 500");
        c = good;
        c.sids.push_back(700);
        c.sninp.push_back(7 * 16);
        c.soff.push_back(c.soff.back() + 7 * 16);
        refuse("a slab too many", build_slab_tables(c.in(), &t), "3 slab reservoirs for 2 sst regions");
        c = good;
        c.sninp[1] = 8 * 16;
        refuse("inputs", build_slab_tables(c.in(), &t), "slab reservoir of region 500: 128 inputs, the atmo subset has 112");
        c = good;
        c.soff[2] += 1;
        refuse("offsets", build_slab_tables(c.in(), &t), "the atmo subset has 112");
        c = good;
        c.ids[2] = 1152;
        refuse("no such region", build_slab_tables(c.in(), &t), "1152 is no region of 1152");
        c = good;
        SlabLayoutIn in = c.in();
        in.ids = nullptr;
        refuse("null ids", build_slab_tables(in, &t), "bad argument");
        refuse("null out", build_slab_tables(c.in(), nullptr), "bad argument");
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
