// series_layout_check.cpp -- CPU check of the series tables of the reservoir context's
// layout unit (build_series_tables, series_split: speedy-ml-1_amd/csrc/sml_reservoir_layout.cpp):
// every entry is compared with its plain definition, written out here from the regions'
// geometry and the documented feedback layout
//     [atmo(4, inx, iny, 8) | logp(inx, iny) | precip(inx, iny) | sst(inx, iny)? | tisr(inx, iny)]
// without the unit's own index code.  Stand-alone (tests/test_series_layout_cpu.py builds it
// plain and under ASan/UBSan).
#include <cstdio>
#include <string>
#include <vector>

#include "sml_reservoir_layout.hpp"

using namespace sml;

static int g_fail = 0, g_checks = 0;
#define CHECK(cond, ...)                                                 \
    do {                                                                 \
        ++g_checks;                                                      \
        if (!(cond)) {                                                   \
            if (++g_fail <= 40) {                                        \
                std::printf("FAIL %s:%d %s -- ", __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                                \
                std::printf("\n");                                       \
            }                                                            \
        }                                                                \
    } while (0)

struct Reg {
    int id;
    bool sst;
};

// 0-based global column of 0-based local column lx: in_xstart onwards, wrapping past 96
static int wrap_x(const RegionGeom &g, int lx) { return (g.in_xstart - 1 + lx) % kXGrid; }

static void check_context(int numregions, const std::vector<Reg> &regs) {
    const int nlocal = (int)regs.size();
    std::vector<RegionGeom> geom(nlocal);
    std::vector<unsigned char> sst(nlocal);
    std::vector<int> ninp(nlocal), n(nlocal, 64), k(nlocal, 128);
    for (int i = 0; i < nlocal; ++i) {
        CHECK(region_geom(numregions, regs[i].id, &geom[i]), "region %d", regs[i].id);
        sst[i] = regs[i].sst;
        ninp[i] = region_ninp(geom[i], regs[i].sst);
    }
    const int resxy = geom[0].resx * geom[0].resy, ncs = 33 * resxy, nout = 34 * resxy;
    const PoolPlan plan = plan_pools({nlocal, n.data(), k.data(), ninp.data(), ncs, (nout + kRows - 1) / kRows * kRows, false});
    const TablesIn in{numregions, nlocal, ncs, nout, geom.data(), sst.data(), ninp.data(), plan.rd.data(), plan.tot_fb, nullptr};
    SeriesTables t;
    CHECK(build_series_tables(in, &t) == SML_OK, "build_series_tables");
    RegionTables rt;
    CHECK(build_region_tables(in, &rt) == SML_OK, "build_region_tables");
    CHECK((int64_t)t.src.size() == plan.tot_fb && (int64_t)t.l.size() == plan.tot_fb, "sizes");
    CHECK((int)t.pt_off.size() == nlocal + 1 && t.pt_off[0] == 0, "pt_off size");
    for (int i = 0; i < nlocal; ++i) {
        const RegionGeom &g = geom[i];
        const int in2d = g.inx * g.iny;
        const int64_t base = plan.rd[i].fb;
        CHECK(t.pt_off[i + 1] - t.pt_off[i] == in2d, "region %d: %d points", regs[i].id, t.pt_off[i + 1] - t.pt_off[i]);
        // the pole clips the halo, the row's ends wrap it
        CHECK(g.in_ystart >= 1 && g.in_ystart + g.iny - 1 <= kYGrid, "region %d rows", regs[i].id);
        int64_t e = base;
        for (int z = 0; z < kZGrid; ++z)
            for (int ly = 0; ly < g.iny; ++ly)
                for (int lx = 0; lx < g.inx; ++lx)
                    for (int v = 0; v < kVars; ++v, ++e) {
                        const int x = wrap_x(g, lx), y = g.in_ystart - 1 + ly;
                        CHECK(t.src[e] == v + 4 * (x + 96 * (y + 48 * z)), "region %d atmo entry %lld", regs[i].id, (long long)(e - base));
                        CHECK(t.l[e] == v * 8 + z, "region %d atmo slot %lld", regs[i].id, (long long)(e - base));
                        // where the single-grid tables hold the entry, they agree
                        CHECK(rt.fb_src[e] == t.src[e] && rt.fb_l[e] == t.l[e], "region %d entry %lld vs fb_src", regs[i].id, (long long)(e - base));
                    }
        const int field[4] = {0, 1, 2, 3}, slot[4] = {32, 34, 35, 33};
        for (int b = 0; b < 4; ++b) {
            if (b == 2 && !regs[i].sst) continue;
            for (int ly = 0; ly < g.iny; ++ly)
                for (int lx = 0; lx < g.inx; ++lx, ++e) {
                    const int x = wrap_x(g, lx), y = g.in_ystart - 1 + ly;
                    CHECK(t.src[e] == 147456 + field[b] * 4608 + x + 96 * y, "region %d block %d point %d", regs[i].id, b, lx + g.inx * ly);
                    CHECK(t.l[e] == slot[b], "region %d block %d slot", regs[i].id, b);
                    if (b == 0) CHECK(t.pt_grid[t.pt_off[i] + lx + g.inx * ly] == x + 96 * y, "region %d point %d", regs[i].id, lx + g.inx * ly);
                    if (b == 2) CHECK(rt.fb_src[e] == kSrcKeep, "region %d: the sst entry is the single-grid tables' kept one", regs[i].id);
                    if (b < 2) CHECK(rt.fb_src[e] == 147456 + b * 4608 + x + 96 * y, "region %d block %d vs fb_src", regs[i].id, b);
                }
        }
        CHECK(e - base == ninp[i], "region %d: %lld entries, ninp %d", regs[i].id, (long long)(e - base), ninp[i]);
        // the tisr entries' points are the single-grid tisr table's
    }
    CHECK(rt.tisr_grid == t.pt_grid, "pt_grid is tisr_grid");
}

int main() {
    // the 1152-region decomposition: both poles, both wraps, interior with and without sst, neighbours
    check_context(1152, {{0, true}, {23, false}, {7, false}, {1135, true}, {1151, false}, {245, true}, {246, false}, {269, true}});
    {
        RegionGeom g;
        region_geom(1152, 0, &g);
        CHECK(g.iny == 3 && g.inx == 4 && g.in_xstart == 96, "region 0: pole and wrap (%d, %d, %d)", g.iny, g.inx, g.in_xstart);
        region_geom(1152, 1135, &g);
        CHECK(g.iny == 4 && g.in_xstart == 94 && g.in_xend == 1, "region 1135: high-end wrap (%d, %d)", g.in_xstart, g.in_xend);
    }
    // every region of a coarser decomposition, sst on the even ones
    for (int nr : {1152, 288, 72}) {
        std::vector<Reg> all;
        for (int r = 0; r < nr; ++r) all.push_back({r, r % 2 == 0});
        check_context(nr, all);
    }
    // the statistics' split: S chunks of at most len steps cover T with none empty, at most
    // kSerSplitMax chunks, one chunk up to kSerChunkMin steps
    for (int T = 1; T <= 5000; ++T) {
        const SeriesSplit s = series_split(T);
        CHECK(s.S >= 1 && s.S <= kSerSplitMax && s.len >= 1, "T %d: S %d len %d", T, s.S, s.len);
        CHECK((int64_t)s.S * s.len >= T && (int64_t)(s.S - 1) * s.len < T, "T %d: S %d len %d", T, s.S, s.len);
        if (T <= kSerChunkMin) CHECK(s.S == 1, "T %d: S %d", T, s.S);
    }
    CHECK(series_split(37).S == 3 && series_split(37).len == 13, "T 37");
    CHECK(series_split(1460).S == 16 && series_split(1460).len == 92, "T 1460");
    std::printf("series_layout_check: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
