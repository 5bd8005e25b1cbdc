// reservoir_members_check.cpp -- member_shape (csrc/sml_reservoir_layout.cpp): the tiles
// the ensemble-members kernels run with, against the definition with its numbers written
// out.  Stand-alone, no HIP: built plain and with ASan/UBSan by
// tests/test_reservoir_members_cpu.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>

#include "sml_reservoir_layout.hpp"

using namespace sml;

static int g_fail = 0, g_checks = 0;
#define CHECK(cond, ...)                                    \
    do {                                                    \
        ++g_checks;                                         \
        if (!(cond)) {                                      \
            ++g_fail;                                       \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                       \
            std::printf("\n");                              \
        }                                                   \
    } while (0)

// the definition, spelt out on its own: T members per tile at most, the staged update
// also bounded by the tiles that fit the device's LDS per workgroup
static MemberShape plain(int members, size_t lds_region, bool region_lds, size_t max_lds, int T) {
    MemberShape m;
    m.update_lds = region_lds;
    int tile = members < T ? members : T;
    if (region_lds && lds_region > 0) {
        const size_t fit = max_lds / lds_region;
        if (fit < (size_t)tile) tile = (int)fit;
    }
    m.update_tile = tile;
    m.lds = region_lds ? (size_t)tile * lds_region : 0;
    m.readout_tile = members < T ? members : T;
    m.readout_streams = 0;
    for (int e = 0; e < members; e += m.readout_tile) ++m.readout_streams;
    return m;
}

static void same(const MemberShape &a, const MemberShape &b, const char *what, int members, size_t lds_region,
                 bool region_lds, size_t max_lds) {
    CHECK(a.update_tile == b.update_tile && a.update_lds == b.update_lds && a.lds == b.lds &&
              a.readout_tile == b.readout_tile && a.readout_streams == b.readout_streams,
          "%s: members %d lds_region %zu region_lds %d max_lds %zu: got (%d, %d, %zu, %d, %d) want (%d, %d, %zu, %d, %d)",
          what, members, lds_region, (int)region_lds, max_lds, a.update_tile, (int)a.update_lds, a.lds, a.readout_tile,
          a.readout_streams, b.update_tile, (int)b.update_lds, b.lds, b.readout_tile, b.readout_streams);
}

static void expect(int members, size_t lds_region, bool region_lds, size_t max_lds, int update_tile, size_t lds,
                   int readout_tile, int readout_streams) {
    const MemberShape m = member_shape({members, lds_region, region_lds, max_lds});
    const MemberShape want{update_tile, region_lds, lds, readout_tile, readout_streams};
    same(m, want, "written out", members, lds_region, region_lds, max_lds);
    same(m, plain(members, lds_region, region_lds, max_lds, kMemberTile), "plain", members, lds_region, region_lds,
         max_lds);
}

int main() {
    const int T = kMemberTile;
    CHECK(T == 2 || T == 4, "kMemberTile %d", T);
    CHECK(kMaxMembers == 32, "kMaxMembers %d", kMaxMembers);
    const size_t k64 = 65536, k160 = 163840;
    // --- members 1, 2, T - 1, T, T + 1, 32 on a small staged region (8 KiB: no LDS bound)
    const size_t small = 8192;
    expect(1, small, true, k160, 1, small, 1, 1);
    expect(2, small, true, k160, 2, 2 * small, 2, 1);
    expect(T - 1, small, true, k160, T - 1, (size_t)(T - 1) * small, T - 1, 1);
    expect(T, small, true, k160, T, (size_t)T * small, T, 1);
    expect(T + 1, small, true, k160, T, (size_t)T * small, T, 2);
    expect(32, small, true, k160, T, (size_t)T * small, T, 32 / T);
    expect(32, small, true, k64, T, (size_t)T * small, T, 32 / T);
    // --- the LDS bound: lds_region such that exactly f members fit max_lds, and 8 bytes over
    for (size_t max_lds : {k64, k160}) {
        for (int f = 1; f <= 3; ++f) {
            const size_t fits = max_lds / f / 8 * 8;  // the largest multiple of 8 with f * fits <= max_lds
            if (fits > kRegionLdsMax) continue;     // (not a staged region: step_shape gathers instead)
            CHECK((size_t)f * fits <= max_lds && (size_t)(f + 1) * fits > max_lds, "fits %zu f %d", fits, f);
            const int tile = std::min(f, T);
            expect(32, fits, true, max_lds, tile, (size_t)tile * fits, T, 32 / T);
            const size_t over = fits + 8;
            if (over > kRegionLdsMax) continue;
            const int fo = (int)(max_lds / over), tile_o = std::min(fo, T);
            CHECK(fo == f - 1 || (size_t)f * over <= max_lds, "over %zu f %d fo %d", over, f, fo);
            expect(32, over, true, max_lds, tile_o, (size_t)tile_o * over, T, 32 / T);
        }
    }
    // the numbers of the bound themselves
    expect(32, 65536, true, k64, 1, 65536, T, 32 / T);              // one member fills 64 KiB
    expect(32, 65536, true, k160, 2, 131072, T, 32 / T);            // two fit 160 KiB, three do not
    expect(32, 54608, true, k160, std::min(3, T), (size_t)std::min(3, T) * 54608, T, 32 / T);  // 3 x 54608 = 163824
    expect(32, 54616, true, k160, 2, 2 * 54616, T, 32 / T);         // 3 x 54616 = 163848: 8 bytes over
    expect(32, 32768, true, k64, 2, 65536, T, 32 / T);              // two fill 64 KiB
    expect(32, 32776, true, k64, 1, 32776, T, 32 / T);              // 8 bytes over: one
    expect(32, 21840, true, k64, std::min(3, T), (size_t)std::min(3, T) * 21840, T, 32 / T);  // 3 x 21840 = 65520
    expect(32, 21848, true, k64, 2, 2 * 21848, T, 32 / T);          // 3 x 21848 = 65544
    expect(2, 65536, true, k160, 2, 131072, 2, 1);                  // capped by the members
    expect(1, 65536, true, k160, 1, 65536, 1, 1);
    // --- no staging: the tile is min(members, T) whatever the region's size, no LDS
    expect(1, 70000, false, k160, 1, 0, 1, 1);
    expect(3, 70000, false, k160, std::min(3, T), 0, std::min(3, T), 3 <= T ? 1 : 2);
    expect(32, 600000, false, k64, T, 0, T, 32 / T);
    // --- an empty context (no region: nothing staged, no bound)
    expect(2, 0, true, k160, 2, 0, 2, 1);
    // --- readout_streams at E = T, T + 1, 2 T, 2 T + 1
    expect(T, small, false, k160, T, 0, T, 1);
    expect(T + 1, small, false, k160, T, 0, T, 2);
    expect(2 * T, small, false, k160, T, 0, T, 2);
    expect(2 * T + 1, small, false, k160, T, 0, T, 3);
    // --- random inputs against the plain predicate
    std::mt19937_64 rng(20240607);
    for (int it = 0; it < 4000; ++it) {
        const int members = 1 + (int)(rng() % kMaxMembers);
        const size_t max_lds = rng() % 2 ? k64 : k160;
        const bool staged = rng() % 4 != 0;
        size_t lds_region = 8 * (1 + rng() % (staged ? kRegionLdsMax / 8 : 100000));
        if (rng() % 8 == 0) lds_region = max_lds / (1 + rng() % 4) / 8 * 8 + 8 * (rng() % 2);  // at an edge
        if (staged && lds_region > kRegionLdsMax) lds_region = kRegionLdsMax;
        const MemberShape m = member_shape({members, lds_region, staged, max_lds});
        same(m, plain(members, lds_region, staged, max_lds, kMemberTile), "random", members, lds_region, staged,
             max_lds);
        CHECK(m.update_tile >= 1 && m.update_tile <= kMemberTile && m.lds <= max_lds, "random: tile %d lds %zu",
              m.update_tile, m.lds);
        CHECK(m.readout_tile * m.readout_streams >= members && m.readout_tile * (m.readout_streams - 1) < members,
              "random: streams %d of %d cover %d", m.readout_streams, m.readout_tile, members);
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail != 0;
}
