// reservoir_members_split_check.cpp -- member_finish (csrc/sml_reservoir_layout.cpp): the
// tile of the members' grid finish (k_res_finish_grid_mem), against the definition with its
// numbers written out.  Stand-alone, no HIP: built plain and with ASan/UBSan by
// tests/test_reservoir_members_split_cpu.py.
#include <cstdint>
#include <cstdio>
#include <random>

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

// one member's LDS in a block of the finish: slm [256] and red [7][144] doubles
static const size_t kPerMember = (256 + 7 * 144) * 8;

// the definition, spelt out: the cap is `want` where it names a tile, else the build's
static void plain(int members, int want, int *tile, int *tiles, bool *looped, size_t *lds) {
    int cap = kFinTile;
    if (want >= 1 && want <= kFinTileMax) cap = want;
    *tile = members < cap ? members : cap;
    if (*tile < 1) *tile = 1;
    *tiles = 0;
    for (int e = 0; e < (members > 1 ? members : 1); e += *tile) ++*tiles;
    *looped = *tile == 1 && members > 1;
    *lds = (size_t)*tile * kPerMember;
}

static void expect(int members, int want) {
    int tile, tiles;
    bool looped;
    size_t lds;
    plain(members, want, &tile, &tiles, &looped, &lds);
    const MemberFinish f = want ? member_finish(members, want) : member_finish(members);
    CHECK(f.tile == tile && f.tiles == tiles && f.looped == looped && f.lds == lds,
          "members %d want %d: got (%d, %d, %d, %zu) want (%d, %d, %d, %zu)", members, want, f.tile, f.tiles,
          (int)f.looped, f.lds, tile, tiles, (int)looped, lds);
    CHECK(f.tile >= 1 && f.tile <= kFinTileMax && f.tile <= (members > 1 ? members : 1), "members %d want %d: tile %d",
          members, want, f.tile);
    CHECK(f.tile * f.tiles >= members && f.tile * (f.tiles - 1) < (members > 1 ? members : 1),
          "members %d want %d: %d tiles of %d", members, want, f.tiles, f.tile);
    CHECK(f.lds <= 65536, "members %d want %d: %zu bytes of LDS", members, want, f.lds);  // static LDS: 64 KiB
}

int main() {
    CHECK(kFinTileMax == 4, "kFinTileMax %d", kFinTileMax);
    CHECK(kFinTile >= 1 && kFinTile <= kFinTileMax, "kFinTile %d", kFinTile);
    CHECK(kMaxNcs == 256 && kFinGroups == 7 && kFinOutMax == 144, "the finish's bounds %d %d %d", kMaxNcs, kFinGroups,
          kFinOutMax);
    CHECK(kPerMember == 10112, "one member's LDS %zu", kPerMember);
    // the numbers themselves, for a tile of 1, 2 and 4 chosen by `want`
    {
        MemberFinish f = member_finish(1, 4);
        CHECK(f.tile == 1 && f.tiles == 1 && !f.looped && f.lds == 10112, "E 1: (%d, %d, %d, %zu)", f.tile, f.tiles,
              (int)f.looped, f.lds);
        f = member_finish(8, 1);
        CHECK(f.tile == 1 && f.tiles == 8 && f.looped && f.lds == 10112, "E 8 looped: (%d, %d, %d, %zu)", f.tile,
              f.tiles, (int)f.looped, f.lds);
        f = member_finish(3, 2);
        CHECK(f.tile == 2 && f.tiles == 2 && !f.looped && f.lds == 20224, "E 3 TF 2: (%d, %d, %d, %zu)", f.tile, f.tiles,
              (int)f.looped, f.lds);
        f = member_finish(3, 4);
        CHECK(f.tile == 3 && f.tiles == 1 && !f.looped && f.lds == 30336, "E 3 TF 4: (%d, %d, %d, %zu)", f.tile, f.tiles,
              (int)f.looped, f.lds);
        f = member_finish(9, 4);
        CHECK(f.tile == 4 && f.tiles == 3 && !f.looped && f.lds == 40448, "E 9 TF 4: (%d, %d, %d, %zu)", f.tile, f.tiles,
              (int)f.looped, f.lds);
        f = member_finish(32, 4);
        CHECK(f.tile == 4 && f.tiles == 8, "E 32 TF 4: (%d, %d)", f.tile, f.tiles);
    }
    // every E and every choice, the build's tile (0) and out-of-range choices (the build's) included
    for (int members = 1; members <= kMaxMembers; ++members)
        for (int want : {0, 1, 2, 3, 4, 5, -1}) expect(members, want);
    // E on both sides of the build's tile
    const int T = kFinTile;
    for (int members : {T - 1, T, T + 1, 2 * T, 2 * T + 1})
        if (members >= 1) {
            const MemberFinish f = member_finish(members);
            CHECK(f.tile == (members < T ? members : T), "E %d: tile %d", members, f.tile);
            CHECK(f.tiles == (members + f.tile - 1) / f.tile, "E %d: tiles %d", members, f.tiles);
        }
    std::mt19937_64 rng(20240611);
    for (int it = 0; it < 2000; ++it) expect(1 + (int)(rng() % kMaxMembers), (int)(rng() % 7) - 1);
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail != 0;
}
