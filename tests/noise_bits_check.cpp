// noise_bits_check.cpp -- CPU check of the input noise's integer definition
// (speedy-ml-1_amd/csrc/sml_counter_rng.hpp and sml_noise_bits in sml_genres.cpp): the index
// packing, the refusals and the two uniforms' ranges, against the definition written out here.
// Stand-alone (tests/test_input_noise_cpu.py builds it plain and under ASan/UBSan).
#include <cstdint>
#include <cstdio>

#include "sml_counter_rng.hpp"
#include "sml_internal.hpp"

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

// the definition, restated
static uint64_t r_mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
static uint64_t r_bits(uint64_t seed, int region, int stream, int64_t t, int64_t e) {
    const uint64_t golden = 0x9E3779B97F4A7C15ull;
    const uint64_t key = r_mix(r_mix(seed + golden) ^ (8ull * (uint64_t)region + (uint64_t)stream));
    const uint64_t index = ((uint64_t)t << 20) | (uint64_t)e;
    return r_mix(key + (index + 1) * golden) >> 11;
}

int main() {
    const int64_t tmax = ((int64_t)1 << 43) - 1, emax = ((int64_t)1 << 20) - 1;
    // ---- the index packing: t above bit 20, e below, no overlap at the corners
    uint64_t idx = 0;
    CHECK(sml::noise_index(0, 0, &idx) && idx == 0, "index(0, 0) = %llu", (unsigned long long)idx);
    CHECK(sml::noise_index(1, 0, &idx) && idx == (1ull << 20), "index(1, 0)");
    CHECK(sml::noise_index(0, emax, &idx) && idx == (1ull << 20) - 1, "index(0, emax)");
    CHECK(sml::noise_index(tmax, emax, &idx) && idx == 0x7FFFFFFFFFFFFFFFull, "index(tmax, emax) = %llx",
          (unsigned long long)idx);
    CHECK(sml::noise_index(5, 7, &idx) && idx == ((5ull << 20) | 7ull), "index(5, 7)");
    // ---- the refusals, of the header and of the ABI call
    uint64_t b1 = 0, b2 = 0;
    const int64_t bad_t[] = {-1, tmax + 1, INT64_MAX, INT64_MIN}, bad_e[] = {-1, emax + 1, INT64_MAX, INT64_MIN};
    for (int64_t t : bad_t) {
        CHECK(!sml::noise_index(t, 0, &idx), "t = %lld accepted", (long long)t);
        CHECK(sml_noise_bits(1, 0, t, 0, &b1, &b2) == SML_ERR_ARG, "sml_noise_bits t = %lld", (long long)t);
    }
    for (int64_t e : bad_e) {
        CHECK(!sml::noise_index(0, e, &idx), "e = %lld accepted", (long long)e);
        CHECK(sml_noise_bits(1, 0, 0, e, &b1, &b2) == SML_ERR_ARG, "sml_noise_bits e = %lld", (long long)e);
    }
    CHECK(sml_noise_bits(1, -1, 0, 0, &b1, &b2) == SML_ERR_ARG, "region -1");
    CHECK(sml_noise_bits(1, 0, 0, 0, nullptr, &b2) == SML_ERR_ARG, "null b1");
    CHECK(sml_noise_bits(1, 0, 0, 0, &b1, nullptr) == SML_ERR_ARG, "null b2");
    // ---- the bits against the restatement, corners and a sweep
    const uint64_t seeds[] = {0ull, 0xFFFFFFFFFFFFFFFFull, 0x0123456789ABCDEFull};
    const int regions[] = {0, 1151, 245};
    const int64_t ts[] = {0, 1, 77, tmax}, es[] = {0, 1, 419, emax};
    for (uint64_t seed : seeds)
        for (int region : regions)
            for (int64_t t : ts)
                for (int64_t e : es) {
                    CHECK(sml_noise_bits(seed, region, t, e, &b1, &b2) == SML_OK, "sml_noise_bits");
                    CHECK(b1 == r_bits(seed, region, 4, t, e) && b2 == r_bits(seed, region, 5, t, e),
                          "bits of seed %llx region %d t %lld e %lld", (unsigned long long)seed, region, (long long)t,
                          (long long)e);
                    CHECK(b1 < (1ull << 53) && b2 < (1ull << 53), "53 bits");
                    const double u1 = sml::noise_u1(b1), u2 = sml::noise_u2(b2);
                    CHECK(u1 > 0.0 && u1 <= 1.0 && u2 >= 0.0 && u2 < 1.0, "u1 = %a u2 = %a", u1, u2);
                }
    // ---- the uniforms' ranges at the ends of the 53 bits, exact
    const uint64_t top = (1ull << 53) - 1;
    CHECK(sml::noise_u1(0) == 0x1p-53 && sml::noise_u1(0) > 0.0, "u1(0) = %a", sml::noise_u1(0));
    CHECK(sml::noise_u1(top) == 1.0, "u1(2^53 - 1) = %a", sml::noise_u1(top));
    CHECK(sml::noise_u2(0) == 0.0, "u2(0) = %a", sml::noise_u2(0));
    CHECK(sml::noise_u2(top) == 1.0 - 0x1p-53 && sml::noise_u2(top) < 1.0, "u2(2^53 - 1) = %a", sml::noise_u2(top));
    CHECK(sml::noise_u1(12345) - sml::noise_u2(12345) == 0x1p-53, "u1(b) - u2(b) = 2^-53");
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
