// sml_genres.cpp -- one region's untrained reservoir on the host: makesparse's A
// before gen_res scales it and train_reservoir's W_in.  Host only, no GPU.
//
// Reference: makesparse (src/mod_linalg.f90:180-218) with shuffle
// (src/mod_utilities.f90:1562-1589), the W_in fill of train_reservoir
// (src/mod_reservoir.f90:260-278).  The reference draws from RANDOM_NUMBER seeded by
// system_clock, so its matrices were never reproducible; here every number is a pure
// function of (seed, region, stream, index) -- the generator of sml_counter_rng.hpp, which
// the input noise's kernel shares (streams 4 and 5; sml_noise_bits below is its host form):
//
//   mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;
//            z ^= z >> 27;  z *= 0x94D049BB133111EB;
//            z ^= z >> 31                                  (64-bit, wrapping)
//   key(stream)  = mix(mix(seed + 0x9E3779B97F4A7C15) ^ (8 * region + stream))
//   draw(stream, index) = mix(key(stream) + (index + 1) * 0x9E3779B97F4A7C15)
//
//   stream 0  rows   index = the entry's 0-based position e in rows[k]
//   stream 1  cols   index = e
//   stream 2  vals   index = e
//   stream 3  W_in   index = the 0-based row r
//
// rows / cols: the entries come in blocks of n (k / n full blocks, then k % n picks;
// one partial block when k <= n).  Each block is the first entries of a fresh shuffle
// of 1..n, rows and cols shuffled independently.  shuffle keeps choices[0..n) = 1..n
// and at step j (m = n - j values left) takes
//   t = (hi32(draw) * m) >> 32                (0 <= t < m; hi32 = draw >> 32)
//   out[j] = choices[t];  choices[t] = choices[m - 1];  choices[m - 1] = out[j]
// -- the reference's swap-with-last selection, with its single-precision
// int(a * m) + 1 (which can round to m + 1) replaced by the integer product.
//
// vals[e] = (draw >> 40) * 2^-24: in [0, 1), exact in fp32 and fp64.
// W_in: row r reads input r / q, q = n / ninp; its value is sigma * (2 u - 1) with
// u = ((draw >> 40) + 0.5) * 2^-24 in (0, 1), computed in fp64 and rounded to fp32:
// 2 u - 1 is an odd multiple of 2^-24, never 0.
#include <vector>

#include "sml_counter_rng.hpp"
#include "sml_internal.hpp"

using namespace sml;  // mix, stream_key, draw: sml_counter_rng.hpp, shared with the device

namespace {

// out[0 .. count) = the first `count` entries of a shuffle of 1..n, draws first, first + 1, ...
void shuffle(int n, int count, uint64_t key, uint64_t first, std::vector<int> &choices, int *out) {
    for (int i = 0; i < n; ++i) choices[i] = i + 1;
    for (int j = 0; j < count; ++j) {
        const uint64_t m = (uint64_t)(n - j);
        const int t = (int)(((draw(key, first + (uint64_t)j) >> 32) * m) >> 32);
        const int tmp = choices[t];
        out[j] = tmp;
        choices[t] = choices[m - 1];
        choices[m - 1] = tmp;
    }
}

}  // namespace

extern "C" int sml_gen_region(int n, int k, int ninp, uint64_t seed, int region, double sigma, int *rows, int *cols,
                              float *vals, int *win_col, float *win_val) {
    SML_REQUIRE(n >= 1 && n <= 65535, "sml_gen_region: n = %d outside 1..65535", n);
    SML_REQUIRE(k >= 0, "sml_gen_region: k = %d is negative", k);
    SML_REQUIRE(ninp >= 1 && n % ninp == 0, "sml_gen_region: ninp = %d does not divide n = %d", ninp, n);
    SML_REQUIRE(region >= 0, "sml_gen_region: region = %d is negative", region);
    SML_REQUIRE((k == 0 || (rows && cols && vals)) && win_col && win_val, "sml_gen_region: null output array");
    const uint64_t krow = stream_key(seed, region, 0), kcol = stream_key(seed, region, 1),
                   kval = stream_key(seed, region, 2), kwin = stream_key(seed, region, 3);
    std::vector<int> choices((size_t)n);
    for (int64_t first = 0; first < k; first += n) {
        const int count = (int)(k - first < n ? k - first : n);
        shuffle(n, count, krow, (uint64_t)first, choices, rows + first);
        shuffle(n, count, kcol, (uint64_t)first, choices, cols + first);
    }
    for (int e = 0; e < k; ++e) vals[e] = (float)(draw(kval, (uint64_t)e) >> 40) * 0x1p-24f;
    const int q = n / ninp;
    for (int r = 0; r < n; ++r) {
        const double u = ((double)(draw(kwin, (uint64_t)r) >> 40) + 0.5) * 0x1p-24;
        win_col[r] = r / q;
        win_val[r] = (float)(sigma * (2.0 * u - 1.0));
    }
    return SML_OK;
}

// the two 53-bit integers the input noise draws for step t, entry e of noise region `region`
// (sml_res_input_noise): host only, the device's own functions
extern "C" int sml_noise_bits(uint64_t seed, int region, int64_t t, int64_t e, uint64_t *b1, uint64_t *b2) {
    SML_REQUIRE(region >= 0, "sml_noise_bits: region = %d is negative", region);
    SML_REQUIRE(b1 && b2, "sml_noise_bits: null output");
    uint64_t index;
    SML_REQUIRE(noise_index(t, e, &index), "sml_noise_bits: t = %lld outside [0, 2^43) or e = %lld outside [0, 2^20)",
                (long long)t, (long long)e);
    *b1 = noise_bits(stream_key(seed, region, kNoiseStreamU1), index);
    *b2 = noise_bits(stream_key(seed, region, kNoiseStreamU2), index);
    return SML_OK;
}
