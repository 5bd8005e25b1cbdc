// sml_counter_rng.hpp -- the library's counter-based generator, for the host and the
// device: every number is a pure function of (seed, region, stream, index).
//
//   mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;
//            z ^= z >> 27;  z *= 0x94D049BB133111EB;
//            z ^= z >> 31                                  (64-bit, wrapping)
//   key(stream)  = mix(mix(seed + 0x9E3779B97F4A7C15) ^ (8 * region + stream))
//   draw(stream, index) = mix(key(stream) + (index + 1) * 0x9E3779B97F4A7C15)
//
// Streams 0..3 are the reservoir generation's (sml_genres.cpp: rows, cols, vals, W_in);
// streams 4 and 5 the input noise's two uniforms (sml_res_noise.hpp):
//   index = (t << 20) | e     t the block's absolute 0-based step, e the region's 0-based
//                             feedback entry; e < 2^20 and 0 <= t < 2^43
//   b1 = draw(4, index) >> 11,  u1 = (b1 + 1) * 2^-53  in (0, 1]
//   b2 = draw(5, index) >> 11,  u2 = b2 * 2^-53        in [0, 1)
// Integer arithmetic and exact fp64 products only: the same bits on the host and the device.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SML_HD __host__ __device__
#else
#define SML_HD
#endif

namespace sml {

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
constexpr int kNoiseStreamU1 = 4, kNoiseStreamU2 = 5;
constexpr int kNoiseEntryBits = 20;                                // e < 2^20
constexpr int64_t kNoiseEntryMax = (int64_t)1 << kNoiseEntryBits;  // ninp below this
constexpr int64_t kNoiseStepMax = (int64_t)1 << (63 - kNoiseEntryBits);  // t below 2^43

SML_HD inline uint64_t mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

SML_HD inline uint64_t stream_key(uint64_t seed, int region, int stream) {
    return mix(mix(seed + kGolden) ^ (8ull * (uint64_t)region + (uint64_t)stream));
}

SML_HD inline uint64_t draw(uint64_t key, uint64_t index) { return mix(key + (index + 1) * kGolden); }

// the noise's index of (step t, entry e); false where either is out of range
SML_HD inline bool noise_index(int64_t t, int64_t e, uint64_t *index) {
    if (t < 0 || t >= kNoiseStepMax || e < 0 || e >= kNoiseEntryMax) return false;
    *index = ((uint64_t)t << kNoiseEntryBits) | (uint64_t)e;
    return true;
}

SML_HD inline uint64_t noise_bits(uint64_t key, uint64_t index) { return draw(key, index) >> 11; }  // 53 bits

// (b + 1 <= 2^53 and b < 2^53 are exact in fp64, and so are their products with 2^-53)
SML_HD inline double noise_u1(uint64_t b1) { return (double)(b1 + 1) * 0x1p-53; }  // (0, 1]
SML_HD inline double noise_u2(uint64_t b2) { return (double)b2 * 0x1p-53; }        // [0, 1)

}  // namespace sml
