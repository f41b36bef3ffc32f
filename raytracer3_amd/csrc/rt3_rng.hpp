// rt3_rng.hpp -- the counter-based random stream and the blue-noise shift.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt3_math.hpp"

namespace rt3 {

// ------------------------------------------------------------------------------------------------ RNG
// random.slang:5-15
RT3_DEV uint32_t jenkins_hash(uint32_t a) {
    a = (a + 0x7ed55d16u) + (a << 12);
    a = (a ^ 0xc761c23cu) ^ (a >> 19);
    a = (a + 0x165667b1u) + (a << 5);
    a = (a + 0xd3a2646cu) ^ (a << 9);
    a = (a + 0xfd7046c5u) + (a << 3);
    a = (a ^ 0xb55a4f09u) ^ (a >> 16);
    return a;
}
// math.slang:105-117
RT3_DEV uint32_t integer_explode(uint32_t x) {
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}
RT3_DEV uint32_t zcurve(uint32_t x, uint32_t y) { return integer_explode(x) | (integer_explode(y) << 1); }
// random.slang:42-46
RT3_DEV uint32_t rng_seed(uint32_t px, uint32_t py, uint32_t frame) { return jenkins_hash(zcurve(px, py)) + frame; }
// random.slang:49-79, counter passed explicitly (the stream is counter-based; see DESIGN.md for the index rule)
RT3_DEV uint32_t murmur3(uint32_t seed, uint32_t index) {
    uint32_t k = index * 0xcc9e2d51u;
    k = (k << 15) | (k >> 17);
    k *= 0x1b873593u;
    uint32_t h = seed ^ k;
    h = ((h << 13) | (h >> 19)) * 5u + 0xe6546b64u;
    h ^= 4u;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}
// random.slang:82-89
RT3_DEV float uniform_float(uint32_t seed, uint32_t index) {
    return __uint_as_float((murmur3(seed, index) & 0x007FFFFFu) | 0x3F800000u) - 1.0f;
}
// Cranley-Patterson shift by one blue-noise byte (north_star): frac(u + c/256)
RT3_DEV float bluenoise_shift(float u, uint32_t c) {
    float r = u + (float)c * 0.00390625f;
    return r >= 1.0f ? r - 1.0f : r;
}

}  // namespace rt3
