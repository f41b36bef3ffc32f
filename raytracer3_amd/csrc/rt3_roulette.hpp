// rt3_roulette.hpp -- Russian roulette on extension rays (rt3_path_set_roulette): the rule k_roulette applies to one
// record of the extension queue, and that kernel's argument.  No reference counterpart (refrence_mode.slang traces every path to the end).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rt3_math.hpp"
#include "rt3_rng.hpp"

namespace rt3 {

// the first RNG index of the roulette draws: 0x60000000 + s B + b for the extension ray that sample s (absolute index) emitted at bounce b.
// With s B 8 <= 2^30 (the host refuses more) the range ends below 0x68000000: above the glass draws (from 0x40000000, 2 s B of them), below
// the camera's (from 0x80000000).
constexpr uint32_t kRouletteRngBase = 0x60000000u;

// max(r, g, b) that hands a NaN on, whichever component holds it: !(m > 0) then ends a path with a NaN throughput
RT3_DEV float roulette_max(V3 T) {
    auto mx = [](float a, float b) { return (a > b || a != a) ? a : b; };
    return mx(mx(T.x, T.y), T.z);
}
// The survival probability of a record with m = roulette_max(T) > 0, on uniform_float's grid: q = min(1, max(m, min_survival)) rounded up to a
// multiple of 2^-23 (both scalings are exact), so that u < q <=> u < q_g and P(u < q_g) = q_g exactly.  1: the record survives, no draw.
RT3_DEV float roulette_qg(float m, float min_survival) {
    const float q = fmin_sel(1.0f, fmax_sel(m, min_survival));
    return q >= 1.0f ? 1.0f : ceilf(q * 8388608.0f) * 1.1920928955078125e-7f;
}
struct RouletteOutcome {
    bool survive;
    float qg;  // 0: the throughput was not positive, nothing was drawn
    V3 T;      // a survivor's throughput T / q_g (T itself, bit for bit, when q_g = 1); zeros for an ended record
};
// u is read only when 0 < q_g < 1
RT3_DEV RouletteOutcome roulette_rule(V3 T, float min_survival, float u) {
    RouletteOutcome r;
    r.survive = false;
    r.qg = 0.0f;
    r.T = v3(0.0f, 0.0f, 0.0f);
    const float m = roulette_max(T);
    if (!(m > 0.0f)) return r;
    r.qg = roulette_qg(m, min_survival);
    if (r.qg >= 1.0f) {
        r.survive = true;
        r.T = T;
    } else if (u < r.qg) {
        r.survive = true;
        r.T = v3(T.x / r.qg, T.y / r.qg, T.z / r.qg);
    }
    return r;
}

// One k_roulette launch: the extension queue k_shade of bounce `bounce` wrote (`in_*`, its length in *in_count) is compacted into the free
// half of the ping-pong pair (`out_*`), whose length *out_count (zero before the launch) receives.  Both queues have `stride` records.
struct RouletteLaunch {
    const float* in_rays;   // {o, pdf} x stride, {d, path id} x stride
    const float* in_T;      // three planes of stride floats
    const uint32_t* in_count;
    float* out_rays;
    float* out_T;
    uint32_t* out_count;
    size_t stride;
    const uint32_t* pixels;  // x | y << 16; path id = sample_in_batch * npix + pixel index
    uint32_t npix;
    FastDiv npix_div;
    uint32_t s0;             // first sample index of the batch
    uint32_t bounces, bounce, frame;
    float min_survival;
};

}  // namespace rt3
