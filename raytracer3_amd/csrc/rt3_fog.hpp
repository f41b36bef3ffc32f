// rt3_fog.hpp -- fog: one axis-aligned box of homogeneous medium with single scattering (rt3_scene_set_medium).  THE
// RULE, stated once: k_fog_segment, k_fog_shadow and self-test op 45 call these functions, tests/ref_fog.py restates them in float64.
// No reference counterpart (the reference renders a vacuum).
//
//   segment      a ray o + s d ends at its hit distance t, or at +inf on a miss.  Per axis with d.k != 0 the slab gives a = (lo.k - o.k) / d.k,
//                b = (hi.k - o.k) / d.k; an axis with d.k == 0 asks lo.k <= o.k <= hi.k and restricts nothing.  [t0, t1] = [max(0, min(a, b) ..),
//                min(t, max(a, b) ..)]; the segment is in the medium when t1 > t0 and t1 is finite.  len = (t1 - t0) |d|.
//   attenuation  T.c *= expf(-(sigma_t.c len)), sigma_t = sigma_a + sigma_s (fp32 sum, made once by rt3_scene_set_medium).
//   point        sb = (sigma_t.r + sigma_t.g + sigma_t.b) / 3, a = sb len.  One uniform draw u in [0, 1):
//                a >= 2^-23:  E = -expm1f(-a), ds = min(-log1pf(-(u E)) / sb, len), pdf = sb expf(-(sb ds)) / E   (per unit length)
//                otherwise:   ds = u len, pdf = 1 / len                                              (below the grid of u: the uniform density)
//                s = t0 + ds / |d|, x = o + s d.
//   phase        p_HG(c) = (1 - g^2) / (4 pi (1 + g^2 - 2 g c)^(3/2)), c = dot(d, w_l) / |d|, w_l the unit direction towards the light.
//   contribution T_before expf(-(sigma_t ds)) sigma_s / pdf  x  p_HG  x  L_e / pdf_light  x  expf(-(sigma_t len_shadow)), len_shadow the length
//                of the shadow ray x + r w_l, r in [0, tmax], inside the box (the same segment rule, from x).  No MIS: weight 1.
//   light sample every queued shadow ray of a surface vertex has its contribution multiplied by expf(-(sigma_t len_shadow)) the same way.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rt3_emit_tex.hpp"
#include "rt3_math.hpp"
#include "rt3_surface.hpp"

namespace rt3 {

// the fog draws' RNG indices: kFogRngBase + 8 ((sample B) + segment) + dim, between the roulette draws' (0x60000000) and the camera's
// (0x80000000); dim 0 the distance, 3 and 4 the sky sample, 5, 6, 7 the light table's pick and point (k_shade's places); no blue-noise shift
constexpr uint32_t kFogRngBase = 0x70000000u;
constexpr uint32_t kFogRngDims = 8u;
constexpr float kFogUniformBelow = 0x1p-23f;  // a = sb len below the grid of uniform_float: the uniform density

// == rt3_medium as the kernels read it
struct FogDev {
    float sigma_t[3];  // sigma_a + sigma_s
    float sigma_s[3];
    float g;
    float lo[3], hi[3];
};

RT3_DEV bool fog_axis(float o, float d, float lo, float hi, float& t0, float& t1) {
    if (d == 0.0f) return o >= lo && o <= hi;
    const float a = (lo - o) / d, b = (hi - o) / d;
    const float nr = a < b ? a : b, fr = a > b ? a : b;
    t0 = t0 > nr ? t0 : nr;
    t1 = t1 < fr ? t1 : fr;
    return true;
}
// the part [t0, t1] of the ray o + s d, s in [0, t_end], inside the box; false: none (t0, t1 then hold no meaning)
RT3_DEV bool fog_span(V3 o, V3 d, float t_end, const FogDev& f, float& t0, float& t1) {
    t0 = 0.0f;
    t1 = t_end;
    if (!fog_axis(o.x, d.x, f.lo[0], f.hi[0], t0, t1)) return false;
    if (!fog_axis(o.y, d.y, f.lo[1], f.hi[1], t0, t1)) return false;
    if (!fog_axis(o.z, d.z, f.lo[2], f.hi[2], t0, t1)) return false;
    return t1 > t0 && t1 <= kFloatMax;
}
RT3_DEV V3 fog_transmittance(const FogDev& f, float len) {
    return v3(expf(-(f.sigma_t[0] * len)), expf(-(f.sigma_t[1] * len)), expf(-(f.sigma_t[2] * len)));
}
RT3_DEV float fog_sigma_bar(const FogDev& f) { return (f.sigma_t[0] + f.sigma_t[1] + f.sigma_t[2]) / 3.0f; }
struct FogPoint {
    float ds;   // distance from the segment's start, in world units
    float pdf;  // per unit length
};
RT3_DEV FogPoint fog_sample_distance(float sb, float len, float u) {
    FogPoint p;
    const float a = sb * len;
    if (a >= kFogUniformBelow) {
        const float E = -expm1f(-a);
        const float ds = -log1pf(-(u * E)) / sb;
        p.ds = ds < len ? ds : len;
        p.pdf = sb * expf(-(sb * p.ds)) / E;
    } else {
        p.ds = u * len;
        p.pdf = 1.0f / len;
    }
    return p;
}
RT3_DEV float fog_phase(float g, float c) {
    const float den = (1.0f + g * g) - (2.0f * g) * c;
    return (1.0f - g * g) / ((4.0f * kPi) * (den * sqrtf(den)));
}
// expf(-(sigma_t len)) of the shadow ray x + r w, r in [0, tmax]; 1 where it does not meet the box
RT3_DEV V3 fog_shadow_transmittance(const FogDev& f, V3 x, V3 w, float tmax) {
    float t0, t1;
    if (!fog_span(x, w, tmax, f, t0, t1)) return v3(1.0f, 1.0f, 1.0f);
    return fog_transmittance(f, (t1 - t0) * sqrtf(dot(w, w)));
}

// One k_fog_segment launch over the extension queue k_extend has just traced (`rays`, `hits`, `T`; *count records, `stride` per plane):
// every record's throughput is attenuated in place; with `scatter` a record whose segment runs through the medium draws one point on it
// and appends at most one shadow ray to each of the two queues q[0] (the sky sample, when `sky`) and q[1] (the light table's, when
// lights.n != 0), in the emitter shadow queue's layout: {x, c.r} {w_l, c.g} x q_stride, {c.b, path id}, tmax.
struct FogSegmentLaunch {
    FogDev fog;
    SceneDev sc;
    LightsDev lights;
    const EmitTexDev* emit_tex;  // the table's side array, or null
    const float* rays;
    const float* hits;
    float* T;
    const uint32_t* count;
    size_t stride;
    // the camera segment of a frame whose escaped samples took the sky in k_lens_miss (throughput 1, before this launch): the radiance slots
    // of the records that missed are attenuated here; null otherwise
    float* lacc_miss;
    uint32_t scatter, sky;
    float* q_rays[2];
    float* q_contrib[2];
    float* q_tmax[2];
    uint32_t* q_count[2];
    size_t q_stride;
    const uint32_t* pixels;  // x | y << 16; path id = sample_in_batch * npix + pixel index
    uint32_t npix;
    FastDiv npix_div;
    uint32_t s0, bounces, segment, frame;
    unsigned long long* info;  // {segments in the medium, shadow rays queued}: rt3_medium_info
};
// One k_fog_shadow launch over a shadow queue k_shade wrote ({o, c.r} {d, c.g} x stride, {c.b, path id}; tmax null: the sky queue, whose
// rays run to the box's exit): the three contribution words of every ray are multiplied by the medium's transmittance along it.
struct FogShadowLaunch {
    FogDev fog;
    float* rays;
    float* contrib;
    const float* tmax;
    const uint32_t* count;
    size_t stride;
};

}  // namespace rt3
