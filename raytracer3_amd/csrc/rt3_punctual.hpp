// rt3_punctual.hpp -- the punctual-light function of RT3_F_NEE_PUNCTUAL, shared by k_shade_punct and self-test op 30.
#pragma once
#include <hip/hip_runtime.h>

#include "rt3_math.hpp"

namespace rt3 {

// the shadow ray of a light sample ends this far along its way to the sampled point (an emitter's, RT3_F_NEE_EMISSIVE, or a point or spot
// light): the emitter never occludes itself, another one in front does
constexpr float kEmitShadowEnd = 0.9990234375f;  // 1 - 2^-10

// A punctual record of the light table (64 bytes, the emitter records' size; made by k_punct_records):
//   r0 = {position, p_sel}   r1 = {unit axis, I.r}   r2 = {cone a, cone o, 1 / range or 0, I.g}   r3 = {tag, 0, 0, I.b}
// tag = kPunctTag + type.  A triangle record holds a unit normal (or (0, 0, 1)) in r3.xyz, so r3.x <= 1 < kPunctTag tells the two apart.
// A point light is a spot with a = 0, o = 1: c = clamp(0 + 1) = 1, exactly.
constexpr float kPunctTag = 2.0f;
constexpr float kPunctTagDirectional = 4.0f;  // kPunctTag + RT3_LIGHT_DIRECTIONAL
RT3_DEV bool is_punctual_record(const float4& r3) { return r3.x >= kPunctTag; }

struct PunctualSample {
    V3 wl;       // unit direction to the light
    float tmax;  // the shadow ray's range end
    float cs;    // N . wl
    float geo;   // 1 / d^2 (point, spot) or 1 (directional); 0 = nothing arrives
    V3 Ic;       // I cone window, or E
};
// the light of record (r0 .. r3) seen from x with shading normal N; kEnd = the fraction of the way at which a point light's shadow ray ends
RT3_DEV PunctualSample punctual_sample(const float4& r0, const float4& r1, const float4& r2, const float4& r3, V3 x, V3 N, float kEnd) {
    PunctualSample s;
    const V3 axis = v3(r1.x, r1.y, r1.z), I = v3(r1.w, r2.w, r3.w);
    if (r3.x >= kPunctTagDirectional) {
        s.wl = neg(axis);
        s.tmax = kBackgroundDepth;
        s.cs = dot(N, s.wl);
        s.geo = 1.0f;
        s.Ic = I;
        return s;
    }
    const V3 wv = v3(r0.x - x.x, r0.y - x.y, r0.z - x.z);
    const float d2 = dot(wv, wv), d = sqrtf(d2);
    if (!(d2 > 0.0f)) {
        s.wl = v3(0.0f, 0.0f, 0.0f);
        s.tmax = s.cs = s.geo = 0.0f;
        s.Ic = v3(0.0f, 0.0f, 0.0f);
        return s;
    }
    s.wl = wv * (1.0f / d);
    s.cs = dot(N, s.wl);
    s.tmax = d * kEnd;
    s.geo = 1.0f / d2;
    const float c = fminf(fmaxf(-dot(s.wl, axis) * r2.x + r2.y, 0.0f), 1.0f);
    const float q = d * r2.z, q2 = q * q;
    const float window = fminf(fmaxf(1.0f - q2 * q2, 0.0f), 1.0f);
    const float k = (c * c) * window;
    s.Ic = v3(I.x * k, I.y * k, I.z * k);
    return s;
}

}  // namespace rt3
