// rt3_glass.hpp -- transmissive dielectric surfaces (rt3_scene_set_transmission): the side table of k_shade_glass and
// the one function a glass vertex evaluates.  No reference counterpart (every surface of the reference is DiffuseBrdf under GGX).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt3_bsdf.hpp"
#include "rt3_math.hpp"

namespace rt3 {

// == rt3_transmission, per flattened geometry; the table exists only when some transmission is > 0
struct GlassDev {
    float transmission, ior;
    uint32_t thin_walled, pad;
};
static_assert(sizeof(GlassDev) == 16, "Glass layout");

// The pdf slot of a glass vertex's extension ray.  Both values are delta markers in the sense of rt3_lens.hip's header comment: k_shade's MIS
// weights pdf_b / (pdf_b + p_light) are exactly 1 while p_light stays below half an ulp of the marker (2^103), under the same assumption
// for an emitter seen edge-on.  kFloatMax is the camera's own marker and is handed on by a glass vertex that received it: "nothing but
// glass since the camera", which lets an escaped ray show the sky without RT3_F_NEE_SKY, as k_lens_miss does for a camera ray.  A glass
// vertex reached from an opaque one hands on kGlassDeltaPdf, the next float below.
constexpr float kGlassDeltaPdf = 3.4028232635611926e38f;  // 0x7F7FFFFE
// the first RNG index of the glass draws: 0x40000000 + 2 (s B + b) selects the lobe, + 1 the event
constexpr uint32_t kGlassRngBase = 0x40000000u;

struct GlassEvent {
    uint32_t transmit;  // 0: mirror reflection about n, 1: transmission
    V3 dir;             // unit up to rounding
    float F;            // the reflection probability: exact Fresnel, or F' = 2 F / (1 + F) of a thin slab
};
// A smooth dielectric interface air <-> ior with shading normal n (not face-forwarded), met by a ray of direction d (any length); u picks
// the event.  The ray enters when dot(n, d) < 0: eta = ior, else 1 / ior; thin-walled: eta = ior on both sides, the transmitted direction
// is d's.  cos_t^2 <= 0 is total internal reflection.
RT3_DEV GlassEvent glass_sample(float ior, bool thin, V3 d, V3 n, float u) {
    const float dl = sqrtf(dot(d, d));
    const V3 ud = v3(d.x / dl, d.y / dl, d.z / dl);
    const float c = dot(n, ud);
    const bool enter = c < 0.0f;
    const float cos_i = fabsf(c);
    const float eta = (thin || enter) ? ior : 1.0f / ior;
    // cos_t^2 = 1 - (1 - cos_i^2) / eta^2, written without the cancellation of 1 - (1 - x): at eta = 1 it is cos_i^2 exactly, so an
    // index-matched surface has cos_t = cos_i, F = 0 and hands the unit direction on unchanged
    const float eta2 = eta * eta;
    const float cos_t2 = (cos_i * cos_i + (eta2 - 1.0f)) / eta2;
    float F = 1.0f, cos_t = 0.0f;
    if (cos_t2 > 0.0f) {
        cos_t = sqrtf(cos_t2);
        const float rs = (cos_i - eta * cos_t) / (cos_i + eta * cos_t);
        const float rp = (eta * cos_i - cos_t) / (eta * cos_i + cos_t);
        F = 0.5f * (rs * rs + rp * rp);
    }
    if (thin) F = (2.0f * F) / (1.0f + F);
    GlassEvent e;
    e.F = F;
    if (u < F) {
        const float k = 2.0f * c;
        e.transmit = 0u;
        e.dir = v3(ud.x - k * n.x, ud.y - k * n.y, ud.z - k * n.z);
    } else if (thin) {
        e.transmit = 1u;
        e.dir = ud;
    } else {
        const float k = cos_i / eta - cos_t, sg = enter ? k : -k;  // along n', the normal on the incoming side
        e.transmit = 1u;
        e.dir = v3(ud.x / eta + sg * n.x, ud.y / eta + sg * n.y, ud.z / eta + sg * n.z);
    }
    return e;
}

// Pane shadows (rt3_scene_set_pane_shadows).  GlassDev::pad of a geometry the build classified as a pane:
constexpr uint32_t kGlassPaneBit = 1u;
// 1 - F' of a thin-walled pane of index ior met at cos_i = |n.d| / |d|: glass_sample's Fresnel expression at eta = ior (a pane has the
// same eta on both sides), so that an index-matched pane gives exactly 1.  With the transmission and the tint it is the expectation of
// what a glass vertex there does to the throughput of a path that goes straight on.
RT3_DEV float pane_pass_fraction(float ior, float cos_i) {
    const float eta2 = ior * ior;
    const float cos_t2 = (cos_i * cos_i + (eta2 - 1.0f)) / eta2;
    float F = 1.0f;
    if (cos_t2 > 0.0f) {
        const float cos_t = sqrtf(cos_t2);
        const float rs = (cos_i - ior * cos_t) / (cos_i + ior * cos_t);
        const float rp = (ior * cos_i - cos_t) / (ior * cos_i + cos_t);
        F = 0.5f * (rs * rs + rp * rp);
    }
    return 1.0f - (2.0f * F) / (1.0f + F);
}

// Rough transmission (rt3_scene_set_rough_transmission).  GlassDev::pad of a geometry the build classified as frosted:
constexpr uint32_t kGlassFrostBit = 2u;
// the first RNG index of the micro-normal draws: 0x50000000 + 2 (s B + b) + {0, 1}, behind the glass draws and below roulette's
constexpr uint32_t kFrostRngBase = 0x50000000u;
constexpr float kFrostMinCos = 1e-5f;  // the opaque BSDF's BRDF_SAMPLING_MIN_COS

struct FrostEvent {
    uint32_t event;  // 0: reflection, 1: transmission, 2: invalid (the path ends)
    V3 dir;          // world space, unit up to rounding; the incoming unit direction for an invalid sample
    float F;         // the reflection probability at the micro-normal (0 when the frame itself was invalid)
    float weight;    // G1(|wi.z|, alpha^2): what is left of f cos / pdf; 0 for an invalid sample
};
// A rough dielectric interface: glass_sample's event at a GGX micro-normal m, drawn from the distribution of normals visible from wo
// (sample_vndf, the opaque BSDF's, alpha = roughness > 0).  The frame stands on n_in, the shading normal turned to the incoming side; wo = -d
// in it.  u picks the event as in glass_sample; u2, u3 pick m.  Reflection: r = 2 cos_i m - wo, valid above the macro-surface.  Solid
// transmission: t = -wo / eta + (cos_i / eta - cos_t) m, valid below it.  Thin-walled: r mirrored through the macro-surface -- a thin rough
// slab as one lobe, an approximation.  An invalid sample ends the path (single scattering: that energy is lost).
RT3_DEV FrostEvent frost_sample(float ior, bool thin, V3 d, V3 n, float alpha, float u, float u2, float u3) {
    const float dl = sqrtf(dot(d, d));
    const V3 ud = v3(d.x / dl, d.y / dl, d.z / dl);
    const bool enter = dot(n, ud) < 0.0f;
    const V3 n_in = enter ? n : neg(n);
    V3 b1, b2;
    build_orthonormal_basis(n_in, b1, b2);
    const V3 wo = v3(-(ud.x * b1.x + ud.y * b1.y + ud.z * b1.z), -(ud.x * b2.x + ud.y * b2.y + ud.z * b2.z), -(ud.x * n_in.x + ud.y * n_in.y + ud.z * n_in.z));
    FrostEvent e;
    e.event = 2u;
    e.dir = ud;
    e.F = 0.0f;
    e.weight = 0.0f;
    if (!(wo.z > kFrostMinCos)) return e;
    const V3 m = sample_vndf(alpha, wo, u2, u3);
    const float cos_i = dot(wo, m);
    const float eta = (thin || enter) ? ior : 1.0f / ior;
    const float eta2 = eta * eta;
    const float cos_t2 = (cos_i * cos_i + (eta2 - 1.0f)) / eta2;  // (glass_sample's expressions, at this cos_i)
    float F = 1.0f, cos_t = 0.0f;
    if (cos_t2 > 0.0f) {
        cos_t = sqrtf(cos_t2);
        const float rs = (cos_i - eta * cos_t) / (cos_i + eta * cos_t);
        const float rp = (eta * cos_i - cos_t) / (eta * cos_i + cos_t);
        F = 0.5f * (rs * rs + rp * rp);
    }
    if (thin) F = (2.0f * F) / (1.0f + F);
    e.F = F;
    const float s2 = 2.0f * cos_i;
    const V3 r = v3(s2 * m.x - wo.x, s2 * m.y - wo.y, s2 * m.z - wo.z);
    V3 wi;
    bool ok;
    const bool reflect = u < F;
    if (reflect) {
        wi = r;
        ok = r.z > kFrostMinCos;
    } else if (thin) {
        wi = v3(r.x, r.y, -r.z);
        ok = r.z > kFrostMinCos;
    } else {
        const float k = cos_i / eta - cos_t;
        wi = v3(k * m.x - wo.x / eta, k * m.y - wo.y / eta, k * m.z - wo.z / eta);
        ok = wi.z < -kFrostMinCos;
    }
    if (!ok) return e;
    e.event = reflect ? 0u : 1u;
    e.dir = basis_apply(b1, b2, n_in, wi);
    e.weight = g_smith_ggx1(fabsf(wi.z), alpha * alpha);
    return e;
}

}  // namespace rt3
