// rt3_volume.hpp -- Beer-Lambert absorption inside solid glass (rt3_scene_set_attenuation): the rule k_absorb applies to
// one record of the extension queue, the table entry it reads, and that kernel's argument.  No reference counterpart (the reference has no
// transmissive surfaces).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rt3_math.hpp"
#include "rt3_surface.hpp"

namespace rt3 {

// == rt3_attenuation as the build stores it, per flattened geometry: sigma of an absorbing geometry (transmission > 0, solid, some sigma > 0)
// and absorbing = 1; all zero for every other geometry, whatever the caller uploaded for it.  The table exists only when some geometry is
// absorbing.
struct AbsorbDev {
    float sigma[3];
    uint32_t absorbing;
};
static_assert(sizeof(AbsorbDev) == 16, "Absorb layout");

// The shading normal of a hit as hit_finish makes it for a geometry without a normal map: the three vertex normals of the shading record
// at barycentrics (bu, bv), normalised, through the geometry's matrix unless it is the identity, normalised again.  Not face-forwarded.
RT3_DEV V3 absorb_normal(uint4 rec, float bu, float bv, bool identity, const float* m9) {
    const V3 n0 = octa_decode16(rec.x), n1 = octa_decode16(rec.y), n2 = octa_decode16(rec.z);
    const float b0 = 1.0f - bu - bv;
    V3 n = v3(n0.x * b0 + n1.x * bu + n2.x * bv, n0.y * b0 + n1.y * bu + n2.y * bv, n0.z * b0 + n1.z * bu + n2.z * bv);
    n = normalize(n);
    if (!identity) n = transform_vector(m9, n);
    return normalize(n);
}

struct AbsorbOutcome {
    bool applied;
    V3 T;  // T itself, bit for bit, when not applied
};
// A segment of length t |d| that arrives at a back face (dot(n, d) > 0) of a geometry with some sigma > 0 ran inside it:
// T.c *= expf(-(sigma.c x)), x = t sqrtf(dot(d, d)), in this order.  expf(-0.0f) = 1: a channel with sigma 0 keeps its bits.
RT3_DEV AbsorbOutcome absorb_rule(V3 T, V3 sigma, float t, V3 d, V3 n) {
    AbsorbOutcome r;
    r.applied = (sigma.x > 0.0f || sigma.y > 0.0f || sigma.z > 0.0f) && dot(n, d) > 0.0f;
    r.T = T;
    if (r.applied) {
        const float x = t * sqrtf(dot(d, d));
        r.T = v3(T.x * expf(-(sigma.x * x)), T.y * expf(-(sigma.y * x)), T.z * expf(-(sigma.z * x)));
    }
    return r;
}

// One k_absorb launch: the records of the extension queue k_extend has just traced (`rays`, `hits`, `T`; *count of them, `stride` records per
// plane) get their throughput attenuated in place where the rule applies.  Nothing else is written.
struct AbsorbLaunch {
    const float* rays;   // {o, pdf} x stride, {d, path id} x stride: only the second plane is read
    const float* hits;   // {t, u, v, prim} x stride
    float* T;            // three planes of stride floats
    const uint32_t* count;
    size_t stride;
    const uint4* tri_shade;           // SceneDev::tri_shade
    const ShadeGeomDev* shade_geoms;  // SceneDev::shade_geoms: identity and the matrix's upper 3 x 3
    const AbsorbDev* table;           // per flattened geometry
};

}  // namespace rt3
