// rt3_hit.hpp -- intersection: the hit record, the fused dot / cross products and the slab tests.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt3_math.hpp"

namespace rt3 {

// ------------------------------------------------------------------------------------------------ intersection (north_star)
struct Hit {
    float t, u, v;
    uint32_t prim;
};
// Triangle records: 3 x float4 {v0.xyz,v1.x} {v1.yz,v2.xy} {v2.z,prim,cutoff,slot} (alpha mask, 0 0 = opaque: AlphaDev); the watertight two-sided test is tri_test_nb
// (rt3_trace.hip).  Order-independent acceptance: t > tmin && (t < best.t || (t == best.t && prim < best.prim)).
// Dot products use explicit fused multiply-adds in a fixed order (the oracle mirrors them with fmaf).
RT3_DEV float dot_fma(V3 a, V3 b) { return __builtin_fmaf(a.x, b.x, __builtin_fmaf(a.y, b.y, a.z * b.z)); }
RT3_DEV V3 cross_fma(V3 a, V3 b) {
    return V3{__builtin_fmaf(a.y, b.z, -(a.z * b.y)), __builtin_fmaf(a.z, b.x, -(a.x * b.z)), __builtin_fmaf(a.x, b.y, -(a.y * b.x))};
}
RT3_DEV float guarded_inverse(float d) {
    float a = d < 0.0f ? -d : d;
    float g = a < 1e-20f ? (d < 0.0f ? -1e-20f : 1e-20f) : d;
    return 1.0f / g;
}
// slab test of one child box; returns hit and the entry distance
RT3_DEV bool slab_test(V3 bmin, V3 bmax, V3 o, V3 inv, float tmin, float tbest, float& tn_out) {
    float t0 = (bmin.x - o.x) * inv.x, t1 = (bmax.x - o.x) * inv.x;
    float tn = tmin, tf = tbest;
    float lo = t0 < t1 ? t0 : t1, hi = t0 < t1 ? t1 : t0;
    tn = lo > tn ? lo : tn;
    tf = hi < tf ? hi : tf;
    t0 = (bmin.y - o.y) * inv.y;
    t1 = (bmax.y - o.y) * inv.y;
    lo = t0 < t1 ? t0 : t1;
    hi = t0 < t1 ? t1 : t0;
    tn = lo > tn ? lo : tn;
    tf = hi < tf ? hi : tf;
    t0 = (bmin.z - o.z) * inv.z;
    t1 = (bmax.z - o.z) * inv.z;
    lo = t0 < t1 ? t0 : t1;
    hi = t0 < t1 ? t1 : t0;
    tn = lo > tn ? lo : tn;
    tf = hi < tf ? hi : tf;
    tn_out = tn;
    return tn <= tf;
}

// slab test on the hardware min / max / max3 / min3 instructions.  Same values as slab_test up to the sign of a zero
// (no NaN can occur: the inverse direction is guarded and finite), hence the same hit / order decisions.
RT3_DEV bool slab_test_hw(V3 bmin, V3 bmax, V3 o, V3 inv, float tmin, float tbest, float& tn_out) {
    float ax = (bmin.x - o.x) * inv.x, bx = (bmax.x - o.x) * inv.x;
    float ay = (bmin.y - o.y) * inv.y, by = (bmax.y - o.y) * inv.y;
    float az = (bmin.z - o.z) * inv.z, bz = (bmax.z - o.z) * inv.z;
    float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(ax, bx), __builtin_fminf(ay, by)), __builtin_fmaxf(__builtin_fminf(az, bz), tmin));
    float tf = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(ax, bx), __builtin_fmaxf(ay, by)), __builtin_fminf(__builtin_fmaxf(az, bz), tbest));
    tn_out = tn;
    return tn <= tf;
}

// slab test on ray parameters that are already computed (quantised nodes: t = fma(q, step*inv, (org-o)*inv)); arguments are
// (lo, hi) per axis in x, y, z order
RT3_DEV bool slab_test_q(float ax, float bx, float ay, float by, float az, float bz, float tmin, float tbest, float& tn_out) {
    float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(ax, bx), __builtin_fminf(ay, by)), __builtin_fmaxf(__builtin_fminf(az, bz), tmin));
    float tf = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(ax, bx), __builtin_fmaxf(ay, by)), __builtin_fminf(__builtin_fmaxf(az, bz), tbest));
    tn_out = tn;
    return tn <= tf;
}

}  // namespace rt3
