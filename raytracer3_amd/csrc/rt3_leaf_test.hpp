// rt3_leaf_test.hpp -- what a ray does at a leaf and at the exit table, shared by the traversal (rt3_trace.hip) and by the shade kernel that
// tries a sky shadow ray's exit-table leaf before it queues the ray (k_shade_defer_exit, rt3_shade.hip): the watertight triangle test and the
// rule that names a ray's exit cell.  One definition each, so that both users decide every ray alike, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt3_glass.hpp"
#include "rt3_hit.hpp"
#include "rt3_internal.hpp"
#include "rt3_math.hpp"
#include "rt3_surface.hpp"

namespace rt3 {

constexpr uint32_t kEmptySlot = 0xFFFFFFFFu;

// Watertight ray / triangle test, branch-free (the oracle's tri_test_dd has the argument): edge functions as signed volumes
// U = d.(B x C), V = d.(C x A), W = d.(A x B) of the vertices relative to the ray origin, every cross-product component two rounded
// products and a subtraction (NO fma: the file is compiled with -ffp-contract=off), so the two triangles of a shared edge compute
// the same number for it up to sign and no ray passes between them.  No early-outs: the three loads of a triangle are issued
// together instead of being sunk behind branches.  Record: {v0.xyz, v1.x} {v1.yz, v2.xy} {v2.z, prim, -, -}.
__device__ __forceinline__ V3 cross_exact(V3 a, V3 b) { return V3{(a.y * b.z) - (a.z * b.y), (a.z * b.x) - (a.x * b.z), (a.x * b.y) - (a.y * b.x)}; }
// MASK: a candidate that would be accepted is, if its record is masked (q2.z = cutoff > 0, q2.w = slot), kept only when its alpha passes
// (alpha_counts): a masked triangle that fails is not there for this ray.
// PANE (any hit, the path tracer's own shadow queues): a candidate that would be accepted -- the cutout test included -- on
// a pane record does not occlude: the ray's contribution pay[0..2] is multiplied by the pane's expected straight-through transmittance
// (pane_attenuation) and best stays what it is.  A contribution that has become 0 in all three channels ends the ray as occluded.
__device__ __forceinline__ bool pane_record(float cutoff, uint32_t slot, uint32_t first_slot) { return cutoff != 0.0f ? slot >= first_slot : slot != 0u; }
// A = transmission (1 - F'(cos_i)) tint at barycentrics (u, v) of primitive prim: hit_finish's shading normal (not face-forwarded) and albedo
__device__ __forceinline__ V3 pane_attenuation(const PaneDev& p, uint32_t prim, float u, float v, V3 d) {
    const HitRecord h = hit_fetch(p.sc, prim);
    const Surface s = hit_finish(p.sc, p.sc.shade_geoms, h, u, v);
    const GlassDev gl = p.glass[h.rec.w];
    const float cos_i = fabsf(dot(s.normal, d)) / sqrtf(dot(d, d));
    return s.albedo * (gl.transmission * pane_pass_fraction(gl.ior, cos_i));
}
template <bool MASK = false, bool PANE = false>
__device__ __forceinline__ void tri_test_nb(float4 q0, float4 q1, float4 q2, V3 o, V3 d, float inv_dd, float tmin, Hit& best, const AlphaDev& alpha = AlphaDev{},
                                            const PaneDev* pane = nullptr, float* pay0 = nullptr, float* pay1 = nullptr, float* pay2 = nullptr) {
    const V3 A = v3(q0.x, q0.y, q0.z) - o, B = v3(q0.w, q1.x, q1.y) - o, C = v3(q1.z, q1.w, q2.x) - o;
    const float U = dot_fma(d, cross_exact(B, C)), V = dot_fma(d, cross_exact(C, A)), W = dot_fma(d, cross_exact(A, B));
    const float det = U + (V + W);  // the association of T below: equal vertex distances give t exactly
    const float inv = 1.0f / det;
    const float w = U * inv, u = V * inv, v = W * inv;
    const float T = __builtin_fmaf(U, dot_fma(A, d), __builtin_fmaf(V, dot_fma(B, d), W * dot_fma(C, d)));
    const float t = (T * inv) * inv_dd;
    const uint32_t prim = __float_as_uint(q2.y);
    // barycentrics >= -2^-20: a superset of "U, V, W share a sign" (the shared-edge guarantee stands) that also closes T-junctions
    // and edges of separate meshes that merely coincide, which no watertight test covers
    constexpr float kEdgeEps = 9.5367431640625e-07f;
    const bool inside = (w >= -kEdgeEps) & (u >= -kEdgeEps) & (v >= -kEdgeEps);
    bool ok = (det != 0.0f) & inside & (t > tmin) & ((t < best.t) | ((t == best.t) & (prim < best.prim)));
    if (MASK && ok && q2.z != 0.0f) ok = alpha_counts(alpha, __float_as_uint(q2.w), q2.z, prim, u, v);
    if constexpr (PANE) {
        if (ok && pane_record(q2.z, __float_as_uint(q2.w), pane->first_slot)) {
            const V3 att = pane_attenuation(*pane, prim, u, v, d);
            *pay0 *= att.x;
            *pay1 *= att.y;
            *pay2 *= att.z;
            ok = *pay0 == 0.0f && *pay1 == 0.0f && *pay2 == 0.0f;
        }
    }
    best.t = ok ? t : best.t;
    best.u = ok ? u : best.u;
    best.v = ok ? v : best.v;
    best.prim = ok ? prim : best.prim;
}

// The exit table's cell of a ray (DESIGN.md sections 5 and 7; `inv` = the guarded inverses of d): where the ray leaves the box -- the
// nearest of the three far planes; the other two coordinates of that point, in cells.  Whatever the ray is (origin outside, pointing away,
// zero components, overflow to inf or NaN), the index is clamped into the table: fmax / fmin drop a NaN, the integer minimum below is the
// last word.
__device__ __forceinline__ uint32_t exit_cell(const ExitHeader& e, V3 o, V3 d, V3 inv) {
    const float tx = ((inv.x < 0.0f ? e.lo[0] : e.hi[0]) - o.x) * inv.x, ty = ((inv.y < 0.0f ? e.lo[1] : e.hi[1]) - o.y) * inv.y,
                tz = ((inv.z < 0.0f ? e.lo[2] : e.hi[2]) - o.z) * inv.z;
    const bool ax0 = (tx <= ty) & (tx <= tz), ax1 = !ax0 & (ty <= tz);
    const float te = ax0 ? tx : (ax1 ? ty : tz);
    const float cx = (__builtin_fmaf(te, d.x, o.x) - e.lo[0]) * e.scale[0], cy = (__builtin_fmaf(te, d.y, o.y) - e.lo[1]) * e.scale[1],
                cz = (__builtin_fmaf(te, d.z, o.z) - e.lo[2]) * e.scale[2];
    // axis 0: (u, v) = (y, z); 1: (z, x); 2: (x, y); face = 2 axis + (leaves through the high plane)
    const float cu = ax0 ? cy : (ax1 ? cz : cx), cv = ax0 ? cz : (ax1 ? cx : cy);
    const float ia = ax0 ? inv.x : (ax1 ? inv.y : inv.z);
    const uint32_t face = (ax0 ? 0u : (ax1 ? 2u : 4u)) + (ia < 0.0f ? 0u : 1u);
    const float top = (float)(e.R - 1u);
    const uint32_t iu = (uint32_t)__builtin_fminf(__builtin_fmaxf(cu, 0.0f), top), iv = (uint32_t)__builtin_fminf(__builtin_fmaxf(cv, 0.0f), top);
    const uint32_t cell = (face * e.R + iv) * e.R + iu;
    return cell < e.last ? cell : e.last;
}

}  // namespace rt3
