// rt3_skin.hpp -- the skinning rule: morph, blend, place and range-check one vertex.  No reference counterpart.
// Stated once here; k_skin_pose (rt3_skin.hip) only fetches and stores around it, and tests/ref_skin.py restates every line in numpy float32.
//
// Arithmetic contract: fp32, no contraction, every operation singly rounded in the order written.
//   morph   for t = 0 .. n_targets-1 with a_t != 0:  p.k = p.k + a_t * dP[t][v].k   (n the same with dN, when the skin has normal deltas)
//   blend   k0 = the first k in 0..3 with w_k != 0:  M = w_k0 * J[j_k0];  every later k with w_k != 0:  M = M + w_k * J[j_k]
//           (entry by entry, a product, then a sum).  No w_k != 0: the vertex keeps its morphed p and n as they are.
//   place   p' = transform_point(M, p);  n' = normalize(transform_vector(M, n)) -- no inverse transpose, the instance rule of hit_finish
//   range   every |p'.k| <= 1e18, else the skin's flag word gets bit 0 (the record is written all the same)
// A palette entry is the joint matrix as the device tables hold matrices (pack3x4): 12 floats, column-major 3 x 4, the last row (0, 0, 0, 1)
// implied -- what transform_point reads, and in its first nine floats what transform_vector reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt3_math.hpp"
#include "rt3_surface.hpp"

namespace rt3 {

constexpr float kSkinRange = 1.0e18f;  // check_positions' bound (rt3_scene.hip)

RT3_DEV V3 skin_morph(V3 p, float a, V3 d) { return v3(p.x + a * d.x, p.y + a * d.y, p.z + a * d.z); }

// M (12 floats) = sum of w_k J[j_k] over the non-zero weights, in the order k = 0, 1, 2, 3; false: every weight is 0 and M is not written.
// j = {j0 | j1 << 16, j2 | j3 << 16}
RT3_DEV bool skin_blend(const float4* __restrict__ palette, uint2 j, float4 w, float* M) {
    const uint32_t jk[4] = {j.x & 0xFFFFu, j.x >> 16, j.y & 0xFFFFu, j.y >> 16};
    const float wk[4] = {w.x, w.y, w.z, w.w};
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (wk[k] != 0.0f) {
            const float4* J = palette + 3 * (size_t)jk[k];
            const float4 c0 = J[0], c1 = J[1], c2 = J[2];
            const float e[12] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w};
            if (!any) {
#pragma unroll
                for (int q = 0; q < 12; q++) M[q] = wk[k] * e[q];
            } else {
#pragma unroll
                for (int q = 0; q < 12; q++) M[q] = M[q] + wk[k] * e[q];
            }
            any = true;
        }
    }
    return any;
}

RT3_DEV void skin_place(const float* M, V3& p, V3& n) {
    p = transform_point(M, p);
    n = normalize(transform_vector(M, n));
}

RT3_DEV bool skin_in_range(V3 p) { return fabsf(p.x) <= kSkinRange && fabsf(p.y) <= kSkinRange && fabsf(p.z) <= kSkinRange; }

}  // namespace rt3
