// rt3_bvh_device.hpp -- device code shared by the acceleration-structure builder (rt3_lbvh.hip) and its refit (rt3_refit.hip):
// the triangle fetch, the leaf padding and the quantised node encoder.  A refitted tree is written by the same expressions a build uses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt3_math.hpp"
#include "rt3_surface.hpp"

namespace rt3 {

// The world-space triangle of flattened primitive `prim`: the vertices of its geometry under its instance's matrix (as uploaded when
// that matrix is the identity).  Every user goes through here, so two triangles that share an edge see bit-identical end points.
__device__ __forceinline__ void fetch_triangle(const float* verts, const uint32_t* indices, const FlatGeomDev* geoms, const uint32_t* prim_geom,
                                               const uint32_t* first_prim, uint32_t prim, V3& a, V3& b, V3& c) {
    uint32_t g = prim_geom[prim];
    const FlatGeomDev& fg = geoms[g];
    uint32_t io = fg.g.index_offset + 3u * (prim - first_prim[g]);
    const float* v0 = verts + 8 * (size_t)(fg.g.vertex_offset + indices[io]);
    const float* v1 = verts + 8 * (size_t)(fg.g.vertex_offset + indices[io + 1]);
    const float* v2 = verts + 8 * (size_t)(fg.g.vertex_offset + indices[io + 2]);
    a = v3(v0[0], v0[1], v0[2]);
    b = v3(v1[0], v1[1], v1[2]);
    c = v3(v2[0], v2[1], v2[2]);
    if (!fg.identity) {
        a = transform_point(fg.m, a);
        b = transform_point(fg.m, b);
        c = transform_point(fg.m, c);
    }
}
// The same triangle in object space: fetch_triangle's index arithmetic without the matrix (the "motion" pass puts the previous frame's
// matrix on the interpolated point instead, rt3_motion.hip)
__device__ __forceinline__ void fetch_triangle_object(const float* verts, const uint32_t* indices, const FlatGeomDev* geoms, const uint32_t* prim_geom,
                                                      const uint32_t* first_prim, uint32_t prim, V3& a, V3& b, V3& c) {
    uint32_t g = prim_geom[prim];
    const FlatGeomDev& fg = geoms[g];
    uint32_t io = fg.g.index_offset + 3u * (prim - first_prim[g]);
    const float* v0 = verts + 8 * (size_t)(fg.g.vertex_offset + indices[io]);
    const float* v1 = verts + 8 * (size_t)(fg.g.vertex_offset + indices[io + 1]);
    const float* v2 = verts + 8 * (size_t)(fg.g.vertex_offset + indices[io + 2]);
    a = v3(v0[0], v0[1], v0[2]);
    b = v3(v1[0], v1[1], v1[2]);
    c = v3(v2[0], v2[1], v2[2]);
}
// fetch_triangle_object's index arithmetic over the snapshot's 16-byte records (rt3_scene_snapshot_vertices): the triangle one frame ago
// (rt3_motion.hip, rt3_guide.hip)
__device__ __forceinline__ void fetch_triangle_snapshot(const float4* prev_pos, const uint32_t* indices, const FlatGeomDev* geoms, const uint32_t* prim_geom,
                                                        const uint32_t* first_prim, uint32_t prim, V3& a, V3& b, V3& c) {
    uint32_t g = prim_geom[prim];
    const FlatGeomDev& fg = geoms[g];
    uint32_t io = fg.g.index_offset + 3u * (prim - first_prim[g]);
    const float4 v0 = prev_pos[(size_t)(fg.g.vertex_offset + indices[io])];
    const float4 v1 = prev_pos[(size_t)(fg.g.vertex_offset + indices[io + 1])];
    const float4 v2 = prev_pos[(size_t)(fg.g.vertex_offset + indices[io + 2])];
    a = v3(v0.x, v0.y, v0.z);
    b = v3(v1.x, v1.y, v1.z);
    c = v3(v2.x, v2.y, v2.z);
}
// conservative leaf padding from the scene bounds (ordered-uint encoded min.xyz, max.xyz): a share of the extent, and at least 2^-20
// of the largest coordinate magnitude ("Leaf padding")
__device__ __forceinline__ float leaf_pad(const uint32_t* bounds) {
    float ex = ordered_to_float(bounds[3]) - ordered_to_float(bounds[0]);
    float ey = ordered_to_float(bounds[4]) - ordered_to_float(bounds[1]);
    float ez = ordered_to_float(bounds[5]) - ordered_to_float(bounds[2]);
    float mag = fmax_sel(fmax_sel(fabsf(ordered_to_float(bounds[0])), fabsf(ordered_to_float(bounds[3]))),
                         fmax_sel(fmax_sel(fabsf(ordered_to_float(bounds[1])), fabsf(ordered_to_float(bounds[4]))),
                                  fmax_sel(fabsf(ordered_to_float(bounds[2])), fabsf(ordered_to_float(bounds[5])))));
    return fmax_sel(fmax_sel(ex, fmax_sel(ey, ez)) * 1.0e-5f, mag * 0x1p-20f);
}

// 64-byte four-wide node with 8-bit child boxes on a per-axis power-of-two grid anchored at the node's min corner:
//   float4 0: origin.xyz, exponents ex | ey << 8 | ez << 16 (quantize_words; quantize_node turns them into three float steps: word 3, words 14 / 15)
//   float4 1 + first half of 2: 4 x {qlo.xyz, qhi.xyz} bytes
//   float4 2 second half + float4 3 first half: the four references
// Conservative with respect to the decode expression origin + float(q) * scale used by the traversal kernels.
__device__ void quantize_words(const float (*mn)[3], const float (*mx)[3], const uint32_t* ref, uint32_t ns, uint32_t* w) {
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = 0u;
    uint32_t qb[4][6];
    for (int a = 0; a < 3; a++) {
        float lo = mn[0][a], hi = mx[0][a];
        for (uint32_t k = 1; k < ns; k++) {
            lo = fmin_sel(lo, mn[k][a]);
            hi = fmax_sel(hi, mx[k][a]);
        }
        w[a] = __float_as_uint(lo);
        float sdiv = (hi - lo) / 255.0f;
        uint32_t bits = __float_as_uint(sdiv), e = (bits >> 23) & 0xFFu;
        if (bits & 0x7FFFFFu) e += 1;
        if (e < 1) e = 1;
        for (;;) {  // grow the step until every child fits in 8 bits
            float scale = __uint_as_float(e << 23);
            uint32_t worst = 0;
            for (uint32_t k = 0; k < ns; k++) {
                float fl = floorf((mn[k][a] - lo) / scale);
                uint32_t ql = fl > 255.0f ? 255u : (uint32_t)fl;
                while (ql > 0 && lo + (float)ql * scale > mn[k][a]) ql--;
                float fh = ceilf((mx[k][a] - lo) / scale);
                uint32_t qh = fh > 1024.0f ? 1024u : (uint32_t)fh;
                while (qh < 1024u && lo + (float)qh * scale < mx[k][a]) qh++;
                worst = qh > worst ? qh : worst;
                qb[k][a] = ql;
                qb[k][3 + a] = qh > 255u ? 255u : qh;
            }
            if (worst <= 255u) break;
            e++;
        }
        w[3] |= e << (8 * a);
    }
    for (uint32_t k = 0; k < 4; k++) {
        for (int j = 0; j < 6; j++) {
            uint32_t v = k < ns ? qb[k][j] : (j < 3 ? 255u : 0u);
            uint32_t byte = 6 * k + j;
            w[4 + (byte >> 2)] |= v << (8 * (byte & 3u));
        }
        w[10 + k] = k < ns ? ref[k] : 0xFFFFFFFFu;
    }
}
__device__ void quantize_node(const float (*mn)[3], const float (*mx)[3], const uint32_t* ref, uint32_t ns, float4* out) {
    uint32_t w[16];
    quantize_words(mn, mx, ref, ns, w);
    // the 64-byte node carries its three steps as FLOATS (word 3 and the two spare words 14, 15): the walk multiplies them into the
    // ray's inverse direction at every node and used to rebuild each from its exponent byte first (a shift and a mask per axis)
    const uint32_t ex = w[3];
    w[3] = (ex & 0xFFu) << 23;
    w[14] = ((ex >> 8) & 0xFFu) << 23;
    w[15] = ((ex >> 16) & 0xFFu) << 23;
#pragma unroll
    for (int k = 0; k < 4; k++)
        out[k] = make_float4(__uint_as_float(w[4 * k]), __uint_as_float(w[4 * k + 1]), __uint_as_float(w[4 * k + 2]), __uint_as_float(w[4 * k + 3]));
}

}  // namespace rt3
