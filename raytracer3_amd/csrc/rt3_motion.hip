// rt3_motion.hip -- the "motion" pass: per pixel, where the surface point the primary ray hit was one frame ago.  No
// reference counterpart.  The input of "temporal" when instances move between frames (rt3_temporal_set_motion_input).
//
//   k_motion -> per pixel of the rank's list: the primary hit record {t, u, v, prim} and
//                 miss                                  -> {0, 0, 0, 0}
//                 hit on an instance that did not move  -> {P, 1},  P = dn_position(g, px, py, t): the bits "denoise" and "temporal" compute
//                 hit on an instance that moved         -> {P', 2}, P' = prev_i * ((a w + b u) + c v), w = (1 - u) - v, from the triangle's
//                                                          object-space vertices a, b, c (P' = the point itself when prev_i is the identity)
//
// Arithmetic contract: tests/ref_motion.py restates every operation in numpy float32; the pass equals it bit for bit.  Which instances
// moved is decided on the host, word for word (rt3_api.hip: motion_tables); the kernel only follows the table.
//
// One thread per listed pixel, like k_gbuffer: the 16-byte hit record is read and the 16-byte texel stored in list order.  With no moved
// instance the table is absent and a hit lane only computes primary_ray.  Otherwise every hit lane reads prim_geom[prim] and its geometry's
// 4-byte slot; only lanes on moved instances go on to first_prim, the geometry's two offsets, three indices, three vertices and the 64-byte
// previous matrix, and lanes of a wave on one instance read the same lines of the small tables.  No LDS, no atomics.
#include <hip/hip_runtime.h>

#include "rt3_bvh_device.hpp"
#include "rt3_filter_device.hpp"
#include "rt3_internal.hpp"

namespace rt3 {

namespace {

__global__ __launch_bounds__(256) void k_motion(GConstDev g, MotionDev m, const uint32_t* __restrict__ pixels, uint32_t npix, uint32_t width,
                                                const float* __restrict__ hits, float4* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        const uint32_t xy = pixels[i];
        const uint32_t px = xy & 0xFFFFu, py = xy >> 16;
        const size_t pi = (size_t)py * width + px;
        const float4 hrec = reinterpret_cast<const float4*>(hits)[i];
        const uint32_t prim = __float_as_uint(hrec.w);
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (prim != kMiss) {
            const uint32_t slot = m.geom_slot ? m.geom_slot[m.prim_geom[prim]] : kMotionUnmoved;
            if (slot == kMotionUnmoved) {
                const V3 P = dn_position(g, px, py, hrec.x);
                r = make_float4(P.x, P.y, P.z, 1.0f);
            } else {
                V3 a, b, c;
                fetch_triangle_object(m.verts, m.indices, m.geoms, m.prim_geom, m.first_prim, prim, a, b, c);
                const float u = hrec.y, v = hrec.z, w = (1.0f - u) - v;  // a, b, c pair with (w, u, v) like hit_finish's normals
                V3 p = v3((a.x * w + b.x * u) + c.x * v, (a.y * w + b.y * u) + c.y * v, (a.z * w + b.z * u) + c.z * v);
                const MotionPrevDev& pm = m.prev[slot];
                if (!pm.identity) p = transform_point(pm.m, p);
                r = make_float4(p.x, p.y, p.z, 2.0f);
            }
        }
        out[pi] = r;
    }
}

}  // namespace

void launch_motion(hipStream_t st, const MotionLaunch& L) {
    const unsigned want = (L.npix + 255u) / 256u, grid = want < 1u ? 1u : (want > 4096u ? 4096u : want);  // k_gbuffer's shape
    hipLaunchKernelGGL(k_motion, dim3(grid), dim3(256), 0, st, L.g, L.m, L.pixels, L.npix, L.width, L.hits, (float4*)L.out);
}

}  // namespace rt3
