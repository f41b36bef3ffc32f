// rt3_motion.hip -- the "motion" pass: per pixel, where the surface point the primary ray hit was one frame ago (DESIGN.md sections 4h, 4i).
// No reference counterpart.  The input of "temporal" when instances move or meshes deform between frames (rt3_temporal_set_motion_input).
//
//   k_motion -> per pixel of the rank's list: the primary hit record {t, u, v, prim} and
//                 miss                                  -> {0, 0, 0, 0}
//                 hit on an instance that did not move  -> {P, 1},  P = dn_position(g, px, py, t): the bits "denoise" and "temporal" compute
//                 hit on an instance that moved         -> {P', 2}, P' = prev_i * ((a w + b u) + c v), w = (1 - u) - v, from the triangle's
//                                                          object-space vertices a, b, c (P' = the point itself when prev_i is the identity)
//                 hit on a deformed geometry (DEFORM)   -> {P'', 3}, the same expression over the triangle's snapshot positions a', b', c'
//                                                          (rt3_scene_snapshot_vertices); prev_i = the current matrix without previous ones
//
// Arithmetic contract: tests/ref_motion.py and tests/ref_deform.py restate every operation in numpy float32; the pass equals them bit for
// bit.  Which instances moved is decided on the host, word for word, and which geometries are deformed by k_compare_positions below, word
// for word too (rt3_passes.hip: motion_tables); the kernel only follows the table.
//
// One thread per listed pixel, like k_gbuffer: the 16-byte hit record is read and the 16-byte texel stored in list order.  With nothing moved
// or deformed the table is absent and a hit lane only computes primary_ray.  Otherwise every hit lane reads prim_geom[prim] and its
// geometry's 4-byte slot; only lanes on moved instances or deformed geometries go on to first_prim, the geometry's two offsets, three
// indices, three vertices (or three 16-byte snapshot records) and the 64-byte previous matrix, and lanes of a wave on one instance read
// the same lines of the small tables.  No LDS, no atomics.  k_motion<false> is the kernel without deformation, instruction for instruction.
//
//   k_snapshot_positions -> the snapshot: one {x, y, z, 0} record per vertex of a range, a device-side copy
//   k_compare_positions  -> per chunk (geometry, [lo, hi)) of at most kDeformChunk vertices: "any position word differs from the snapshot",
//                           reduced over the group; one lane ORs 1 into the geometry's flag
#include <hip/hip_runtime.h>

#include "rt3_bvh_device.hpp"
#include "rt3_camera.hpp"
#include "rt3_filter_device.hpp"
#include "rt3_internal.hpp"
#include "rt3_math.hpp"
#include "rt3_surface.hpp"

namespace rt3 {

namespace {

__device__ __forceinline__ const float4* snapshot_of() { return nullptr; }
__device__ __forceinline__ const float4* snapshot_of(const float4* prev_pos) { return prev_pos; }

// Snapshot: k_motion<true, const float4*> takes the snapshot as one more argument; k_motion<false> has exactly the arguments (and so the
// kernel-argument offsets and instruction stream) of the kernel without deformation
template <bool DEFORM, typename... Snapshot>
__global__ __launch_bounds__(256) void k_motion(GConstDev g, MotionDev m, const uint32_t* __restrict__ pixels, uint32_t npix, uint32_t width,
                                                const float* __restrict__ hits, float4* __restrict__ out, Snapshot... snapshot) {
    static_assert(sizeof...(Snapshot) == (DEFORM ? 1 : 0), "the snapshot goes with DEFORM");
    const float4* __restrict__ prev_pos = snapshot_of(snapshot...);
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
                uint32_t inst = slot;
                float kind = 2.0f;
                if (DEFORM && (slot & kMotionDeformed)) {
                    fetch_triangle_snapshot(prev_pos, m.indices, m.geoms, m.prim_geom, m.first_prim, prim, a, b, c);
                    inst = slot & ~kMotionDeformed;
                    kind = 3.0f;
                } else {
                    fetch_triangle_object(m.verts, m.indices, m.geoms, m.prim_geom, m.first_prim, prim, a, b, c);
                }
                const float u = hrec.y, v = hrec.z, w = (1.0f - u) - v;  // a, b, c pair with (w, u, v) like hit_finish's normals
                V3 p = v3((a.x * w + b.x * u) + c.x * v, (a.y * w + b.y * u) + c.y * v, (a.z * w + b.z * u) + c.z * v);
                const MotionPrevDev& pm = m.prev[inst];
                if (!pm.identity) p = transform_point(pm.m, p);
                r = make_float4(p.x, p.y, p.z, kind);
            }
        }
        out[pi] = r;
    }
}

__global__ __launch_bounds__(256) void k_snapshot_positions(const float* __restrict__ verts, uint32_t first, uint32_t n, float4* __restrict__ prev_pos) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float* v = verts + 8 * (size_t)(first + i);
        prev_pos[(size_t)(first + i)] = make_float4(v[0], v[1], v[2], 0.0f);
    }
}

__global__ __launch_bounds__(256) void k_compare_positions(const float* __restrict__ verts, const float4* __restrict__ prev_pos,
                                                           const uint4* __restrict__ chunks, uint32_t* __restrict__ flags) {
    const uint4 ch = chunks[blockIdx.x];  // {geometry, lo, hi, -}
    int differs = 0;
    for (uint32_t v = ch.y + threadIdx.x; v < ch.z; v += blockDim.x) {
        const uint32_t* cur = reinterpret_cast<const uint32_t*>(verts) + 8 * (size_t)v;
        const float4 p = prev_pos[v];
        differs |= (int)(((cur[0] ^ __float_as_uint(p.x)) | (cur[1] ^ __float_as_uint(p.y)) | (cur[2] ^ __float_as_uint(p.z))) != 0u);
    }
    differs = __syncthreads_or(differs);
    if (threadIdx.x == 0 && differs) atomicOr(&flags[ch.x], 1u);
}

}  // namespace

void launch_motion(hipStream_t st, const MotionLaunch& L) {
    const unsigned want = (L.npix + 255u) / 256u, grid = want < 1u ? 1u : (want > 4096u ? 4096u : want);  // k_gbuffer's shape
    if (L.prev_pos)
        hipLaunchKernelGGL((k_motion<true, const float4*>), dim3(grid), dim3(256), 0, st, L.g, L.m, L.pixels, L.npix, L.width, L.hits, (float4*)L.out, L.prev_pos);
    else
        hipLaunchKernelGGL(k_motion<false>, dim3(grid), dim3(256), 0, st, L.g, L.m, L.pixels, L.npix, L.width, L.hits, (float4*)L.out);
}

void launch_snapshot_positions(hipStream_t st, const float* verts, uint32_t first, uint32_t n, float4* prev_pos) {
    if (n == 0) return;
    const unsigned want = (n + 255u) / 256u, grid = want > 4096u ? 4096u : want;
    hipLaunchKernelGGL(k_snapshot_positions, dim3(grid), dim3(256), 0, st, verts, first, n, prev_pos);
}

void launch_compare_positions(hipStream_t st, const float* verts, const float4* prev_pos, const uint4* chunks, uint32_t n_chunks, uint32_t* flags) {
    if (n_chunks == 0) return;
    hipLaunchKernelGGL(k_compare_positions, dim3(n_chunks), dim3(256), 0, st, verts, prev_pos, chunks, flags);
}

}  // namespace rt3
