// rt3_tlas.hip -- the device side of the two-level structure (RT3_OPT_INSTANCE_MODE 1).
//
// One node array in the quantised 64-byte four-wide format:
//   [0, n_top)                 the top tree, root at node 0 (so the traversal kernels' LDS copy, k_top_cache, holds it)
//   [rec_base, rec_base + 2n)  two 64-byte records per instance: {inverse 3 x 4, bottom root, prim base | identity << 31, pad_abs, pad_rel}
//                              and {forward 3 x 4, -}
//   [bottom ...)               the bottom trees, one per distinct mesh, concatenated (references rebased to the combined arrays)
// The bottom trees are built by lbvh_build over an identity table with local primitive ids; the top tree by lbvh_build too, over one
// degenerate triangle per instance whose bounds are the instance's world box (its leaves are then re-pointed at the records).
#include <hip/hip_runtime.h>

#include "rt3_internal.hpp"

namespace rt3 {

__global__ void k_tlas_rebase(const float4* __restrict__ src, float4* __restrict__ dst, uint32_t n, uint32_t node_from, uint32_t node_to,
                              uint32_t tri_from, uint32_t tri_to) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float4 q0 = src[4 * (size_t)i], q1 = src[4 * (size_t)i + 1], q2 = src[4 * (size_t)i + 2], q3 = src[4 * (size_t)i + 3];
        uint32_t r[4] = {__float_as_uint(q2.z), __float_as_uint(q2.w), __float_as_uint(q3.x), __float_as_uint(q3.y)};
        for (int k = 0; k < 4; k++) {
            if (r[k] == 0xFFFFFFFFu) continue;  // empty slot
            if (r[k] & 0x80000000u) r[k] = (r[k] & 0xF0000000u) | ((r[k] & 0x0FFFFFFFu) - tri_from + tri_to);
            else r[k] = r[k] - node_from + node_to;
        }
        q2.z = __uint_as_float(r[0]);
        q2.w = __uint_as_float(r[1]);
        q3.x = __uint_as_float(r[2]);
        q3.y = __uint_as_float(r[3]);
        dst[4 * (size_t)i] = q0;
        dst[4 * (size_t)i + 1] = q1;
        dst[4 * (size_t)i + 2] = q2;
        dst[4 * (size_t)i + 3] = q3;
    }
}
void tlas_rebase_nodes(hipStream_t st, const float4* src, float4* dst, uint32_t n, uint32_t node_from, uint32_t node_to, uint32_t tri_from, uint32_t tri_to) {
    if (n == 0) return;
    const unsigned grid = (n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256;
    hipLaunchKernelGGL(k_tlas_rebase, dim3(grid), dim3(256), 0, st, src, dst, n, node_from, node_to, tri_from, tri_to);
}

__global__ void k_tlas_box_tris(const float* __restrict__ boxes, uint32_t n, float* __restrict__ verts, uint32_t* __restrict__ indices) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float* b = boxes + 6 * (size_t)i;
        for (int v = 0; v < 3; v++) {
            float* o = verts + 8 * (3 * (size_t)i + v);
            const float* c = v == 1 ? b + 3 : b;
            o[0] = c[0];
            o[1] = c[1];
            o[2] = c[2];
            for (int k = 3; k < 8; k++) o[k] = 0.0f;
            o[3 + 2] = 1.0f;  // a unit normal: nothing reads it, but the vertex stays well formed
            indices[3 * (size_t)i + v] = 3u * i + (uint32_t)v;
        }
    }
}
void tlas_box_tris(hipStream_t st, const float* boxes, uint32_t n, float* verts, uint32_t* indices) {
    if (n == 0) return;
    const unsigned grid = (n + 255) / 256 > 1024 ? 1024 : (n + 255) / 256;
    hipLaunchKernelGGL(k_tlas_box_tris, dim3(grid), dim3(256), 0, st, boxes, n, verts, indices);
}

__global__ void k_tlas_emit_top(const float4* __restrict__ top_nodes, uint32_t n, const float4* __restrict__ top_tris, uint32_t rec_base,
                                float4* __restrict__ dst) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float4 q2 = top_nodes[4 * (size_t)i + 2], q3 = top_nodes[4 * (size_t)i + 3];
        uint32_t r[4] = {__float_as_uint(q2.z), __float_as_uint(q2.w), __float_as_uint(q3.x), __float_as_uint(q3.y)};
        for (int k = 0; k < 4; k++) {
            if (r[k] == 0xFFFFFFFFu || !(r[k] & 0x80000000u)) continue;
            // leaf_max 1: one triangle per leaf, its record's primitive id is the instance slot
            const uint32_t slot = __float_as_uint(top_tris[3 * (size_t)(r[k] & 0x0FFFFFFFu) + 2].y);
            r[k] = 0x80000000u | (rec_base + 2u * slot);
        }
        q2.z = __uint_as_float(r[0]);
        q2.w = __uint_as_float(r[1]);
        q3.x = __uint_as_float(r[2]);
        q3.y = __uint_as_float(r[3]);
        dst[4 * (size_t)i] = top_nodes[4 * (size_t)i];
        dst[4 * (size_t)i + 1] = top_nodes[4 * (size_t)i + 1];
        dst[4 * (size_t)i + 2] = q2;
        dst[4 * (size_t)i + 3] = q3;
    }
}
void tlas_emit_top(hipStream_t st, const float4* top_nodes, uint32_t n_nodes, const float4* top_tris, uint32_t rec_base, float4* dst) {
    if (n_nodes == 0) return;
    const unsigned grid = (n_nodes + 255) / 256 > 1024 ? 1024 : (n_nodes + 255) / 256;
    hipLaunchKernelGGL(k_tlas_emit_top, dim3(grid), dim3(256), 0, st, top_nodes, n_nodes, top_tris, rec_base, dst);
}

}  // namespace rt3
