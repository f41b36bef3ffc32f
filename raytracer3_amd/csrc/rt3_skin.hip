// rt3_skin.hip -- k_skin_pose: a skin's rest pose, resident on the device, blended into the vertex buffer.  No reference
// counterpart.  The stage ahead of rt3_accel_refit, rt3_scene_snapshot_vertices and "motion" (sections 4c, 4i): those run unchanged.
//
//   k_skin_pose -> per vertex v of the skin: the rest record {p, n, uv} (two 16-byte loads), its four joints (one 8-byte load) and weights
//                  (one 16-byte load); per target with a weight != 0 three (six with normal deltas) 4-byte loads of the tight delta arrays,
//                  consecutive over the lanes; up to four palette entries of 48 bytes (three 16-byte loads each, a gather over a table that
//                  stays in the cache: 3 KiB at 64 joints); the rule of rt3_skin.hpp; the whole 32-byte record stored with two 16-byte stores.
//
// Arithmetic contract: tests/ref_skin.py restates every operation in numpy float32; the kernel equals it bit for bit.  One thread per vertex,
// 256-thread groups, the grid-stride loop of the other streaming kernels.  No LDS, no scratch; the only atomic is the range flag's, issued by
// the lanes whose position left the range (none, in a frame that renders).  The target weights travel in the kernel arguments.
#include <hip/hip_runtime.h>

#include "rt3_internal.hpp"
#include "rt3_math.hpp"
#include "rt3_skin.hpp"

namespace rt3 {

namespace {

__global__ __launch_bounds__(256) void k_skin_pose(SkinLaunch L) {
    const float4* __restrict__ rest = L.rest;
    const uint2* __restrict__ joints = L.joints;
    const float4* __restrict__ weights = L.weights;
    const float4* __restrict__ palette = L.palette;
    const float* __restrict__ dpos = L.dpos;
    const float* __restrict__ dnrm = L.dnrm;
    float4* __restrict__ out = L.out;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < L.n; i += gridDim.x * blockDim.x) {
        const float4 r0 = rest[2 * (size_t)i], r1 = rest[2 * (size_t)i + 1];  // {p.xyz, n.x} {n.yz, uv}
        const uint2 j = joints[i];
        const float4 w = weights[i];
        V3 p = v3(r0.x, r0.y, r0.z), n = v3(r0.w, r1.x, r1.y);
#pragma unroll
        for (uint32_t t = 0; t < kSkinMaxTargets; t++) {
            if (t < L.n_targets && L.a[t] != 0.0f) {  // (uniform: the weights are the launch's)
                const size_t at = 3 * ((size_t)t * L.n + i);
                p = skin_morph(p, L.a[t], v3(dpos[at], dpos[at + 1], dpos[at + 2]));
                if (dnrm) n = skin_morph(n, L.a[t], v3(dnrm[at], dnrm[at + 1], dnrm[at + 2]));
            }
        }
        float M[12];
        if (skin_blend(palette, j, w, M)) skin_place(M, p, n);
        out[2 * (size_t)i] = make_float4(p.x, p.y, p.z, n.x);
        out[2 * (size_t)i + 1] = make_float4(n.y, n.z, r1.z, r1.w);
        if (!skin_in_range(p)) atomicOr(L.flag, 1u);
    }
}

}  // namespace

void launch_skin_pose(hipStream_t st, const SkinLaunch& L) {
    if (L.n == 0) return;
    const unsigned want = (L.n + 255u) / 256u, grid = want > 4096u ? 4096u : want;
    hipLaunchKernelGGL(k_skin_pose, dim3(grid), dim3(256), 0, st, L);
}

}  // namespace rt3
