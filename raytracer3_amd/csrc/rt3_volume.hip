// rt3_volume.hip -- k_absorb: Beer-Lambert absorption inside solid glass, on the extension queue between the k_extend of a bounce and the
// k_shade that follows (rt3_scene_set_attenuation), and the kernel of self-test op 36.  A kernel of its own name,
// launched only for a built scene with an absorbing geometry: no instance of k_shade, k_extend or k_shadow changes.
#include <hip/hip_runtime.h>

#include "rt3_internal.hpp"
#include "rt3_math.hpp"
#include "rt3_surface.hpp"
#include "rt3_volume.hpp"

namespace rt3 {

constexpr int kAbsorbBlock = 256;
constexpr unsigned kAbsorbMaxBlocks = 2048;  // 256 CUs x 8: grid-stride beyond that

// Pure streaming, one thread per record, no barrier, no LDS: the hit record and the {d, path id} ray record (two coalesced 16-byte loads,
// issued together) decide most records -- a miss leaves after them, a hit on a geometry that does not absorb after two gathers (its shading
// record, then the 16-byte table entry).  Only a back-face hit on an absorbing geometry reads and writes its three throughput words.
__global__ __launch_bounds__(kAbsorbBlock) void k_absorb(AbsorbLaunch a) {
    const size_t S = a.stride;
    const uint32_t n = *a.count;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 hrec = reinterpret_cast<const float4*>(a.hits)[i];
        const float4 rd = reinterpret_cast<const float4*>(a.rays)[S + i];
        const uint32_t prim = __float_as_uint(hrec.w);
        if (prim == kMiss) continue;
        const uint4 rec = a.tri_shade[prim];
        const AbsorbDev e = a.table[rec.w];
        if (!e.absorbing) continue;
        const ShadeGeomDev& gi = a.shade_geoms[rec.w];
        const bool identity = gi.identity != 0u;
        float m9[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
        if (!identity) {
#pragma unroll
            for (int k = 0; k < 9; k++) m9[k] = gi.m[k];
        }
        const V3 d = v3(rd.x, rd.y, rd.z);
        const V3 nrm = absorb_normal(rec, hrec.y, hrec.z, identity, m9);
        if (!(dot(nrm, d) > 0.0f)) continue;
        const AbsorbOutcome r = absorb_rule(v3(a.T[i], a.T[S + i], a.T[2 * S + i]), v3(e.sigma[0], e.sigma[1], e.sigma[2]), hrec.x, d, nrm);
        a.T[i] = r.T.x;
        a.T[S + i] = r.T.y;
        a.T[2 * S + i] = r.T.z;
    }
}
// self-test op 36: {T rgb, sigma rgb, t, d xyz, n xyz} -> {T' rgb, applied}
__global__ void k_selftest_absorb(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* p = in + kSelftestAbsorbIn * (size_t)i;
    auto F = [](uint32_t u) { return __uint_as_float(u); };
    const AbsorbOutcome r = absorb_rule(v3(F(p[0]), F(p[1]), F(p[2])), v3(F(p[3]), F(p[4]), F(p[5])), F(p[6]), v3(F(p[7]), F(p[8]), F(p[9])),
                                        v3(F(p[10]), F(p[11]), F(p[12])));
    uint32_t* o = out + kSelftestAbsorbOut * (size_t)i;
    o[0] = __float_as_uint(r.T.x); o[1] = __float_as_uint(r.T.y); o[2] = __float_as_uint(r.T.z);
    o[3] = r.applied ? 1u : 0u;
}

void launch_absorb(hipStream_t st, const AbsorbLaunch& a, uint32_t n_max, uint32_t groups) {
    const unsigned grid = groups ? groups : grid_for(n_max, kAbsorbBlock, kAbsorbMaxBlocks);
    hipLaunchKernelGGL(k_absorb, dim3(grid), dim3(kAbsorbBlock), 0, st, a);
}
void launch_selftest_absorb(hipStream_t st, const uint32_t* in, uint32_t n, uint32_t* out) {
    hipLaunchKernelGGL(k_selftest_absorb, dim3((n + 255) / 256), dim3(256), 0, st, in, n, out);
}

}  // namespace rt3
