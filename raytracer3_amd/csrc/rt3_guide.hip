// rt3_guide.hip -- guide images of a lens frame (rt3_camera_set_guide_output): per listed pixel the means of the
// first-vertex features over the frame's camera samples, which "denoise" can take as its guide (rt3_denoise_set_guide_input) where the
// pinhole G-buffer at pixel centres describes the wrong surface.
//   k_lens_rays -> k_extend -> [k_lens_miss] -> k_lens_guide -> k_shade<FIRST = false>(bounce 0) -> ...      ("refrence_mode" with a lens)
// The kernel reads the camera queue and its hit queue between the launches that write and consume them, and writes nothing the path
// tracer reads: the frame's Light has the bits it has without it.
//
// Arithmetic contract: tests/ref_guide.py accumulate() restates the sums in numpy float32 -- one rounding per written operation, no
// contraction, samples in ascending order whatever the batch size (between batches the images hold the running sums, the hit count in
// position.w), IEEE divisions at the end.
#include <hip/hip_runtime.h>

#include "rt3_internal.hpp"
#include "rt3_math.hpp"
#include "rt3_surface.hpp"

namespace rt3 {

// One thread per listed pixel, grid-stride.  For a fixed sample the wave reads 64 consecutive 16-byte records of the hit queue and of both
// planes of the camera queue: three coalesced 1 KiB streams, issued together ahead of hit_info's dependent gathers (shading record ->
// geometry entry -> texels).  52 bytes read per sample, 64 bytes written per pixel (and read again from the second batch on); no LDS, no
// atomics, no barrier: a thread writes its own pixel only, so the result does not depend on the launch shape.
__global__ __launch_bounds__(256) void k_lens_guide(SceneDev sc, const uint32_t* __restrict__ pixels, uint32_t npix, uint32_t width,
                                                    const float* __restrict__ rays, const float* __restrict__ hits, size_t stride, uint32_t nsb,
                                                    int first_batch, int last_batch, float samples, float4* __restrict__ position,
                                                    float4* __restrict__ normal, float4* __restrict__ albedo, float4* __restrict__ emission) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        const uint32_t xy = pixels[i];
        const size_t pi = (size_t)(xy >> 16) * width + (xy & 0xFFFFu);
        float4 aP = make_float4(0.0f, 0.0f, 0.0f, 0.0f), aN = aP, aA = aP, aE = aP;
        if (!first_batch) {
            aP = position[pi];
            aN = normal[pi];
            aA = albedo[pi];
            aE = emission[pi];
        }
        for (uint32_t s = 0; s < nsb; s++) {
            const size_t p = (size_t)s * npix + i;
            const float4 h = reinterpret_cast<const float4*>(hits)[p];
            const float4 ro = reinterpret_cast<const float4*>(rays)[p];
            const float4 rd = reinterpret_cast<const float4*>(rays)[stride + p];
            const uint32_t prim = __float_as_uint(h.w);
            if (prim == kMiss) {  // the sky is not albedo-modulated
                aA.x = aA.x + 1.0f;
                aA.y = aA.y + 1.0f;
                aA.z = aA.z + 1.0f;
                continue;
            }
            const Surface sf = hit_info(sc, prim, h.y, h.z);
            aP.x = aP.x + (ro.x + rd.x * h.x);
            aP.y = aP.y + (ro.y + rd.y * h.x);
            aP.z = aP.z + (ro.z + rd.z * h.x);
            aP.w = aP.w + 1.0f;
            aN.x = aN.x + sf.normal.x;
            aN.y = aN.y + sf.normal.y;
            aN.z = aN.z + sf.normal.z;
            aA.x = aA.x + sf.albedo.x;
            aA.y = aA.y + sf.albedo.y;
            aA.z = aA.z + sf.albedo.z;
            aE.x = aE.x + sf.emissive.x;
            aE.y = aE.y + sf.emissive.y;
            aE.z = aE.z + sf.emissive.z;
        }
        if (last_batch) {
            const float nh = aP.w;
            if (nh > 0.0f) {
                aP = make_float4(aP.x / nh, aP.y / nh, aP.z / nh, nh / samples);
                aN = make_float4(aN.x / nh, aN.y / nh, aN.z / nh, 0.0f);
            } else {
                aP = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                aN = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            aA = make_float4(aA.x / samples, aA.y / samples, aA.z / samples, 0.0f);
            aE = make_float4(aE.x / samples, aE.y / samples, aE.z / samples, 0.0f);
        }
        position[pi] = aP;
        normal[pi] = aN;
        albedo[pi] = aA;
        emission[pi] = aE;
    }
}

void launch_lens_guide(hipStream_t st, const GuideLaunch& a, uint32_t groups) {
    const unsigned grid = groups ? groups : grid_for(a.npix, 256, 8192);
    hipLaunchKernelGGL(k_lens_guide, dim3(grid), dim3(256), 0, st, a.sc, a.pixels, a.npix, a.width, a.rays, a.hits, a.stride, a.nsb, a.first_batch ? 1 : 0,
                       a.last_batch ? 1 : 0, (float)a.samples, a.img[0], a.img[1], a.img[2], a.img[3]);
}

}  // namespace rt3
