// rt3_frame.hip -- the per-pixel kernels around the path tracer: raygen, gbuffer, pixbn, postprocess and the tile pack / unpack.
//
// The wavefront path-tracing kernels (hand-written HIP, wave64) are split by stage: traversal in rt3_trace.hip, shading in rt3_shade.hip.
// Pipeline (replaces shaders/old/{gbuffer,refrence_mode,postprocess}.slang + the driver's ray traversal):
//   k_raygen -> k_extend -> k_gbuffer                                   ("gbuffer" pass)
//   k_shade<first> -> [k_shadow] -> [k_roulette] -> k_extend -> [k_absorb] -> k_shade -> ... -> k_accumulate   ("refrence_mode" pass)
//   k_postprocess                                                        ("postprocess" pass)
// All queues are structure-of-arrays of 16-byte records (ray = {o, tmin} + {d, tmax}, state = {T, pdf}, hit = {t, u, v, prim};
// shadow ray = {o, contribution.r} + {d, contribution.g} + 8 bytes {contribution.b, path id}): lane i touches record i of each
// stream, 1 KiB per wave instruction, the widest coalesced access; live rays are compacted with __ballot / popcount, one
// 64-bit atomic per workgroup for both output queues.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "rt3_camera.hpp"
#include "rt3_internal.hpp"
#include "rt3_math.hpp"
#include "rt3_sky.hpp"
#include "rt3_surface.hpp"
#include "rt3_tonemap.hpp"

namespace rt3 {

// ------------------------------------------------------------------------------------------------ gbuffer pass
// gbuffer.slang:8-12 : primary rays for the pixels this rank owns (pixel list is in tile / Z-curve order)
__global__ void k_raygen(GConstDev g, const uint32_t* __restrict__ pixels, uint32_t npix, float* __restrict__ rays, size_t stride) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        uint32_t xy = pixels[i];
        V3 o, d;
        primary_ray(g, xy & 0xFFFFu, xy >> 16, o, d);
        reinterpret_cast<float4*>(rays)[i] = make_float4(o.x, o.y, o.z, 0.0f);                         // TMin, gbuffer_helpers.slang:100
        reinterpret_cast<float4*>(rays)[stride + i] = make_float4(d.x, d.y, d.z, kBackgroundDepth);    // TMax, :101
    }
}
// gbuffer.slang:15-20
__global__ void k_gbuffer(SceneDev sc, const uint32_t* __restrict__ pixels, uint32_t npix, uint32_t width,
                          const float* __restrict__ hits, size_t stride, uint4* __restrict__ gbuffer, float* __restrict__ depth) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        uint32_t xy = pixels[i];
        size_t pi = (size_t)(xy >> 16) * width + (xy & 0xFFFFu);
        const float4 hrec = reinterpret_cast<const float4*>(hits)[i];
        uint32_t prim = __float_as_uint(hrec.w);
        if (prim == kMiss) {
            depth[pi] = kBackgroundDepth;
        } else {
            Surface s = hit_info(sc, prim, hrec.y, hrec.z);
            gbuffer[pi] = gbuffer_pack(s);
            depth[pi] = hrec.x;
        }
    }
}

// ------------------------------------------------------------------------------------------------ postprocess
// postprocess.slang:90-112
__global__ void k_postprocess(GConstDev g, SceneDev sc, const uint32_t* __restrict__ pixels, uint32_t npix, uint32_t width,
                              const float* __restrict__ depth, const float4* __restrict__ in, float4* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        uint32_t xy = pixels[i], px = xy & 0xFFFFu, py = xy >> 16;
        size_t pi = (size_t)py * width + px;
        V3 col;
        if (depth[pi] != kBackgroundDepth) {
            float4 c = in[pi];
            col = v3(c.x, c.y, c.z);
        } else {
            V3 o, d;
            primary_ray(g, px, py, o, d);
            float su, sv;
            direction_to_equirect_uv(d, su, sv);
            col = sky_eval(sc, su, sv);
        }
        V3 r = agx_tonemap(col);
        out[pi] = make_float4(r.x, r.y, r.z, 1.0f);
    }
}

// ------------------------------------------------------------------------------------------------ tiles
__global__ void k_pack_tiles(const uint32_t* __restrict__ pixels, uint32_t npix, uint32_t width, const float4* __restrict__ img,
                             float4* __restrict__ dst) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        uint32_t xy = pixels[i];
        dst[i] = img[(size_t)(xy >> 16) * width + (xy & 0xFFFFu)];
    }
}
__global__ void k_unpack_tiles(const uint32_t* __restrict__ pixels, uint32_t npix, uint32_t width, const float4* __restrict__ src,
                               float4* __restrict__ img) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        uint32_t xy = pixels[i];
        img[(size_t)(xy >> 16) * width + (xy & 0xFFFFu)] = src[i];
    }
}

// ------------------------------------------------------------------------------------------------ launchers
void launch_raygen(hipStream_t st, const GConstDev& g, const uint32_t* pixels, uint32_t npix, float* rays, size_t stride) {
    hipLaunchKernelGGL(k_raygen, dim3(grid_for(npix, 256, 4096)), dim3(256), 0, st, g, pixels, npix, rays, stride);
}
void launch_gbuffer(hipStream_t st, const SceneDev& sc, const uint32_t* pixels, uint32_t npix, uint32_t width, const float* hits,
                    size_t stride, void* gbuffer, float* depth) {
    hipLaunchKernelGGL(k_gbuffer, dim3(grid_for(npix, 256, 4096)), dim3(256), 0, st, sc, pixels, npix, width, hits, stride, (uint4*)gbuffer, depth);
}
__global__ void k_pixbn(const uint32_t* __restrict__ pixels, uint32_t npix, const uint8_t* __restrict__ bluenoise, uint32_t bn_w, uint32_t bn_h,
                        uint2* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        const uint32_t xy = pixels[i], px = xy & 0xFFFFu, py = xy >> 16;
        uint32_t bn = 0;
        if (bluenoise) bn = *reinterpret_cast<const uint32_t*>(bluenoise + 4 * ((size_t)(py % bn_h) * bn_w + (px % bn_w)));
        out[i] = make_uint2(xy, bn);
    }
}
void launch_pixbn(hipStream_t st, const uint32_t* pixels, uint32_t npix, const uint8_t* bluenoise, uint32_t bn_w, uint32_t bn_h, uint2* out) {
    hipLaunchKernelGGL(k_pixbn, dim3(grid_for(npix, 256, 4096)), dim3(256), 0, st, pixels, npix, bluenoise, bn_w, bn_h, out);
}
void launch_postprocess(hipStream_t st, const GConstDev& g, const SceneDev& sc, const uint32_t* pixels, uint32_t npix, uint32_t width,
                        const float* depth, const void* in, void* out) {
    hipLaunchKernelGGL(k_postprocess, dim3(grid_for(npix, 256, 8192)), dim3(256), 0, st, g, sc, pixels, npix, width, depth, (const float4*)in,
                       (float4*)out);
}
void launch_pack_tiles(hipStream_t st, const uint32_t* pixels, uint32_t npix, uint32_t width, const void* img, void* dst) {
    hipLaunchKernelGGL(k_pack_tiles, dim3(grid_for(npix, 256, 8192)), dim3(256), 0, st, pixels, npix, width, (const float4*)img, (float4*)dst);
}
void launch_unpack_tiles(hipStream_t st, const uint32_t* pixels, uint32_t npix, uint32_t width, const void* src, void* img) {
    hipLaunchKernelGGL(k_unpack_tiles, dim3(grid_for(npix, 256, 8192)), dim3(256), 0, st, pixels, npix, width, (const float4*)src, (float4*)img);
}

}  // namespace rt3
