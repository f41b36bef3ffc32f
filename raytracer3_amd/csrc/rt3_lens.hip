// rt3_lens.hip -- per-sample camera rays (rt3_camera_set_lens): the kernels a lens frame runs beside the path tracer's.
//   k_lens_rays -> k_extend -> [k_lens_miss] -> k_shade<FIRST = false>(bounce 0) -> ... -> k_accumulate_lens   ("refrence_mode" with a lens)
//   k_postprocess_lens                                                                                        ("postprocess" with a lens)
// Vertex 0 of a lens frame is a hit record of k_extend's queue like every later vertex; the G-buffer is not read.
#include <hip/hip_runtime.h>

#include "rt3_camera.hpp"
#include "rt3_internal.hpp"
#include "rt3_math.hpp"
#include "rt3_sky.hpp"
#include "rt3_surface.hpp"
#include "rt3_tonemap.hpp"

namespace rt3 {

// The camera rays of one batch, in path order (pid = sample_in_batch * npix + pixel index), as records of the path tracer's extension queue:
// {o, pdf} {d, pid}, throughput 1, radiance 0.  The pdf slot holds FLT_MAX: a camera ray is a delta "sample", and k_shade's MIS weights
// pdf_b / (pdf_b + p_light) -- an emitter seen directly, the sky behind an escaped ray -- are then exactly 1 while p_light stays below half
// an ulp of FLT_MAX, 2^103.  The sky's density is bounded by its texels and is far below that.  For the emitter branch it is an assumption:
// p_light = p_sel / area * dist^2 / |cos| has no bound as the emitter is seen edge-on; beyond 2^103 the weight is no longer 1, and once
// the sum overflows it is 0.  That takes |cos| below 1e-31 p_sel / area * dist^2: not met in practice, not excluded.
// One thread also writes the queue's length, which the launches that follow read from the device.
// Streaming: 4 bytes read and 60 written per path (16 + 16 + 3 x 4 + 16), 16-byte stores but for the three throughput planes; no LDS.
__global__ __launch_bounds__(256) void k_lens_rays(GConstDev g, LensDev lens, const uint32_t* __restrict__ pixels, uint32_t npix, FastDiv npix_div,
                                                   uint32_t s0, uint32_t n_first, float* __restrict__ rays, float* __restrict__ T,
                                                   float* __restrict__ lacc, size_t stride, uint32_t* __restrict__ count) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = n_first;
    for (uint32_t pid = blockIdx.x * blockDim.x + threadIdx.x; pid < n_first; pid += gridDim.x * blockDim.x) {
        const uint32_t s = fast_div(npix_div, pid);
        const uint32_t xy = pixels[pid - s * npix];
        const LensSample r = lens_ray(g, lens, xy & 0xFFFFu, xy >> 16, s0 + s);
        reinterpret_cast<float4*>(rays)[pid] = make_float4(r.o.x, r.o.y, r.o.z, kFloatMax);
        reinterpret_cast<float4*>(rays)[stride + pid] = make_float4(r.d.x, r.d.y, r.d.z, __uint_as_float(pid));
        T[pid] = 1.0f;
        T[stride + pid] = 1.0f;
        T[2 * stride + pid] = 1.0f;
        reinterpret_cast<float4*>(lacc)[pid] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// Escaped camera samples of a frame whose k_shade does not collect the sky (no RT3_F_NEE_SKY): the sky's bilinear radiance along the ray, the
// value "postprocess" shows behind a pinhole frame.  Record i of the camera queue is path i; its radiance is still 0 and its throughput 1.
__global__ __launch_bounds__(256) void k_lens_miss(SceneDev sc, const float* __restrict__ rays, const float* __restrict__ hits,
                                                   float* __restrict__ lacc, size_t stride, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 hrec = reinterpret_cast<const float4*>(hits)[i];
        if (__float_as_uint(hrec.w) != kMiss) continue;
        const float4 rd = reinterpret_cast<const float4*>(rays)[stride + i];
        float su, sv;
        direction_to_equirect_uv(v3(rd.x, rd.y, rd.z), su, sv);
        const V3 rad = sky_eval(sc, su, sv);
        reinterpret_cast<float4*>(lacc)[i] = make_float4(rad.x, rad.y, rad.z, 0.0f);
    }
}

// k_accumulate (rt3_shade.hip) for every listed pixel: a pixel whose centre sees the background may be partly covered
__global__ void k_accumulate_lens(GConstDev g, const uint32_t* __restrict__ pixels, uint32_t npix, uint32_t width, const float* __restrict__ lacc,
                                  uint32_t sb, int first_batch, int last_batch, float* __restrict__ radsum, float4* __restrict__ light,
                                  const float4* __restrict__ prev) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        uint32_t xy = pixels[i];
        size_t pi = (size_t)(xy >> 16) * width + (xy & 0xFFFFu);
        float r = first_batch ? 0.0f : radsum[i], gg = first_batch ? 0.0f : radsum[npix + i], bb = first_batch ? 0.0f : radsum[2 * (size_t)npix + i];
        for (uint32_t s = 0; s < sb; s++) {
            size_t p = (size_t)s * npix + i;
            const float4 lv = reinterpret_cast<const float4*>(lacc)[p];
            r += lv.x;
            gg += lv.y;
            bb += lv.z;
        }
        if (!last_batch) {
            radsum[i] = r;
            radsum[npix + i] = gg;
            radsum[2 * (size_t)npix + i] = bb;
        } else {
            float fs = (float)g.samples;
            r = r / fs;
            gg = gg / fs;
            bb = bb / fs;
            if (g.blendfactor >= 1.0f) {
                light[pi] = make_float4(r, gg, bb, 0.0f);
            } else {
                float4 pv = prev[pi];
                float bf = g.blendfactor;
                light[pi] = make_float4(pv.x + (r - pv.x) * bf, pv.y + (gg - pv.y) * bf, pv.z + (bb - pv.z) * bf, 0.0f);
            }
        }
    }
}

// k_postprocess (rt3_frame.hip) with every pixel taken from In: the sky is part of a lens frame's Light already
__global__ void k_postprocess_lens(const uint32_t* __restrict__ pixels, uint32_t npix, uint32_t width, const float4* __restrict__ in,
                                   float4* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        uint32_t xy = pixels[i];
        size_t pi = (size_t)(xy >> 16) * width + (xy & 0xFFFFu);
        float4 c = in[pi];
        V3 r = agx_tonemap(v3(c.x, c.y, c.z));
        out[pi] = make_float4(r.x, r.y, r.z, 1.0f);
    }
}

// self-test op 31: {proj_inverse[16], view_inverse[16], window_size[2], aperture_radius, focus_distance, pixel_jitter, px, py, frame, sm}
// -> {o, d, film point (pixels), lens point (view space)}
__global__ void k_selftest_lens(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* p = in + kSelftestLensIn * (size_t)i;
    GConstDev g = {};
    for (int k = 0; k < 16; k++) {
        g.proj_inverse[k] = __uint_as_float(p[k]);
        g.view_inverse[k] = __uint_as_float(p[16 + k]);
    }
    g.window_size[0] = __uint_as_float(p[32]);
    g.window_size[1] = __uint_as_float(p[33]);
    g.frame = p[39];
    LensDev L;
    L.aperture_radius = __uint_as_float(p[34]);
    L.focus_distance = __uint_as_float(p[35]);
    L.pixel_jitter = __uint_as_float(p[36]);
    const LensSample r = lens_ray(g, L, p[37], p[38], p[40]);
    uint32_t* o = out + kSelftestLensOut * (size_t)i;
    o[0] = __float_as_uint(r.o.x); o[1] = __float_as_uint(r.o.y); o[2] = __float_as_uint(r.o.z);
    o[3] = __float_as_uint(r.d.x); o[4] = __float_as_uint(r.d.y); o[5] = __float_as_uint(r.d.z);
    o[6] = __float_as_uint(r.fx); o[7] = __float_as_uint(r.fy);
    o[8] = __float_as_uint(r.lx); o[9] = __float_as_uint(r.ly);
}

// ------------------------------------------------------------------------------------------------ launchers
void launch_lens_rays(hipStream_t st, const GConstDev& g, const LensDev& lens, const uint32_t* pixels, uint32_t npix, uint32_t s0, uint32_t n_first,
                      float* rays, float* T, float* lacc, size_t stride, uint32_t* count) {
    hipLaunchKernelGGL(k_lens_rays, dim3(grid_for(n_first, 256, 8192)), dim3(256), 0, st, g, lens, pixels, npix, make_fastdiv(npix), s0, n_first, rays, T,
                       lacc, stride, count);
}
void launch_lens_miss(hipStream_t st, const SceneDev& sc, const float* rays, const float* hits, float* lacc, size_t stride, uint32_t n) {
    hipLaunchKernelGGL(k_lens_miss, dim3(grid_for(n, 256, 8192)), dim3(256), 0, st, sc, rays, hits, lacc, stride, n);
}
void launch_accumulate_lens(hipStream_t st, const GConstDev& g, const uint32_t* pixels, uint32_t npix, uint32_t width, const float* lacc, uint32_t sb,
                            int first_batch, int last_batch, float* radsum, void* light, const void* prev) {
    hipLaunchKernelGGL(k_accumulate_lens, dim3(grid_for(npix, 256, 8192)), dim3(256), 0, st, g, pixels, npix, width, lacc, sb, first_batch, last_batch,
                       radsum, (float4*)light, (const float4*)prev);
}
void launch_postprocess_lens(hipStream_t st, const uint32_t* pixels, uint32_t npix, uint32_t width, const void* in, void* out) {
    hipLaunchKernelGGL(k_postprocess_lens, dim3(grid_for(npix, 256, 8192)), dim3(256), 0, st, pixels, npix, width, (const float4*)in, (float4*)out);
}
void launch_selftest_lens(hipStream_t st, const uint32_t* in, uint32_t n, uint32_t* out) {
    hipLaunchKernelGGL(k_selftest_lens, dim3((n + 255) / 256), dim3(256), 0, st, in, n, out);
}

}  // namespace rt3
