// rt3_guide.hip -- guide images of a lens frame (rt3_camera_set_guide_output): per listed pixel the means of the
// first-vertex features over the frame's camera samples, which "denoise" can take as its guide (rt3_denoise_set_guide_input) where the
// pinhole G-buffer at pixel centres describes the wrong surface.
//   k_lens_rays -> k_extend -> [k_lens_miss] -> k_lens_guide -> [k_lens_guide_prev] -> k_shade<FIRST = false>(bounce 0) -> ...
//                                                                                                         ("refrence_mode" with a lens)
// The kernels read the camera queue and its hit queue between the launches that write and consume them, and write nothing the path
// tracer reads: the frame's Light has the bits it has without them.  k_lens_guide_prev (rt3_camera_set_guide_motion_output, DESIGN.md
// section 4w) writes a fifth image, the samples' mean previous position, which "temporal" looks up in the previous frame when instances
// move or meshes deform under a lens (rt3_temporal_set_guide_motion_input).
//
// Arithmetic contract: tests/ref_guide.py accumulate() restates the sums in numpy float32 -- one rounding per written operation, no
// contraction, samples in ascending order whatever the batch size (between batches the images hold the running sums, the hit count in
// position.w), IEEE divisions at the end.
#include <hip/hip_runtime.h>

#include "rt3_bvh_device.hpp"
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

// The fifth image (rt3_camera_set_guide_motion_output): per listed pixel the mean over the hit samples of where each
// sample's surface point was one frame ago, {sum R / n_hit, n_hit / S}; tests/ref_guide_motion.py accumulate_prev() restates it.  R follows
// the slot of the hit geometry like k_motion's texel (rt3_motion.hip): unmoved -> o + d t, the addend k_lens_guide gives sum P, bit for
// bit; moved -> prev_i * ((a w + b u) + c v) over the object-space corners; deformed -> the same over the snapshot's records.
// k_lens_guide's shape: one thread per listed pixel, grid-stride; per sample the hit record and both ray planes are three coalesced 1 KiB
// streams per wave, issued together ahead of the dependent prim_geom -> slot pair.  Only lanes on moved or deformed geometry go on to
// first_prim, the geometry's two offsets, three indices, three vertices (or snapshot records) and the 64-byte previous matrix; lanes of a
// wave on one instance read the same lines of the small tables.  48 bytes read per sample (plus those gathers), 16 bytes written per pixel
// (and read again from the second batch on); no LDS, no atomics, no barrier, and hit_info is not called.  m.geom_slot and prev_pos are
// kernel arguments: the branches on them are wave-uniform.
__global__ __launch_bounds__(256) void k_lens_guide_prev(MotionDev m, const float4* __restrict__ prev_pos, const uint32_t* __restrict__ pixels, uint32_t npix,
                                                         uint32_t width, const float* __restrict__ rays, const float* __restrict__ hits, size_t stride,
                                                         uint32_t nsb, int first_batch, int last_batch, float samples, float4* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        const uint32_t xy = pixels[i];
        const size_t pi = (size_t)(xy >> 16) * width + (xy & 0xFFFFu);
        float4 aR = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (!first_batch) aR = out[pi];
        for (uint32_t s = 0; s < nsb; s++) {
            const size_t p = (size_t)s * npix + i;
            const float4 h = reinterpret_cast<const float4*>(hits)[p];
            const float4 ro = reinterpret_cast<const float4*>(rays)[p];
            const float4 rd = reinterpret_cast<const float4*>(rays)[stride + p];
            const uint32_t prim = __float_as_uint(h.w);
            if (prim == kMiss) continue;
            const uint32_t slot = m.geom_slot ? m.geom_slot[m.prim_geom[prim]] : kMotionUnmoved;
            V3 R;
            if (slot == kMotionUnmoved) {
                R = v3(ro.x + rd.x * h.x, ro.y + rd.y * h.x, ro.z + rd.z * h.x);
            } else {
                V3 a, b, c;
                if (prev_pos != nullptr && (slot & kMotionDeformed))
                    fetch_triangle_snapshot(prev_pos, m.indices, m.geoms, m.prim_geom, m.first_prim, prim, a, b, c);
                else
                    fetch_triangle_object(m.verts, m.indices, m.geoms, m.prim_geom, m.first_prim, prim, a, b, c);
                const float u = h.y, v = h.z, w = (1.0f - u) - v;  // k_motion's pairing
                R = v3((a.x * w + b.x * u) + c.x * v, (a.y * w + b.y * u) + c.y * v, (a.z * w + b.z * u) + c.z * v);
                const MotionPrevDev& pm = m.prev[slot & ~kMotionDeformed];
                if (!pm.identity) R = transform_point(pm.m, R);
            }
            aR.x = aR.x + R.x;
            aR.y = aR.y + R.y;
            aR.z = aR.z + R.z;
            aR.w = aR.w + 1.0f;
        }
        if (last_batch) {
            const float nh = aR.w;
            aR = nh > 0.0f ? make_float4(aR.x / nh, aR.y / nh, aR.z / nh, nh / samples) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        out[pi] = aR;
    }
}

void launch_lens_guide_prev(hipStream_t st, const GuidePrevLaunch& a, uint32_t groups) {
    const unsigned grid = groups ? groups : grid_for(a.npix, 256, 8192);
    hipLaunchKernelGGL(k_lens_guide_prev, dim3(grid), dim3(256), 0, st, a.m, a.prev_pos, a.pixels, a.npix, a.width, a.rays, a.hits, a.stride, a.nsb,
                       a.first_batch ? 1 : 0, a.last_batch ? 1 : 0, (float)a.samples, a.out);
}

}  // namespace rt3
