// rt3_camera.hpp -- the frame constants, the primary ray of a pixel and the per-sample camera ray of a lens frame.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt3_math.hpp"
#include "rt3_rng.hpp"

namespace rt3 {

// ------------------------------------------------------------------------------------------------ camera / primary ray
struct GConstDev {  // == rt3_gconst (renderer/mod.rs:47-63)
    float proj[16], view[16], proj_inverse[16], view_inverse[16];
    float window_size[2];
    uint32_t frame;
    float blendfactor;
    uint32_t bounces, samples, proberng;
    float cell_size;
    uint32_t mouse[2], pad[2];
};
static_assert(sizeof(GConstDev) == 304, "GConst layout");

// gbuffer_helpers.slang:85-103 (view_dir + setupPrimaryRay); pixel (0,0) top-left, upright image (d.y flipped)
RT3_DEV void primary_ray(const GConstDev& g, uint32_t px, uint32_t py, V3& o, V3& d) {
    float cx = ((float)px + 0.5f) / g.window_size[0], cy = ((float)py + 0.5f) / g.window_size[1];
    float dx = cx * 2.0f - 1.0f, dy = -(cy * 2.0f - 1.0f);
    const float* m = g.proj_inverse;
    V3 target = v3(m[0] * dx + m[4] * dy + m[8] * 1.0f + m[12] * 1.0f, m[1] * dx + m[5] * dy + m[9] * 1.0f + m[13] * 1.0f,
                   m[2] * dx + m[6] * dy + m[10] * 1.0f + m[14] * 1.0f);
    V3 t = normalize(target);
    const float* w = g.view_inverse;
    d = v3(w[0] * t.x + w[4] * t.y + w[8] * t.z + w[12] * 0.0f, w[1] * t.x + w[5] * t.y + w[9] * t.z + w[13] * 0.0f,
           w[2] * t.x + w[6] * t.y + w[10] * t.z + w[14] * 0.0f);
    o = v3(w[12], w[13], w[14]);
}

// ------------------------------------------------------------------------------------------------ per-sample camera ray
struct LensDev {  // rt3_lens_params as the kernels see it (rt3_camera_set_lens)
    float aperture_radius, focus_distance, pixel_jitter;
};
struct LensSample {
    V3 o, d;        // world-space ray
    float fx, fy;   // the film point, in pixels (pixel (px, py) covers [px, px + 1) x [py, py + 1))
    float lx, ly;   // the lens point, in view space (z = 0)
};
// first RNG index of the camera dimensions: the path's vertices use indices below samples * bounces * 8 <= 2^31
constexpr uint32_t kLensRngBase = 0x80000000u;
// Sample `sm` of pixel (px, py): dims kLensRngBase + 4 sm + {0, 1} pick the film point in the box of width pixel_jitter around the pixel
// centre, dims + {2, 3} the point on the lens disk (uniform: r = R sqrt(u2), phi = 2 pi u3); no blue-noise shift.  The ray leaves the lens
// point towards the point where the pinhole ray through the film point meets the plane of focus, view depth focus_distance.
// aperture_radius = 0 and pixel_jitter = 0 is primary_ray, bit for bit (its own branch).
RT3_DEV LensSample lens_ray(const GConstDev& g, const LensDev& L, uint32_t px, uint32_t py, uint32_t sm) {
    LensSample r;
    r.lx = r.ly = 0.0f;
    if (L.aperture_radius == 0.0f && L.pixel_jitter == 0.0f) {
        r.fx = (float)px + 0.5f;
        r.fy = (float)py + 0.5f;
        primary_ray(g, px, py, r.o, r.d);
        return r;
    }
    const uint32_t seed = rng_seed(px, py, g.frame), idx = kLensRngBase + 4u * sm;
    const float u0 = uniform_float(seed, idx), u1 = uniform_float(seed, idx + 1u);
    r.fx = ((float)px + 0.5f) + L.pixel_jitter * (u0 - 0.5f);
    r.fy = ((float)py + 0.5f) + L.pixel_jitter * (u1 - 0.5f);
    const float cx = r.fx / g.window_size[0], cy = r.fy / g.window_size[1];
    const float dx = cx * 2.0f - 1.0f, dy = -(cy * 2.0f - 1.0f);
    const float* m = g.proj_inverse;
    const V3 target = v3(m[0] * dx + m[4] * dy + m[8] * 1.0f + m[12] * 1.0f, m[1] * dx + m[5] * dy + m[9] * 1.0f + m[13] * 1.0f,
                         m[2] * dx + m[6] * dy + m[10] * 1.0f + m[14] * 1.0f);
    const V3 t = normalize(target);
    const float* w = g.view_inverse;
    V3 dv = t;
    if (L.aperture_radius != 0.0f) {
        const float u2 = uniform_float(seed, idx + 2u), u3 = uniform_float(seed, idx + 3u);
        const float rad = L.aperture_radius * sqrtf(u2);
        float sn, cs;
        sincos_2pi(u3, sn, cs);
        r.lx = rad * cs;
        r.ly = rad * sn;
        const V3 Pv = t * (L.focus_distance / -t.z);  // the focus point: view depth focus_distance along the pinhole direction
        dv = normalize(v3(Pv.x - r.lx, Pv.y - r.ly, Pv.z));
    }
    r.d = v3(w[0] * dv.x + w[4] * dv.y + w[8] * dv.z, w[1] * dv.x + w[5] * dv.y + w[9] * dv.z, w[2] * dv.x + w[6] * dv.y + w[10] * dv.z);
    r.o = v3(w[0] * r.lx + w[4] * r.ly + w[12], w[1] * r.lx + w[5] * r.ly + w[13], w[2] * r.lx + w[6] * r.ly + w[14]);
    return r;
}

}  // namespace rt3
