// rt3_camera.hpp -- the frame constants and the primary ray of a pixel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt3_math.hpp"

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

}  // namespace rt3
