// rt3_filter_device.hpp -- what the image-space filters ("denoise", rt3_denoise.hip; "temporal", rt3_temporal.hip) share: the per-pixel
// surface record of DESIGN.md section 4f stage 1 (world position from the depth and the camera, albedo / emission modulation from the
// G-buffer, the demodulated signal and its luminance) and the 32 x 8 launch tile.  One definition, so that both passes round alike: the
// numpy restatements (tests/ref_denoise.py prepare(), tests/ref_temporal.py) state each expression once as well.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt3_camera.hpp"
#include "rt3_math.hpp"

namespace rt3 {

constexpr int kDnTileX = 32, kDnTileY = 8;  // one 256-thread workgroup; a wave covers two 32-pixel rows (512 B per record stream and row)
constexpr float kDnAlbedoFloor = 1.0f / 256.0f;

RT3_DEV float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// m = max(albedo, 1/256) and e = emission of G-buffer word w; m = 1, e = 0 with RT3_DENOISE_NO_DEMODULATION / RT3_TEMPORAL_NO_DEMODULATION (bit 0)
RT3_DEV void dn_modulation(uint32_t flags, const uint4& w, V3& m, V3& e) {
    m = v3(1.0f, 1.0f, 1.0f);
    e = v3(0.0f, 0.0f, 0.0f);
    if (!(flags & 1u)) {
        const V3 a = unpack_color_888(w.x);
        m = v3(a.x > kDnAlbedoFloor ? a.x : kDnAlbedoFloor, a.y > kDnAlbedoFloor ? a.y : kDnAlbedoFloor, a.z > kDnAlbedoFloor ? a.z : kDnAlbedoFloor);
        e = rgb9e5_to_float3(w.w);
    }
}
// world position of pixel (px, py) at depth t under camera g
RT3_DEV V3 dn_position(const GConstDev& g, uint32_t px, uint32_t py, float t) {
    V3 o, d;
    primary_ray(g, px, py, o, d);
    return v3(o.x + d.x * t, o.y + d.y * t, o.z + d.z * t);
}
RT3_DEV V3 dn_demodulate(const float4& L, V3 e, V3 m) { return v3((L.x - e.x) / m.x, (L.y - e.y) / m.y, (L.z - e.z) / m.z); }
RT3_DEV V3 dn_modulate(V3 c, V3 e, V3 m) { return v3(e.x + c.x * m.x, e.y + c.y * m.y, e.z + c.z * m.z); }

inline dim3 dn_grid(uint32_t W, uint32_t H) { return dim3((W + kDnTileX - 1) / kDnTileX, (H + kDnTileY - 1) / kDnTileY); }

}  // namespace rt3
