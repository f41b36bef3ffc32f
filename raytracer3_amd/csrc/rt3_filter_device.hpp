// rt3_filter_device.hpp -- what the image-space filters ("denoise", rt3_denoise.hip; "temporal", rt3_temporal.hip) share: the per-pixel
// surface record of DESIGN.md section 4f stage 1 (world position, normal, albedo / emission modulation, the demodulated signal and its
// luminance), the two places such a record comes from -- the pinhole G-buffer (DnGbuffer) and the guide images of a lens or glass frame
// (DnGuide, DESIGN.md sections 4u and 4v) -- and the 32 x 8 launch tile.  One definition of every rule, so that both passes and both
// sources round alike: the numpy restatements (tests/ref_denoise.py prepare(), tests/ref_guide.py prepare_guide()) state each expression
// once as well.  The kernels take the source as a template parameter.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt3_camera.hpp"
#include "rt3_math.hpp"

namespace rt3 {

constexpr int kDnTileX = 32, kDnTileY = 8;  // one 256-thread workgroup; a wave covers two 32-pixel rows (512 B per record stream and row)
constexpr float kDnAlbedoFloor = 1.0f / 256.0f;

RT3_DEV float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

RT3_DEV V3 dn_albedo_floor(V3 a) {
    return v3(a.x > kDnAlbedoFloor ? a.x : kDnAlbedoFloor, a.y > kDnAlbedoFloor ? a.y : kDnAlbedoFloor, a.z > kDnAlbedoFloor ? a.z : kDnAlbedoFloor);
}
// world position of pixel (px, py) at depth t under camera g
RT3_DEV V3 dn_position(const GConstDev& g, uint32_t px, uint32_t py, float t) {
    V3 o, d;
    primary_ray(g, px, py, o, d);
    return v3(o.x + d.x * t, o.y + d.y * t, o.z + d.z * t);
}
struct DnModulation {
    V3 m, e;  // m = max(albedo, 1/256), e = emission: Out = e + c * m
};
RT3_DEV V3 dn_demodulate(const float4& L, const DnModulation& k) { return v3((L.x - k.e.x) / k.m.x, (L.y - k.e.y) / k.m.y, (L.z - k.e.z) / k.m.z); }
RT3_DEV V3 dn_modulate(V3 c, const DnModulation& k) { return v3(k.e.x + c.x * k.m.x, k.e.y + c.y * k.m.y, k.e.z + c.z * k.m.z); }

struct DnSurface {
    V3 P, n;  // world position, unit normal
    DnModulation k;
};

// A source of surface records.  fetch() loads what the foreground test of pixel pi needs (the texel); unit_normal() and world_position()
// take that texel back and load the rest, so a pixel or a tap that is rejected early costs the fewest bytes; surface() is the whole
// record of a foreground pixel.  modulation() gives m = max(albedo, 1/256) and e = emission, or m = 1 and e = 0 with
// RT3_DENOISE_NO_DEMODULATION / RT3_TEMPORAL_NO_DEMODULATION (bit 0 of flags).  prepared() is the foreground test once a pass has written
// the record image gP {P.xyz, 1 = foreground}: whichever costs fewer bytes.

// The pinhole G-buffer: foreground by the depth (4 B); normal, albedo and emission unpacked from the pixel's four words; the position
// reconstructed along the primary ray of camera g.
struct DnGbuffer {
    const uint4* gbuffer;
    const float* depth;
    typedef float Texel;  // the depth
    RT3_DEV Texel fetch(size_t pi) const { return depth[pi]; }
    RT3_DEV bool foreground(Texel t) const { return t != kBackgroundDepth; }
    RT3_DEV bool prepared(const float4*, size_t pi) const { return foreground(fetch(pi)); }
    RT3_DEV V3 unit_normal(size_t pi, Texel) const { return unpack_normal_11_10_11(gbuffer[pi].y); }
    RT3_DEV V3 world_position(const GConstDev& g, uint32_t px, uint32_t py, Texel t) const { return dn_position(g, px, py, t); }
    RT3_DEV static DnModulation modulation(uint32_t flags, const uint4& w) {
        V3 m = v3(1.0f, 1.0f, 1.0f), e = v3(0.0f, 0.0f, 0.0f);
        if (!(flags & 1u)) {
            m = dn_albedo_floor(unpack_color_888(w.x));
            e = rgb9e5_to_float3(w.w);
        }
        return {m, e};
    }
    RT3_DEV DnModulation modulation(uint32_t flags, size_t pi) const { return modulation(flags, gbuffer[pi]); }
    RT3_DEV DnSurface surface(const GConstDev& g, uint32_t flags, uint32_t px, uint32_t py, size_t pi, Texel t) const {
        const uint4 w = gbuffer[pi];  // by value: the words are loaded here, not under modulation()'s branch, which costs registers
        DnSurface s;
        s.k = modulation(flags, w);
        s.n = unpack_normal_11_10_11(w.y);
        s.P = world_position(g, px, py, t);
        return s;
    }
};

// The guide images {position, normal, albedo, emission} of a lens or glass frame, the means over the camera samples (rt3_guide.hip).  A
// pixel is foreground iff every sample hit (position.w == 1) and the summed normal has a finite, positive squared length l2; then P =
// position.xyz and n = normal.xyz * (1 / sqrtf(l2)) (rt3_math.hpp's normalize), unquantised: what the lens frame shaded.  The texel is
// position and normal (32 B); it keeps only the lanes that are read (normal.w is not: a 12-byte load).
struct DnGuide {
    const float4 *position, *normal, *albedo, *emission;
    struct Texel {
        V3 P, N;
        float cover, l2;
    };
    RT3_DEV Texel fetch(size_t pi) const {
        const float4 GP = position[pi], GN = normal[pi];
        const V3 N = v3(GN.x, GN.y, GN.z);
        return {v3(GP.x, GP.y, GP.z), N, GP.w, dot(N, N)};
    }
    RT3_DEV bool foreground(const Texel& x) const { return x.cover == 1.0f && x.l2 > 0.0f && x.l2 <= kFloatMax; }
    RT3_DEV bool prepared(const float4* gP, size_t pi) const { return gP[pi].w != 0.0f; }
    RT3_DEV V3 unit_normal(size_t, const Texel& x) const {
        const float inv = 1.0f / sqrtf(x.l2);
        return v3(x.N.x * inv, x.N.y * inv, x.N.z * inv);
    }
    RT3_DEV V3 world_position(const GConstDev&, uint32_t, uint32_t, const Texel& x) const { return x.P; }
    RT3_DEV DnModulation modulation(uint32_t flags, size_t pi) const {
        V3 m = v3(1.0f, 1.0f, 1.0f), e = v3(0.0f, 0.0f, 0.0f);
        if (!(flags & 1u)) {
            const float4 a = albedo[pi], em = emission[pi];
            m = dn_albedo_floor(v3(a.x, a.y, a.z));
            e = v3(em.x, em.y, em.z);
        }
        return {m, e};
    }
    RT3_DEV DnSurface surface(const GConstDev& g, uint32_t flags, uint32_t px, uint32_t py, size_t pi, const Texel& x) const {
        DnSurface s;
        s.n = unit_normal(pi, x);
        s.P = world_position(g, px, py, x);
        s.k = modulation(flags, pi);
        return s;
    }
};

inline dim3 dn_grid(uint32_t W, uint32_t H) { return dim3((W + kDnTileX - 1) / kDnTileX, (H + kDnTileY - 1) / kDnTileY); }

}  // namespace rt3
