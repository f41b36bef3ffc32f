// rt3_emit_tex.hpp -- textured emitters (rt3_scene_set_textured_emitters): the light table's side array, the emissive
// lookup of a point on an emitter, the quadrature rule of a textured emitter's selection mass, and k_emit_tex's argument.  No reference
// counterpart (the reference samples no emitter).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rt3_math.hpp"
#include "rt3_rng.hpp"
#include "rt3_surface.hpp"

namespace rt3 {

// One entry per entry of the light table, 32 bytes: the emitter's vertex uvs in fetch_triangle's vertex order (the order A, E1 = b - a,
// E2 = c - a of its record were made in, so the barycentrics (1 - b1 - b2, b1, b2) of a sampled point weight uv[0], uv[1], uv[2]) and its
// emissive texture; tex = -1 (and zeros): a punctual light, an emitter without an emissive texture, or one whose index is not uploaded
struct alignas(16) EmitTexDev {
    float2 uv[3];
    int32_t tex;
    uint32_t pad;
};
static_assert(sizeof(EmitTexDev) == 32, "EmitTex layout");

// the emissive texture at barycentrics (1 - b1 - b2, b1, b2) of emitter record t (t.tex >= 0): hit_finish<true>'s uv expression and lookup
RT3_DEV V3 emit_tex_rgb(const SceneDev& sc, const EmitTexDev& t, float b1, float b2) {
    float uu, vv;
    tri_uv_at(t.uv, 0u, 1.0f - b1 - b2, b1, b2, uu, vv);
    const TexQuad q = tex_quad(sc, (uint32_t)t.tex, uu, vv);
    return v3(quad_srgb(sc, q, 0), quad_srgb(sc, q, 1), quad_srgb(sc, q, 2));
}

// The quadrature of a textured emitter's mean texel (include/rt3.h has the rule).  L: the subdivision, from the longest uv edge in texels
constexpr uint32_t kEmitTexMaxL = 64;
RT3_DEV float emit_tex_edge(float2 a, float2 b, float W, float H) { return fmaxf(fabsf(b.x - a.x) * W, fabsf(b.y - a.y) * H); }
RT3_DEV uint32_t emit_tex_subdiv(const EmitTexDev& t, uint32_t W, uint32_t H) {
    const float fw = (float)W, fh = (float)H;
    const float e0 = emit_tex_edge(t.uv[0], t.uv[1], fw, fh), e1 = emit_tex_edge(t.uv[0], t.uv[2], fw, fh), e2 = emit_tex_edge(t.uv[1], t.uv[2], fw, fh);
    if (!(e0 <= kFloatMax && e1 <= kFloatMax && e2 <= kFloatMax)) return 1u;  // a non-finite edge (a NaN fails the comparison too)
    const float m = ceilf(fmaxf(e0, fmaxf(e1, e2)));
    if (!(m >= 1.0f)) return 1u;
    return m >= (float)kEmitTexMaxL ? kEmitTexMaxL : (uint32_t)m;
}
// centroid k of L^2, as (b1, b2): cell (a, c) = (k / L, k % L) of the L x L grid is the upright small triangle (a, c) when a + c < L and the
// inverted one (L - 1 - a, L - 1 - c) otherwise; centroids ((3 i + 1) / 3L, (3 j + 1) / 3L) and ((3 i + 2) / 3L, (3 j + 2) / 3L)
RT3_DEV void emit_tex_centroid(uint32_t L, uint32_t k, float& b1, float& b2) {
    const uint32_t a = k / L, c = k - a * L;
    const bool up = a + c < L;
    const uint32_t i = up ? a : L - 1u - a, j = up ? c : L - 1u - c, o = up ? 1u : 2u;
    const float d = (float)(3u * L);
    b1 = (float)(3u * i + o) / d;
    b2 = (float)(3u * j + o) / d;
}

// One k_emit_tex launch: the emitter shadow queue k_shade of bounce `bounce` wrote (its length in *count) has the contribution of every ray
// whose emitter carries an emissive texture multiplied by the texture at the sampled point, channel by channel.  The pick and the point are
// k_shade's: the path's RNG dims 5, 6, 7 are drawn again.
struct EmitTexLaunch {
    SceneDev sc;
    LightsDev lights;
    const EmitTexDev* emit_tex;
    float* rays;      // {o, contribution r} x stride, {d, contribution g} x stride
    float* contrib;   // {contribution b, path id} x stride
    const uint32_t* count;
    size_t stride;
    const uint32_t* pixels;  // x | y << 16; path id = sample_in_batch * npix + pixel index
    uint32_t npix;
    FastDiv npix_div;
    uint32_t s0;             // first sample index of the batch
    uint32_t bounces, bounce, frame;
    uint32_t dims;           // RNG dimensions per vertex (k_shade's: 8 with any flag)
};

}  // namespace rt3
