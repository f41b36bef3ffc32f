// rt3_sky.hpp -- the sky: bilinear lookups and the importance sampler over SceneDev's sky tables.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt3_math.hpp"
#include "rt3_surface.hpp"

namespace rt3 {

// ------------------------------------------------------------------------------------------------ sky (north_star)
// Texels are 8 bytes {RGB9E5 radiance, pdf_uv as f32}: the importance-sampling density of a texel travels with its colour (the
// texel is always one of the four bilinear corners), and a 4 x 4 texel tile is exactly one 128-byte line -- the unit the fabric
// moves whatever a lane asks for (profiles/r02_fetch_calibration.md): the 2 x 2 bilinear footprint costs 1.56 lines on average
// instead of 2.25 with row-major 16-byte texels.
RT3_DEV uint32_t sky_texel_index(const SceneDev& sc, int x, int y) {
    return (((uint32_t)y >> 2) * sc.sky_wt + ((uint32_t)x >> 2)) * 16u + ((((uint32_t)y & 3u) << 2) | ((uint32_t)x & 3u));
}
RT3_DEV V3 sky_eval_pdf(const SceneDev& sc, float u, float v, int tx, int ty, float& pdf_texel) {
    int W = (int)sc.sky_w, H = (int)sc.sky_h;
    float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
    float xf = floorf(x), yf = floorf(y);
    float fx = x - xf, fy = y - yf;
    int x0 = (int)xf, y0 = (int)yf, x1 = x0 + 1, y1 = y0 + 1;
    x0 = wrap_index(x0, W);
    x1 = wrap_index(x1, W);
    y0 = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0);
    y1 = y1 < 0 ? 0 : (y1 > H - 1 ? H - 1 : y1);
    const uint2 t00 = sc.sky[sky_texel_index(sc, x0, y0)], t10 = sc.sky[sky_texel_index(sc, x1, y0)];
    const uint2 t01 = sc.sky[sky_texel_index(sc, x0, y1)], t11 = sc.sky[sky_texel_index(sc, x1, y1)];
    if (tx >= 0) {
        const bool in_x = tx == x0 || tx == x1, in_y = ty == y0 || ty == y1;
        pdf_texel = __uint_as_float(ty == y0 ? (tx == x0 ? t00.y : t10.y) : (tx == x0 ? t01.y : t11.y));
        if (!(in_x && in_y)) pdf_texel = __uint_as_float(sc.sky[sky_texel_index(sc, tx, ty)].y);  // not reached for (u, v) inside texel (tx, ty)
    }
    const V3 p00 = rgb9e5_to_float3(t00.x), p10 = rgb9e5_to_float3(t10.x), p01 = rgb9e5_to_float3(t01.x), p11 = rgb9e5_to_float3(t11.x);
    const float a[3] = {p00.x, p00.y, p00.z}, bq[3] = {p10.x, p10.y, p10.z}, c[3] = {p01.x, p01.y, p01.z}, dq[3] = {p11.x, p11.y, p11.z};
    float o[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float top = a[k] * (1.0f - fx) + bq[k] * fx, bot = c[k] * (1.0f - fx) + dq[k] * fx;
        o[k] = top * (1.0f - fy) + bot * fy;
    }
    return v3(o[0], o[1], o[2]);
}
RT3_DEV V3 sky_eval(const SceneDev& sc, float u, float v) {  // Skybox.SampleLevel(uv, 0): bilinear, wrap u, clamp v
    if (!sc.sky) return v3(0.0f, 0.0f, 0.0f);
    float unused;
    return sky_eval_pdf(sc, u, v, -1, -1, unused);
}
// radiance and solid-angle pdf of the sky sampler for a direction that left the scene (equirect coordinates u, v)
RT3_DEV V3 sky_eval_and_pdf(const SceneDev& sc, float u, float v, float& pdf) {
    int W = (int)sc.sky_w, H = (int)sc.sky_h;
    int ix = (int)(u * (float)W), iy = (int)(v * (float)H);
    ix = ix < 0 ? 0 : (ix > W - 1 ? W - 1 : ix);
    iy = iy < 0 ? 0 : (iy > H - 1 ? H - 1 : iy);
    float pt;
    V3 rad = sky_eval_pdf(sc, u, v, ix, iy, pt);
    float st, ct;
    sincos_2pi(v * 0.5f, st, ct);
    pdf = st > 0.0f ? pt / (2.0f * kPi * kPi * st) : 0.0f;
    return rad;
}
// The oracle's cdf_find -- first i with cdf[i] > u -- plus the bracket {cdf[i-1] (0 for i = 0), cdf[i]}, in two memory
// round trips: the guide cell of u gives bounds [lo, hi] around the answer; when they are at most two apart (81-93 % of
// the lookups on the bench sky) ONE unaligned 16-byte load {cdf[lo-1] .. cdf[lo+2]} of the padded CDF holds every
// candidate and the bracket.  Wider cells fall back to the binary search.  Used for the MARGINAL (row) table only, which
// k_shade stages in LDS; inside a row a light sample reads ONE word of the row's alias table instead of searching a CDF.
typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));
RT3_DEV uint32_t cdf_find_guided(const float* cdfp, const uint32_t* guide, uint32_t n, float u, float& lo_v, float& hi_v) {
    uint32_t k = (uint32_t)(u * (float)n);
    k = k > n - 1 ? n - 1 : k;
    const uint32_t g = guide[k];
    uint32_t lo = g & 0xFFFFu, hi = g >> 16;
    if (hi - lo <= 2u) {
        const f32x4_u c = *reinterpret_cast<const f32x4_u*>(cdfp + lo);
        const bool s1 = lo < hi && !(c.y > u);
        const bool s2 = s1 && lo + 1u < hi && !(c.z > u);
        lo_v = s2 ? c.z : (s1 ? c.y : c.x);
        hi_v = s2 ? c.w : (s1 ? c.z : c.y);
        return lo + (s1 ? 1u : 0u) + (s2 ? 1u : 0u);
    }
    while (lo < hi) {
        uint32_t mid = (lo + hi) >> 1;
        if (cdfp[mid + 1] > u) hi = mid;
        else lo = mid + 1;
    }
    lo_v = cdfp[lo];
    hi_v = cdfp[lo + 1];
    return lo;
}
// Light sample in two steps, so that the caller can drop samples below the surface's horizon (cos <= 0: nearly half of
// them) BEFORE paying for the radiance texels: (1) invert the CDFs -> texel, equirect coordinates, direction;
// (2) bilinear radiance + the texel's density.
struct SkyPick {
    float u, v, sin_theta;
    int x, y;
};
// cdf_marg / guide_marg: the marginal tables (the caller may have staged them in LDS)
RT3_DEV SkyPick sky_sample_direction(const SceneDev& sc, const float* cdf_marg, const uint32_t* guide_marg, float u0, float u1, V3& dir) {
    uint32_t W = sc.sky_w, H = sc.sky_h;
    float lo, hi;
    uint32_t y = cdf_find_guided(cdf_marg, guide_marg, H, u0, lo, hi);
    float dv = hi > lo ? (u0 - lo) / (hi - lo) : 0.5f;
    // the row's alias table (the oracle's sky_sample has the construction): cell k = floor(u1 W); xi = frac(u1 W) decides between
    // column k and its alias and is stretched back to [0, 1) as the position inside the chosen texel.  ONE gathered word.
    const float sx = u1 * (float)W;
    uint32_t k = (uint32_t)sx;
    k = k > W - 1 ? W - 1 : k;
    float xi = sx - (float)k;
    xi = xi < 0.99999994f ? xi : 0.99999994f;
    const uint32_t e = sc.sky_alias[(size_t)y * W + k];
    const float Q = (float)((e & 0xFFFFu) + 1u) * (1.0f / 65536.0f);
    const bool keep = xi < Q;
    const uint32_t x = keep ? k : (e >> 16);
    float du = keep ? xi / Q : (xi - Q) / (1.0f - Q);
    du = du < 0.99999994f ? du : 0.99999994f;
    SkyPick p;
    p.u = ((float)x + du) / (float)W;
    p.v = ((float)y + dv) / (float)H;
    p.x = (int)x;
    p.y = (int)y;
    float st, ct, s2, c2;
    sincos_2pi(p.v * 0.5f, st, ct);
    sincos_2pi(p.u, s2, c2);
    p.sin_theta = st;
    dir = v3((-c2) * st, ct, (-s2) * st);
    return p;
}
RT3_DEV void sky_sample_radiance(const SceneDev& sc, const SkyPick& p, V3& rad, float& pdf) {
    float pt;
    rad = sky_eval_pdf(sc, p.u, p.v, p.x, p.y, pt);
    pdf = p.sin_theta > 0.0f ? pt / (2.0f * kPi * kPi * p.sin_theta) : 0.0f;
}
RT3_DEV void sky_sample(const SceneDev& sc, float u0, float u1, V3& dir, V3& rad, float& pdf) {
    const SkyPick p = sky_sample_direction(sc, sc.cdf_marg, sc.guide_marg, u0, u1, dir);
    sky_sample_radiance(sc, p, rad, pdf);
}

}  // namespace rt3
