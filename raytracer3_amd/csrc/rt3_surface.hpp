// rt3_surface.hpp -- the scene's device tables (geometry, textures, alpha, material textures, emitters) and the surface of a hit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt3_math.hpp"

namespace rt3 {

// ------------------------------------------------------------------------------------------------ scene access
struct GeometryInfoDev {  // datatypes.slang:11-19 padded to 64 B
    float base_color[4];
    int32_t tex;
    float metallic;
    uint32_t index_offset, vertex_offset;
    float emission[4];
    float roughness;
    uint32_t pad[3];
};
static_assert(sizeof(GeometryInfoDev) == 64, "GeometryInfo layout");
// One entry per (instance, geometry) pair of the world (world/mod.rs:34-60: InstanceInfo{mesh_index, transform} + Transform{Mat4}):
// rt3_accel_build flattens the instances into world-space triangles (the 3 ms device build stands in for the TLAS), so the builder
// needs each pair's index / vertex offsets and its matrix, and hit_info its material and the matrix's upper 3 x 3 (hit_logic.slang:23).
struct FlatGeomDev {
    GeometryInfoDev g;
    float m[12];        // column-major 3 x 4: x_axis, y_axis, z_axis, w_axis (glam Mat4 columns without their last row)
    uint32_t identity;  // 1: the instance matrix is exactly the identity -- positions and normals are used as uploaded
    uint32_t geom, instance, pad;
};
static_assert(sizeof(FlatGeomDev) == 128, "FlatGeom layout");
// What hit_info reads of a flattened geometry, 80 bytes: k_shade keeps the whole table in LDS when it has at most kShadeGeomsLds entries
// ("material table in LDS when <= a few hundred"), so that a hit costs ONE dependent global gather (its shading record)
struct ShadeGeomDev {
    float base_color[3];
    int32_t tex;
    float metallic, roughness;
    float emission[3];
    uint32_t identity;
    float m[9];  // upper 3 x 3 of the instance matrix, column-major
    uint32_t pad;
};
static_assert(sizeof(ShadeGeomDev) == 80, "ShadeGeom layout");
constexpr uint32_t kShadeGeomsLds = 256;
RT3_DEV V3 transform_point(const float* m, V3 p) {  // glam Mat4::transform_point3: ((x_axis * x + y_axis * y) + z_axis * z) + w_axis
    return v3(m[9] + (m[6] * p.z + (m[3] * p.y + m[0] * p.x)), m[10] + (m[7] * p.z + (m[4] * p.y + m[1] * p.x)), m[11] + (m[8] * p.z + (m[5] * p.y + m[2] * p.x)));
}
RT3_DEV V3 transform_vector(const float* m9, V3 v) {  // mul(transform, float4(v, 0)).xyz, hit_logic.slang:23
    return v3(m9[6] * v.z + (m9[3] * v.y + m9[0] * v.x), m9[7] * v.z + (m9[4] * v.y + m9[1] * v.x), m9[8] * v.z + (m9[5] * v.y + m9[2] * v.x));
}

// == rt3_material_textures, per flattened geometry (the side table of hit_finish<true>)
struct MatTexDev {
    int32_t mr_tex, normal_tex, emissive_tex;
    float normal_scale;
};
static_assert(sizeof(MatTexDev) == 16, "MatTex layout");

struct SceneDev {
    const float* verts;          // interleaved p n t (8 floats)
    const uint32_t* indices;
    const FlatGeomDev* geoms;    // one per (instance, geometry), in instance order
    const ShadeGeomDev* shade_geoms;  // the same table as hit_info needs it (80-byte entries)
    uint32_t n_geoms;
    const uint32_t* prim_geom;   // global primitive -> geometry
    const uint32_t* first_prim;  // geometry -> first global primitive
    const uint4* tri_shade;      // per global primitive, 16 B: the three vertex normals, octahedral 2 x 16 bit each, + the flattened geometry index
    const float2* tri_uv;        // per global primitive, 3 x float2: the vertex uvs (read only for textured geometries)
    const uint8_t* tex_pixels;   // all base-colour textures, RGBA8 (sRGB-encoded colour), back to back
    const uint4* tex_table;      // per texture {byte offset, width, height, -}
    const float* srgb_lut;       // 256 entries: sRGB EOTF
    uint32_t n_tex;
    // sky
    const uint2* sky;            // 8-byte texels {RGB9E5 radiance, pdf_uv}, in 4 x 4 texel tiles of 128 bytes = one cache line
    const uint32_t* sky_alias;   // sky_w x sky_h words, row-major: per-row alias tables, q16 | alias column << 16
    const float* cdf_marg;       // padded: {0, cdf[0..h-1], 2, 2, 2}
    const uint32_t* guide_marg;  // sky_h cells: lo | hi << 16 = search bounds of the cell's answers
    uint32_t sky_w, sky_h, sky_wt;  // sky_wt = tiles per tile row = ceil(sky_w / 4)
    const uint8_t* bluenoise;
    uint32_t bn_w, bn_h;
    // material textures: null unless the built scene names one
    const MatTexDev* mat_tex;    // per flattened geometry, 16 B
    const uint32_t* tri_tan;     // per global primitive: the tangent word (tan_encode); null unless some geometry names a normal texture
};

// hit_logic.slang:5-40 (transform = identity, vertex colour = 1).  The three index + three vertex gathers of
// :10-20 are folded at build time into one 64-byte shading record per primitive (same values, one cache line).
// Textures[i].SampleLevel(uv, 0).xyz (hit_logic.slang:32): sRGB decode per texel, bilinear, repeat addressing, mip 0
RT3_DEV V3 texture_sample(const SceneDev& sc, uint32_t index, float u, float v) {
    const uint4 t = sc.tex_table[index];
    const int W = (int)t.y, H = (int)t.z;
    const uint8_t* px = sc.tex_pixels + t.x;
    float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
    float xf = floorf(x), yf = floorf(y), fx = x - xf, fy = y - yf;
    int x0 = (int)xf, y0 = (int)yf, x1 = x0 + 1, y1 = y0 + 1;
    x0 = wrap_index(x0, W);
    x1 = wrap_index(x1, W);
    y0 = wrap_index(y0, H);
    y1 = wrap_index(y1, H);
    const uint32_t p00 = *reinterpret_cast<const uint32_t*>(px + 4 * ((size_t)y0 * W + x0)), p10 = *reinterpret_cast<const uint32_t*>(px + 4 * ((size_t)y0 * W + x1));
    const uint32_t p01 = *reinterpret_cast<const uint32_t*>(px + 4 * ((size_t)y1 * W + x0)), p11 = *reinterpret_cast<const uint32_t*>(px + 4 * ((size_t)y1 * W + x1));
    float o[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float top = sc.srgb_lut[(p00 >> (8 * k)) & 0xFFu] * (1.0f - fx) + sc.srgb_lut[(p10 >> (8 * k)) & 0xFFu] * fx;
        float bot = sc.srgb_lut[(p01 >> (8 * k)) & 0xFFu] * (1.0f - fx) + sc.srgb_lut[(p11 >> (8 * k)) & 0xFFu] * fx;
        o[k] = top * (1.0f - fy) + bot * fy;
    }
    return v3(o[0], o[1], o[2]);
}
// Alpha-masked geometry (glTF alphaMode MASK).  tex_alpha: the bilinear alpha of base-colour texture `index` at mip 0,
// texture_sample's texel coordinates, weights and association on the alpha byte (linear: byte * (1 / 255), no sRGB decode); 1 without a
// texture (index -1 or out of range)
RT3_DEV float tex_alpha(const uint4* tex_table, const uint8_t* tex_pixels, uint32_t n_tex, int32_t index, float u, float v) {
    if (index < 0 || (uint32_t)index >= n_tex) return 1.0f;
    const uint4 t = tex_table[index];
    const int W = (int)t.y, H = (int)t.z;
    const uint8_t* px = tex_pixels + t.x;
    float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
    float xf = floorf(x), yf = floorf(y), fx = x - xf, fy = y - yf;
    int x0 = (int)xf, y0 = (int)yf, x1 = x0 + 1, y1 = y0 + 1;
    x0 = wrap_index(x0, W);
    x1 = wrap_index(x1, W);
    y0 = wrap_index(y0, H);
    y1 = wrap_index(y1, H);
    const float a00 = (float)px[4 * ((size_t)y0 * W + x0) + 3] * (1.0f / 255.0f), a10 = (float)px[4 * ((size_t)y0 * W + x1) + 3] * (1.0f / 255.0f);
    const float a01 = (float)px[4 * ((size_t)y1 * W + x0) + 3] * (1.0f / 255.0f), a11 = (float)px[4 * ((size_t)y1 * W + x1) + 3] * (1.0f / 255.0f);
    const float top = a00 * (1.0f - fx) + a10 * fx, bot = a01 * (1.0f - fx) + a11 * fx;
    return top * (1.0f - fy) + bot * fy;
}
// What the masked traversal kernels read besides the tree.  A masked triangle record carries {v2.z, prim, cutoff, slot} (unmasked: cutoff
// 0.0f and slot 0): table[slot] = {base-colour texture index (int32), base_color[3] bits} of its geometry.
struct AlphaDev {
    const uint2* table;
    const float2* tri_uv;  // SceneDev::tri_uv
    const uint4* tex_table;
    const uint8_t* tex_pixels;
    uint32_t n_tex;
};
// the uv at barycentrics (b0, bu, bv) of primitive `prim`: its three vertex uvs (SceneDev::tri_uv), weighted in this order
RT3_DEV void tri_uv_at(const float2* tri_uv, uint32_t prim, float b0, float bu, float bv, float& uu, float& vv) {
    const float2 t0 = tri_uv[3 * (size_t)prim], t1 = tri_uv[3 * (size_t)prim + 1], t2 = tri_uv[3 * (size_t)prim + 2];
    uu = t0.x * b0 + t1.x * bu + t2.x * bv;
    vv = t0.y * b0 + t1.y * bu + t2.y * bv;
}
// does the intersection (prim, bu, bv) of a masked triangle count?  alpha = base_color[3] * tex_alpha at the uv hit_finish interpolates
RT3_DEV bool alpha_counts(const AlphaDev& a, uint32_t slot, float cutoff, uint32_t prim, float bu, float bv) {
    const uint2 e = a.table[slot];
    float uu, vv;
    tri_uv_at(a.tri_uv, prim, 1.0f - bu - bv, bu, bv, uu, vv);
    const float alpha = __uint_as_float(e.y) * tex_alpha(a.tex_table, a.tex_pixels, a.n_tex, (int32_t)e.x, uu, vv);
    return alpha >= cutoff;
}

// ------------------------------------------------------------------------------------------------ material textures
// Tangent word of a primitive: the unit tangent T through the octahedral map at 15 bits per coordinate (bits 0-14 x, 15-29 y), bit 30 = the
// handedness h is -1, bit 31 = the primitive has a tangent.  0 = no tangent.
constexpr uint32_t kTanValid = 0x80000000u, kTanFlip = 0x40000000u;
RT3_DEV bool finite_pos(float x) { return x > 0.0f && x <= kFloatMax; }
RT3_DEV uint32_t tan_encode(V3 T, bool flip) {  // octa_encode16's steps on a 15-bit grid
    const float s = fabsf(T.x) + fabsf(T.y) + fabsf(T.z);
    if (!finite_pos(s)) return 0u;
    float x = T.x / s, y = T.y / s;
    const float z = T.z / s;
    if (z < 0.0f) {  // octa_wrap
        const float wx = (1.0f - fabsf(y)) * ((x >= 0.0f ? 1.0f : 0.0f) * 2.0f - 1.0f);
        const float wy = (1.0f - fabsf(x)) * ((y >= 0.0f ? 1.0f : 0.0f) * 2.0f - 1.0f);
        x = wx;
        y = wy;
    }
    x = x * 0.5f + 0.5f;
    y = y * 0.5f + 0.5f;
    const uint32_t qx = (uint32_t)(fmin_sel(fmax_sel(x, 0.0f), 1.0f) * 32767.0f + 0.5f), qy = (uint32_t)(fmin_sel(fmax_sel(y, 0.0f), 1.0f) * 32767.0f + 0.5f);
    return qx | (qy << 15) | (flip ? kTanFlip : 0u) | kTanValid;
}
RT3_DEV V3 tan_decode(uint32_t w) { return octa_decode((float)(w & 0x7FFFu) * (1.0f / 32767.0f), (float)((w >> 15) & 0x7FFFu) * (1.0f / 32767.0f)); }
// The tangent word of a triangle from its object-space positions, uvs and vertex normals (k_tri_tangent; rt3.h has the rule)
RT3_DEV uint32_t tangent_word(V3 p0, V3 p1, V3 p2, float2 t0, float2 t1, float2 t2, V3 nsum) {
    const V3 e1 = p1 - p0, e2 = p2 - p0;
    const float du1 = t1.x - t0.x, dv1 = t1.y - t0.y, du2 = t2.x - t0.x, dv2 = t2.y - t0.y;
    const float det = du1 * dv2 - du2 * dv1;
    if (!(det != 0.0f)) return 0u;  // (a NaN determinant too)
    const V3 r = e1 * dv2 - e2 * dv1;
    const float l2 = dot(r, r);
    if (!finite_pos(l2)) return 0u;
    V3 T = r * (1.0f / sqrtf(l2));
    if (det < 0.0f) T = neg(T);
    const bool flip = (det < 0.0f) != (dot(cross(e1, e2), nsum) < 0.0f);
    return tan_encode(T, flip);
}
// the four texels of texture_sample's bilinear footprint and its weights
struct TexQuad {
    uint32_t p00, p10, p01, p11;
    float fx, fy;
};
RT3_DEV TexQuad tex_quad(const SceneDev& sc, uint32_t index, float u, float v) {
    const uint4 t = sc.tex_table[index];
    const int W = (int)t.y, H = (int)t.z;
    const uint8_t* px = sc.tex_pixels + t.x;
    float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
    float xf = floorf(x), yf = floorf(y);
    int x0 = (int)xf, y0 = (int)yf, x1 = x0 + 1, y1 = y0 + 1;
    x0 = wrap_index(x0, W);
    x1 = wrap_index(x1, W);
    y0 = wrap_index(y0, H);
    y1 = wrap_index(y1, H);
    TexQuad q;
    q.fx = x - xf;
    q.fy = y - yf;
    q.p00 = *reinterpret_cast<const uint32_t*>(px + 4 * ((size_t)y0 * W + x0));
    q.p10 = *reinterpret_cast<const uint32_t*>(px + 4 * ((size_t)y0 * W + x1));
    q.p01 = *reinterpret_cast<const uint32_t*>(px + 4 * ((size_t)y1 * W + x0));
    q.p11 = *reinterpret_cast<const uint32_t*>(px + 4 * ((size_t)y1 * W + x1));
    return q;
}
RT3_DEV float lerp_ab(float a, float b, float f) { return a + (b - a) * f; }
// channel k of the footprint, bytes decoded linearly; x first, then y
RT3_DEV float quad_linear(const TexQuad& q, int k) {
    const float a = (float)((q.p00 >> (8 * k)) & 0xFFu) * (1.0f / 255.0f), b = (float)((q.p10 >> (8 * k)) & 0xFFu) * (1.0f / 255.0f);
    const float c = (float)((q.p01 >> (8 * k)) & 0xFFu) * (1.0f / 255.0f), d = (float)((q.p11 >> (8 * k)) & 0xFFu) * (1.0f / 255.0f);
    return lerp_ab(lerp_ab(a, b, q.fx), lerp_ab(c, d, q.fx), q.fy);
}
RT3_DEV float quad_srgb(const SceneDev& sc, const TexQuad& q, int k) {
    const float a = sc.srgb_lut[(q.p00 >> (8 * k)) & 0xFFu], b = sc.srgb_lut[(q.p10 >> (8 * k)) & 0xFFu];
    const float c = sc.srgb_lut[(q.p01 >> (8 * k)) & 0xFFu], d = sc.srgb_lut[(q.p11 >> (8 * k)) & 0xFFu];
    return lerp_ab(lerp_ab(a, b, q.fx), lerp_ab(c, d, q.fx), q.fy);
}
// n (unit, object space) tilted by the normal-map texel c = 2 lerp - 1 in the frame of tangent word `tanw`; n itself where the rule says so
RT3_DEV V3 normal_map_apply(V3 n, uint32_t tanw, float cx, float cy, float cz, float s) {
    if (!(tanw & kTanValid)) return n;
    const V3 T = tan_decode(tanw);
    const V3 tp = T - n * dot(n, T);
    const float l2 = dot(tp, tp);
    if (!finite_pos(l2)) return n;
    const V3 t = tp * (1.0f / sqrtf(l2));
    V3 b = cross(n, t);
    if (tanw & kTanFlip) b = neg(b);
    const V3 m = t * (s * cx) + b * (s * cy) + n * cz;
    const float m2 = dot(m, m);
    if (!finite_pos(m2)) return n;
    return m * (1.0f / sqrtf(m2));
}

// In two steps so that a caller can put independent work (the light sample's table gathers) between the issue of the
// shading-record load and its use.  The record is 16 bytes {n0, n1, n2, geometry}: a quarter of round 2's 64-byte record, i.e.
// a 4 MB table for 260 k triangles instead of 16.6 MB (an L2 miss costs a 128-byte line whatever the record's size).
struct HitRecord {
    uint4 rec;
    uint32_t prim;
};
RT3_DEV HitRecord hit_fetch(const SceneDev& sc, uint32_t prim) { return HitRecord{sc.tri_shade[prim], prim}; }
// the tangent word of a hit: issued beside hit_fetch's record (it depends on the primitive alone), used by hit_finish<true>
RT3_DEV uint32_t tan_fetch(const SceneDev& sc, uint32_t prim) { return sc.tri_tan ? sc.tri_tan[prim] : 0u; }
// `geoms`: the ShadeGeomDev table -- sc.shade_geoms, or the caller's LDS copy of it.  MAT: the material textures of DESIGN.md section 4j;
// `mats` is sc.mat_tex or the caller's LDS copy of it, `tanw` the hit's tan_fetch
template <bool MAT = false>
RT3_DEV Surface hit_finish(const SceneDev& sc, const ShadeGeomDev* geoms, const HitRecord& h, float bu, float bv, const MatTexDev* mats = nullptr,
                           uint32_t tanw = 0u) {
    const ShadeGeomDev& gi = geoms[h.rec.w];
    const V3 n0 = octa_decode16(h.rec.x), n1 = octa_decode16(h.rec.y), n2 = octa_decode16(h.rec.z);
    float b0 = 1.0f - bu - bv;
    V3 n = v3(n0.x * b0 + n1.x * bu + n2.x * bv, n0.y * b0 + n1.y * bu + n2.y * bv, n0.z * b0 + n1.z * bu + n2.z * bv);
    n = normalize(n);                                   // :22
    V3 tex_albedo = v3(1.0f, 1.0f, 1.0f), tex_emissive = v3(1.0f, 1.0f, 1.0f);
    float tex_rough = 1.0f, tex_metal = 1.0f;
    bool has_base = false, has_mr = false, has_e = false;
    if constexpr (MAT) {
        const MatTexDev mt = mats[h.rec.w];
        has_base = gi.tex > -1 && (uint32_t)gi.tex < sc.n_tex;
        has_mr = mt.mr_tex > -1 && (uint32_t)mt.mr_tex < sc.n_tex;
        has_e = mt.emissive_tex > -1 && (uint32_t)mt.emissive_tex < sc.n_tex;
        const bool has_n = mt.normal_tex > -1 && (uint32_t)mt.normal_tex < sc.n_tex;
        if (has_base || has_mr || has_n || has_e) {
            float uu, vv;
            tri_uv_at(sc.tri_uv, h.prim, b0, bu, bv, uu, vv);
            // the footprints first (up to sixteen independent texel loads in flight), their arithmetic after
            TexQuad qn = {}, qm = {}, qe = {};
            if (has_n) qn = tex_quad(sc, (uint32_t)mt.normal_tex, uu, vv);
            if (has_mr) qm = tex_quad(sc, (uint32_t)mt.mr_tex, uu, vv);
            if (has_e) qe = tex_quad(sc, (uint32_t)mt.emissive_tex, uu, vv);
            if (has_base) tex_albedo = texture_sample(sc, (uint32_t)gi.tex, uu, vv);
            if (has_n) n = normal_map_apply(n, tanw, 2.0f * quad_linear(qn, 0) - 1.0f, 2.0f * quad_linear(qn, 1) - 1.0f, 2.0f * quad_linear(qn, 2) - 1.0f, mt.normal_scale);
            if (has_mr) {
                tex_rough = quad_linear(qm, 1);
                tex_metal = quad_linear(qm, 2);
            }
            if (has_e) tex_emissive = v3(quad_srgb(sc, qe, 0), quad_srgb(sc, qe, 1), quad_srgb(sc, qe, 2));
        }
    }
    if (!gi.identity) n = transform_vector(gi.m, n);    // :23 mul(geometryInfo.transform, float4(normal, 0.0)).xyz
    n = normalize(n);                                   // :23
    Surface s;
    s.albedo = v3(gi.base_color[0], gi.base_color[1], gi.base_color[2]);
    if constexpr (MAT) {
        if (has_base) s.albedo = s.albedo * tex_albedo;
    } else if (gi.tex > -1 && (uint32_t)gi.tex < sc.n_tex) {  // :27,31-33
        float uu, vv;
        tri_uv_at(sc.tri_uv, h.prim, b0, bu, bv, uu, vv);
        s.albedo = s.albedo * texture_sample(sc, (uint32_t)gi.tex, uu, vv);
    }
    s.emissive = v3(gi.emission[0] * 12.0f, gi.emission[1] * 12.0f, gi.emission[2] * 12.0f);  // :36
    s.normal = n;
    s.roughness = gi.roughness;
    s.metalness = gi.metallic;
    if constexpr (MAT) {
        if (has_e) s.emissive = s.emissive * tex_emissive;
        if (has_mr) {
            s.roughness = gi.roughness * tex_rough;
            s.metalness = gi.metallic * tex_metal;
        }
    }
    return s;
}
// (a uniform branch: kernels off the hot path -- k_gbuffer, the probes, selftest op 29 -- take whichever the built scene needs)
RT3_DEV Surface hit_info(const SceneDev& sc, uint32_t prim, float bu, float bv) {
    if (sc.mat_tex) return hit_finish<true>(sc, sc.shade_geoms, hit_fetch(sc, prim), bu, bv, sc.mat_tex, tan_fetch(sc, prim));
    return hit_finish(sc, sc.shade_geoms, hit_fetch(sc, prim), bu, bv);
}

// ------------------------------------------------------------------------------------------------ emitters (RT3_F_NEE_EMISSIVE)
// The emitter table (rt3_lights.hip).  Record e, 64 bytes = 4 float4:
//   {A.xyz, p_sel / area}  {E1.xyz, Le.r}  {E2.xyz, Le.g}  {unit geometric normal, Le.b}
// A, A + E1, A + E2: the world-space triangle as flattening makes it; Le = 12 emission (hit_finish's value); p_sel = mass / 2^23, exact.
// cdf: inclusive integer CDF (cdf[n - 1] = 2^23); guide: 2^23 >> guide_shift cells + 1, cell c holds the first e with cdf[e] > c << shift (n in a
// table without power, which is never looked up: LightTable::dev gives it n = 0); the last word is n - 1.
struct LightsDev {
    const float4* rec;
    const uint32_t* cdf;
    const uint32_t* guide;
    const uint32_t* geom_base;  // per flattened geometry: its first emitter, or kMiss for a geometry without emission
    uint32_t n, guide_shift;    // n = 0: nothing to sample
};
// the emitter that owns k in [0, 2^23): the first e with cdf[e] > k (emitters of zero mass are never returned)
RT3_DEV uint32_t light_find(const LightsDev& lt, uint32_t k) {
    const uint32_t c = k >> lt.guide_shift;
    uint32_t lo = lt.guide[c], hi = lt.guide[c + 1];
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (lt.cdf[mid] > k) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

}  // namespace rt3
