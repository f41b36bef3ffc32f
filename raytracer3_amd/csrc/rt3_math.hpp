// rt3_math.hpp -- device-side arithmetic of the gfx950 wavefront path tracer: constants, V3, exact integer division, the G-buffer packing,
// the transcendental polynomials and the octahedral maps.
//
// Each function names the reference shader lines it implements (paths relative to DerEchteKarsten/RayTracer3).
// Arithmetic contract: fp32, compiled with -ffp-contract=off, IEEE divide/sqrt, min/max as explicit
// selects, transcendental functions only through the polynomials below -- so results are reproducible bit for bit
// on any IEEE-754 machine and can be checked exactly by the CPU oracle in tests.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RT3_DEV __device__ __forceinline__

namespace rt3 {

constexpr float kPi = 3.14159265358979323846f;
constexpr float kTau = 6.28318530717958647692f;       // math.slang:3
constexpr float kInvPi = 0.318309886183790671538f;    // math.slang:4
constexpr float kHalfPi = 1.57079632679489661923f;
constexpr float kBackgroundDepth = 100000.0f;         // datatypes.slang:3
constexpr uint32_t kMiss = 0xFFFFFFFFu;
constexpr float kRayTMin = 0.001f;                    // refrence_mode.slang:31
constexpr float kFloatMax = 3.4028234663852886e38f;   // the largest finite fp32: x <= kFloatMax is "x is neither +inf nor NaN"

struct V3 {
    float x, y, z;
};
RT3_DEV V3 v3(float x, float y, float z) { return V3{x, y, z}; }
RT3_DEV V3 operator+(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
RT3_DEV V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
RT3_DEV V3 operator*(V3 a, V3 b) { return V3{a.x * b.x, a.y * b.y, a.z * b.z}; }
RT3_DEV V3 operator*(V3 a, float s) { return V3{a.x * s, a.y * s, a.z * s}; }
RT3_DEV V3 neg(V3 a) { return V3{-a.x, -a.y, -a.z}; }
RT3_DEV float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
RT3_DEV V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
RT3_DEV V3 normalize(V3 a) {
    float inv = 1.0f / sqrtf(dot(a, a));
    return a * inv;
}
// exact n / d for 32-bit operands without a hardware divide (round-up magic number, Granlund-Montgomery / libdivide
// "branch-free"): q = umulhi(mul, n); n / d = (((n - q) >> 1) + q) >> shift.  A runtime integer division costs ~30 VALU.
struct FastDiv {
    uint32_t d, mul, shift;
};
__host__ __device__ inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f{d, 0u, 0u};
    if (d > 1u) {
        uint32_t l = 0;
        while (l < 32u && (1ull << l) < (unsigned long long)d) ++l;  // ceil(log2 d)
        f.mul = (uint32_t)((((1ull << l) - d) << 32) / d + 1ull);
        f.shift = l - 1u;
    }
    return f;
}
RT3_DEV uint32_t fast_div(const FastDiv& f, uint32_t n) {
    if (f.d <= 1u) return n;
    const uint32_t q = __umulhi(f.mul, n);
    return (((n - q) >> 1) + q) >> f.shift;
}
// ((x % W) + W) % W.  Texel neighbours of a coordinate in [0, 1] lie within one period of the image, where the wrap is a
// conditional add; the general form is kept for everything else.
RT3_DEV int wrap_index(int x, int W) {
    if ((uint32_t)(x + W) < 3u * (uint32_t)W) return x < 0 ? x + W : (x >= W ? x - W : x);
    return ((x % W) + W) % W;
}
RT3_DEV float fmin_sel(float a, float b) { return a < b ? a : b; }
RT3_DEV float fmax_sel(float a, float b) { return a > b ? a : b; }
// fp32 <-> uint32 with the same order (so that atomicMin / atomicMax on the uint compute the float min / max): LBVH build, SAH top
RT3_DEV uint32_t float_to_ordered(float f) {
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
RT3_DEV float ordered_to_float(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

// ------------------------------------------------------------------------------------------------ packing.slang
RT3_DEV float unpack_unorm(uint32_t p, uint32_t bits) {  // :2-5
    uint32_t maxv = (1u << bits) - 1u;
    return (float)(p & maxv) / (float)maxv;
}
RT3_DEV uint32_t pack_unorm(float v, uint32_t bits) {  // :7-10
    uint32_t maxv = (1u << bits) - 1u;
    float c = fmin_sel(fmax_sel(v, 0.0f), 1.0f);
    return (uint32_t)(c * (float)maxv + 0.5f);
}
RT3_DEV uint32_t pack_normal_11_10_11(V3 n) {  // :12-18
    return pack_unorm(n.x * 0.5f + 0.5f, 11) + (pack_unorm(n.y * 0.5f + 0.5f, 10) << 11) + (pack_unorm(n.z * 0.5f + 0.5f, 11) << 21);
}
RT3_DEV V3 unpack_normal_11_10_11(uint32_t p) {  // :20-27
    return normalize(v3(unpack_unorm(p, 11) * 2.0f - 1.0f, unpack_unorm(p >> 11, 10) * 2.0f - 1.0f, unpack_unorm(p >> 21, 11) * 2.0f - 1.0f));
}
RT3_DEV uint32_t pack_color_888(V3 c) {  // :46-53
    return pack_unorm(sqrtf(c.x), 8) + (pack_unorm(sqrtf(c.y), 8) << 8) + (pack_unorm(sqrtf(c.z), 8) << 16);
}
RT3_DEV V3 unpack_color_888(uint32_t p) {  // :55-62
    V3 c = v3(unpack_unorm(p, 8), unpack_unorm(p >> 8, 8), unpack_unorm(p >> 16, 8));
    return c * c;
}
RT3_DEV uint32_t f32_to_f16_bits(float f) { return (uint32_t)__half_as_ushort(__float2half_rn(f)); }
RT3_DEV float f16_bits_to_f32(uint32_t h) { return __half2float(__ushort_as_half((unsigned short)h)); }
RT3_DEV uint32_t pack_2x16f(float a, float b) { return f32_to_f16_bits(a) | (f32_to_f16_bits(b) << 16); }  // :88-90
RT3_DEV float exp2_int(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }
RT3_DEV uint32_t float3_to_rgb9e5(V3 c) {  // :99-144
    const float max_rgb9e5 = (511.0f / 512.0f) * 65536.0f;
    float rc = fmin_sel(fmax_sel(c.x, 0.0f), max_rgb9e5), gc = fmin_sel(fmax_sel(c.y, 0.0f), max_rgb9e5), bc = fmin_sel(fmax_sel(c.z, 0.0f), max_rgb9e5);
    float maxrgb = fmax_sel(rc, fmax_sel(gc, bc));
    int fl2 = (int)((__float_as_uint(maxrgb) & 0x7F800000u) >> 23) - 127;
    int exp_shared = (fl2 > -16 ? fl2 : -16) + 1 + 15;
    float denom = exp2_int(exp_shared - 15 - 9);
    int maxm = (int)floorf(maxrgb / denom + 0.5f);
    if (maxm == 512) {
        denom *= 2.0f;
        exp_shared += 1;
    }
    int rm = (int)floorf(rc / denom + 0.5f), gm = (int)floorf(gc / denom + 0.5f), bm = (int)floorf(bc / denom + 0.5f);
    return ((uint32_t)rm << 23) | ((uint32_t)gm << 14) | ((uint32_t)bm << 5) | (uint32_t)exp_shared;
}
RT3_DEV V3 rgb9e5_to_float3(uint32_t v) {  // :146-162
    float scale = exp2_int((int)(v & 31u) - 24);
    return v3((float)((v >> 23) & 511u) * scale, (float)((v >> 14) & 511u) * scale, (float)((v >> 5) & 511u) * scale);
}

// gbuffer_helpers.slang:5-71
struct Surface {
    V3 albedo, emissive, normal;
    float roughness, metalness;
};
RT3_DEV uint4 gbuffer_pack(const Surface& s) {  // :22-34
    return make_uint4(pack_color_888(s.albedo), pack_normal_11_10_11(s.normal), pack_2x16f(sqrtf(s.roughness), s.metalness),
                      float3_to_rgb9e5(s.emissive));
}
RT3_DEV Surface gbuffer_unpack(uint4 p) {  // :59-70
    Surface s;
    s.albedo = unpack_color_888(p.x);
    s.normal = unpack_normal_11_10_11(p.y);
    float pr = f16_bits_to_f32(p.z & 0xFFFFu);
    s.roughness = pr * pr;
    s.metalness = f16_bits_to_f32((p.z >> 16) & 0xFFFFu);
    s.emissive = rgb9e5_to_float3(p.w);
    return s;
}

// ------------------------------------------------------------------------------------------------ math
// sin(2 pi u), cos(2 pi u), u in [0,1): exact quadrant split, odd/even Taylor polynomials on [0, pi/4]
RT3_DEV void sincos_2pi(float u, float& s_out, float& c_out) {
    float x = u * 4.0f;
    int q = (int)x;
    float r = x - (float)q;
    bool sw = r > 0.5f;
    if (sw) r = 1.0f - r;
    float a = r * kHalfPi, a2 = a * a;
    float s = a * (1.0f + a2 * (-1.6666667163e-01f + a2 * (8.3333337680e-03f + a2 * (-1.9841270114e-04f + a2 * 2.7557314297e-06f))));
    float c = 1.0f + a2 * (-0.5f + a2 * (4.1666667908e-02f + a2 * (-1.3888889225e-03f + a2 * (2.4801587642e-05f + a2 * -2.7557314297e-07f))));
    float ss = sw ? c : s, cc = sw ? s : c;
    q &= 3;
    s_out = q == 0 ? ss : (q == 1 ? cc : (q == 2 ? -ss : -cc));
    c_out = q == 0 ? cc : (q == 1 ? -ss : (q == 2 ? -cc : ss));
}
// e^-x for x >= 0 (the denoise pass's edge weights): t = x log2(e) rounded once, i = int(t + 1/2), f = t - i exact with |f| <= 1/2; 2^-f by
// the degree-7 Taylor polynomial of exp(-f ln 2); scaled by 2^-i in two exact power-of-two factors, so that a result below 2^-126 is
// rounded once, as a denormal; 0 from t >= 150 on (2^-150 ties to 0), which +inf and NaN reach too.  tests/ref_denoise.py restates it.
RT3_DEV float expn(float x) {
    const float t = x * 1.442695022e+00f;
    const bool live = t < 150.0f;
    const float tc = live ? t : 0.0f;
    const int i = (int)(tc + 0.5f);
    const float f = tc - (float)i;
    float p = -1.525273365e-05f;
    p = p * f + 1.540352969e-04f;
    p = p * f + -1.333355787e-03f;
    p = p * f + 9.618128650e-03f;
    p = p * f + -5.550410971e-02f;
    p = p * f + 2.402265072e-01f;
    p = p * f + -6.931471825e-01f;
    p = p * f + 1.0f;
    const int i0 = i >> 1;
    const float r = (p * exp2_int(-i0)) * exp2_int(i0 - i);
    return live ? r : 0.0f;
}
RT3_DEV float atan2_poly(float y, float x) {
    float ax = x < 0.0f ? -x : x, ay = y < 0.0f ? -y : y;
    float mx = fmax_sel(ax, ay), mn = fmin_sel(ax, ay);
    if (mx == 0.0f) return 0.0f;
    float a = mn / mx, s = a * a;
    float r = a * (0.99997726f + s * (-0.33262347f + s * (0.19354346f + s * (-0.11643287f + s * (0.05265332f + s * -0.01172120f)))));
    if (ay > ax) r = kHalfPi - r;
    if (x < 0.0f) r = kPi - r;
    if (y < 0.0f) r = -r;
    return r;
}
// math.slang:6-12
RT3_DEV void direction_to_equirect_uv(V3 d, float& u, float& v) {
    float as = atan2_poly(d.y, sqrtf(fmax_sel(0.0f, 1.0f - d.y * d.y)));
    u = 0.5f + atan2_poly(d.z, d.x) / kTau;
    v = 0.5f - as / kPi;
}
RT3_DEV float luminance(V3 c) { return c.x * 0.299f + c.y * 0.587f + c.z * 0.114f; }  // math.slang:119-122
// math.slang:29-50 ; columns b1, b2 (third column is n)
RT3_DEV void build_orthonormal_basis(V3 n, V3& b1, V3& b2) {
    if (n.z < 0.0f) {
        const float a = 1.0f / (1.0f - n.z);
        const float b = n.x * n.y * a;
        b1 = v3(1.0f - n.x * n.x * a, -b, n.x);
        b2 = v3(b, n.y * n.y * a - 1.0f, -n.y);
    } else {
        const float a = 1.0f / (1.0f + n.z);
        const float b = -n.x * n.y * a;
        b1 = v3(1.0f - n.x * n.x * a, b, -n.x);
        b2 = v3(b, 1.0f - n.y * n.y * a, -n.y);
    }
}
// mul(tangent_to_world, wi), refrence_mode.slang:48
RT3_DEV V3 basis_apply(V3 b1, V3 b2, V3 n, V3 w) {
    return v3(b1.x * w.x + b2.x * w.y + n.x * w.z, b1.y * w.x + b2.y * w.y + n.y * w.z, b1.z * w.x + b2.z * w.y + n.z * w.z);
}
// brdf.slang:56-65 DiffuseBrdf::sample direction
RT3_DEV V3 diffuse_sample(float u0, float u1) {
    float sp, cp;
    sincos_2pi(u0, sp, cp);
    float cos_theta = sqrtf(fmax_sel(0.0f, 1.0f - u1));
    float sin_theta = sqrtf(fmax_sel(0.0f, 1.0f - cos_theta * cos_theta));
    return v3(cp * sin_theta, sp * sin_theta, cos_theta);
}

// packing.slang:64-86: the reference's octahedral map.  Vertex normals live in the shading records through it, 16 bits per
// coordinate (the oracle's tri_shade defines the same representation: a normal IS octa_decode16(octa_encode16(n)) on both sides).
RT3_DEV V3 octa_decode(float fx, float fy) {  // :77-86
    fx = fx * 2.0f - 1.0f;
    fy = fy * 2.0f - 1.0f;
    V3 n = v3(fx, fy, 1.0f - fabsf(fx) - fabsf(fy));
    float t = fmin_sel(fmax_sel(-n.z, 0.0f), 1.0f);
    n.x -= ((n.x >= 0.0f ? 1.0f : 0.0f) * 2.0f - 1.0f) * t;
    n.y -= ((n.y >= 0.0f ? 1.0f : 0.0f) * 2.0f - 1.0f) * t;
    return normalize(n);
}
RT3_DEV uint32_t octa_encode16(V3 n) {  // :64-75, then 16-bit unorm per coordinate (round to nearest); a zero vector encodes +z
    const float s = fabsf(n.x) + fabsf(n.y) + fabsf(n.z);
    if (!(s > 0.0f) || !(s <= kFloatMax)) return 0x80008000u;  // (0.5, 0.5) -> +z
    float x = n.x / s, y = n.y / s;
    const float z = n.z / s;
    if (z < 0.0f) {  // octa_wrap
        const float wx = (1.0f - fabsf(y)) * ((x >= 0.0f ? 1.0f : 0.0f) * 2.0f - 1.0f);
        const float wy = (1.0f - fabsf(x)) * ((y >= 0.0f ? 1.0f : 0.0f) * 2.0f - 1.0f);
        x = wx;
        y = wy;
    }
    x = x * 0.5f + 0.5f;
    y = y * 0.5f + 0.5f;
    const uint32_t qx = (uint32_t)(fmin_sel(fmax_sel(x, 0.0f), 1.0f) * 65535.0f + 0.5f), qy = (uint32_t)(fmin_sel(fmax_sel(y, 0.0f), 1.0f) * 65535.0f + 0.5f);
    return qx | (qy << 16);
}
RT3_DEV V3 octa_decode16(uint32_t w) { return octa_decode((float)(w & 0xFFFFu) * (1.0f / 65535.0f), (float)(w >> 16) * (1.0f / 65535.0f)); }

}  // namespace rt3
