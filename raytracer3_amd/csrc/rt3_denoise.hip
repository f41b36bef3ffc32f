// rt3_denoise.hip -- the "denoise" pass: a G-buffer-guided, edge-avoiding a-trous wavelet filter (the spatial half of SVGF) over a
// low-sample radiance image.  No reference counterpart (the reference has no spatial filter); DESIGN.md section 4f.
//
//   k_dn_prepare  -> per-pixel records: guide {P.xyz, foreground}, {n.xyz, 0} and signal {c.rgb, 0}, c = (In - emission) / max(albedo, 1/256)
//   k_dn_variance -> signal.w = spatial variance of luminance(c) over 7 x 7, weighted by w_n * w_z (or the temporal variance of the
//                    "temporal" pass where its history is at least 4 frames long: rt3_denoise_set_variance_input)
//   k_dn_atrous   -> one iteration at step 2^i: 5 x 5 B3-spline taps weighted by h * w_n * expn(x_z + x_l); ping-pong between two signal images
//   k_dn_finish   -> Out = emission + c * albedo (alpha and background pixels: In, bit for bit)
// The first and the last are templates over the source of the records (rt3_filter_device.hpp): k_dn_prepare<DnGbuffer> and
// k_dn_finish<DnGbuffer>, or with a guide input (rt3_denoise_set_guide_input) the <DnGuide> instances, which take
// the records from a lens frame's guide images instead of the G-buffer; the two in between are the same launches.
//
// Arithmetic contract: tests/ref_denoise.py restates every operation below in numpy float32, in this order (taps rows outer, columns
// inner); the pass equals it bit for bit.  A background record is all zero: its normal makes w_n, hence the tap's weight, exactly 0, so
// background taps need no branch.  Taps outside the window are skipped (they would add +0).  Every thread writes its own pixel only and
// reads only images the previous launch wrote, so the result does not depend on the launch shape.
//
// A tap is three 16-byte records and about a hundred VALU operations (a correctly rounded sqrt, one IEEE divide, one expn).  At 1080p the
// record images (33 MB each) stay in the last-level cache.  A workgroup stages its 32 x 8 tile plus border in LDS where that was measured
// to win on the MI355X: the 7 x 7 variance stage (245 -> 181 us) and steps 1 and 2 (149 -> 110 / 117 us); at step 4
// it loses (197 us: the border is 3.5 x the tile), so steps >= 4 read through the caches.
#include <hip/hip_runtime.h>

#include "rt3_camera.hpp"
#include "rt3_filter_device.hpp"
#include "rt3_internal.hpp"
#include "rt3_math.hpp"

namespace rt3 {

namespace {

constexpr float kDnTinyR = 1e-20f, kDnTinyL = 1e-6f;  // the tile, the modulation and the luminance: rt3_filter_device.hpp

struct DnCentre {
    V3 P, n;
};
// the geometric terms of a tap: w_n = max(0, n_p . n_q)^(2^squarings) and the exponent x_z = sin(angle out of p's tangent plane) / sigma_z
RT3_DEV void dn_geo(const DnCentre& p, float4 gP, float4 gN, uint32_t squarings, float inv_sigma_z, float& wn, float& xz) {
    const float dn = dot(p.n, v3(gN.x, gN.y, gN.z));
    wn = dn > 0.0f ? dn : 0.0f;
    for (uint32_t k = 0; k < squarings; k++) wn = wn * wn;
    const V3 dP = v3(gP.x, gP.y, gP.z) - p.P;
    const float r = sqrtf(dot(dP, dP));
    const float d = fabsf(dot(p.n, dP));
    xz = (d / (r + kDnTinyR)) * inv_sigma_z;
}

// Src: DnGbuffer (36 bytes read per foreground pixel) or, with a guide input, DnGuide (80: rt3_denoise_set_guide_input, DESIGN.md section
// 4u; tests/ref_guide.py prepare_guide() restates that one).  Every pixel the source does not call foreground gets the all-zero record.
template <class Src>
__global__ __launch_bounds__(256) void k_dn_prepare(GConstDev g, uint32_t W, uint32_t H, uint32_t flags, Src src, const float4* __restrict__ in,
                                                    float4* __restrict__ gP, float4* __restrict__ gN, float4* __restrict__ sig) {
    const uint32_t px = blockIdx.x * kDnTileX + threadIdx.x, py = blockIdx.y * kDnTileY + threadIdx.y;
    if (px >= W || py >= H) return;
    const size_t pi = (size_t)py * W + px;
    const typename Src::Texel x = src.fetch(pi);
    if (!src.foreground(x)) {
        gP[pi] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        gN[pi] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        sig[pi] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 L = in[pi];
    const DnSurface r = src.surface(g, flags, px, py, pi, x);
    const V3 s = dn_demodulate(L, r.k);
    gP[pi] = make_float4(r.P.x, r.P.y, r.P.z, 1.0f);
    gN[pi] = make_float4(r.n.x, r.n.y, r.n.z, 0.0f);
    sig[pi] = make_float4(s.x, s.y, s.z, 0.0f);
}

// The tile of a workgroup and a HALO-wide border of the three record images, staged in LDS (HALO > 0), or the images themselves (HALO = 0:
// every tap is three 16-byte loads through the caches).  The arithmetic is the same code either way; pixels outside the window are never
// read (the tap loops skip them), so their LDS slots stay unwritten.
template <int HALO>
struct DnTile {
    static constexpr int TW = kDnTileX + 2 * HALO, TH = kDnTileY + 2 * HALO, N = HALO ? TW * TH : 1;
    float4 *sP, *sN, *sS;
    const float4 *gP, *gN, *sin;
    int x0, y0;
    uint32_t W;
    __device__ void stage(uint32_t H) {
        if constexpr (HALO > 0) {
            for (int i = threadIdx.y * kDnTileX + threadIdx.x; i < N; i += kDnTileX * kDnTileY) {
                const int qx = x0 + i % TW, qy = y0 + i / TW;
                if (qx >= 0 && qx < (int)W && qy >= 0 && qy < (int)H) {
                    const size_t qi = (size_t)qy * W + qx;
                    sP[i] = gP[qi];
                    sN[i] = gN[qi];
                    sS[i] = sin[qi];
                }
            }
            __syncthreads();
        }
    }
    RT3_DEV size_t at(int qx, int qy) const {
        if constexpr (HALO > 0) return (size_t)((qy - y0) * TW + (qx - x0));
        else return (size_t)qy * W + qx;
    }
    RT3_DEV float4 P(size_t i) const { return HALO ? sP[i] : gP[i]; }
    RT3_DEV float4 Nn(size_t i) const { return HALO ? sN[i] : gN[i]; }
    RT3_DEV float4 S(size_t i) const { return HALO ? sS[i] : sin[i]; }
};
#define RT3_DN_TILE(HALO)                                                                                                     \
    __shared__ float4 lds_p[DnTile<HALO>::N], lds_n[DnTile<HALO>::N], lds_s[DnTile<HALO>::N];                                  \
    DnTile<HALO> tile = {lds_p, lds_n, lds_s, gP, gN, sin, (int)(blockIdx.x * kDnTileX) - HALO, (int)(blockIdx.y * kDnTileY) - HALO, W}; \
    tile.stage(H)

// TEMPORAL: the "temporal" pass's Moments image {mu1, mu2, variance, N} overrides the spatial estimate where N >= 4 (SVGF's rule)
template <bool TEMPORAL>
__global__ __launch_bounds__(256) void k_dn_variance(uint32_t W, uint32_t H, uint32_t squarings, float inv_sigma_z, const float4* __restrict__ gP,
                                                     const float4* __restrict__ gN, const float4* __restrict__ sin, float4* __restrict__ sout,
                                                     const float4* __restrict__ moments) {
    RT3_DN_TILE(3);
    const uint32_t px = blockIdx.x * kDnTileX + threadIdx.x, py = blockIdx.y * kDnTileY + threadIdx.y;
    if (px >= W || py >= H) return;
    const size_t pi = (size_t)py * W + px, ti = tile.at((int)px, (int)py);
    const float4 cP = tile.P(ti);
    float4 c = tile.S(ti);
    if (cP.w == 0.0f) {  // background
        sout[pi] = c;
        return;
    }
    const float4 cN = tile.Nn(ti);
    const DnCentre p = {v3(cP.x, cP.y, cP.z), v3(cN.x, cN.y, cN.z)};
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int dy = -3; dy <= 3; dy++) {
        const int qy = (int)py + dy;
        if (qy < 0 || qy >= (int)H) continue;
        for (int dx = -3; dx <= 3; dx++) {
            const int qx = (int)px + dx;
            if (qx < 0 || qx >= (int)W) continue;
            const size_t qi = tile.at(qx, qy);
            const float4 q = tile.S(qi);
            float wn, xz;
            dn_geo(p, tile.P(qi), tile.Nn(qi), squarings, inv_sigma_z, wn, xz);
            const float w = wn * expn(xz);
            const float lq = dn_lum(q.x, q.y, q.z);
            s0 = s0 + w;
            s1 = s1 + w * lq;
            s2 = s2 + w * (lq * lq);
        }
    }
    const float mu1 = s1 / s0;
    const float d = s2 / s0 - mu1 * mu1;
    c.w = d > 0.0f ? d : 0.0f;
    if constexpr (TEMPORAL) {
        const float4 mo = moments[pi];
        if (mo.w >= 4.0f) c.w = mo.z;
    }
    sout[pi] = c;
}

template <int HALO>  // 0, or 2 * step
__global__ __launch_bounds__(256) void k_dn_atrous(uint32_t W, uint32_t H, int step, uint32_t squarings, float inv_sigma_z, float sigma_l,
                                                   const float4* __restrict__ gP, const float4* __restrict__ gN, const float4* __restrict__ sin,
                                                   float4* __restrict__ sout) {
    RT3_DN_TILE(HALO);
    const uint32_t px = blockIdx.x * kDnTileX + threadIdx.x, py = blockIdx.y * kDnTileY + threadIdx.y;
    if (px >= W || py >= H) return;
    const size_t pi = (size_t)py * W + px, ti = tile.at((int)px, (int)py);
    const float4 cP = tile.P(ti);
    if (cP.w == 0.0f) {  // background
        sout[pi] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 cN = tile.Nn(ti);
    const float4 c = tile.S(ti);
    const DnCentre p = {v3(cP.x, cP.y, cP.z), v3(cN.x, cN.y, cN.z)};
    // 3 x 3 binomial blur of the variance image over the taps inside the window
    float gs = 0.0f, ks = 0.0f;
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = (int)py + dy;
        if (qy < 0 || qy >= (int)H) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = (int)px + dx;
            if (qx < 0 || qx >= (int)W) continue;
            const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
            gs = gs + k * tile.S(tile.at(qx, qy)).w;
            ks = ks + k;
        }
    }
    const float gv = gs / ks;
    const float inv_l = 1.0f / (sigma_l * sqrtf(gv) + kDnTinyL);
    const float l = dn_lum(c.x, c.y, c.z);
    const float h5[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, ws = 0.0f, vs = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = (int)py + dy * step;
        if (qy < 0 || qy >= (int)H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = (int)px + dx * step;
            if (qx < 0 || qx >= (int)W) continue;
            const size_t qi = tile.at(qx, qy);
            const float4 q = tile.S(qi);
            float wn, xz;
            dn_geo(p, tile.P(qi), tile.Nn(qi), squarings, inv_sigma_z, wn, xz);
            const float dl = dn_lum(q.x, q.y, q.z) - l;
            const float xl = fabsf(dl) * inv_l;
            const float w = ((h5[dy + 2] * h5[dx + 2]) * wn) * expn(xz + xl);
            ar = ar + w * q.x;
            ag = ag + w * q.y;
            ab = ab + w * q.z;
            ws = ws + w;
            vs = vs + (w * w) * q.w;
        }
    }
    sout[pi] = make_float4(ar / ws, ag / ws, ab / ws, vs / (ws * ws));
}

// Out = e + c * m where k_dn_prepare<Src> made a foreground record (Src::prepared: the depth again for the G-buffer, 4 bytes; gP.w, which
// no stage in between writes, for the guide); alpha and every other pixel: In, bit for bit
template <class Src>
__global__ __launch_bounds__(256) void k_dn_finish(uint32_t W, uint32_t H, uint32_t flags, Src src, const float4* __restrict__ gP,
                                                   const float4* __restrict__ in, const float4* __restrict__ sig, float4* __restrict__ out) {
    const uint32_t px = blockIdx.x * kDnTileX + threadIdx.x, py = blockIdx.y * kDnTileY + threadIdx.y;
    if (px >= W || py >= H) return;
    const size_t pi = (size_t)py * W + px;
    float4 L = in[pi];
    if (src.prepared(gP, pi)) {
        const float4 c = sig[pi];
        const V3 r = dn_modulate(v3(c.x, c.y, c.z), src.modulation(flags, pi));
        L.x = r.x;
        L.y = r.y;
        L.z = r.z;
    }
    out[pi] = L;
}

__global__ void k_selftest_expn(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = __float_as_uint(expn(__uint_as_float(in[i])));
}

}  // namespace

void denoise_plan(uint32_t W, uint32_t H, BufLayout& plan, DenoiseScratch* s) {
    const size_t n = (size_t)W * H;
    plan.add(&s->gP, n).add(&s->gN, n).add(&s->sig[0], n).add(&s->sig[1], n);
}
// the two end stages take their records from the guide input where one is set (rt3_denoise_set_guide_input), else from the G-buffer
template <class Launch>
static void with_source(const DenoiseLaunch& L, Launch launch) {
    if (L.guide[0]) launch(DnGuide{L.guide[0], L.guide[1], L.guide[2], L.guide[3]});
    else launch(DnGbuffer{(const uint4*)L.gbuffer, L.depth});
}
// prepare writes sig[0]; the variance stage sig[0] -> sig[1]; iteration i reads sig[(i + 1) & 1] and writes sig[i & 1]
void launch_denoise_prepare(hipStream_t st, const DenoiseLaunch& L) {
    with_source(L, [&](auto src) {
        hipLaunchKernelGGL(k_dn_prepare<decltype(src)>, dn_grid(L.W, L.H), dim3(kDnTileX, kDnTileY), 0, st, L.g, L.W, L.H, L.flags, src,
                           (const float4*)L.in, L.s.gP, L.s.gN, L.s.sig[0]);
    });
}
void launch_denoise_variance(hipStream_t st, const DenoiseLaunch& L) {
    auto k = L.moments ? k_dn_variance<true> : k_dn_variance<false>;
    hipLaunchKernelGGL(k, dn_grid(L.W, L.H), dim3(kDnTileX, kDnTileY), 0, st, L.W, L.H, L.squarings, 1.0f / L.sigma_z, L.s.gP, L.s.gN, L.s.sig[0],
                       L.s.sig[1], (const float4*)L.moments);
}
void launch_denoise_atrous(hipStream_t st, const DenoiseLaunch& L, uint32_t iteration) {
    const uint32_t step = 1u << iteration;
    auto k = step == 1 ? k_dn_atrous<2> : (step == 2 ? k_dn_atrous<4> : k_dn_atrous<0>);  // LDS tiles where they were measured to win
    hipLaunchKernelGGL(k, dn_grid(L.W, L.H), dim3(kDnTileX, kDnTileY), 0, st, L.W, L.H, (int)step, L.squarings, 1.0f / L.sigma_z, L.sigma_l, L.s.gP,
                       L.s.gN, L.s.sig[(iteration + 1u) & 1u], L.s.sig[iteration & 1u]);
}
void launch_denoise_finish(hipStream_t st, const DenoiseLaunch& L, uint32_t iterations) {
    with_source(L, [&](auto src) {
        hipLaunchKernelGGL(k_dn_finish<decltype(src)>, dn_grid(L.W, L.H), dim3(kDnTileX, kDnTileY), 0, st, L.W, L.H, L.flags, src,
                           (const float4*)L.s.gP, (const float4*)L.in, (const float4*)L.s.sig[(iterations - 1u) & 1u], (float4*)L.out);
    });
}
void launch_selftest_denoise(hipStream_t st, const uint32_t* in, uint32_t n, uint32_t* out) {
    hipLaunchKernelGGL(k_selftest_expn, dim3((n + 255) / 256), dim3(256), 0, st, in, n, out);
}

}  // namespace rt3
