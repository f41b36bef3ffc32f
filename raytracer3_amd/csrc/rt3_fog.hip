// rt3_fog.hip -- k_fog_segment and k_fog_shadow: a homogeneous medium with single scattering, on the extension queue behind every k_extend
// and on the shadow queues between k_shade and their k_shadow (rt3_scene_set_medium), and the kernel of self-test op
// 45.  Kernels of their own names, launched only while a medium is set: no instance of k_shade, k_extend or k_shadow changes.
#include <hip/hip_runtime.h>

#include "rt3_fog.hpp"
#include "rt3_internal.hpp"
#include "rt3_math.hpp"
#include "rt3_punctual.hpp"
#include "rt3_rng.hpp"
#include "rt3_sky.hpp"

namespace rt3 {

constexpr int kFogBlock = 256;
constexpr int kFogWaves = kFogBlock / 64;
constexpr unsigned kFogMaxBlocks = 8192;

// Queue append for a whole workgroup, two queues (block_append1 of rt3_roulette.hip has the scheme): every wave ballots its lanes, the wave
// totals meet in LDS and thread 0 reserves each queue's range with ONE returning atomic.  The third ballot only counts (segments in the
// medium).  Must be reached by all threads of the block; the caller alternates between two lds buffers from one iteration to the next.
struct FogAppend {
    uint32_t slot[2];
};
constexpr int kFogLdsWords = 3 * kFogWaves + 2;
__device__ __forceinline__ FogAppend fog_append(bool w0, bool w1, bool seg, uint32_t* const* count, uint32_t* lds, unsigned long long& n_seg,
                                                unsigned long long& n_rays) {
    const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
    const unsigned long long m0 = __ballot(w0), m1 = __ballot(w1), ms = __ballot(seg);
    if (lane == 0) {
        lds[wave] = (uint32_t)__popcll(m0);
        lds[kFogWaves + wave] = (uint32_t)__popcll(m1);
        lds[2 * kFogWaves + wave] = (uint32_t)__popcll(ms);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t0 = 0, t1 = 0, ts = 0;
#pragma unroll
        for (int w = 0; w < kFogWaves; w++) {
            const uint32_t c0 = lds[w], c1 = lds[kFogWaves + w];
            lds[w] = t0;
            lds[kFogWaves + w] = t1;
            t0 += c0;
            t1 += c1;
            ts += lds[2 * kFogWaves + w];
        }
        lds[3 * kFogWaves] = t0 ? atomicAdd(count[0], t0) : 0u;
        lds[3 * kFogWaves + 1] = t1 ? atomicAdd(count[1], t1) : 0u;
        n_seg += ts;
        n_rays += t0 + t1;
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    FogAppend r;
    r.slot[0] = lds[3 * kFogWaves] + lds[wave] + (uint32_t)__popcll(m0 & below);
    r.slot[1] = lds[3 * kFogWaves + 1] + lds[kFogWaves + wave] + (uint32_t)__popcll(m1 & below);
    return r;
}

// Streaming, one thread per record: the hit record and the two ray records decide whether the segment meets the box; only then are the
// three throughput words read and written, and only with `scatter` are the point, the light samples (the sky's two table lookups and four
// texels; the light table's guide, CDF and record, and a textured emitter's texels) and the two appends' stores made.
__global__ __launch_bounds__(kFogBlock) void k_fog_segment(FogSegmentLaunch a) {
    __shared__ uint32_t append_lds[2][kFogLdsWords];
    const size_t S = a.stride, QS = a.q_stride;
    const uint32_t n = *a.count;
    const uint32_t n_round = (n + (kFogBlock - 1)) & ~(uint32_t)(kFogBlock - 1);  // whole workgroups iterate: barriers inside
    uint32_t parity = 0;
    unsigned long long n_seg = 0ull, n_rays = 0ull;  // thread 0's
    uint32_t* const counts[2] = {a.q_count[0], a.q_count[1]};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += gridDim.x * blockDim.x) {
        bool seg = false, e0 = false, e1 = false;
        V3 x = v3(0.0f, 0.0f, 0.0f), w0 = v3(0.0f, 1.0f, 0.0f), w1 = w0, c0 = x, c1 = x;
        float tm1 = 0.0f;
        uint32_t pid = 0;
        if (i < n) {
            const float4 hrec = reinterpret_cast<const float4*>(a.hits)[i];
            const float4 ro = reinterpret_cast<const float4*>(a.rays)[i];
            const float4 rd = reinterpret_cast<const float4*>(a.rays)[S + i];
            pid = __float_as_uint(rd.w);
            const bool miss = __float_as_uint(hrec.w) == kMiss;
            const V3 o = v3(ro.x, ro.y, ro.z), d = v3(rd.x, rd.y, rd.z);
            float t0, t1;
            seg = fog_span(o, d, miss ? __uint_as_float(0x7F800000u) : hrec.x, a.fog, t0, t1);
            if (seg) {
                const float dl = sqrtf(dot(d, d)), len = (t1 - t0) * dl;
                const V3 Tb = v3(a.T[i], a.T[S + i], a.T[2 * S + i]);
                const V3 tr = fog_transmittance(a.fog, len);
                a.T[i] = Tb.x * tr.x;
                a.T[S + i] = Tb.y * tr.y;
                a.T[2 * S + i] = Tb.z * tr.z;
                if (a.lacc_miss != nullptr && miss) {
                    float4* Lp = reinterpret_cast<float4*>(a.lacc_miss) + pid;
                    const float4 lv = *Lp;
                    *Lp = make_float4(lv.x * tr.x, lv.y * tr.y, lv.z * tr.z, lv.w);
                }
                if (a.scatter && (Tb.x > 0.0f || Tb.y > 0.0f || Tb.z > 0.0f)) {
                    const uint32_t sample_in_batch = fast_div(a.npix_div, pid);
                    const uint32_t xy = a.pixels[pid - sample_in_batch * a.npix];
                    const uint32_t seed = rng_seed(xy & 0xFFFFu, xy >> 16, a.frame);
                    const uint32_t base = kFogRngBase + ((a.s0 + sample_in_batch) * a.bounces + a.segment) * kFogRngDims;
                    const FogPoint p = fog_sample_distance(fog_sigma_bar(a.fog), len, uniform_float(seed, base));
                    const float s = t0 + p.ds / dl;
                    x = v3(o.x + s * d.x, o.y + s * d.y, o.z + s * d.z);
                    // T_before expf(-(sigma_t ds)) sigma_s / pdf
                    const V3 w = v3(Tb.x * (expf(-(a.fog.sigma_t[0] * p.ds)) * a.fog.sigma_s[0] / p.pdf),
                                    Tb.y * (expf(-(a.fog.sigma_t[1] * p.ds)) * a.fog.sigma_s[1] / p.pdf),
                                    Tb.z * (expf(-(a.fog.sigma_t[2] * p.ds)) * a.fog.sigma_s[2] / p.pdf));
                    if (a.sky) {
                        V3 rad;
                        float pl;
                        sky_sample(a.sc, uniform_float(seed, base + 3), uniform_float(seed, base + 4), w0, rad, pl);
                        if (pl > 0.0f) {
                            const float k = fog_phase(a.fog.g, dot(d, w0) / dl) / pl;
                            const V3 ts = fog_shadow_transmittance(a.fog, x, w0, kBackgroundDepth);
                            c0 = v3(w.x * (rad.x * k) * ts.x, w.y * (rad.y * k) * ts.y, w.z * (rad.z * k) * ts.z);
                            e0 = c0.x > 0.0f || c0.y > 0.0f || c0.z > 0.0f;
                        }
                    }
                    if (a.lights.n != 0u) {
                        const uint32_t ke = (uint32_t)(uniform_float(seed, base + 5) * 8388608.0f);  // k_shade's pick
                        const float eu6 = uniform_float(seed, base + 6), eu7 = uniform_float(seed, base + 7);
                        const uint32_t e = light_find(a.lights, ke);
                        const float4* R = a.lights.rec + 4 * (size_t)e;
                        const float4 er0 = R[0], er1 = R[1], er2 = R[2], er3 = R[3];
                        V3 le = v3(0.0f, 0.0f, 0.0f);  // L_e / pdf_light
                        if (er0.w > 0.0f && is_punctual_record(er3)) {  // (er0.w = p_sel; the cosine a surface would add is left out)
                            const PunctualSample ls = punctual_sample(er0, er1, er2, er3, x, d, kEmitShadowEnd);
                            if (ls.geo > 0.0f) {
                                const float sc = ls.geo / er0.w;
                                w1 = ls.wl;
                                tm1 = ls.tmax;
                                le = v3(ls.Ic.x * sc, ls.Ic.y * sc, ls.Ic.z * sc);
                            }
                        } else if (er0.w > 0.0f) {  // k_shade's point: p = A + b1 E1 + b2 E2, b1 = u7 sqrt(u6), b2 = sqrt(u6) - b1
                            const float su = sqrtf(eu6), lb1 = eu7 * su, lb2 = su - lb1;
                            const V3 pe = v3(er0.x + er1.x * lb1 + er2.x * lb2, er0.y + er1.y * lb1 + er2.y * lb2, er0.z + er1.z * lb1 + er2.z * lb2);
                            const V3 wv = pe - x;
                            const float dist2 = dot(wv, wv), dist = sqrtf(dist2);
                            if (dist2 > 0.0f) {
                                w1 = wv * (1.0f / dist);
                                const float cle = fabsf(er3.x * w1.x + er3.y * w1.y + er3.z * w1.z);  // emission is two-sided
                                if (cle > 0.0f) {
                                    const float ps = er0.w * dist2 / cle;  // p_sel / area * dist^2 / |cos_l|
                                    le = v3(er1.w / ps, er2.w / ps, er3.w / ps);
                                    tm1 = dist * kEmitShadowEnd;
                                    if (a.emit_tex != nullptr) {
                                        const EmitTexDev t = a.emit_tex[e];
                                        if (t.tex >= 0) le = le * emit_tex_rgb(a.sc, t, lb1, lb2);
                                    }
                                }
                            }
                        }
                        if (le.x > 0.0f || le.y > 0.0f || le.z > 0.0f) {
                            const float k = fog_phase(a.fog.g, dot(d, w1) / dl);
                            const V3 ts = fog_shadow_transmittance(a.fog, x, w1, tm1);
                            c1 = v3(w.x * (le.x * k) * ts.x, w.y * (le.y * k) * ts.y, w.z * (le.z * k) * ts.z);
                            e1 = c1.x > 0.0f || c1.y > 0.0f || c1.z > 0.0f;
                        }
                    }
                }
            }
        }
        const FogAppend slot = fog_append(e0, e1, seg, counts, append_lds[parity], n_seg, n_rays);
        parity ^= 1u;
        if (e0) {
            const uint32_t j = slot.slot[0];
            reinterpret_cast<float4*>(a.q_rays[0])[j] = make_float4(x.x, x.y, x.z, c0.x);
            reinterpret_cast<float4*>(a.q_rays[0])[QS + j] = make_float4(w0.x, w0.y, w0.z, c0.y);
            reinterpret_cast<float2*>(a.q_contrib[0])[j] = make_float2(c0.z, __uint_as_float(pid));
            a.q_tmax[0][j] = kBackgroundDepth;
        }
        if (e1) {
            const uint32_t j = slot.slot[1];
            reinterpret_cast<float4*>(a.q_rays[1])[j] = make_float4(x.x, x.y, x.z, c1.x);
            reinterpret_cast<float4*>(a.q_rays[1])[QS + j] = make_float4(w1.x, w1.y, w1.z, c1.y);
            reinterpret_cast<float2*>(a.q_contrib[1])[j] = make_float2(c1.z, __uint_as_float(pid));
            a.q_tmax[1][j] = tm1;
        }
    }
    if (threadIdx.x == 0 && a.info != nullptr) {
        if (n_seg) atomicAdd(&a.info[0], n_seg);
        if (n_rays) atomicAdd(&a.info[1], n_rays);
    }
}

// Pure streaming, one thread per queued ray: 44 bytes in (40 without a range end), 12 bytes out where the ray meets the box.
__global__ __launch_bounds__(kFogBlock) void k_fog_shadow(FogShadowLaunch a) {
    const size_t S = a.stride;
    const uint32_t n = *a.count;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 ro = reinterpret_cast<const float4*>(a.rays)[i];
        const float4 rd = reinterpret_cast<const float4*>(a.rays)[S + i];
        const float tmax = a.tmax != nullptr ? a.tmax[i] : kBackgroundDepth;
        const V3 o = v3(ro.x, ro.y, ro.z), d = v3(rd.x, rd.y, rd.z);
        float t0, t1;
        if (!fog_span(o, d, tmax, a.fog, t0, t1)) continue;
        const V3 tr = fog_transmittance(a.fog, (t1 - t0) * sqrtf(dot(d, d)));
        a.rays[4 * (size_t)i + 3] = ro.w * tr.x;
        a.rays[4 * (S + i) + 3] = rd.w * tr.y;
        a.contrib[2 * (size_t)i] = a.contrib[2 * (size_t)i] * tr.z;
    }
}

// self-test op 45: {o xyz, d xyz, t, lo xyz, hi xyz, sigma_a rgb, sigma_s rgb, u} -> {in medium, t0, t1, s, pdf, Tr rgb}
__global__ void k_selftest_fog(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* p = in + kSelftestFogIn * (size_t)i;
    auto F = [](uint32_t u) { return __uint_as_float(u); };
    FogDev f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        f.lo[k] = F(p[7 + k]);
        f.hi[k] = F(p[10 + k]);
        f.sigma_s[k] = F(p[16 + k]);
        f.sigma_t[k] = F(p[13 + k]) + F(p[16 + k]);
    }
    f.g = 0.0f;
    const V3 o = v3(F(p[0]), F(p[1]), F(p[2])), d = v3(F(p[3]), F(p[4]), F(p[5]));
    uint32_t* q = out + kSelftestFogOut * (size_t)i;
    float t0, t1;
    const bool seg = fog_span(o, d, F(p[6]), f, t0, t1);
    q[0] = seg ? 1u : 0u;
#pragma unroll
    for (int k = 1; k < 8; k++) q[k] = 0u;
    if (!seg) return;
    const float dl = sqrtf(dot(d, d)), len = (t1 - t0) * dl;
    const FogPoint pt = fog_sample_distance(fog_sigma_bar(f), len, F(p[19]));
    const V3 tr = fog_transmittance(f, len);
    q[1] = __float_as_uint(t0); q[2] = __float_as_uint(t1);
    q[3] = __float_as_uint(t0 + pt.ds / dl); q[4] = __float_as_uint(pt.pdf);
    q[5] = __float_as_uint(tr.x); q[6] = __float_as_uint(tr.y); q[7] = __float_as_uint(tr.z);
}

void launch_fog_segment(hipStream_t st, const FogSegmentLaunch& launch, uint32_t n_max, uint32_t groups) {
    FogSegmentLaunch a = launch;
    a.npix_div = make_fastdiv(a.npix);
    const unsigned grid = groups ? groups : grid_for(n_max, kFogBlock, kFogMaxBlocks);
    hipLaunchKernelGGL(k_fog_segment, dim3(grid), dim3(kFogBlock), 0, st, a);
}
void launch_fog_shadow(hipStream_t st, const FogShadowLaunch& a, uint32_t n_max, uint32_t groups) {
    const unsigned grid = groups ? groups : grid_for(n_max, kFogBlock, kFogMaxBlocks);
    hipLaunchKernelGGL(k_fog_shadow, dim3(grid), dim3(kFogBlock), 0, st, a);
}
void launch_selftest_fog(hipStream_t st, const uint32_t* in, uint32_t n, uint32_t* out) {
    hipLaunchKernelGGL(k_selftest_fog, dim3((n + 255) / 256), dim3(256), 0, st, in, n, out);
}

}  // namespace rt3
