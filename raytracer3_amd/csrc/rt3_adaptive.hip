// rt3_adaptive.hip -- the kernels of the "adaptive" pass (include/rt3.h states the semantics): per-pixel sums and
// luminance moments over a compacted pixel list, the convergence test, the stable compaction of the list, and the final divide.
//
// Per-pixel state lives in window space (index y * width + x), so that compacting the list moves nothing:
//   sums[pi] = {sum r, sum g, sum b, n as uint32 bits}     mom[pi] = {S1, S2}     mask[pi] = 1: the pixel's last test failed
// A list is what k_shade reads: the words x | y << 16 and, beside them, the {xy, blue-noise word} records of k_pixbn, in the same order.
#include <hip/hip_runtime.h>

#include "rt3_internal.hpp"
#include "rt3_math.hpp"

namespace rt3 {

namespace {

constexpr int kAdBlock = 256, kAdWaves = kAdBlock / 64;
constexpr int kAdItems = 8;                       // list entries per thread of a compaction block
constexpr uint32_t kAdTile = kAdBlock * kAdItems;  // ... and per block
static_assert(kAdTile == kAdaptiveTile, "rt3_internal.hpp states the tile for whoever reads block_count");

// Round 0's input: foreground pixels of the rank's list count as "failed" (so the first compaction keeps exactly them); a background pixel
// gets Moments = 0 and is never listed.  `mask` was zeroed for the whole window before: pixels of other ranks stay 0.
__global__ void k_ad_init(const uint32_t* __restrict__ pixels, uint32_t npix, uint32_t width, const float* __restrict__ depth,
                          uint8_t* __restrict__ mask, float4* __restrict__ moments) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        const uint32_t xy = pixels[i];
        const size_t pi = (size_t)(xy >> 16) * width + (xy & 0xFFFFu);
        if (depth[pi] == kBackgroundDepth) moments[pi] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        else mask[pi] = 1;
    }
}

// k_accumulate's loop (the colour sums start at 0.0f and take the samples in order, whatever the batch split) plus S1 = sum y and
// S2 = sum y * y, y = luminance(sample).  n_after: the pixel's sample count once this batch is in.
__global__ void k_ad_accumulate(const uint32_t* __restrict__ pixels, uint32_t npix, uint32_t width, const float* __restrict__ lacc, uint32_t sb,
                                int first, uint32_t n_after, float4* __restrict__ sums, float2* __restrict__ mom) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        const uint32_t xy = pixels[i];
        const size_t pi = (size_t)(xy >> 16) * width + (xy & 0xFFFFu);
        float r = 0.0f, gg = 0.0f, bb = 0.0f, s1 = 0.0f, s2 = 0.0f;
        if (!first) {
            const float4 sv = sums[pi];
            const float2 mv = mom[pi];
            r = sv.x, gg = sv.y, bb = sv.z, s1 = mv.x, s2 = mv.y;
        }
        for (uint32_t s = 0; s < sb; s++) {
            const float4 lv = reinterpret_cast<const float4*>(lacc)[(size_t)s * npix + i];
            r += lv.x;
            gg += lv.y;
            bb += lv.z;
            const float y = luminance(v3(lv.x, lv.y, lv.z));
            s1 += y;
            s2 += y * y;
        }
        sums[pi] = make_float4(r, gg, bb, __uint_as_float(n_after));
        mom[pi] = make_float2(s1, s2);
    }
}

// The convergence test of one listed pixel, in the header's operation order.  A NaN fails (the comparison is false): such a pixel runs to the cap.
__global__ void k_ad_test(const uint32_t* __restrict__ pixels, uint32_t npix, uint32_t width, const float4* __restrict__ sums,
                          const float2* __restrict__ mom, float threshold, float dark, uint8_t* __restrict__ mask) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        const uint32_t xy = pixels[i];
        const size_t pi = (size_t)(xy >> 16) * width + (xy & 0xFFFFu);
        const float n = (float)__float_as_uint(sums[pi].w);
        const float2 mv = mom[pi];
        const float mean = mv.x / n;
        float var = (mv.y - mv.x * mean) / (n - 1.0f);
        var = var < 0.0f ? 0.0f : var;
        const float rel = threshold * (mean + dark);
        mask[pi] = var <= (rel * rel) * n ? 0 : 1;
    }
}

// does the listed pixel xy stay: its own test failed or, with dilate, that of a pixel of its 3 x 3 neighbourhood inside the window (whatever
// is not a listed foreground pixel of this rank has mask 0)
__device__ __forceinline__ bool ad_keep(uint32_t xy, uint32_t W, uint32_t H, const uint8_t* __restrict__ mask, uint32_t dilate) {
    const uint32_t x = xy & 0xFFFFu, y = xy >> 16;
    if (mask[(size_t)y * W + x]) return true;
    if (!dilate) return false;
    const uint32_t x0 = x ? x - 1 : 0, x1 = x + 1 < W ? x + 1 : W - 1, y0 = y ? y - 1 : 0, y1 = y + 1 < H ? y + 1 : H - 1;
    uint32_t any = 0;
    for (uint32_t yy = y0; yy <= y1; yy++)
        for (uint32_t xx = x0; xx <= x1; xx++) any |= mask[(size_t)yy * W + xx];
    return any != 0;
}

// Compaction, first of three launches: block b counts the entries it keeps of its tile [b kAdTile, (b + 1) kAdTile) of the list.
__global__ __launch_bounds__(kAdBlock) void k_ad_count(const uint2* __restrict__ in_bn, uint32_t n_in, uint32_t W, uint32_t H,
                                                       const uint8_t* __restrict__ mask, uint32_t dilate, uint32_t* __restrict__ block_count) {
    __shared__ uint32_t lds[kAdWaves];
    uint32_t kept = 0;  // of the wave (every lane holds the same number)
    for (int k = 0; k < kAdItems; k++) {
        const uint32_t i = blockIdx.x * kAdTile + k * kAdBlock + threadIdx.x;
        const bool keep = i < n_in && ad_keep(in_bn[i].x, W, H, mask, dilate);
        kept += (uint32_t)__popcll(__ballot(keep));
    }
    if (__lane_id() == 0) lds[threadIdx.x >> 6] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kAdWaves; w++) t += lds[w];
        block_count[blockIdx.x] = t;
    }
}
// second: the counts become exclusive offsets in place, the total goes to *count.  One block; a wave scans 64 counts with shuffles, the
// wave totals meet in LDS, and the running total carries from one chunk of kAdBlock counts to the next.
__global__ __launch_bounds__(kAdBlock) void k_ad_scan(uint32_t* __restrict__ block_count, uint32_t n_blocks, uint32_t* __restrict__ count) {
    __shared__ uint32_t lds[2][kAdWaves];
    const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
    uint32_t carry = 0, parity = 0;
    for (uint32_t base = 0; base < n_blocks; base += kAdBlock) {  // (uniform: every thread takes every iteration)
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_blocks ? block_count[i] : 0u;
        uint32_t x = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(x, d);
            if ((int)lane >= d) x += t;
        }
        if (lane == 63) lds[parity][wave] = x;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < (uint32_t)kAdWaves; w++) {
            const uint32_t t = lds[parity][w];
            before += w < wave ? t : 0u;
            total += t;
        }
        if (i < n_blocks) block_count[i] = carry + before + (x - v);
        carry += total;
        parity ^= 1u;  // two buffers: a wave that runs ahead writes the other one
    }
    if (threadIdx.x == 0) *count = carry;
}
// third: every block writes what it keeps from its offset on, in the list's order: entry (k, wave, lane) goes behind everything of an
// earlier k, an earlier wave or a lower lane.  The new list is a stable subsequence of the old one.
__global__ __launch_bounds__(kAdBlock) void k_ad_scatter(const uint2* __restrict__ in_bn, uint32_t n_in, uint32_t W, uint32_t H,
                                                         const uint8_t* __restrict__ mask, uint32_t dilate, const uint32_t* __restrict__ block_off,
                                                         uint32_t* __restrict__ out_xy, uint2* __restrict__ out_bn) {
    __shared__ uint32_t lds[2][kAdWaves];
    const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t at = block_off[blockIdx.x];
    for (int k = 0; k < kAdItems; k++) {
        const uint32_t i = blockIdx.x * kAdTile + k * kAdBlock + threadIdx.x;
        uint2 rec = make_uint2(0u, 0u);
        if (i < n_in) rec = in_bn[i];
        const bool keep = i < n_in && ad_keep(rec.x, W, H, mask, dilate);
        const unsigned long long m = __ballot(keep);
        if (lane == 0) lds[k & 1][wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < (uint32_t)kAdWaves; w++) {
            const uint32_t t = lds[k & 1][w];
            before += w < wave ? t : 0u;
            total += t;
        }
        if (keep) {
            const uint32_t j = at + before + (uint32_t)__popcll(m & below);  // < the total the scan reported <= n_in
            out_xy[j] = rec.x;
            out_bn[j] = rec;
        }
        at += total;
    }
}

// Light = sums / (float)n, then k_accumulate's blend; Moments = {S1, S2, n, stopped before the cap ? 1 : 0}.  Background: untouched.
__global__ void k_ad_finalise(const uint32_t* __restrict__ pixels, uint32_t npix, uint32_t width, const float* __restrict__ depth, float blendfactor,
                              uint32_t cap, const float4* __restrict__ sums, const float2* __restrict__ mom, float4* __restrict__ light,
                              const float4* __restrict__ prev, float4* __restrict__ moments) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        const uint32_t xy = pixels[i];
        const size_t pi = (size_t)(xy >> 16) * width + (xy & 0xFFFFu);
        if (depth[pi] == kBackgroundDepth) continue;
        const float4 sv = sums[pi];
        const float2 mv = mom[pi];
        const uint32_t n = __float_as_uint(sv.w);
        const float fs = (float)n;
        const float r = sv.x / fs, gg = sv.y / fs, bb = sv.z / fs;
        if (blendfactor >= 1.0f) {
            light[pi] = make_float4(r, gg, bb, 0.0f);
        } else {
            const float4 pv = prev[pi];
            const float bf = blendfactor;
            light[pi] = make_float4(pv.x + (r - pv.x) * bf, pv.y + (gg - pv.y) * bf, pv.z + (bb - pv.z) * bf, 0.0f);
        }
        moments[pi] = make_float4(mv.x, mv.y, fs, n < cap ? 1.0f : 0.0f);
    }
}

// Coverage mode (rt3_adaptive_set_coverage): k_ad_finalise for every listed pixel.  A pixel whose centre sees the background may be partly
// covered and was sampled like any other, so there is no depth test; the blend is k_accumulate_lens's.  Streaming: 4 + 16 + 8 (+ 16) bytes
// read and 32 written per pixel, sums and mom in window order under a list of row-major tiles; no LDS.
__global__ __launch_bounds__(256) void k_ad_finalise_all(const uint32_t* __restrict__ pixels, uint32_t npix, uint32_t width, float blendfactor,
                                                         uint32_t cap, const float4* __restrict__ sums, const float2* __restrict__ mom,
                                                         float4* __restrict__ light, const float4* __restrict__ prev, float4* __restrict__ moments) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        const uint32_t xy = pixels[i];
        const size_t pi = (size_t)(xy >> 16) * width + (xy & 0xFFFFu);
        const float4 sv = sums[pi];
        const float2 mv = mom[pi];
        const uint32_t n = __float_as_uint(sv.w);
        const float fs = (float)n;
        const float r = sv.x / fs, gg = sv.y / fs, bb = sv.z / fs;
        if (blendfactor >= 1.0f) {
            light[pi] = make_float4(r, gg, bb, 0.0f);
        } else {
            const float4 pv = prev[pi];
            const float bf = blendfactor;
            light[pi] = make_float4(pv.x + (r - pv.x) * bf, pv.y + (gg - pv.y) * bf, pv.z + (bb - pv.z) * bf, 0.0f);
        }
        moments[pi] = make_float4(mv.x, mv.y, fs, n < cap ? 1.0f : 0.0f);
    }
}

}  // namespace

void adaptive_plan(uint32_t W, uint32_t H, uint32_t npix, BufLayout& plan, AdaptiveScratch* s) {
    const size_t win = (size_t)W * H, list = npix ? npix : 1;
    plan.add(&s->sums, win).add(&s->mom, win).add(&s->mask, win);
    for (int k = 0; k < 2; k++) plan.add(&s->xy[k], list).add(&s->bn[k], list);
    plan.add(&s->block_count, (list + kAdTile - 1) / kAdTile).add(&s->count, 1);
}
void launch_adaptive_init(hipStream_t st, const uint32_t* pixels, uint32_t npix, uint32_t width, const float* depth, const AdaptiveScratch& s,
                          void* moments) {
    hipLaunchKernelGGL(k_ad_init, dim3(grid_for(npix, 256, 8192)), dim3(256), 0, st, pixels, npix, width, depth, s.mask, (float4*)moments);
}
void launch_adaptive_accumulate(hipStream_t st, const uint32_t* pixels, uint32_t npix, uint32_t width, const float* lacc, uint32_t sb, bool first,
                                uint32_t n_after, const AdaptiveScratch& s) {
    hipLaunchKernelGGL(k_ad_accumulate, dim3(grid_for(npix, 256, 8192)), dim3(256), 0, st, pixels, npix, width, lacc, sb, first ? 1 : 0, n_after,
                       s.sums, s.mom);
}
void launch_adaptive_test(hipStream_t st, const uint32_t* pixels, uint32_t npix, uint32_t width, float threshold, float dark,
                          const AdaptiveScratch& s) {
    hipLaunchKernelGGL(k_ad_test, dim3(grid_for(npix, 256, 8192)), dim3(256), 0, st, pixels, npix, width, s.sums, s.mom, threshold, dark, s.mask);
}
void launch_adaptive_compact(hipStream_t st, const uint2* in_bn, uint32_t n_in, uint32_t W, uint32_t H, uint32_t dilate, const AdaptiveScratch& s,
                             int out) {
    const uint32_t n_blocks = (n_in + kAdTile - 1) / kAdTile;  // n_in >= 1
    hipLaunchKernelGGL(k_ad_count, dim3(n_blocks), dim3(kAdBlock), 0, st, in_bn, n_in, W, H, s.mask, dilate, s.block_count);
    hipLaunchKernelGGL(k_ad_scan, dim3(1), dim3(kAdBlock), 0, st, s.block_count, n_blocks, s.count);
    hipLaunchKernelGGL(k_ad_scatter, dim3(n_blocks), dim3(kAdBlock), 0, st, in_bn, n_in, W, H, s.mask, dilate, s.block_count, s.xy[out], s.bn[out]);
}
void launch_adaptive_finalise(hipStream_t st, const uint32_t* pixels, uint32_t npix, uint32_t width, const float* depth, float blendfactor,
                              uint32_t cap, const AdaptiveScratch& s, void* light, const void* prev, void* moments) {
    hipLaunchKernelGGL(k_ad_finalise, dim3(grid_for(npix, 256, 8192)), dim3(256), 0, st, pixels, npix, width, depth, blendfactor, cap, s.sums, s.mom,
                       (float4*)light, (const float4*)prev, (float4*)moments);
}
void launch_adaptive_finalise_all(hipStream_t st, const uint32_t* pixels, uint32_t npix, uint32_t width, float blendfactor, uint32_t cap,
                                  const AdaptiveScratch& s, void* light, const void* prev, void* moments) {
    hipLaunchKernelGGL(k_ad_finalise_all, dim3(grid_for(npix, 256, 8192)), dim3(256), 0, st, pixels, npix, width, blendfactor, cap, s.sums, s.mom,
                       (float4*)light, (const float4*)prev, (float4*)moments);
}

}  // namespace rt3
