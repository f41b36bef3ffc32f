// rt3_shade.hip -- the path-tracing shade step: k_shade (one bounce of every live path, with its queue appends) and k_accumulate.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rt3_bsdf.hpp"
#include "rt3_camera.hpp"
#include "rt3_glass.hpp"
#include "rt3_internal.hpp"
#include "rt3_leaf_test.hpp"
#include "rt3_math.hpp"
#include "rt3_punctual.hpp"
#include "rt3_rng.hpp"
#include "rt3_sky.hpp"
#include "rt3_surface.hpp"

namespace rt3 {

// ------------------------------------------------------------------------------------------------ shading
// Queue append for a whole workgroup: every wave ballots its lanes, the wave totals meet in LDS and ONE returning
// atomic per workgroup and queue reserves the range (a single counter word sustains only ~88 returning atomics per
// microsecond chip-wide, so one atomic per wave made k_shade atomic-bound: 1 M atomics per launch ~ 10 ms).
// Order is preserved inside the workgroup.  Must be reached by all threads of the block.
constexpr int kShadeBlock = 512;
struct BlockAppend {
    uint32_t ext, sh;
};
__device__ __forceinline__ BlockAppend block_append2(bool want_ext, bool want_sh, unsigned long long* pair /* {ext count, shadow count} */,
                                                     uint32_t* lds /* 2 * (waves + 1) words */) {
    constexpr int kWaves = kShadeBlock / 64;
    const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
    const unsigned long long m_ext = __ballot(want_ext), m_sh = __ballot(want_sh);
    if (lane == 0) {
        lds[wave] = (uint32_t)__popcll(m_ext);
        lds[kWaves + 1 + wave] = (uint32_t)__popcll(m_sh);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t te = 0, ts = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
            uint32_t ce = lds[w], cs = lds[kWaves + 1 + w];
            lds[w] = te;
            lds[kWaves + 1 + w] = ts;
            te += ce;
            ts += cs;
        }
        // both queue sizes live in one 8-byte word and move with ONE returning atomic (they used to be two atomics on the same
        // cache line, i.e. on the same L2 atomic unit: the unit's throughput is what a 256-thread block size ran into)
        unsigned long long old = 0ull;
        if (te | ts) old = atomicAdd(pair, (unsigned long long)te | ((unsigned long long)ts << 32));
        lds[kWaves] = (uint32_t)old;
        lds[2 * kWaves + 1] = (uint32_t)(old >> 32);
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    BlockAppend r;
    r.ext = lds[kWaves] + lds[wave] + (uint32_t)__popcll(m_ext & below);
    r.sh = lds[2 * kWaves + 1] + lds[kWaves + 1 + wave] + (uint32_t)__popcll(m_sh & below);
    return r;  // no third barrier: the caller alternates between two lds buffers from one loop iteration to the next
}
// block_append2 plus the emitter shadow queue of RT3_F_NEE_EMISSIVE (k_shade<.., .., true> only): the pair moves with its one 64-bit atomic
// as before, the third count with one 32-bit atomic of its own
struct BlockAppend3 {
    uint32_t ext, sh, sh2;
};
__device__ __forceinline__ BlockAppend3 block_append3(bool want_ext, bool want_sh, bool want_sh2, unsigned long long* pair, uint32_t* count2,
                                                      uint32_t* lds /* 3 * (waves + 1) words */) {
    constexpr int kWaves = kShadeBlock / 64, kW1 = kWaves + 1;
    const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
    const unsigned long long m_ext = __ballot(want_ext), m_sh = __ballot(want_sh), m_sh2 = __ballot(want_sh2);
    if (lane == 0) {
        lds[wave] = (uint32_t)__popcll(m_ext);
        lds[kW1 + wave] = (uint32_t)__popcll(m_sh);
        lds[2 * kW1 + wave] = (uint32_t)__popcll(m_sh2);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t te = 0, ts = 0, t2 = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
            const uint32_t ce = lds[w], cs = lds[kW1 + w], c2 = lds[2 * kW1 + w];
            lds[w] = te;
            lds[kW1 + w] = ts;
            lds[2 * kW1 + w] = t2;
            te += ce;
            ts += cs;
            t2 += c2;
        }
        unsigned long long old = 0ull;
        if (te | ts) old = atomicAdd(pair, (unsigned long long)te | ((unsigned long long)ts << 32));
        lds[kWaves] = (uint32_t)old;
        lds[kW1 + kWaves] = (uint32_t)(old >> 32);
        lds[2 * kW1 + kWaves] = t2 ? atomicAdd(count2, t2) : 0u;
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    BlockAppend3 r;
    r.ext = lds[kWaves] + lds[wave] + (uint32_t)__popcll(m_ext & below);
    r.sh = lds[kW1 + kWaves] + lds[kW1 + wave] + (uint32_t)__popcll(m_sh & below);
    r.sh2 = lds[2 * kW1 + kWaves] + lds[2 * kW1 + wave] + (uint32_t)__popcll(m_sh2 & below);
    return r;
}
// (kEmitShadowEnd, where an emitter's or a punctual light's shadow ray ends, is rt3_punctual.hpp's)

// One trip of k_light's loop.  The workgroup looks at slots it .. of the deferred shadow queue, one per thread: slot j
// holds, in the two planes of sh_contrib, the queue index of the vertex that sent ray j (k_shade_defer) and whether the ray was occluded
// (k_shadow's reporting mode).  The indices of the unoccluded ones are packed into LDS behind the `held` ones earlier trips left there, in
// slot order.  Once a workgroup's worth is packed -- or on the last trip, it >= n_round, which finds no slot and takes what is left -- every
// thread gets one: `i`, with `active` saying whether there was one for it; the rest moves to the front.  Returns false when the workgroup
// shades nothing this trip.  No atomics: the packing never leaves the workgroup.  Must be reached by all threads of the block, with `it`
// of one trip either below n_round for all of them or not (n_round and the loop's stride are multiples of the block).
__device__ __forceinline__ bool light_next(const ShadeLaunch& a, uint32_t it, uint32_t n, uint32_t n_round, uint32_t& held, uint32_t& i, bool& active) {
    constexpr int kWaves = kShadeBlock / 64;
    __shared__ uint32_t packed[2 * kShadeBlock];  // held < kShadeBlock before a trip adds at most kShadeBlock
    __shared__ uint32_t wave_count[kWaves];
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.sh_contrib);
    const uint32_t* occluded = src + a.stride;
    bool keep = false;
    uint32_t s = 0;
    if (it < n) {
        keep = occluded[it] == 0u;
        s = src[it];
    }
    const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_count[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
        const uint32_t c = wave_count[w];
        before += (uint32_t)w < wave ? c : 0u;
        total += c;
    }
    if (keep) packed[held + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = s;
    held += total;
    __syncthreads();  // (the next trip writes wave_count behind this barrier, and packed behind its own first one)
    if (held < (uint32_t)kShadeBlock && !(it >= n_round && held != 0u)) return false;
    const uint32_t take = held < (uint32_t)kShadeBlock ? held : (uint32_t)kShadeBlock;
    active = threadIdx.x < take;
    i = active ? packed[threadIdx.x] : 0u;
    held -= take;
    if (threadIdx.x < held) packed[threadIdx.x] = packed[kShadeBlock + threadIdx.x];  // thread t alone reads and writes packed[t] here
    return true;
}

// refrence_mode.slang:28-57 for one bounce of every live path
// GLDS: the flattened-geometry table (80-byte entries, at most kShadeGeomsLds of them) is staged in LDS, so that a hit's material and
// normal matrix cost an LDS read behind the shading record instead of a second dependent global gather
// EMIT: next-event estimation to emissive triangles with MIS; launched only with RT3_F_NEE_EMISSIVE and a non-empty table
// MAT: material textures (hit_finish<true>); launched only when the built scene has the side table (sc.mat_tex), and
// never for the first vertex, which comes from the G-buffer.  With GLDS the 16-byte side table sits in LDS beside the geometry table, so
// only the tangent word -- fetched by primitive, beside the shading record -- and the texels themselves are global gathers.
// Waves per SIMD: 6 (80 VGPRs, 32 bytes of scratch) without MAT: the kernel lives off memory-level parallelism -- 28.8 -> 27.7 ms against
// the compiler's own choice of 93 VGPRs (4 waves with 512-thread blocks).  MAT holds up to twelve more texels and three footprints' weights
// across the light sample: the compiler's own allocation is 94 VGPRs (116 with EMIT), above the 80 that 6 waves leave, and a 512-thread
// block is 2 waves per SIMD, so the next step down from 6 is 4 = 128 VGPRs, which holds both without scratch.
// PUNCT (on the EMIT instances): the table in use also holds punctual lights (RT3_F_NEE_PUNCTUAL); a record's tag
// says which kind the draw of dim 5 picked.  Launched only when the table holds a punctual record, so every other instance keeps its code.
constexpr int shade_waves(bool mat) { return mat ? 4 : 6; }
// The body is rt3_shade_body.inc, included once per kernel template: the PUNCT twins are kernels of their own name, and the instances of
// k_shade keep both their names and, being compiled from the same text with PUNCT = false, their instructions.
template <bool FIRST, bool GLDS, bool EMIT = false, bool MAT = false>
__global__ __launch_bounds__(kShadeBlock) __attribute__((amdgpu_waves_per_eu(shade_waves(MAT), shade_waves(MAT)))) void k_shade(ShadeLaunch a) {
    constexpr bool PUNCT = false, GLASS = false, DEFER = false, LIGHT = false;
    constexpr bool PANE = false, EXIT = false, FROST = false;
    float* const pane_dist = nullptr;
    const ShadeExit x = {};
#include "rt3_shade_body.inc"
}
// Waves: at six (80 VGPRs) the light function costs the FIRST and GLDS twins more scratch than their EMIT instance has (108 against 96 bytes,
// 124 against 120), so all five take the four-wave step that MAT took: 128 VGPRs, no scratch.
template <bool FIRST, bool GLDS, bool MAT>
__global__ __launch_bounds__(kShadeBlock) __attribute__((amdgpu_waves_per_eu(shade_waves(true), shade_waves(true)))) void k_shade_punct(ShadeLaunch a) {
    constexpr bool EMIT = true, PUNCT = true, GLASS = false, DEFER = false, LIGHT = false;
    constexpr bool PANE = false, EXIT = false, FROST = false;
    float* const pane_dist = nullptr;
    const ShadeExit x = {};
#include "rt3_shade_body.inc"
}
// GLASS: the built scene has the transmission side table (a.glass); a vertex on a geometry with transmission > 0 is,
// with that probability, a smooth dielectric (rt3_glass.hpp) instead of the opaque surface.  Launched only for such scenes, which always
// start from per-sample camera rays (FIRST = false).  Kernels of their own name, like the PUNCT twins, so that every other instance keeps
// its name and its instructions.  Waves: the four-wave step of MAT and PUNCT (128 VGPRs); the table of registers and scratch per instance
// is in DESIGN.md section 4n.
template <bool GLDS, bool EMIT, bool MAT, bool PUNCT>
__global__ __launch_bounds__(kShadeBlock) __attribute__((amdgpu_waves_per_eu(shade_waves(true), shade_waves(true)))) void k_shade_glass(ShadeLaunch a) {
    constexpr bool FIRST = false, GLASS = true, DEFER = false, LIGHT = false;
    constexpr bool PANE = false, EXIT = false, FROST = false;
    float* const pane_dist = nullptr;
    const ShadeExit x = {};
#include "rt3_shade_body.inc"
}
// PANE: k_shade_glass for a built scene with panes under rt3_scene_set_pane_shadows.  A glass vertex on a pane that
// transmits hands the incoming pdf slot on instead of a delta marker, because the light samples of the vertex before it now cross the pane
// (k_shadow_pane) and the two must share one pair of MIS weights; pane_dist[path] carries the distance walked along the direction since the
// vertex that sampled it, which an emitter hit needs for that vertex's solid-angle density.  A kernel of its own name and argument list,
// so that every other instance keeps its name and its instructions.  Registers and scratch per instance: DESIGN.md section 4q.
template <bool GLDS, bool EMIT, bool MAT, bool PUNCT>
__global__ __launch_bounds__(kShadeBlock) __attribute__((amdgpu_waves_per_eu(shade_waves(true), shade_waves(true)))) void k_shade_pane(ShadeLaunch a, float* pane_dist) {
    constexpr bool FIRST = false, GLASS = true, DEFER = false, LIGHT = false, PANE = true, EXIT = false, FROST = false;
    const ShadeExit x = {};
#include "rt3_shade_body.inc"
}
// FROST: k_shade_glass / k_shade_pane for a built scene with a frosted geometry under rt3_scene_set_rough_transmission.  A
// glass vertex on such a geometry whose roughness is > 0 takes its event at a GGX micro-normal (frost_sample); every other vertex does what
// it does in the PANE twin.  A kernel of its own name, so that every other instance keeps its name and its instructions.  Twelve
// instances: {no light table, EMIT, EMIT + PUNCT} x MAT x PANE; the geometry tables are read from global memory (no GLDS twin: staging is an
// optimisation for small scenes, and doubling the build's largest kernels for it waits for a measurement).  pane_dist is null without PANE.
// Registers and scratch per instance: DESIGN.md section 4t.
template <bool EMIT, bool MAT, bool PUNCT, bool PANE>
__global__ __launch_bounds__(kShadeBlock) __attribute__((amdgpu_waves_per_eu(shade_waves(true), shade_waves(true)))) void k_shade_frost(ShadeLaunch a, float* pane_dist) {
    constexpr bool FIRST = false, GLDS = false, GLASS = true, DEFER = false, LIGHT = false, EXIT = false, FROST = true;
    const ShadeExit x = {};
#include "rt3_shade_body.inc"
}
// DEFER: k_shade<FIRST, GLDS, EMIT> with the sky light sample cut off behind its direction.  Four of five sky shadow
// rays are occluded, and for those the radiance texels, the BSDF towards the light and the weight were thrown away; this kernel sends the
// ray with the vertex's queue index instead, and k_light finishes the samples whose ray came through.  A kernel of its own name, so that
// k_shade's instances keep their names and instructions.  Launched only for scenes without material textures, punctual lights and glass.
template <bool FIRST, bool GLDS, bool EMIT>
__global__ __launch_bounds__(kShadeBlock) __attribute__((amdgpu_waves_per_eu(shade_waves(false), shade_waves(false)))) void k_shade_defer(ShadeLaunch a) {
    constexpr bool MAT = false, PUNCT = false, GLASS = false, DEFER = true, LIGHT = false;
    constexpr bool PANE = false, EXIT = false, FROST = false;
    float* const pane_dist = nullptr;
    const ShadeExit x = {};
#include "rt3_shade_body.inc"
}
// EXIT: k_shade_defer<FIRST, GLDS, false> for a structure with an exit table.  Three of four sky shadow rays are
// occluded by the leaf their exit cell names, which k_shadow_exit found out in the ray's first two steps -- after the ray had been written,
// read back, prepared at a refill and its occlusion word written and scanned.  Origin and direction are in this kernel's registers: it
// makes that test itself and queues only the rays the table cannot decide, which the plain k_shadow then walks from the root.  A kernel of
// its own name, so that every other instance keeps its name and its instructions.  Launched only without an emitter queue, alpha masks,
// panes and counting (trace_batch).
template <bool FIRST, bool GLDS>
__global__ __launch_bounds__(kShadeBlock) __attribute__((amdgpu_waves_per_eu(shade_waves(false), shade_waves(false)))) void k_shade_defer_exit(ShadeLaunch a, ShadeExit x) {
    constexpr bool EMIT = false, MAT = false, PUNCT = false, GLASS = false, DEFER = true, LIGHT = false;
    constexpr bool PANE = false, EXIT = true, FROST = false;
    float* const pane_dist = nullptr;
#include "rt3_shade_body.inc"
}
// The second half of k_shade_defer's light samples, for the rays k_shadow reported as unoccluded: a.sh_count slots in a.sh_contrib (light_next),
// the vertices behind them in the queues the k_shade_defer launch read, which nothing has overwritten yet.  The emitter table plays no part
// (the emitter sample is k_shade_defer's), so one instance serves both of its EMIT twins.
template <bool FIRST, bool GLDS>
__global__ __launch_bounds__(kShadeBlock) __attribute__((amdgpu_waves_per_eu(shade_waves(false), shade_waves(false)))) void k_light(ShadeLaunch a) {
    constexpr bool EMIT = false, MAT = false, PUNCT = false, GLASS = false, DEFER = false, LIGHT = true;
    constexpr bool PANE = false, EXIT = false, FROST = false;
    float* const pane_dist = nullptr;
    const ShadeExit x = {};
#include "rt3_shade_body.inc"
}
// self-test op 32: {ior, thin_walled, d xyz, n xyz, u} -> {event (0 reflect / 1 transmit), direction xyz, F}
__global__ void k_selftest_glass(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* p = in + kSelftestGlassIn * (size_t)i;
    auto F = [](uint32_t u) { return __uint_as_float(u); };
    const GlassEvent e = glass_sample(F(p[0]), p[1] != 0u, v3(F(p[2]), F(p[3]), F(p[4])), v3(F(p[5]), F(p[6]), F(p[7])), F(p[8]));
    uint32_t* o = out + kSelftestGlassOut * (size_t)i;
    o[0] = e.transmit;
    o[1] = __float_as_uint(e.dir.x); o[2] = __float_as_uint(e.dir.y); o[3] = __float_as_uint(e.dir.z);
    o[4] = __float_as_uint(e.F);
}
// self-test op 38: {ior, thin_walled, d xyz, n xyz, alpha, u_event, u2, u3} -> {event (0 reflect / 1 transmit / 2 invalid), direction xyz, F,
// weight}: the vertex rule of a frosted geometry as the kernels apply it -- frost_sample at alpha > 0, glass_sample (weight 1) at alpha = 0
__global__ void k_selftest_frost(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* p = in + kSelftestFrostIn * (size_t)i;
    auto F = [](uint32_t u) { return __uint_as_float(u); };
    const V3 d = v3(F(p[2]), F(p[3]), F(p[4])), nn = v3(F(p[5]), F(p[6]), F(p[7]));
    FrostEvent e;
    if (F(p[8]) > 0.0f) {
        e = frost_sample(F(p[0]), p[1] != 0u, d, nn, F(p[8]), F(p[9]), F(p[10]), F(p[11]));
    } else {
        const GlassEvent g = glass_sample(F(p[0]), p[1] != 0u, d, nn, F(p[9]));
        e.event = g.transmit;
        e.dir = g.dir;
        e.F = g.F;
        e.weight = 1.0f;
    }
    uint32_t* o = out + kSelftestFrostOut * (size_t)i;
    o[0] = e.event;
    o[1] = __float_as_uint(e.dir.x); o[2] = __float_as_uint(e.dir.y); o[3] = __float_as_uint(e.dir.z);
    o[4] = __float_as_uint(e.F);
    o[5] = __float_as_uint(e.weight);
}

// refrence_mode.slang:59-65 : radiance = (sum over samples, in sample order) / S, then blend with PrevLight
__global__ void k_accumulate(GConstDev g, const uint32_t* __restrict__ pixels, uint32_t npix, uint32_t width,
                             const float* __restrict__ depth, const float* __restrict__ lacc, size_t stride, uint32_t sb,
                             int first_batch, int last_batch, float* __restrict__ radsum, float4* __restrict__ light,
                             const float4* __restrict__ prev) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        uint32_t xy = pixels[i];
        size_t pi = (size_t)(xy >> 16) * width + (xy & 0xFFFFu);
        if (depth[pi] == kBackgroundDepth) continue;
        float r = first_batch ? 0.0f : radsum[i], gg = first_batch ? 0.0f : radsum[npix + i], bb = first_batch ? 0.0f : radsum[2 * (size_t)npix + i];
        for (uint32_t s = 0; s < sb; s++) {
            size_t p = (size_t)s * npix + i;
            const float4 lv = reinterpret_cast<const float4*>(lacc)[p];
            r += lv.x;
            gg += lv.y;
            bb += lv.z;
        }
        if (!last_batch) {
            radsum[i] = r;
            radsum[npix + i] = gg;
            radsum[2 * (size_t)npix + i] = bb;
        } else {
            float fs = (float)g.samples;
            r = r / fs;
            gg = gg / fs;
            bb = bb / fs;
            if (g.blendfactor >= 1.0f) {
                light[pi] = make_float4(r, gg, bb, 0.0f);
            } else {
                float4 pv = prev[pi];
                float bf = g.blendfactor;
                light[pi] = make_float4(pv.x + (r - pv.x) * bf, pv.y + (gg - pv.y) * bf, pv.z + (bb - pv.z) * bf, 0.0f);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ launchers
// The k_shade instance of (first, glds, emit, mat): `launch` is called with four std::integral_constant<bool, ..>, in that order.  The first
// vertex comes from the G-buffer and has neither the LDS table nor material textures, so ten instances of k_shade exist: FIRST x EMIT, and
// GLDS x EMIT x MAT for the later vertices; and five of k_shade_punct, one beside each EMIT instance.
// With punctual lights in the table (punct, which implies emit) the five EMIT shapes have a PUNCT twin: FIRST, and GLDS x MAT.
template <typename Launch>
static void dispatch_shade(bool first, bool glds, bool emit, bool mat, bool punct, Launch launch) {
    auto by_emit = [&](auto f, auto g, auto m) {
        if (emit && punct) launch(f, g, std::true_type{}, m, std::true_type{});
        else if (emit) launch(f, g, std::true_type{}, m, std::false_type{});
        else launch(f, g, std::false_type{}, m, std::false_type{});
    };
    auto by_mat = [&](auto g) {
        if (mat) by_emit(std::false_type{}, g, std::true_type{});
        else by_emit(std::false_type{}, g, std::false_type{});
    };
    if (first) by_emit(std::true_type{}, std::false_type{}, std::false_type{});
    else if (glds) by_mat(std::true_type{});
    else by_mat(std::false_type{});
}
// defer: the k_shade_defer instance (the caller has checked that the scene is inside its cover: shade_defer_covers)
// pane_dist: the built scene has panes and pane shadows are on (with `glass`): k_shade_pane, twelve instances shaped like k_shade_glass's
// exit (with defer and an empty emitter table): k_shade_defer_exit
// frost (with glass): the built scene has a frosted geometry: k_shade_frost, twelve instances {no table, EMIT, EMIT + PUNCT} x MAT x PANE
void launch_shade(hipStream_t st, bool first, ShadeLaunch a, bool punct, const GlassDev* glass, bool defer, float* pane_dist, const ShadeExit* exit, bool frost) {
    a.npix_div = make_fastdiv(a.npix);
    const unsigned grid = grid_for(a.n_first, kShadeBlock, 8192);
    const bool glds = a.sc.shade_geoms != nullptr && a.sc.n_geoms <= kShadeGeomsLds;
    if (defer && exit != nullptr && a.lights.n == 0u) {
        dispatch_shade(first, glds, false, false, false, [&](auto f, auto g, auto, auto, auto) {
            hipLaunchKernelGGL((k_shade_defer_exit<decltype(f)::value, decltype(g)::value>), dim3(grid), dim3(kShadeBlock), 0, st, a, *exit);
        });
        return;
    }
    if (defer) {
        dispatch_shade(first, glds, a.lights.n != 0u, false, false, [&](auto f, auto g, auto e, auto, auto) {
            hipLaunchKernelGGL((k_shade_defer<decltype(f)::value, decltype(g)::value, decltype(e)::value>), dim3(grid), dim3(kShadeBlock), 0, st, a);
        });
        return;
    }
    // emit: RT3_F_NEE_EMISSIVE with something to sample; mat: the built scene has material textures
    // punct: that table holds punctual lights (RT3_F_NEE_PUNCTUAL)
    // glass: the built scene has the transmission table; twelve instances of k_shade_glass, GLDS x MAT x {no table, EMIT, EMIT + PUNCT}
    dispatch_shade(first, glds, a.lights.n != 0u, a.sc.mat_tex != nullptr, punct && a.lights.n != 0u, [&](auto f, auto g, auto e, auto m, auto p) {
        if constexpr (!decltype(f)::value) {
            if (glass != nullptr) {
                a.glass = glass;  // (in the slot of the G-buffer, which these kernels do not read)
                if (frost) {
                    if (pane_dist != nullptr) hipLaunchKernelGGL((k_shade_frost<decltype(e)::value, decltype(m)::value, decltype(p)::value, true>), dim3(grid), dim3(kShadeBlock), 0, st, a, pane_dist);
                    else hipLaunchKernelGGL((k_shade_frost<decltype(e)::value, decltype(m)::value, decltype(p)::value, false>), dim3(grid), dim3(kShadeBlock), 0, st, a, pane_dist);
                    return;
                }
                if (pane_dist != nullptr) {
                    hipLaunchKernelGGL((k_shade_pane<decltype(g)::value, decltype(e)::value, decltype(m)::value, decltype(p)::value>), dim3(grid), dim3(kShadeBlock), 0, st, a, pane_dist);
                    return;
                }
                hipLaunchKernelGGL((k_shade_glass<decltype(g)::value, decltype(e)::value, decltype(m)::value, decltype(p)::value>), dim3(grid), dim3(kShadeBlock), 0, st, a);
                return;
            }
        }
        if constexpr (decltype(p)::value) hipLaunchKernelGGL((k_shade_punct<decltype(f)::value, decltype(g)::value, decltype(m)::value>), dim3(grid), dim3(kShadeBlock), 0, st, a);
        else hipLaunchKernelGGL((k_shade<decltype(f)::value, decltype(g)::value, decltype(e)::value, decltype(m)::value>), dim3(grid), dim3(kShadeBlock), 0, st, a);
    });
}
// k_light over the shadow queue of the k_shade_defer launch of the same arguments.  A workgroup takes several trips, so that the few
// unoccluded slots of each add up to whole workgroups of vertices.
void launch_light(hipStream_t st, bool first, ShadeLaunch a) {
    a.npix_div = make_fastdiv(a.npix);
    const unsigned grid = grid_for(a.n_first, kShadeBlock * 8, 8192);
    const bool glds = a.sc.shade_geoms != nullptr && a.sc.n_geoms <= kShadeGeomsLds;
    dispatch_shade(first, glds, false, false, false, [&](auto f, auto g, auto, auto, auto) {
        hipLaunchKernelGGL((k_light<decltype(f)::value, decltype(g)::value>), dim3(grid), dim3(kShadeBlock), 0, st, a);
    });
}
void launch_selftest_glass(hipStream_t st, const uint32_t* in, uint32_t n, uint32_t* out) {
    hipLaunchKernelGGL(k_selftest_glass, dim3((n + 255) / 256), dim3(256), 0, st, in, n, out);
}
void launch_selftest_frost(hipStream_t st, const uint32_t* in, uint32_t n, uint32_t* out) {
    hipLaunchKernelGGL(k_selftest_frost, dim3((n + 255) / 256), dim3(256), 0, st, in, n, out);
}
void launch_accumulate(hipStream_t st, const GConstDev& g, const uint32_t* pixels, uint32_t npix, uint32_t width, const float* depth,
                       const float* lacc, size_t stride, uint32_t sb, int first_batch, int last_batch, float* radsum, void* light,
                       const void* prev) {
    hipLaunchKernelGGL(k_accumulate, dim3(grid_for(npix, 256, 8192)), dim3(256), 0, st, g, pixels, npix, width, depth, lacc, stride, sb,
                       first_batch, last_batch, radsum, (float4*)light, (const float4*)prev);
}

}  // namespace rt3
