// rt3_trace.hip -- the persistent-wave BVH traversal (trace_stream) and its two kernels: k_extend (closest hit) and k_shadow (any hit).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rt3_hit.hpp"
#include "rt3_internal.hpp"
#include "rt3_leaf_test.hpp"
#include "rt3_math.hpp"
#include "rt3_surface.hpp"

namespace rt3 {

// ------------------------------------------------------------------------------------------------ traversal
// One ray per lane.  Short stack: kLdsStack entries per lane in LDS ([entry][lane] so a wave's ds_read_b32 /
// ds_write_b32 hit 64 consecutive dwords: conflict-free), deeper entries spill to a private array (scratch).
// LDS per 256-thread block: 12 KiB of stack + 8 KiB of cached top-of-tree nodes = 20 KiB -> 8 blocks = 8 waves per SIMD in 160 KiB.
// Stack: a diffuse ray's stack is 4 entries deep at the median, 6 at the 90th and 9 at the 99th percentile (13 at most on the atrium).
constexpr int kLdsStack = 12;
// Top-of-tree cache (quantised four-wide layout): the first kTopNodes nodes of the tree in breadth-first order live in LDS, copied at
// kernel start from a 8 KiB array the builder prepares (k_top_cache).  They receive 46 % of all node visits (the root alone 5 %), and the
// walk is bound by the rate at which the vector-memory path returns gathered bytes (profiles/r02_gather_cap.md): these visits now go
// through the LDS instead.  In the cached copies a reference to a child that is itself cached is kTopFlag | slot.
constexpr uint32_t kTopFlag = 0x40000000u;
constexpr int kSpill = 64 - kLdsStack;  // kLdsStack + kSpill >= kMaxBvhDepth (checked on the host after the build)
constexpr uint32_t kMaxSteps = 1u << 20;  // safety bound on traversal steps per ray (a corrupt tree must not hang the GPU)

// two-level walk: the boxes of the top tree are widened by kTopPadRel max|o| (the rounding of the slab test itself, which grows with the
// distance of the origin; the instance boxes carry the rest of the bound)
constexpr float kTopPadRel = 2.44140625e-4f;  // 2^-12

struct Cand {  // a child slot that the ray enters: entry distance + reference
    float tn;
    uint32_t ref;
};
// compare-exchange on the entry distance alone (strict <).  Equal distances are ordered by the fixed 5-comparator
// network itself; the oracle runs the identical network, so the visiting order is the same on both sides.
__device__ __forceinline__ void cswap(Cand& a, Cand& b) {
    bool sw = b.tn < a.tn;
    float ta = a.tn;
    uint32_t ra = a.ref;
    a.tn = sw ? b.tn : a.tn;
    a.ref = sw ? b.ref : a.ref;
    b.tn = sw ? ta : b.tn;
    b.ref = sw ? ra : b.ref;
}
__device__ __forceinline__ void pin(float4& q) { asm volatile("" : "+v"(q.x), "+v"(q.y), "+v"(q.z), "+v"(q.w)); }
// (the watertight triangle test tri_test_nb and its pane helpers: rt3_leaf_test.hpp)

// Persistent-wave traversal.  The waves of a launch share one pool of rays (chunks of g_pool_chunk, handed out by an atomic
// cursor).  One ray per lane; a lane that finishes its ray takes the next one from the wave's current chunk (refill once
// >= g_refill_lanes lanes are idle), so the wave keeps its 64 lanes busy instead of idling until its slowest ray is done: a
// plain one-ray-per-lane loop spent ~49 iterations per 64 rays whose mean length is ~23 steps.
//
// Layouts: kLayoutBinary64 (two fp32 boxes), kLayoutWide128 (four fp32 boxes), kLayoutWide64Q (four 8-bit boxes, default),
// kLayoutWide48Q (the same boxes, implied references).
// Closest hit: children are visited nearest first, the others are pushed so that they pop in ascending entry distance
// (order fixed by a 5-comparator network); any hit: farthest first (same network on the negated distance).  No re-cull on pop.  A leaf reference holds 1..8 consecutive triangles.
// Every step makes exactly ONE memory round trip: a lane first fetches its next item -- the node, or the next
// triangle(s) of its current leaf -- with one batch of 16-byte loads issued together, then branches into box or
// triangle tests (both branch-free).
__constant__ uint32_t g_pool_chunk = 256;   // rays per pool grab (RT3_OPT_POOL_CHUNK)
__constant__ uint32_t g_refill_lanes = 12;  // tuning knob (RT3_OPT_EXTEND_VARIANT)
// rays per pool grab of a launch over n rays by n_waves waves (trace_stream; k_shadow_exit derives its sampled count from the same number)
__device__ __forceinline__ uint32_t pool_chunk_for(uint32_t n, uint32_t n_waves) {
    return (n < 2u * n_waves * g_pool_chunk && g_pool_chunk >= 128u) ? ((g_pool_chunk >> 1) & ~63u) : g_pool_chunk;
}
void set_refill_lanes(uint32_t v) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_refill_lanes), &v, 4); }
void set_pool_chunk(uint32_t v) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_pool_chunk), &v, 4); }
static unsigned g_trace_max_blocks = kExtendMaxBlocks;  // persistent traversal workgroups per launch (RT3_OPT_TRACE_BLOCKS)
void set_trace_blocks(uint32_t v) { g_trace_max_blocks = v; }

constexpr uint32_t kTopNodes = kTopCacheNodes;  // 8 KiB; ONE constant (rt3_internal.hpp) sizes the builder's array and the LDS copies
// copies the builder's top-of-tree array into LDS (kernel-uniform: either every thread of every block does, or none)
__device__ __forceinline__ bool load_top(float4* s_top, const float4* __restrict__ top, uint32_t n_top) {
    if (top == nullptr || n_top == 0u) return false;
    n_top = n_top < kTopNodes ? n_top : kTopNodes;  // never past the LDS array, whatever the host read back
    for (uint32_t i = threadIdx.x; i < 4u * n_top; i += kExtendBlock) s_top[i] = top[i];
    __syncthreads();
    return true;
}

// slab test of a quantised child whose plane bytes arrive near-first: p = {near.x, near.y, near.z, far.x}, q = {far.y, far.z, -, -}
// (v_perm_b32 by the ray's sign selectors).  The same maxima / minima as slab_test_q, minus the six that ordered each axis' pair.
__device__ __forceinline__ bool slab_test_sorted(uint32_t p, uint32_t q, V3 A, V3 B, float tmin, float tbest, float& tn_out) {
    const float nx = __builtin_fmaf((float)(p & 0xFFu), A.x, B.x), ny = __builtin_fmaf((float)((p >> 8) & 0xFFu), A.y, B.y),
                nz = __builtin_fmaf((float)((p >> 16) & 0xFFu), A.z, B.z), fx = __builtin_fmaf((float)(p >> 24), A.x, B.x),
                fy = __builtin_fmaf((float)(q & 0xFFu), A.y, B.y), fz = __builtin_fmaf((float)((q >> 8) & 0xFFu), A.z, B.z);
    const float tn = __builtin_fmaxf(__builtin_fmaxf(nx, ny), __builtin_fmaxf(nz, tmin));
    const float tf = __builtin_fminf(__builtin_fminf(fx, fy), __builtin_fminf(fz, tbest));
    tn_out = tn;
    return tn <= tf;
}

// the same test on a box widened by pad.{x,y,z} (= P |inv|: a box grown by P on every side) -- the two-level walk's conservative boxes
__device__ __forceinline__ bool slab_test_sorted_pad(uint32_t p, uint32_t q, V3 A, V3 B, V3 pad, float tmin, float tbest, float& tn_out) {
    const float nx = __builtin_fmaf((float)(p & 0xFFu), A.x, B.x) - pad.x, ny = __builtin_fmaf((float)((p >> 8) & 0xFFu), A.y, B.y) - pad.y,
                nz = __builtin_fmaf((float)((p >> 16) & 0xFFu), A.z, B.z) - pad.z, fx = __builtin_fmaf((float)(p >> 24), A.x, B.x) + pad.x,
                fy = __builtin_fmaf((float)(q & 0xFFu), A.y, B.y) + pad.y, fz = __builtin_fmaf((float)((q >> 8) & 0xFFu), A.z, B.z) + pad.z;
    const float tn = __builtin_fmaxf(__builtin_fmaxf(nx, ny), __builtin_fmaxf(nz, tmin));
    const float tf = __builtin_fminf(__builtin_fminf(fx, fy), __builtin_fminf(fz, tbest));
    tn_out = tn;
    return tn <= tf;
}

// Exit table (any hit, default layout, single level: EXIT; DESIGN.md sections 5 and 7).  A lane's first item is not the root but the table
// entry of the cell where its ray leaves the root box: r.cur = kExitFlag | cell (never a leaf reference, never a node index: the arena
// holds fewer than 2^26 nodes; bit 30, kTopFlag, stays clear so the item is fetched from memory).  The step's own batch fetches the 16-byte
// group of the entry; the entry, a leaf reference, becomes r.cur with the root pushed, and the ordinary leaf steps test it.  Occlusion
// does not depend on WHICH occluder is found, so the table's contents decide the speed only.
constexpr uint32_t kExitFlag = 0x20000000u;
struct ExitWalk {  // per wave, all wave-uniform: where the table is, the launch's decision and what the wave counted
    uint32_t off = 0;       // byte offset of the table's header in the arena (ExitHeader, then the entries)
    uint32_t mode = 0;      // 1: every 32nd chunk starts at the table, so that the rate stays known; 2: every chunk does
    uint32_t occluded = 0;  // rays an entry's leaf occluded
};
// rays of a queue of n that start at the table when only every 32nd chunk of `chunk` rays does
__device__ __forceinline__ unsigned long long exit_sampled_rays(uint32_t n, uint32_t chunk) {
    if (n == 0u) return 0ull;
    const uint32_t n_chunks = (n - 1u) / chunk + 1u, m = (n_chunks + 31u) / 32u;  // m >= 1 sampled chunks: 0, 32, ...
    const unsigned long long last_first = 32ull * (m - 1u) * chunk, rest = n - last_first;
    return (unsigned long long)(m - 1u) * chunk + (rest < chunk ? rest : chunk);
}

struct LaneRay {  // traversal state of the ray a lane currently owns
    V3 o, d, inv;
    float tmin, inv_dd;  // inv_dd = 1 / d.d (the triangle test makes no unit-length assumption)
    Hit best;
    uint32_t cur, leaf_k, index, steps, cn, ct, cl;  // cn / ct / cl: node visits, triangle tests, node visits served by the LDS copy (COUNT)
    int sp;
    float pay0, pay1;  // shadow rays of the path tracer's own queue: two words of payload ride in the .w of the two ray records,
    float pay2, pay3;  // two more ({blue, path id}) in an 8-byte record fetched WITH the ray: at the end of the walk nothing is left to wait for
    uint32_t sel_p0, sel_q0, sel_p1, sel_q1;  // default layout: v_perm_b32 selectors that put a child's NEAR planes first (see the box block)
};

// MODE 0: closest hit over one queue; 1: any hit over one queue.
// TWO: the two-level structure (kLayoutTwoLevel) over the quantised 64-byte node format: node 0 is the root of the top
// tree, whose leaf references name instance records (0x80000000 | record node, count field 0: in the top tree every leaf is an instance).  A
// lane that reaches one fetches the record, moves its ray into object space for the box tests of the bottom tree, marks its stack and walks
// that tree; its triangles are transformed to world space with flattening's own expression and tested against the world ray.  Once the
// bottom walk has popped down to the mark the lane goes back to the world ray and the top tree's entries.
// RANGE (any hit only): ray i ends at any_tmax[i] instead of kBackgroundDepth -- the emitter shadow queue of RT3_F_NEE_EMISSIVE.
// MASK: the structure holds alpha-masked triangles: a candidate that would be accepted (inside, t in range, better than
// best) is alpha-tested inline in its leaf step -- the extra gathers (table, 3 uvs, texture entry, 4 texels) stay out of every other step.
// best is only updated, and an any-hit lane only finishes, on an intersection that counts.
// PANE (any hit, MASK instances): pane triangles attenuate the lane's payload instead of occluding it (tri_test_nb).  Like
// the alpha test, the gathers of an attenuation (shading record, geometry and glass entries, texels) stay inside the leaf step that meets one.
template <int MODE, bool COUNT, int LAYOUT, bool TWO = false, bool RANGE = false, bool MASK = false, bool EXIT = false, bool PANE = false, typename Finish>
__device__ __forceinline__ void trace_stream(const float4* __restrict__ nodes, uint32_t tri_off,
                                             const float* __restrict__ rays, size_t stride, uint32_t n, uint32_t* __restrict__ work_counter,
                                             uint32_t* __restrict__ lds, Finish finish, bool any_payload = false, bool ext_payload = false, const float4* top_lds = nullptr, bool use_top = false,
                                             const float2* __restrict__ any_contrib = nullptr, const float* __restrict__ any_tmax = nullptr,
                                             const AlphaDev& alpha = AlphaDev{}, ExitWalk* xw = nullptr, const PaneDev* pane = nullptr) {
    static_assert(!PANE || (MODE == 1 && MASK && !EXIT && LAYOUT == kLayoutWide64Q), "panes: the any-hit walk of the default node layout, never from the exit table");
    static_assert(!EXIT || (MODE == 1 && !COUNT && !TWO && !RANGE && LAYOUT == kLayoutWide64Q), "the exit table serves the plain any-hit walk only");
    // any_payload: the any-hit rays come from k_shade's shadow queue, where every ray has the range (kRayTMin, kBackgroundDepth):
    // the two .w slots of its record carry payload (two contribution channels) instead of tmin / tmax -- 16 bytes less per ray.
    // ext_payload: likewise for the extension rays of the path tracer's own queue (.w = the path's pdf and id, read by k_shade)
    constexpr bool ANY = MODE == 1;
    constexpr bool WIDE = LAYOUT == kLayoutWide128;   // 8 x 16 B per fetch
    constexpr bool WIDEQ = LAYOUT == kLayoutWide64Q || LAYOUT == kLayoutWide48Q;  // quantised boxes
    constexpr bool C48 = LAYOUT == kLayoutWide48Q;  // 3 x 16 B per fetch: node and triangle records are both 48 B
    // ray pool: waves grab chunks of kPoolChunk consecutive rays from a per-launch counter (one returning atomic per
    // chunk: ~110 k per launch, ~20 / us, below the ~88 / us a single counter word sustains; 64-ray chunks were
    // atomic-bound, 1024 and more left a visible tail), so no wave idles at the end of a
    // launch while another still owns untouched rays
    uint32_t pool_next = 0, pool_end = 0;
    bool queue_empty = false;
    const uint32_t lane = __lane_id();
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
    // a launch whose queue is mostly covered by the waves' static first chunks (a 1-spp frame: 2 M rays over 8192 waves) balances
    // better with chunks of half the size: 0.79 -> 0.72 ms per frame at 1080p, 1 spp, one bounce; long queues keep the full chunk
    const uint32_t kRefillLanes = g_refill_lanes,
                   kPoolChunk = pool_chunk_for(n, n_waves);
    // the first chunk of every wave is static (chunk number = global wave number): no atomic storm at launch, when all the
    // waves of the grid would hit the cursor at once (8192 returning atomics on one word ~ 0.1 ms); the cursor counts the
    // chunks handed out after those
    // (wave-uniform, but only the hardware knows: without the readfirstlane the pool cursors live in vector registers)
    const uint32_t wave_id = blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    bool first_chunk = true;
    bool chunk_exit = false;  // EXIT: the rays of the current chunk start at their table entry
    uint32_t spill[kSpill];
    LaneRay r;
    r.o = r.d = r.inv = v3(0.0f, 0.0f, 0.0f);
    r.tmin = 0.0f;
    r.inv_dd = 1.0f;
    r.best = Hit{0.0f, 0.0f, 0.0f, kMiss};
    r.cur = r.leaf_k = r.index = r.steps = r.cn = r.ct = r.cl = 0u;
    r.sp = 0;
    r.pay0 = r.pay1 = r.pay2 = r.pay3 = 0.0f;
    r.sel_p0 = r.sel_q0 = r.sel_p1 = r.sel_q1 = 0u;
    bool busy = false;
    // two-level state (TWO only): the origin the box tests use (object space in a bottom tree), the slab widening P |inv| of the
    // current level, the stack mark of the instance being walked, its record's node and its primitive base | identity << 31
    V3 tl_o = v3(0.0f, 0.0f, 0.0f), tl_pad = v3(0.0f, 0.0f, 0.0f);
    uint32_t tl_mark = 0u, tl_rec = 0u, tl_base = 0u;
    bool tl_bottom = false;
    // the world level: the ray's own inverses, selectors and widening (ray start, and back from a bottom tree)
    auto tl_world = [&]() {
        r.inv = v3(guarded_inverse(r.d.x), guarded_inverse(r.d.y), guarded_inverse(r.d.z));
        tl_o = r.o;
        const float pw = kTopPadRel * __builtin_fmaxf(__builtin_fmaxf(fabsf(r.o.x), fabsf(r.o.y)), fabsf(r.o.z));
        tl_pad = v3(pw * fabsf(r.inv.x), pw * fabsf(r.inv.y), pw * fabsf(r.inv.z));
        tl_bottom = false;
    };
    auto tl_sels = [&]() {  // as at ray start: v_perm_b32 selectors that put a child's near planes first, for the current r.inv
        const uint32_t sx = r.inv.x < 0.0f ? 1u : 0u, sy = r.inv.y < 0.0f ? 1u : 0u, sz = r.inv.z < 0.0f ? 1u : 0u;
        const uint32_t nx = 3u * sx, ny = 1u + 3u * sy, nz = 2u + 3u * sz, fx = 3u - 3u * sx, fy = 4u - 3u * sy, fz = 5u - 3u * sz;
        r.sel_p0 = nx | (ny << 8) | (nz << 16) | (fx << 24);
        r.sel_q0 = fy | (fz << 8);
        r.sel_p1 = r.sel_p0 + 0x02020202u;
        r.sel_q1 = r.sel_q0 + 0x00000202u;
    };
    for (;;) {
        // ---- refill idle lanes from the pool
        const unsigned long long m_idle = __ballot(!busy);
        if (pool_next >= pool_end && !queue_empty && m_idle != 0ull) {  // grab the next chunk (wave-uniform)
            uint32_t base = 0;
            if (first_chunk) {
                base = wave_id * kPoolChunk;
                first_chunk = false;
            } else {
                if (lane == 0) base = atomicAdd(work_counter, kPoolChunk);
                base = __builtin_amdgcn_readfirstlane(base);
                const unsigned long long b64 = (unsigned long long)n_waves * kPoolChunk + base;  // may exceed 2^32 only past the end
                base = b64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)b64;
            }
            queue_empty = base >= n;
            pool_next = base < n ? base : n;
            pool_end = (n - pool_next) > kPoolChunk ? pool_next + kPoolChunk : n;
            if constexpr (EXIT) chunk_exit = xw->mode == 2u || (xw->mode == 1u && ((base / kPoolChunk) & 31u) == 0u);
        }
        if (m_idle != 0ull && pool_next < pool_end && ((uint32_t)__popcll(m_idle) >= kRefillLanes || m_idle == ~0ull)) {
            const uint32_t idx = pool_next + (uint32_t)__popcll(m_idle & lanes_below);
            if (!busy && idx < pool_end) {
                const float4 ro = reinterpret_cast<const float4*>(rays)[idx], rd = reinterpret_cast<const float4*>(rays)[stride + idx];
                r.o = v3(ro.x, ro.y, ro.z);
                r.d = v3(rd.x, rd.y, rd.z);
                const bool payload = ANY ? any_payload : ext_payload;
                r.tmin = payload ? kRayTMin : ro.w;
                r.best = Hit{payload ? kBackgroundDepth : rd.w, 0.0f, 0.0f, kMiss};
                if (RANGE) r.best.t = any_tmax[idx];
                r.pay0 = ro.w;
                r.pay1 = rd.w;
                if (ANY && any_contrib != nullptr) {
                    const float2 c2 = any_contrib[idx];
                    r.pay2 = c2.x;
                    r.pay3 = c2.y;
                }
                r.inv = v3(guarded_inverse(r.d.x), guarded_inverse(r.d.y), guarded_inverse(r.d.z));
                r.inv_dd = 1.0f / dot_fma(r.d, r.d);
                if (LAYOUT == kLayoutWide64Q) {
                    // A child's six plane bytes are {lo.xyz, hi.xyz} at bytes 0..5 (children 0, 2) or 2..7 (children 1, 3) of a word pair.
                    // Which of lo / hi is the NEAR plane of an axis is the sign of the ray's direction there, the same for every node:
                    // two v_perm_b32 per child pull {near.x, near.y, near.z, far.x} and {far.y, far.z} out, and the six min / max that
                    // ordered each pair are gone.  Same values: fma(q, A, B) is monotone in q, increasing for A >= 0, decreasing below,
                    // and no operand can be NaN (positions are bounded at upload, rays are checked finite, inverses are guarded).
                    const uint32_t sx = r.inv.x < 0.0f ? 1u : 0u, sy = r.inv.y < 0.0f ? 1u : 0u, sz = r.inv.z < 0.0f ? 1u : 0u;
                    const uint32_t nx = 3u * sx, ny = 1u + 3u * sy, nz = 2u + 3u * sz, fx = 3u - 3u * sx, fy = 4u - 3u * sy, fz = 5u - 3u * sz;
                    r.sel_p0 = nx | (ny << 8) | (nz << 16) | (fx << 24);
                    r.sel_q0 = fy | (fz << 8);
                    r.sel_p1 = r.sel_p0 + 0x02020202u;
                    r.sel_q1 = r.sel_q0 + 0x00000202u;
                }
                r.cur = (LAYOUT == kLayoutWide64Q && use_top) ? kTopFlag : 0u;  // the root: slot 0 of the LDS copy, or node 0
                if constexpr (EXIT) {
                    if (chunk_exit) {
                        // the cell where the ray leaves the box (exit_cell, rt3_leaf_test.hpp).
                        // The box and the grid come from the table's header in the arena, read here with scalar loads (the offset is made
                        // opaque so that they stay in this block: held across the walk they cost the kernel a wave of occupancy).
                        uint32_t hoff = xw->off;
                        asm volatile("" : "+s"(hoff));
                        const ExitHeader e = *reinterpret_cast<const ExitHeader*>(reinterpret_cast<const char*>(nodes) + hoff);
                        r.cur = kExitFlag | exit_cell(e, r.o, r.d, r.inv);
                    }
                }
                if (TWO) tl_world();
                r.leaf_k = 0u;
                r.sp = 0;
                r.index = idx;
                r.steps = 0u;
                r.cn = r.ct = r.cl = 0u;
                busy = true;
                // a ray with a non-finite origin or direction (NaN camera, a zero-length shading normal upstream) misses: with NaNs every
                // slab test of the min/max form passes and the ray would walk the whole tree
                const bool finite_ray = fabsf(r.o.x) <= kFloatMax && fabsf(r.o.y) <= kFloatMax && fabsf(r.o.z) <= kFloatMax && fabsf(r.d.x) <= kFloatMax &&
                                        fabsf(r.d.y) <= kFloatMax && fabsf(r.d.z) <= kFloatMax;
                if (nodes == nullptr || !finite_ray) {  // empty scene: everything misses
                    finish(r.index, r.best, 0u, 0u, 0u, r.pay0, r.pay1, r.pay2, r.pay3);
                    busy = false;
                }
            }
            const uint32_t taken = (uint32_t)__popcll(m_idle);
            pool_next = pool_next + taken < pool_end ? pool_next + taken : pool_end;
        }
        if (__ballot(busy) == 0ull && pool_next >= pool_end && queue_empty) break;
        // ---- one traversal step.  (One region under `if (busy)` and a single way back to the loop header: with `continue`s in front of it
        // the compiler copied the eight registers of the walk's state aside at the top of every step and back at its end.)
        bool by_entry = false;  // EXIT: the lane finishes in this step on a hit in its table entry's leaf
        if (busy) {
        const bool is_leaf = (r.cur & 0x80000000u) != 0u;
        const uint32_t first = r.cur & 0x0FFFFFFFu, cnt = ((r.cur >> 28) & 7u) + 1u;
        const bool cached = LAYOUT == kLayoutWide64Q && !is_leaf && (r.cur & kTopFlag) != 0u;  // a top-of-tree node held in LDS
        const bool is_inst = TWO && is_leaf && !tl_bottom;  // a leaf of the top tree: the instance record at node `first`
        const bool is_tri = is_leaf && !is_inst;
        // `nodes` is the base of the structure's ONE arena (node array, then the triangle records at byte tri_off: LbvhResult) and a lane's
        // item sits at a 32-bit byte offset from it, chosen by a select: the loads take the uniform base in scalar registers and the offset
        // in one vector register, with no 64-bit address arithmetic and no divergent region that only computes an address.  The host
        // refuses an arena beyond 4 GiB - 128 (kArenaMaxBytes), so no offset wraps.
        constexpr uint32_t kNodeBytes = 16u * (WIDE ? 8 : (C48 ? kC48Stride : 4));
        uint32_t off_tri = tri_off + 48u * (first + r.leaf_k), off_node = kNodeBytes * (cached ? 0u : (is_inst ? first : r.cur));
        // (both offsets exist before the select: left to itself the compiler turns the select back into two exec regions, one per product)
        asm volatile("" : "+v"(off_tri), "+v"(off_node));
        uint32_t off = is_tri ? off_tri : off_node;
        bool is_exit = false;
        if constexpr (EXIT) {  // a third value for the select: the 16-byte group that holds the lane's table entry
            is_exit = !is_leaf && (r.cur & kExitFlag) != 0u;
            uint32_t off_exit = xw->off + (uint32_t)sizeof(ExitHeader) + ((r.cur & 0x00FFFFFCu) << 2);
            asm volatile("" : "+v"(off_exit));
            off = is_exit ? off_exit : off;
        }
        const float4* p = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(nodes) + off);
        // one batch of loads (the arena ends in 128 B of slack so that over-reading the last leaf is in bounds)
        float4 q0, q1, q2, q3, q4, q5, q6, q7;
        if (TWO && is_tri) {  // the instance's forward matrix (the record's second node), in the same batch as the triangle
            const float4* pm = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(nodes) + 64u * (tl_rec + 1u));
            q4 = pm[0];
            q5 = pm[1];
            q6 = pm[2];
        }
        if (LAYOUT == kLayoutWide64Q && cached) {
            const float4* t = top_lds + 4 * (r.cur & 0xFFFFu);
            q0 = t[0];
            q1 = t[1];
            q2 = t[2];
            q3 = t[3];
        } else {
            q0 = p[0];
            q1 = p[1];
            q2 = p[2];
            q3 = C48 ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : p[3];
        }
        if (WIDE) {
            q4 = p[4];
            q5 = p[5];
            q6 = p[6];
            q7 = p[7];
        }
        if (TWO && is_tri) { pin(q4); pin(q5); pin(q6); }
        // pin the fetched registers: without this LLVM sinks the loads only one branch needs into that branch, which
        // turns one memory round trip per step into two
        pin(q0); pin(q1); pin(q2);
        if (!C48) pin(q3);
        if (WIDE) { pin(q4); pin(q5); pin(q6); pin(q7); }
        bool pop = false, done = false;
        const V3 o = r.o, d = r.d, inv = r.inv;
        const float tmin = r.tmin;
        if (EXIT && is_exit) {
            // table step: the entry becomes the current item with the root left pending (the lane's stack is empty here); an empty
            // entry means the walk starts at the root as it always did
            const uint32_t k = r.cur & 3u;
            const uint32_t e = __float_as_uint(k == 0u ? q0.x : (k == 1u ? q0.y : (k == 2u ? q0.z : q0.w)));
            const uint32_t root = use_top ? kTopFlag : 0u;
            if (e != kEmptySlot) {
                lds[0] = root;
                r.sp = 1;
            }
            r.cur = e != kEmptySlot ? e : root;
        } else if (TWO && is_inst) {
            // hand-over: record = {inverse 3 x 4 (words 0..11, FlatGeomDev order), bottom root, prim base | identity << 31, pad_abs, pad_rel}.
            // The object-space ray (direction not normalised: t keeps its meaning) only steers the bottom tree's box tests.
            if (COUNT) r.cn++;
            const float mi[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
            const V3 oo = transform_point(mi, o), dd = transform_vector(mi, d);
            r.inv = v3(guarded_inverse(dd.x), guarded_inverse(dd.y), guarded_inverse(dd.z));
            tl_sels();
            const float om = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(fabsf(o.x), fabsf(o.y)), __builtin_fmaxf(fabsf(o.z), fabsf(oo.x))),
                                             __builtin_fmaxf(fabsf(oo.y), fabsf(oo.z)));
            const float pb = __builtin_fmaf(q3.w, om, q3.z);  // P = pad_abs + pad_rel max(|o|, |o'|)
            tl_pad = v3(pb * fabsf(r.inv.x), pb * fabsf(r.inv.y), pb * fabsf(r.inv.z));
            tl_o = oo;
            tl_mark = (uint32_t)r.sp;
            tl_rec = first;
            tl_base = __float_as_uint(q3.y);
            tl_bottom = true;
            r.cur = __float_as_uint(q3.x);
        } else if (is_leaf) {
            if (COUNT) r.ct++;
            if (TWO) {
                // world-space triangle: the object-space vertices under the instance's matrix, fetch_triangle's expression (an identity
                // instance keeps the uploaded bits), and the global primitive id -- the flattened build's record, bit for bit
                const float fm[12] = {q4.x, q4.y, q4.z, q4.w, q5.x, q5.y, q5.z, q5.w, q6.x, q6.y, q6.z, q6.w};
                V3 a = v3(q0.x, q0.y, q0.z), b = v3(q0.w, q1.x, q1.y), c = v3(q1.z, q1.w, q2.x);
                if ((tl_base >> 31) == 0u) {
                    a = transform_point(fm, a);
                    b = transform_point(fm, b);
                    c = transform_point(fm, c);
                }
                const uint32_t gp = __float_as_uint(q2.y) + (tl_base & 0x7FFFFFFFu);
                tri_test_nb<MASK, PANE>(make_float4(a.x, a.y, a.z, b.x), make_float4(b.y, b.z, c.x, c.y),
                                        make_float4(c.z, __uint_as_float(gp), MASK ? q2.z : 0.0f, MASK ? q2.w : 0.0f), o, d, r.inv_dd, tmin, r.best, alpha, pane,
                                        &r.pay0, &r.pay1, &r.pay2);
            } else {
                tri_test_nb<MASK, PANE>(q0, q1, q2, o, d, r.inv_dd, tmin, r.best, alpha, pane, &r.pay0, &r.pay1, &r.pay2);
            }
            r.leaf_k++;
            if (WIDE) {  // the 128 B fetch holds a second triangle
                if (r.leaf_k < cnt && !(ANY && r.best.prim != kMiss)) {
                    if (COUNT) r.ct++;
                    tri_test_nb(q3, q4, q5, o, d, r.inv_dd, tmin, r.best);
                    r.leaf_k++;
                }
            }
            if (ANY && r.best.prim != kMiss) done = true;
            if (r.leaf_k >= cnt) {
                r.leaf_k = 0;
                pop = true;
            }
        } else {
            if (COUNT) {
                r.cn++;
                r.cl += cached ? 1u : 0u;
            }
            if (WIDE || WIDEQ) {
                const float kInf = __builtin_huge_valf();
                float t0, t1, t2, t3;
                uint32_t r0, r1, r2, r3;
                bool h0, h1, h2, h3;
                if (WIDEQ) {
                    // the dequantisation is folded into the ray: a child plane sits at org + q * 2^(e-127), so its ray parameter is
                    // q * (step * inv) + (org - o) * inv = fma(q, A, B): one v_cvt_f32_ubyte + one v_fma_f32 per plane.
                    // Bytes 6k..6k+5 of words 4..9 hold child k {lo.xyz, hi.xyz}.
                    const uint32_t ex = __float_as_uint(q0.w);
                    // (the 64-byte node holds its steps as floats -- word 3, words 14 / 15; the 48-byte one as three exponent bytes)
                    const V3 A = C48 ? v3(__uint_as_float((ex & 0xFFu) << 23) * inv.x, __uint_as_float(((ex >> 8) & 0xFFu) << 23) * inv.y,
                                          __uint_as_float(((ex >> 16) & 0xFFu) << 23) * inv.z)
                                     : v3(q0.w * inv.x, q3.z * inv.y, q3.w * inv.z);
                    const V3 ob = TWO ? tl_o : o;  // two-level: the object-space origin inside a bottom tree
                    const V3 B = v3((q0.x - ob.x) * inv.x, (q0.y - ob.y) * inv.y, (q0.z - ob.z) * inv.z);
                    const uint32_t w0 = __float_as_uint(q1.x), w1 = __float_as_uint(q1.y), w2 = __float_as_uint(q1.z), w3 = __float_as_uint(q1.w),
                                   w4 = __float_as_uint(q2.x), w5 = __float_as_uint(q2.y);
                    if (C48) {
                        // implied references: internal children count up from node_base, leaf triangles from tri_base
                        const uint32_t wa = __float_as_uint(q2.z), wb = __float_as_uint(q2.w);
                        const uint32_t m0 = (ex >> 24) & 15u, m1 = ex >> 28, m2 = wa >> 28, m3 = wb >> 28;
                        uint32_t nb = wa & 0x0FFFFFFFu, tb = wb & 0x0FFFFFFFu;
#define RT3_REF48(m, out)                                                         \
    {                                                                             \
        const bool in_ = (m) == 0u, lf_ = ((m)&8u) != 0u;                         \
        out = in_ ? nb : (lf_ ? (0x80000000u | (((m)&7u) << 28) | tb) : kEmptySlot); \
        nb += in_ ? 1u : 0u;                                                      \
        tb += lf_ ? ((m)&7u) + 1u : 0u;                                           \
    }
                        RT3_REF48(m0, r0)
                        RT3_REF48(m1, r1)
                        RT3_REF48(m2, r2)
                        RT3_REF48(m3, r3)
#undef RT3_REF48
                    } else {
                        r0 = __float_as_uint(q2.z);
                        r1 = __float_as_uint(q2.w);
                        r2 = __float_as_uint(q3.x);
                        r3 = __float_as_uint(q3.y);
                    }
#define RT3_Q(w, b) ((float)(((w) >> (8 * (b))) & 0xFFu))
#define RT3_SLABQ(lx, ly, lz, hx, hy, hz, tn) \
    slab_test_q(__builtin_fmaf(lx, A.x, B.x), __builtin_fmaf(hx, A.x, B.x), __builtin_fmaf(ly, A.y, B.y), __builtin_fmaf(hy, A.y, B.y), \
                __builtin_fmaf(lz, A.z, B.z), __builtin_fmaf(hz, A.z, B.z), tmin, r.best.t, tn)
                    if (LAYOUT == kLayoutWide64Q) {
#define RT3_SLABS(wlo, whi, selp, selq, tn)                                                                                                    \
    (TWO ? slab_test_sorted_pad(__builtin_amdgcn_perm(whi, wlo, selp), __builtin_amdgcn_perm(whi, wlo, selq), A, B, tl_pad, tmin, r.best.t, tn) \
         : slab_test_sorted(__builtin_amdgcn_perm(whi, wlo, selp), __builtin_amdgcn_perm(whi, wlo, selq), A, B, tmin, r.best.t, tn))
                        h0 = RT3_SLABS(w0, w1, r.sel_p0, r.sel_q0, t0) & (r0 != kEmptySlot);
                        h1 = RT3_SLABS(w1, w2, r.sel_p1, r.sel_q1, t1) & (r1 != kEmptySlot);
                        h2 = RT3_SLABS(w3, w4, r.sel_p0, r.sel_q0, t2) & (r2 != kEmptySlot);
                        h3 = RT3_SLABS(w4, w5, r.sel_p1, r.sel_q1, t3) & (r3 != kEmptySlot);
#undef RT3_SLABS
                    } else {
                    h0 = RT3_SLABQ(RT3_Q(w0, 0), RT3_Q(w0, 1), RT3_Q(w0, 2), RT3_Q(w0, 3), RT3_Q(w1, 0), RT3_Q(w1, 1), t0) & (r0 != kEmptySlot);
                    h1 = RT3_SLABQ(RT3_Q(w1, 2), RT3_Q(w1, 3), RT3_Q(w2, 0), RT3_Q(w2, 1), RT3_Q(w2, 2), RT3_Q(w2, 3), t1) & (r1 != kEmptySlot);
                    h2 = RT3_SLABQ(RT3_Q(w3, 0), RT3_Q(w3, 1), RT3_Q(w3, 2), RT3_Q(w3, 3), RT3_Q(w4, 0), RT3_Q(w4, 1), t2) & (r2 != kEmptySlot);
                    h3 = RT3_SLABQ(RT3_Q(w4, 2), RT3_Q(w4, 3), RT3_Q(w5, 0), RT3_Q(w5, 1), RT3_Q(w5, 2), RT3_Q(w5, 3), t3) & (r3 != kEmptySlot);
                    }
#undef RT3_Q
#undef RT3_SLABQ
                } else {
                    r0 = __float_as_uint(q1.z);
                    r1 = __float_as_uint(q3.z);
                    r2 = __float_as_uint(q5.z);
                    r3 = __float_as_uint(q7.z);
                    h0 = slab_test_hw(v3(q0.x, q0.y, q0.z), v3(q0.w, q1.x, q1.y), o, inv, tmin, r.best.t, t0) & (r0 != kEmptySlot);
                    h1 = slab_test_hw(v3(q2.x, q2.y, q2.z), v3(q2.w, q3.x, q3.y), o, inv, tmin, r.best.t, t1) & (r1 != kEmptySlot);
                    h2 = slab_test_hw(v3(q4.x, q4.y, q4.z), v3(q4.w, q5.x, q5.y), o, inv, tmin, r.best.t, t2) & (r2 != kEmptySlot);
                    h3 = slab_test_hw(v3(q6.x, q6.y, q6.z), v3(q6.w, q7.x, q7.y), o, inv, tmin, r.best.t, t3) & (r3 != kEmptySlot);
                }
                // sort key: the entry distance for the closest hit (nearest child first); its NEGATIVE for any-hit rays
                // (farthest child first).  Occlusion does not depend on the order, but a shadow ray starts on a surface whose
                // neighbourhood it only grazes and is usually blocked far away (ceiling, opposite wall): far-first reaches that
                // occluder in ~35 % fewer node visits than slot order.  Non-entered slots carry +inf and sink to the end.
                // A slot that was not entered keeps its raw reference: after the sort the entered slots are the first nh candidates (every
                // entered key is finite, so +inf is never in front of one), and nh gates every use of a reference below -- r.cur is popped
                // over when nh == 0, the pushes ask nh > 1 / 2 / 3.  Four selects less per node.
                Cand c0{h0 ? (ANY ? -t0 : t0) : kInf, r0}, c1{h1 ? (ANY ? -t1 : t1) : kInf, r1};
                Cand c2{h2 ? (ANY ? -t2 : t2) : kInf, r2}, c3{h3 ? (ANY ? -t3 : t3) : kInf, r3};
                const uint32_t nh = (uint32_t)h0 + (uint32_t)h1 + (uint32_t)h2 + (uint32_t)h3;
                // 5-comparator sorting network on the key
                cswap(c0, c1);
                cswap(c2, c3);
                cswap(c0, c2);
                cswap(c1, c3);
                cswap(c1, c2);
                if (nh > 3) {
                    if (r.sp < kLdsStack) lds[r.sp * kExtendBlock] = c3.ref;
                    else spill[r.sp - kLdsStack] = c3.ref;
                    ++r.sp;
                }
                if (nh > 2) {
                    if (r.sp < kLdsStack) lds[r.sp * kExtendBlock] = c2.ref;
                    else spill[r.sp - kLdsStack] = c2.ref;
                    ++r.sp;
                }
                if (nh > 1) {
                    if (r.sp < kLdsStack) lds[r.sp * kExtendBlock] = c1.ref;
                    else spill[r.sp - kLdsStack] = c1.ref;
                    ++r.sp;
                }
                r.cur = c0.ref;
                pop = nh == 0;
            } else {
                float tn0, tn1;
                uint32_t r0 = __float_as_uint(q3.x), r1 = __float_as_uint(q3.y);
                bool h0 = slab_test_hw(v3(q0.x, q0.y, q0.z), v3(q0.w, q1.x, q1.y), o, inv, tmin, r.best.t, tn0) & (r0 != kEmptySlot);
                bool h1 = slab_test_hw(v3(q1.z, q1.w, q2.x), v3(q2.y, q2.z, q2.w), o, inv, tmin, r.best.t, tn1) & (r1 != kEmptySlot);
                bool near1 = tn1 < tn0;
                if (h0 & h1) {
                    uint32_t far = near1 ? r0 : r1;
                    if (r.sp < kLdsStack) lds[r.sp * kExtendBlock] = far;
                    else spill[r.sp - kLdsStack] = far;
                    ++r.sp;
                }
                r.cur = (h0 & h1) ? (near1 ? r1 : r0) : (h0 ? r0 : r1);
                pop = !(h0 | h1);
            }
        }
        if (pop && !done) {
            if (TWO && tl_bottom && (uint32_t)r.sp == tl_mark) {  // the bottom tree is done: back to the world ray and the top tree's entries
                tl_world();
                tl_sels();
            }
            if (r.sp == 0) {
                done = true;
            } else {
                --r.sp;
                // two explicit paths: a pointer select here would turn the pop into a flat_load
                if (r.sp < kLdsStack) {
                    r.cur = lds[r.sp * kExtendBlock];
                } else {
                    r.cur = spill[r.sp - kLdsStack];
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        // kMaxSteps bounds the walk so that a corrupt tree can never hang the GPU (a valid tree visits < 2 n nodes)
        if (++r.steps >= kMaxSteps) done = true;
        if (done) {
            if constexpr (EXIT) {
                // the entry's leaf occluded the ray: a hit with the root still pending (the root is nobody's child, so no walk pushes it)
                by_entry = r.best.prim != kMiss && r.sp == 1 && lds[0] == (use_top ? kTopFlag : 0u);
            }
            finish(r.index, r.best, r.cn, r.ct, r.cl, r.pay0, r.pay1, r.pay2, r.pay3);
            busy = false;
        }
        }  // if (busy)
        // counted here, where the whole wave passes: a sum kept inside the divergent region would be one per lane (two scalar instructions a step)
        if constexpr (EXIT) xw->occluded += (uint32_t)__popcll(__ballot(by_entry));
    }
}

// counting mode: the per-ray counts a traversal kernel stores (cnt_nodes / cnt_tris, either may be null) and the sums each thread adds,
// once, at its end to totals[0..1] and lds_total
template <bool COUNT>
struct TraceCounts {
    uint32_t *cnt_nodes, *cnt_tris;
    unsigned long long nodes = 0, tris = 0, lds = 0;
    __device__ __forceinline__ void ray(uint32_t i, uint32_t cn, uint32_t ct, uint32_t cl) {
        if (!COUNT) return;
        if (cnt_nodes) cnt_nodes[i] = cn;
        if (cnt_tris) cnt_tris[i] = ct;
        nodes += cn;
        tris += ct;
        lds += cl;
    }
    __device__ __forceinline__ void add_totals(unsigned long long* totals, unsigned long long* lds_total) {
        if (!COUNT || !totals) return;
        atomicAdd(&totals[0], nodes);
        atomicAdd(&totals[1], tris);
        if (lds_total) atomicAdd(lds_total, lds);
    }
};

// the alpha-mask kernel argument: AlphaDev for the MASK instances; for the others an empty struct, placed in the padding after a 32-bit
// argument, so that their argument layout -- and their machine code -- stays what it is without masks
template <bool MASK>
struct AlphaArg {
    AlphaDev a;
    __device__ __forceinline__ AlphaDev get() const { return a; }
};
template <>
struct AlphaArg<false> {
    __device__ __forceinline__ AlphaDev get() const { return AlphaDev{}; }
};

// closest-hit over a ray queue.  rays: two float4 streams of `stride` records, {o.xyz, tmin} then {d.xyz, tmax};
// hits: one float4 {t, u, v, prim} per ray.  16-byte records are the widest coalesced access (1 KiB per wave instruction).
template <bool COUNT, int LAYOUT, bool MASK = false>
__global__ __launch_bounds__(kExtendBlock) void k_extend(const float4* __restrict__ nodes, uint32_t tri_off, const float4* __restrict__ top, uint32_t n_top,
                                                         const float* __restrict__ rays, size_t stride,
                                                         const uint32_t* __restrict__ count_ptr, uint32_t count_imm,
                                                         float* __restrict__ hits, uint32_t* __restrict__ cnt_nodes,
                                                         uint32_t* __restrict__ cnt_tris, unsigned long long* __restrict__ totals,
                                                         uint32_t* __restrict__ work_counter, int payload, AlphaArg<MASK> alpha,
                                                         unsigned long long* __restrict__ lds_total) {
    __shared__ uint32_t stack[kLdsStack * kExtendBlock];
    __shared__ float4 s_top[4 * kTopNodes];
    const bool use_top = load_top(s_top, top, n_top);  // (the LDS array itself is passed on, never a selected pointer: a select would turn its reads into flat loads)
    const uint32_t n = count_ptr ? *count_ptr : count_imm;
    TraceCounts<COUNT> counts{cnt_nodes, cnt_tris};
    auto finish = [&](uint32_t i, const Hit& h, uint32_t cn, uint32_t ct, uint32_t cl, float, float, float, float) {
        // one 16-byte record per ray: with persistent waves rays finish out of order, four SoA streams would be four
        // scattered partial-line writes
        reinterpret_cast<float4*>(hits)[i] = make_float4(h.t, h.u, h.v, __uint_as_float(h.prim));
        counts.ray(i, cn, ct, cl);
    };
    trace_stream<0, COUNT, LAYOUT == kLayoutTwoLevel ? kLayoutWide64Q : LAYOUT, LAYOUT == kLayoutTwoLevel, false, MASK>(
        nodes, tri_off, rays, stride, n, work_counter, stack + threadIdx.x, finish, false, payload != 0, s_top, use_top, nullptr, nullptr, alpha.get());
    counts.add_totals(totals, lds_total);
}

// any-hit over the shadow queue; unoccluded rays add their contribution to the path's radiance slot.
// If `occluded_out` != nullptr the kernel only reports occlusion (rt3_trace_rays).
// RANGE: the emitter shadow queue, whose rays end short of their sampled emitter point (range (kRayTMin, tmax[i]))
template <bool COUNT, int LAYOUT, bool RANGE = false, bool MASK = false>
__global__ __launch_bounds__(kExtendBlock) void k_shadow(const float4* __restrict__ nodes, uint32_t tri_off, const float4* __restrict__ top, uint32_t n_top,
                                                         const float* __restrict__ rays, size_t stride,
                                                         const uint32_t* __restrict__ count_ptr, uint32_t count_imm, AlphaArg<MASK> alpha,
                                                         const float* __restrict__ contrib, float* __restrict__ lacc,
                                                         uint32_t* __restrict__ occluded_out, uint32_t* __restrict__ cnt_nodes,
                                                         uint32_t* __restrict__ cnt_tris, unsigned long long* __restrict__ totals,
                                                         uint32_t* __restrict__ work_counter, unsigned long long* __restrict__ lds_total,
                                                         const float* __restrict__ tmax) {
    __shared__ uint32_t stack[kLdsStack * kExtendBlock];
    __shared__ float4 s_top[4 * kTopNodes];
    const bool use_top = load_top(s_top, top, n_top);  // (the LDS array itself is passed on, never a selected pointer: a select would turn its reads into flat loads)
    const uint32_t n = count_ptr ? *count_ptr : count_imm;
    TraceCounts<COUNT> counts{cnt_nodes, cnt_tris};
    trace_stream<1, COUNT, LAYOUT == kLayoutTwoLevel ? kLayoutWide64Q : LAYOUT, LAYOUT == kLayoutTwoLevel, RANGE, MASK>(
        nodes, tri_off, rays, stride, n, work_counter, stack + threadIdx.x,
        [&](uint32_t i, const Hit& h, uint32_t cn, uint32_t ct, uint32_t cl, float c_r, float c_g, float c_b, float c_pid) {
            if (occluded_out) {
                occluded_out[i] = h.prim != kMiss ? 1u : 0u;
            } else if (h.prim == kMiss) {
                // red and green rode with the ray, {blue, path id} arrived with it: one 16-byte read-modify-write per path, and the
                // wave waits for ONE round trip here (it used to be two: the id first, the slot after)
                float4* L = reinterpret_cast<float4*>(lacc) + __float_as_uint(c_pid);
                float4 v = *L;
                *L = make_float4(v.x + c_r, v.y + c_g, v.z + c_b, 0.0f);
            }
            counts.ray(i, cn, ct, cl);
        },
        occluded_out == nullptr, false, s_top, use_top, occluded_out == nullptr ? reinterpret_cast<const float2*>(contrib) : nullptr, tmax,
        alpha.get());
    counts.add_totals(totals, lds_total);
}

// k_shadow<COUNT, LAYOUT, RANGE, MASK = true> for a structure with panes (rt3_scene_set_pane_shadows): the path tracer's own
// shadow queues only (no reporting mode), and an unoccluded ray adds its contribution as the panes it crossed left it.  A kernel of its own
// name, so that every instance of k_shadow keeps its name and its instructions.  Always carries the alpha test: a scene without masks has no
// record with a cutoff, and its alpha table is never read.
template <bool COUNT, int LAYOUT, bool RANGE>
__global__ __launch_bounds__(kExtendBlock) void k_shadow_pane(const float4* __restrict__ nodes, uint32_t tri_off, const float4* __restrict__ top, uint32_t n_top,
                                                              const float* __restrict__ rays, size_t stride,
                                                              const uint32_t* __restrict__ count_ptr, uint32_t count_imm, AlphaDev alpha, PaneDev pane,
                                                              const float* __restrict__ contrib, float* __restrict__ lacc,
                                                              uint32_t* __restrict__ cnt_nodes, uint32_t* __restrict__ cnt_tris,
                                                              unsigned long long* __restrict__ totals, uint32_t* __restrict__ work_counter,
                                                              unsigned long long* __restrict__ lds_total, const float* __restrict__ tmax) {
    __shared__ uint32_t stack[kLdsStack * kExtendBlock];
    __shared__ float4 s_top[4 * kTopNodes];
    const bool use_top = load_top(s_top, top, n_top);
    const uint32_t n = count_ptr ? *count_ptr : count_imm;
    TraceCounts<COUNT> counts{cnt_nodes, cnt_tris};
    trace_stream<1, COUNT, LAYOUT == kLayoutTwoLevel ? kLayoutWide64Q : LAYOUT, LAYOUT == kLayoutTwoLevel, RANGE, true, false, true>(
        nodes, tri_off, rays, stride, n, work_counter, stack + threadIdx.x,
        [&](uint32_t i, const Hit& h, uint32_t cn, uint32_t ct, uint32_t cl, float c_r, float c_g, float c_b, float c_pid) {
            if (h.prim == kMiss) {
                float4* L = reinterpret_cast<float4*>(lacc) + __float_as_uint(c_pid);
                float4 v = *L;
                *L = make_float4(v.x + c_r, v.y + c_g, v.z + c_b, 0.0f);
            }
            counts.ray(i, cn, ct, cl);
        },
        true, false, s_top, use_top, reinterpret_cast<const float2*>(contrib), tmax, alpha, nullptr, &pane);
    counts.add_totals(totals, lds_total);
}

// k_shadow<false, kLayoutWide64Q, false, MASK> with the exit table (DESIGN.md sections 5 and 7): the same queue, the same finish; every ray, or
// every 32nd chunk of rays, first tries the leaf its exit cell names.  exit_off: the table's header in the arena; counters: the context's
// {rays that started at an entry, rays an entry's leaf occluded}.
template <bool MASK>
__global__ __launch_bounds__(kExtendBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_shadow_exit(const float4* __restrict__ nodes, uint32_t tri_off, const float4* __restrict__ top, uint32_t n_top,
                                                              const float* __restrict__ rays, size_t stride,
                                                              const uint32_t* __restrict__ count_ptr, uint32_t count_imm, AlphaArg<MASK> alpha,
                                                              const float* __restrict__ contrib, float* __restrict__ lacc,
                                                              uint32_t* __restrict__ occluded_out, uint32_t* __restrict__ work_counter, uint32_t exit_off,
                                                              unsigned long long* __restrict__ counters) {
    __shared__ uint32_t stack[kLdsStack * kExtendBlock];
    __shared__ float4 s_top[4 * kTopNodes];
    const bool use_top = load_top(s_top, top, n_top);
    const uint32_t n = count_ptr ? *count_ptr : count_imm;
    // The switch: every ray starts at its table entry while fewer than 2^16 rays have, and while at least a quarter of those that did were
    // occluded by the entry's leaf; below that only every 32nd chunk does.  Every workgroup reads the counters at its own start, and the
    // workgroups of the same launch add to them at their end: on a queue so short that some finish before others start, two workgroups of
    // one launch can decide differently, and block 0's count of started rays then follows its own decision.  That moves the rate a
    // little and no result.  (The launcher takes this kernel only for a structure that has nodes and a table.)
    ExitWalk xw;
    xw.off = exit_off;
    {
        const unsigned long long tried = counters[0], occluded = counters[1];
        xw.mode = (tried < kExitWarmupTries || 4ull * occluded >= tried) ? 2u : 1u;
    }
    trace_stream<1, false, kLayoutWide64Q, false, false, MASK, true>(
        nodes, tri_off, rays, stride, n, work_counter, stack + threadIdx.x,
        [&](uint32_t i, const Hit& h, uint32_t, uint32_t, uint32_t, float c_r, float c_g, float c_b, float c_pid) {
            if (occluded_out) {
                occluded_out[i] = h.prim != kMiss ? 1u : 0u;
            } else if (h.prim == kMiss) {
                float4* L = reinterpret_cast<float4*>(lacc) + __float_as_uint(c_pid);
                float4 v = *L;
                *L = make_float4(v.x + c_r, v.y + c_g, v.z + c_b, 0.0f);
            }
        },
        occluded_out == nullptr, false, s_top, use_top, occluded_out == nullptr ? reinterpret_cast<const float2*>(contrib) : nullptr, nullptr, alpha.get(), &xw);
    {  // the workgroup's count: its waves' scalars through the stack's LDS, which nobody walks any more
        __syncthreads();
        if ((threadIdx.x & 63u) == 0u) stack[threadIdx.x >> 6] = xw.occluded;
        __syncthreads();
        if (threadIdx.x == 0u) {
            unsigned long long o = 0;
            for (uint32_t w = 0; w < kExtendBlock / 64u; w++) o += stack[w];
            if (o) atomicAdd(&counters[1], o);
            if (blockIdx.x == 0u) {  // the rays that started at an entry follow from the queue's length: all of them, or the sampled chunks
                const unsigned long long t = xw.mode == 2u ? n : exit_sampled_rays(n, pool_chunk_for(n, gridDim.x * (kExtendBlock / 64u)));
                if (t) atomicAdd(&counters[0], t);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ launchers
// The k_extend / k_shadow instance of (count, layout, mask): `launch` is called with std::integral_constant<bool, COUNT>,
// std::integral_constant<int, LAYOUT> and std::integral_constant<bool, MASK>.  A layout that is none of the named ones runs as kLayoutBinary64.
// MASK instances exist for the default layout and the two-level one only (rt3_accel_build refuses masks with the others).
template <typename Launch>
static void dispatch_traversal(bool count, int layout, bool masked, Launch launch) {
    auto by_mask = [&](auto c, auto l) {
        if (masked) launch(c, l, std::true_type{});
        else launch(c, l, std::false_type{});
    };
    auto by_layout = [&](auto c) {
        if (layout == kLayoutTwoLevel) by_mask(c, std::integral_constant<int, kLayoutTwoLevel>{});
        else if (layout == kLayoutWide48Q) launch(c, std::integral_constant<int, kLayoutWide48Q>{}, std::false_type{});
        else if (layout == kLayoutWide64Q) by_mask(c, std::integral_constant<int, kLayoutWide64Q>{});
        else if (layout == kLayoutWide128) launch(c, std::integral_constant<int, kLayoutWide128>{}, std::false_type{});
        else launch(c, std::integral_constant<int, kLayoutBinary64>{}, std::false_type{});
    };
    if (count) by_layout(std::true_type{});
    else by_layout(std::false_type{});
}
template <bool MASK>
static AlphaArg<MASK> alpha_arg(const TraceLaunch& L) {
    if constexpr (MASK) return AlphaArg<true>{L.alpha};
    else return AlphaArg<false>{};
}
void launch_extend(hipStream_t st, const LbvhResult& bvh, const TraceLaunch& L) {
    const unsigned grid = grid_for(L.n, kExtendBlock, g_trace_max_blocks);
    unsigned long long* const tot = L.totals ? L.totals + kTotExtendNodes : nullptr;
    unsigned long long* const lds_tot = L.totals ? L.totals + kTotExtendLds : nullptr;
    dispatch_traversal(L.count, bvh.layout, L.alpha.table != nullptr, [&](auto c, auto l, auto m) {
        hipLaunchKernelGGL((k_extend<decltype(c)::value, decltype(l)::value, decltype(m)::value>), dim3(grid), dim3(kExtendBlock), 0, st, bvh.nodes.get(),
                           bvh.tri_off, bvh.top.get(), bvh.n_top, L.rays, L.stride, L.count_ptr, L.n, L.hits, L.cnt_nodes, L.cnt_tris, tot, L.work_counter,
                           L.payload ? 1 : 0, alpha_arg<decltype(m)::value>(L), lds_tot);
    });
}
// the k_shadow_pane instance of (count, layout, range): L.pane set, the path tracer's own queue (contrib and lacc set, no reporting).  Never
// from the exit table: a leaf tried there is walked again from the root and would attenuate twice.
static void launch_shadow_pane(hipStream_t st, const LbvhResult& bvh, const TraceLaunch& L, unsigned grid) {
    unsigned long long* const tot = L.totals ? L.totals + kTotShadowNodes : nullptr;
    unsigned long long* const lds_tot = L.totals ? L.totals + kTotShadowLds : nullptr;
    auto launch = [&](auto c, auto l, auto range) {
        hipLaunchKernelGGL((k_shadow_pane<decltype(c)::value, decltype(l)::value, decltype(range)::value>), dim3(grid), dim3(kExtendBlock), 0, st, bvh.nodes.get(),
                           bvh.tri_off, bvh.top.get(), bvh.n_top, L.rays, L.stride, L.count_ptr, L.n, L.alpha, *L.pane, L.contrib, L.lacc, L.cnt_nodes, L.cnt_tris, tot,
                           L.work_counter, lds_tot, L.tmax);
    };
    auto by_range = [&](auto c, auto l) {
        if (L.tmax) launch(c, l, std::true_type{});
        else launch(c, l, std::false_type{});
    };
    auto by_layout = [&](auto c) {
        if (bvh.layout == kLayoutTwoLevel) by_range(c, std::integral_constant<int, kLayoutTwoLevel>{});
        else by_range(c, std::integral_constant<int, kLayoutWide64Q>{});
    };
    if (L.count) by_layout(std::true_type{});
    else by_layout(std::false_type{});
}
void launch_shadow(hipStream_t st, const LbvhResult& bvh, const TraceLaunch& L) {
    const unsigned grid = grid_for(L.n, kExtendBlock, g_trace_max_blocks);
    if (L.pane != nullptr && L.occluded == nullptr && (bvh.layout == kLayoutWide64Q || bvh.layout == kLayoutTwoLevel)) return launch_shadow_pane(st, bvh, L, grid);
    if (!L.from_root && bvh.exit.on && bvh.exit.off && bvh.exit.counters && bvh.layout == kLayoutWide64Q && bvh.nodes && !L.count && !L.tmax) {  // the plain any-hit walk, table present
        auto launch = [&](auto m) {
            hipLaunchKernelGGL((k_shadow_exit<decltype(m)::value>), dim3(grid), dim3(kExtendBlock), 0, st, bvh.nodes.get(), bvh.tri_off, bvh.top.get(), bvh.n_top, L.rays,
                               L.stride, L.count_ptr, L.n, alpha_arg<decltype(m)::value>(L), L.contrib, L.lacc, L.occluded, L.work_counter, bvh.exit.off, bvh.exit.counters);
        };
        if (L.alpha.table != nullptr) launch(std::true_type{});
        else launch(std::false_type{});
        return;
    }
    unsigned long long* const tot = L.totals ? L.totals + kTotShadowNodes : nullptr;
    unsigned long long* const lds_tot = L.totals ? L.totals + kTotShadowLds : nullptr;
    dispatch_traversal(L.count, bvh.layout, L.alpha.table != nullptr, [&](auto c, auto l, auto m) {
        auto launch = [&](auto range) {
            hipLaunchKernelGGL((k_shadow<decltype(c)::value, decltype(l)::value, decltype(range)::value, decltype(m)::value>), dim3(grid), dim3(kExtendBlock), 0,
                               st, bvh.nodes.get(), bvh.tri_off, bvh.top.get(), bvh.n_top, L.rays, L.stride, L.count_ptr, L.n,
                               alpha_arg<decltype(m)::value>(L), L.contrib, L.lacc, L.occluded, L.cnt_nodes, L.cnt_tris, tot, L.work_counter, lds_tot, L.tmax);
        };
        if (L.tmax) launch(std::true_type{});
        else launch(std::false_type{});
    });
}

}  // namespace rt3
