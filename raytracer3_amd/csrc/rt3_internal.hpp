// rt3_internal.hpp -- declarations shared by the kernel translation units and the C-ABI host layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "rt3_camera.hpp"
#include "rt3_emit_tex.hpp"
#include "rt3_glass.hpp"
#include "rt3_math.hpp"
#include "rt3_surface.hpp"

#define RT3_FLAG_NEE_SKY 1u
#define RT3_FLAG_BLUENOISE 2u
#define RT3_FLAG_SPECULAR 4u
#define RT3_FLAG_FACEFORWARD 8u
#define RT3_FLAG_PROBE_RADIANCE 16u
#define RT3_FLAG_NEE_EMISSIVE 32u
#define RT3_FLAG_NEE_PUNCTUAL 64u

namespace rt3 {

constexpr int kExtendBlock = 256;          // threads per traversal workgroup (4 waves)
constexpr unsigned kExtendMaxBlocks = 2048;  // 256 CUs x 8: grid-stride beyond that
// traversal node layouts
constexpr int kLayoutBinary64 = 0;   // 64 B: two fp32 child boxes + two references
constexpr int kLayoutWide128 = 1;    // 128 B: four {fp32 min, max, ref, pad} slots
constexpr int kLayoutWide48Q = 3;    // 48 B: as kLayoutWide64Q, references implied (node_base / tri_base + a nibble per child): 3 loads per node
constexpr int kC48Stride = 3;        // float4s per compact node
constexpr int kLayoutWide64Q = 2;    // 64 B: origin + power-of-two steps + four 8-bit boxes + four references
constexpr int kLayoutTwoLevel = 4;   // RT3_OPT_INSTANCE_MODE 1: kLayoutWide64Q nodes of a top tree over instance records and shared bottom trees (rt3_tlas.hip)
constexpr uint32_t kMaxStack = 64;         // traversal stack entries: LDS short stack (12) + private spill (52)
constexpr uint32_t kTopCacheNodes = 128;   // top-of-tree nodes the traversal kernels hold in LDS (8 KiB)
// counting mode (RT3_OPT_COUNT_TRAVERSAL): the words of the context's block of 64-bit traversal totals.  TraceLaunch::totals is the
// block's base; each kernel adds its {nodes, tris} at the word it is handed (so a kind's two words are adjacent) and its
// LDS-served node visits at a second pointer.
enum TotalsWord : int {
    kTotExtendNodes = 0,
    kTotExtendTris = 1,
    kTotShadowNodes = 2,
    kTotShadowTris = 3,
    kTotExtendLds = 4,  // node visits served by the LDS top-of-tree copy
    kTotShadowLds = 5,
    kTotWords = 6
};

// One k_shade launch (refrence_mode.slang:28-57 for one bounce of every live path): the kernel's argument, filled by the host.  launch_shade
// sets npix_div, sizes the grid from n_first and picks the instance.
struct ShadeLaunch {
    GConstDev g;
    SceneDev sc;
    const uint32_t* pixels;  // x | y << 16, this rank's pixels in render order
    const uint2* pixbn;      // the same list with each pixel's blue-noise word beside it
    uint32_t npix, width;
    FastDiv npix_div;        // path id = sample_in_batch * npix + pixel_index
    uint32_t s0;             // first sample index of this batch
    uint32_t bounce;         // b
    // FIRST: gbuffer images.  GLASS (k_shade_glass, rt3_scene_set_transmission): the side table per flattened geometry
    // in the G-buffer's slot -- a glass frame never shades from the G-buffer (FIRST = false), and a member of its own would move the
    // arguments behind it, the hidden ones included, in every kernel that takes this struct.  launch_shade fills it in.
    union {
        const uint4* gbuffer;
        const GlassDev* glass;
    };
    const float* depth;
    // !FIRST: input queue
    const float* in_rays;
    const float* in_hits;
    const float* in_T;       // throughput: three planes of `stride` floats (the path's pdf and id ride in the .w of its two ray records)
    const uint32_t* in_count;
    uint32_t n_first;        // npix * samples_in_batch: the paths of bounce 0, an upper bound of the live paths after it
    // outputs
    float* out_rays;
    float* out_T;
    uint32_t* out_count;
    float* sh_rays;
    float* sh_contrib;
    uint32_t* sh_count;
    float* lacc;             // float4 {r, g, b, -} per path id
    size_t stride;
    // EMIT (RT3_F_NEE_EMISSIVE): the emitter table and the emitter shadow queue {o, c.r} {d, c.g} {c.b, path id} + range
    // end, and its count; lights.n == 0 = the flag is off
    LightsDev lights;
    float* sh2_rays;
    float* sh2_contrib;
    float* sh2_tmax;
    uint32_t* sh2_count;
};
// The geometry tables a builder reads triangles through: primitive p belongs to geoms[prim_geom[p]] and is that geometry's triangle
// p - first_prim[prim_geom[p]], its corners found through the geometry's offsets into indices and verts.  The five go together: the
// flattened world's, or the world's verts and indices with a bottom tree's tables (local primitive ids).
struct GeomTables {
    const float* verts;
    const uint32_t* indices;
    const FlatGeomDev* geoms;
    const uint32_t *prim_geom, *first_prim;
};

// blocks of `block` threads that cover n elements: at least one, at most max_blocks (grid-stride beyond that)
inline unsigned grid_for(uint64_t n, unsigned block, unsigned max_blocks) {
    uint64_t b = (n + block - 1) / block;
    if (b < 1) b = 1;
    return (unsigned)(b > max_blocks ? max_blocks : b);
}

void launch_raygen(hipStream_t st, const GConstDev& g, const uint32_t* pixels, uint32_t npix, float* rays, size_t stride);
void launch_gbuffer(hipStream_t st, const SceneDev& sc, const uint32_t* pixels, uint32_t npix, uint32_t width, const float* hits,
                    size_t stride, void* gbuffer, float* depth);
// punct: L.lights holds punctual records; glass: the built scene's transmission table (null: none), never with `first`
// defer: k_shade_defer -- the sky shadow queue then holds plain ray records in sh_rays and, in sh_contrib, one plane
// of `stride` words with each ray's vertex (its index in the input queue) and a second plane for k_shadow's occlusion words; launch_light
// finishes the unoccluded light samples from them.  Only without material textures, punctual lights and glass.
// pane_dist (with glass): k_shade_pane and its per-path distance array, one float per path of the batch, zero at its start
// frost (with glass): k_shade_frost -- the built scene has a frosted geometry (pane_dist as above, or null)
// exit (with defer, no emitter table): k_shade_defer_exit, which tries a sky shadow ray against the leaf of its
// exit-table entry and queues it only when that leaf does not occlude it
struct ShadeExit {
    const float4* arena = nullptr;            // the structure's arena (LbvhResult::nodes): triangle records at tri_off, the table at exit_off
    uint32_t tri_off = 0, exit_off = 0;
    unsigned long long* counters = nullptr;   // the context's {rays that tried an entry, rays an entry occluded} (ExitTable::counters)
    uint32_t* decided = nullptr;              // the bounce's word for the shadow rays that were generated and decided here, never queued
};
void launch_shade(hipStream_t st, bool first, ShadeLaunch L, bool punct = false, const GlassDev* glass = nullptr, bool defer = false, float* pane_dist = nullptr,
                  const ShadeExit* exit = nullptr, bool frost = false);
void launch_light(hipStream_t st, bool first, ShadeLaunch L);
void launch_pixbn(hipStream_t st, const uint32_t* pixels, uint32_t npix, const uint8_t* bluenoise, uint32_t bn_w, uint32_t bn_h, uint2* out);
void launch_accumulate(hipStream_t st, const GConstDev& g, const uint32_t* pixels, uint32_t npix, uint32_t width, const float* depth,
                       const float* lacc, size_t stride, uint32_t sb, int first_batch, int last_batch, float* radsum, void* light,
                       const void* prev);
void launch_postprocess(hipStream_t st, const GConstDev& g, const SceneDev& sc, const uint32_t* pixels, uint32_t npix, uint32_t width,
                        const float* depth, const void* in, void* out);
// per-sample camera rays (rt3_lens.hip)
// the camera rays of samples s0 .. of the listed pixels as records 0 .. n_first-1 of the extension queue `rays` (path id = record index), with
// throughput 1 in T and radiance 0 in lacc; *count = n_first
void launch_lens_rays(hipStream_t st, const GConstDev& g, const LensDev& lens, const uint32_t* pixels, uint32_t npix, uint32_t s0, uint32_t n_first,
                      float* rays, float* T, float* lacc, size_t stride, uint32_t* count);
// the sky's radiance into lacc for the records of that queue whose hit is a miss
void launch_lens_miss(hipStream_t st, const SceneDev& sc, const float* rays, const float* hits, float* lacc, size_t stride, uint32_t n);
// launch_accumulate for every listed pixel, background-centred ones included
void launch_accumulate_lens(hipStream_t st, const GConstDev& g, const uint32_t* pixels, uint32_t npix, uint32_t width, const float* lacc, uint32_t sb,
                            int first_batch, int last_batch, float* radsum, void* light, const void* prev);
// launch_postprocess with every pixel taken from `in`
void launch_postprocess_lens(hipStream_t st, const uint32_t* pixels, uint32_t npix, uint32_t width, const void* in, void* out);
// guide images of a lens frame (rt3_guide.hip): k_lens_guide over the camera queue `rays` and its hit queue `hits`
// (record = sample_in_batch * npix + pixel index, `stride` records per plane), both read-only, for samples of one batch; img = {position,
// normal, albedo, emission}, window-space float4 images of row length `width`.  first_batch: the sums start at 0; last_batch: the sums
// become means over `samples`, the frame's sample count.  The grid covers npix, or is `groups` workgroups when that is not 0 (self-test
// op 39).  GuidePrevLaunch, below the "motion" pass's tables, describes k_lens_guide_prev's launch over the same queues
struct GuideLaunch {
    SceneDev sc;
    const uint32_t* pixels;
    uint32_t npix, width;
    const float *rays, *hits;
    size_t stride;
    uint32_t nsb, samples;
    bool first_batch, last_batch;
    float4* img[4];
};
void launch_lens_guide(hipStream_t st, const GuideLaunch& a, uint32_t groups = 0);
// self-test op 39: k_lens_guide on caller-made queues; header words, then the pixel words, then records of kSelftestGuideRecord words;
// kSelftestGuideOut words out per listed pixel
constexpr uint32_t kSelftestGuideHeader = 6, kSelftestGuideRecord = 10, kSelftestGuideOut = 16;
// self-test op 31: lens_ray, kSelftestLensIn words in, kSelftestLensOut words out
constexpr uint32_t kSelftestLensIn = 41, kSelftestLensOut = 10;
void launch_selftest_lens(hipStream_t st, const uint32_t* in, uint32_t n, uint32_t* out);
// self-test op 32: glass_sample, {ior, thin_walled, d xyz, n xyz, u} -> {event, direction xyz, F} (rt3_shade.hip)
constexpr uint32_t kSelftestGlassIn = 9, kSelftestGlassOut = 5;
void launch_selftest_glass(hipStream_t st, const uint32_t* in, uint32_t n, uint32_t* out);
// self-test op 38: the frosted vertex rule, {ior, thin_walled, d xyz, n xyz, alpha, u_event, u2, u3} -> {event, direction xyz, F, weight} (rt3_shade.hip)
constexpr uint32_t kSelftestFrostIn = 12, kSelftestFrostOut = 6;
void launch_selftest_frost(hipStream_t st, const uint32_t* in, uint32_t n, uint32_t* out);
// Russian roulette on the extension queue (rt3_roulette.hip); rt3_roulette.hpp has the argument.  The grid is sized
// for n_max records (an upper bound of *in_count), or is `groups` workgroups when that is not 0 (self-test op 34)
struct RouletteLaunch;
void launch_roulette(hipStream_t st, const RouletteLaunch& a, uint32_t n_max, uint32_t groups = 0);
// self-test op 33: roulette_rule, {T rgb, min_survival, u} -> {survived, T' rgb, q_g}
constexpr uint32_t kSelftestRouletteIn = 5, kSelftestRouletteOut = 5;
void launch_selftest_roulette(hipStream_t st, const uint32_t* in, uint32_t n, uint32_t* out);
// self-test op 34: k_roulette on a caller-made queue; header words, then the pixel words, then records of kSelftestQueueRecord words
constexpr uint32_t kSelftestQueueHeader = 7, kSelftestQueueRecord = 11;
// Beer-Lambert absorption on the extension queue (rt3_volume.hip); rt3_volume.hpp has the argument.  The grid is sized
// for n_max records (an upper bound of *count), or is `groups` workgroups when that is not 0 (self-test op 37)
struct AbsorbLaunch;
void launch_absorb(hipStream_t st, const AbsorbLaunch& a, uint32_t n_max, uint32_t groups = 0);
// self-test op 36: absorb_rule, {T rgb, sigma rgb, t, d xyz, n xyz} -> {T' rgb, applied}
constexpr uint32_t kSelftestAbsorbIn = 13, kSelftestAbsorbOut = 4;
void launch_selftest_absorb(hipStream_t st, const uint32_t* in, uint32_t n, uint32_t* out);
// self-test op 37: k_absorb on a caller-made queue; one header word, then records of kSelftestAbsorbRecord words, three words out per record
constexpr uint32_t kSelftestAbsorbHeader = 1, kSelftestAbsorbRecord = 10;
// Fog (rt3_fog.hip); rt3_fog.hpp has the rule and the arguments.  The grids are sized for n_max records (an upper bound
// of *count), or are `groups` workgroups when that is not 0 (self-test op 46)
struct FogSegmentLaunch;
struct FogShadowLaunch;
void launch_fog_segment(hipStream_t st, const FogSegmentLaunch& a, uint32_t n_max, uint32_t groups = 0);
void launch_fog_shadow(hipStream_t st, const FogShadowLaunch& a, uint32_t n_max, uint32_t groups = 0);
// self-test op 45: the fog rule, {o xyz, d xyz, t, lo xyz, hi xyz, sigma_a rgb, sigma_s rgb, u} -> {in medium, t0, t1, s, pdf, Tr rgb}
constexpr uint32_t kSelftestFogIn = 20, kSelftestFogOut = 8;
void launch_selftest_fog(hipStream_t st, const uint32_t* in, uint32_t n, uint32_t* out);
// self-test op 46: k_fog_segment or k_fog_shadow on caller-made queues (rt3_passes.hip: selftest_fog_queue has the layout)
constexpr uint32_t kSelftestFogQueueHeader = 9, kSelftestFogSegmentRecord = 12, kSelftestFogShadowRecord = 11, kSelftestFogRayOut = 12;
void launch_pack_tiles(hipStream_t st, const uint32_t* pixels, uint32_t npix, uint32_t width, const void* img, void* dst);
void launch_unpack_tiles(hipStream_t st, const uint32_t* pixels, uint32_t npix, uint32_t width, const void* src, void* img);

// probe-GI passes (rt3_probes.hip); atlas images are (8 * probes_x) x (8 * probes_y)
void launch_sis(hipStream_t st, uint32_t W, uint32_t probes_x, uint32_t probes_y, const void* gbuffer, void* out, float* debug);
void launch_probe_raygen(hipStream_t st, const GConstDev& g, uint32_t W, uint32_t probes_x, uint32_t probes_y, const float* depth, const void* directions,
                         void* atlas, float* rays, size_t stride, void* d2);
void launch_probe_store(hipStream_t st, const SceneDev& sc, uint32_t flags, float blend, uint32_t probes_x, uint32_t probes_y, const float* hits,
                        const void* d2, const void* prev, void* atlas);
void launch_sh_conversion(hipStream_t st, uint32_t probes_x, uint32_t probes_y, const void* atlas, void* out);
void launch_interpolate(hipStream_t st, const GConstDev& g, uint32_t W, uint32_t H, const void* gbuffer, const float* depth, const void* sh, void* light);
void launch_selftest_probes(hipStream_t st, int op, const uint32_t* in, uint32_t n, uint32_t* out);

void launch_prim_geom(hipStream_t st, const uint32_t* first_prim, uint32_t n_geoms, uint32_t n, uint32_t* prim_geom);
void set_refill_lanes(uint32_t v);
void set_pool_chunk(uint32_t v);
void set_trace_blocks(uint32_t v);
bool selftest_widths(int op, uint32_t* in_w, uint32_t* out_w);
void launch_selftest(hipStream_t st, int op, const SceneDev& sc, const uint32_t* in, uint32_t n, uint32_t* out);

// early return from host code that returns hipError_t
#define RT3_TRY(x)                           \
    do {                                     \
        const hipError_t e_ = (x);           \
        if (e_ != hipSuccess) return e_;     \
    } while (0)

// Owner of at most one hipMalloc allocation, freed when the owner goes.  The only place the host layer frees device memory.
template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) {
        o.p_ = nullptr;
        o.cap_ = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_;
            cap_ = o.cap_;
            o.p_ = nullptr;
            o.cap_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    T* get() const { return p_; }
    size_t capacity_bytes() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // frees the old allocation BEFORE allocating, so the two never coexist (peak memory); empty on failure
    hipError_t alloc_bytes(size_t bytes) {
        reset();
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) {
            p_ = static_cast<T*>(p);
            cap_ = bytes;
        }
        return e;
    }
    // grow-only: keeps the allocation when it holds `bytes` already, otherwise alloc_bytes
    hipError_t grow_bytes(size_t bytes) { return bytes <= cap_ ? hipSuccess : alloc_bytes(bytes); }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

// Several arrays in one device allocation.  add() records a typed piece (where its pointer goes, how many elements) at the next 256-byte
// boundary; bytes() is the size of all of them; carve() points every recorded pointer into a buffer of at least that size, and refuses a
// smaller one.
class BufLayout {
public:
    template <typename T>
    BufLayout& add(T** dst, size_t count) {
        const size_t at = (end_ + 255) & ~(size_t)255;
        pieces_.push_back({dst, at, &set_ptr<T>});
        end_ = at + count * sizeof(T);
        return *this;
    }
    size_t bytes() const { return end_; }
    hipError_t carve(const DevBuf<char>& buf) const {
        if (buf.capacity_bytes() < end_) return hipErrorOutOfMemory;
        for (const Piece& p : pieces_) p.set(p.dst, buf.get() + p.at);
        return hipSuccess;
    }

private:
    struct Piece {
        void* dst;
        size_t at;
        void (*set)(void* dst, char* p);
    };
    template <typename T>
    static void set_ptr(void* dst, char* p) { *static_cast<T**>(dst) = reinterpret_cast<T*>(p); }
    std::vector<Piece> pieces_;
    size_t end_ = 0;
};

// A piece of an allocation that somebody else owns, with DevBuf's reading interface.
template <typename T>
class DevView {
public:
    DevView() = default;
    explicit DevView(T* p) : p_(p) {}
    T* get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    T* p_ = nullptr;
};

// The traversal kernels address a structure as ONE base plus a 32-bit byte offset per lane: the arena may not be
// larger than this, over-read slack included.
constexpr uint64_t kArenaMaxBytes = (4ull << 30) - 128;
uint64_t next_arena_serial();  // 1, 2, ...: process-wide, one per arena allocated (rt3_lbvh.hip)
constexpr size_t kArenaSlack = 128;  // a leaf fetch reads 64 B (four-wide fp32 layout: 128 B) from a 48 B record: zeroed bytes behind the last record

// Exit table of k_shadow: 6 R^2 leaf references, one per cell of an R x R grid on each face of the
// root box -- the leaf an axis-aligned probe from the cell's centre meets first, or kEmptySlot.  A shadow ray tries the entry of the cell
// where it leaves the box before it walks.  The table lives in the arena behind the slack; a step fetches the 16-byte group of an entry
// with the step's 64-byte batch, so kExitTableSlack bytes follow the last entry.  In front of the entries sits ExitHeader, which the walk
// reads when it starts a ray.
constexpr uint32_t kExitDefaultR = 256, kExitMaxR = 1024;
constexpr size_t kExitTableSlack = 64;
struct ExitHeader {
    float lo[3], hi[3], scale[3];  // ExitTable's
    uint32_t R, last;              // cells per face edge; the last entry's index, 6 R^2 - 1
    uint32_t pad[5];
};
static_assert(sizeof(ExitHeader) == 64, "the entries start 64 bytes behind the header");
constexpr uint64_t kExitWarmupTries = 1ull << 16;  // every ray uses the table until this many have (launch-start decision)
struct ExitTable {
    uint32_t off = 0;                     // byte offset of the table (ExitHeader, then the entries) in the arena; 0 = none
    uint32_t R = 0;                       // cells per face edge
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};  // the box the cells are laid on (the root's, decoded as the walk decodes it)
    float scale[3] = {0, 0, 0};           // R / extent per axis; 0 where the extent is 0 (every ray falls in cell 0 of that axis)
    unsigned long long* counters = nullptr;  // the context's {rays that tried an entry, rays an entry occluded}
    bool on = false;                      // launches use it (RT3_OPT_SHADOW_EXIT_TABLE != 0 and the entries are written)
};

struct LbvhResult {
    // One allocation for what a walk fetches: the node array at byte 0, the triangle records at byte tri_off (the node bytes rounded up to
    // 128), then kArenaSlack zero bytes.  nodes / tris are views into it.
    DevBuf<float4> arena;
    DevView<float4> nodes;     // n_nodes x node_bytes: 64 B {box0, box1, ref0, ref1, pad} or 128 B 4 x {min, max, ref, pad}
    uint32_t node_bytes = 128;
    int layout = kLayoutWide128;
    DevView<float4> tris;      // n_tris x 3 float4 (48 B), Morton order
    uint32_t tri_off = 0;
    uint64_t arena_need = 0;   // the size the last alloc_arena asked for: > kArenaMaxBytes when it refused (hipErrorInvalidValue)
    uint64_t arena_serial = 0; // which allocation the arena is (next_arena_serial, taken where it is allocated); 0 = none
    DevBuf<float4> top;        // quantised four-wide layout: the first n_top nodes in breadth-first order (64 B each), child references to
    uint32_t n_top = 0;        // cached nodes rewritten as 0x40000000 | slot -- the traversal kernels keep this copy in LDS
    uint32_t n_nodes = 0, n_tris = 0, max_depth = 0;
    ExitTable exit;            // k_shadow's exit table: room for it is part of the arena (exit_cells), the host fills it in after a build

    // a fresh arena for nodes_bytes of nodes, n_records triangle records and an exit table of 6 exit_R^2 entries (0 = none); the old one
    // goes first; the slack is zeroed and the table emptied on `st`
    hipError_t alloc_arena(size_t nodes_bytes, size_t n_records, hipStream_t st, uint32_t exit_R = 0) {
        const uint32_t exit_cells = 6u * exit_R * exit_R;
        free_arena();
        const size_t off = (nodes_bytes + 127) & ~(size_t)127, rec_end = off + n_records * 48;
        const size_t table = exit_cells ? sizeof(ExitHeader) + (size_t)exit_cells * 4 + kExitTableSlack : 0;
        arena_need = rec_end + kArenaSlack + table;
        if (arena_need > kArenaMaxBytes) return hipErrorInvalidValue;
        RT3_TRY(arena.alloc_bytes(rec_end + kArenaSlack + table));
        arena_serial = next_arena_serial();
        tri_off = (uint32_t)off;
        nodes = DevView<float4>(arena.get());
        tris = DevView<float4>(reinterpret_cast<float4*>(reinterpret_cast<char*>(arena.get()) + off));
        RT3_TRY(hipMemsetAsync(reinterpret_cast<char*>(arena.get()) + rec_end, 0, kArenaSlack, st));
        if (!table) return hipSuccess;
        exit.R = exit_R;
        exit.off = (uint32_t)(rec_end + kArenaSlack);  // (a multiple of 16: the records start at a multiple of 128 and are 48 bytes each)
        return hipMemsetAsync(reinterpret_cast<char*>(arena.get()) + exit.off, 0xFF, table, st);  // kEmptySlot everywhere (the header is written with the entries)
    }
    void free_arena() {
        arena.reset();
        nodes = tris = DevView<float4>();
        tri_off = 0;
        arena_serial = 0;
        exit = ExitTable{};
    }
    // the arena of `from` becomes this structure's (counts, layout and top copy stay what they are)
    void take_arena(LbvhResult& from) {
        arena = std::move(from.arena);
        nodes = from.nodes;
        tris = from.tris;
        tri_off = from.tri_off;
        arena_serial = from.arena_serial;
        exit = from.exit;
        from.exit = ExitTable{};
        from.nodes = from.tris = DevView<float4>();
        from.tri_off = 0;
        from.arena_serial = 0;
    }
};
// What k_shadow_pane reads besides the tree and the alpha tables (pane shadows): the scene tables hit_finish needs for
// a pane's shading normal and tint, the glass table for its transmission and index, and the first alpha slot that marks a masked pane
// record (an unmasked pane record is {0, 1}; a masked one {cutoff, slot >= first_slot}, its slot a copy of the geometry's alpha entry).
struct PaneDev {
    SceneDev sc;
    const GlassDev* glass;
    uint32_t first_slot;
};
// One traversal launch over a ray queue: closest hit (launch_extend) or any hit (launch_shadow).  Each reads only its own outputs.
struct TraceLaunch {
    const float* rays = nullptr;          // two float4 streams of `stride` records, {o.xyz, tmin} then {d.xyz, tmax}
    size_t stride = 0;
    const uint32_t* count_ptr = nullptr;  // the queue's length on the device, or null
    uint32_t n = 0;                       // the queue's length without count_ptr; with it, the upper bound that sizes the grid
    uint32_t* work_counter = nullptr;     // the launch's ray-pool cursor, zero before it
    float* hits = nullptr;                // closest hit: one float4 {t, u, v, prim} per ray
    bool payload = false;                 // the .w of the ray records carry the path's pdf and id (the path tracer's own queue)
    const float* contrib = nullptr;       // any hit: an unoccluded ray adds its contribution to its path's radiance slot in lacc
    float* lacc = nullptr;
    const float* tmax = nullptr;          // every ray has its own range (kRayTMin, tmax[i]): the emitter queue of RT3_F_NEE_EMISSIVE
    uint32_t* occluded = nullptr;         // set: the launch only reports occlusion (rt3_trace_rays)
    bool count = false;                   // counting: per-ray node visits / triangle tests (either may be null) and the totals (TotalsWord)
    uint32_t *cnt_nodes = nullptr, *cnt_tris = nullptr;
    unsigned long long* totals = nullptr;
    AlphaDev alpha = {};                  // alpha.table set: the structure holds masked triangles, the launch runs the MASK instance
    const PaneDev* pane = nullptr;        // any hit over the path tracer's own queue in a structure with panes: k_shadow_pane
    bool from_root = false;               // any hit: every ray starts at the root even when the structure has an exit table -- the queue holds
                                          // what k_shade_defer_exit has tried against it already
};
// traversal of `bvh` (its layout, nodes, triangle records and LDS top copy)
void launch_extend(hipStream_t st, const LbvhResult& bvh, const TraceLaunch& L);
void launch_shadow(hipStream_t st, const LbvhResult& bvh, const TraceLaunch& L);
// LBVH build (rt3_lbvh.hip).  All pointers are device memory owned by the caller.  The build's scratch is carved from `scratch`, which grows
// to what this configuration and size need and is kept for the next build.  On failure *out may hold some of its arrays: they go with it.
// geom_mask: the alpha-mask words of the triangle records per uploaded geometry, or null (every record {v2.z, prim, 0, 0}).
hipError_t lbvh_build(hipStream_t st, GeomTables t, uint32_t n_prims, uint32_t leaf_max, uint32_t node_width, uint32_t node_quant, uint32_t collapse_mode,
                      uint32_t sah_top, DevBuf<char>& scratch, LbvhResult* out, const uint2* geom_mask = nullptr, uint32_t exit_R = 0);
// exit_R: room in the arena for an exit table of 6 exit_R^2 entries (default node layout only; ignored for the others)

// Exit table (rt3_exit_table.hip).  Scratch of a fill: the probe rays, their hits, the primitive -> leaf reference array, the pool cursor.
struct ExitScratch {
    float *rays, *hits;
    uint32_t *prim_leaf, *cursor;
};
void exit_table_plan(uint32_t cells, uint32_t n_prims, BufLayout& plan, ExitScratch* s);
// Writes the bvh.exit.R^2 x 6 entries of bvh's table from bvh.exit.{lo, hi}: probes through launch_extend, then prim -> leaf reference.
// scramble: every entry becomes a pseudo-random valid leaf reference instead (a test aid: results may not depend on the table's contents).
hipError_t exit_table_fill(hipStream_t st, const LbvhResult& bvh, uint32_t n_prims, const ExitScratch& s, bool scramble);
// Scratch of the binned-SAH top (rt3_sah_top.hip), part of the builder's: sah_top_plan adds it to `plan` for a tree over n triangles (at
// most n clusters under n - 1 top nodes).  The segment and tile records are of types private to rt3_sah_top.hip.
struct SahTopScratch {
    uint32_t *top, *ncl, *pool_pos, *cl_pos, *pool, *cl_ref, *cl_cnt, *idx, *tmp, *counters, *tile_left, *tile_woff, *tile_roff;
    float *cl_mn, *cl_mx;
    char *seg_a, *seg_b, *seg_small, *huge, *tiles;
    char* scan_tmp;
    size_t scan_bytes;
};
hipError_t sah_top_plan(hipStream_t st, uint32_t n, BufLayout& plan, SahTopScratch* s);
// Binned-SAH top: re-links, in place, the nodes of the Karras tree (left / right / rcnt / pint / pleaf, boxes in nbox) above its subtrees
// of at most T triangles, and writes the boxes of the re-linked nodes.  *relinked = false (and nothing written) when there are fewer than
// three such subtrees.
hipError_t sah_top_relink_gpu(hipStream_t st, uint32_t nn, uint32_t* left, uint32_t* right, uint32_t* rcnt, uint32_t* pint, uint32_t* pleaf,
                              const float* lmin, const float* lmax, float* nbox, uint32_t T, const SahTopScratch& s, bool* relinked);

// shading records (SceneDev::tri_shade, tri_uv) of n flattened primitives: they depend on no tree and no matrix
void launch_tri_shade(hipStream_t st, GeomTables t, uint32_t n, uint4* tri_shade, float2* tri_uv);
// tangent words (SceneDev::tri_tan) of the same primitives, for scenes with a normal texture
void launch_tri_tangent(hipStream_t st, GeomTables t, uint32_t n, uint32_t* tri_tan);

// Two-level structure (rt3_tlas.hip).  One node array: [top tree | two 64-byte records per instance | bottom trees], one triangle array of
// the bottom trees' object-space records (local primitive ids).
// dst[k] = src[k] with internal references moved from node_from to node_to and leaf references from tri_from to tri_to
void tlas_rebase_nodes(hipStream_t st, const float4* src, float4* dst, uint32_t n, uint32_t node_from, uint32_t node_to, uint32_t tri_from, uint32_t tri_to);
// n boxes {lo.xyz, hi.xyz} -> the degenerate triangles (lo, hi, lo) whose bounds they are (8-float vertices, indices 0..3n-1): the top tree is
// built by lbvh_build over them
void tlas_box_tris(hipStream_t st, const float* boxes, uint32_t n, float* verts, uint32_t* indices);
// copy the top tree built over those triangles to dst, its leaf references (one triangle each) now naming instance records:
// 0x80000000 | (rec_base + 2 * instance slot)
void tlas_emit_top(hipStream_t st, const float4* top_nodes, uint32_t n_nodes, const float4* top_tris, uint32_t rec_base, float4* dst);

// Refit (rt3_refit.hip) of a quantised 64-byte four-wide tree in place, after its vertices moved (rt3_accel_refit).  The plan comes from the
// node array alone: the internal nodes reachable from `root`, level by level (order[] holds level 0, then level 1, ...).
struct RefitTree {
    DevBuf<uint32_t> order;
    std::vector<uint32_t> level_count;
};
// max_depth: the tree's levels down to the leaf slots (LbvhResult::max_depth); hipErrorInvalidValue if the node array disagrees with it
hipError_t refit_plan(hipStream_t st, const float4* nodes, uint32_t root, uint32_t n_nodes, uint32_t max_depth, RefitTree* plan);
// Rewrites the triangle records [tri_first, tri_first + n_tris) from their primitives (fetched through `t`; the leaf pad from the bounds of
// primitives 0 .. n_prims-1) and then every node of the plan.  Scratch: bounds (6 words), nbox (6 floats per node of `nodes`), tbox (6
// floats per record of `tris`).
hipError_t refit_tree(hipStream_t st, const RefitTree& plan, GeomTables t, uint32_t n_prims, uint32_t tri_first, uint32_t n_tris, float4* nodes,
                      float4* tris, uint32_t* bounds, float* nbox, float* tbox);

// Emitter table of RT3_F_NEE_EMISSIVE (rt3_lights.hip): every flattened primitive of a geometry with non-zero emission,
// in flattened order.  Selection by an integer CDF on the 2^-23 grid of uniform_float; records as LightsDev describes.
struct LightTable {
    DevBuf<float4> rec;                       // 4 per emitter
    DevBuf<uint32_t> cdf, guide, prim, geom_base;
    DevBuf<float> area;
    DevBuf<char> scratch;                     // grow-only: power, quantised power and its scan, the scan's temporary storage
    uint32_t n = 0, n_guide = 0, guide_shift = 0, total = 0;  // total: cdf[n - 1] (2^23, or 0 when no emitter has power)
    // RT3_F_NEE_PUNCTUAL: of the n entries the first n_emit are emitter triangles, the last n_punct punctual lights
    // (prim = kMiss, area = 1, so that their record's p_sel / area is p_sel)
    uint32_t n_emit = 0, n_punct = 0;
    uint64_t stamp = 0;                       // the acceleration-structure stamp the table was built for (0 = none)
    uint64_t lights_stamp = 0;                // the punctual-light list it was built for (rt3_ctx::Scene::lights_stamp)
    uint32_t combo = 0;                       // flags & (RT3_F_NEE_EMISSIVE | RT3_F_NEE_PUNCTUAL) it was built for
    // textured emitters (rt3_scene_set_textured_emitters): the mode and the texture pool (rt3_ctx::Scene::tex_stamp) the
    // table was built for; textured: it holds an emitter with an emissive texture, and only then the side array (one entry per table entry)
    // and k_emit_tex_power's mean texels (3 floats per entry) exist
    bool tex_mode = false, textured = false;
    uint64_t tex_stamp = 0;
    DevBuf<EmitTexDev> emit_tex;
    DevBuf<float> emit_mean;
    LightsDev dev() const {
        LightsDev d;
        d.rec = rec.get(); d.cdf = cdf.get(); d.guide = guide.get(); d.geom_base = geom_base.get();
        d.n = total ? n : 0u; d.guide_shift = guide_shift;
        return d;
    }
};
// geom_base: per flattened geometry its first emitter or kMiss (host table, n_flat_geoms entries); eg_geom / eg_first: the emissive flattened
// geometries and their first emitter (n_eg entries); n: emitters.  Reads back nothing but the CDF's last word (into *total).
// punct / n_punct: the punctual lights to append (host, rt3_punctual_light's 16 words each); n_world_prims: the primitives the tables `t`
// cover, whose box gives the R of a directional light's mass (read only when there are punctual lights).
hipError_t lights_build(hipStream_t st, GeomTables t, const std::vector<uint32_t>& geom_base, const std::vector<uint32_t>& eg_geom,
                        const std::vector<uint32_t>& eg_first, uint32_t n, LightTable* out, const float* punct = nullptr, uint32_t n_punct = 0,
                        uint32_t n_world_prims = 0, const SceneDev* textured = nullptr);
// `textured` (above): the scene's tables when some listed emitter names an uploaded emissive texture (the atlas synchronised), else null.
// k_emit_tex (rt3_emit_tex.hip) over the emitter shadow queue; rt3_emit_tex.hpp has the argument.  The grid is sized for
// n_max records (an upper bound of *count), or is `groups` workgroups when that is not 0 (self-test op 43)
void launch_emit_tex(hipStream_t st, const EmitTexLaunch& a, uint32_t n_max, uint32_t groups = 0);
// self-test op 42: rows {table entry, b1, b2} -> the emitter-side radiance there, 3 words
void launch_selftest_emit_radiance(hipStream_t st, const SceneDev& sc, const float4* rec, const EmitTexDev* emit_tex, const uint32_t* in, uint32_t n, uint32_t* out);
// self-test op 43: k_emit_tex on a caller-made queue; header words, then the pixel words, then records of kSelftestEmitTexRecord words
constexpr uint32_t kSelftestEmitTexHeader = 9, kSelftestEmitTexRecord = 4;
// self-test op 40: the selection part of lights_build (weights, scan, CDF and p_sel / area, guide cells; the same function, scratch layout
// and launch shapes) on n caller-made powers and areas, then light_find on n_k values of k.  Host arrays; max_power is the largest power.
// out: {cells, shift, total}, cdf[n], the records' p_sel / area words [n], guide[cells + 1], n_k entries found.  Every device array is one
// element longer and pattern-filled: *overrun when a word behind an end, or a record word that is not p_sel / area, changed.
constexpr uint32_t kSelftestTableHeaderIn = 2, kSelftestTableHeader = 3;
hipError_t lights_selftest_table(hipStream_t st, uint32_t n, const float* power, float max_power, const float* area, uint32_t n_k, const uint32_t* k,
                                 uint32_t* out, bool* overrun);
// self-test op 30: rows {light index, P, N} -> {wl, range end, cs, I'} from punctual records made of `lights` (n_lights x 16 words, device)
void launch_selftest_light(hipStream_t st, const float4* lights, uint32_t n_lights, const uint32_t* in, uint32_t n, uint32_t* out);

// "denoise" pass (rt3_denoise.hip).  Scratch: two guide records and two signal images of W x H float4, carved from the
// context's grow-only denoise buffer.  Stages in stream order: prepare, variance, `iterations` x atrous (iteration 0, 1, ...), finish.
struct DenoiseScratch {
    float4 *gP, *gN;  // {P.xyz, 1 = foreground} and {n.xyz, 0}; a background record is all zero
    float4* sig[2];   // {c.rgb, variance}, ping-pong
};
struct DenoiseLaunch {
    GConstDev g;
    uint32_t W, H, squarings, flags;
    float sigma_z, sigma_l;
    const void* gbuffer;
    const float* depth;
    const void* in;
    void* out;
    const void* moments = nullptr;  // rt3_denoise_set_variance_input: the "temporal" pass's Moments image, or none
    // rt3_denoise_set_guide_input: {position, normal, albedo, emission} of a lens frame (all set, or all null: the G-buffer guides)
    const float4* guide[4] = {nullptr, nullptr, nullptr, nullptr};
    DenoiseScratch s;
};
void denoise_plan(uint32_t W, uint32_t H, BufLayout& plan, DenoiseScratch* s);
// prepare and finish read L.guide where it is set, in the G-buffer's place; the stages between them do not differ
void launch_denoise_prepare(hipStream_t st, const DenoiseLaunch& L);
void launch_denoise_variance(hipStream_t st, const DenoiseLaunch& L);
void launch_denoise_atrous(hipStream_t st, const DenoiseLaunch& L, uint32_t iteration);
void launch_denoise_finish(hipStream_t st, const DenoiseLaunch& L, uint32_t iterations);
void launch_selftest_denoise(hipStream_t st, const uint32_t* in, uint32_t n, uint32_t* out);  // selftest op 28: expn

// "temporal" pass (rt3_temporal.hip): one kernel, one thread per pixel, no scratch.  `prev` is the previous frame's
// GConst (rt3_temporal_set_prev_view), captured by value like `g`.
struct TemporalLaunch {
    GConstDev g, prev;
    uint32_t W, H, flags;
    float alpha, alpha_moments, max_history, normal_cos, plane_tolerance;
    const void *gbuffer, *in, *prev_gbuffer, *prev_history, *prev_moments;
    const float *depth, *prev_depth;
    void *out, *history, *moments;
    const void* motion = nullptr;  // rt3_temporal_set_motion_input: the "motion" pass's image, or none
    // rt3_temporal_set_guide_input: {position, normal, albedo, emission} of this lens frame and of the previous
    // one (all set, or all null: the G-buffer).  With them k_temporal<TemporalGuide> runs: gbuffer, depth, prev_gbuffer, prev_depth and
    // motion are not read, nor are prev_guide[2] and [3]
    const float4* guide[4] = {nullptr, nullptr, nullptr, nullptr};
    const float4* prev_guide[4] = {nullptr, nullptr, nullptr, nullptr};
    // rt3_temporal_set_guide_motion_input, only with the guide: the samples' mean previous position, the point
    // k_temporal<TemporalGuideMotion> looks up in the previous frame; null: none
    const float4* guide_motion = nullptr;
};
void launch_temporal(hipStream_t st, const TemporalLaunch& L);

// "motion" pass (rt3_motion.hip, DESIGN.md sections 4h and 4i): one kernel behind the primary trace, one thread per listed pixel, no scratch.
// `prev` holds one record per instance; the host's "moved" and "deformed" flags travel as `geom_slot`: per flattened geometry
// kMotionUnmoved, or its instance's index when that instance moved, or that index | kMotionDeformed when the geometry's vertices differ
// from the snapshot (rt3_scene_snapshot_vertices).  geom_slot = nullptr: nothing moved, nothing but `hits` and the camera is read.
constexpr uint32_t kMotionUnmoved = 0xFFFFFFFFu;
constexpr uint32_t kMotionDeformed = 0x80000000u;
struct MotionPrevDev {
    float m[12];        // the previous object -> world matrix, stored like FlatGeomDev::m
    uint32_t identity;  // 1: it is exactly the identity -- the object-space point is used as it is (the flattening's rule)
    uint32_t pad[3];
};
static_assert(sizeof(MotionPrevDev) == 64, "MotionPrev layout");
struct MotionDev {
    const float* verts;
    const uint32_t *indices, *prim_geom, *first_prim, *geom_slot;
    const FlatGeomDev* geoms;
    const MotionPrevDev* prev;
};
struct MotionLaunch {
    GConstDev g;
    MotionDev m;
    const uint32_t* pixels;  // the rank's pixel list, c->hits in its order
    uint32_t npix, width;
    const float* hits;
    void* out;
    const float4* prev_pos = nullptr;  // some geometry is deformed: the snapshot, one {x, y, z, 0} per vertex; selects k_motion<true>
};
void launch_motion(hipStream_t st, const MotionLaunch& L);
// GuideLaunch's companion (rt3_guide.hip): k_lens_guide_prev over the same camera queue and hit queue, following the
// "motion" pass's tables `m` (geom_slot = nullptr: nothing moved, only the queues are read) and the snapshot `prev_pos` (null: nothing is
// deformed).  out: one window-space float4 image of row length `width`, {sum R, n_hit} between batches, {sum R / n_hit, n_hit / samples}
// after the last.  The grid covers npix, or is `groups` workgroups when that is not 0 (self-test op 41)
struct GuidePrevLaunch {
    MotionDev m;
    const float4* prev_pos;
    const uint32_t* pixels;
    uint32_t npix, width;
    const float *rays, *hits;
    size_t stride;
    uint32_t nsb, samples;
    bool first_batch, last_batch;
    float4* out;
};
void launch_lens_guide_prev(hipStream_t st, const GuidePrevLaunch& a, uint32_t groups = 0);
// self-test op 41: k_lens_guide_prev on caller-made queues; op 39's header, pixel words and records; kSelftestGuidePrevOut words out per
// listed pixel
constexpr uint32_t kSelftestGuidePrevOut = 4;
// The snapshot of rt3_scene_snapshot_vertices: prev_pos[v] = {verts[8 v], verts[8 v + 1], verts[8 v + 2], 0} for v in [first, first + n)
void launch_snapshot_positions(hipStream_t st, const float* verts, uint32_t first, uint32_t n, float4* prev_pos);
// Which geometries are deformed: chunk {geometry, lo, hi, -} sets flags[geometry] = 1 when a vertex v in [lo, hi) has a position word that
// differs from prev_pos[v]'s (as uint32).  One 256-thread group per chunk; flags are zeroed by the caller.
constexpr uint32_t kDeformChunk = 1024;  // vertices per chunk, at most
void launch_compare_positions(hipStream_t st, const float* verts, const float4* prev_pos, const uint4* chunks, uint32_t n_chunks, uint32_t* flags);

// Skinning (rt3_skin.hip): one launch of k_skin_pose poses one skin.  Every array is the skin's own, indexed by the
// vertex within the skin: rest 2 x float4 per vertex (the Vertex layout), joints 4 x uint16, weights float4, dpos / dnrm n_targets x n x 3
// floats (tight; dnrm null: normals are not morphed), palette 3 x float4 per joint (pack3x4).  out: the skin's first record in the vertex
// buffer.  flag: the skin's range word.  The caller has checked every joint index against the palette and the range against the buffer.
constexpr uint32_t kSkinMaxTargets = 8;  // == RT3_SKIN_MAX_TARGETS
struct SkinLaunch {
    const float4* rest;
    const uint2* joints;
    const float4* weights;
    const float4* palette;
    const float *dpos, *dnrm;
    float4* out;
    uint32_t* flag;
    uint32_t n, n_targets;
    float a[kSkinMaxTargets];  // the target weights
};
void launch_skin_pose(hipStream_t st, const SkinLaunch& L);

// "adaptive" pass (rt3_adaptive.hip).  Scratch, carved from the context's grow-only adaptive buffer: the per-pixel
// state in window space (index y * W + x, so that compacting the list moves nothing), two pixel lists that take turns (a list is the words
// x | y << 16 and, in the same order, k_pixbn's {xy, blue-noise word} records), and the compaction's per-block counts and result.
struct AdaptiveScratch {
    float4* sums;           // {sum r, sum g, sum b, n as uint32 bits}
    float2* mom;            // {S1, S2}
    uint8_t* mask;          // 1: the pixel's last test failed; 0 for everything that is not a listed foreground pixel of this rank
    uint32_t* xy[2];
    uint2* bn[2];
    uint32_t* block_count;  // one word per compaction block: its count, then its offset
    uint32_t* count;        // the length of the list the last compaction wrote
};
void adaptive_plan(uint32_t W, uint32_t H, uint32_t npix, BufLayout& plan, AdaptiveScratch* s);
constexpr uint32_t kAdaptiveTile = 2048;  // list entries per compaction block: s.block_count has one word per tile of the list
// self-test op 35: the compaction on a caller-made list; header words, then the mask bytes padded to whole words, then the records
constexpr uint32_t kSelftestCompactHeader = 4;
// foreground pixels of the rank's list: mask = 1 (s.mask zeroed for the whole window before); background ones: Moments = 0
void launch_adaptive_init(hipStream_t st, const uint32_t* pixels, uint32_t npix, uint32_t width, const float* depth, const AdaptiveScratch& s,
                          void* moments);
// k_accumulate's sums plus S1, S2 over the list's `sb` samples in lacc (path id = sample * npix + index); first: the pixels' first batch
void launch_adaptive_accumulate(hipStream_t st, const uint32_t* pixels, uint32_t npix, uint32_t width, const float* lacc, uint32_t sb, bool first,
                                uint32_t n_after, const AdaptiveScratch& s);
void launch_adaptive_test(hipStream_t st, const uint32_t* pixels, uint32_t npix, uint32_t width, float threshold, float dark,
                          const AdaptiveScratch& s);
// the entries of the n_in >= 1 records in_bn that stay active (mask, with the 3 x 3 rule if dilate) into s.xy[out] / s.bn[out], in order;
// their number into *s.count.  Three launches: count, scan, scatter.
void launch_adaptive_compact(hipStream_t st, const uint2* in_bn, uint32_t n_in, uint32_t W, uint32_t H, uint32_t dilate, const AdaptiveScratch& s,
                             int out);
void launch_adaptive_finalise(hipStream_t st, const uint32_t* pixels, uint32_t npix, uint32_t width, const float* depth, float blendfactor,
                              uint32_t cap, const AdaptiveScratch& s, void* light, const void* prev, void* moments);
// coverage mode (rt3_adaptive_set_coverage): the same for every listed pixel, whatever the G-buffer's depth says
void launch_adaptive_finalise_all(hipStream_t st, const uint32_t* pixels, uint32_t npix, uint32_t width, float blendfactor, uint32_t cap,
                                  const AdaptiveScratch& s, void* light, const void* prev, void* moments);

hipError_t lbvh_make_top(hipStream_t st, const float4* nodes, uint32_t n_nodes, DevBuf<float4>& top, uint32_t* n_top);

}  // namespace rt3
