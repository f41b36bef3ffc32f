// rt3_api.hip -- host layer + C ABI of librt3.so (include/rt3.h).
//
// One context = one GPU + one HIP stream.  It owns the world buffers (world/mod.rs:103-125), the LBVH
// (raytracing.rs:88-148), the name-less resource table with bindless-style handles (bindless/mod.rs:67-77) and the
// wavefront work queues.  rt3_pass_launch() is the drop-in for executing one pass node of the reference's frame graph
// (render_graph/mod.rs:80-107): the pass name selects a HIP kernel sequence instead of a SPIR-V pipeline.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/rt3.h"
#include "rt3_internal.hpp"

using namespace rt3;

static_assert(sizeof(rt3_gconst) == 304 && sizeof(GConstDev) == 304, "GConst is 304 bytes (renderer/mod.rs:47-63)");
static_assert(sizeof(rt3_geometry_info) == 64, "geometry info is 64 bytes");
static_assert(RT3_F_NEE_SKY == RT3_FLAG_NEE_SKY && RT3_F_BLUENOISE == RT3_FLAG_BLUENOISE && RT3_F_FACEFORWARD == RT3_FLAG_FACEFORWARD && RT3_F_SPECULAR == RT3_FLAG_SPECULAR && RT3_F_PROBE_RADIANCE == RT3_FLAG_PROBE_RADIANCE && RT3_F_NEE_EMISSIVE == RT3_FLAG_NEE_EMISSIVE, "flags");

namespace {

thread_local std::string g_create_error;
static const rt3_denoise_params kDenoiseDefaults = {5u, 7u, 0.05f, 4.0f, 0u};
static const rt3_temporal_params kTemporalDefaults = {0.2f, 0.2f, 32u, 0.9f, 0.01f, 0u};

struct Resource {
    uint32_t tag = 0;
    void* ptr = nullptr;    // mem.get(), or the caller's memory for rt3_image_import (never freed here)
    DevBuf<char> mem;
    size_t bytes = 0;
    uint32_t w = 0, h = 0, format = 0;
};
struct PixelList {
    uint32_t w, h, rank, n_ranks, count;
    DevBuf<uint32_t> dev;
    DevBuf<uint2> dev_bn;         // {x | y << 16, blue-noise word of that pixel}: one load instead of two dependent ones in k_shade
    uint64_t bn_stamp = ~0ull;    // which blue-noise upload dev_bn was built from
};
// Frame-end gather (north_star: "a single RCCL gather over xGMI at frame end").  The root receives every other rank's tiles
// into ONE contiguous buffer -- rank r's count[r] pixels at pixel offset off[r], ranks in ascending order, the root itself
// contributing nothing (its tiles are already in its image) -- and scatters all of them with ONE untile launch over `dev`,
// the concatenation of those ranks' pixel lists.
struct GatherLayout {
    uint32_t w, h, root, n_ranks;
    std::vector<uint64_t> off;  // n_ranks + 1 entries, in pixels
    DevBuf<uint32_t> dev;       // off[n_ranks] pixel words (x | y << 16)
};
enum Cat { CAT_EXTEND = 0, CAT_SHADOW = 1, CAT_SHADE = 2, CAT_OTHER = 3, CAT_GATHER = 4 };
struct Timed {
    hipEvent_t a, b;
    int cat;
};
struct CounterBlock {  // device counters of one refrence_mode launch, harvested lazily
    uint32_t first, n_pairs;  // n_pairs x {extension-queue size, shadow-queue size}: one 8-byte pair per bounce (k_shade bumps both with ONE 64-bit atomic)
    uint32_t emit_first = 0, n_emit = 0;  // RT3_F_NEE_EMISSIVE: n_emit emitter-shadow-queue sizes from emit_first (one per bounce)
};

// RT3_OPT_INSTANCE_MODE 1: what a build keeps for the next one.  The bottom trees live in the combined arrays
// (rt3_tlas.hip's layout); `meshes` says where, and they are reused while `gen` equals the context's scene generation.
struct TlMesh {
    uint32_t first, count;              // the geometry run
    uint32_t node_off, tri_off;         // in the combined arrays
    uint32_t n_nodes, n_tris, depth;
    double box[6];                      // the root's (quantised, conservative) object-space box
};
struct TlInstance {                     // one placement: the inverse of its matrix as the record holds it (fp32 values, in double)
    double A[3][3], b[3];
    double nA, nM;                      // row-sum norms of A and of the matrix's upper 3 x 3
    float m[16];                        // object -> world, column-major (rt3_instance::transform)
    uint32_t mesh, prim_base;           // mesh = ~0u: the instance places no triangles
    bool identity;
};
struct TwoLevelState {
    bool valid = false;                 // c->bvh holds a two-level structure whose bottom trees match `meshes`
    uint64_t gen = 0;
    uint32_t head = 0;                  // nodes before the first bottom tree: top capacity + 2 per instance
    uint32_t n_alloc_nodes = 0;         // nodes of the combined array
    std::vector<TlMesh> meshes;
    std::vector<TlInstance> inst;       // the instances of that build (a refit redoes their records and the top tree)
    uint32_t n_placed = 0, top_cap = 0; // of `inst`: those that place triangles (records, top-tree leaves); top-tree node capacity
    uint32_t n_meshes = 0, n_built = 0, n_top = 0;
    DevBuf<char> scratch;               // grow-only: the top build's inputs (tl_records_and_top)
};
// A bottom tree's geometry tables: the identity table of its geometries as uploaded, first_prim and prim_geom (local primitive ids), in one
// device allocation
struct MeshTables {
    DevBuf<char> mem;
    FlatGeomDev* geoms = nullptr;
    uint32_t *first_prim = nullptr, *prim_geom = nullptr;
};
// Shading records (k_tri_shade), per placed triangle in flattened order.  They depend on the flattening, the vertices and the indices, never
// on a tree or a matrix.  `key` = what they were made for: content_gen, then (geometry_first, geometry_count) of every placement; empty
// = nothing valid.
struct ShadeRecords {
    DevBuf<uint4> rec;
    DevBuf<float2> uv;
    uint32_t n = 0;  // records the buffers hold
    std::vector<uint64_t> key;
};

}  // namespace

struct rt3_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    char name[256] = {0};
    // scene
    DevBuf<float> d_verts;
    uint32_t n_verts = 0;
    DevBuf<uint32_t> d_indices;
    uint32_t n_indices = 0;
    DevBuf<FlatGeomDev> d_geoms;             // one entry per (instance, geometry): built by rt3_accel_build (flatten_world)
    DevBuf<ShadeGeomDev> d_shade_geoms;      // the same table as hit_info reads it
    uint32_t n_geoms = 0, n_prims = 0;       // uploaded geometries / their primitives (one instance of each)
    uint32_t n_flat_geoms = 0, n_flat_prims = 0;  // after flattening: what the acceleration structure and the shading records cover
    DevBuf<uint32_t> d_prim_geom, d_first_prim;
    std::vector<rt3_instance> h_instances;   // empty = one identity instance of every geometry
    uint64_t bulk_copies = 0;                // host <-> device copies of more than 64 KiB made by rt3_accel_build (rt3_stats.accel_bulk_copies)
    DevBuf<uint2> d_sky;  // 8-byte texels {RGB9E5, pdf_uv} in 4 x 4 tiles
    DevBuf<float> d_cdf_marg;
    DevBuf<uint32_t> d_sky_alias, d_guide_marg;
    uint32_t sky_w = 0, sky_h = 0, sky_wt = 0;
    DevBuf<uint8_t> d_bn;
    uint32_t bn_w = 0, bn_h = 0;
    uint64_t bn_stamp = 0;  // bumped by every rt3_scene_set_bluenoise
    // base-colour textures: host staging (RGBA8) + device atlas rebuilt lazily
    std::vector<std::vector<uint8_t>> h_tex;
    std::vector<uint32_t> tex_w, tex_h;
    DevBuf<uint8_t> d_tex_pixels;
    DevBuf<uint4> d_tex_table;
    DevBuf<float> d_srgb_lut;
    bool tex_dirty = false;
    LbvhResult bvh;
    ShadeRecords shade;
    DevBuf<char> build_scratch;  // grow-only: lbvh_build's scratch, kept from build to build
    bool accel_built = false;
    std::vector<uint32_t> h_indices;  // host copies, only for range validation (rt3_scene_set_geometry, again in rt3_accel_build)
    std::vector<rt3_geometry_info> h_geoms;
    std::vector<uint32_t> h_prim_counts;
    int64_t max_tex_index = -1;
    // alpha masks: cutoff per uploaded geometry (empty = all 0, opaque); the tables of the last rt3_accel_build:
    // d_geom_mask per uploaded geometry {cutoff bits, slot}, d_alpha per masked geometry {texture index, base_color[3] bits}
    std::vector<float> h_cutoffs;
    DevBuf<uint2> d_geom_mask, d_alpha;
    bool accel_masked = false;  // the structure holds masked triangles: traversal launches run the MASK kernels
    // resources.  A Resource* / PixelList* holds until the next push_back; the device memory they own never moves
    std::vector<Resource> resources;
    std::vector<PixelList> pixlists;
    std::vector<GatherLayout> gather_layouts;
    uint32_t rank = 0, n_ranks = 1, part_w = 0, part_h = 0;
    // communicator of the frame-end gather (RCCL): one rank per context / GPU / process
    ncclComm_t comm = nullptr;
    uint32_t comm_rank = 0, comm_size = 0;
    DevBuf<char> gather_buf;  // grow-only; non-root: this rank's packed tiles; root: the receive buffer of all other ranks' tiles
    // work queues (capacity in paths)
    size_t cap = 0, cap_pix = 0;
    DevBuf<float> rays[2], hits, T[2];
    DevBuf<float> sh_rays, sh_contrib, lacc, radsum;
    DevBuf<float> sh2_rays, sh2_contrib, sh2_tmax;  // RT3_F_NEE_EMISSIVE: the emitter shadow queue, allocated when the flag is first used
    size_t cap_emit = 0;
    DevBuf<uint32_t> d_counters;
    uint32_t counters_cap = 1 << 16, counters_next = 0;
    DevBuf<unsigned long long> d_totals;  // counting mode: kTotWords words (TotalsWord)
    std::vector<CounterBlock> pending_counters;
    // options / stats
    int64_t opt_batch_spp = 0;
    bool opt_profile = false, opt_count = false;
    int opt_variant = 0;  // RT3_OPT_EXTEND_VARIANT: reserved for traversal experiments
    uint32_t opt_leaf_size = 2, opt_node_width = 4, opt_node_quant = 1, opt_collapse = 2, opt_sah_top = 1;
    int opt_instance_mode = 0;  // RT3_OPT_INSTANCE_MODE: 0 flatten, 1 two-level
    // generations: topo_gen is bumped by everything a tree's shape depends on (vertex count, indices, geometry, leaf size, layout, collapse,
    // SAH top); content_gen by all of that and by rt3_scene_update_vertices too.  A refit needs the topology of the build it updates; the
    // two-level structure keeps its bottom trees while the content is what they were built (or refitted) for
    uint64_t topo_gen = 1, content_gen = 1;
    uint64_t accel_topo_gen = 0;  // topo_gen of the last successful rt3_accel_build
    bool accel_stale = false;     // vertices updated since the structure was built or refitted: nothing traces it until a refit or build
    uint64_t accel_stamp = 0;     // bumped by every successful rt3_accel_build / rt3_accel_refit / rt3_accel_import
    LightTable lights;            // RT3_F_NEE_EMISSIVE: built lazily for accel_stamp (ensure_lights)
    // refit plans (rt3_refit.hip), made on the first refit after a build or import: one per tree (instance mode 1: one per bottom tree)
    bool refit_planned = false;
    std::vector<RefitTree> refit_trees;
    std::vector<MeshTables> refit_tables;    // instance mode 1: each bottom tree's (tl_build_mesh's)
    DevBuf<char> refit_scratch;              // grow-only: refit_tree's bounds, node boxes and record boxes
    TwoLevelState tl;
    // "denoise" pass: parameters (rt3_denoise_set_params) and the grow-only scratch its records are carved from
    rt3_denoise_params dn_params = kDenoiseDefaults;
    DevBuf<char> dn_scratch;
    uint32_t dn_variance_image = 0;  // rt3_denoise_set_variance_input: the "temporal" pass's Moments image, 0 = none
    // "temporal" pass: parameters (rt3_temporal_set_params) and the previous frame's GConst (rt3_temporal_set_prev_view)
    rt3_temporal_params tp_params = kTemporalDefaults;
    rt3_gconst tp_prev;
    bool tp_has_prev = false;
    uint32_t tp_motion_image = 0;  // rt3_temporal_set_motion_input: the "motion" pass's image, 0 = none
    // "motion" pass: the previous frame's instance matrices (rt3_scene_set_prev_transforms; empty = every instance unmoved) and the device
    // tables made from them for the structure of accel_stamp mo_stamp (motion_tables)
    std::vector<float> mo_prev;  // n x 16, column-major
    bool mo_dirty = false, mo_any_moved = false;
    uint64_t mo_stamp = 0;
    DevBuf<MotionPrevDev> d_mo_prev;
    DevBuf<uint32_t> d_mo_slot;
    bool mo_any_deformed = false;
    // deformation: the snapshot of rt3_scene_snapshot_vertices, one {x, y, z, 0} per vertex; the vertex ranges
    // rt3_scene_update_vertices touched since it, sorted and merged; per uploaded geometry its vertex span [lo, hi] (lo > hi: no triangle)
    // and, once deform_flags has run, whether some position word inside the span differs from the snapshot
    DevBuf<float4> d_prev_pos;
    bool df_snapshot = false, df_dirty = false;
    std::vector<std::pair<uint32_t, uint32_t>> df_ranges;  // [first, end)
    std::vector<std::pair<uint32_t, uint32_t>> h_geom_span;
    std::vector<uint32_t> h_deformed;
    DevBuf<uint32_t> d_deformed;
    DevBuf<uint4> d_df_chunks;
    rt3_stats stats;
    uint64_t primary_rays_pending = 0;
    std::vector<Timed> pending_events;
    std::vector<Timed> free_events;
};

static int ensure_lights(rt3_ctx* c);
static int motion_tables(rt3_ctx* c);
static int deform_flags(rt3_ctx* c);

namespace {

int fail(rt3_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    else g_create_error = msg;
    return code;
}
#define HIPC(ctx, call)                                                                                              \
    do {                                                                                                             \
        hipError_t e_ = (call);                                                                                      \
        if (e_ != hipSuccess) return fail(ctx, RT3_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));        \
    } while (0)

template <typename T>
int dev_alloc(rt3_ctx* c, DevBuf<T>& b, size_t count) {
    HIPC(c, b.alloc_bytes((count ? count : 1) * sizeof(T)));
    return RT3_OK;
}

uint32_t spread1by1(uint32_t x) {  // math.slang:105-112 integer_explode
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}
uint32_t zcurve_host(uint32_t x, uint32_t y) { return spread1by1(x) | (spread1by1(y) << 1); }  // math.slang:114-117
uint32_t compact1by1(uint32_t x) {
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    x = (x | (x >> 8)) & 0x0000FFFFu;
    return x;
}
// 64x64 tiles, Z-order over the tile grid, tile i -> rank i % n_ranks; Z-order inside a tile (primary-ray coherence)
void tile_pixels(uint32_t w, uint32_t h, uint32_t rank, uint32_t n_ranks, std::vector<uint32_t>& out) {
    out.clear();
    uint32_t tw = (w + 63) / 64, th = (h + 63) / 64, side = 1, tile_no = 0;
    while (side < tw || side < th) side *= 2;
    for (uint32_t z = 0; z < side * side; z++) {
        uint32_t tx = compact1by1(z), ty = compact1by1(z >> 1);
        if (tx >= tw || ty >= th) continue;
        uint32_t owner = tile_no++ % n_ranks;
        if (owner != rank) continue;
        for (uint32_t k = 0; k < 4096; k++) {
            uint32_t x = tx * 64 + compact1by1(k), y = ty * 64 + compact1by1(k >> 1);
            if (x < w && y < h) out.push_back(x | (y << 16));
        }
    }
}
int get_pixlist(rt3_ctx* c, uint32_t w, uint32_t h, uint32_t rank, uint32_t n_ranks, PixelList** out) {
    for (auto& p : c->pixlists)
        if (p.w == w && p.h == h && p.rank == rank && p.n_ranks == n_ranks) {
            *out = &p;
            return RT3_OK;
        }
    if (w == 0 || h == 0 || w > 65535 || h > 65535 || n_ranks == 0 || rank >= n_ranks) return fail(c, RT3_E_INVALID, "bad window / rank for tile partition");
    std::vector<uint32_t> px;
    tile_pixels(w, h, rank, n_ranks, px);
    PixelList pl;
    pl.w = w; pl.h = h; pl.rank = rank; pl.n_ranks = n_ranks; pl.count = (uint32_t)px.size();
    HIPC(c, pl.dev.alloc_bytes((px.size() ? px.size() : 1) * 4));
    if (!px.empty()) HIPC(c, hipMemcpy(pl.dev.get(), px.data(), px.size() * 4, hipMemcpyHostToDevice));
    c->pixlists.push_back(std::move(pl));
    *out = &c->pixlists.back();
    return RT3_OK;
}

Resource* get_res(rt3_ctx* c, uint32_t handle, uint32_t want_tag) {
    uint32_t tag = handle >> 30, idx = handle & 0x3FFFFFFFu;
    if (tag != want_tag || idx >= c->resources.size()) return nullptr;
    Resource* r = &c->resources[idx];
    return r->tag == want_tag && r->ptr ? r : nullptr;
}
size_t format_bytes(uint32_t f) {
    switch (f) {
        case RT3_FORMAT_R32_SFLOAT: return 4;
        case RT3_FORMAT_R32G32B32A32_SFLOAT: return 16;
        case RT3_FORMAT_R32G32B32A32_UINT: return 16;
        case RT3_FORMAT_R8G8B8A8_UNORM: return 4;
        case RT3_FORMAT_R16_UINT: return 2;
        default: return 0;
    }
}

SceneDev scene_dev(const rt3_ctx* c) {
    SceneDev s;
    s.verts = c->d_verts.get();
    s.indices = c->d_indices.get();
    s.geoms = c->d_geoms.get();
    s.shade_geoms = c->d_shade_geoms.get();
    s.n_geoms = c->n_flat_geoms;
    s.prim_geom = c->d_prim_geom.get();
    s.first_prim = c->d_first_prim.get();
    s.tri_shade = c->shade.rec.get();
    s.tri_uv = c->shade.uv.get();
    s.guide_marg = c->d_guide_marg.get();
    s.sky = c->d_sky.get();
    s.sky_alias = c->d_sky_alias.get();
    s.cdf_marg = c->d_cdf_marg.get();
    s.sky_w = c->sky_w;
    s.sky_h = c->sky_h;
    s.sky_wt = c->sky_wt;
    s.bluenoise = c->d_bn.get();
    s.bn_w = c->bn_w;
    s.bn_h = c->bn_h;
    s.tex_pixels = c->d_tex_pixels.get();
    s.tex_table = c->d_tex_table.get();
    s.srgb_lut = c->d_srgb_lut.get();
    s.n_tex = c->d_tex_pixels ? (uint32_t)c->h_tex.size() : 0u;
    return s;
}

// the geometry tables of the flattened world ...
GeomTables world_tables(const rt3_ctx* c) { return {c->d_verts.get(), c->d_indices.get(), c->d_geoms.get(), c->d_prim_geom.get(), c->d_first_prim.get()}; }
// ... and of a bottom tree: the world's vertices and indices, read through the tree's own tables
GeomTables mesh_tables(const rt3_ctx* c, const MeshTables& t) { return {c->d_verts.get(), c->d_indices.get(), t.geoms, t.prim_geom, t.first_prim}; }

// a change every tree's shape depends on: the structure goes, and a refit cannot bring it back
void invalidate_topology(rt3_ctx* c) {
    c->accel_built = false;
    c->topo_gen++;
    c->content_gen++;
}
// RT3_OK when the structure may be traced: built, and no vertex updated since
int check_accel_current(rt3_ctx* c, const char* unbuilt = "rt3_accel_build has not been called for the current scene") {
    if (!c || !c->accel_built) return fail(c, RT3_E_STATE, unbuilt);
    if (c->accel_stale) return fail(c, RT3_E_STATE, "vertices were updated since the acceleration structure was built: rt3_accel_refit or rt3_accel_build first");
    return RT3_OK;
}

// (re)build the device texture atlas after rt3_scene_set_texture calls
int sync_textures(rt3_ctx* c) {
    if (!c->tex_dirty) return RT3_OK;
    std::vector<uint4> table(c->h_tex.size());
    size_t total = 0;
    for (size_t i = 0; i < c->h_tex.size(); i++) {
        if (c->h_tex[i].empty()) return fail(c, RT3_E_STATE, "texture " + std::to_string(i) + " was never set (indices must be dense)");
        table[i] = make_uint4((uint32_t)total, c->tex_w[i], c->tex_h[i], 0u);
        total += c->h_tex[i].size();
    }
    if (total > 0xFFFFFFF0ull) return fail(c, RT3_E_INVALID, "textures exceed 4 GiB");
    std::vector<uint8_t> all(total);
    for (size_t i = 0; i < c->h_tex.size(); i++) memcpy(all.data() + table[i].x, c->h_tex[i].data(), c->h_tex[i].size());
    if (int r = dev_alloc(c, c->d_tex_pixels, total)) return r;
    if (int r = dev_alloc(c, c->d_tex_table, table.size())) return r;
    HIPC(c, hipMemcpy(c->d_tex_pixels.get(), all.data(), total, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->d_tex_table.get(), table.data(), table.size() * sizeof(uint4), hipMemcpyHostToDevice));
    if (!c->d_srgb_lut) {
        float lut[256];
        for (int i = 0; i < 256; i++) {  // sRGB EOTF (IEC 61966-2-1), evaluated in double
            double v = i / 255.0;
            lut[i] = (float)(v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4));
        }
        if (int r = dev_alloc(c, c->d_srgb_lut, (size_t)256)) return r;
        HIPC(c, hipMemcpy(c->d_srgb_lut.get(), lut, sizeof(lut), hipMemcpyHostToDevice));
    }
    c->tex_dirty = false;
    return RT3_OK;
}

// Failure-atomic: if any allocation fails the whole queue set is released and the capacities drop to 0, so the next pass
// re-allocates (or reports the error again) instead of launching kernels on a half-resized set.
void free_work(rt3_ctx* c) {
    for (int k = 0; k < 2; k++) { c->rays[k].reset(); c->T[k].reset(); }
    c->hits.reset(); c->sh_rays.reset(); c->sh_contrib.reset(); c->lacc.reset(); c->radsum.reset();
    c->sh2_rays.reset(); c->sh2_contrib.reset(); c->sh2_tmax.reset();
    c->cap_emit = 0;
    c->cap = 0;
    c->cap_pix = 0;
}
int ensure_work(rt3_ctx* c, size_t paths, size_t npix) {
    int r = RT3_OK;
    if (paths > c->cap) {
        size_t P = (paths + 255) & ~(size_t)255;
        c->cap = 0;
        for (int k = 0; k < 2 && !r; k++) {
            if (!r) r = dev_alloc(c, c->rays[k], 8 * P);
            if (!r) r = dev_alloc(c, c->T[k], 3 * P);  // throughput planes (the path's pdf and id ride in the ray records)
        }
        if (!r) r = dev_alloc(c, c->hits, 4 * P);
        if (!r) r = dev_alloc(c, c->sh_rays, 8 * P);
        if (!r) r = dev_alloc(c, c->sh_contrib, 2 * P);  // {blue contribution, path id} records (red / green ride with the ray)
        if (!r) r = dev_alloc(c, c->lacc, 4 * P);        // float4 per path
        if (!r) c->cap = P;
    }
    if (!r && npix > c->cap_pix) {
        c->cap_pix = 0;
        r = dev_alloc(c, c->radsum, 3 * npix);
        if (!r) c->cap_pix = npix;
    }
    if (r) free_work(c);
    return r;
}
// the emitter shadow queue, as large as the other queues (after ensure_work)
int ensure_emit_queue(rt3_ctx* c) {
    if (c->cap_emit >= c->cap) return RT3_OK;
    c->cap_emit = 0;
    int r = dev_alloc(c, c->sh2_rays, 8 * c->cap);
    if (!r) r = dev_alloc(c, c->sh2_contrib, 2 * c->cap);
    if (!r) r = dev_alloc(c, c->sh2_tmax, c->cap);
    if (!r) c->cap_emit = c->cap;
    else free_work(c);
    return r;
}

int harvest(rt3_ctx* c) {  // stream must be idle
    if (!c->pending_counters.empty()) {
        std::vector<uint32_t> h(c->counters_next);
        HIPC(c, hipMemcpy(h.data(), c->d_counters.get(), (size_t)c->counters_next * 4, hipMemcpyDeviceToHost));
        for (auto& b : c->pending_counters) {
            for (uint32_t k = 0; k < b.n_pairs; k++) {
                c->stats.extension_rays += h[b.first + 2 * k];
                c->stats.shadow_rays += h[b.first + 2 * k + 1];
            }
            for (uint32_t k = 0; k < b.n_emit; k++) c->stats.shadow_rays += h[b.emit_first + k];
        }
        c->pending_counters.clear();
    }
    c->counters_next = 0;
    c->stats.extension_rays += c->primary_rays_pending;
    c->primary_rays_pending = 0;
    if (c->opt_count) {
        unsigned long long t[kTotWords] = {};
        HIPC(c, hipMemcpy(t, c->d_totals.get(), sizeof(t), hipMemcpyDeviceToHost));
        c->stats.nodes_visited += t[kTotExtendNodes];
        c->stats.tris_tested += t[kTotExtendTris];
        c->stats.shadow_nodes_visited += t[kTotShadowNodes];
        c->stats.shadow_tris_tested += t[kTotShadowTris];
        c->stats.nodes_visited_lds += t[kTotExtendLds];
        c->stats.shadow_nodes_visited_lds += t[kTotShadowLds];
        HIPC(c, hipMemset(c->d_totals.get(), 0, sizeof(t)));
    }
    for (auto& t : c->pending_events) {
        float ms = 0.0f;
        HIPC(c, hipEventElapsedTime(&ms, t.a, t.b));
        switch (t.cat) {
            case CAT_EXTEND: c->stats.extend_ms += ms; c->stats.extend_launches++; break;
            case CAT_SHADOW: c->stats.shadow_ms += ms; c->stats.shadow_launches++; break;
            case CAT_SHADE: c->stats.shade_ms += ms; break;
            case CAT_GATHER: c->stats.gather_ms += ms; break;
            default: c->stats.other_ms += ms; break;
        }
        c->free_events.push_back(t);
    }
    c->pending_events.clear();
    return RT3_OK;
}

struct ScopedTimer {  // brackets one kernel launch with HIP events on the context's stream when profiling is on
    rt3_ctx* c;
    Timed t;
    bool on;
    ScopedTimer(rt3_ctx* ctx, int cat) : c(ctx), on(ctx->opt_profile) {
        if (!on) return;
        if (!c->free_events.empty()) {
            t = c->free_events.back();
            c->free_events.pop_back();
        } else if (hipEventCreate(&t.a) != hipSuccess || hipEventCreate(&t.b) != hipSuccess) {
            on = false;
            return;
        }
        t.cat = cat;
        (void)hipEventRecord(t.a, c->stream);
    }
    ~ScopedTimer() {
        if (!on) return;
        (void)hipEventRecord(t.b, c->stream);
        c->pending_events.push_back(t);
    }
};

int reserve_counters(rt3_ctx* c, uint32_t n, uint32_t* first) {
    if (c->counters_next + n > c->counters_cap) {
        HIPC(c, hipStreamSynchronize(c->stream));
        if (int r = harvest(c)) return r;
    }
    if (n > c->counters_cap) return fail(c, RT3_E_INVALID, "too many bounces x batches for the counter block");
    *first = c->counters_next;
    c->counters_next += n;
    HIPC(c, hipMemsetAsync(c->d_counters.get() + *first, 0, (size_t)n * 4, c->stream));
    return RT3_OK;
}
// the alpha-mask tables of a traversal launch over the current structure: empty (table null) without masked triangles.  The texture atlas
// must be synchronised (sync_textures) first.
AlphaDev alpha_dev(const rt3_ctx* c) {
    AlphaDev a = {};
    if (!c->accel_masked) return a;
    a.table = c->d_alpha.get();
    a.tri_uv = c->shade.uv.get();
    a.tex_table = c->d_tex_table.get();
    a.tex_pixels = c->d_tex_pixels.get();
    a.n_tex = c->d_tex_pixels ? (uint32_t)c->h_tex.size() : 0u;
    return a;
}
// a traversal launch over the context's queues (`stride` records), counting into its totals when RT3_OPT_COUNT_TRAVERSAL is on
TraceLaunch ctx_trace(rt3_ctx* c) {
    TraceLaunch L;
    L.stride = c->cap;
    L.count = c->opt_count;
    L.totals = c->opt_count ? c->d_totals.get() : nullptr;
    L.alpha = alpha_dev(c);
    return L;
}
// closest hits of the n primary rays in c->rays[0], into c->hits
int trace_primary(rt3_ctx* c, uint32_t n) {
    uint32_t wc_slot;
    if (int r = reserve_counters(c, 1, &wc_slot)) return r;  // ray-pool cursor of the launch
    TraceLaunch L = ctx_trace(c);
    L.rays = c->rays[0].get(); L.n = n; L.work_counter = c->d_counters.get() + wc_slot; L.hits = c->hits.get();
    c->primary_rays_pending += n;
    ScopedTimer t(c, CAT_EXTEND);
    launch_extend(c->stream, c->bvh, L);
    return RT3_OK;
}

// ---------------------------------------------------------------------------------------------- passes
// A pass is one entry of kPasses (below): launch_pass checks the launch against the entry and hands the pass function (pass_*) the window
// and the resolved bindings, in the entry's order.  What a pass function still checks is its own: context state, the least size of a
// buffer, the optional context-state inputs.
GConstDev gconst_dev(const rt3_gconst* g) {
    GConstDev gd;
    memcpy(&gd, g, sizeof(gd));
    return gd;
}
int check_window(rt3_ctx* c, const rt3_gconst* g, uint32_t* W, uint32_t* H) {
    float fw = g->window_size[0], fh = g->window_size[1];
    if (!(fw >= 1.0f && fh >= 1.0f && fw <= 65535.0f && fh <= 65535.0f) || fw != std::floor(fw) || fh != std::floor(fh))
        return fail(c, RT3_E_INVALID, "GConst.window_size must hold integral pixel counts in [1, 65535]");
    *W = (uint32_t)fw;
    *H = (uint32_t)fh;
    return RT3_OK;
}
Resource* image_checked(rt3_ctx* c, uint32_t handle, uint32_t W, uint32_t H, uint32_t format, const char* what) {
    Resource* r = get_res(c, handle, RT3_TAG_IMAGE);
    if (!r || r->w != W || r->h != H || r->format != format) {
        c->err = std::string("binding '") + what + "' is not a " + std::to_string(W) + "x" + std::to_string(H) + " image of the expected format";
        return nullptr;
    }
    return r;
}
int buffer_at_least(rt3_ctx* c, const Resource* r, size_t need, const char* what) {
    if (r->bytes >= need) return RT3_OK;
    return fail(c, RT3_E_INVALID, std::string("binding '") + what + "' must be a buffer of at least " + std::to_string(need) + " bytes");
}
// The primary rays of this rank's pixels of the W x H window (*out: the list) into c->rays[0], their closest hits into c->hits, in the
// list's order.  An empty list: nothing is allocated, nothing enqueued.
int primary_hits(rt3_ctx* c, const GConstDev& gd, uint32_t W, uint32_t H, PixelList** out) {
    if (int r = get_pixlist(c, W, H, c->rank, c->n_ranks, out)) return r;
    const PixelList* pl = *out;
    if (pl->count == 0) return RT3_OK;
    if (int r = ensure_work(c, pl->count, pl->count)) return r;
    {
        ScopedTimer t(c, CAT_OTHER);
        launch_raygen(c->stream, gd, pl->dev.get(), pl->count, c->rays[0].get(), c->cap);
    }
    return trace_primary(c, pl->count);
}

// gbuffer.slang:8-21
int pass_gbuffer(rt3_ctx* c, const rt3_gconst* g, uint32_t W, uint32_t H, Resource* const* res) {
    PixelList* pl;
    if (int r = primary_hits(c, gconst_dev(g), W, H, &pl)) return r;
    if (pl->count == 0) return RT3_OK;
    {
        ScopedTimer t(c, CAT_OTHER);
        launch_gbuffer(c->stream, scene_dev(c), pl->dev.get(), pl->count, W, c->hits.get(), c->cap, res[0]->ptr, (float*)res[1]->ptr);
    }
    HIPC(c, hipGetLastError());
    return RT3_OK;
}

// refrence_mode.slang:14-66 as a wavefront loop
int pass_reference_mode(rt3_ctx* c, const rt3_gconst* g, uint32_t W, uint32_t H, Resource* const* res) {
    const Resource *gb = res[0], *dp = res[1], *li = res[2], *pv = res[3];
    const uint32_t Sspp = g->samples, B = g->bounces;
    if (Sspp == 0 || B == 0) return RT3_OK;  // GConst::default() leaves samples = bounces = 0 (renderer/mod.rs:47-63): nothing to trace
    if (B > 64) return fail(c, RT3_E_INVALID, "bounces > 64");
    PixelList* pl;
    if (int r = get_pixlist(c, W, H, c->rank, c->n_ranks, &pl)) return r;
    const uint32_t npix = pl->count;
    if (npix == 0) return RT3_OK;
    if (pl->bn_stamp != c->bn_stamp || !pl->dev_bn) {  // (re)build the {pixel, blue-noise word} list of this window / rank
        if (!pl->dev_bn) HIPC(c, pl->dev_bn.alloc_bytes((size_t)npix * 8));
        launch_pixbn(c->stream, pl->dev.get(), npix, c->d_bn.get(), c->bn_w, c->bn_h, pl->dev_bn.get());
        pl->bn_stamp = c->bn_stamp;
    }
    // paths per wavefront batch: 160 B of queue state each, so 2^28 paths = 43 GB of the 288 GB; the C3 frame (132.7 M paths)
    // is ONE batch.  Larger launches amortise the ramp / tail of the persistent traversal kernels: 16 -> 64 spp per batch = -6.5 % frame time.
    uint64_t max_paths = 1ull << 28;
    uint32_t sb = c->opt_batch_spp > 0 ? (uint32_t)c->opt_batch_spp : (uint32_t)std::max<uint64_t>(1, max_paths / npix);
    if (sb > Sspp) sb = Sspp;
    if ((uint64_t)sb * npix > 0xFFFFFF00ull) return fail(c, RT3_E_INVALID, "batch too large");
    if (int r = ensure_work(c, (size_t)sb * npix, npix)) return r;
    const size_t S = c->cap;
    const GConstDev gd = gconst_dev(g);
    const bool nee = (g->pad[0] & RT3_F_NEE_SKY) && c->d_sky;
    // RT3_F_NEE_EMISSIVE: only with something to sample; otherwise the frame is the flag-less one, same kernels
    // (and B >= 2: emitter shadow rays leave vertices 0 .. B-2)
    LightsDev lights{};
    if ((g->pad[0] & RT3_F_NEE_EMISSIVE) && B > 1) {
        if (int r = ensure_lights(c)) return r;
        lights = c->lights.dev();
        if (lights.n)
            if (int r = ensure_emit_queue(c)) return r;
    }
    const bool nee_e = lights.n != 0u;
    SceneDev sc = scene_dev(c);
    for (uint32_t s0 = 0; s0 < Sspp; s0 += sb) {
        const uint32_t nsb = std::min(sb, Sspp - s0);
        const uint32_t n_first = nsb * npix;
        uint32_t first;
        if (int r = reserve_counters(c, (nee_e ? 6 : 4) * B + 1, &first)) return r;
        first += first & 1u;  // 8-byte aligned pairs
        // pair b = {extension rays emitted at bounce b (b < B-1), shadow rays emitted at bounce b}; then the ray-pool cursors
        uint32_t* pairs = c->d_counters.get() + first;
        uint32_t* pool_cur = c->d_counters.get() + first + 2 * B;  // [b], [B + b]: ray-pool cursors of the k_extend / k_shadow launch of bounce b
        // with emitter NEE: [4B + b] emitter shadow rays emitted at bounce b, [5B + b] the ray-pool cursor of their k_shadow launch
        uint32_t* emit_cnt = c->d_counters.get() + first + 4 * B;
        c->pending_counters.push_back(CounterBlock{first, B, first + 4 * B, nee_e ? B : 0u});
        auto ext_cnt_at = [pairs](uint32_t b) { return pairs + 2 * b; };
        auto sh_cnt_at = [pairs](uint32_t b) { return pairs + 2 * b + 1; };
        int cur = 0;
        for (uint32_t bn = 0; bn < B; bn++) {
            ShadeLaunch L;
            L.g = gd; L.sc = sc; L.pixels = pl->dev.get(); L.pixbn = pl->dev_bn.get(); L.npix = npix; L.width = W; L.s0 = s0; L.bounce = bn;
            L.gbuffer = (const uint4*)gb->ptr; L.depth = (const float*)dp->ptr;
            L.in_rays = c->rays[cur].get(); L.in_hits = c->hits.get(); L.in_T = c->T[cur].get();
            L.in_count = bn ? ext_cnt_at(bn - 1) : nullptr; L.n_first = n_first;
            L.out_rays = c->rays[cur ^ 1].get(); L.out_T = c->T[cur ^ 1].get(); L.out_count = ext_cnt_at(bn);
            L.sh_rays = c->sh_rays.get(); L.sh_contrib = c->sh_contrib.get(); L.sh_count = sh_cnt_at(bn);
            L.lacc = c->lacc.get(); L.stride = S;
            L.lights = lights;
            L.sh2_rays = c->sh2_rays.get(); L.sh2_contrib = c->sh2_contrib.get(); L.sh2_tmax = c->sh2_tmax.get(); L.sh2_count = emit_cnt + bn;
            {
                ScopedTimer t(c, CAT_SHADE);
                launch_shade(c->stream, bn == 0, L);
            }
            cur ^= 1;
            if (nee) {
                TraceLaunch tr = ctx_trace(c);
                tr.rays = c->sh_rays.get(); tr.count_ptr = sh_cnt_at(bn); tr.n = n_first; tr.work_counter = pool_cur + B + bn;
                tr.contrib = c->sh_contrib.get(); tr.lacc = c->lacc.get();
                ScopedTimer t(c, CAT_SHADOW);
                launch_shadow(c->stream, c->bvh, tr);
            }
            if (nee_e && bn + 1 < B) {  // after the sky's: the two add into the same radiance slots, one launch after the other
                TraceLaunch tr = ctx_trace(c);
                tr.rays = c->sh2_rays.get(); tr.count_ptr = emit_cnt + bn; tr.n = n_first; tr.work_counter = emit_cnt + B + bn;
                tr.contrib = c->sh2_contrib.get(); tr.lacc = c->lacc.get(); tr.tmax = c->sh2_tmax.get();
                ScopedTimer t(c, CAT_SHADOW);
                launch_shadow(c->stream, c->bvh, tr);
            }
            if (bn != B - 1) {
                TraceLaunch tr = ctx_trace(c);
                tr.rays = c->rays[cur].get(); tr.count_ptr = ext_cnt_at(bn); tr.n = n_first; tr.work_counter = pool_cur + bn;
                tr.hits = c->hits.get(); tr.payload = true;
                ScopedTimer t(c, CAT_EXTEND);
                launch_extend(c->stream, c->bvh, tr);
            }
        }
        {
            ScopedTimer t(c, CAT_OTHER);
            launch_accumulate(c->stream, gd, pl->dev.get(), npix, W, (const float*)dp->ptr, c->lacc.get(), S, nsb, s0 == 0, s0 + nsb >= Sspp, c->radsum.get(), li->ptr,
                              pv->ptr);
        }
    }
    HIPC(c, hipGetLastError());
    return RT3_OK;
}

// postprocess.slang:90-112
int pass_postprocess(rt3_ctx* c, const rt3_gconst* g, uint32_t W, uint32_t H, Resource* const* res) {
    const Resource *dp = res[0], *out = res[1], *in = res[2];
    PixelList* pl;
    if (int r = get_pixlist(c, W, H, c->rank, c->n_ranks, &pl)) return r;
    if (pl->count == 0) return RT3_OK;
    ScopedTimer t(c, CAT_OTHER);
    launch_postprocess(c->stream, gconst_dev(g), scene_dev(c), pl->dev.get(), pl->count, W, (const float*)dp->ptr, in->ptr, out->ptr);
    HIPC(c, hipGetLastError());
    return RT3_OK;
}

// ---- probe-GI passes.  A probe owns a 16x16 pixel block and an 8x8-texel cell of the probe atlas; the passes
//      run on the whole window on every rank (they are not part of the tile-partitioned path).  The probe grid is the atlas binding's
//      size over 8.
// structured_importance_sampling.slang:7-11 : set 1 {gbuffer, gbuffer_depth, out, debug}, set 2 {probe_atlas}
int pass_sis(rt3_ctx* c, const rt3_gconst*, uint32_t W, uint32_t, Resource* const* res) {
    ScopedTimer t(c, CAT_OTHER);
    launch_sis(c->stream, W, res[4]->w / 8, res[4]->h / 8, res[0]->ptr, res[2]->ptr, (float*)res[3]->ptr);
    HIPC(c, hipGetLastError());
    return RT3_OK;
}
// trace_probes.slang:8-12 : set 1 {gbuffer, gbuffer_depth, directions}, set 2 {probe_atlas}, set 3 {prev_probe_atlas}
int pass_trace_probes(rt3_ctx* c, const rt3_gconst* g, uint32_t W, uint32_t, Resource* const* res) {
    const Resource *dp = res[1], *dir = res[2], *at = res[3], *pv = res[4];
    const uint32_t px = at->w / 8, py = at->h / 8, n = at->w * at->h;
    if (int r = ensure_work(c, n, 0)) return r;
    const size_t S = c->cap;
    {
        ScopedTimer t(c, CAT_OTHER);
        launch_probe_raygen(c->stream, gconst_dev(g), W, px, py, (const float*)dp->ptr, dir->ptr, at->ptr, c->rays[0].get(), S, c->T[0].get());
    }
    if (int r = trace_primary(c, n)) return r;
    {
        ScopedTimer t(c, CAT_OTHER);
        launch_probe_store(c->stream, scene_dev(c), g->pad[0], g->blendfactor, px, py, c->hits.get(), c->T[0].get(), pv->ptr, at->ptr);
    }
    HIPC(c, hipGetLastError());
    return RT3_OK;
}
// spherical_harmonic_conversion.slang:6-7 : set 0 {out}, set 1 {probe_atlas}
int pass_sh_conversion(rt3_ctx* c, const rt3_gconst*, uint32_t, uint32_t, Resource* const* res) {
    const Resource *out = res[0], *at = res[1];
    const uint32_t px = at->w / 8, py = at->h / 8;
    // float3x3 elements at Z-curve indices (:30-32)
    if (int r = buffer_at_least(c, out, ((size_t)zcurve_host(px * 3 - 1, py - 1) + 1) * 48, "out")) return r;
    ScopedTimer t(c, CAT_OTHER);
    launch_sh_conversion(c->stream, px, py, at->ptr, out->ptr);
    HIPC(c, hipGetLastError());
    return RT3_OK;
}
// interpolate_probes.slang:6-9 : set 1 {gbuffer, gbuffer_depth, sh_coeficents}, set 2 {Light}
int pass_interpolate_probes(rt3_ctx* c, const rt3_gconst* g, uint32_t W, uint32_t H, Resource* const* res) {
    const Resource *gb = res[0], *dp = res[1], *sh = res[2], *li = res[3];
    const uint32_t npx = W / 16, npy = H / 16;
    if (int r = buffer_at_least(c, sh, npx && npy ? ((size_t)zcurve_host(npx * 3 - 1, npy - 1) + 1) * 48 : 0, "sh_coeficents")) return r;
    ScopedTimer t(c, CAT_OTHER);
    launch_interpolate(c->stream, gconst_dev(g), W, H, gb->ptr, (const float*)dp->ptr, sh->ptr, li->ptr);
    HIPC(c, hipGetLastError());
    return RT3_OK;
}

// "denoise": edge-avoiding a-trous filter over the whole window (no reference counterpart)
int pass_denoise(rt3_ctx* c, const rt3_gconst* g, uint32_t W, uint32_t H, Resource* const* res) {
    const Resource *gb = res[0], *dp = res[1], *in = res[2], *out = res[3];
    const Resource* mo = nullptr;
    if (c->dn_variance_image) {
        mo = image_checked(c, c->dn_variance_image, W, H, RT3_FORMAT_R32G32B32A32_SFLOAT, "variance input");
        if (!mo) return RT3_E_INVALID;
        if (mo->ptr == out->ptr) return fail(c, RT3_E_INVALID, "denoise: the variance input (rt3_denoise_set_variance_input) must not be 'Out'");
    }
    const rt3_denoise_params& p = c->dn_params;
    if (p.iterations == 0) {
        ScopedTimer t(c, CAT_OTHER);
        HIPC(c, hipMemcpyAsync(out->ptr, in->ptr, (size_t)W * H * 16, hipMemcpyDeviceToDevice, c->stream));
        return RT3_OK;
    }
    DenoiseLaunch L;
    L.g = gconst_dev(g);
    L.W = W; L.H = H; L.squarings = p.normal_squarings; L.flags = p.flags; L.sigma_z = p.sigma_z; L.sigma_l = p.sigma_l;
    L.gbuffer = gb->ptr; L.depth = (const float*)dp->ptr; L.in = in->ptr; L.out = out->ptr;
    L.moments = mo ? mo->ptr : nullptr;
    BufLayout plan;
    denoise_plan(W, H, plan, &L.s);
    if (c->dn_scratch.capacity_bytes() < plan.bytes()) {  // the stream may still read the old allocation
        HIPC(c, hipStreamSynchronize(c->stream));
        HIPC(c, c->dn_scratch.grow_bytes(plan.bytes()));
    }
    HIPC(c, plan.carve(c->dn_scratch));
    {
        ScopedTimer t(c, CAT_OTHER);
        launch_denoise_prepare(c->stream, L);
    }
    {
        ScopedTimer t(c, CAT_OTHER);
        launch_denoise_variance(c->stream, L);
    }
    for (uint32_t i = 0; i < p.iterations; i++) {
        ScopedTimer t(c, CAT_OTHER);
        launch_denoise_atrous(c->stream, L, i);
    }
    {
        ScopedTimer t(c, CAT_OTHER);
        launch_denoise_finish(c->stream, L, p.iterations);
    }
    HIPC(c, hipGetLastError());
    return RT3_OK;
}

// "temporal": reprojected accumulation of the previous frame's history (no reference counterpart)
int pass_temporal(rt3_ctx* c, const rt3_gconst* g, uint32_t W, uint32_t H, Resource* const* r) {
    if (!c->tp_has_prev) return fail(c, RT3_E_STATE, "temporal: no previous view (rt3_temporal_set_prev_view)");
    if (c->tp_prev.window_size[0] != g->window_size[0] || c->tp_prev.window_size[1] != g->window_size[1])
        return fail(c, RT3_E_INVALID, "temporal: the previous view's window_size differs from this frame's (after a resize, start over from zeroed history)");
    const rt3_temporal_params& p = c->tp_params;
    TemporalLaunch L;
    L.g = gconst_dev(g);
    L.prev = gconst_dev(&c->tp_prev);
    L.W = W; L.H = H; L.flags = p.flags;
    L.alpha = p.alpha; L.alpha_moments = p.alpha_moments; L.max_history = (float)p.max_history; L.normal_cos = p.normal_cos;
    L.plane_tolerance = p.plane_tolerance;
    L.gbuffer = r[0]->ptr; L.depth = (const float*)r[1]->ptr; L.in = r[2]->ptr;
    L.prev_gbuffer = r[3]->ptr; L.prev_depth = (const float*)r[4]->ptr; L.prev_history = r[5]->ptr; L.prev_moments = r[6]->ptr;
    L.out = r[7]->ptr; L.history = r[8]->ptr; L.moments = r[9]->ptr;
    if (c->tp_motion_image) {
        const Resource* mv = image_checked(c, c->tp_motion_image, W, H, RT3_FORMAT_R32G32B32A32_SFLOAT, "motion input");
        if (!mv) return RT3_E_INVALID;
        if (mv->ptr == r[7]->ptr || mv->ptr == r[8]->ptr || mv->ptr == r[9]->ptr)
            return fail(c, RT3_E_INVALID, "temporal: the motion input (rt3_temporal_set_motion_input) must not be 'Out', 'History' or 'Moments'");
        L.motion = mv->ptr;
    }
    {
        ScopedTimer t(c, CAT_OTHER);
        launch_temporal(c->stream, L);
    }
    HIPC(c, hipGetLastError());
    return RT3_OK;
}

// "motion": where each pixel's surface point was one frame ago (no reference counterpart).  The primary trace is
// pass_gbuffer's (primary_hits), so the hits are the G-buffer's.
int pass_motion(rt3_ctx* c, const rt3_gconst* g, uint32_t W, uint32_t H, Resource* const* res) {
    if (int r = motion_tables(c)) return r;
    MotionLaunch L;
    L.g = gconst_dev(g);
    PixelList* pl;
    if (int r = primary_hits(c, L.g, W, H, &pl)) return r;
    if (pl->count == 0) return RT3_OK;
    const GeomTables t = world_tables(c);
    L.m.verts = t.verts; L.m.indices = t.indices; L.m.geoms = t.geoms; L.m.prim_geom = t.prim_geom; L.m.first_prim = t.first_prim;
    L.m.geom_slot = c->mo_any_moved ? c->d_mo_slot.get() : nullptr;
    L.m.prev = c->d_mo_prev.get();
    L.pixels = pl->dev.get(); L.npix = pl->count; L.width = W; L.hits = c->hits.get(); L.out = res[0]->ptr;
    L.prev_pos = c->mo_any_deformed ? c->d_prev_pos.get() : nullptr;
    {
        ScopedTimer t(c, CAT_OTHER);
        launch_motion(c->stream, L);
    }
    HIPC(c, hipGetLastError());
    return RT3_OK;
}

// ---- the pass table: everything rt3_pass_launch checks before a pass function runs, and the texts of its errors.  include/rt3.h describes
//      the same passes for callers.
enum Shape {
    kWindow,      // (x, y) = the window exactly (WorkSize2D::FullScreen, executions.rs:73); z is ignored, here and by the next
    kProbeAtlas,  // (x, y) = the probe atlas, 8 x 8 texels for each of 1x1 .. floor(W/16) x floor(H/16) probes
    kGroups,      // ceil(W/8) x ceil(H/8) x 1 groups of 8x8 threads (DispatchSize::FullScreen, build.rs:254-258)
    kProbeGrid    // probes_x x probes_y x 1 groups, one per probe: at most floor(W/16) x floor(H/16), or 8191 x 8191 without a window
};
constexpr uint32_t kBuffer = 0;  // a binding that is a buffer, not an image of a format; the pass function checks its size
constexpr uint32_t kU4 = RT3_FORMAT_R32G32B32A32_UINT, kF4 = RT3_FORMAT_R32G32B32A32_SFLOAT, kF1 = RT3_FORMAT_R32_SFLOAT, kU16 = RT3_FORMAT_R16_UINT;
constexpr uint32_t kMaxBindings = 10;
struct Binding {
    const char* name;       // null: the end of the list
    uint32_t format;
    bool atlas = false;     // the image is as large as the probe atlas, not the window
    uint32_t distinct = 0;  // bit j: the image may not be the one bound at (the earlier) position j
};
struct PassDesc {
    const char* name;
    Shape shape;
    bool window;    // reads GConst.window_size
    bool one_rank;  // reads pixels around its own: refused under a tile partition of several ranks
    int (*run)(rt3_ctx* c, const rt3_gconst* g, uint32_t W, uint32_t H, Resource* const* res);
    Binding b[kMaxBindings];
};
const PassDesc kPasses[] = {
    {"gbuffer", kWindow, true, false, pass_gbuffer, {{"gbuffer", kU4}, {"gbuffer_depth", kF1}}},
    {"refrence_mode", kWindow, true, false, pass_reference_mode, {{"gbuffer", kU4}, {"gbuffer_depth", kF1}, {"Light", kF4}, {"PrevLight", kF4}}},
    {"postprocess", kGroups, true, false, pass_postprocess, {{"Depth", kF1}, {"Out", kF4}, {"In", kF4}}},
    {"structured_importance_sampling", kProbeGrid, true, false, pass_sis,
     {{"gbuffer", kU4}, {"gbuffer_depth", kF1}, {"out", kU16, true}, {"debug", kF1, true}, {"probe_atlas", kF4, true}}},
    {"trace_probes", kProbeAtlas, true, false, pass_trace_probes,
     {{"gbuffer", kU4}, {"gbuffer_depth", kF1}, {"directions", kU16, true}, {"probe_atlas", kF4, true}, {"prev_probe_atlas", kF4, true, 1u << 3}}},
    {"spherical_harmonic_conversion", kProbeGrid, false, false, pass_sh_conversion, {{"out", kBuffer}, {"probe_atlas", kF4, true}}},
    {"interpolate_probes", kGroups, true, false, pass_interpolate_probes,
     {{"gbuffer", kU4}, {"gbuffer_depth", kF1}, {"sh_coeficents", kBuffer}, {"Light", kF4}}},
    {"denoise", kGroups, true, true, pass_denoise, {{"gbuffer", kU4}, {"gbuffer_depth", kF1}, {"In", kF4}, {"Out", kF4, false, 1u << 2}}},
    {"temporal", kGroups, true, true, pass_temporal,
     {{"gbuffer", kU4}, {"gbuffer_depth", kF1}, {"In", kF4}, {"PrevGbuffer", kU4}, {"PrevDepth", kF1}, {"PrevHistory", kF4}, {"PrevMoments", kF4},
      {"Out", kF4, false, 0x7Fu}, {"History", kF4, false, 0xFFu}, {"Moments", kF4, false, 0x1FFu}}},
    {"motion", kWindow, true, false, pass_motion, {{"Motion", kF4}}},
};
// a, b, ... : the names of a table's entries
template <typename T, size_t N>
std::string names_of(const T (&list)[N]) {
    std::string s;
    for (size_t i = 0; i < N && list[i].name; i++) s += (i ? ", " : "") + std::string(list[i].name);
    return s;
}

// Checks in this order: window, launch shape, binding count, the bindings in their order, aliasing, tile partition; then the pass function
int launch_pass(rt3_ctx* c, const PassDesc& p, const rt3_gconst* g, uint32_t x, uint32_t y, uint32_t z, const uint32_t* b, uint32_t nb) {
    const std::string name = p.name;
    uint32_t W = 0, H = 0, ax = 0, ay = 0;  // the window; the probe atlas
    if (p.window)
        if (int r = check_window(c, g, &W, &H)) return r;
    const uint32_t max_px = p.window ? W / 16 : 8191u, max_py = p.window ? H / 16 : 8191u;
    switch (p.shape) {
        case kWindow:
            if (x != W || y != H) return fail(c, RT3_E_INVALID, name + ": launch size must be the window size (WorkSize2D::FullScreen, executions.rs:73)");
            break;
        case kProbeAtlas:
            if (x % 8 || y % 8 || x == 0 || y == 0 || x / 8 > max_px || y / 8 > max_py)
                return fail(c, RT3_E_INVALID, name + ": launch size is the probe atlas, 8 x 8 texels per probe, of 1x1 to floor(W/16) x floor(H/16) probes");
            ax = x, ay = y;
            break;
        case kGroups:
            if (x != (W + 7) / 8 || y != (H + 7) / 8 || z != 1)
                return fail(c, RT3_E_INVALID, name + ": dispatch must be ceil(W/8) x ceil(H/8) x 1 groups (DispatchSize::FullScreen, build.rs:254-258)");
            break;
        case kProbeGrid:
            if (z != 1 || x == 0 || y == 0 || x > max_px || y > max_py)
                return fail(c, RT3_E_INVALID, name + ": dispatch is probes_x x probes_y x 1 groups of 8x8 threads, 1x1 to floor(W/16) x floor(H/16) probes");
            ax = 8 * x, ay = 8 * y;
            break;
    }
    uint32_t n = 0;
    while (n < kMaxBindings && p.b[n].name) n++;
    if (nb != n)
        return fail(c, RT3_E_INVALID, name + " expects " + std::to_string(n) + (n == 1 ? " binding {" : " bindings {") + names_of(p.b) + "}");
    Resource* res[kMaxBindings];
    for (uint32_t i = 0; i < n; i++) {
        const Binding& bd = p.b[i];
        if (bd.format == kBuffer) {
            if (!(res[i] = get_res(c, b[i], RT3_TAG_BUFFER))) return fail(c, RT3_E_INVALID, name + ": binding '" + bd.name + "' is not a buffer");
        } else if (!(res[i] = image_checked(c, b[i], bd.atlas ? ax : W, bd.atlas ? ay : H, bd.format, bd.name))) {
            return RT3_E_INVALID;
        }
    }
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t j = 0; j < i; j++)
            if ((p.b[i].distinct >> j & 1u) && res[i]->ptr == res[j]->ptr)
                return fail(c, RT3_E_INVALID, name + ": '" + p.b[i].name + "' and '" + p.b[j].name +
                                                  "' must be different images (one is read while pixels of the other are written)");
    if (p.one_rank && c->n_ranks > 1)
        return fail(c, RT3_E_STATE, name + ": a tap may need pixels that other ranks own; run it on the gathered image with the tile partition "
                                           "switched off (rt3_set_tile_partition(w, h, 0, 1))");
    return p.run(c, g, W, H, res);
}

}  // namespace

// ================================================================================================== C ABI
extern "C" {

int rt3_create(int device, rt3_ctx** out) {
    if (!out) return fail(nullptr, RT3_E_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(nullptr, RT3_E_NO_DEVICE, "no HIP device visible (librt3 has no CPU fallback)");
    if (device < 0 || device >= n) return fail(nullptr, RT3_E_INVALID, "device index out of range");
    hipDeviceProp_t prop;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(nullptr, RT3_E_HIP, "hipSetDevice failed");
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(nullptr, RT3_E_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", librt3 is built for gfx950 only");
    rt3_ctx* c = new rt3_ctx();
    c->device = device;
    snprintf(c->name, sizeof(c->name), "%s (%s)", prop.name, prop.gcnArchName);
    memset(&c->stats, 0, sizeof(c->stats));
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || c->d_counters.alloc_bytes((size_t)c->counters_cap * 4) != hipSuccess ||
        c->d_totals.alloc_bytes(kTotWords * 8) != hipSuccess || hipMemset(c->d_totals.get(), 0, kTotWords * 8) != hipSuccess) {
        rt3_destroy(c);  // the stream too
        return fail(nullptr, RT3_E_HIP, "stream / counter allocation failed");
    }
    *out = c;
    return RT3_OK;
}

void rt3_destroy(rt3_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);  // no device memory is freed before the stream is idle
    if (c->comm) (void)ncclCommDestroy(c->comm);
    for (auto& t : c->pending_events) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
    for (auto& t : c->free_events) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
    hipStream_t stream = c->stream;
    delete c;  // releases every device buffer the context owns
    if (stream) (void)hipStreamDestroy(stream);  // the stream goes last
}

const char* rt3_last_error(rt3_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int rt3_device_name(rt3_ctx* c, char* buf, size_t n) {
    if (!c || !buf || !n) return RT3_E_INVALID;
    snprintf(buf, n, "%s", c->name);
    return RT3_OK;
}

int rt3_set_option(rt3_ctx* c, int option, int64_t value) {
    if (!c) return RT3_E_INVALID;
    switch (option) {
        case RT3_OPT_BATCH_SPP: c->opt_batch_spp = value; return RT3_OK;
        case RT3_OPT_PROFILE: c->opt_profile = value != 0; return RT3_OK;
        case RT3_OPT_COUNT_TRAVERSAL: c->opt_count = value != 0; return RT3_OK;
        case RT3_OPT_EXTEND_VARIANT:
            c->opt_variant = (int)value;
            HIPC(c, hipSetDevice(c->device));  // the traversal knobs are __constant__ words of the device the context runs on
            set_refill_lanes((uint32_t)value);
            return RT3_OK;
        case RT3_OPT_LEAF_SIZE:
            if (value < 1 || value > 8) return fail(c, RT3_E_INVALID, "leaf size must be 1..8");
            c->opt_leaf_size = (uint32_t)value;
            invalidate_topology(c);
            return RT3_OK;
        case RT3_OPT_NODE_QUANT:
            if (value < 0 || value > 2) return fail(c, RT3_E_INVALID, "node quantisation must be 0 (fp32), 1 (64 B) or 2 (compact 48 B)");
            c->opt_node_quant = (uint32_t)value;
            invalidate_topology(c);
            return RT3_OK;
        case RT3_OPT_SAH_TOP:
            if (value < 0 || value > 65536) return fail(c, RT3_E_INVALID, "SAH-top cluster size must be 0 (off) .. 65536");
            c->opt_sah_top = (uint32_t)value;
            invalidate_topology(c);
            return RT3_OK;
        case RT3_OPT_POOL_CHUNK:
            if (value < 64 || value > 65536 || (value & 63)) return fail(c, RT3_E_INVALID, "pool chunk must be a multiple of 64 in [64, 65536]");
            HIPC(c, hipSetDevice(c->device));
            set_pool_chunk((uint32_t)value);
            return RT3_OK;
        case RT3_OPT_TRACE_BLOCKS:
            if (value < 1 || value > 65535) return fail(c, RT3_E_INVALID, "trace blocks must be in [1, 65535]");
            set_trace_blocks((uint32_t)value);
            return RT3_OK;
        case RT3_OPT_WIDE_COLLAPSE:
            if (value < 0 || value > 2) return fail(c, RT3_E_INVALID, "wide collapse must be 0 (even depth), 1 (surface area) or 2 (cost-driven)");
            c->opt_collapse = (uint32_t)value;
            invalidate_topology(c);
            return RT3_OK;
        case RT3_OPT_NODE_WIDTH:
            if (value != 2 && value != 4) return fail(c, RT3_E_INVALID, "node width must be 2 or 4");
            c->opt_node_width = (uint32_t)value;
            invalidate_topology(c);
            return RT3_OK;
        case RT3_OPT_INSTANCE_MODE:
            if (value != 0 && value != 1) return fail(c, RT3_E_INVALID, "instance mode must be 0 (flatten) or 1 (two-level)");
            c->opt_instance_mode = (int)value;
            c->accel_built = false;
            return RT3_OK;
        default: return fail(c, RT3_E_INVALID, "unknown option");
    }
}

// ---- scene
// [first, end) joins the sorted list of disjoint ranges; ranges that touch merge.  A list that grows long collapses into its hull.
static void add_dirty_range(std::vector<std::pair<uint32_t, uint32_t>>& ranges, uint32_t first, uint32_t end) {
    std::vector<std::pair<uint32_t, uint32_t>> out;
    bool placed = false;
    for (const auto& r : ranges) {
        if (r.second < first) out.push_back(r);
        else if (end < r.first) {
            if (!placed) out.push_back({first, end});
            placed = true;
            out.push_back(r);
        } else {
            first = std::min(first, r.first);
            end = std::max(end, r.second);
        }
    }
    if (!placed) out.push_back({first, end});
    if (out.size() > 64) out.assign(1, {out.front().first, out.back().second});
    ranges.swap(out);
}
// no previous positions: "motion" is what it is without them
static void forget_snapshot(rt3_ctx* c) {
    c->df_snapshot = false;
    c->df_ranges.clear();
    c->df_dirty = true;
}
// Which geometries are deformed: geometry g is when some vertex of its span differs from the snapshot in a position
// word.  Only vertices updated since the snapshot can differ, so the compare kernel runs over the spans' intersections with the dirty
// ranges, in chunks of at most kDeformChunk vertices; with none no kernel runs.  Leaves the flags in h_deformed and marks the motion
// tables for a rebuild.
static int deform_flags(rt3_ctx* c) {
    if (!c->df_dirty) return RT3_OK;
    c->h_deformed.assign(c->n_geoms, 0u);
    std::vector<uint4> chunks;
    if (c->df_snapshot)
        for (uint32_t g = 0; g < c->n_geoms && g < c->h_geom_span.size(); g++) {
            const auto [lo, hi] = c->h_geom_span[g];
            if (lo > hi) continue;
            for (const auto& r : c->df_ranges) {  // (every range lies inside the vertex buffer and the snapshot: rt3_scene_update_vertices)
                const uint32_t a = std::max(lo, r.first), b = std::min(hi + 1u, r.second);
                for (uint32_t at = a; at < b; at += kDeformChunk) chunks.push_back(make_uint4(g, at, std::min(b, at + kDeformChunk), 0u));
            }
        }
    if (!chunks.empty()) {
        HIPC(c, hipSetDevice(c->device));
        HIPC(c, hipStreamSynchronize(c->stream));  // an earlier launch may still read the chunk table
        HIPC(c, c->d_df_chunks.grow_bytes(chunks.size() * sizeof(uint4)));
        HIPC(c, c->d_deformed.grow_bytes((size_t)c->n_geoms * 4));
        HIPC(c, hipMemcpy(c->d_df_chunks.get(), chunks.data(), chunks.size() * sizeof(uint4), hipMemcpyHostToDevice));
        HIPC(c, hipMemsetAsync(c->d_deformed.get(), 0, (size_t)c->n_geoms * 4, c->stream));
        {
            ScopedTimer t(c, CAT_OTHER);
            launch_compare_positions(c->stream, c->d_verts.get(), c->d_prev_pos.get(), c->d_df_chunks.get(), (uint32_t)chunks.size(), c->d_deformed.get());
        }
        HIPC(c, hipGetLastError());
        HIPC(c, hipMemcpyAsync(c->h_deformed.data(), c->d_deformed.get(), (size_t)c->n_geoms * 4, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
    }
    c->df_dirty = false;
    c->mo_dirty = true;
    return RT3_OK;
}
int rt3_scene_set_vertices(rt3_ctx* c, const float* v, uint32_t n) {
    if (!c || (!v && n)) return fail(c, RT3_E_INVALID, "vertices NULL");
    // a NaN / infinite position would poison the scene bounds, the Morton codes and every box above it: reject it here
    // (bounded magnitude too, so that box extents and the quantisation grid cannot overflow to infinity)
    for (size_t i = 0; i < (size_t)n; i++)
        for (int k = 0; k < 3; k++)
            if (!(std::fabs(v[8 * i + k]) <= 1.0e18f)) return fail(c, RT3_E_INVALID, "vertex " + std::to_string(i) + ": position is not finite (or beyond 1e18)");
    HIPC(c, hipSetDevice(c->device));
    if (int r = dev_alloc(c, c->d_verts, (size_t)n * 8)) return r;
    if (n) HIPC(c, hipMemcpy(c->d_verts.get(), v, (size_t)n * 32, hipMemcpyHostToDevice));
    c->n_verts = n;
    invalidate_topology(c);
    forget_snapshot(c);
    return RT3_OK;
}
// vertices [first, first + n) in place; the shape of every tree stays, so a structure built before is stale, not gone (rt3_accel_refit)
int rt3_scene_update_vertices(rt3_ctx* c, const float* v, uint32_t first, uint32_t n) {
    if (!c || (!v && n)) return fail(c, RT3_E_INVALID, "vertices NULL");
    if ((uint64_t)first + n > c->n_verts) return fail(c, RT3_E_INVALID, "update_vertices: [first, first + n) exceeds the vertex buffer (rt3_scene_set_vertices)");
    for (size_t i = 0; i < (size_t)n; i++)  // rt3_scene_set_vertices' check
        for (int k = 0; k < 3; k++)
            if (!(std::fabs(v[8 * i + k]) <= 1.0e18f)) return fail(c, RT3_E_INVALID, "vertex " + std::to_string(first + i) + ": position is not finite (or beyond 1e18)");
    if (n == 0) return RT3_OK;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));  // work in flight may still read the old vertices
    c->content_gen++;
    if (c->accel_built) c->accel_stale = true;
    HIPC(c, hipMemcpy(c->d_verts.get() + 8 * (size_t)first, v, (size_t)n * 32, hipMemcpyHostToDevice));
    if (c->df_snapshot) {
        add_dirty_range(c->df_ranges, first, first + n);
        c->df_dirty = true;
    }
    return RT3_OK;
}
// "the positions the vertex buffer holds now are the previous frame's" (DESIGN.md section 4i): a device-side copy of the ranges updated since
// the last snapshot (the first one: of every vertex) on the context's stream.  Nothing a build or refit reads changes.
int rt3_scene_snapshot_vertices(rt3_ctx* c) {
    if (!c) return fail(c, RT3_E_INVALID, "context NULL");
    if (!c->d_verts || c->n_verts == 0) return fail(c, RT3_E_STATE, "snapshot_vertices: no vertices (rt3_scene_set_vertices)");
    HIPC(c, hipSetDevice(c->device));
    if (!c->df_snapshot) {
        HIPC(c, hipStreamSynchronize(c->stream));  // an earlier "motion" launch may still read the old records
        HIPC(c, c->d_prev_pos.grow_bytes((size_t)c->n_verts * sizeof(float4)));
        c->df_ranges.assign(1, {0u, c->n_verts});
    }
    for (const auto& r : c->df_ranges) {
        ScopedTimer t(c, CAT_OTHER);
        launch_snapshot_positions(c->stream, c->d_verts.get(), r.first, r.second - r.first, c->d_prev_pos.get());
    }
    HIPC(c, hipGetLastError());
    c->df_ranges.clear();
    c->df_snapshot = true;
    c->df_dirty = true;
    return RT3_OK;
}
int rt3_scene_forget_prev_vertices(rt3_ctx* c) {
    if (!c) return fail(c, RT3_E_INVALID, "context NULL");
    forget_snapshot(c);
    return RT3_OK;
}
// The flags of deform_flags, one byte per uploaded geometry
int rt3_scene_deformed_geometries(rt3_ctx* c, uint8_t* flags, uint32_t n) {
    if (!c || (!flags && n)) return fail(c, RT3_E_INVALID, "deformed_geometries: NULL");
    if (!c->df_snapshot) return fail(c, RT3_E_STATE, "deformed_geometries: no snapshot (rt3_scene_snapshot_vertices)");
    if (n != c->n_geoms) return fail(c, RT3_E_INVALID, "deformed_geometries: n must be the geometry count of rt3_scene_set_geometry (" + std::to_string(c->n_geoms) + ")");
    if (int r = deform_flags(c)) return r;
    for (uint32_t i = 0; i < n; i++) flags[i] = c->h_deformed[i] ? 1 : 0;
    return RT3_OK;
}
int rt3_scene_set_indices(rt3_ctx* c, const uint32_t* idx, uint32_t n) {
    if (!c || (!idx && n)) return fail(c, RT3_E_INVALID, "indices NULL");
    HIPC(c, hipSetDevice(c->device));
    if (int r = dev_alloc(c, c->d_indices, (size_t)n)) return r;
    if (n) HIPC(c, hipMemcpy(c->d_indices.get(), idx, (size_t)n * 4, hipMemcpyHostToDevice));
    c->n_indices = n;
    c->h_indices.assign(idx, idx + n);
    invalidate_topology(c);
    forget_snapshot(c);
    return RT3_OK;
}
// bounds of every geometry's index / vertex range against the world buffers as they are NOW: the kernels index them without
// checks (a GPU fault would take the node down).  Run by rt3_scene_set_geometry and again by rt3_accel_build, because the vertex
// and index buffers may be replaced (by smaller ones) after the geometry was set.
// spans: per geometry the vertices [vertex_offset + least index, vertex_offset + largest index] its triangles lie in ({1, 0}: none)
static int validate_geometry(rt3_ctx* c, const rt3_geometry_info* g, const uint32_t* prim_counts, uint32_t n,
                             std::vector<std::pair<uint32_t, uint32_t>>* spans = nullptr) {
    for (uint32_t i = 0; i < n; i++) {
        if ((uint64_t)g[i].index_offset + 3ull * prim_counts[i] > c->n_indices)
            return fail(c, RT3_E_INVALID, "geometry " + std::to_string(i) + ": index range exceeds the index buffer");
        uint32_t mx = 0, mn = 0xFFFFFFFFu;
        for (uint64_t k = 0; k < 3ull * prim_counts[i]; k++) {
            uint32_t v = c->h_indices[g[i].index_offset + k];
            mx = v > mx ? v : mx;
            mn = v < mn ? v : mn;
        }
        if (prim_counts[i] && (uint64_t)g[i].vertex_offset + mx >= (uint64_t)c->n_verts)
            return fail(c, RT3_E_INVALID, "geometry " + std::to_string(i) + ": vertex range exceeds the vertex buffer (set vertices and indices before geometry)");
        if (spans) spans->push_back(prim_counts[i] ? std::make_pair(g[i].vertex_offset + mn, g[i].vertex_offset + mx) : std::make_pair(1u, 0u));
    }
    return RT3_OK;
}
int rt3_scene_set_geometry(rt3_ctx* c, const rt3_geometry_info* g, const uint32_t* prim_counts, uint32_t n) {
    if (!c || ((!g || !prim_counts) && n)) return fail(c, RT3_E_INVALID, "geometry NULL");
    HIPC(c, hipSetDevice(c->device));
    std::vector<std::pair<uint32_t, uint32_t>> spans;
    if (int r = validate_geometry(c, g, prim_counts, n, &spans)) return r;
    c->h_geom_span.swap(spans);
    uint64_t total = 0;
    int64_t max_tex = -1;
    for (uint32_t i = 0; i < n; i++) {
        if (g[i].base_color_texture_index > max_tex) max_tex = g[i].base_color_texture_index;
        total += prim_counts[i];
    }
    if (total > 0x7FFFFFFFull) return fail(c, RT3_E_INVALID, "too many primitives");
    // (the device tables -- one entry per (instance, geometry) -- are made by rt3_accel_build, which knows the instances)
    c->h_geoms.assign(g, g + n);
    c->h_prim_counts.assign(prim_counts, prim_counts + n);
    c->h_cutoffs.clear();  // every geometry opaque again
    c->n_geoms = n;
    c->max_tex_index = max_tex;
    c->n_prims = (uint32_t)total;
    invalidate_topology(c);
    forget_snapshot(c);
    return RT3_OK;
}
// alpha cutoffs of the geometries of the last rt3_scene_set_geometry; n = 0: all opaque
int rt3_scene_set_alpha_cutoffs(rt3_ctx* c, const float* cutoffs, uint32_t n) {
    if (!c || (!cutoffs && n)) return fail(c, RT3_E_INVALID, "alpha cutoffs NULL");
    if (n != 0 && n != c->n_geoms)
        return fail(c, RT3_E_INVALID, "alpha cutoffs: n must be 0 or the geometry count of rt3_scene_set_geometry (" + std::to_string(c->n_geoms) + ")");
    for (uint32_t i = 0; i < n; i++)
        if (!(cutoffs[i] >= 0.0f && cutoffs[i] <= 1.0f)) return fail(c, RT3_E_INVALID, "alpha cutoff " + std::to_string(i) + " is not in [0, 1]");
    c->h_cutoffs.clear();
    if (std::any_of(cutoffs, cutoffs + n, [](float v) { return v > 0.0f; })) c->h_cutoffs.assign(cutoffs, cutoffs + n);  // (kept only when some geometry is masked)
    invalidate_topology(c);  // the triangle records carry the masks: a new build, not a refit
    return RT3_OK;
}
static bool any_cutoff(const rt3_ctx* c) { return !c->h_cutoffs.empty(); }
// Sky storage and importance tables (north_star; the oracle's orc_scene_set_sky has the definitions and is built by the same
// arithmetic, in double, in the same order): radiance stored as RGB9E5 (packing.slang:99-162), marginal CDF over rows, one alias
// table per row with 16-bit keep-thresholds, pdf_uv = the density the quantised tables really realise.
static uint32_t host_rgb9e5(const float* c) {  // packing.slang:99-144 == rt3_device.hpp float3_to_rgb9e5
    auto bits = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
    auto from_bits = [](uint32_t u) { float f; memcpy(&f, &u, 4); return f; };
    const float mx = (511.0f / 512.0f) * 65536.0f;
    auto clampf = [&](float v) { v = v > 0.0f ? v : 0.0f; return v < mx ? v : mx; };
    const float rc = clampf(c[0]), gc = clampf(c[1]), bc = clampf(c[2]);
    const float m1 = gc > bc ? gc : bc, maxrgb = rc > m1 ? rc : m1;
    const int fl2 = (int)((bits(maxrgb) & 0x7F800000u) >> 23) - 127;
    int exp_shared = (fl2 > -16 ? fl2 : -16) + 1 + 15;
    float denom = from_bits((uint32_t)(exp_shared - 15 - 9 + 127) << 23);
    const int maxm = (int)std::floor(maxrgb / denom + 0.5f);
    if (maxm == 512) {
        denom *= 2.0f;
        exp_shared += 1;
    }
    const int rm = (int)std::floor(rc / denom + 0.5f), gm = (int)std::floor(gc / denom + 0.5f), bm = (int)std::floor(bc / denom + 0.5f);
    return ((uint32_t)rm << 23) | ((uint32_t)gm << 14) | ((uint32_t)bm << 5) | (uint32_t)exp_shared;
}
static void host_rgb9e5_decode(uint32_t v, float* c) {  // packing.slang:146-162
    const uint32_t sb = (uint32_t)((int)(v & 31u) - 24 + 127) << 23;
    float scale;
    memcpy(&scale, &sb, 4);
    c[0] = (float)((v >> 23) & 511u) * scale;
    c[1] = (float)((v >> 14) & 511u) * scale;
    c[2] = (float)((v >> 5) & 511u) * scale;
}
int rt3_scene_set_sky(rt3_ctx* c, const float* rgb, uint32_t w, uint32_t h) {
    if (!c || !rgb || !w || !h) return fail(c, RT3_E_INVALID, "sky NULL / empty");
    if (w > 65535 || h > 65535) return fail(c, RT3_E_INVALID, "sky larger than 65535 texels per side");
    HIPC(c, hipSetDevice(c->device));
    const size_t n = (size_t)w * h;
    for (size_t i = 0; i < 3 * n; i++)  // a NaN or negative texel would poison the sampling tables
        if (!(rgb[i] >= 0.0f && rgb[i] <= 3.4028234663852886e38f))
            return fail(c, RT3_E_INVALID, "sky texel " + std::to_string(i / 3) + " is negative or not finite (clamp the image before uploading it)");
    std::vector<uint32_t> texq(n), alias(n);
    std::vector<float> pdf(n), marg(h);
    std::vector<double> rows(h), f(w), sc(w), real(w);
    std::vector<uint32_t> small(w), large(w);
    double total = 0.0;
    for (uint32_t y = 0; y < h; y++) {
        const double st = std::sin(3.14159265358979323846 * ((double)y + 0.5) / (double)h);
        double acc = 0.0;
        for (uint32_t x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            texq[i] = host_rgb9e5(rgb + 3 * i);
            float p[3];
            host_rgb9e5_decode(texq[i], p);
            const float lum = p[0] * 0.299f + p[1] * 0.587f + p[2] * 0.114f;  // luminance(), math.slang:119-122
            f[x] = ((double)lum + 1e-6) * st;
            acc += f[x];
        }
        rows[y] = acc;
        total += acc;
        uint32_t ns = 0, nl = 0;
        uint32_t* al = alias.data() + (size_t)y * w;
        for (uint32_t x = 0; x < w; x++) {
            sc[x] = f[x] * (double)w / acc;
            if (sc[x] < 1.0) small[ns++] = x;
            else large[nl++] = x;
        }
        for (uint32_t x = 0; x < w; x++) al[x] = 65535u | (x << 16);
        while (ns && nl) {  // Vose's alias method; both stacks filled in ascending column order and popped from the top
            const uint32_t a = small[--ns], g = large[--nl];
            const double q = sc[a] * 65536.0;
            int64_t q16 = (int64_t)std::floor(q + 0.5) - 1;
            q16 = q16 < 0 ? 0 : (q16 > 65535 ? 65535 : q16);
            al[a] = (uint32_t)q16 | (g << 16);
            sc[g] = (sc[g] + sc[a]) - 1.0;
            if (sc[g] < 1.0) small[ns++] = g;
            else large[nl++] = g;
        }
        for (uint32_t x = 0; x < w; x++) real[x] = 0.0;
        for (uint32_t x = 0; x < w; x++) {
            const double Q = (double)((al[x] & 0xFFFFu) + 1u) / 65536.0;
            real[x] += Q;
            real[al[x] >> 16] += 1.0 - Q;
        }
        for (uint32_t x = 0; x < w; x++) pdf[(size_t)y * w + x] = (float)real[x];
    }
    double run = 0.0;
    for (uint32_t y = 0; y < h; y++) {
        run += rows[y];
        marg[y] = (float)(run / total);
        const double rowp = rows[y] / total * (double)h;
        for (uint32_t x = 0; x < w; x++) pdf[(size_t)y * w + x] = (float)((double)pdf[(size_t)y * w + x] * rowp);
    }
    marg[h - 1] = 1.0f;
    // guide table of the marginal CDF: guide[k] = first index with cdf > k / n, so a lookup of u (cell k = floor(u n)) starts inside
    // [guide[k-1], guide[k+1]].  Stored per cell as one word lo | hi << 16 (hi clamped to n-1): one load instead of two.
    std::vector<uint32_t> gmarg(h);
    {
        std::vector<uint32_t> g(h + 1);
        uint32_t i = 0;
        for (uint32_t k = 0; k <= h; k++) {
            const float thr = (float)k / (float)h;
            while (i < h - 1 && !(marg[i] > thr)) i++;
            g[k] = i;
        }
        for (uint32_t k = 0; k < h; k++) {
            const uint32_t lo = g[k > 0 ? k - 1 : 0], hi = g[k + 1] > h - 1 ? h - 1 : g[k + 1];
            gmarg[k] = lo | (hi << 16);
        }
    }
    // the marginal CDF is stored with one leading 0 and three trailing pads (2.0 > any u): cdfp[i + 1] = cdf[i], so that
    // {cdf[i-1], cdf[i], cdf[i+1], cdf[i+2]} is ONE 16-byte load at cdfp + i for every i
    std::vector<float> margp((size_t)h + 4);
    margp[0] = 0.0f;
    std::memcpy(margp.data() + 1, marg.data(), (size_t)h * 4);
    margp[h + 1] = margp[h + 2] = margp[h + 3] = 2.0f;
    // texels in 4 x 4 tiles of 128 bytes; ragged edges are padded (never addressed: lookups wrap / clamp to [0, w) x [0, h))
    const uint32_t wt = (w + 3) / 4, ht = (h + 3) / 4;
    std::vector<uint2> tiled((size_t)wt * ht * 16, make_uint2(0u, 0u));
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            uint32_t pb;
            memcpy(&pb, &pdf[(size_t)y * w + x], 4);
            tiled[((size_t)(y >> 2) * wt + (x >> 2)) * 16 + (((y & 3u) << 2) | (x & 3u))] = make_uint2(texq[(size_t)y * w + x], pb);
        }
    if (int r = dev_alloc(c, c->d_guide_marg, gmarg.size())) return r;
    if (int r = dev_alloc(c, c->d_sky_alias, alias.size())) return r;
    if (int r = dev_alloc(c, c->d_sky, tiled.size())) return r;
    if (int r = dev_alloc(c, c->d_cdf_marg, margp.size())) return r;
    HIPC(c, hipMemcpy(c->d_guide_marg.get(), gmarg.data(), gmarg.size() * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->d_sky_alias.get(), alias.data(), alias.size() * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->d_sky.get(), tiled.data(), tiled.size() * 8, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->d_cdf_marg.get(), margp.data(), margp.size() * 4, hipMemcpyHostToDevice));
    c->sky_w = w;
    c->sky_h = h;
    c->sky_wt = wt;
    return RT3_OK;
}
int rt3_scene_set_bluenoise(rt3_ctx* c, const uint8_t* rgba, uint32_t w, uint32_t h) {
    if (!c || !rgba || !w || !h) return fail(c, RT3_E_INVALID, "bluenoise NULL / empty");
    HIPC(c, hipSetDevice(c->device));
    if (int r = dev_alloc(c, c->d_bn, (size_t)w * h * 4)) return r;
    HIPC(c, hipMemcpy(c->d_bn.get(), rgba, (size_t)w * h * 4, hipMemcpyHostToDevice));
    c->bn_w = w;
    c->bn_h = h;
    c->bn_stamp++;
    return RT3_OK;
}
// base-colour texture `index` (RGBA8, sRGB-encoded colour), sampled by hit_info when GeometryInfo.baseColorTextureIndex == index
int rt3_scene_set_texture(rt3_ctx* c, uint32_t index, const uint8_t* rgba, uint32_t w, uint32_t h) {
    if (!c || !rgba || !w || !h || w > 16384 || h > 16384 || index > 4096) return fail(c, RT3_E_INVALID, "texture: NULL / bad size / index");
    if (index >= c->h_tex.size()) {
        c->h_tex.resize(index + 1);
        c->tex_w.resize(index + 1, 0);
        c->tex_h.resize(index + 1, 0);
    }
    c->h_tex[index].assign(rgba, rgba + (size_t)w * h * 4);
    c->tex_w[index] = w;
    c->tex_h[index] = h;
    c->tex_dirty = true;
    return RT3_OK;
}
int rt3_sky_download(rt3_ctx* c, uint32_t* alias, uint32_t* texels, float* marg, float* pdf) {
    if (!c || !c->d_sky) return fail(c, RT3_E_STATE, "no sky set");
    const uint32_t w = c->sky_w, h = c->sky_h, wt = c->sky_wt, ht = (h + 3) / 4;
    if (alias) HIPC(c, hipMemcpy(alias, c->d_sky_alias.get(), (size_t)w * h * 4, hipMemcpyDeviceToHost));
    if (marg) HIPC(c, hipMemcpy(marg, c->d_cdf_marg.get() + 1, (size_t)h * 4, hipMemcpyDeviceToHost));  // strip the padding
    if (texels || pdf) {  // un-tile
        std::vector<uint2> tiled((size_t)wt * ht * 16);
        HIPC(c, hipMemcpy(tiled.data(), c->d_sky.get(), tiled.size() * 8, hipMemcpyDeviceToHost));
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) {
                const uint2 t = tiled[((size_t)(y >> 2) * wt + (x >> 2)) * 16 + (((y & 3u) << 2) | (x & 3u))];
                if (texels) texels[(size_t)y * w + x] = t.x;
                if (pdf) memcpy(&pdf[(size_t)y * w + x], &t.y, 4);
            }
    }
    return RT3_OK;
}

// world/mod.rs:34-60,104-125: InstanceInfo{mesh_index, transform} + Transform{Mat4}, global instance / transform buffers
int rt3_scene_set_instances(rt3_ctx* c, const rt3_instance* inst, uint32_t n) {
    if (!c || (!inst && n)) return fail(c, RT3_E_INVALID, "instances NULL");
    for (uint32_t i = 0; i < n; i++) {
        for (int k = 0; k < 16; k++)
            if (!(std::fabs(inst[i].transform[k]) <= 1.0e18f)) return fail(c, RT3_E_INVALID, "instance " + std::to_string(i) + ": transform is not finite (or beyond 1e18)");
        const float* m = inst[i].transform;
        if (m[3] != 0.0f || m[7] != 0.0f || m[11] != 0.0f || m[15] != 1.0f)
            return fail(c, RT3_E_INVALID, "instance " + std::to_string(i) + ": the last row of the transform must be (0, 0, 0, 1) (VkTransformMatrixKHR is 3 x 4 too)");
    }
    c->h_instances.assign(inst, inst + n);
    c->accel_built = false;
    return RT3_OK;
}
// The previous frame's matrices of the same instances, for the "motion" pass only: no build reads them and the structure stays as it is
int rt3_scene_set_prev_transforms(rt3_ctx* c, const float* transforms, uint32_t n) {
    if (!c || (!transforms && n)) return fail(c, RT3_E_INVALID, "previous transforms NULL");
    for (uint32_t i = 0; i < n; i++) {
        const float* m = transforms + 16 * (size_t)i;
        for (int k = 0; k < 16; k++)
            if (!(std::fabs(m[k]) <= 1.0e18f)) return fail(c, RT3_E_INVALID, "previous transform " + std::to_string(i) + " is not finite (or beyond 1e18)");
        if (m[3] != 0.0f || m[7] != 0.0f || m[11] != 0.0f || m[15] != 1.0f)
            return fail(c, RT3_E_INVALID, "previous transform " + std::to_string(i) + ": the last row must be (0, 0, 0, 1), as for an instance's matrix");
    }
    c->mo_prev.assign(transforms, transforms + 16 * (size_t)n);
    c->mo_dirty = true;
    return RT3_OK;
}
static const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
// The placements a build covers: the instances set, or (none) one identity instance of every geometry, which `whole` then holds
static std::pair<const rt3_instance*, size_t> placements(const rt3_ctx* c, rt3_instance& whole) {
    if (!c->h_instances.empty()) return {c->h_instances.data(), c->h_instances.size()};
    whole.geometry_first = 0;
    whole.geometry_count = c->n_geoms;
    memcpy(whole.transform, kIdentity, sizeof(kIdentity));
    return {&whole, 1};
}
// One (instance, geometry) pair per entry, instance-major.  A few KiB of tables go up; primitive -> entry is filled in on the device
// (k_prim_geom), so a rebuild after a moved instance copies nothing big.
static int flatten_world(rt3_ctx* c) {
    rt3_instance whole;
    const auto [inst, n_inst] = placements(c, whole);
    std::vector<FlatGeomDev> flat;
    std::vector<ShadeGeomDev> shade;
    std::vector<uint32_t> first;
    uint64_t total = 0;
    for (size_t i = 0; i < n_inst; i++) {
        if ((uint64_t)inst[i].geometry_first + inst[i].geometry_count > c->n_geoms)
            return fail(c, RT3_E_INVALID, "instance " + std::to_string(i) + ": geometry range exceeds the geometries set (rt3_scene_set_geometry)");
        const float* m = inst[i].transform;
        const bool identity = memcmp(m, kIdentity, sizeof(kIdentity)) == 0;
        for (uint32_t k = 0; k < inst[i].geometry_count; k++) {
            const uint32_t g = inst[i].geometry_first + k;
            FlatGeomDev f;
            memset(&f, 0, sizeof(f));
            static_assert(sizeof(rt3_geometry_info) == sizeof(GeometryInfoDev), "geometry info layouts");
            memcpy(&f.g, &c->h_geoms[g], sizeof(f.g));
            for (int col = 0; col < 4; col++)
                for (int row = 0; row < 3; row++) f.m[3 * col + row] = m[4 * col + row];
            f.identity = identity ? 1u : 0u;
            f.geom = g;
            f.instance = (uint32_t)i;
            ShadeGeomDev sg;
            memset(&sg, 0, sizeof(sg));
            for (int q = 0; q < 3; q++) { sg.base_color[q] = f.g.base_color[q]; sg.emission[q] = f.g.emission[q]; }
            sg.tex = f.g.tex;
            sg.metallic = f.g.metallic;
            sg.roughness = f.g.roughness;
            sg.identity = f.identity;
            memcpy(sg.m, f.m, 9 * sizeof(float));
            flat.push_back(f);
            shade.push_back(sg);
            first.push_back((uint32_t)total);
            total += c->h_prim_counts[g];
            if (total > (1ull << 28)) return fail(c, RT3_E_UNSUPPORTED, "more than 2^28 triangles after instancing (leaf references hold 28 bits)");
        }
    }
    const size_t nf = flat.size();
    if (int r = dev_alloc(c, c->d_geoms, nf)) return r;
    if (int r = dev_alloc(c, c->d_shade_geoms, nf)) return r;
    if (int r = dev_alloc(c, c->d_first_prim, nf)) return r;
    if (int r = dev_alloc(c, c->d_prim_geom, (size_t)total)) return r;
    if (nf) {
        HIPC(c, hipMemcpy(c->d_geoms.get(), flat.data(), nf * sizeof(FlatGeomDev), hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(c->d_shade_geoms.get(), shade.data(), nf * sizeof(ShadeGeomDev), hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(c->d_first_prim.get(), first.data(), nf * 4, hipMemcpyHostToDevice));
        if (nf * sizeof(FlatGeomDev) > (64u << 10)) c->bulk_copies += 3;
        launch_prim_geom(c->stream, c->d_first_prim.get(), (uint32_t)nf, (uint32_t)total, c->d_prim_geom.get());
        HIPC(c, hipGetLastError());
    }
    c->n_flat_geoms = (uint32_t)nf;
    c->n_flat_prims = (uint32_t)total;
    return RT3_OK;
}
// The device tables of the "motion" pass for the built structure: per instance its previous matrix, per flattened geometry its slot --
// kMotionUnmoved, or its instance's index if that instance moved (the 12 stored floats of the two matrices differ in some word), or that
// index | kMotionDeformed if the geometry is deformed (deform_flags).  Without previous transforms a deformed geometry's record holds its
// instance's current matrix.  Remade when the previous transforms, the snapshot, the vertices or the structure changed; the count is
// checked at every launch.
static int motion_tables(rt3_ctx* c) {
    rt3_instance whole;
    const auto [inst, n_inst] = placements(c, whole);
    const size_t n = c->mo_prev.size() / 16;
    if (n != 0 && n != n_inst)
        return fail(c, RT3_E_STATE, "motion: " + std::to_string(n) + " previous transforms (rt3_scene_set_prev_transforms) for a structure of " +
                                        std::to_string(n_inst) + " instance(s)");
    if (int r = deform_flags(c)) return r;
    if (!c->mo_dirty && c->mo_stamp == c->accel_stamp) return RT3_OK;
    const bool deformed_any = std::any_of(c->h_deformed.begin(), c->h_deformed.end(), [](uint32_t f) { return f != 0; });
    std::vector<MotionPrevDev> rec(n || deformed_any ? n_inst : 0);
    std::vector<uint32_t> slot;
    bool any = false, any_deformed = false;
    for (size_t i = 0; i < rec.size(); i++) {
        const float *cm = inst[i].transform, *pm = n ? &c->mo_prev[16 * i] : cm;
        float cur[12];
        memset(&rec[i], 0, sizeof(rec[i]));
        for (int col = 0; col < 4; col++)
            for (int row = 0; row < 3; row++) {
                rec[i].m[3 * col + row] = pm[4 * col + row];
                cur[3 * col + row] = cm[4 * col + row];
            }
        rec[i].identity = memcmp(pm, kIdentity, sizeof(kIdentity)) == 0 ? 1u : 0u;
        const bool moved = memcmp(rec[i].m, cur, sizeof(cur)) != 0;  // word for word: -0 is not +0
        for (uint32_t k = 0; k < inst[i].geometry_count; k++) {
            const uint32_t g = inst[i].geometry_first + k;
            const bool deformed = g < c->h_deformed.size() && c->h_deformed[g];
            slot.push_back(deformed ? ((uint32_t)i | kMotionDeformed) : (moved ? (uint32_t)i : kMotionUnmoved));
            any = any || moved || deformed;
            any_deformed = any_deformed || deformed;
        }
    }
    if (any) {
        HIPC(c, hipStreamSynchronize(c->stream));  // an earlier launch may still read the old tables
        if (int r = dev_alloc(c, c->d_mo_prev, rec.size())) return r;
        if (int r = dev_alloc(c, c->d_mo_slot, slot.size())) return r;
        HIPC(c, hipMemcpy(c->d_mo_prev.get(), rec.data(), rec.size() * sizeof(MotionPrevDev), hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(c->d_mo_slot.get(), slot.data(), slot.size() * 4, hipMemcpyHostToDevice));
    }
    c->mo_any_moved = any;
    c->mo_any_deformed = any_deformed;
    c->mo_dirty = false;
    c->mo_stamp = c->accel_stamp;
    return RT3_OK;
}
// the shading records of the flattened world, remade only when what they depend on has changed since they were made
static int make_shade_records(rt3_ctx* c) {
    rt3_instance whole;
    const auto [inst, n_inst] = placements(c, whole);
    std::vector<uint64_t> key{c->content_gen};
    for (size_t i = 0; i < n_inst; i++) {
        key.push_back(inst[i].geometry_first);
        key.push_back(inst[i].geometry_count);
    }
    ShadeRecords& s = c->shade;
    if (key == s.key) return RT3_OK;
    s.key.clear();  // until the new records are in place
    if (!s.rec || !s.uv || s.n != c->n_flat_prims) {  // (a refit rewrites them in place)
        if (int r = dev_alloc(c, s.rec, (size_t)c->n_flat_prims)) return r;
        if (int r = dev_alloc(c, s.uv, 3 * (size_t)c->n_flat_prims)) return r;
        s.n = c->n_flat_prims;
    }
    launch_tri_shade(c->stream, world_tables(c), c->n_flat_prims, s.rec.get(), s.uv.get());
    HIPC(c, hipGetLastError());
    s.key = std::move(key);
    return RT3_OK;
}
// The emitter table (RT3_F_NEE_EMISSIVE, rt3_lights.hip) of the current structure, remade when a build, refit or import has happened since.  The
// host walks only the flattened geometries (as flatten_world does) to find the emissive ones; the table itself is made on the GPU.
static int ensure_lights(rt3_ctx* c) {
    if (int r = check_accel_current(c)) return r;
    if (c->lights.stamp == c->accel_stamp) return RT3_OK;
    rt3_instance whole;
    const auto [inst, n_inst] = placements(c, whole);
    std::vector<uint32_t> geom_base, eg_geom, eg_first;
    uint64_t n = 0;
    for (size_t i = 0; i < n_inst; i++)
        for (uint32_t k = 0; k < inst[i].geometry_count; k++) {
            const uint32_t g = inst[i].geometry_first + k;
            const float* em = c->h_geoms[g].emission;
            const bool masked = any_cutoff(c) && c->h_cutoffs[g] > 0.0f;  // left out: its points may be cut away
            const bool emissive = (em[0] != 0.0f || em[1] != 0.0f || em[2] != 0.0f) && c->h_prim_counts[g] > 0 && !masked;
            geom_base.push_back(emissive ? (uint32_t)n : kMiss);
            if (emissive) {
                eg_geom.push_back((uint32_t)(geom_base.size() - 1));
                eg_first.push_back((uint32_t)n);
                n += c->h_prim_counts[g];
            }
        }
    if (geom_base.size() != c->n_flat_geoms) return fail(c, RT3_E_STATE, "emitter table: the placements changed since rt3_accel_build");
    HIPC(c, hipSetDevice(c->device));
    const hipError_t e = lights_build(c->stream, world_tables(c), geom_base, eg_geom, eg_first, (uint32_t)n, &c->lights);
    if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("emitter table: ") + hipGetErrorString(e));
    c->lights.stamp = c->accel_stamp;
    return RT3_OK;
}

// worst-case stack use of the near-first walk over a tree of `depth` levels: (children per node - 1) entries per level above the leaves
static uint32_t stack_entries(uint32_t width, uint32_t depth) { return depth > 1 ? (width - 1) * (depth - 1) : 0; }

// ---- two-level structure (RT3_OPT_INSTANCE_MODE 1): shared bottom trees under a top tree over instance records
// Conservativeness of the two-level boxes: every box is grown by kTlPad times a bound on the magnitudes involved,
// three orders above the rounding it must cover; matrices with ||M3|| ||M3^-1|| above kTlMaxCondition are refused
constexpr double kTlPad = 1.0 / 4096.0;
constexpr double kTlMaxCondition = 1048576.0;
static void tl_reset(rt3_ctx* c) {
    c->tl.valid = false;
    c->tl.meshes.clear();
    c->tl.n_meshes = c->tl.n_built = c->tl.n_top = 0;
    c->tl.n_alloc_nodes = 0;
}
static void free_accel(rt3_ctx* c) {
    c->bvh = LbvhResult{};
    tl_reset(c);
}
// the union of the child boxes of a quantised 64-byte node, decoded as the traversal decodes them (origin + q * step), in double
static void quantised_node_box(const uint32_t* w, double box[6]) {
    float org[3], step[3];
    memcpy(org, w, 12);
    memcpy(&step[0], &w[3], 4);
    memcpy(&step[1], &w[14], 4);
    memcpy(&step[2], &w[15], 4);
    for (int a = 0; a < 3; a++) {
        box[a] = INFINITY;
        box[3 + a] = -INFINITY;
    }
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(w + 4);
    for (int k = 0; k < 4; k++) {
        if (w[10 + k] == 0xFFFFFFFFu) continue;
        for (int a = 0; a < 3; a++) {
            const double lo = (double)org[a] + (double)bytes[6 * k + a] * (double)step[a], hi = (double)org[a] + (double)bytes[6 * k + 3 + a] * (double)step[a];
            box[a] = lo < box[a] ? lo : box[a];
            box[3 + a] = hi > box[3 + a] ? hi : box[3 + a];
        }
    }
}
// the tables of a bottom tree over the geometries [first, first + count) as uploaded: identity matrices, local primitive ids
static hipError_t make_mesh_tables(rt3_ctx* c, const TlMesh& m, MeshTables* t) {
    std::vector<FlatGeomDev> tbl(m.count);
    std::vector<uint32_t> fp(m.count);
    uint32_t tot = 0;
    for (uint32_t k = 0; k < m.count; k++) {
        FlatGeomDev& f = tbl[k];
        memset(&f, 0, sizeof(f));
        memcpy(&f.g, &c->h_geoms[m.first + k], sizeof(f.g));
        f.m[0] = f.m[4] = f.m[8] = 1.0f;
        f.identity = 1u;
        f.geom = m.first + k;
        fp[k] = tot;
        tot += c->h_prim_counts[m.first + k];
    }
    BufLayout plan;
    plan.add(&t->geoms, tbl.size()).add(&t->first_prim, fp.size()).add(&t->prim_geom, m.n_tris);
    RT3_TRY(t->mem.alloc_bytes(plan.bytes()));
    RT3_TRY(plan.carve(t->mem));
    hipError_t e = hipMemcpy(t->geoms, tbl.data(), tbl.size() * sizeof(FlatGeomDev), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t->first_prim, fp.data(), fp.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) launch_prim_geom(c->stream, t->first_prim, m.count, m.n_tris, t->prim_geom);
    return e;
}
// one bottom tree: the geometries [first, first + count) as uploaded
static int tl_build_mesh(rt3_ctx* c, TlMesh& m, LbvhResult* res) {
    MeshTables t;
    hipError_t e = make_mesh_tables(c, m, &t);
    if (e == hipSuccess)
        e = lbvh_build(c->stream, mesh_tables(c, t), m.n_tris, c->opt_leaf_size, 4, 1, c->opt_collapse, c->opt_sah_top, c->build_scratch, res,
                       c->accel_masked ? c->d_geom_mask.get() : nullptr);
    uint32_t root[16];
    if (e == hipSuccess) e = hipMemcpyAsync(root, res->nodes.get(), 64, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("two-level: bottom tree: ") + hipGetErrorString(e));
    m.n_nodes = res->n_nodes;
    m.depth = res->max_depth;
    quantised_node_box(root, m.box);
    return RT3_OK;
}
static float round_down(double x) {
    float f = (float)x;
    return (double)f > x ? std::nextafter(f, -INFINITY) : f;
}
static float round_up(double x) {
    float f = (float)x;
    return (double)f < x ? std::nextafter(f, INFINITY) : f;
}

static int tl_records_and_top(rt3_ctx* c);
static int build_two_level(rt3_ctx* c) {
    if (c->opt_node_width != 4 || c->opt_node_quant != 1)
        return fail(c, RT3_E_UNSUPPORTED, "instance mode 1 (two-level) needs the default node layout: RT3_OPT_NODE_WIDTH 4, RT3_OPT_NODE_QUANT 1");
    TwoLevelState& tl = c->tl;
    if (!tl.valid) free_accel(c);  // what c->bvh holds is a flattened tree (or nothing)
    rt3_instance whole;
    const auto [inst, n_inst] = placements(c, whole);

    // ---- matrices: the inverse (double, then fp32) and its conditioning; meshes = distinct geometry runs that hold triangles
    std::vector<TlInstance> ii(n_inst);
    std::vector<TlMesh> meshes;
    uint32_t total = 0;
    for (size_t i = 0; i < n_inst; i++) {
        const float* m = inst[i].transform;
        double M[3][3];
        for (int r = 0; r < 3; r++)
            for (int k = 0; k < 3; k++) M[r][k] = m[4 * k + r];
        const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
        TlInstance& in = ii[i];
        memcpy(in.m, m, sizeof(in.m));
        in.identity = memcmp(m, kIdentity, sizeof(kIdentity)) == 0;
        if (!(std::fabs(det) > 0.0) || !std::isfinite(1.0 / det))
            return fail(c, RT3_E_UNSUPPORTED, "instance " + std::to_string(i) + ": the upper 3 x 3 of the transform is singular (instance mode 1 needs its inverse)");
        const double id = 1.0 / det;
        in.A[0][0] = (M[1][1] * M[2][2] - M[1][2] * M[2][1]) * id;
        in.A[0][1] = (M[0][2] * M[2][1] - M[0][1] * M[2][2]) * id;
        in.A[0][2] = (M[0][1] * M[1][2] - M[0][2] * M[1][1]) * id;
        in.A[1][0] = (M[1][2] * M[2][0] - M[1][0] * M[2][2]) * id;
        in.A[1][1] = (M[0][0] * M[2][2] - M[0][2] * M[2][0]) * id;
        in.A[1][2] = (M[0][2] * M[1][0] - M[0][0] * M[1][2]) * id;
        in.A[2][0] = (M[1][0] * M[2][1] - M[1][1] * M[2][0]) * id;
        in.A[2][1] = (M[0][1] * M[2][0] - M[0][0] * M[2][1]) * id;
        in.A[2][2] = (M[0][0] * M[1][1] - M[0][1] * M[1][0]) * id;
        for (int r = 0; r < 3; r++) {
            for (int k = 0; k < 3; k++) in.A[r][k] = (double)(float)in.A[r][k];  // what the record holds
            in.b[r] = (double)(float)-(in.A[r][0] * m[12] + in.A[r][1] * m[13] + in.A[r][2] * m[14]);
        }
        in.nA = in.nM = 0.0;
        for (int r = 0; r < 3; r++) {
            in.nA = std::fmax(in.nA, std::fabs(in.A[r][0]) + std::fabs(in.A[r][1]) + std::fabs(in.A[r][2]));
            in.nM = std::fmax(in.nM, std::fabs(M[r][0]) + std::fabs(M[r][1]) + std::fabs(M[r][2]));
        }
        if (!std::isfinite(in.nA) || in.nA * in.nM > kTlMaxCondition)
            return fail(c, RT3_E_UNSUPPORTED, "instance " + std::to_string(i) + ": the transform is too badly conditioned for instance mode 1 (||M|| ||M^-1|| > 2^20)");
        in.prim_base = total;
        uint32_t cnt = 0;
        for (uint32_t k = 0; k < inst[i].geometry_count; k++) cnt += c->h_prim_counts[inst[i].geometry_first + k];
        total += cnt;
        in.mesh = ~0u;
        if (cnt == 0) continue;
        for (size_t q = 0; q < meshes.size(); q++)
            if (meshes[q].first == inst[i].geometry_first && meshes[q].count == inst[i].geometry_count) in.mesh = (uint32_t)q;
        if (in.mesh == ~0u) {
            TlMesh nm;
            memset(&nm, 0, sizeof(nm));
            nm.first = inst[i].geometry_first;
            nm.count = inst[i].geometry_count;
            nm.n_tris = cnt;
            in.mesh = (uint32_t)meshes.size();
            meshes.push_back(nm);
        }
    }
    uint32_t n_ne = 0;  // instances that place triangles: they get records and top-tree leaves, the others are left out
    for (auto& in : ii) n_ne += in.mesh != ~0u ? 1u : 0u;
    if (n_ne >= (1u << 26)) return fail(c, RT3_E_UNSUPPORTED, "instance mode 1: too many instances");
    const uint32_t top_cap = n_ne ? n_ne : 1u;  // a four-wide tree over n leaves has at most max(1, n - 1) nodes
    const uint32_t head = top_cap + 2u * n_ne;

    // ---- bottom trees: kept while the meshes, the generation and the head are what the last build had
    bool same = tl.valid && tl.gen == c->content_gen && tl.head == head && tl.meshes.size() == meshes.size();
    for (size_t q = 0; same && q < meshes.size(); q++) same = tl.meshes[q].first == meshes[q].first && tl.meshes[q].count == meshes[q].count;
    tl.n_built = 0;
    if (same) {
        meshes = tl.meshes;
    } else {
        const bool reuse = tl.valid && tl.gen == c->content_gen;
        std::vector<LbvhResult> built(meshes.size());
        std::vector<int> from(meshes.size(), -1);
        int rc = RT3_OK;
        for (size_t q = 0; q < meshes.size() && rc == RT3_OK; q++) {
            for (size_t o = 0; reuse && o < tl.meshes.size(); o++)
                if (tl.meshes[o].first == meshes[q].first && tl.meshes[o].count == meshes[q].count) from[q] = (int)o;
            if (from[q] >= 0) {
                const TlMesh& om = tl.meshes[from[q]];
                meshes[q].n_nodes = om.n_nodes;
                meshes[q].depth = om.depth;
                memcpy(meshes[q].box, om.box, sizeof(om.box));
            } else {
                rc = tl_build_mesh(c, meshes[q], &built[q]);
                tl.n_built++;
            }
        }
        uint64_t nodes_total = head, tris_total = 0;
        for (auto& m : meshes) {
            m.node_off = (uint32_t)nodes_total;
            m.tri_off = (uint32_t)tris_total;
            nodes_total += m.n_nodes;
            tris_total += m.n_tris;
        }
        if (rc == RT3_OK && (nodes_total >= (1ull << 29) || tris_total > (1ull << 28)))
            rc = fail(c, RT3_E_UNSUPPORTED, "instance mode 1: the bottom trees exceed the 28-bit references");
        DevBuf<float4> nodes, tris;
        hipError_t e = hipSuccess;
        if (rc == RT3_OK) {
            e = nodes.alloc_bytes((size_t)nodes_total * 64);
            if (e == hipSuccess) e = tris.alloc_bytes((size_t)tris_total * 48 + 128);  // + the traversal's over-read slack
            if (e == hipSuccess) e = hipMemsetAsync((char*)tris.get() + (size_t)tris_total * 48, 0, 128, c->stream);
            for (size_t q = 0; e == hipSuccess && q < meshes.size(); q++) {
                const TlMesh& m = meshes[q];
                if (from[q] >= 0) {
                    const TlMesh& om = tl.meshes[from[q]];
                    tlas_rebase_nodes(c->stream, c->bvh.nodes.get() + 4 * (size_t)om.node_off, nodes.get() + 4 * (size_t)m.node_off, m.n_nodes, om.node_off,
                                      m.node_off, om.tri_off, m.tri_off);
                    e = hipMemcpyAsync(tris.get() + 3 * (size_t)m.tri_off, c->bvh.tris.get() + 3 * (size_t)om.tri_off, (size_t)m.n_tris * 48, hipMemcpyDeviceToDevice,
                                       c->stream);
                } else {
                    tlas_rebase_nodes(c->stream, built[q].nodes.get(), nodes.get() + 4 * (size_t)m.node_off, m.n_nodes, 0u, m.node_off, 0u, m.tri_off);
                    e = hipMemcpyAsync(tris.get() + 3 * (size_t)m.tri_off, built[q].tris.get(), (size_t)m.n_tris * 48, hipMemcpyDeviceToDevice, c->stream);
                }
            }
            if (e == hipSuccess) e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) rc = fail(c, RT3_E_HIP, std::string("two-level: bottom trees: ") + hipGetErrorString(e));
        }
        if (rc != RT3_OK) {
            free_accel(c);
            return rc;
        }
        c->bvh.nodes = std::move(nodes);
        c->bvh.tris = std::move(tris);
        tl.meshes = meshes;
        tl.head = head;
        tl.gen = c->content_gen;
        tl.n_alloc_nodes = (uint32_t)nodes_total;
        tl.valid = true;
    }
    tl.inst = std::move(ii);
    tl.n_placed = n_ne;
    tl.top_cap = top_cap;
    return tl_records_and_top(c);
}

// The instance records and world boxes (host, a few KiB), then the top tree (GPU), over bottom trees that are in place: the tail of a
// two-level build, and what a refit redoes after the bottom trees' boxes moved.
static int tl_records_and_top(rt3_ctx* c) {
    TwoLevelState& tl = c->tl;
    const std::vector<TlInstance>& ii = tl.inst;
    const std::vector<TlMesh>& meshes = tl.meshes;  // (free_accel clears it: nothing reads it after that)
    const size_t n_inst = ii.size();
    const uint32_t n_ne = tl.n_placed, top_cap = tl.top_cap;
    std::vector<uint32_t> rec((size_t)32 * n_ne);
    std::vector<float> boxes((size_t)6 * n_ne);
    uint32_t slot = 0, max_bottom = 0;
    for (size_t i = 0; i < n_inst; i++) {
        const TlInstance& in = ii[i];
        if (in.mesh == ~0u) continue;
        const TlMesh& ms = meshes[in.mesh];
        max_bottom = ms.depth > max_bottom ? ms.depth : max_bottom;
        const float* m = in.m;
        const double nA = in.nA, nM = in.nM;
        double tM = 0.0, Bobj = 0.0, lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int r = 0; r < 3; r++) tM = std::fmax(tM, std::fabs((double)m[12 + r]));
        for (int k = 0; k < 6; k++) Bobj = std::fmax(Bobj, std::fabs(ms.box[k]));
        for (int corner = 0; corner < 8; corner++) {
            const double p[3] = {ms.box[(corner & 1) ? 3 : 0], ms.box[(corner & 2) ? 4 : 1], ms.box[(corner & 4) ? 5 : 2]};
            for (int r = 0; r < 3; r++) {
                const double w = (double)m[r] * p[0] + (double)m[4 + r] * p[1] + (double)m[8 + r] * p[2] + (double)m[12 + r];
                lo[r] = std::fmin(lo[r], w);
                hi[r] = std::fmax(hi[r], w);
            }
        }
        double Bw = 0.0;
        for (int r = 0; r < 3; r++) Bw = std::fmax(Bw, std::fmax(std::fabs(lo[r]), std::fabs(hi[r])));
        const double widen = kTlPad * (Bw + nM * Bobj + tM);
        for (int r = 0; r < 3; r++) {
            boxes[6 * slot + r] = round_down(lo[r] - widen);
            boxes[6 * slot + 3 + r] = round_up(hi[r] + widen);
        }
        uint32_t* a = &rec[32 * (size_t)slot];
        float fa[12], ff[12];
        for (int k = 0; k < 3; k++)
            for (int r = 0; r < 3; r++) fa[3 * k + r] = (float)in.A[r][k];
        for (int r = 0; r < 3; r++) fa[9 + r] = (float)in.b[r];
        for (int k = 0; k < 4; k++)
            for (int r = 0; r < 3; r++) ff[3 * k + r] = m[4 * k + r];
        memcpy(a, fa, 48);
        a[12] = ms.node_off;
        a[13] = (ii[i].prim_base + 0u) | (in.identity ? 0x80000000u : 0u);
        const float pad_abs = round_up(kTlPad * (nA * (2.0 * Bw + nM * Bobj + tM) + Bobj)), pad_rel = round_up(kTlPad * (2.0 * nA + 1.0));
        memcpy(&a[14], &pad_abs, 4);
        memcpy(&a[15], &pad_rel, 4);
        memcpy(a + 16, ff, 48);
        slot++;
    }
    if (n_ne == 0) {  // nothing placed: every ray misses (the kernels' empty-scene path)
        c->bvh.nodes.reset();
        c->bvh.tris.reset();
        c->bvh.top.reset();
        tl.valid = false;
        tl.n_meshes = 0;
        tl.n_top = 0;
        c->bvh.n_nodes = c->bvh.n_tris = c->bvh.n_top = 0;
        c->bvh.max_depth = 0;
        c->bvh.node_bytes = 64;
        c->bvh.layout = kLayoutTwoLevel;
        return RT3_OK;
    }
    const size_t rec_bytes = rec.size() * 4;
    HIPC(c, hipMemcpyAsync(c->bvh.nodes.get() + 4 * (size_t)top_cap, rec.data(), rec_bytes, hipMemcpyHostToDevice, c->stream));
    if (rec_bytes > (64u << 10)) c->bulk_copies += 1;
    // the top build's inputs: boxes, degenerate triangles, a one-entry identity table, prim_geom = 0 and then first_prim = 0
    float *boxes_d = nullptr, *verts = nullptr;
    uint32_t *idx = nullptr, *zeros = nullptr;
    FlatGeomDev* tbl = nullptr;
    BufLayout plan;
    plan.add(&boxes_d, boxes.size()).add(&verts, (size_t)n_ne * 24).add(&idx, (size_t)n_ne * 3).add(&tbl, 1).add(&zeros, (size_t)n_ne + 1);
    HIPC(c, tl.scratch.grow_bytes(plan.bytes()));
    HIPC(c, plan.carve(tl.scratch));
    FlatGeomDev tg;
    memset(&tg, 0, sizeof(tg));
    tg.m[0] = tg.m[4] = tg.m[8] = 1.0f;
    tg.identity = 1u;
    HIPC(c, hipMemcpyAsync(boxes_d, boxes.data(), boxes.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (boxes.size() * 4 > (64u << 10)) c->bulk_copies += 1;
    HIPC(c, hipMemcpyAsync(tbl, &tg, sizeof(tg), hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemsetAsync(zeros, 0, ((size_t)n_ne + 1) * 4, c->stream));
    tlas_box_tris(c->stream, boxes_d, n_ne, verts, idx);
    LbvhResult top;
    hipError_t e = lbvh_build(c->stream, GeomTables{verts, idx, tbl, zeros, zeros + n_ne}, n_ne, 1u, 4u, 1u, c->opt_collapse, 1u, c->build_scratch, &top);
    if (e == hipSuccess && top.n_nodes > top_cap) e = hipErrorInvalidValue;  // cannot happen (see top_cap); never write past the top's region
    if (e == hipSuccess) {
        tlas_emit_top(c->stream, top.nodes.get(), top.n_nodes, top.tris.get(), top_cap, c->bvh.nodes.get());
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = lbvh_make_top(c->stream, c->bvh.nodes.get(), tl.n_alloc_nodes, c->bvh.top, &c->bvh.n_top);
    const uint32_t top_nodes = top.n_nodes, top_depth = top.max_depth;
    if (e != hipSuccess) {
        free_accel(c);
        return fail(c, RT3_E_HIP, std::string("two-level: top tree: ") + hipGetErrorString(e));
    }
    // stack bound: the top walk's entries below the instance leaf, then the bottom walk's (the hand-over pushes nothing)
    const uint32_t stack_need = stack_entries(4, top_depth) + stack_entries(4, max_bottom);
    if (stack_need > kMaxStack) {
        free_accel(c);
        return fail(c, RT3_E_DEPTH, "two-level structure needs " + std::to_string(stack_need) + " stack entries (top " + std::to_string(top_depth) +
                                        " levels + bottom " + std::to_string(max_bottom) + "), the traversal kernels hold " + std::to_string(kMaxStack));
    }
    uint32_t bottom_nodes = 0, bottom_tris = 0;
    for (auto& m : meshes) {
        bottom_nodes += m.n_nodes;
        bottom_tris += m.n_tris;
    }
    tl.n_meshes = (uint32_t)meshes.size();
    tl.n_top = top_nodes;
    c->bvh.n_nodes = top_nodes + bottom_nodes;
    c->bvh.n_tris = bottom_tris;
    c->bvh.max_depth = top_depth + max_bottom;
    c->bvh.node_bytes = 64;
    c->bvh.layout = kLayoutTwoLevel;
    return RT3_OK;
}

// ---- acceleration structure
// The alpha-mask tables of a build: per uploaded geometry the triangle records' last two words {cutoff bits, slot} and
// per masked geometry (slot) {texture index, base_color[3] bits}.  c->accel_masked: some placed geometry with triangles is masked.
static int make_alpha_tables(rt3_ctx* c) {
    c->accel_masked = false;
    if (!any_cutoff(c)) return RT3_OK;
    if (c->opt_node_width != 4 || c->opt_node_quant != 1)
        return fail(c, RT3_E_UNSUPPORTED, "alpha-masked geometry needs the default node layout (RT3_OPT_NODE_WIDTH 4, RT3_OPT_NODE_QUANT 1)");
    std::vector<uint2> mask(c->n_geoms, make_uint2(0u, 0u)), table;
    for (uint32_t g = 0; g < c->n_geoms; g++) {
        if (!(c->h_cutoffs[g] > 0.0f)) continue;
        uint32_t cb, ab;
        memcpy(&cb, &c->h_cutoffs[g], 4);
        memcpy(&ab, &c->h_geoms[g].base_color[3], 4);
        mask[g] = make_uint2(cb, (uint32_t)table.size());
        table.push_back(make_uint2((uint32_t)c->h_geoms[g].base_color_texture_index, ab));
    }
    rt3_instance whole;
    const auto [inst, n_inst] = placements(c, whole);
    for (size_t i = 0; i < n_inst && !c->accel_masked; i++)
        for (uint32_t k = 0; k < inst[i].geometry_count; k++) {
            const uint32_t g = inst[i].geometry_first + k;
            if (mask[g].x != 0u && c->h_prim_counts[g] > 0) c->accel_masked = true;
        }
    if (int r = dev_alloc(c, c->d_geom_mask, mask.size())) return r;
    if (int r = dev_alloc(c, c->d_alpha, table.size())) return r;
    HIPC(c, hipMemcpy(c->d_geom_mask.get(), mask.data(), mask.size() * sizeof(uint2), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->d_alpha.get(), table.data(), table.size() * sizeof(uint2), hipMemcpyHostToDevice));
    return RT3_OK;
}
// the end of a successful build or refit: the shading records, then the structure goes live
static int accel_finish(rt3_ctx* c, uint32_t* out_handle) {
    if (int r = make_shade_records(c)) return r;
    HIPC(c, hipStreamSynchronize(c->stream));
    c->stats.accel_bulk_copies += c->bulk_copies;
    c->bulk_copies = 0;
    c->accel_built = true;
    c->accel_stale = false;
    c->accel_stamp++;                 // the emitter table follows (ensure_lights)
    c->accel_topo_gen = c->topo_gen;  // (unchanged by a refit, which needs the build's)
    if (out_handle) *out_handle = (RT3_TAG_ACCEL << 30) | 0u;
    return RT3_OK;
}
int rt3_accel_build(rt3_ctx* c, uint32_t* out_handle) {
    if (!c) return RT3_E_INVALID;
    HIPC(c, hipSetDevice(c->device));
    if (c->n_prims && (!c->d_verts || !c->d_indices)) return fail(c, RT3_E_STATE, "set vertices, indices and geometry before rt3_accel_build");
    // the vertex / index buffers may have been replaced since rt3_scene_set_geometry checked its ranges against them
    std::vector<std::pair<uint32_t, uint32_t>> spans;  // (the indices may have been replaced since rt3_scene_set_geometry)
    if (int r = validate_geometry(c, c->h_geoms.data(), c->h_prim_counts.data(), (uint32_t)c->h_geoms.size(), &spans)) return r;
    c->h_geom_span.swap(spans);
    HIPC(c, hipStreamSynchronize(c->stream));
    const auto t_build0 = std::chrono::steady_clock::now();
    // until the rebuild has succeeded: a failed one (the geometry tables reallocated by flatten_world included) must leave
    // RT3_E_STATE behind, not an empty tree or one that points at freed tables
    c->accel_built = false;
    c->accel_stale = false;
    c->refit_planned = false;
    if (int r = flatten_world(c)) return r;
    if (int r = make_alpha_tables(c)) return r;
    if (c->opt_instance_mode == 1) {
        if (int r = build_two_level(c)) return r;
    } else {
        free_accel(c);  // the old tree (two-level or not) goes before the new one is allocated
        hipError_t e = lbvh_build(c->stream, world_tables(c), c->n_flat_prims, c->opt_leaf_size, c->opt_node_width, c->opt_node_quant, c->opt_collapse,
                                  c->opt_sah_top, c->build_scratch, &c->bvh, c->accel_masked ? c->d_geom_mask.get() : nullptr);
        if (c->build_scratch.capacity_bytes() > ((size_t)1 << 30)) c->build_scratch.reset();  // a big scene's scratch is not worth keeping resident
        if (e != hipSuccess) {
            free_accel(c);  // (what the failed build allocated)
            return fail(c, RT3_E_HIP, std::string("lbvh_build: ") + hipGetErrorString(e));
        }
        const uint32_t stack_need = stack_entries(c->opt_node_width, c->bvh.max_depth);
        if (stack_need > kMaxStack) {
            const int rc = fail(c, RT3_E_DEPTH, "LBVH with " + std::to_string(c->bvh.max_depth) + " levels needs " + std::to_string(stack_need) +
                                                    " stack entries, the traversal kernels hold " + std::to_string(kMaxStack));
            free_accel(c);  // (after the message: it clears max_depth)
            return rc;
        }
    }
    if (int r = accel_finish(c, out_handle)) return r;
    c->stats.accel_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_build0).count();
    return RT3_OK;
}
int rt3_accel_info(rt3_ctx* c, uint32_t* n_nodes, uint32_t* n_tris, uint32_t* max_depth, uint32_t* node_bytes) {
    if (!c || !c->accel_built) return fail(c, RT3_E_STATE, "no acceleration structure built");
    if (n_nodes) *n_nodes = c->bvh.n_nodes;
    if (n_tris) *n_tris = c->bvh.n_tris;
    if (max_depth) *max_depth = c->bvh.max_depth;
    if (node_bytes) *node_bytes = c->bvh.node_bytes;
    return RT3_OK;
}
int rt3_accel_levels(rt3_ctx* c, uint32_t* n_meshes, uint32_t* n_meshes_built, uint32_t* n_top_nodes, uint64_t* accel_bytes) {
    if (!c || !c->accel_built) return fail(c, RT3_E_STATE, "no acceleration structure built");
    const bool two = c->bvh.layout == kLayoutTwoLevel;
    if (n_meshes) *n_meshes = two ? c->tl.n_meshes : 0u;
    if (n_meshes_built) *n_meshes_built = two ? c->tl.n_built : 0u;
    if (n_top_nodes) *n_top_nodes = two ? c->tl.n_top : 0u;
    if (accel_bytes) {  // what the traversal kernels read: node array (two-level: top tree, instance records, bottom trees), triangle records, LDS top copy
        const uint64_t nodes = !c->bvh.nodes ? 0u : (two ? (uint64_t)c->tl.n_alloc_nodes * 64u : (uint64_t)c->bvh.n_nodes * c->bvh.node_bytes);
        *accel_bytes = nodes + (!c->bvh.tris ? 0u : (uint64_t)c->bvh.n_tris * 48u) + (uint64_t)c->bvh.n_top * 64u;
    }
    return RT3_OK;
}
int rt3_accel_download(rt3_ctx* c, void* nodes, size_t nodes_bytes, void* tris, size_t tris_bytes) {
    if (int r = check_accel_current(c, "no acceleration structure built")) return r;
    if (c->bvh.layout == kLayoutTwoLevel) return fail(c, RT3_E_UNSUPPORTED, "accel_download: not for the two-level structure (RT3_OPT_INSTANCE_MODE 1)");
    if (nodes) {
        if (nodes_bytes != (size_t)c->bvh.n_nodes * c->bvh.node_bytes) return fail(c, RT3_E_INVALID, "nodes_bytes mismatch");
        if (nodes_bytes) HIPC(c, hipMemcpy(nodes, c->bvh.nodes.get(), nodes_bytes, hipMemcpyDeviceToHost));
    }
    if (tris) {
        if (tris_bytes != (size_t)c->bvh.n_tris * 48) return fail(c, RT3_E_INVALID, "tris_bytes mismatch");
        if (tris_bytes) HIPC(c, hipMemcpy(tris, c->bvh.tris.get(), tris_bytes, hipMemcpyDeviceToHost));
    }
    return RT3_OK;
}
// The counterpart of rt3_accel_download: install a tree somebody else built over the SAME flattened triangles (an offline builder,
// a cache of an earlier run; Vulkan's vkCmdCopyMemoryToAccelerationStructureKHR plays this role for the reference's driver).  Default
// layout only (64-byte quantised four-wide nodes, 48-byte triangle records).  Every reference is checked on the host before the
// kernels may follow it: in range, no node reachable twice (so the walk terminates), depth within the traversal stack.
int rt3_accel_import(rt3_ctx* c, const void* nodes, size_t nodes_bytes, const void* tris, size_t tris_bytes) {
    if (!c || !nodes || !tris) return fail(c, RT3_E_INVALID, "accel_import: NULL argument");
    if (!c->accel_built) return fail(c, RT3_E_STATE, "accel_import: build the scene's own structure first (rt3_accel_build makes the shading records)");
    if (c->bvh.layout == kLayoutTwoLevel) return fail(c, RT3_E_UNSUPPORTED, "accel_import: not for the two-level structure (RT3_OPT_INSTANCE_MODE 1)");
    if (c->bvh.layout != kLayoutWide64Q) return fail(c, RT3_E_UNSUPPORTED, "accel_import: default node layout only");
    if (any_cutoff(c)) return fail(c, RT3_E_UNSUPPORTED, "accel_import: not for a scene with alpha-masked geometry (rt3_scene_set_alpha_cutoffs)");
    if (nodes_bytes == 0 || nodes_bytes % 64 || tris_bytes % 48 || nodes_bytes / 64 > 0x3FFFFFFFull) return fail(c, RT3_E_INVALID, "accel_import: sizes must be multiples of 64 / 48 bytes");
    const uint32_t nn = (uint32_t)(nodes_bytes / 64), nt = (uint32_t)(tris_bytes / 48);
    const uint32_t* w = static_cast<const uint32_t*>(nodes);
    const uint32_t* tw = static_cast<const uint32_t*>(tris);
    for (uint32_t k = 0; k < nt; k++)
        if (tw[12 * (size_t)k + 9] >= c->n_flat_prims) return fail(c, RT3_E_INVALID, "accel_import: triangle record " + std::to_string(k) + " names a primitive the scene does not have");
    std::vector<uint8_t> seen(nn, 0);
    std::vector<std::pair<uint32_t, uint32_t>> st;  // (node, level)
    st.emplace_back(0u, 1u);
    seen[0] = 1;
    uint32_t max_level = 1;
    while (!st.empty()) {
        const auto [node, level] = st.back();
        st.pop_back();
        max_level = level > max_level ? level : max_level;
        for (int k = 0; k < 4; k++) {
            const uint32_t ref = w[16 * (size_t)node + 10 + k];
            if (ref == 0xFFFFFFFFu) continue;
            if (ref & 0x80000000u) {
                const uint64_t first = ref & 0x0FFFFFFFu, cnt = ((ref >> 28) & 7u) + 1u;
                if (first + cnt > nt) return fail(c, RT3_E_INVALID, "accel_import: node " + std::to_string(node) + " references triangles beyond the array");
            } else {
                if (ref >= nn || seen[ref]) return fail(c, RT3_E_INVALID, "accel_import: node " + std::to_string(node) + " references a node out of range or reachable twice");
                seen[ref] = 1;
                st.emplace_back(ref, level + 1);
            }
        }
    }
    const uint32_t depth = max_level + 1;  // levels from the root to the leaf slots, as lbvh_build counts them
    if (stack_entries(4, depth) > kMaxStack) return fail(c, RT3_E_DEPTH, "accel_import: the tree is deeper than the traversal stack supports");
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    DevBuf<float4> d_nodes, d_tris;
    HIPC(c, d_nodes.alloc_bytes(nodes_bytes));
    hipError_t e = d_tris.alloc_bytes(tris_bytes + 128);  // (the walk over-reads a leaf's last record by up to 128 bytes)
    if (e == hipSuccess) e = hipMemset(d_tris.get(), 0, tris_bytes + 128);
    if (e == hipSuccess) e = hipMemcpy(d_nodes.get(), nodes, nodes_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && tris_bytes) e = hipMemcpy(d_tris.get(), tris, tris_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("accel_import: ") + hipGetErrorString(e));
    c->bvh.nodes = std::move(d_nodes);
    c->bvh.tris = std::move(d_tris);
    c->bvh.n_nodes = nn;
    c->bvh.n_tris = nt;
    c->bvh.max_depth = depth;
    c->refit_planned = false;
    c->accel_stamp++;
    e = lbvh_make_top(c->stream, c->bvh.nodes.get(), nn, c->bvh.top, &c->bvh.n_top);
    if (e != hipSuccess) {
        c->accel_built = false;
        return fail(c, RT3_E_HIP, std::string("accel_import: top-of-tree copy: ") + hipGetErrorString(e));
    }
    return RT3_OK;
}

// ---- refit (rt3_refit.hip): the last build's trees, their boxes and triangle records recomputed from the current vertices
struct RefitScratch {
    uint32_t* bounds;
    float *nbox, *tbox;
};
static int refit_scratch(rt3_ctx* c, size_t n_nodes, size_t n_tris, RefitScratch* s) {
    BufLayout plan;
    plan.add(&s->bounds, 6).add(&s->nbox, 6 * n_nodes).add(&s->tbox, 6 * n_tris);
    HIPC(c, c->refit_scratch.grow_bytes(plan.bytes()));
    HIPC(c, plan.carve(c->refit_scratch));
    return RT3_OK;
}
static int refit_flat(rt3_ctx* c) {
    LbvhResult& b = c->bvh;
    if (!b.n_nodes) return RT3_OK;
    if (!c->refit_planned) {
        c->refit_trees.clear();
        c->refit_trees.resize(1);
        const hipError_t e = refit_plan(c->stream, b.nodes.get(), 0u, b.n_nodes, b.max_depth, &c->refit_trees[0]);
        if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("accel_refit: plan: ") + hipGetErrorString(e));
        c->refit_planned = true;
    }
    RefitScratch s;
    if (int r = refit_scratch(c, b.n_nodes, b.n_tris, &s)) return r;
    hipError_t e = refit_tree(c->stream, c->refit_trees[0], world_tables(c), c->n_flat_prims, 0u, b.n_tris, b.nodes.get(), b.tris.get(), s.bounds, s.nbox,
                              s.tbox);
    if (e == hipSuccess) e = lbvh_make_top(c->stream, b.nodes.get(), b.n_nodes, b.top, &b.n_top);
    if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("accel_refit: ") + hipGetErrorString(e));
    return RT3_OK;
}
// instance mode 1: every bottom tree in the combined arrays (object space, its own bounds and pad, as tl_build_mesh builds it), then the
// instance records and the top tree over the bottom trees' new root boxes
static int refit_two_level(rt3_ctx* c) {
    TwoLevelState& tl = c->tl;
    tl.n_built = 0;
    if (!tl.valid) return RT3_OK;  // nothing placed: no trees
    const std::vector<TlMesh>& meshes = tl.meshes;
    const size_t nm = meshes.size();
    if (!c->refit_planned) {
        c->refit_trees.clear();
        c->refit_trees.resize(nm);
        c->refit_tables.clear();
        c->refit_tables.resize(nm);
        for (size_t q = 0; q < nm; q++) {
            const TlMesh& m = meshes[q];
            hipError_t e = make_mesh_tables(c, m, &c->refit_tables[q]);
            if (e == hipSuccess && m.count * sizeof(FlatGeomDev) > (64u << 10)) c->bulk_copies += 1;
            if (e == hipSuccess) e = refit_plan(c->stream, c->bvh.nodes.get(), m.node_off, m.n_nodes, m.depth, &c->refit_trees[q]);
            if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("accel_refit: plan: ") + hipGetErrorString(e));
        }
        c->refit_planned = true;
    }
    RefitScratch s;
    if (int r = refit_scratch(c, tl.n_alloc_nodes, c->bvh.n_tris, &s)) return r;
    std::vector<uint32_t> roots(16 * nm);
    hipError_t e = hipSuccess;
    for (size_t q = 0; e == hipSuccess && q < nm; q++) {
        const TlMesh& m = meshes[q];
        e = refit_tree(c->stream, c->refit_trees[q], mesh_tables(c, c->refit_tables[q]), m.n_tris, m.tri_off, m.n_tris, c->bvh.nodes.get(), c->bvh.tris.get(),
                       s.bounds, s.nbox, s.tbox);
        if (e == hipSuccess) e = hipMemcpyAsync(&roots[16 * q], c->bvh.nodes.get() + 4 * (size_t)m.node_off, 64, hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("accel_refit: bottom trees: ") + hipGetErrorString(e));
    for (size_t q = 0; q < nm; q++) quantised_node_box(&roots[16 * q], tl.meshes[q].box);
    tl.gen = c->content_gen;  // the bottom trees now match the vertices: a later build that only moved instances keeps them
    return tl_records_and_top(c);
}
int rt3_accel_refit(rt3_ctx* c, uint32_t* out_handle) {
    if (!c) return RT3_E_INVALID;
    if (c->opt_node_width != 4 || c->opt_node_quant != 1)
        return fail(c, RT3_E_UNSUPPORTED, "accel_refit: default node layout only (RT3_OPT_NODE_WIDTH 4, RT3_OPT_NODE_QUANT 1)");
    if (!c->accel_built || c->accel_topo_gen != c->topo_gen)
        return fail(c, RT3_E_STATE, "accel_refit: no acceleration structure for the current scene (only rt3_scene_update_vertices may come between rt3_accel_build and a refit)");
    const bool two = c->bvh.layout == kLayoutTwoLevel;
    if (!two && c->bvh.layout != kLayoutWide64Q) return fail(c, RT3_E_UNSUPPORTED, "accel_refit: default node layout only");
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    c->accel_built = false;  // until the refit has succeeded: a failed one leaves boxes of neither the old nor the new vertices
    if (int r = two ? refit_two_level(c) : refit_flat(c)) return r;
    return accel_finish(c, out_handle);
}

// ---- resources
int rt3_buffer_create(rt3_ctx* c, size_t bytes, uint32_t* out) {
    if (!c || !out || !bytes) return fail(c, RT3_E_INVALID, "bad buffer size");
    HIPC(c, hipSetDevice(c->device));
    Resource r;
    r.tag = RT3_TAG_BUFFER;
    r.bytes = bytes;
    HIPC(c, r.mem.alloc_bytes(bytes));
    r.ptr = r.mem.get();
    HIPC(c, hipMemset(r.ptr, 0, bytes));
    c->resources.push_back(std::move(r));
    *out = (RT3_TAG_BUFFER << 30) | (uint32_t)(c->resources.size() - 1);
    return RT3_OK;
}
int rt3_image_create(rt3_ctx* c, uint32_t w, uint32_t h, uint32_t format, uint32_t* out) {
    size_t px = format_bytes(format);
    if (!c || !out || !w || !h || !px) return fail(c, RT3_E_INVALID, "bad image size / format");
    HIPC(c, hipSetDevice(c->device));
    Resource r;
    r.tag = RT3_TAG_IMAGE;
    r.w = w; r.h = h; r.format = format;
    r.bytes = (size_t)w * h * px;
    HIPC(c, r.mem.alloc_bytes(r.bytes));
    r.ptr = r.mem.get();
    HIPC(c, hipMemset(r.ptr, 0, r.bytes));
    c->resources.push_back(std::move(r));
    *out = (RT3_TAG_IMAGE << 30) | (uint32_t)(c->resources.size() - 1);
    return RT3_OK;
}
int rt3_image_import(rt3_ctx* c, void* device_ptr, uint32_t w, uint32_t h, uint32_t format, uint32_t* out) {
    size_t px = format_bytes(format);
    if (!c || !out || !device_ptr || !w || !h || !px) return fail(c, RT3_E_INVALID, "bad import");
    Resource r;
    r.tag = RT3_TAG_IMAGE;
    r.w = w; r.h = h; r.format = format;
    r.bytes = (size_t)w * h * px;
    r.ptr = device_ptr;  // borrowed: r.mem stays empty
    c->resources.push_back(std::move(r));
    *out = (RT3_TAG_IMAGE << 30) | (uint32_t)(c->resources.size() - 1);
    return RT3_OK;
}
static Resource* any_res(rt3_ctx* c, uint32_t handle) {
    Resource* r = get_res(c, handle, RT3_TAG_IMAGE);
    return r ? r : get_res(c, handle, RT3_TAG_BUFFER);
}
int rt3_resource_upload(rt3_ctx* c, uint32_t handle, const void* src, size_t bytes) {
    if (!c || !src) return RT3_E_INVALID;
    Resource* r = any_res(c, handle);
    if (!r || bytes != r->bytes) return fail(c, RT3_E_INVALID, "upload: bad handle or size");
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipMemcpy(r->ptr, src, bytes, hipMemcpyHostToDevice));
    return RT3_OK;
}
int rt3_resource_download(rt3_ctx* c, uint32_t handle, void* dst, size_t bytes) {
    if (!c || !dst) return RT3_E_INVALID;
    Resource* r = any_res(c, handle);
    if (!r || bytes != r->bytes) return fail(c, RT3_E_INVALID, "download: bad handle or size");
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    HIPC(c, hipMemcpy(dst, r->ptr, bytes, hipMemcpyDeviceToHost));
    return RT3_OK;
}
int rt3_resource_device_ptr(rt3_ctx* c, uint32_t handle, void** out_ptr, size_t* out_bytes) {
    if (!c || !out_ptr) return RT3_E_INVALID;
    Resource* r = any_res(c, handle);
    if (!r) return fail(c, RT3_E_INVALID, "bad handle");
    *out_ptr = r->ptr;
    if (out_bytes) *out_bytes = r->bytes;
    return RT3_OK;
}

// ---- tiles
int rt3_set_tile_partition(rt3_ctx* c, uint32_t w, uint32_t h, uint32_t rank, uint32_t n_ranks) {
    if (!c) return RT3_E_INVALID;
    HIPC(c, hipSetDevice(c->device));
    PixelList* pl;
    if (int r = get_pixlist(c, w, h, rank, n_ranks, &pl)) return r;
    c->rank = rank;
    c->n_ranks = n_ranks;
    c->part_w = w;
    c->part_h = h;
    return RT3_OK;
}
int rt3_tile_pixel_count(rt3_ctx* c, uint32_t rank, uint32_t n_ranks, uint32_t* out) {
    if (!c || !out || !c->part_w) return fail(c, RT3_E_STATE, "call rt3_set_tile_partition first");
    PixelList* pl;
    if (int r = get_pixlist(c, c->part_w, c->part_h, rank, n_ranks, &pl)) return r;
    *out = pl->count;
    return RT3_OK;
}
int rt3_image_pack_tiles(rt3_ctx* c, uint32_t image, uint32_t rank, uint32_t n_ranks, void* dst) {
    if (!c || !dst) return RT3_E_INVALID;
    Resource* r = get_res(c, image, RT3_TAG_IMAGE);
    if (!r || format_bytes(r->format) != 16) return fail(c, RT3_E_INVALID, "pack_tiles needs a 16-byte-per-pixel image");
    HIPC(c, hipSetDevice(c->device));
    PixelList* pl;
    if (int e = get_pixlist(c, r->w, r->h, rank, n_ranks, &pl)) return e;
    if (pl->count) launch_pack_tiles(c->stream, pl->dev.get(), pl->count, r->w, r->ptr, dst);
    HIPC(c, hipGetLastError());
    return RT3_OK;
}
int rt3_image_unpack_tiles(rt3_ctx* c, uint32_t image, uint32_t rank, uint32_t n_ranks, const void* src) {
    if (!c || !src) return RT3_E_INVALID;
    Resource* r = get_res(c, image, RT3_TAG_IMAGE);
    if (!r || format_bytes(r->format) != 16) return fail(c, RT3_E_INVALID, "unpack_tiles needs a 16-byte-per-pixel image");
    HIPC(c, hipSetDevice(c->device));
    PixelList* pl;
    if (int e = get_pixlist(c, r->w, r->h, rank, n_ranks, &pl)) return e;
    if (pl->count) launch_unpack_tiles(c->stream, pl->dev.get(), pl->count, r->w, src, r->ptr);
    HIPC(c, hipGetLastError());
    return RT3_OK;
}

// ---- frame-end gather over RCCL (north_star).  One rank per context: ncclCommInitRank from a unique id the host
//      application carries from rank 0 to the others over whatever channel it has (the ABI never opens a socket itself).
#define NCCLC(ctx, call)                                                                                          \
    do {                                                                                                          \
        ncclResult_t e_ = (call);                                                                                 \
        if (e_ != ncclSuccess) return fail(ctx, RT3_E_COMM, std::string(#call) + ": " + ncclGetErrorString(e_));  \
    } while (0)
static_assert(sizeof(ncclUniqueId) == RT3_COMM_ID_BYTES, "RT3_COMM_ID_BYTES must be sizeof(ncclUniqueId)");

// A failed send / receive leaves a half-posted exchange behind: peers would block on operations that are never matched and the next
// gather on this communicator would hang with them.  Abort it (ncclCommAbort also ends an open group) and drop it, so that the next
// call answers RT3_E_STATE instead; the host then decides (bench.py: the run fails, nothing is reported as measured).
static int comm_abort(rt3_ctx* c, const std::string& what) {
    if (c->comm) {
        (void)ncclCommAbort(c->comm);
        c->comm = nullptr;
        c->comm_size = 0;
    }
    return fail(c, RT3_E_COMM, what + " (communicator aborted)");
}
static int get_gather_layout(rt3_ctx* c, uint32_t w, uint32_t h, uint32_t root, uint32_t n_ranks, GatherLayout** out) {
    for (auto& g : c->gather_layouts)
        if (g.w == w && g.h == h && g.root == root && g.n_ranks == n_ranks) {
            *out = &g;
            return RT3_OK;
        }
    if (w == 0 || h == 0 || w > 65535 || h > 65535 || n_ranks == 0 || root >= n_ranks) return fail(c, RT3_E_INVALID, "bad window / root / rank count for the gather");
    GatherLayout gl;
    gl.w = w; gl.h = h; gl.root = root; gl.n_ranks = n_ranks;
    gl.off.assign((size_t)n_ranks + 1, 0);
    std::vector<uint32_t> all, px;
    for (uint32_t r = 0; r < n_ranks; r++) {
        gl.off[r] = all.size();
        if (r == root) continue;  // the root's tiles never leave its image
        tile_pixels(w, h, r, n_ranks, px);
        all.insert(all.end(), px.begin(), px.end());
    }
    gl.off[n_ranks] = all.size();
    HIPC(c, gl.dev.alloc_bytes((all.size() ? all.size() : 1) * 4));
    if (!all.empty()) {
        hipError_t e = hipMemcpy(gl.dev.get(), all.data(), all.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("gather layout upload: ") + hipGetErrorString(e));
    }
    c->gather_layouts.push_back(std::move(gl));
    *out = &c->gather_layouts.back();
    return RT3_OK;
}
static int ensure_gather_buf(rt3_ctx* c, size_t bytes) {
    if (bytes <= c->gather_buf.capacity_bytes()) return RT3_OK;
    HIPC(c, hipStreamSynchronize(c->stream));  // an earlier gather may still be reading the old buffer: idle before it is dropped
    HIPC(c, c->gather_buf.alloc_bytes(bytes));
    return RT3_OK;
}

int rt3_comm_unique_id(void* id_out) {
    if (!id_out) return fail(nullptr, RT3_E_INVALID, "id_out is NULL");
    ncclUniqueId id;
    ncclResult_t e = ncclGetUniqueId(&id);
    if (e != ncclSuccess) return fail(nullptr, RT3_E_COMM, std::string("ncclGetUniqueId: ") + ncclGetErrorString(e));
    memcpy(id_out, &id, sizeof(id));
    return RT3_OK;
}
int rt3_comm_version(int* out) {  // ncclGetVersion: major * 10000 + minor * 100 + patch (RCCL reports the NCCL API level it implements)
    if (!out) return RT3_E_INVALID;
    ncclResult_t e = ncclGetVersion(out);
    return e == ncclSuccess ? RT3_OK : fail(nullptr, RT3_E_COMM, std::string("ncclGetVersion: ") + ncclGetErrorString(e));
}
int rt3_comm_init(rt3_ctx* c, const void* id, uint32_t rank, uint32_t n_ranks) {
    if (!c || !id) return fail(c, RT3_E_INVALID, "comm_init: NULL argument");
    if (n_ranks == 0 || rank >= n_ranks) return fail(c, RT3_E_INVALID, "comm_init: rank must be < n_ranks");
    if (c->comm) return fail(c, RT3_E_STATE, "comm_init: this context already has a communicator (rt3_comm_destroy first)");
    HIPC(c, hipSetDevice(c->device));
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    NCCLC(c, ncclCommInitRank(&c->comm, (int)n_ranks, uid, (int)rank));
    c->comm_rank = rank;
    c->comm_size = n_ranks;
    return RT3_OK;
}
int rt3_comm_destroy(rt3_ctx* c) {
    if (!c) return RT3_E_INVALID;
    if (!c->comm) return RT3_OK;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    ncclComm_t comm = c->comm;
    c->comm = nullptr;
    c->comm_size = 0;
    NCCLC(c, ncclCommDestroy(comm));
    return RT3_OK;
}
int rt3_gather_layout(rt3_ctx* c, uint32_t image, uint32_t root, uint32_t n_ranks, uint64_t* offsets) {
    if (!c || !offsets) return fail(c, RT3_E_INVALID, "gather_layout: NULL argument");
    Resource* r = get_res(c, image, RT3_TAG_IMAGE);
    if (!r || format_bytes(r->format) != 16) return fail(c, RT3_E_INVALID, "the gather needs a 16-byte-per-pixel image");
    HIPC(c, hipSetDevice(c->device));
    GatherLayout* gl;
    if (int e = get_gather_layout(c, r->w, r->h, root, n_ranks, &gl)) return e;
    memcpy(offsets, gl->off.data(), ((size_t)n_ranks + 1) * sizeof(uint64_t));
    return RT3_OK;
}
// the root's half of the gather without the exchange: `recv_device` is laid out as rt3_gather_layout says
int rt3_gather_unpack(rt3_ctx* c, uint32_t image, uint32_t root, uint32_t n_ranks, const void* recv_device) {
    if (!c || !recv_device) return fail(c, RT3_E_INVALID, "gather_unpack: NULL argument");
    Resource* r = get_res(c, image, RT3_TAG_IMAGE);
    if (!r || format_bytes(r->format) != 16) return fail(c, RT3_E_INVALID, "the gather needs a 16-byte-per-pixel image");
    HIPC(c, hipSetDevice(c->device));
    GatherLayout* gl;
    if (int e = get_gather_layout(c, r->w, r->h, root, n_ranks, &gl)) return e;
    const uint64_t total = gl->off[n_ranks];
    if (total) launch_unpack_tiles(c->stream, gl->dev.get(), (uint32_t)total, r->w, recv_device, r->ptr);  // ONE launch for all ranks
    HIPC(c, hipGetLastError());
    return RT3_OK;
}
int rt3_gather_tiles(rt3_ctx* c, uint32_t image, uint32_t root) {
    if (!c) return RT3_E_INVALID;
    if (!c->comm) return fail(c, RT3_E_STATE, "gather_tiles: call rt3_comm_init first");
    Resource* r = get_res(c, image, RT3_TAG_IMAGE);
    if (!r || format_bytes(r->format) != 16) return fail(c, RT3_E_INVALID, "the gather needs a 16-byte-per-pixel image");
    const uint32_t n = c->comm_size, me = c->comm_rank;
    if (root >= n) return fail(c, RT3_E_INVALID, "gather_tiles: root must be < n_ranks");
    if (c->n_ranks != n || c->rank != me)
        return fail(c, RT3_E_STATE, "gather_tiles: the tile partition (rt3_set_tile_partition) and the communicator disagree on rank / n_ranks");
    if (n == 1) return RT3_OK;  // the frame is already whole
    HIPC(c, hipSetDevice(c->device));
    if (me != root) {
        PixelList* pl;
        if (int e = get_pixlist(c, r->w, r->h, me, n, &pl)) return e;
        if (pl->count == 0) return RT3_OK;  // (the root skips empty ranks too)
        if (int e = ensure_gather_buf(c, (size_t)pl->count * 16)) return e;
        {
            ScopedTimer t(c, CAT_OTHER);
            launch_pack_tiles(c->stream, pl->dev.get(), pl->count, r->w, r->ptr, c->gather_buf.get());
        }
        HIPC(c, hipGetLastError());
        ScopedTimer t(c, CAT_GATHER);
        ncclResult_t se = ncclSend(c->gather_buf.get(), (size_t)pl->count * 4, ncclFloat, (int)root, c->comm, c->stream);
        if (se != ncclSuccess) return comm_abort(c, std::string("ncclSend: ") + ncclGetErrorString(se));
        return RT3_OK;
    }
    GatherLayout* gl;
    if (int e = get_gather_layout(c, r->w, r->h, root, n, &gl)) return e;
    const uint64_t total = gl->off[n];
    if (total == 0) return RT3_OK;
    if (int e = ensure_gather_buf(c, (size_t)total * 16)) return e;
    {
        // exact per-rank counts at exact offsets, every peer's recv in ONE group = one gather; xGMI is point to point, so the
        // root's inbound links run concurrently and nothing is forwarded (a ring would move (n-1) x the bytes)
        ScopedTimer t(c, CAT_GATHER);
        NCCLC(c, ncclGroupStart());
        for (uint32_t p = 0; p < n; p++) {
            const uint64_t cnt = gl->off[p + 1] - gl->off[p];
            if (p == root || cnt == 0) continue;
            ncclResult_t e = ncclRecv((char*)c->gather_buf.get() + gl->off[p] * 16, (size_t)cnt * 4, ncclFloat, (int)p, c->comm, c->stream);
            if (e != ncclSuccess) return comm_abort(c, std::string("ncclRecv: ") + ncclGetErrorString(e));
        }
        ncclResult_t ge = ncclGroupEnd();
        if (ge != ncclSuccess) return comm_abort(c, std::string("ncclGroupEnd: ") + ncclGetErrorString(ge));
    }
    ScopedTimer t(c, CAT_OTHER);
    launch_unpack_tiles(c->stream, gl->dev.get(), (uint32_t)total, r->w, c->gather_buf.get(), r->ptr);  // stream-ordered behind the receives
    HIPC(c, hipGetLastError());
    return RT3_OK;
}

// ---- pass launch
int rt3_pass_launch(rt3_ctx* c, const char* pass_name, const char* entry, uint32_t x, uint32_t y, uint32_t z, const void* constants,
                    size_t constants_size, const uint32_t* bindings, uint32_t n_bindings) {
    if (!c || !pass_name) return fail(c, RT3_E_INVALID, "pass_name NULL");
    if (entry && strcmp(entry, "main") != 0) return fail(c, RT3_E_INVALID, std::string("unknown entry point '") + entry + "' (the reference passes use \"main\")");
    if (!constants || constants_size != sizeof(rt3_gconst)) return fail(c, RT3_E_INVALID, "constants must be the 304-byte GConst block");
    if (!bindings && n_bindings) return fail(c, RT3_E_INVALID, "bindings NULL");
    if (int r = check_accel_current(c)) return r;
    HIPC(c, hipSetDevice(c->device));
    if (int r = sync_textures(c)) return r;
    if (c->max_tex_index >= (int64_t)c->h_tex.size())
        return fail(c, RT3_E_STATE, "a geometry references base-colour texture " + std::to_string(c->max_tex_index) + " but only " +
                                        std::to_string(c->h_tex.size()) + " texture(s) were set (rt3_scene_set_texture)");
    rt3_gconst g;
    memcpy(&g, constants, sizeof(g));
    for (const PassDesc& p : kPasses)
        if (!strcmp(pass_name, p.name)) return launch_pass(c, p, &g, x, y, z, bindings, n_bindings);
    return fail(c, RT3_E_INVALID, std::string("unknown pass '") + pass_name + "' (known: " + names_of(kPasses) + ")");
}
int rt3_denoise_set_params(rt3_ctx* c, const rt3_denoise_params* p) {
    if (!c) return RT3_E_INVALID;
    if (!p) {
        c->dn_params = kDenoiseDefaults;
        return RT3_OK;
    }
    if (p->iterations > 8) return fail(c, RT3_E_INVALID, "denoise params: iterations must be 0..8 (step 2^i: 8 iterations reach 512 pixels)");
    if (p->normal_squarings > 16) return fail(c, RT3_E_INVALID, "denoise params: normal_squarings must be 0..16 (the exponent is 2^k)");
    if (!(std::isfinite(p->sigma_z) && p->sigma_z > 0.0f) || !(std::isfinite(p->sigma_l) && p->sigma_l > 0.0f))
        return fail(c, RT3_E_INVALID, "denoise params: sigma_z and sigma_l must be finite and positive");
    if (p->flags & ~RT3_DENOISE_NO_DEMODULATION) return fail(c, RT3_E_INVALID, "denoise params: unknown flag bits");
    c->dn_params = *p;
    return RT3_OK;
}
int rt3_denoise_set_variance_input(rt3_ctx* c, uint32_t moments_image) {
    if (!c) return RT3_E_INVALID;
    c->dn_variance_image = moments_image;  // checked when "denoise" is launched: the image may be created, resized or destroyed in between
    return RT3_OK;
}
int rt3_temporal_set_prev_view(rt3_ctx* c, const void* prev_gconst, size_t size) {
    if (!c) return RT3_E_INVALID;
    if (!prev_gconst && size == 0) {
        c->tp_has_prev = false;
        return RT3_OK;
    }
    if (!prev_gconst || size != sizeof(rt3_gconst)) return fail(c, RT3_E_INVALID, "temporal prev view: must be the 304-byte GConst block of the previous frame, or (NULL, 0)");
    memcpy(&c->tp_prev, prev_gconst, sizeof(rt3_gconst));
    c->tp_has_prev = true;
    return RT3_OK;
}
int rt3_temporal_set_motion_input(rt3_ctx* c, uint32_t motion_image) {
    if (!c) return RT3_E_INVALID;
    c->tp_motion_image = motion_image;  // checked when "temporal" is launched, like the variance input of "denoise"
    return RT3_OK;
}
int rt3_temporal_set_params(rt3_ctx* c, const rt3_temporal_params* p) {
    if (!c) return RT3_E_INVALID;
    if (!p) {
        c->tp_params = kTemporalDefaults;
        return RT3_OK;
    }
    if (!(p->alpha >= 0.0f && p->alpha <= 1.0f) || !(p->alpha_moments >= 0.0f && p->alpha_moments <= 1.0f))
        return fail(c, RT3_E_INVALID, "temporal params: alpha and alpha_moments must lie in [0, 1]");
    if (p->max_history < 1 || p->max_history > 65535) return fail(c, RT3_E_INVALID, "temporal params: max_history must be 1..65535");
    if (!(p->normal_cos >= -1.0f && p->normal_cos <= 1.0f)) return fail(c, RT3_E_INVALID, "temporal params: normal_cos must lie in [-1, 1]");
    if (!(std::isfinite(p->plane_tolerance) && p->plane_tolerance > 0.0f)) return fail(c, RT3_E_INVALID, "temporal params: plane_tolerance must be finite and positive");
    if (p->flags & ~RT3_TEMPORAL_NO_DEMODULATION) return fail(c, RT3_E_INVALID, "temporal params: unknown flag bits");
    c->tp_params = *p;
    return RT3_OK;
}
int rt3_frame_wait(rt3_ctx* c) {
    if (!c) return RT3_E_INVALID;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    return RT3_OK;
}

// ---- ray batches
int rt3_trace_rays(rt3_ctx* c, const float* rays, uint32_t n, int any_hit, float* t, float* u, float* v, uint32_t* prim, uint32_t* n_nodes,
                   uint32_t* n_tris, int repeat, double* kernel_ms) {
    if (!c || !rays || !prim || (!any_hit && (!t || !u || !v))) return fail(c, RT3_E_INVALID, "trace_rays: NULL argument");
    if (int r = check_accel_current(c)) return r;
    if (n == 0) return RT3_OK;
    HIPC(c, hipSetDevice(c->device));
    DevBuf<float> d_rays, d_hits;
    DevBuf<uint32_t> d_cn, d_ct, d_occ, d_cur;
    const bool count = n_nodes || n_tris;
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() {
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        }
    } ev;
    HIPC(c, d_rays.alloc_bytes((size_t)n * 32));
    HIPC(c, d_hits.alloc_bytes((size_t)n * 16));
    HIPC(c, d_occ.alloc_bytes((size_t)n * 4));
    HIPC(c, d_cur.alloc_bytes(4));
    if (count) {
        HIPC(c, d_cn.alloc_bytes((size_t)n * 4));
        HIPC(c, d_ct.alloc_bytes((size_t)n * 4));
    }
    {  // host SoA (ox..tmax) -> device records {o.xyz, tmin} x n, {d.xyz, tmax} x n
        std::vector<float> rec((size_t)n * 8);
        for (uint32_t i = 0; i < n; i++) {
            float* a = &rec[4 * (size_t)i];
            float* b = &rec[4 * ((size_t)n + i)];
            a[0] = rays[i]; a[1] = rays[(size_t)n + i]; a[2] = rays[2 * (size_t)n + i]; a[3] = rays[6 * (size_t)n + i];
            b[0] = rays[3 * (size_t)n + i]; b[1] = rays[4 * (size_t)n + i]; b[2] = rays[5 * (size_t)n + i]; b[3] = rays[7 * (size_t)n + i];
        }
        HIPC(c, hipMemcpy(d_rays.get(), rec.data(), (size_t)n * 32, hipMemcpyHostToDevice));
    }
    HIPC(c, hipEventCreate(&ev.e0));
    HIPC(c, hipEventCreate(&ev.e1));
    if (repeat < 1) repeat = 1;
    TraceLaunch L;
    L.rays = d_rays.get(); L.stride = n; L.n = n; L.work_counter = d_cur.get();
    L.hits = d_hits.get(); L.occluded = d_occ.get();  // the launch below writes one of the two
    L.count = count; L.cnt_nodes = d_cn.get(); L.cnt_tris = d_ct.get();
    if (c->accel_masked) {
        if (int r = sync_textures(c)) return r;
        L.alpha = alpha_dev(c);
    }
    auto launch = [&]() {
        (void)hipMemsetAsync(d_cur.get(), 0, 4, c->stream);  // ray-pool cursor
        if (any_hit) launch_shadow(c->stream, c->bvh, L);
        else launch_extend(c->stream, c->bvh, L);
    };
    launch();  // warm-up (also the result-producing launch)
    HIPC(c, hipEventRecord(ev.e0, c->stream));
    for (int k = 0; k < repeat; k++) launch();
    HIPC(c, hipEventRecord(ev.e1, c->stream));
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    HIPC(c, hipEventElapsedTime(&ms, ev.e0, ev.e1));
    if (kernel_ms) *kernel_ms = (double)ms / repeat;
    if (any_hit) {
        HIPC(c, hipMemcpy(prim, d_occ.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
    } else {
        std::vector<float> rec((size_t)n * 4);  // device hits are {t, u, v, prim} records
        HIPC(c, hipMemcpy(rec.data(), d_hits.get(), (size_t)n * 16, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; i++) {
            t[i] = rec[4 * (size_t)i];
            u[i] = rec[4 * (size_t)i + 1];
            v[i] = rec[4 * (size_t)i + 2];
            memcpy(&prim[i], &rec[4 * (size_t)i + 3], 4);
        }
    }
    if (n_nodes) HIPC(c, hipMemcpy(n_nodes, d_cn.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
    if (n_tris) HIPC(c, hipMemcpy(n_tris, d_ct.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
    return RT3_OK;
}

int rt3_selftest_eval(rt3_ctx* c, int op, const void* in, uint32_t n, void* out) {
    uint32_t iw, ow;
    if (!c || !in || !out || !selftest_widths(op, &iw, &ow)) return fail(c, RT3_E_INVALID, "selftest: bad op / NULL");
    if ((op == 25 || op == 26) && !c->d_sky) return fail(c, RT3_E_STATE, "selftest: the sky ops need a sky (rt3_scene_set_sky)");
    if (n == 0) return RT3_OK;
    HIPC(c, hipSetDevice(c->device));
    if (op == 27)
        if (int r = sync_textures(c)) return r;
    DevBuf<uint32_t> d_in, d_out;
    HIPC(c, d_in.alloc_bytes((size_t)n * iw * 4));
    HIPC(c, d_out.alloc_bytes((size_t)n * ow * 4));
    hipError_t e = hipMemcpy(d_in.get(), in, (size_t)n * iw * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_selftest(c->stream, op, scene_dev(c), d_in.get(), n, d_out.get());
        e = hipStreamSynchronize(c->stream);
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out.get(), (size_t)n * ow * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("selftest: ") + hipGetErrorString(e));
    return RT3_OK;
}

// ---- emitter table of RT3_F_NEE_EMISSIVE
int rt3_light_info(rt3_ctx* c, uint32_t* n_emitters, uint64_t* cdf_total) {
    if (!c) return RT3_E_INVALID;
    if (int r = ensure_lights(c)) return r;
    if (n_emitters) *n_emitters = c->lights.n;
    if (cdf_total) *cdf_total = c->lights.total;
    return RT3_OK;
}
int rt3_light_download(rt3_ctx* c, uint32_t* prim, float* area, uint32_t* mass) {
    if (!c) return RT3_E_INVALID;
    if (int r = ensure_lights(c)) return r;
    const LightTable& t = c->lights;
    if (!t.n) return RT3_OK;
    if (prim) HIPC(c, hipMemcpy(prim, t.prim.get(), (size_t)t.n * 4, hipMemcpyDeviceToHost));
    if (area) HIPC(c, hipMemcpy(area, t.area.get(), (size_t)t.n * 4, hipMemcpyDeviceToHost));
    if (mass) {
        HIPC(c, hipMemcpy(mass, t.cdf.get(), (size_t)t.n * 4, hipMemcpyDeviceToHost));
        for (uint32_t k = t.n - 1; k > 0; k--) mass[k] -= mass[k - 1];  // inclusive CDF -> masses
    }
    return RT3_OK;
}

int rt3_stats_reset(rt3_ctx* c) {
    if (!c) return RT3_E_INVALID;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (int r = harvest(c)) return r;
    memset(&c->stats, 0, sizeof(c->stats));
    return RT3_OK;
}
int rt3_stats_get(rt3_ctx* c, rt3_stats* out) {
    if (!c || !out) return RT3_E_INVALID;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (int r = harvest(c)) return r;
    *out = c->stats;
    return RT3_OK;
}

// ---- camera: components/camera.rs:52-58 (glam look_at_rh / perspective_rh with depth 0..1) + renderer/mod.rs:72-78
static void invert4(const float* m, float* out) {
    double a[4][4], inv[4][4];
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++) a[r][c] = m[c * 4 + r];
    // adjugate through 3x3 minors
    auto minor3 = [&](int rr, int cc) {
        double s[3][3];
        int ri = 0;
        for (int r = 0; r < 4; r++) {
            if (r == rr) continue;
            int ci = 0;
            for (int c = 0; c < 4; c++) {
                if (c == cc) continue;
                s[ri][ci++] = a[r][c];
            }
            ri++;
        }
        return s[0][0] * (s[1][1] * s[2][2] - s[1][2] * s[2][1]) - s[0][1] * (s[1][0] * s[2][2] - s[1][2] * s[2][0]) +
               s[0][2] * (s[1][0] * s[2][1] - s[1][1] * s[2][0]);
    };
    double det = 0.0;
    for (int c = 0; c < 4; c++) det += ((c & 1) ? -1.0 : 1.0) * a[0][c] * minor3(0, c);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) inv[c][r] = (((r + c) & 1) ? -1.0 : 1.0) * minor3(r, c) / det;
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++) out[c * 4 + r] = (float)inv[r][c];
}
void rt3_camera_gconst(const float position[3], const float direction[3], float fov_y, float aspect, float z_near, float z_far, float width,
                       float height, rt3_gconst* g) {
    memset(g, 0, sizeof(*g));
    float len = std::sqrt(direction[0] * direction[0] + direction[1] * direction[1] + direction[2] * direction[2]);
    float f[3] = {direction[0] / len, direction[1] / len, direction[2] / len};  // Camera::new normalises, camera.rs:43
    // look_to_rh(eye, dir, up=+Y): s = normalize(f x up), u = s x f
    float s[3] = {f[1] * 0.0f - f[2] * 1.0f, f[2] * 0.0f - f[0] * 0.0f, f[0] * 1.0f - f[1] * 0.0f};
    float sl = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    s[0] /= sl; s[1] /= sl; s[2] /= sl;
    float u[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};
    float* v = g->view;
    v[0] = s[0]; v[1] = u[0]; v[2] = -f[0];
    v[4] = s[1]; v[5] = u[1]; v[6] = -f[1];
    v[8] = s[2]; v[9] = u[2]; v[10] = -f[2];
    v[12] = -(position[0] * s[0] + position[1] * s[1] + position[2] * s[2]);
    v[13] = -(position[0] * u[0] + position[1] * u[1] + position[2] * u[2]);
    v[14] = position[0] * f[0] + position[1] * f[1] + position[2] * f[2];
    v[15] = 1.0f;
    float sf = (float)std::sin(0.5 * (double)fov_y), cf = (float)std::cos(0.5 * (double)fov_y);
    float hh = cf / sf, ww = hh / aspect, r = z_far / (z_near - z_far);
    g->proj[0] = ww;
    g->proj[5] = hh;
    g->proj[10] = r;
    g->proj[11] = -1.0f;
    g->proj[14] = r * z_near;
    invert4(g->proj, g->proj_inverse);
    invert4(g->view, g->view_inverse);
    g->window_size[0] = width;
    g->window_size[1] = height;
    g->blendfactor = 1.0f;
}

}  // extern "C"
