// rt3_ctx.hpp -- the private context of the host layer: host-only types, rt3_ctx grouped by the file that writes each part, and the few
// functions one host file needs from another.  Included by the host translation units only (rt3_api.hip, rt3_scene.hip, rt3_accel.hip,
// rt3_passes.hip, rt3_tiles.hip): no kernel object depends on it.
//
// Ownership rule: a file writes another owner's state only through a function declared at the end of this header; reads are free.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rt3.h"
#include "rt3_internal.hpp"
#include "rt3_volume.hpp"

struct ncclComm;  // <rccl/rccl.h> (ncclComm_t), which only rt3_tiles.hip includes

namespace rt3 {

inline const rt3_denoise_params kDenoiseDefaults = {5u, 7u, 0.05f, 4.0f, 0u};
inline const rt3_temporal_params kTemporalDefaults = {0.2f, 0.2f, 32u, 0.9f, 0.01f, 0u};
inline const rt3_adaptive_params kAdaptiveDefaults = {16u, 16u, 0.05f, 0.01f, 1u, 0u};
inline constexpr float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
// a column-major 4 x 4 whose last row is (0, 0, 0, 1) as the device tables hold it: 3 x 4, column-major (FlatGeomDev::m)
inline void pack3x4(const float* m16, float* m12) {
    for (int col = 0; col < 4; col++)
        for (int row = 0; row < 3; row++) m12[3 * col + row] = m16[4 * col + row];
}

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
    // roulette: for bounces rr_lo .. n_pairs-2 the rays k_extend traced are k_roulette's survivors, whose count is word
    // rr_first + bounce; rr_first = 0: no roulette in this batch.  `launch`: the pass launch the batch belongs to (Work::launch_serial)
    uint32_t rr_first = 0, rr_lo = 0;
    uint64_t launch = 0;
    // RT3_OPT_SHADE_EXIT_TEST: word dec_first + bounce counts the sky shadow rays k_shade_defer_exit generated and decided
    // itself, which the shadow-queue size no longer holds; dec_first = 0: none in this batch
    uint32_t dec_first = 0;
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
    bool valid = false;                 // accel.bvh holds a two-level structure whose bottom trees match `meshes`
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
// on a tree or a matrix.  `key` = what they were made for: content_gen, then the uploaded geometry of every flattened one; empty
// = nothing valid.
struct ShadeRecords {
    DevBuf<uint4> rec;
    DevBuf<float2> uv;
    DevBuf<uint32_t> tan;  // tangent words (k_tri_tangent): held only while some geometry names a normal texture; has_tan says whether valid
    bool has_tan = false;
    uint32_t n = 0;  // records the buffers hold
    std::vector<uint64_t> key;
};
// One flattened geometry of the last rt3_accel_build, in flattened (instance-major) order: the one walk over the placements, recorded by
// flatten_world for everything that needs "the (instance, geometry) pairs the structure covers" afterwards
struct Placed {
    uint32_t instance, geom;       // the placement's index; the uploaded geometry
    uint32_t first_prim, n_prims;  // its flattened primitives
    bool identity;                 // the instance's matrix is exactly the identity
};

// One skin (rt3_scene_add_skin): the vertex range it writes and k_skin_pose's inputs.  flag_pending: posed since its
// flag word was last read clear
struct Skin {
    uint32_t first = 0, n = 0, n_joints = 0, n_targets = 0;
    DevBuf<float4> rest, weights, palette;
    DevBuf<uint2> joints;
    DevBuf<float> dpos, dnrm;
    uint64_t bytes = 0;
    bool flag_pending = false;
};
// A pinned host buffer and the event behind the last copy out of it
struct PaletteSlot {
    float* host = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool in_flight = false;
    PaletteSlot() = default;
    PaletteSlot(const PaletteSlot&) = delete;
    PaletteSlot& operator=(const PaletteSlot&) = delete;
    ~PaletteSlot() {
        if (host) (void)hipHostFree(host);
        if (done) (void)hipEventDestroy(done);
    }
};

}  // namespace rt3

struct rt3_ctx {
    // rt3_api.hip (rt3_create, the resource calls)
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    char name[256] = {0};
    // A Resource* / PixelList* holds until the next push_back; the device memory they own never moves
    std::vector<rt3::Resource> resources;

    // rt3_scene.hip: what the caller uploaded
    struct Scene {
        rt3::DevBuf<float> d_verts;
        uint32_t n_verts = 0;
        rt3::DevBuf<uint32_t> d_indices;
        uint32_t n_indices = 0;
        uint32_t n_geoms = 0, n_prims = 0;       // uploaded geometries / their primitives (one instance of each)
        std::vector<uint32_t> h_indices;         // host copies, only for range validation (rt3_scene_set_geometry, again in rt3_accel_build)
        std::vector<rt3_geometry_info> h_geoms;
        std::vector<uint32_t> h_prim_counts;
        std::vector<std::pair<uint32_t, uint32_t>> h_geom_span;  // per uploaded geometry its vertex span [lo, hi] (lo > hi: no triangle)
        int64_t max_tex_index = -1;
        // alpha masks: cutoff per uploaded geometry (empty = all 0, opaque)
        std::vector<float> h_cutoffs;
        // material textures per uploaded geometry (empty = none anywhere)
        std::vector<rt3_material_textures> h_mat_tex;
        // transmission per uploaded geometry (empty = no glass anywhere)
        std::vector<rt3_transmission> h_transmission;
        // absorption inside solid glass per uploaded geometry (empty = every sigma 0)
        std::vector<rt3_attenuation> h_attenuation;
        std::vector<rt3_instance> h_instances;   // empty = one identity instance of every geometry
        // the previous frame's instance matrices, n x 16 column-major (rt3_scene_set_prev_transforms; empty = every instance unmoved)
        std::vector<float> prev_transforms;
        // punctual lights (rt3_scene_set_lights), as validated; lights_stamp is bumped by every successful call, and is
        // all that changes: the acceleration structure stays as it is
        std::vector<rt3_punctual_light> lights;
        uint64_t lights_stamp = 1;
        // textured emitters (rt3_scene_set_textured_emitters): a mode of the light table alone, like the light list
        bool textured_emitters = false;
        rt3::DevBuf<uint2> d_sky;  // 8-byte texels {RGB9E5, pdf_uv} in 4 x 4 tiles
        rt3::DevBuf<float> d_cdf_marg;
        rt3::DevBuf<uint32_t> d_sky_alias, d_guide_marg;
        uint32_t sky_w = 0, sky_h = 0, sky_wt = 0;
        float sky_min_pdf = 0.0f;  // the smallest texel density rt3_scene_set_sky stored (what RT3_OPT_DEFER_SKY_LIGHT's cover asks of it)
        rt3::DevBuf<uint8_t> d_bn;
        uint32_t bn_w = 0, bn_h = 0;
        uint64_t bn_stamp = 0;  // bumped by every rt3_scene_set_bluenoise
        // base-colour textures: host staging (RGBA8) + device atlas rebuilt lazily (sync_textures)
        std::vector<std::vector<uint8_t>> h_tex;
        std::vector<uint32_t> tex_w, tex_h;
        rt3::DevBuf<uint8_t> d_tex_pixels;
        rt3::DevBuf<uint4> d_tex_table;
        rt3::DevBuf<float> d_srgb_lut;
        bool tex_dirty = false;
        uint64_t tex_stamp = 1;  // bumped by every rt3_scene_set_texture: a textured emitter's mass depends on texels
        // generations: topo_gen is bumped by everything a tree's shape depends on (vertex count, indices, geometry, leaf size, layout,
        // collapse, SAH top); content_gen by all of that and by rt3_scene_update_vertices too.  A refit needs the topology of the build it
        // updates; the two-level structure keeps its bottom trees while the content is what they were built (or refitted) for
        uint64_t topo_gen = 1, content_gen = 1;
    } scene;

    // rt3_accel.hip: the acceleration structure and everything made for one build of it
    struct Accel {
        rt3::DevBuf<rt3::FlatGeomDev> d_geoms;             // one entry per (instance, geometry): built by rt3_accel_build (flatten_world)
        rt3::DevBuf<rt3::ShadeGeomDev> d_shade_geoms;      // the same table as hit_info reads it
        rt3::DevBuf<rt3::MatTexDev> d_mat_tex;             // per flattened geometry; has_mat_tex: the built scene names a material texture
        bool has_mat_tex = false, has_normal_tex = false;
        rt3::DevBuf<rt3::GlassDev> d_glass;                // per flattened geometry; has_glass: the built scene has a transmission > 0
        bool has_glass = false;
        // absorption: per flattened geometry, kept only while the last rt3_accel_build classified some geometry as
        // absorbing (n_absorbing of them; 0: no table, no k_absorb)
        rt3::DevBuf<rt3::AbsorbDev> d_absorb;
        uint32_t n_absorbing = 0;
        rt3::DevBuf<uint32_t> d_prim_geom, d_first_prim;
        uint32_t n_flat_geoms = 0, n_flat_prims = 0;  // after flattening: what the acceleration structure and the shading records cover
        std::vector<rt3::Placed> placed;              // the same, on the host: n_flat_geoms entries
        uint64_t bulk_copies = 0;                     // host <-> device copies of more than 64 KiB made by rt3_accel_build (rt3_stats.accel_bulk_copies)
        // the alpha-mask tables of the last rt3_accel_build: d_geom_mask per uploaded geometry {cutoff bits, slot}, d_alpha per masked
        // geometry {texture index, base_color[3] bits}
        rt3::DevBuf<uint2> d_geom_mask, d_alpha;
        bool masked = false;  // the structure holds masked triangles: traversal launches run the MASK kernels
        // pane shadows: flattened geometries with triangles that the last rt3_accel_build classified as panes (0 while
        // the mode is off) and the first alpha slot of the masked ones' marked records.  marked: the records carry mask or pane words
        uint32_t n_panes = 0, pane_first_slot = 0;
        // rough transmission: flattened geometries with triangles that the last rt3_accel_build classified as frosted (0
        // while the mode is off); their d_glass entries carry kGlassFrostBit
        uint32_t n_frosted = 0;
        bool marked = false;
        rt3::LbvhResult bvh;
        rt3::ShadeRecords shade;
        rt3::DevBuf<char> build_scratch;  // grow-only: lbvh_build's scratch, kept from build to build
        bool built = false;
        bool stale = false;     // vertices updated since the structure was built or refitted: nothing traces it until a refit or build
        uint64_t topo_gen = 0;  // scene.topo_gen of the last successful rt3_accel_build
        uint64_t stamp = 0;     // bumped by every successful rt3_accel_build / rt3_accel_refit / rt3_accel_import
        rt3::LightTable lights; // RT3_F_NEE_EMISSIVE / RT3_F_NEE_PUNCTUAL: built lazily for `stamp`, the light list and the flag pair (ensure_lights)
        // refit plans (rt3_refit.hip), made on the first refit after a build or import: one per tree (instance mode 1: one per bottom tree)
        bool refit_planned = false;
        std::vector<rt3::RefitTree> refit_trees;
        std::vector<rt3::MeshTables> refit_tables;    // instance mode 1: each bottom tree's (tl_build_mesh's)
        rt3::DevBuf<char> refit_scratch;              // grow-only: refit_tree's bounds, node boxes and record boxes
        rt3::TwoLevelState tl;
        // k_shadow's exit table: the context's two counters {tried, occluded} and the grow-only scratch of a fill
        rt3::DevBuf<unsigned long long> exit_counters;
        rt3::DevBuf<char> exit_scratch;
    } accel;

    // rt3_passes.hip: the wavefront work queues (capacity in paths) and the device counters of the launches.  rt3_create allocates the
    // counters; harvest (rt3_api.hip) is what drains counters_next, pending_counters, primary_rays_pending and the totals into the stats
    struct Work {
        size_t cap = 0, cap_pix = 0;
        rt3::DevBuf<float> rays[2], hits, T[2];
        rt3::DevBuf<float> sh_rays, sh_contrib, lacc, radsum;
        rt3::DevBuf<float> sh2_rays, sh2_contrib, sh2_tmax;  // RT3_F_NEE_EMISSIVE: the emitter shadow queue, allocated when the flag is first used
        size_t cap_emit = 0;
        rt3::DevBuf<float> pane_dist;  // pane shadows: one float per path of the batch (k_shade_pane), allocated when a frame first needs it
        size_t cap_pane = 0;
        rt3::DevBuf<uint32_t> d_counters;
        uint32_t counters_cap = 1 << 16, counters_next = 0;
        rt3::DevBuf<unsigned long long> d_totals;  // counting mode: kTotWords words (TotalsWord)
        std::vector<rt3::CounterBlock> pending_counters;
        uint64_t primary_rays_pending = 0;
        // roulette: records k_roulette read / ended in the pass launch numbered launch_serial (rt3_path_roulette_info)
        uint64_t launch_serial = 0, roulette_tested = 0, roulette_ended = 0;
    } work;

    // rt3_tiles.hip: the tile partition and the frame-end gather
    struct Tiles {
        std::vector<rt3::PixelList> pixlists;
        std::vector<rt3::GatherLayout> gather_layouts;
        uint32_t rank = 0, n_ranks = 1, part_w = 0, part_h = 0;
        // communicator of the frame-end gather (RCCL): one rank per context / GPU / process
        ncclComm* comm = nullptr;
        uint32_t comm_rank = 0, comm_size = 0;
        rt3::DevBuf<char> gather_buf;  // grow-only; non-root: this rank's packed tiles; root: the receive buffer of all other ranks' tiles
    } tiles;

    // rt3_passes.hip: "denoise" pass: parameters (rt3_denoise_set_params) and the grow-only scratch its records are carved from
    struct Denoise {
        rt3_denoise_params params = rt3::kDenoiseDefaults;
        rt3::DevBuf<char> scratch;
        uint32_t variance_image = 0;  // rt3_denoise_set_variance_input: the "temporal" pass's Moments image, 0 = none
    } denoise;
    // rt3_passes.hip: "temporal" pass: parameters (rt3_temporal_set_params) and the previous frame's GConst (rt3_temporal_set_prev_view)
    struct Temporal {
        rt3_temporal_params params = rt3::kTemporalDefaults;
        rt3_gconst prev;
        bool has_prev = false;
        uint32_t motion_image = 0;  // rt3_temporal_set_motion_input: the "motion" pass's image, 0 = none
    } temporal;
    // rt3_passes.hip: "motion" pass: the device tables made from scene.prev_transforms and deform.h_deformed for the structure of
    // accel.stamp `stamp` (motion_tables); `dirty`: an input changed since (motion_tables_stale)
    struct Motion {
        bool dirty = false, any_moved = false, any_deformed = false;
        uint64_t stamp = 0;
        rt3::DevBuf<rt3::MotionPrevDev> d_prev;
        rt3::DevBuf<uint32_t> d_slot;
    } motion;
    // rt3_passes.hip: "adaptive" pass: parameters (rt3_adaptive_set_params), the grow-only scratch its state and lists are carved from, and
    // what the last launch did (rt3_adaptive_info); `coverage` (rt3_adaptive_set_coverage): with a lens set the pass lists every pixel of the
    // rank instead of refusing; off by default, untouched by scene changes
    struct Adaptive {
        rt3_adaptive_params params = rt3::kAdaptiveDefaults;
        bool coverage = false;
        rt3::DevBuf<char> scratch;
        uint32_t rounds = 0, pixels_capped = 0;
        uint64_t paths_traced = 0;
    } adaptive;
    // rt3_passes.hip: per-sample camera rays (rt3_camera_set_lens): off by default
    struct Lens {
        rt3_lens_params params = {0.0f, 1.0f, 1.0f, 0u};
        bool on = false;
    } lens;
    // rt3_passes.hip: guide images: the four images a lens frame's "refrence_mode" writes (rt3_camera_set_guide_output)
    // and the four "denoise" is guided by (rt3_denoise_set_guide_input); both off by default, both checked again at every launch
    struct Guide {
        rt3_guide_images out = {0u, 0u, 0u, 0u}, in = {0u, 0u, 0u, 0u};
        bool out_on = false, in_on = false;
        // rt3_temporal_set_guide_input: the sets of this frame and of the previous one that "temporal" takes its
        // records from; off by default, checked at every launch
        rt3_guide_images temporal_cur = {0u, 0u, 0u, 0u}, temporal_prev = {0u, 0u, 0u, 0u};
        bool temporal_on = false;
        // the fifth image "refrence_mode" writes beside the four (rt3_camera_set_guide_motion_output), the samples'
        // mean previous position, and the one "temporal" looks up (rt3_temporal_set_guide_motion_input); 0 = off, checked at every launch
        uint32_t motion_out = 0, temporal_motion = 0;
    } guide;
    // rt3_passes.hip: Russian roulette on extension rays (rt3_path_set_roulette): off by default
    struct Roulette {
        rt3_roulette_params params = {2u, 0.0625f, {0u, 0u}};
        bool on = false;
    } roulette;
    // rt3_scene.hip: pane shadows (rt3_scene_set_pane_shadows): the mode, read by the next rt3_accel_build; off by default.
    // It lives here, not in `scene`: rt3_scene_set_geometry leaves it as it is
    bool pane_shadows = false;
    // rt3_scene.hip: rough transmission (rt3_scene_set_rough_transmission): the mode, read by the next rt3_accel_build; off
    // by default; like pane_shadows it is not part of `scene`
    bool rough_transmission = false;
    // rt3_scene.hip: fog (rt3_scene_set_medium): the medium as validated; `on`: set, and some sigma_a + sigma_s > 0.  Not
    // part of `scene`: rt3_scene_set_geometry leaves it as it is.  rt3_passes.hip owns the rest: the two in-scatter shadow queues (as large
    // as the other queues, allocated while a medium is on, freed by the first launch without one) and the device words of rt3_medium_info
    struct Medium {
        rt3_medium params = {};
        bool set = false, on = false;
        rt3::DevBuf<float> q_rays[2], q_contrib[2], q_tmax[2];
        size_t cap = 0;
        rt3::DevBuf<unsigned long long> d_info;  // {segments, in-scatter rays} of the last launch
    } medium;
    // rt3_scene.hip: deformation: the snapshot of rt3_scene_snapshot_vertices, one {x, y, z, 0} per vertex; the vertex
    // ranges rt3_scene_update_vertices touched since it, sorted and merged; and, once deform_flags has run, per uploaded geometry whether
    // some position word inside its span differs from the snapshot
    struct Deform {
        rt3::DevBuf<float4> d_prev_pos;
        bool snapshot = false, dirty = false;
        std::vector<std::pair<uint32_t, uint32_t>> ranges;  // [first, end)
        std::vector<uint32_t> h_deformed;
        rt3::DevBuf<uint32_t> d_deformed;
        rt3::DevBuf<uint4> d_chunks;
    } deform;
    // rt3_scene.hip: skins (rt3_scene_add_skin): what k_skin_pose reads of each, resident on the device; one range flag
    // word per skin in d_flags (grown in steps, behind a stream synchronise); and the pinned ring a pose's palette is packed into, so that
    // rt3_scene_pose_skin uploads it stream-ordered from memory the caller cannot change (a slot is reused once its copy has completed)
    struct Skins {
        std::vector<rt3::Skin> list;
        rt3::DevBuf<uint32_t> d_flags;
        uint32_t flags_cap = 0;
        rt3::PaletteSlot ring[4];
        uint32_t ring_next = 0;
    } skin;

    // rt3_api.hip (rt3_set_option)
    struct Opt {
        int64_t batch_spp = 0;
        bool profile = false, count = false;
        int variant = 0;  // RT3_OPT_EXTEND_VARIANT: reserved for traversal experiments
        uint32_t leaf_size = 2, node_width = 4, node_quant = 1, collapse = 2, sah_top = 1;
        int instance_mode = 0;  // RT3_OPT_INSTANCE_MODE: 0 flatten, 1 two-level
        int exit_table = 1;     // RT3_OPT_SHADOW_EXIT_TABLE: 0 off, 1 on, 2 on with scrambled entries (a test aid)
        bool defer_sky_light = true;  // RT3_OPT_DEFER_SKY_LIGHT
        bool shade_exit_test = true;  // RT3_OPT_SHADE_EXIT_TEST
    } opt;
    // rt3_api.hip (harvest, rt3_stats_reset), the events through ScopedTimer; stats.accel_* are rt3_accel.hip's (a build's time and copies)
    struct Prof {
        rt3_stats stats;
        std::vector<rt3::Timed> pending_events;
        std::vector<rt3::Timed> free_events;
    } prof;
};

namespace rt3 {

// ---- rt3_api.hip
int fail(rt3_ctx* c, int code, const std::string& msg);  // c null: the error of rt3_create and of the calls without a context
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
struct ScopedTimer {  // brackets one kernel launch with HIP events on the context's stream when profiling is on
    rt3_ctx* c;
    Timed t;
    bool on;
    ScopedTimer(rt3_ctx* ctx, int cat) : c(ctx), on(ctx->opt.profile) {
        if (!on) return;
        if (!c->prof.free_events.empty()) {
            t = c->prof.free_events.back();
            c->prof.free_events.pop_back();
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
        c->prof.pending_events.push_back(t);
    }
};
Resource* get_res(rt3_ctx* c, uint32_t handle, uint32_t want_tag);
size_t format_bytes(uint32_t f);
int harvest(rt3_ctx* c);  // stream must be idle

// ---- rt3_scene.hip
// a change every tree's shape depends on: the structure goes, and a refit cannot bring it back
void invalidate_topology(rt3_ctx* c);
// (re)build the device texture atlas after rt3_scene_set_texture calls
int sync_textures(rt3_ctx* c);
// rt3_scene_set_geometry's range checks again, against the vertex and index buffers as they are now; remakes scene.h_geom_span
int revalidate_geometry(rt3_ctx* c);
int deform_flags(rt3_ctx* c);
// the range flags of the skins posed since they were last read clear; the stream must be idle.  RT3_E_INVALID when one
// is set: rt3_accel_build and rt3_accel_refit refuse, before they change anything, to put boxes around such positions
int check_skin_flags(rt3_ctx* c);
inline bool any_cutoff(const rt3_ctx* c) { return !c->scene.h_cutoffs.empty(); }
inline bool any_mat_tex(const rt3_ctx* c) { return !c->scene.h_mat_tex.empty(); }
inline bool any_glass(const rt3_ctx* c) { return !c->scene.h_transmission.empty(); }
// does uploaded geometry g absorb (rt3_scene_set_attenuation)?  Transmission > 0, solid, some sigma > 0
inline bool absorbing_geometry(const rt3_ctx* c, uint32_t g) {
    if (c->scene.h_attenuation.empty() || !any_glass(c)) return false;
    const rt3_transmission& t = c->scene.h_transmission[g];
    if (!(t.transmission > 0.0f) || t.thin_walled != 0u) return false;
    const float* s = c->scene.h_attenuation[g].sigma;
    return s[0] > 0.0f || s[1] > 0.0f || s[2] > 0.0f;
}
// is uploaded geometry g frosted (rt3_scene_set_rough_transmission)?  Mode on, transmission > 0, and a roughness that can
// be > 0 somewhere: the factor is, or a metallic-roughness texture scales it
inline bool frosted_geometry(const rt3_ctx* c, uint32_t g) {
    if (!c->rough_transmission || !any_glass(c)) return false;
    if (!(c->scene.h_transmission[g].transmission > 0.0f)) return false;
    return c->scene.h_geoms[g].roughness > 0.0f || (any_mat_tex(c) && c->scene.h_mat_tex[g].metallic_roughness_texture >= 0);
}
// is uploaded geometry g a pane (rt3_scene_set_pane_shadows)?  Mode on, transmission > 0, thin-walled, no normal texture,
// not frosted (a path through a frosted pane does not go straight on)
inline bool pane_geometry(const rt3_ctx* c, uint32_t g) {
    if (!c->pane_shadows || !any_glass(c) || frosted_geometry(c, g)) return false;
    const rt3_transmission& t = c->scene.h_transmission[g];
    if (!(t.transmission > 0.0f) || t.thin_walled != 1u) return false;
    return !any_mat_tex(c) || c->scene.h_mat_tex[g].normal_texture < 0;
}

// ---- rt3_accel.hip
void invalidate_accel(rt3_ctx* c);  // the structure is not for the current scene any more: accel.built goes
void mark_accel_stale(rt3_ctx* c);  // vertices were updated in place: a built structure is stale until a refit or build
// RT3_OK when the structure may be traced: built, and no vertex updated since
int check_accel_current(rt3_ctx* c, const char* unbuilt = "rt3_accel_build has not been called for the current scene");
// The placements a build covers: the instances set, or (none) one identity instance of every geometry, which `whole` then holds
std::pair<const rt3_instance*, size_t> placements(const rt3_ctx* c, rt3_instance& whole);
SceneDev scene_dev(const rt3_ctx* c);
// the geometry tables of the flattened world
GeomTables world_tables(const rt3_ctx* c);
// the alpha-mask tables of a traversal launch over the current structure: empty (table null) without masked triangles.  The texture atlas
// must be synchronised (sync_textures) first.
AlphaDev alpha_dev(const rt3_ctx* c);
// what k_shadow_pane reads of a structure with panes (accel.n_panes != 0)
PaneDev pane_dev(const rt3_ctx* c);
int ensure_lights(rt3_ctx* c, uint32_t combo = RT3_F_NEE_EMISSIVE);  // combo: flags & (RT3_F_NEE_EMISSIVE | RT3_F_NEE_PUNCTUAL)
// RT3_OPT_SHADOW_EXIT_TABLE changed: the table of a built, current structure is refilled (or switched off) now
int exit_table_update(rt3_ctx* c);
// what the counters measured is no longer what the launches see (a new sky): they start again
void exit_counters_reset(rt3_ctx* c);

// ---- rt3_passes.hip
void motion_tables_stale(rt3_ctx* c);  // the previous transforms or the deformed flags changed: motion_tables remakes its tables
// motion_tables for the built structure (its refusals; it may synchronise the stream), then the tables as a kernel follows them: geom_slot
// null when nothing moved, *prev_pos null when nothing is deformed
int motion_launch_tables(rt3_ctx* c, MotionDev* m, const float4** prev_pos);
// self-test op 46 (include/rt3.h): k_fog_segment / k_fog_shadow on caller-made queues, with the light setup of a frame
int selftest_fog_queue(rt3_ctx* c, const uint32_t* in, uint32_t n, uint32_t* out);

// ---- rt3_tiles.hip
int get_pixlist(rt3_ctx* c, uint32_t w, uint32_t h, uint32_t rank, uint32_t n_ranks, PixelList** out);
// the list's {pixel, blue-noise word} records, (re)made when the blue noise was uploaded since
int pixlist_bluenoise(rt3_ctx* c, PixelList* pl);
void comm_release(rt3_ctx* c);  // rt3_destroy: the communicator goes with the context

}  // namespace rt3
