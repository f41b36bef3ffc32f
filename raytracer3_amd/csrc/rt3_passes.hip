// rt3_passes.hip -- host layer, the passes: the wavefront work queues and counter reservation, the primary trace, every pass function,
// the pass table kPasses and its validator, rt3_pass_launch, and the state of the "denoise", "temporal", "motion" and "adaptive" passes
// (include/rt3.h: rt3_pass_launch, rt3_denoise_*, rt3_temporal_*, rt3_adaptive_*).  Owns rt3_ctx::work, ::denoise, ::temporal, ::motion
// and ::adaptive.
// rt3_pass_launch() is the drop-in for executing one pass node of the reference's frame graph (render_graph/mod.rs:80-107): the pass
// name selects a HIP kernel sequence instead of a SPIR-V pipeline.
// Also owns rt3_ctx::lens: per-sample camera rays (rt3_camera_set_lens), which "refrence_mode", "postprocess" and
// "adaptive" read.
// Also owns rt3_ctx::roulette: Russian roulette on extension rays (rt3_path_set_roulette), which trace_batch applies
// for "refrence_mode" and "adaptive".
// trace_batch also launches k_absorb (rt3_scene_set_attenuation) when the built scene has an absorption table.
// Also owns the launch side of rt3_ctx::medium (rt3_scene_set_medium): the in-scatter shadow queues, the words of
// rt3_medium_info, and the k_fog_segment / k_fog_shadow launches of trace_batch.
// Also owns rt3_ctx::guide: the guide images of a lens frame (rt3_camera_set_guide_output, rt3_denoise_set_guide_input, DESIGN.md section
// 4u), which trace_batch writes with k_lens_guide for "refrence_mode" and "denoise" reads through the <DnGuide> instances of its two end
// kernels, and the two sets "temporal" reads through k_temporal<TemporalGuide> (rt3_temporal_set_guide_input); and
// the fifth image, the samples' mean previous position (rt3_camera_set_guide_motion_output, rt3_temporal_set_guide_motion_input, DESIGN.md
// section 4w), which trace_batch writes with k_lens_guide_prev and "temporal" reads through k_temporal<TemporalGuideMotion>.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "rt3_ctx.hpp"
#include "rt3_emit_tex.hpp"
#include "rt3_fog.hpp"
#include "rt3_roulette.hpp"
#include "rt3_volume.hpp"

using namespace rt3;

namespace rt3 {

void motion_tables_stale(rt3_ctx* c) { c->motion.dirty = true; }

}  // namespace rt3

namespace {

uint32_t spread1by1(uint32_t x) {  // math.slang:105-112 integer_explode
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}
uint32_t zcurve_host(uint32_t x, uint32_t y) { return spread1by1(x) | (spread1by1(y) << 1); }  // math.slang:114-117

// Failure-atomic: if any allocation fails the whole queue set is released and the capacities drop to 0, so the next pass
// re-allocates (or reports the error again) instead of launching kernels on a half-resized set.
void free_work(rt3_ctx* c) {
    for (int k = 0; k < 2; k++) { c->work.rays[k].reset(); c->work.T[k].reset(); }
    c->work.hits.reset(); c->work.sh_rays.reset(); c->work.sh_contrib.reset(); c->work.lacc.reset(); c->work.radsum.reset();
    c->work.sh2_rays.reset(); c->work.sh2_contrib.reset(); c->work.sh2_tmax.reset();
    c->work.cap_emit = 0;
    c->work.pane_dist.reset();
    c->work.cap_pane = 0;
    c->work.cap = 0;
    c->work.cap_pix = 0;
}
int ensure_work(rt3_ctx* c, size_t paths, size_t npix) {
    int r = RT3_OK;
    if (paths > c->work.cap) {
        size_t P = (paths + 255) & ~(size_t)255;
        c->work.cap = 0;
        for (int k = 0; k < 2 && !r; k++) {
            if (!r) r = dev_alloc(c, c->work.rays[k], 8 * P);
            if (!r) r = dev_alloc(c, c->work.T[k], 3 * P);  // throughput planes (the path's pdf and id ride in the ray records)
        }
        if (!r) r = dev_alloc(c, c->work.hits, 4 * P);
        if (!r) r = dev_alloc(c, c->work.sh_rays, 8 * P);
        if (!r) r = dev_alloc(c, c->work.sh_contrib, 2 * P);  // {blue contribution, path id} records (red / green ride with the ray)
        if (!r) r = dev_alloc(c, c->work.lacc, 4 * P);        // float4 per path
        if (!r) c->work.cap = P;
    }
    if (!r && npix > c->work.cap_pix) {
        c->work.cap_pix = 0;
        r = dev_alloc(c, c->work.radsum, 3 * npix);
        if (!r) c->work.cap_pix = npix;
    }
    if (r) free_work(c);
    return r;
}
// the emitter shadow queue, as large as the other queues (after ensure_work)
int ensure_emit_queue(rt3_ctx* c) {
    if (c->work.cap_emit >= c->work.cap) return RT3_OK;
    c->work.cap_emit = 0;
    int r = dev_alloc(c, c->work.sh2_rays, 8 * c->work.cap);
    if (!r) r = dev_alloc(c, c->work.sh2_contrib, 2 * c->work.cap);
    if (!r) r = dev_alloc(c, c->work.sh2_tmax, c->work.cap);
    if (!r) c->work.cap_emit = c->work.cap;
    else free_work(c);
    return r;
}

// the two in-scatter shadow queues of a medium, as large as the other queues (after ensure_work), and the info words
int ensure_fog_queues(rt3_ctx* c) {
    if (!c->medium.d_info) {
        HIPC(c, c->medium.d_info.alloc_bytes(16));
        HIPC(c, hipMemsetAsync(c->medium.d_info.get(), 0, 16, c->stream));
    }
    if (c->medium.cap >= c->work.cap && c->medium.q_rays[0]) return RT3_OK;
    c->medium.cap = 0;
    int r = RT3_OK;
    for (int k = 0; k < 2 && !r; k++) {
        r = dev_alloc(c, c->medium.q_rays[k], 8 * c->work.cap);
        if (!r) r = dev_alloc(c, c->medium.q_contrib[k], 2 * c->work.cap);
        if (!r) r = dev_alloc(c, c->medium.q_tmax[k], c->work.cap);
    }
    if (!r) c->medium.cap = c->work.cap;
    return r;
}
// a launch without a medium: the queues go (hipFree waits for the device)
void release_fog_queues(rt3_ctx* c) {
    if (!c->medium.q_rays[0] && !c->medium.q_rays[1]) return;
    for (int k = 0; k < 2; k++) { c->medium.q_rays[k].reset(); c->medium.q_contrib[k].reset(); c->medium.q_tmax[k].reset(); }
    c->medium.cap = 0;
}
FogDev fog_dev(const rt3_ctx* c) {
    const rt3_medium& m = c->medium.params;
    FogDev f;
    for (int k = 0; k < 3; k++) {
        f.sigma_t[k] = m.sigma_a[k] + m.sigma_s[k];
        f.sigma_s[k] = m.sigma_s[k];
        f.lo[k] = m.box_min[k];
        f.hi[k] = m.box_max[k];
    }
    f.g = m.g;
    return f;
}

// k_shade_pane's distance per path, as many as the queues hold (after ensure_work)
int ensure_pane_dist(rt3_ctx* c) {
    if (c->work.cap_pane >= c->work.cap) return RT3_OK;
    c->work.cap_pane = 0;
    int r = dev_alloc(c, c->work.pane_dist, c->work.cap);
    if (!r) c->work.cap_pane = c->work.cap;
    else free_work(c);
    return r;
}

int reserve_counters(rt3_ctx* c, uint32_t n, uint32_t* first) {
    if (c->work.counters_next + n > c->work.counters_cap) {
        HIPC(c, hipStreamSynchronize(c->stream));
        if (int r = harvest(c)) return r;
    }
    if (n > c->work.counters_cap) return fail(c, RT3_E_INVALID, "too many bounces x batches for the counter block");
    *first = c->work.counters_next;
    c->work.counters_next += n;
    HIPC(c, hipMemsetAsync(c->work.d_counters.get() + *first, 0, (size_t)n * 4, c->stream));
    return RT3_OK;
}
// a traversal launch over the context's queues (`stride` records), counting into its totals when RT3_OPT_COUNT_TRAVERSAL is on
TraceLaunch ctx_trace(rt3_ctx* c) {
    TraceLaunch L;
    L.stride = c->work.cap;
    L.count = c->opt.count;
    L.totals = c->opt.count ? c->work.d_totals.get() : nullptr;
    L.alpha = alpha_dev(c);
    return L;
}
// closest hits of the n primary rays in c->work.rays[0], into c->work.hits
int trace_primary(rt3_ctx* c, uint32_t n) {
    uint32_t wc_slot;
    if (int r = reserve_counters(c, 1, &wc_slot)) return r;  // ray-pool cursor of the launch
    TraceLaunch L = ctx_trace(c);
    L.rays = c->work.rays[0].get(); L.n = n; L.work_counter = c->work.d_counters.get() + wc_slot; L.hits = c->work.hits.get();
    c->work.primary_rays_pending += n;
    ScopedTimer t(c, CAT_EXTEND);
    launch_extend(c->stream, c->accel.bvh, L);
    return RT3_OK;
}

// The device tables of the "motion" pass for the built structure: per instance its previous matrix, per flattened geometry its slot --
// kMotionUnmoved, or its instance's index if that instance moved (the 12 stored floats of the two matrices differ in some word), or that
// index | kMotionDeformed if the geometry is deformed (deform_flags).  Without previous transforms a deformed geometry's record holds its
// instance's current matrix.  Remade when the previous transforms, the snapshot, the vertices or the structure changed; the count is
// checked at every launch.
int motion_tables(rt3_ctx* c) {
    rt3_instance whole;
    const auto [inst, n_inst] = placements(c, whole);
    const size_t n = c->scene.prev_transforms.size() / 16;
    if (n != 0 && n != n_inst)
        return fail(c, RT3_E_STATE, "motion: " + std::to_string(n) + " previous transforms (rt3_scene_set_prev_transforms) for a structure of " +
                                        std::to_string(n_inst) + " instance(s)");
    if (int r = deform_flags(c)) return r;
    if (!c->motion.dirty && c->motion.stamp == c->accel.stamp) return RT3_OK;
    const bool deformed_any = std::any_of(c->deform.h_deformed.begin(), c->deform.h_deformed.end(), [](uint32_t f) { return f != 0; });
    std::vector<MotionPrevDev> rec(n || deformed_any ? n_inst : 0);
    std::vector<uint8_t> moved(rec.size());
    std::vector<uint32_t> slot;
    bool any = false, any_deformed = false;
    for (size_t i = 0; i < rec.size(); i++) {
        const float *cm = inst[i].transform, *pm = n ? &c->scene.prev_transforms[16 * i] : cm;
        float cur[12];
        memset(&rec[i], 0, sizeof(rec[i]));
        pack3x4(pm, rec[i].m);
        pack3x4(cm, cur);
        rec[i].identity = memcmp(pm, kIdentity, sizeof(kIdentity)) == 0 ? 1u : 0u;
        moved[i] = memcmp(rec[i].m, cur, sizeof(cur)) != 0;  // word for word: -0 is not +0
    }
    if (!rec.empty())
        for (const Placed& p : c->accel.placed) {  // one slot per flattened geometry
            const bool deformed = p.geom < c->deform.h_deformed.size() && c->deform.h_deformed[p.geom];
            slot.push_back(deformed ? (p.instance | kMotionDeformed) : (moved[p.instance] ? p.instance : kMotionUnmoved));
            any = any || moved[p.instance] || deformed;
            any_deformed = any_deformed || deformed;
        }
    if (any) {
        HIPC(c, hipStreamSynchronize(c->stream));  // an earlier launch may still read the old tables
        if (int r = dev_alloc(c, c->motion.d_prev, rec.size())) return r;
        if (int r = dev_alloc(c, c->motion.d_slot, slot.size())) return r;
        HIPC(c, hipMemcpy(c->motion.d_prev.get(), rec.data(), rec.size() * sizeof(MotionPrevDev), hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(c->motion.d_slot.get(), slot.data(), slot.size() * 4, hipMemcpyHostToDevice));
    }
    c->motion.any_moved = any;
    c->motion.any_deformed = any_deformed;
    c->motion.dirty = false;
    c->motion.stamp = c->accel.stamp;
    return RT3_OK;
}

}  // namespace

namespace rt3 {

int motion_launch_tables(rt3_ctx* c, MotionDev* m, const float4** prev_pos) {
    if (int r = motion_tables(c)) return r;
    const GeomTables t = world_tables(c);
    m->verts = t.verts; m->indices = t.indices; m->geoms = t.geoms; m->prim_geom = t.prim_geom; m->first_prim = t.first_prim;
    m->geom_slot = c->motion.any_moved ? c->motion.d_slot.get() : nullptr;
    m->prev = c->motion.d_prev.get();
    *prev_pos = c->motion.any_deformed ? c->deform.d_prev_pos.get() : nullptr;
    return RT3_OK;
}

}  // namespace rt3

namespace {

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
// The primary rays of this rank's pixels of the W x H window (*out: the list) into c->work.rays[0], their closest hits into c->work.hits, in the
// list's order.  An empty list: nothing is allocated, nothing enqueued.
int primary_hits(rt3_ctx* c, const GConstDev& gd, uint32_t W, uint32_t H, PixelList** out) {
    if (int r = get_pixlist(c, W, H, c->tiles.rank, c->tiles.n_ranks, out)) return r;
    const PixelList* pl = *out;
    if (pl->count == 0) return RT3_OK;
    if (int r = ensure_work(c, pl->count, pl->count)) return r;
    {
        ScopedTimer t(c, CAT_OTHER);
        launch_raygen(c->stream, gd, pl->dev.get(), pl->count, c->work.rays[0].get(), c->work.cap);
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
        launch_gbuffer(c->stream, scene_dev(c), pl->dev.get(), pl->count, W, c->work.hits.get(), c->work.cap, res[0]->ptr, (float*)res[1]->ptr);
    }
    HIPC(c, hipGetLastError());
    return RT3_OK;
}

// What every batch of a path-tracing frame shares: the constants as the kernels see them, which estimators run, the light table
struct PathSetup {
    GConstDev gd;
    SceneDev sc;
    LightsDev lights{};
    bool nee = false, nee_e = false, punct = false;
    // textured emitters (rt3_scene_set_textured_emitters): the table's side array, null unless it holds a textured
    // emitter -- k_emit_tex
    const EmitTexDev* emit_tex = nullptr;
    // RT3_OPT_DEFER_SKY_LIGHT: k_shade_defer, k_shadow in its reporting mode, k_light.  Only inside their cover: sky NEE
    // on; no glass, punctual record or material table; every sky texel's density large enough that a sample's pdf cannot round to 0
    bool defer = false;
    // RT3_OPT_SHADE_EXIT_TEST: k_shade_defer_exit, the plain k_shadow from the root, k_light.  Only with deferral, an
    // exit table in use, no emitter queue, no alpha masks, no panes and no counting; `exit` is what the kernel needs of the structure
    bool shade_exit = false;
    ShadeExit exit{};
    bool lens_on = false;  // every sample starts from its own camera ray (rt3_camera_set_lens), not from the G-buffer ...
    LensDev lens{};        // ... made by these parameters
    // Russian roulette (rt3_path_set_roulette) on the extension rays of vertices rr_start .. B-2; off when no vertex is in that range
    bool rr = false;
    uint32_t rr_start = 0;
    float rr_min = 1.0f;
    // pane shadows (rt3_scene_set_pane_shadows): the built structure has panes -- k_shade_pane and k_shadow_pane
    bool panes = false;
    PaneDev pane{};
    // absorption (rt3_scene_set_attenuation): the built scene's table, null without an absorbing geometry -- k_absorb
    const AbsorbDev* absorb = nullptr;
    // guide images (rt3_camera_set_guide_output): the frame's four images, null unless "refrence_mode" resolved them -- k_lens_guide
    float4* guide[4] = {nullptr, nullptr, nullptr, nullptr};
    // the fifth (rt3_camera_set_guide_motion_output), null unless "refrence_mode" resolved it, and the "motion" pass's
    // tables and snapshot it follows -- k_lens_guide_prev
    float4* guide_prev = nullptr;
    MotionDev motion{};
    const float4* prev_pos = nullptr;
    // fog (rt3_scene_set_medium): a medium is on -- k_fog_segment behind every k_extend, k_fog_shadow ahead of the
    // surface vertices' k_shadow launches; fog_scatter: some sigma_s > 0 and the frame samples a light -- the in-scatter queues and their walks
    bool fog = false, fog_scatter = false;
    FogDev fogdev{};
};
// pl = pt / (2 pi^2 sin_theta) of a light sample is positive for every sin_theta in (0, 1] when the texel density pt is at least this
constexpr float kSkyDeferMinPdf = 0x1p-100f;
// (B = g->bounces >= 1; the queues must exist before an emitter queue can be sized: call after ensure_work)
int path_setup(rt3_ctx* c, const rt3_gconst* g, PathSetup* ps) {
    const uint32_t B = g->bounces;
    ps->gd = gconst_dev(g);
    // RT3_F_NEE_PUNCTUAL without lights, or with B = 1, is the frame without the bit, bit for bit: the kernels draw 8 RNG dimensions per
    // vertex for any flag word but 0, so the bit itself goes where it changes nothing else
    if (c->scene.lights.empty() || B <= 1) ps->gd.pad[0] &= ~RT3_F_NEE_PUNCTUAL;
    ps->nee = (g->pad[0] & RT3_F_NEE_SKY) && c->scene.d_sky;
    // RT3_F_NEE_EMISSIVE: only with something to sample; otherwise the frame is the flag-less one, same kernels
    // (and B >= 2: emitter shadow rays leave vertices 0 .. B-2)
    // RT3_F_NEE_PUNCTUAL (section 4k): the same, with the punctual lights as further entries of the table
    const uint32_t combo = g->pad[0] & (RT3_F_NEE_EMISSIVE | (c->scene.lights.empty() ? 0u : RT3_F_NEE_PUNCTUAL));
    if (combo && B > 1) {
        if (int r = ensure_lights(c, combo)) return r;
        ps->lights = c->accel.lights.dev();
        ps->punct = ps->lights.n != 0u && c->accel.lights.n_punct != 0u;
        if (ps->lights.n)
            if (int r = ensure_emit_queue(c)) return r;
    }
    ps->nee_e = ps->lights.n != 0u;
    ps->emit_tex = ps->nee_e && c->accel.lights.textured ? c->accel.lights.emit_tex.get() : nullptr;
    ps->sc = scene_dev(c);
    ps->fog = c->medium.on;
    if (ps->fog) {
        ps->fogdev = fog_dev(c);
        const float* ss = ps->fogdev.sigma_s;
        ps->fog_scatter = (ss[0] > 0.0f || ss[1] > 0.0f || ss[2] > 0.0f) && (ps->nee || ps->nee_e);
        if (int r = ensure_fog_queues(c)) return r;
    } else {
        release_fog_queues(c);
    }
    // (a medium: in a deferred frame sh_contrib holds vertices, not the contributions k_fog_shadow multiplies)
    ps->defer = !ps->fog && c->opt.defer_sky_light && ps->nee && !c->accel.has_glass && !ps->punct && ps->sc.mat_tex == nullptr && c->scene.sky_min_pdf >= kSkyDeferMinPdf;
    {
        const LbvhResult& bvh = c->accel.bvh;
        ps->shade_exit = c->opt.shade_exit_test && ps->defer && !ps->nee_e && !c->opt.count && alpha_dev(c).table == nullptr && c->accel.n_panes == 0u &&
                         bvh.exit.on && bvh.exit.off && bvh.exit.counters && bvh.layout == kLayoutWide64Q && bvh.nodes;
        if (ps->shade_exit) {
            ps->exit.arena = bvh.nodes.get();
            ps->exit.tri_off = bvh.tri_off;
            ps->exit.exit_off = bvh.exit.off;
            ps->exit.counters = bvh.exit.counters;
        }
    }
    ps->panes = c->accel.n_panes != 0u && c->accel.has_glass;
    if (ps->panes) {
        if (int r = ensure_pane_dist(c)) return r;
        ps->pane = pane_dev(c);
    }
    ps->absorb = c->accel.n_absorbing != 0u ? c->accel.d_absorb.get() : nullptr;
    ps->rr = c->roulette.on && c->roulette.params.start_bounce < B - 1u;
    ps->rr_start = c->roulette.params.start_bounce;
    ps->rr_min = c->roulette.params.min_survival;
    return RT3_OK;
}
LensDev lens_dev(const rt3_ctx* c) {
    const rt3_lens_params& p = c->lens.params;
    return LensDev{p.aperture_radius, p.focus_distance, p.pixel_jitter};
}
// A path-tracing launch begins: the roulette counts of rt3_path_roulette_info start again, and with roulette on the vertices' RNG indices may
// not reach the roulette draws' (kRouletteRngBase)
int roulette_begin(rt3_ctx* c, const char* pass, uint32_t samples, uint32_t bounces) {
    if (c->roulette.on && (uint64_t)samples * bounces * 8u > (1ull << 30))
        return fail(c, RT3_E_INVALID, std::string(pass) + " with roulette: samples * bounces * 8 may not exceed 2^30 (the roulette draws' RNG indices start behind it)");
    c->work.launch_serial++;
    c->work.roulette_tested = c->work.roulette_ended = 0;
    return RT3_OK;
}
// Ahead of roulette_begin, so that a refused launch leaves its counts alone: with a medium on the fog draws' RNG indices, 8 per (sample,
// segment) from kFogRngBase, may not run into the camera's (kLensRngBase)
int fog_range_check(rt3_ctx* c, const char* pass, uint32_t samples, uint32_t bounces) {
    if (c->medium.on && (uint64_t)samples * bounces * kFogRngDims > (uint64_t)(kLensRngBase - kFogRngBase))
        return fail(c, RT3_E_INVALID, std::string(pass) + " with a medium: samples * bounces * 8 may not exceed 2^28 (the fog draws' RNG indices end where the camera's start)");
    return RT3_OK;
}
// A path-tracing launch begins (behind roulette_begin): the counts of rt3_medium_info start again
int fog_begin(rt3_ctx* c) {
    if (c->medium.d_info) HIPC(c, hipMemsetAsync(c->medium.d_info.get(), 0, 16, c->stream));
    return RT3_OK;
}
// One wavefront batch: samples s0 .. s0 + nsb - 1 of the npix listed pixels (path id = sample_in_batch * npix + index) through all B
// bounces; each path's radiance ends up in c->work.lacc.  The loop body of "refrence_mode", and of a round of "adaptive".
int trace_batch(rt3_ctx* c, const PathSetup& ps, uint32_t W, const Resource* gb, const Resource* dp, const uint32_t* pixels, const uint2* pixbn,
                uint32_t npix, uint32_t s0, uint32_t nsb) {
    const uint32_t B = ps.gd.bounces;
    const size_t S = c->work.cap;
    const bool nee = ps.nee, nee_e = ps.nee_e;
    const uint32_t n_first = nsb * npix;
    const bool lens = ps.lens_on;
    const uint32_t n_words = (nee_e ? 6 : 4) * B;
    uint32_t first;
    // (a lens frame: two words more, the camera queue's length and the ray-pool cursor of its k_extend launch)
    // (roulette: B words more, [b] the extension queue's length after k_roulette of bounce b)
    const bool rr = ps.rr;
    // (the exit test in the shade kernel: B words more, [b] the sky shadow rays of bounce b that were decided there and never queued)
    const bool shade_exit = ps.shade_exit;
    // (a medium that scatters: 4 B words more, per segment the two in-scatter queues' lengths, then the ray-pool cursors of their k_shadow launches)
    const bool fog = ps.fog, fog_sc = ps.fog && ps.fog_scatter;
    if (int r = reserve_counters(c, n_words + 1 + (lens ? 2 : 0) + (rr ? B : 0) + (shade_exit ? B : 0) + (fog_sc ? 4 * B : 0), &first)) return r;
    first += first & 1u;  // 8-byte aligned pairs
    // pair b = {extension rays emitted at bounce b (b < B-1), shadow rays emitted at bounce b}; then the ray-pool cursors
    uint32_t* pairs = c->work.d_counters.get() + first;
    uint32_t* pool_cur = c->work.d_counters.get() + first + 2 * B;  // [b], [B + b]: ray-pool cursors of the k_extend / k_shadow launch of bounce b
    // with emitter NEE: [4B + b] emitter shadow rays emitted at bounce b, [5B + b] the ray-pool cursor of their k_shadow launch
    uint32_t* emit_cnt = c->work.d_counters.get() + first + 4 * B;
    uint32_t* lens_cnt = c->work.d_counters.get() + first + n_words;  // [0] the camera queue's length, [1] its ray-pool cursor
    uint32_t* rr_cnt = lens_cnt + (lens ? 2 : 0);
    uint32_t* dec_cnt = rr_cnt + (rr ? B : 0);
    uint32_t* fog_cnt = dec_cnt + (shade_exit ? B : 0);  // [2 seg + q]: queue q's length for segment seg; [2 B + 2 seg + q]: its ray-pool cursor
    c->work.pending_counters.push_back(CounterBlock{first, B, first + 4 * B, nee_e ? B : 0u, rr ? first + n_words + (lens ? 2u : 0u) : 0u, ps.rr_start,
                                                    c->work.launch_serial, shade_exit ? (uint32_t)(dec_cnt - c->work.d_counters.get()) : 0u});
    auto ext_cnt_at = [pairs](uint32_t b) { return pairs + 2 * b; };
    auto sh_cnt_at = [pairs](uint32_t b) { return pairs + 2 * b + 1; };
    int cur = 0;
    const uint32_t* live_cnt = lens ? lens_cnt : nullptr;  // the length of the queue the next k_shade reads
    // Fog on segment `seg` (0: the camera's; b + 1: the one the k_extend of bounce b has just closed), the records of queue `q`: the
    // throughputs are attenuated; with scattering one point per segment is lit, and its shadow rays are walked at once, the sky sample's
    // queue first, then the light table's, so that a path's radiance slot sees a fixed sequence of adds
    auto fog_segment = [&](uint32_t seg, int q, const uint32_t* count, float* lacc_miss) {
        FogSegmentLaunch F{};
        F.fog = ps.fogdev; F.sc = ps.sc; F.lights = ps.lights; F.emit_tex = ps.emit_tex;
        F.rays = c->work.rays[q].get(); F.hits = c->work.hits.get(); F.T = c->work.T[q].get(); F.count = count; F.stride = S;
        F.lacc_miss = lacc_miss;
        F.scatter = fog_sc ? 1u : 0u; F.sky = fog_sc && nee ? 1u : 0u;
        if (!fog_sc) F.lights.n = 0u;
        for (int k = 0; k < 2; k++) {
            F.q_rays[k] = c->medium.q_rays[k].get(); F.q_contrib[k] = c->medium.q_contrib[k].get(); F.q_tmax[k] = c->medium.q_tmax[k].get();
            F.q_count[k] = fog_sc ? fog_cnt + 2 * seg + k : nullptr;
        }
        F.q_stride = S;
        F.pixels = pixels; F.npix = npix; F.s0 = s0; F.bounces = B; F.segment = seg; F.frame = ps.gd.frame;
        F.info = c->medium.d_info.get();
        {
            ScopedTimer t(c, CAT_OTHER);
            launch_fog_segment(c->stream, F, n_first);
        }
        for (int k = 0; k < 2 && fog_sc; k++) {
            if (k == 0 ? !nee : !nee_e) continue;
            TraceLaunch tr = ctx_trace(c);
            tr.rays = c->medium.q_rays[k].get(); tr.count_ptr = fog_cnt + 2 * seg + k; tr.n = n_first; tr.work_counter = fog_cnt + 2 * B + 2 * seg + k;
            tr.contrib = c->medium.q_contrib[k].get(); tr.lacc = c->work.lacc.get(); tr.tmax = c->medium.q_tmax[k].get();
            if (ps.panes) tr.pane = &ps.pane;
            ScopedTimer t(c, CAT_SHADOW);
            launch_shadow(c->stream, c->accel.bvh, tr);
        }
    };
    // the light samples k_shade has just queued, before their walk adds them in
    auto fog_shadow = [&](float* rays, float* contrib, const float* tmax, const uint32_t* count) {
        FogShadowLaunch F{};
        F.fog = ps.fogdev; F.rays = rays; F.contrib = contrib; F.tmax = tmax; F.count = count; F.stride = S;
        ScopedTimer t(c, CAT_OTHER);
        launch_fog_shadow(c->stream, F, n_first);
    };
    if (lens) {
        // Vertex 0 of a lens frame: the camera rays become records of the extension queue rays[0], are traced as extension rays (payload:
        // the .w words carry pdf and id, so a camera ray starts at kRayTMin like every extension ray, not at 0 like the G-buffer's), and are
        // shaded below by k_shade<FIRST = false> at bounce 0, which reads the queue's length from lens_cnt[0].
        {
            ScopedTimer t(c, CAT_OTHER);
            launch_lens_rays(c->stream, ps.gd, ps.lens, pixels, npix, s0, n_first, c->work.rays[0].get(), c->work.T[0].get(), c->work.lacc.get(), S,
                             lens_cnt);
        }
        {
            TraceLaunch tr = ctx_trace(c);
            tr.rays = c->work.rays[0].get(); tr.n = n_first; tr.work_counter = lens_cnt + 1; tr.hits = c->work.hits.get(); tr.payload = true;
            c->work.primary_rays_pending += n_first;
            ScopedTimer t(c, CAT_EXTEND);
            launch_extend(c->stream, c->accel.bvh, tr);
        }
        // an escaped camera sample collects the sky once: in k_shade's miss branch with weight 1 under sky NEE, here otherwise
        if (!nee && ps.sc.sky != nullptr) {
            ScopedTimer t(c, CAT_OTHER);
            launch_lens_miss(c->stream, ps.sc, c->work.rays[0].get(), c->work.hits.get(), c->work.lacc.get(), S, n_first);
        }
        // the camera segment in the medium, behind k_lens_miss: the sky an escaped sample took there with throughput 1 is attenuated in
        // this launch (under sky NEE the first k_shade's miss branch takes it, with the throughput this launch leaves)
        if (fog) fog_segment(0u, 0, lens_cnt, !nee && ps.sc.sky != nullptr ? c->work.lacc.get() : nullptr);
        // the first-vertex features of this batch's samples, while the camera queue and its hits are whole: the first k_shade overwrites
        // neither, but the k_extend behind it overwrites the hits
        if (ps.guide[0] != nullptr) {
            GuideLaunch G{};
            G.sc = ps.sc; G.pixels = pixels; G.npix = npix; G.width = W; G.rays = c->work.rays[0].get(); G.hits = c->work.hits.get(); G.stride = S;
            G.nsb = nsb; G.samples = ps.gd.samples; G.first_batch = s0 == 0; G.last_batch = s0 + nsb >= ps.gd.samples;
            for (int k = 0; k < 4; k++) G.img[k] = ps.guide[k];
            ScopedTimer t(c, CAT_OTHER);
            launch_lens_guide(c->stream, G);
            if (ps.guide_prev != nullptr) {  // where the same samples' points were one frame ago, from the same two queues
                GuidePrevLaunch P{};
                P.m = ps.motion; P.prev_pos = ps.prev_pos; P.pixels = pixels; P.npix = npix; P.width = W; P.rays = G.rays; P.hits = G.hits; P.stride = S;
                P.nsb = nsb; P.samples = G.samples; P.first_batch = G.first_batch; P.last_batch = G.last_batch; P.out = ps.guide_prev;
                launch_lens_guide_prev(c->stream, P);
            }
        }
    }
    // every path starts at distance 0 from the vertex that chose its direction (the camera)
    if (ps.panes) HIPC(c, hipMemsetAsync(c->work.pane_dist.get(), 0, (size_t)n_first * sizeof(float), c->stream));
    for (uint32_t bn = 0; bn < B; bn++) {
        ShadeLaunch L;
        L.g = ps.gd; L.sc = ps.sc; L.pixels = pixels; L.pixbn = pixbn; L.npix = npix; L.width = W; L.s0 = s0; L.bounce = bn;
        L.gbuffer = (const uint4*)gb->ptr; L.depth = (const float*)dp->ptr;
        L.in_rays = c->work.rays[cur].get(); L.in_hits = c->work.hits.get(); L.in_T = c->work.T[cur].get();
        L.in_count = live_cnt; L.n_first = n_first;
        L.out_rays = c->work.rays[cur ^ 1].get(); L.out_T = c->work.T[cur ^ 1].get(); L.out_count = ext_cnt_at(bn);
        L.sh_rays = c->work.sh_rays.get(); L.sh_contrib = c->work.sh_contrib.get(); L.sh_count = sh_cnt_at(bn);
        L.lacc = c->work.lacc.get(); L.stride = S;
        L.lights = ps.lights;
        L.sh2_rays = c->work.sh2_rays.get(); L.sh2_contrib = c->work.sh2_contrib.get(); L.sh2_tmax = c->work.sh2_tmax.get(); L.sh2_count = emit_cnt + bn;
        {
            ScopedTimer t(c, CAT_SHADE);
            // (glass only with a lens: pass_reference_mode and pass_adaptive see to it)
            ShadeExit sx = ps.exit;
            sx.decided = dec_cnt + bn;
            launch_shade(c->stream, bn == 0 && !lens, L, ps.punct, c->accel.has_glass ? c->accel.d_glass.get() : nullptr, ps.defer,
                         ps.panes ? c->work.pane_dist.get() : nullptr, shade_exit ? &sx : nullptr, c->accel.has_glass && c->accel.n_frosted != 0u);
        }
        cur ^= 1;
        if (nee && fog) fog_shadow(c->work.sh_rays.get(), c->work.sh_contrib.get(), nullptr, sh_cnt_at(bn));
        if (nee) {
            TraceLaunch tr = ctx_trace(c);
            tr.rays = c->work.sh_rays.get(); tr.count_ptr = sh_cnt_at(bn); tr.n = n_first; tr.work_counter = pool_cur + B + bn;
            if (ps.defer) {  // report only, into the second plane of sh_contrib; the first holds the rays' vertices
                tr.occluded = reinterpret_cast<uint32_t*>(c->work.sh_contrib.get()) + S;
                tr.from_root = shade_exit;  // the queue holds what the entries' leaves did not occlude
            } else {
                tr.contrib = c->work.sh_contrib.get(); tr.lacc = c->work.lacc.get();
                if (ps.panes) tr.pane = &ps.pane;
            }
            ScopedTimer t(c, CAT_SHADOW);
            launch_shadow(c->stream, c->accel.bvh, tr);
        }
        if (ps.defer) {
            // before the emitter launch (which adds into the same radiance slots after the sky's), before k_roulette (which overwrites the
            // half of the ray pair k_shade_defer read) and before k_extend (which overwrites the hit queue)
            ScopedTimer t(c, CAT_SHADE);
            launch_light(c->stream, bn == 0 && !lens, L);
        }
        if (nee_e && bn + 1 < B && ps.emit_tex != nullptr) {
            // the queued emitter samples' contributions carry Le = the factor: those on a textured emitter take their texel here, before
            // the walk adds them in
            EmitTexLaunch E{};
            E.sc = ps.sc; E.lights = ps.lights; E.emit_tex = ps.emit_tex;
            E.rays = c->work.sh2_rays.get(); E.contrib = c->work.sh2_contrib.get(); E.count = emit_cnt + bn; E.stride = S;
            E.pixels = pixels; E.npix = npix; E.s0 = s0; E.bounces = B; E.bounce = bn; E.frame = ps.gd.frame; E.dims = ps.gd.pad[0] ? 8u : 2u;
            ScopedTimer t(c, CAT_OTHER);
            launch_emit_tex(c->stream, E, n_first);
            c->prof.stats.emit_tex_launches++;
        }
        // (behind k_emit_tex: the two products commute only up to rounding)
        if (nee_e && bn + 1 < B && fog) fog_shadow(c->work.sh2_rays.get(), c->work.sh2_contrib.get(), c->work.sh2_tmax.get(), emit_cnt + bn);
        if (nee_e && bn + 1 < B) {  // after the sky's: the two add into the same radiance slots, one launch after the other
            TraceLaunch tr = ctx_trace(c);
            tr.rays = c->work.sh2_rays.get(); tr.count_ptr = emit_cnt + bn; tr.n = n_first; tr.work_counter = emit_cnt + B + bn;
            tr.contrib = c->work.sh2_contrib.get(); tr.lacc = c->work.lacc.get(); tr.tmax = c->work.sh2_tmax.get();
            if (ps.panes) tr.pane = &ps.pane;
            ScopedTimer t(c, CAT_SHADOW);
            launch_shadow(c->stream, c->accel.bvh, tr);
        }
        live_cnt = ext_cnt_at(bn);
        if (rr && bn >= ps.rr_start && bn != B - 1) {
            // k_shade has read the other half of the ping-pong pair: the survivors go there, and k_extend and the next k_shade read them
            RouletteLaunch R{};
            R.in_rays = c->work.rays[cur].get(); R.in_T = c->work.T[cur].get(); R.in_count = live_cnt;
            R.out_rays = c->work.rays[cur ^ 1].get(); R.out_T = c->work.T[cur ^ 1].get(); R.out_count = rr_cnt + bn;
            R.stride = S; R.pixels = pixels; R.npix = npix; R.s0 = s0; R.bounces = B; R.bounce = bn; R.frame = ps.gd.frame;
            R.min_survival = ps.rr_min;
            ScopedTimer t(c, CAT_OTHER);
            launch_roulette(c->stream, R, n_first);
            cur ^= 1;
            live_cnt = rr_cnt + bn;
        }
        if (bn != B - 1) {
            TraceLaunch tr = ctx_trace(c);
            tr.rays = c->work.rays[cur].get(); tr.count_ptr = live_cnt; tr.n = n_first; tr.work_counter = pool_cur + bn;
            tr.hits = c->work.hits.get(); tr.payload = true;
            ScopedTimer t(c, CAT_EXTEND);
            launch_extend(c->stream, c->accel.bvh, tr);
        }
        if (ps.absorb != nullptr && bn != B - 1) {
            // the segments k_extend has just closed (vertex bn -> vertex bn + 1 >= 1) that ran inside an absorbing solid, before the k_shade of
            // vertex bn + 1 reads their throughput
            AbsorbLaunch A{};
            A.rays = c->work.rays[cur].get(); A.hits = c->work.hits.get(); A.T = c->work.T[cur].get(); A.count = live_cnt; A.stride = S;
            A.tri_shade = ps.sc.tri_shade; A.shade_geoms = ps.sc.shade_geoms; A.table = ps.absorb;
            ScopedTimer t(c, CAT_OTHER);
            launch_absorb(c->stream, A, n_first);
        }
        // behind k_absorb (the two products commute only up to rounding): the same segments, where they run through the medium
        if (fog && bn != B - 1) fog_segment(bn + 1u, cur, live_cnt, nullptr);
    }
    return RT3_OK;
}
// paths per wavefront batch: 160 B of queue state each, so 2^28 paths = 43 GB of the 288 GB; the C3 frame (132.7 M paths)
// is ONE batch.  Larger launches amortise the ramp / tail of the persistent traversal kernels: 16 -> 64 spp per batch = -6.5 % frame time.
// *sb: the samples of a batch over npix >= 1 pixels that are to get `spp` samples (RT3_OPT_BATCH_SPP, or as many as fit)
int batch_spp(rt3_ctx* c, uint32_t npix, uint32_t spp, uint32_t* sb) {
    uint64_t max_paths = 1ull << 28;
    *sb = c->opt.batch_spp > 0 ? (uint32_t)c->opt.batch_spp : (uint32_t)std::max<uint64_t>(1, max_paths / npix);
    if (*sb > spp) *sb = spp;
    if ((uint64_t)*sb * npix > 0xFFFFFF00ull) return fail(c, RT3_E_INVALID, "batch too large");
    return RT3_OK;
}

// The four images of a guide set as the launch sees them: live RGBA32F images of the window's size, none of them
// one of the `n_not` images `not_these` (named `not_names` in the error); their device pointers into `out`.  RT3_E_INVALID otherwise.
int guide_resolve(rt3_ctx* c, const rt3_guide_images& gi, uint32_t W, uint32_t H, const std::string& what, const Resource* const* not_these,
                  uint32_t n_not, const char* not_names, float4** out) {
    const uint32_t handles[4] = {gi.position, gi.normal, gi.albedo, gi.emission};
    const char* names[4] = {"position", "normal", "albedo", "emission"};
    for (int k = 0; k < 4; k++) {
        const Resource* r = image_checked(c, handles[k], W, H, RT3_FORMAT_R32G32B32A32_SFLOAT,(what + " image '" + names[k] + "'").c_str());
        if (!r) return RT3_E_INVALID;
        for (uint32_t j = 0; j < n_not; j++)
            if (r->ptr == not_these[j]->ptr) return fail(c, RT3_E_INVALID, what + " image '" + names[k] + "' must not be " + not_names);
        out[k] = static_cast<float4*>(r->ptr);
    }
    return RT3_OK;
}

// refrence_mode.slang:14-66 as a wavefront loop
int pass_reference_mode(rt3_ctx* c, const rt3_gconst* g, uint32_t W, uint32_t H, Resource* const* res) {
    const Resource *gb = res[0], *dp = res[1], *li = res[2], *pv = res[3];
    const uint32_t Sspp = g->samples, B = g->bounces;
    float4* guide[4] = {nullptr, nullptr, nullptr, nullptr};
    if (c->guide.out_on) {  // DESIGN.md section 4u; before anything is enqueued: a refused launch changes nothing
        if (!c->lens.on)
            return fail(c, RT3_E_STATE, "refrence_mode: a guide output is set (rt3_camera_set_guide_output) and no lens is on (rt3_camera_set_lens): the guide "
                                        "images are means over per-sample camera rays");
        if (Sspp > (1u << 24))
            return fail(c, RT3_E_INVALID, "refrence_mode with a guide output: samples may not exceed 2^24 (the hit count is kept in a float)");
        const Resource* const written[2] = {li, pv};
        if (int r = guide_resolve(c, c->guide.out, W, H, "refrence_mode: guide output", written, 2, "'Light' or 'PrevLight'", guide)) return r;
    }
    float4* guide_prev = nullptr;
    MotionDev motion{};
    const float4* prev_pos = nullptr;
    if (c->guide.motion_out) {  // DESIGN.md section 4w; before anything is enqueued too
        if (!c->guide.out_on)
            return fail(c, RT3_E_STATE, "refrence_mode: a guide motion output is set (rt3_camera_set_guide_motion_output) and no guide output "
                                        "(rt3_camera_set_guide_output): the image is written beside the four, from the same samples");
        const Resource* r = image_checked(c, c->guide.motion_out, W, H, RT3_FORMAT_R32G32B32A32_SFLOAT, "refrence_mode: guide motion output");
        if (!r) return RT3_E_INVALID;
        if (r->ptr == li->ptr || r->ptr == pv->ptr)
            return fail(c, RT3_E_INVALID, "refrence_mode: the guide motion output must not be 'Light' or 'PrevLight'");
        for (int k = 0; k < 4; k++)
            if (r->ptr == guide[k]) return fail(c, RT3_E_INVALID, "refrence_mode: the guide motion output must not be one of the four guide images");
        if (int e = motion_launch_tables(c, &motion, &prev_pos)) return e;
        guide_prev = static_cast<float4*>(r->ptr);
    }
    if (Sspp == 0 || B == 0) return RT3_OK;  // GConst::default() leaves samples = bounces = 0 (renderer/mod.rs:47-63): nothing to trace
    if (B > 64) return fail(c, RT3_E_INVALID, "bounces > 64");
    if (c->lens.on && (uint64_t)Sspp * B * 8u > (1ull << 31))
        return fail(c, RT3_E_INVALID, "refrence_mode with a lens: samples * bounces * 8 may not exceed 2^31 (the camera's RNG indices start there)");
    if (c->accel.has_glass) {
        if (!c->lens.on)
            return fail(c, RT3_E_STATE, "refrence_mode: the scene has glass (rt3_scene_set_transmission) and the packed G-buffer has no room for a material "
                                        "class: start every sample from its own camera ray with rt3_camera_set_lens ({0, f, 0} is the per-sample pinhole)");
        if ((uint64_t)Sspp * B * 8u > (1ull << 30))
            return fail(c, RT3_E_INVALID, "refrence_mode with glass: samples * bounces * 8 may not exceed 2^30 (the glass draws' RNG indices start there)");
    }
    if (c->medium.on) {
        if (!c->lens.on)
            return fail(c, RT3_E_STATE, "refrence_mode: a medium is set (rt3_scene_set_medium) and the camera segment of a G-buffer frame is no record of the "
                                        "extension queue: start every sample from its own camera ray with rt3_camera_set_lens ({0, f, 0} is the per-sample pinhole)");
    }
    if (int r = fog_range_check(c, "refrence_mode", Sspp, B)) return r;
    if (int r = roulette_begin(c, "refrence_mode", Sspp, B)) return r;
    if (int r = fog_begin(c)) return r;
    PixelList* pl;
    if (int r = get_pixlist(c, W, H, c->tiles.rank, c->tiles.n_ranks, &pl)) return r;
    const uint32_t npix = pl->count;
    if (npix == 0) return RT3_OK;
    if (int r = pixlist_bluenoise(c, pl)) return r;
    uint32_t sb;
    if (int r = batch_spp(c, npix, Sspp, &sb)) return r;
    if (int r = ensure_work(c, (size_t)sb * npix, npix)) return r;
    PathSetup ps;
    if (int r = path_setup(c, g, &ps)) return r;
    ps.lens_on = c->lens.on;
    ps.lens = lens_dev(c);
    for (int k = 0; k < 4; k++) ps.guide[k] = guide[k];
    ps.guide_prev = guide_prev;
    ps.motion = motion;
    ps.prev_pos = prev_pos;
    for (uint32_t s0 = 0; s0 < Sspp; s0 += sb) {
        const uint32_t nsb = std::min(sb, Sspp - s0);
        if (int r = trace_batch(c, ps, W, gb, dp, pl->dev.get(), pl->dev_bn.get(), npix, s0, nsb)) return r;
        {
            ScopedTimer t(c, CAT_OTHER);
            if (ps.lens_on)  // every listed pixel: one whose centre sees the background may be partly covered
                launch_accumulate_lens(c->stream, ps.gd, pl->dev.get(), npix, W, c->work.lacc.get(), nsb, s0 == 0, s0 + nsb >= Sspp, c->work.radsum.get(),
                                       li->ptr, pv->ptr);
            else
                launch_accumulate(c->stream, ps.gd, pl->dev.get(), npix, W, (const float*)dp->ptr, c->work.lacc.get(), c->work.cap, nsb, s0 == 0, s0 + nsb >= Sspp,
                                  c->work.radsum.get(), li->ptr, pv->ptr);
        }
    }
    HIPC(c, hipGetLastError());
    return RT3_OK;
}

// "adaptive": refrence_mode to a noise threshold, GConst.samples the cap (no reference counterpart).  The rounds'
// paths are trace_batch's; the pixel list shrinks between rounds.  The length of the next list comes back to the host once per round (4
// bytes behind one stream synchronisation): npix and its fast_div constant are launch arguments of k_shade, and sizes every grid.
int pass_adaptive(rt3_ctx* c, const rt3_gconst* g, uint32_t W, uint32_t H, Resource* const* res) {
    const Resource *gb = res[0], *dp = res[1], *li = res[2], *pv = res[3], *mo = res[4];
    const rt3_adaptive_params& p = c->adaptive.params;
    const uint32_t cap = g->samples, B = g->bounces;
    c->adaptive.rounds = c->adaptive.pixels_capped = 0;
    c->adaptive.paths_traced = 0;
    // coverage mode (rt3_adaptive_set_coverage): with a lens every pixel of the rank's list is a pixel of round 0
    const bool cover = c->lens.on && c->adaptive.coverage;
    if (c->guide.out_on)
        return fail(c, RT3_E_STATE, "adaptive: not while a guide output is set (rt3_camera_set_guide_output): the pass writes no guide images, and a "
                                    "stale guide would be filtered; switch it off (NULL) or use refrence_mode");
    if (c->lens.on && !cover)
        return fail(c, RT3_E_STATE, "adaptive: not with a lens set (rt3_camera_set_lens): the pass selects pixels by G-buffer depth, which knows nothing "
                                    "of partly covered pixels; switch the lens off (NULL), use refrence_mode, or let the pass take every pixel with "
                                    "rt3_adaptive_set_coverage");
    if (c->accel.has_glass && !cover)
        return fail(c, RT3_E_STATE, "adaptive: not for a scene with glass (rt3_scene_set_transmission): glass needs per-sample camera rays "
                                    "(rt3_camera_set_lens), which this pass does not take; use refrence_mode");
    if (c->medium.on && !cover)
        return fail(c, RT3_E_STATE, "adaptive: not with a medium set (rt3_scene_set_medium) outside coverage mode: fog needs per-sample camera rays "
                                    "(rt3_camera_set_lens with rt3_adaptive_set_coverage); or use refrence_mode");
    if (cap == 0 || B == 0) return RT3_OK;  // like refrence_mode
    if (B > 64) return fail(c, RT3_E_INVALID, "bounces > 64");
    if (cover) {  // refrence_mode's range rules, the cap as `samples`
        if ((uint64_t)cap * B * 8u > (1ull << 31))
            return fail(c, RT3_E_INVALID, "adaptive with a lens: samples * bounces * 8 may not exceed 2^31 (the camera's RNG indices start there)");
        if (c->accel.has_glass && (uint64_t)cap * B * 8u > (1ull << 30))
            return fail(c, RT3_E_INVALID, "adaptive with glass: samples * bounces * 8 may not exceed 2^30 (the glass draws' RNG indices start there)");
    }
    if (int r = fog_range_check(c, "adaptive", cap, B)) return r;
    if (int r = roulette_begin(c, "adaptive", cap, B)) return r;
    if (int r = fog_begin(c)) return r;
    PixelList* pl;
    if (int r = get_pixlist(c, W, H, c->tiles.rank, c->tiles.n_ranks, &pl)) return r;
    if (pl->count == 0) return RT3_OK;
    if (int r = pixlist_bluenoise(c, pl)) return r;
    AdaptiveScratch s;
    BufLayout plan;
    adaptive_plan(W, H, pl->count, plan, &s);
    if (c->adaptive.scratch.capacity_bytes() < plan.bytes()) {  // the stream may still read the old allocation
        HIPC(c, hipStreamSynchronize(c->stream));
        HIPC(c, c->adaptive.scratch.grow_bytes(plan.bytes()));
    }
    HIPC(c, plan.carve(c->adaptive.scratch));
    const float* depth = (const float*)dp->ptr;
    // the length of the list launch_adaptive_compact wrote last
    auto list_length = [&](uint32_t* n) {
        HIPC(c, hipMemcpyAsync(n, s.count, 4, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
        return (int)RT3_OK;
    };
    // round 0's list: the foreground pixels of the rank's list, in its order; in coverage mode the rank's list itself, whose length the
    // host knows
    uint32_t n_act = 0;
    int cur = 0;
    const uint32_t* list_xy = s.xy[cur];
    const uint2* list_bn = s.bn[cur];
    {
        ScopedTimer t(c, CAT_OTHER);
        HIPC(c, hipMemsetAsync(s.mask, 0, (size_t)W * H, c->stream));
        if (!cover) {
            launch_adaptive_init(c->stream, pl->dev.get(), pl->count, W, depth, s, mo->ptr);
            launch_adaptive_compact(c->stream, pl->dev_bn.get(), pl->count, W, H, 0u, s, cur);
        }
    }
    if (cover) {
        n_act = pl->count;
        list_xy = pl->dev.get();
        list_bn = pl->dev_bn.get();
    } else if (int r = list_length(&n_act)) {
        return r;
    }
    const uint32_t n_fg = n_act;
    if (n_fg) {
        // the queues are sized once, for the largest batch of any round: round 0's list is the longest
        const uint32_t most = std::max(std::min(p.min_samples, cap), std::min(p.step, cap));
        uint32_t sb;
        if (int r = batch_spp(c, n_fg, most, &sb)) return r;
        if (int r = ensure_work(c, (size_t)sb * n_fg, 0)) return r;
    }
    PathSetup ps;
    if (n_fg)
        if (int r = path_setup(c, g, &ps)) return r;
    ps.lens_on = cover;
    ps.lens = lens_dev(c);
    uint32_t n = 0;  // the sample count of every active pixel
    while (n_act) {
        const uint32_t ns = n == 0 ? std::min(p.min_samples, cap) : std::min(p.step, cap - n);
        uint32_t sb;
        if (int r = batch_spp(c, n_act, ns, &sb)) return r;
        sb = (uint32_t)std::min<uint64_t>(sb, c->work.cap / n_act);  // (a shorter list may not take more samples per batch than the queues hold)
        for (uint32_t s0 = 0; s0 < ns; s0 += sb) {
            const uint32_t nsb = std::min(sb, ns - s0);
            if (int r = trace_batch(c, ps, W, gb, dp, list_xy, list_bn, n_act, n + s0, nsb)) return r;
            ScopedTimer t(c, CAT_OTHER);
            launch_adaptive_accumulate(c->stream, list_xy, n_act, W, c->work.lacc.get(), nsb, n + s0 == 0, n + s0 + nsb, s);
        }
        n += ns;
        c->adaptive.rounds++;
        c->adaptive.paths_traced += (uint64_t)ns * n_act;
        if (n >= cap) {
            c->adaptive.pixels_capped = n_act;
            break;
        }
        {
            ScopedTimer t(c, CAT_OTHER);
            launch_adaptive_test(c->stream, list_xy, n_act, W, p.threshold, p.dark, s);
            launch_adaptive_compact(c->stream, list_bn, n_act, W, H, p.dilate, s, cur ^ 1);
        }
        cur ^= 1;
        list_xy = s.xy[cur];
        list_bn = s.bn[cur];
        if (int r = list_length(&n_act)) return r;
    }
    {
        ScopedTimer t(c, CAT_OTHER);
        if (cover)
            launch_adaptive_finalise_all(c->stream, pl->dev.get(), pl->count, W, g->blendfactor, cap, s, li->ptr, pv->ptr, mo->ptr);
        else
            launch_adaptive_finalise(c->stream, pl->dev.get(), pl->count, W, depth, g->blendfactor, cap, s, li->ptr, pv->ptr, mo->ptr);
    }
    HIPC(c, hipGetLastError());
    return RT3_OK;
}

// postprocess.slang:90-112
int pass_postprocess(rt3_ctx* c, const rt3_gconst* g, uint32_t W, uint32_t H, Resource* const* res) {
    const Resource *dp = res[0], *out = res[1], *in = res[2];
    PixelList* pl;
    if (int r = get_pixlist(c, W, H, c->tiles.rank, c->tiles.n_ranks, &pl)) return r;
    if (pl->count == 0) return RT3_OK;
    ScopedTimer t(c, CAT_OTHER);
    if (c->lens.on)  // a lens frame's Light holds the sky already, antialiased (rt3_camera_set_lens)
        launch_postprocess_lens(c->stream, pl->dev.get(), pl->count, W, in->ptr, out->ptr);
    else
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
    const size_t S = c->work.cap;
    {
        ScopedTimer t(c, CAT_OTHER);
        launch_probe_raygen(c->stream, gconst_dev(g), W, px, py, (const float*)dp->ptr, dir->ptr, at->ptr, c->work.rays[0].get(), S, c->work.T[0].get());
    }
    if (int r = trace_primary(c, n)) return r;
    {
        ScopedTimer t(c, CAT_OTHER);
        launch_probe_store(c->stream, scene_dev(c), g->pad[0], g->blendfactor, px, py, c->work.hits.get(), c->work.T[0].get(), pv->ptr, at->ptr);
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
    if (c->denoise.variance_image) {
        mo = image_checked(c, c->denoise.variance_image, W, H, RT3_FORMAT_R32G32B32A32_SFLOAT, "variance input");
        if (!mo) return RT3_E_INVALID;
        if (mo->ptr == out->ptr) return fail(c, RT3_E_INVALID, "denoise: the variance input (rt3_denoise_set_variance_input) must not be 'Out'");
    }
    // rt3_denoise_set_guide_input: a lens frame's sample means guide the filter; gbuffer and gbuffer_depth are not read
    float4* guide[4] = {nullptr, nullptr, nullptr, nullptr};
    if (c->guide.in_on)
        if (int r = guide_resolve(c, c->guide.in, W, H, "denoise: guide input", &out, 1, "'Out'", guide)) return r;
    const rt3_denoise_params& p = c->denoise.params;
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
    if (c->denoise.scratch.capacity_bytes() < plan.bytes()) {  // the stream may still read the old allocation
        HIPC(c, hipStreamSynchronize(c->stream));
        HIPC(c, c->denoise.scratch.grow_bytes(plan.bytes()));
    }
    HIPC(c, plan.carve(c->denoise.scratch));
    for (int k = 0; k < 4; k++) L.guide[k] = guide[k];
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
    if (!c->temporal.has_prev) return fail(c, RT3_E_STATE, "temporal: no previous view (rt3_temporal_set_prev_view)");
    if (c->temporal.prev.window_size[0] != g->window_size[0] || c->temporal.prev.window_size[1] != g->window_size[1])
        return fail(c, RT3_E_INVALID, "temporal: the previous view's window_size differs from this frame's (after a resize, start over from zeroed history)");
    const rt3_temporal_params& p = c->temporal.params;
    TemporalLaunch L;
    L.g = gconst_dev(g);
    L.prev = gconst_dev(&c->temporal.prev);
    L.W = W; L.H = H; L.flags = p.flags;
    L.alpha = p.alpha; L.alpha_moments = p.alpha_moments; L.max_history = (float)p.max_history; L.normal_cos = p.normal_cos;
    L.plane_tolerance = p.plane_tolerance;
    L.gbuffer = r[0]->ptr; L.depth = (const float*)r[1]->ptr; L.in = r[2]->ptr;
    L.prev_gbuffer = r[3]->ptr; L.prev_depth = (const float*)r[4]->ptr; L.prev_history = r[5]->ptr; L.prev_moments = r[6]->ptr;
    L.out = r[7]->ptr; L.history = r[8]->ptr; L.moments = r[9]->ptr;
    if (c->temporal.motion_image) {
        const Resource* mv = image_checked(c, c->temporal.motion_image, W, H, RT3_FORMAT_R32G32B32A32_SFLOAT, "motion input");
        if (!mv) return RT3_E_INVALID;
        if (mv->ptr == r[7]->ptr || mv->ptr == r[8]->ptr || mv->ptr == r[9]->ptr)
            return fail(c, RT3_E_INVALID, "temporal: the motion input (rt3_temporal_set_motion_input) must not be 'Out', 'History' or 'Moments'");
        L.motion = mv->ptr;
    }
    // rt3_temporal_set_guide_input: a lens frame's sample means, this frame's and the previous one's, are the
    // surface records; gbuffer, gbuffer_depth, PrevGbuffer and PrevDepth are not read.  Before anything is enqueued
    if (c->guide.temporal_on) {
        if (c->temporal.motion_image)
            return fail(c, RT3_E_STATE, "temporal: a guide input (rt3_temporal_set_guide_input) and a motion input (rt3_temporal_set_motion_input) are both "
                                        "set: the \"motion\" image is made from pinhole primary hits and does not describe the camera samples; unset one (0 / NULL)");
        const Resource* const written[3] = {r[7], r[8], r[9]};
        float4* gi[8];
        if (int e = guide_resolve(c, c->guide.temporal_cur, W, H, "temporal: guide input, current", written, 3, "'Out', 'History' or 'Moments'", gi)) return e;
        if (int e = guide_resolve(c, c->guide.temporal_prev, W, H, "temporal: guide input, previous", written, 3, "'Out', 'History' or 'Moments'", gi + 4)) return e;
        for (int k = 1; k < 8; k++)
            for (int j = 0; j < k; j++)
                if (gi[j] == gi[k]) return fail(c, RT3_E_INVALID, "temporal: guide input: the eight images (current and previous) must be different images");
        for (int k = 0; k < 4; k++) {
            L.guide[k] = gi[k];
            L.prev_guide[k] = gi[4 + k];
        }
    }
    // rt3_temporal_set_guide_motion_input: the samples' mean previous position is the point looked up
    if (c->guide.temporal_motion) {
        if (!c->guide.temporal_on)
            return fail(c, RT3_E_STATE, "temporal: a guide motion input is set (rt3_temporal_set_guide_motion_input) and no guide input "
                                        "(rt3_temporal_set_guide_input): the image describes a lens frame's samples; unset it (0), or give the guide sets");
        const Resource* gm = image_checked(c, c->guide.temporal_motion, W, H, RT3_FORMAT_R32G32B32A32_SFLOAT, "temporal: guide motion input");
        if (!gm) return RT3_E_INVALID;
        if (gm->ptr == r[7]->ptr || gm->ptr == r[8]->ptr || gm->ptr == r[9]->ptr)
            return fail(c, RT3_E_INVALID, "temporal: the guide motion input must not be 'Out', 'History' or 'Moments'");
        for (int k = 0; k < 4; k++)
            if (gm->ptr == L.guide[k] || gm->ptr == L.prev_guide[k])
                return fail(c, RT3_E_INVALID, "temporal: the guide motion input must not be one of the eight guide images");
        L.guide_motion = static_cast<const float4*>(gm->ptr);
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
    MotionLaunch L;
    if (int r = motion_launch_tables(c, &L.m, &L.prev_pos)) return r;
    L.g = gconst_dev(g);
    PixelList* pl;
    if (int r = primary_hits(c, L.g, W, H, &pl)) return r;
    if (pl->count == 0) return RT3_OK;
    L.pixels = pl->dev.get(); L.npix = pl->count; L.width = W; L.hits = c->work.hits.get(); L.out = res[0]->ptr;
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
    {"adaptive", kWindow, true, false, pass_adaptive,
     {{"gbuffer", kU4}, {"gbuffer_depth", kF1}, {"Light", kF4}, {"PrevLight", kF4}, {"Moments", kF4, false, 0xCu}}},
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
    if (p.one_rank && c->tiles.n_ranks > 1)
        return fail(c, RT3_E_STATE, name + ": a tap may need pixels that other ranks own; run it on the gathered image with the tile partition "
                                           "switched off (rt3_set_tile_partition(w, h, 0, 1))");
    return p.run(c, g, W, H, res);
}

}  // namespace

namespace rt3 {

// Self-test op 46 (include/rt3.h has the layout).  Every plane is one record longer than n and carries a pattern where the kernels have
// nothing to write.
int selftest_fog_queue(rt3_ctx* c, const uint32_t* in, uint32_t n, uint32_t* out) {
    const uint32_t kind = in[0], groups = in[1], flags = in[2], frame = in[3], B = in[4], seg = in[5], s0 = in[6], npix = in[7], miss_lacc = in[8];
    if (kind > 2 || groups == 0 || groups > 65535 || B == 0 || B > 64 || seg >= B || npix == 0 || npix > (1u << 24) || n > (1u << 24) || miss_lacc > 1)
        return fail(c, RT3_E_INVALID, "selftest: fog queue header: kind 0..2, 1..65535 workgroups, bounces 1..64, segment < bounces, 1..2^24 pixels, at most 2^24 records");
    if (((uint64_t)s0 + (n ? n : 1u)) * B * kFogRngDims > (uint64_t)(kLensRngBase - kFogRngBase)) return fail(c, RT3_E_INVALID, "selftest: fog queue: s0 too large");
    if (!c->medium.on) return fail(c, RT3_E_STATE, "selftest: no medium is on (rt3_scene_set_medium)");
    if (int r = check_accel_current(c)) return r;
    HIPC(c, hipSetDevice(c->device));
    constexpr uint32_t kGuard = 0xA5A5A5A5u;
    const size_t S = (size_t)n + 1;
    const uint32_t* rec = in + kSelftestFogQueueHeader + npix;
    DevBuf<uint32_t> d_cnt;
    HIPC(c, d_cnt.alloc_bytes(16));
    const uint32_t cnt0[4] = {n, 0u, 0u, 0u};
    HIPC(c, hipMemcpy(d_cnt.get(), cnt0, 16, hipMemcpyHostToDevice));
    if (kind != 0) {  // k_fog_shadow
        std::vector<uint32_t> rays(8 * S, kGuard), contrib(2 * S, kGuard), tmax(S, kGuard);
        for (size_t i = 0; i < n; i++) {
            const uint32_t* r = rec + kSelftestFogShadowRecord * i;
            memcpy(&rays[4 * i], r, 16);
            memcpy(&rays[4 * (S + i)], r + 4, 16);
            contrib[2 * i] = r[8];
            contrib[2 * i + 1] = r[9];
            tmax[i] = r[10];
        }
        DevBuf<float> d_rays, d_contrib, d_tmax;
        HIPC(c, d_rays.alloc_bytes(8 * S * 4));
        HIPC(c, d_contrib.alloc_bytes(2 * S * 4));
        HIPC(c, d_tmax.alloc_bytes(S * 4));
        HIPC(c, hipMemcpy(d_rays.get(), rays.data(), 8 * S * 4, hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(d_contrib.get(), contrib.data(), 2 * S * 4, hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(d_tmax.get(), tmax.data(), S * 4, hipMemcpyHostToDevice));
        FogShadowLaunch F{};
        F.fog = fog_dev(c); F.rays = d_rays.get(); F.contrib = d_contrib.get(); F.tmax = kind == 2 ? d_tmax.get() : nullptr; F.count = d_cnt.get(); F.stride = S;
        launch_fog_shadow(c->stream, F, n, groups);
        HIPC(c, hipGetLastError());
        HIPC(c, hipStreamSynchronize(c->stream));
        std::vector<uint32_t> rays2(8 * S), contrib2(2 * S), tmax2(S);
        HIPC(c, hipMemcpy(rays2.data(), d_rays.get(), 8 * S * 4, hipMemcpyDeviceToHost));
        HIPC(c, hipMemcpy(contrib2.data(), d_contrib.get(), 2 * S * 4, hipMemcpyDeviceToHost));
        HIPC(c, hipMemcpy(tmax2.data(), d_tmax.get(), S * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < S; i++) {
            const bool guard = i == n;
            for (int k = 0; k < 4; k++)
                if ((guard || k < 3) && (rays2[4 * i + k] != rays[4 * i + k] || rays2[4 * (S + i) + k] != rays[4 * (S + i) + k]))
                    return fail(c, RT3_E_STATE, "selftest: k_fog_shadow changed an origin, a direction or a word behind the queue's end");
            if (contrib2[2 * i + 1] != contrib[2 * i + 1] || (guard && contrib2[2 * i] != kGuard) || tmax2[i] != tmax[i])
                return fail(c, RT3_E_STATE, "selftest: k_fog_shadow changed a path id, a range end or a word behind the queue's end");
        }
        for (size_t i = 0; i < n; i++) {
            out[3 * i] = rays2[4 * i + 3];
            out[3 * i + 1] = rays2[4 * (S + i) + 3];
            out[3 * i + 2] = contrib2[2 * i];
        }
        return RT3_OK;
    }
    {  // every path id once, below max(n, 1): the radiance slots and the queues have n slots
        std::vector<uint8_t> seen(n ? n : 1, 0);
        for (size_t i = 0; i < n; i++) {
            const uint32_t pid = rec[kSelftestFogSegmentRecord * i + 11];
            if (pid >= n || seen[pid]) return fail(c, RT3_E_INVALID, "selftest: fog queue record " + std::to_string(i) + ": path ids are 0 .. n-1, each once");
            seen[pid] = 1;
        }
    }
    rt3_gconst g;
    memset(&g, 0, sizeof(g));
    g.bounces = B;
    g.samples = 1;
    g.frame = frame;
    g.pad[0] = flags;
    // (path_setup as a frame calls it, so that the light table, the sky and the emitter side array are the frame's.  No ensure_work runs
    // ahead of it here: as a side effect it sizes the context's own in-scatter queues for whatever work.cap is, possibly one element; the
    // next frame's path_setup grows them again.  This op launches over queues of its own, below.)
    PathSetup ps;
    if (int r = path_setup(c, &g, &ps)) return r;
    std::vector<uint32_t> rays(8 * S, kGuard), hits(4 * S, kGuard), T(3 * S, kGuard), lacc(4 * S, kGuard);
    const float one = 1.0f;
    uint32_t one_bits;
    memcpy(&one_bits, &one, 4);
    for (size_t i = 0; i < n; i++) {
        const uint32_t* r = rec + kSelftestFogSegmentRecord * i;
        memcpy(&rays[4 * i], r, 12);
        rays[4 * i + 3] = one_bits;  // the pdf slot
        memcpy(&rays[4 * (S + i)], r + 3, 12);
        rays[4 * (S + i) + 3] = r[11];
        hits[4 * i] = r[6];
        hits[4 * i + 1] = hits[4 * i + 2] = 0u;
        hits[4 * i + 3] = r[7];
        for (int k = 0; k < 3; k++) T[k * S + i] = r[8 + k];
        lacc[4 * i] = lacc[4 * i + 1] = lacc[4 * i + 2] = one_bits;
        lacc[4 * i + 3] = 0u;
    }
    DevBuf<float> d_rays, d_hits, d_T, d_lacc, q_rays[2], q_contrib[2], q_tmax[2];
    DevBuf<uint32_t> d_pix;
    DevBuf<unsigned long long> d_info;
    HIPC(c, d_rays.alloc_bytes(8 * S * 4));
    HIPC(c, d_hits.alloc_bytes(4 * S * 4));
    HIPC(c, d_T.alloc_bytes(3 * S * 4));
    HIPC(c, d_lacc.alloc_bytes(4 * S * 4));
    HIPC(c, d_pix.alloc_bytes((size_t)npix * 4));
    HIPC(c, d_info.alloc_bytes(16));
    HIPC(c, hipMemset(d_info.get(), 0, 16));
    HIPC(c, hipMemcpy(d_rays.get(), rays.data(), 8 * S * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(d_hits.get(), hits.data(), 4 * S * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(d_T.get(), T.data(), 3 * S * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(d_lacc.get(), lacc.data(), 4 * S * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(d_pix.get(), in + kSelftestFogQueueHeader, (size_t)npix * 4, hipMemcpyHostToDevice));
    for (int k = 0; k < 2; k++) {
        HIPC(c, q_rays[k].alloc_bytes(8 * S * 4));
        HIPC(c, q_contrib[k].alloc_bytes(2 * S * 4));
        HIPC(c, q_tmax[k].alloc_bytes(S * 4));
        HIPC(c, hipMemset(q_rays[k].get(), 0xA5, 8 * S * 4));
        HIPC(c, hipMemset(q_contrib[k].get(), 0xA5, 2 * S * 4));
        HIPC(c, hipMemset(q_tmax[k].get(), 0xA5, S * 4));
    }
    FogSegmentLaunch F{};
    F.fog = ps.fogdev; F.sc = ps.sc; F.lights = ps.lights; F.emit_tex = ps.emit_tex;
    F.rays = d_rays.get(); F.hits = d_hits.get(); F.T = d_T.get(); F.count = d_cnt.get(); F.stride = S;
    F.lacc_miss = miss_lacc ? d_lacc.get() : nullptr;
    F.scatter = ps.fog_scatter ? 1u : 0u; F.sky = ps.fog_scatter && ps.nee ? 1u : 0u;
    if (!ps.fog_scatter) F.lights.n = 0u;
    for (int k = 0; k < 2; k++) {
        F.q_rays[k] = q_rays[k].get(); F.q_contrib[k] = q_contrib[k].get(); F.q_tmax[k] = q_tmax[k].get();
        F.q_count[k] = d_cnt.get() + 1 + k;
    }
    F.q_stride = S;
    F.pixels = d_pix.get(); F.npix = npix; F.s0 = s0; F.bounces = B; F.segment = seg; F.frame = frame;
    F.info = d_info.get();
    launch_fog_segment(c->stream, F, n, groups);
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->stream));
    std::vector<uint32_t> rays2(8 * S), hits2(4 * S);
    uint32_t cnt[4];
    unsigned long long info[2];
    HIPC(c, hipMemcpy(rays2.data(), d_rays.get(), 8 * S * 4, hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(hits2.data(), d_hits.get(), 4 * S * 4, hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(T.data(), d_T.get(), 3 * S * 4, hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(lacc.data(), d_lacc.get(), 4 * S * 4, hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(cnt, d_cnt.get(), 16, hipMemcpyDeviceToHost));
    HIPC(c, hipMemcpy(info, d_info.get(), 16, hipMemcpyDeviceToHost));
    if (rays2 != rays || hits2 != hits) return fail(c, RT3_E_STATE, "selftest: k_fog_segment wrote a ray or hit record");
    for (int k = 0; k < 3; k++)
        if (T[k * S + n] != kGuard) return fail(c, RT3_E_STATE, "selftest: k_fog_segment wrote behind the queue's end");
    for (int k = 0; k < 4; k++)
        if (lacc[4 * (size_t)n + k] != kGuard) return fail(c, RT3_E_STATE, "selftest: k_fog_segment wrote behind the radiance slots' end");
    if (cnt[0] != n || cnt[1] > n || cnt[2] > n) return fail(c, RT3_E_STATE, "selftest: k_fog_segment left an impossible queue length");
    out[0] = cnt[1];
    out[1] = cnt[2];
    out[2] = (uint32_t)info[0];
    out[3] = (uint32_t)info[1];
    uint32_t* o = out + 4;
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) o[3 * i + k] = T[k * S + i];
    o += 3 * (size_t)n;
    memcpy(o, lacc.data(), 16 * (size_t)n);
    o += 4 * (size_t)n;
    for (int k = 0; k < 2; k++) {
        std::vector<uint32_t> qr(8 * S), qc(2 * S), qt(S);
        HIPC(c, hipMemcpy(qr.data(), q_rays[k].get(), 8 * S * 4, hipMemcpyDeviceToHost));
        HIPC(c, hipMemcpy(qc.data(), q_contrib[k].get(), 2 * S * 4, hipMemcpyDeviceToHost));
        HIPC(c, hipMemcpy(qt.data(), q_tmax[k].get(), S * 4, hipMemcpyDeviceToHost));
        for (size_t i = cnt[1 + k]; i < S; i++) {  // behind the length nothing is written
            bool clean = qc[2 * i] == kGuard && qc[2 * i + 1] == kGuard && qt[i] == kGuard;
            for (int w = 0; w < 4; w++) clean = clean && qr[4 * i + w] == kGuard && qr[4 * (S + i) + w] == kGuard;
            if (!clean) return fail(c, RT3_E_STATE, "selftest: k_fog_segment wrote behind an in-scatter queue's length");
        }
        for (size_t i = 0; i < n; i++) {
            uint32_t* r = o + kSelftestFogRayOut * i;
            memcpy(r, &qr[4 * i], 16);
            memcpy(r + 4, &qr[4 * (S + i)], 16);
            r[8] = qc[2 * i];
            r[9] = qc[2 * i + 1];
            r[10] = qt[i];
            r[11] = 0u;
        }
        o += kSelftestFogRayOut * (size_t)n;
    }
    return RT3_OK;
}

}  // namespace rt3

extern "C" {

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
    if (c->scene.max_tex_index >= (int64_t)c->scene.h_tex.size())
        return fail(c, RT3_E_STATE, "a geometry references base-colour texture " + std::to_string(c->scene.max_tex_index) + " but only " +
                                        std::to_string(c->scene.h_tex.size()) + " texture(s) were set (rt3_scene_set_texture)");
    rt3_gconst g;
    memcpy(&g, constants, sizeof(g));
    for (const PassDesc& p : kPasses)
        if (!strcmp(pass_name, p.name)) return launch_pass(c, p, &g, x, y, z, bindings, n_bindings);
    return fail(c, RT3_E_INVALID, std::string("unknown pass '") + pass_name + "' (known: " + names_of(kPasses) + ")");
}
int rt3_denoise_set_params(rt3_ctx* c, const rt3_denoise_params* p) {
    if (!c) return RT3_E_INVALID;
    if (!p) {
        c->denoise.params = kDenoiseDefaults;
        return RT3_OK;
    }
    if (p->iterations > 8) return fail(c, RT3_E_INVALID, "denoise params: iterations must be 0..8 (step 2^i: 8 iterations reach 512 pixels)");
    if (p->normal_squarings > 16) return fail(c, RT3_E_INVALID, "denoise params: normal_squarings must be 0..16 (the exponent is 2^k)");
    if (!(std::isfinite(p->sigma_z) && p->sigma_z > 0.0f) || !(std::isfinite(p->sigma_l) && p->sigma_l > 0.0f))
        return fail(c, RT3_E_INVALID, "denoise params: sigma_z and sigma_l must be finite and positive");
    if (p->flags & ~RT3_DENOISE_NO_DEMODULATION) return fail(c, RT3_E_INVALID, "denoise params: unknown flag bits");
    c->denoise.params = *p;
    return RT3_OK;
}
int rt3_denoise_set_variance_input(rt3_ctx* c, uint32_t moments_image) {
    if (!c) return RT3_E_INVALID;
    c->denoise.variance_image = moments_image;  // checked when "denoise" is launched: the image may be created, resized or destroyed in between
    return RT3_OK;
}
int rt3_adaptive_set_params(rt3_ctx* c, const rt3_adaptive_params* p) {
    if (!c) return RT3_E_INVALID;
    if (!p) {
        c->adaptive.params = kAdaptiveDefaults;
        return RT3_OK;
    }
    if (p->min_samples < 2) return fail(c, RT3_E_INVALID, "adaptive params: min_samples must be at least 2 (the variance divides by n - 1)");
    if (p->step < 1) return fail(c, RT3_E_INVALID, "adaptive params: step must be at least 1");
    if (!(std::isfinite(p->threshold) && p->threshold >= 0.0f)) return fail(c, RT3_E_INVALID, "adaptive params: threshold must be finite and not negative");
    if (!(std::isfinite(p->dark) && p->dark > 0.0f)) return fail(c, RT3_E_INVALID, "adaptive params: dark must be finite and positive");
    if (p->dilate > 1) return fail(c, RT3_E_INVALID, "adaptive params: dilate must be 0 or 1");
    if (p->flags) return fail(c, RT3_E_INVALID, "adaptive params: unknown flag bits");
    c->adaptive.params = *p;
    return RT3_OK;
}
// coverage mode: the context's, read by the next "adaptive" launch; scene changes leave it
int rt3_adaptive_set_coverage(rt3_ctx* c, int on) {
    if (!c) return RT3_E_INVALID;
    if (on != 0 && on != 1) return fail(c, RT3_E_INVALID, "adaptive coverage: the mode is 0 or 1");
    c->adaptive.coverage = on != 0;
    return RT3_OK;
}
int rt3_adaptive_get_coverage(rt3_ctx* c, int* on) {
    if (!c || !on) return fail(c, RT3_E_INVALID, "adaptive coverage: NULL");
    *on = c->adaptive.coverage ? 1 : 0;
    return RT3_OK;
}
int rt3_adaptive_info(rt3_ctx* c, uint32_t* rounds, uint64_t* paths_traced, uint32_t* pixels_capped) {
    if (!c) return RT3_E_INVALID;
    if (rounds) *rounds = c->adaptive.rounds;
    if (paths_traced) *paths_traced = c->adaptive.paths_traced;
    if (pixels_capped) *pixels_capped = c->adaptive.pixels_capped;
    return RT3_OK;
}
int rt3_camera_set_lens(rt3_ctx* c, const rt3_lens_params* p) {
    if (!c) return RT3_E_INVALID;
    if (!p) {
        c->lens.on = false;
        return RT3_OK;
    }
    if (!std::isfinite(p->aperture_radius) || !std::isfinite(p->focus_distance) || !std::isfinite(p->pixel_jitter))
        return fail(c, RT3_E_INVALID, "lens params: every value must be finite");
    if (!(p->aperture_radius >= 0.0f)) return fail(c, RT3_E_INVALID, "lens params: aperture_radius must not be negative");
    if (!(p->pixel_jitter >= 0.0f && p->pixel_jitter <= 1.0f)) return fail(c, RT3_E_INVALID, "lens params: pixel_jitter must lie in [0, 1]");
    if (p->aperture_radius > 0.0f && !(p->focus_distance > 0.0f))
        return fail(c, RT3_E_INVALID, "lens params: focus_distance must be positive when aperture_radius is");
    if (p->reserved != 0u) return fail(c, RT3_E_INVALID, "lens params: reserved must be 0");
    c->lens.params = *p;
    c->lens.on = true;
    return RT3_OK;
}
// guide images.  The output is checked here (live RGBA32F images, all different) and again at every launch (size,
// not Light / PrevLight); the input at every "denoise" launch, like the variance input
int rt3_camera_set_guide_output(rt3_ctx* c, const rt3_guide_images* gi) {
    if (!c) return RT3_E_INVALID;
    if (!gi) {
        c->guide.out_on = false;
        return RT3_OK;
    }
    const uint32_t h[4] = {gi->position, gi->normal, gi->albedo, gi->emission};
    for (int k = 0; k < 4; k++) {
        const Resource* r = get_res(c, h[k], RT3_TAG_IMAGE);
        if (!r || r->format != RT3_FORMAT_R32G32B32A32_SFLOAT) return fail(c, RT3_E_INVALID, "guide output: every handle must be a live RGBA32F image");
        for (int j = 0; j < k; j++)
            if (h[j] == h[k]) return fail(c, RT3_E_INVALID, "guide output: the four images must be different images");
    }
    c->guide.out = *gi;
    c->guide.out_on = true;
    return RT3_OK;
}
int rt3_camera_get_guide_output(rt3_ctx* c, rt3_guide_images* out, int* enabled) {
    if (!c) return RT3_E_INVALID;
    if (out) *out = c->guide.out;
    if (enabled) *enabled = c->guide.out_on ? 1 : 0;
    return RT3_OK;
}
int rt3_denoise_set_guide_input(rt3_ctx* c, const rt3_guide_images* gi) {
    if (!c) return RT3_E_INVALID;
    c->guide.in_on = gi != nullptr;
    if (gi) c->guide.in = *gi;  // checked when "denoise" is launched, like the variance input
    return RT3_OK;
}
// both NULL: the G-buffer, the default; one NULL: refused, nothing changed.  The images are checked when "temporal" is launched
int rt3_temporal_set_guide_input(rt3_ctx* c, const rt3_guide_images* current, const rt3_guide_images* previous) {
    if (!c) return RT3_E_INVALID;
    if ((current == nullptr) != (previous == nullptr))
        return fail(c, RT3_E_INVALID, "temporal guide input: give the current and the previous guide images, or NULL for both (the G-buffer)");
    c->guide.temporal_on = current != nullptr;
    if (current) {
        c->guide.temporal_cur = *current;
        c->guide.temporal_prev = *previous;
    }
    return RT3_OK;
}
// the fifth guide image.  The output is checked here (a live RGBA32F image) and again at every "refrence_mode" launch
// (size, not one of the images written there); the input at every "temporal" launch
int rt3_camera_set_guide_motion_output(rt3_ctx* c, uint32_t image) {
    if (!c) return RT3_E_INVALID;
    if (image != 0) {
        const Resource* r = get_res(c, image, RT3_TAG_IMAGE);
        if (!r || r->format != RT3_FORMAT_R32G32B32A32_SFLOAT) return fail(c, RT3_E_INVALID, "guide motion output: the handle must be a live RGBA32F image");
    }
    c->guide.motion_out = image;
    return RT3_OK;
}
int rt3_camera_get_guide_motion_output(rt3_ctx* c, uint32_t* image) {
    if (!c || !image) return fail(c, RT3_E_INVALID, "guide motion output: NULL");
    *image = c->guide.motion_out;
    return RT3_OK;
}
int rt3_temporal_set_guide_motion_input(rt3_ctx* c, uint32_t image) {
    if (!c) return RT3_E_INVALID;
    c->guide.temporal_motion = image;  // checked when "temporal" is launched, like the motion input
    return RT3_OK;
}
int rt3_path_set_roulette(rt3_ctx* c, const rt3_roulette_params* p) {
    if (!c) return RT3_E_INVALID;
    if (!p) {
        c->roulette.on = false;
        return RT3_OK;
    }
    if (!std::isfinite(p->min_survival)) return fail(c, RT3_E_INVALID, "roulette params: min_survival must be finite");
    if (!(p->min_survival >= 0.0078125f && p->min_survival <= 1.0f)) return fail(c, RT3_E_INVALID, "roulette params: min_survival must lie in [2^-7, 1]");
    if (p->reserved[0] != 0u || p->reserved[1] != 0u) return fail(c, RT3_E_INVALID, "roulette params: reserved must be 0");
    c->roulette.params = *p;
    c->roulette.on = true;
    return RT3_OK;
}
int rt3_path_get_roulette(rt3_ctx* c, rt3_roulette_params* out, int* enabled) {
    if (!c) return RT3_E_INVALID;
    if (out) *out = c->roulette.params;
    if (enabled) *enabled = c->roulette.on ? 1 : 0;
    return RT3_OK;
}
int rt3_medium_info(rt3_ctx* c, uint64_t* segments, uint64_t* inscatter_rays) {
    if (!c) return RT3_E_INVALID;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    unsigned long long h[2] = {0ull, 0ull};
    if (c->medium.d_info) HIPC(c, hipMemcpy(h, c->medium.d_info.get(), 16, hipMemcpyDeviceToHost));
    if (segments) *segments = h[0];
    if (inscatter_rays) *inscatter_rays = h[1];
    return RT3_OK;
}
int rt3_path_roulette_info(rt3_ctx* c, uint64_t* tested, uint64_t* ended) {
    if (!c) return RT3_E_INVALID;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (int r = harvest(c)) return r;
    if (tested) *tested = c->work.roulette_tested;
    if (ended) *ended = c->work.roulette_ended;
    return RT3_OK;
}
int rt3_camera_get_lens(rt3_ctx* c, rt3_lens_params* out, int* enabled) {
    if (!c) return RT3_E_INVALID;
    if (out) *out = c->lens.params;
    if (enabled) *enabled = c->lens.on ? 1 : 0;
    return RT3_OK;
}
int rt3_temporal_set_prev_view(rt3_ctx* c, const void* prev_gconst, size_t size) {
    if (!c) return RT3_E_INVALID;
    if (!prev_gconst && size == 0) {
        c->temporal.has_prev = false;
        return RT3_OK;
    }
    if (!prev_gconst || size != sizeof(rt3_gconst)) return fail(c, RT3_E_INVALID, "temporal prev view: must be the 304-byte GConst block of the previous frame, or (NULL, 0)");
    memcpy(&c->temporal.prev, prev_gconst, sizeof(rt3_gconst));
    c->temporal.has_prev = true;
    return RT3_OK;
}
int rt3_temporal_set_motion_input(rt3_ctx* c, uint32_t motion_image) {
    if (!c) return RT3_E_INVALID;
    c->temporal.motion_image = motion_image;  // checked when "temporal" is launched, like the variance input of "denoise"
    return RT3_OK;
}
int rt3_temporal_set_params(rt3_ctx* c, const rt3_temporal_params* p) {
    if (!c) return RT3_E_INVALID;
    if (!p) {
        c->temporal.params = kTemporalDefaults;
        return RT3_OK;
    }
    if (!(p->alpha >= 0.0f && p->alpha <= 1.0f) || !(p->alpha_moments >= 0.0f && p->alpha_moments <= 1.0f))
        return fail(c, RT3_E_INVALID, "temporal params: alpha and alpha_moments must lie in [0, 1]");
    if (p->max_history < 1 || p->max_history > 65535) return fail(c, RT3_E_INVALID, "temporal params: max_history must be 1..65535");
    if (!(p->normal_cos >= -1.0f && p->normal_cos <= 1.0f)) return fail(c, RT3_E_INVALID, "temporal params: normal_cos must lie in [-1, 1]");
    if (!(std::isfinite(p->plane_tolerance) && p->plane_tolerance > 0.0f)) return fail(c, RT3_E_INVALID, "temporal params: plane_tolerance must be finite and positive");
    if (p->flags & ~RT3_TEMPORAL_NO_DEMODULATION) return fail(c, RT3_E_INVALID, "temporal params: unknown flag bits");
    c->temporal.params = *p;
    return RT3_OK;
}

}  // extern "C"
