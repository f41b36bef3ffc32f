// rt3_accel.hip -- host layer, the acceleration structure: the placements and their flattening, shading records, alpha tables, the
// two-level build with its conservative-box arithmetic, build / refit / import / info / levels / download, and the emitter table driver
// (include/rt3.h: rt3_accel_*, rt3_light_*).  Owns rt3_ctx::accel.  The kernels are rt3_lbvh.hip, rt3_sah_top.hip, rt3_tlas.hip,
// rt3_refit.hip and rt3_lights.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "rt3_ctx.hpp"

using namespace rt3;

namespace rt3 {

void invalidate_accel(rt3_ctx* c) { c->accel.built = false; }
void mark_accel_stale(rt3_ctx* c) {
    if (c->accel.built) c->accel.stale = true;
}
int check_accel_current(rt3_ctx* c, const char* unbuilt) {
    if (!c || !c->accel.built) return fail(c, RT3_E_STATE, unbuilt);
    if (c->accel.stale) return fail(c, RT3_E_STATE, "vertices were updated since the acceleration structure was built: rt3_accel_refit or rt3_accel_build first");
    return RT3_OK;
}
std::pair<const rt3_instance*, size_t> placements(const rt3_ctx* c, rt3_instance& whole) {
    if (!c->scene.h_instances.empty()) return {c->scene.h_instances.data(), c->scene.h_instances.size()};
    whole.geometry_first = 0;
    whole.geometry_count = c->scene.n_geoms;
    memcpy(whole.transform, kIdentity, sizeof(kIdentity));
    return {&whole, 1};
}
SceneDev scene_dev(const rt3_ctx* c) {
    SceneDev s;
    s.verts = c->scene.d_verts.get();
    s.indices = c->scene.d_indices.get();
    s.geoms = c->accel.d_geoms.get();
    s.shade_geoms = c->accel.d_shade_geoms.get();
    s.n_geoms = c->accel.n_flat_geoms;
    s.prim_geom = c->accel.d_prim_geom.get();
    s.first_prim = c->accel.d_first_prim.get();
    s.tri_shade = c->accel.shade.rec.get();
    s.tri_uv = c->accel.shade.uv.get();
    s.guide_marg = c->scene.d_guide_marg.get();
    s.sky = c->scene.d_sky.get();
    s.sky_alias = c->scene.d_sky_alias.get();
    s.cdf_marg = c->scene.d_cdf_marg.get();
    s.sky_w = c->scene.sky_w;
    s.sky_h = c->scene.sky_h;
    s.sky_wt = c->scene.sky_wt;
    s.bluenoise = c->scene.d_bn.get();
    s.bn_w = c->scene.bn_w;
    s.bn_h = c->scene.bn_h;
    s.tex_pixels = c->scene.d_tex_pixels.get();
    s.tex_table = c->scene.d_tex_table.get();
    s.srgb_lut = c->scene.d_srgb_lut.get();
    s.n_tex = c->scene.d_tex_pixels ? (uint32_t)c->scene.h_tex.size() : 0u;
    s.mat_tex = c->accel.has_mat_tex ? c->accel.d_mat_tex.get() : nullptr;
    s.tri_tan = c->accel.has_mat_tex && c->accel.shade.has_tan ? c->accel.shade.tan.get() : nullptr;
    return s;
}

GeomTables world_tables(const rt3_ctx* c) { return {c->scene.d_verts.get(), c->scene.d_indices.get(), c->accel.d_geoms.get(), c->accel.d_prim_geom.get(), c->accel.d_first_prim.get()}; }
AlphaDev alpha_dev(const rt3_ctx* c) {
    AlphaDev a = {};
    if (!c->accel.masked) return a;
    a.table = c->accel.d_alpha.get();
    a.tri_uv = c->accel.shade.uv.get();
    a.tex_table = c->scene.d_tex_table.get();
    a.tex_pixels = c->scene.d_tex_pixels.get();
    a.n_tex = c->scene.d_tex_pixels ? (uint32_t)c->scene.h_tex.size() : 0u;
    return a;
}

PaneDev pane_dev(const rt3_ctx* c) { return PaneDev{scene_dev(c), c->accel.d_glass.get(), c->accel.pane_first_slot}; }

}  // namespace rt3

// the geometry tables of a bottom tree: the world's vertices and indices, read through the tree's own tables
static GeomTables mesh_tables(const rt3_ctx* c, const MeshTables& t) { return {c->scene.d_verts.get(), c->scene.d_indices.get(), t.geoms, t.prim_geom, t.first_prim}; }
// One (instance, geometry) pair per entry, instance-major.  A few KiB of tables go up; primitive -> entry is filled in on the device
// (k_prim_geom), so a rebuild after a moved instance copies nothing big.
static int flatten_world(rt3_ctx* c) {
    rt3_instance whole;
    const auto [inst, n_inst] = placements(c, whole);
    std::vector<FlatGeomDev> flat;
    std::vector<ShadeGeomDev> shade;
    std::vector<MatTexDev> mats;
    std::vector<GlassDev> glass;
    std::vector<AbsorbDev> absorb;
    uint32_t n_absorbing = 0, n_frosted = 0;
    std::vector<uint32_t> first;
    std::vector<Placed> placed;
    uint64_t total = 0;
    for (size_t i = 0; i < n_inst; i++) {
        if ((uint64_t)inst[i].geometry_first + inst[i].geometry_count > c->scene.n_geoms)
            return fail(c, RT3_E_INVALID, "instance " + std::to_string(i) + ": geometry range exceeds the geometries set (rt3_scene_set_geometry)");
        const float* m = inst[i].transform;
        const bool identity = memcmp(m, kIdentity, sizeof(kIdentity)) == 0;
        for (uint32_t k = 0; k < inst[i].geometry_count; k++) {
            const uint32_t g = inst[i].geometry_first + k;
            FlatGeomDev f;
            memset(&f, 0, sizeof(f));
            static_assert(sizeof(rt3_geometry_info) == sizeof(GeometryInfoDev), "geometry info layouts");
            memcpy(&f.g, &c->scene.h_geoms[g], sizeof(f.g));
            pack3x4(m, f.m);
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
            if (any_mat_tex(c)) {
                static_assert(sizeof(rt3_material_textures) == sizeof(MatTexDev), "material texture layouts");
                MatTexDev mt;
                memcpy(&mt, &c->scene.h_mat_tex[g], sizeof(mt));
                mats.push_back(mt);
            }
            if (any_glass(c)) {
                static_assert(sizeof(rt3_transmission) == sizeof(GlassDev), "transmission layouts");
                GlassDev gd;
                memcpy(&gd, &c->scene.h_transmission[g], sizeof(gd));
                if (pane_geometry(c, g)) gd.pad = kGlassPaneBit;  // (the reserved word is 0 as uploaded)
                if (frosted_geometry(c, g)) {  // (never a pane)
                    gd.pad = kGlassFrostBit;
                    if (c->scene.h_prim_counts[g] > 0) n_frosted++;
                }
                glass.push_back(gd);
            }
            {  // absorption: a geometry that does not absorb holds zeros, whatever was uploaded for it
                AbsorbDev ad = {{0.0f, 0.0f, 0.0f}, 0u};
                if (absorbing_geometry(c, g)) {
                    for (int q = 0; q < 3; q++) ad.sigma[q] = c->scene.h_attenuation[g].sigma[q];
                    ad.absorbing = 1u;
                    n_absorbing++;
                }
                absorb.push_back(ad);
            }
            first.push_back((uint32_t)total);
            placed.push_back({(uint32_t)i, g, (uint32_t)total, c->scene.h_prim_counts[g], identity});
            total += c->scene.h_prim_counts[g];
            if (total > (1ull << 28)) return fail(c, RT3_E_UNSUPPORTED, "more than 2^28 triangles after instancing (leaf references hold 28 bits)");
        }
    }
    const size_t nf = flat.size();
    if (int r = dev_alloc(c, c->accel.d_geoms, nf)) return r;
    if (int r = dev_alloc(c, c->accel.d_shade_geoms, nf)) return r;
    if (int r = dev_alloc(c, c->accel.d_first_prim, nf)) return r;
    if (int r = dev_alloc(c, c->accel.d_prim_geom, (size_t)total)) return r;
    if (nf) {
        HIPC(c, hipMemcpy(c->accel.d_geoms.get(), flat.data(), nf * sizeof(FlatGeomDev), hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(c->accel.d_shade_geoms.get(), shade.data(), nf * sizeof(ShadeGeomDev), hipMemcpyHostToDevice));
        HIPC(c, hipMemcpy(c->accel.d_first_prim.get(), first.data(), nf * 4, hipMemcpyHostToDevice));
        if (nf * sizeof(FlatGeomDev) > (64u << 10)) c->accel.bulk_copies += 3;
        launch_prim_geom(c->stream, c->accel.d_first_prim.get(), (uint32_t)nf, (uint32_t)total, c->accel.d_prim_geom.get());
        HIPC(c, hipGetLastError());
    }
    c->accel.has_mat_tex = c->accel.has_normal_tex = false;
    if (!mats.empty()) {
        if (int r = dev_alloc(c, c->accel.d_mat_tex, nf)) return r;
        HIPC(c, hipMemcpy(c->accel.d_mat_tex.get(), mats.data(), nf * sizeof(MatTexDev), hipMemcpyHostToDevice));
        c->accel.has_mat_tex = true;
        for (const MatTexDev& mt : mats) c->accel.has_normal_tex = c->accel.has_normal_tex || mt.normal_tex >= 0;
    }
    c->accel.has_glass = false;
    if (!glass.empty()) {
        if (int r = dev_alloc(c, c->accel.d_glass, nf)) return r;
        HIPC(c, hipMemcpy(c->accel.d_glass.get(), glass.data(), nf * sizeof(GlassDev), hipMemcpyHostToDevice));
        c->accel.has_glass = true;
    }
    c->accel.n_frosted = n_frosted;
    c->accel.n_absorbing = 0;
    if (n_absorbing) {  // (kept only when some flattened geometry absorbs)
        if (int r = dev_alloc(c, c->accel.d_absorb, nf)) return r;
        HIPC(c, hipMemcpy(c->accel.d_absorb.get(), absorb.data(), nf * sizeof(AbsorbDev), hipMemcpyHostToDevice));
        c->accel.n_absorbing = n_absorbing;
    } else {
        c->accel.d_absorb.reset();
    }
    c->accel.n_flat_geoms = (uint32_t)nf;
    c->accel.n_flat_prims = (uint32_t)total;
    c->accel.placed.swap(placed);
    return RT3_OK;
}
// the shading records of the flattened world, remade only when what they depend on has changed since they were made
static int make_shade_records(rt3_ctx* c) {
    std::vector<uint64_t> key{c->scene.content_gen};
    for (const Placed& p : c->accel.placed) key.push_back(p.geom);
    ShadeRecords& s = c->accel.shade;
    if (key == s.key && s.has_tan == c->accel.has_normal_tex) return RT3_OK;
    s.key.clear();  // until the new records are in place
    s.has_tan = false;
    if (!s.rec || !s.uv || s.n != c->accel.n_flat_prims) {  // (a refit rewrites them in place)
        if (int r = dev_alloc(c, s.rec, (size_t)c->accel.n_flat_prims)) return r;
        if (int r = dev_alloc(c, s.uv, 3 * (size_t)c->accel.n_flat_prims)) return r;
        s.n = c->accel.n_flat_prims;
    }
    launch_tri_shade(c->stream, world_tables(c), c->accel.n_flat_prims, s.rec.get(), s.uv.get());
    HIPC(c, hipGetLastError());
    if (c->accel.has_normal_tex) {  // the tangent records go with the shading records: remade by the same builds and refits
        if (s.tan.capacity_bytes() < (size_t)c->accel.n_flat_prims * sizeof(uint32_t))  // (a refit rewrites them in place)
            if (int r = dev_alloc(c, s.tan, (size_t)c->accel.n_flat_prims)) return r;
        launch_tri_tangent(c->stream, world_tables(c), c->accel.n_flat_prims, s.tan.get());
        HIPC(c, hipGetLastError());
        s.has_tan = true;
    } else {
        s.tan.reset();
    }
    s.key = std::move(key);
    return RT3_OK;
}

namespace rt3 {

// The emitter table (RT3_F_NEE_EMISSIVE, rt3_lights.hip) of the current structure, remade when a build, refit or import has happened since.  The
// host walks only the flattened geometries (flatten_world's list) to find the emissive ones; the table itself is made on the GPU.
// With RT3_F_NEE_PUNCTUAL in `combo` the punctual lights follow the emitters; without RT3_F_NEE_EMISSIVE no triangle
// is an entry (geom_base all kMiss: emission keeps weight 1).  One table is kept, remade when the structure, the lights or the pair changes.
// A directional light's mass takes its R from the box of the flattened world's triangles, found on the device: the same in every layout
// and both instance modes.
int ensure_lights(rt3_ctx* c, uint32_t combo) {
    if (int r = check_accel_current(c)) return r;
    combo &= RT3_F_NEE_EMISSIVE | RT3_F_NEE_PUNCTUAL;
    const bool with_emit = (combo & RT3_F_NEE_EMISSIVE) != 0u;
    const bool with_punct = (combo & RT3_F_NEE_PUNCTUAL) != 0u && !c->scene.lights.empty();
    if (!with_punct) combo &= ~RT3_F_NEE_PUNCTUAL;  // no lights: the table of the other flag alone, whatever the list's stamp
    LightTable& lt = c->accel.lights;
    // textured emitters: the mode is part of the key, and with it the texture pool: the masses depend on texels
    const bool tex_mode = c->scene.textured_emitters;
    if (lt.stamp == c->accel.stamp && lt.combo == combo && (!with_punct || lt.lights_stamp == c->scene.lights_stamp) && lt.tex_mode == tex_mode &&
        (!tex_mode || lt.tex_stamp == c->scene.tex_stamp))
        return RT3_OK;
    HIPC(c, hipSetDevice(c->device));
    // is any geometry a textured emitter?  Only then does the mode change anything: non-zero emission, triangles, no mask, and an emissive
    // texture that is uploaded (hit_finish<true>'s has_e).  Without one the table is the mode-off table, bit for bit.
    bool tex_on = false;
    if (tex_mode && with_emit && any_mat_tex(c)) {
        if (int r = sync_textures(c)) return r;
        const int64_t n_tex = c->scene.d_tex_pixels ? (int64_t)c->scene.h_tex.size() : 0;
        for (const Placed& p : c->accel.placed) {
            const float* em = c->scene.h_geoms[p.geom].emission;
            const bool masked = any_cutoff(c) && c->scene.h_cutoffs[p.geom] > 0.0f;
            const int64_t et = c->scene.h_mat_tex[p.geom].emissive_texture;
            tex_on = tex_on || ((em[0] != 0.0f || em[1] != 0.0f || em[2] != 0.0f) && p.n_prims > 0 && !masked && et >= 0 && et < n_tex);
        }
    }
    std::vector<uint32_t> geom_base, eg_geom, eg_first;
    uint64_t n = 0;
    for (const Placed& p : c->accel.placed) {
        const float* em = c->scene.h_geoms[p.geom].emission;
        const bool masked = any_cutoff(c) && c->scene.h_cutoffs[p.geom] > 0.0f;  // left out: its points may be cut away
        // an emissive texture scales the radiance point by point: left out like a masked geometry, unless the
        // textured-emitter mode samples it (section 4x)
        const bool textured = !tex_on && any_mat_tex(c) && c->scene.h_mat_tex[p.geom].emissive_texture >= 0;
        const bool emissive = with_emit && (em[0] != 0.0f || em[1] != 0.0f || em[2] != 0.0f) && p.n_prims > 0 && !masked && !textured;
        geom_base.push_back(emissive ? (uint32_t)n : kMiss);
        if (emissive) {
            eg_geom.push_back((uint32_t)(geom_base.size() - 1));
            eg_first.push_back((uint32_t)n);
            n += p.n_prims;
        }
    }
    if (n + c->scene.lights.size() > 0x7FFFFFFFull) return fail(c, RT3_E_INVALID, "light table: too many entries");
    const SceneDev sc = scene_dev(c);
    const hipError_t e = lights_build(c->stream, world_tables(c), geom_base, eg_geom, eg_first, (uint32_t)n, &lt,
                                      with_punct ? reinterpret_cast<const float*>(c->scene.lights.data()) : nullptr,
                                      with_punct ? (uint32_t)c->scene.lights.size() : 0u, c->accel.n_flat_prims, tex_on ? &sc : nullptr);
    if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("emitter table: ") + hipGetErrorString(e));
    lt.stamp = c->accel.stamp;
    lt.combo = combo;
    lt.lights_stamp = c->scene.lights_stamp;
    lt.tex_mode = tex_mode;
    lt.tex_stamp = c->scene.tex_stamp;
    return RT3_OK;
}

}  // namespace rt3

extern "C" {

// worst-case stack use of the near-first walk over a tree of `depth` levels: (children per node - 1) entries per level above the leaves
static uint32_t stack_entries(uint32_t width, uint32_t depth) { return depth > 1 ? (width - 1) * (depth - 1) : 0; }

// ---- two-level structure (RT3_OPT_INSTANCE_MODE 1): shared bottom trees under a top tree over instance records
// Conservativeness of the two-level boxes: every box is grown by kTlPad times a bound on the magnitudes involved,
// three orders above the rounding it must cover; matrices with ||M3|| ||M3^-1|| above kTlMaxCondition are refused
constexpr double kTlPad = 1.0 / 4096.0;
constexpr double kTlMaxCondition = 1048576.0;
static void tl_reset(rt3_ctx* c) {
    c->accel.tl.valid = false;
    c->accel.tl.meshes.clear();
    c->accel.tl.n_meshes = c->accel.tl.n_built = c->accel.tl.n_top = 0;
    c->accel.tl.n_alloc_nodes = 0;
}
static void free_accel(rt3_ctx* c) {
    c->accel.bvh = LbvhResult{};
    tl_reset(c);
}
// the RT3_E_INVALID of a structure whose nodes and triangle records do not fit one arena of 32-bit byte offsets (LbvhResult::alloc_arena)
static int fail_arena(rt3_ctx* c, const char* who, uint64_t need) {
    return fail(c, RT3_E_INVALID, std::string(who) + ": the nodes and triangle records need " + std::to_string(need) + " bytes, the traversal kernels address " +
                                      std::to_string(kArenaMaxBytes) + " (one base + 32-bit offsets)");
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
// a table entry that places its triangles as they are: identity matrix, everything else zero
static FlatGeomDev identity_geom() {
    FlatGeomDev f;
    memset(&f, 0, sizeof(f));
    f.m[0] = f.m[4] = f.m[8] = 1.0f;
    f.identity = 1u;
    return f;
}
// the tables of a bottom tree over the geometries [first, first + count) as uploaded: identity matrices, local primitive ids
static hipError_t make_mesh_tables(rt3_ctx* c, const TlMesh& m, MeshTables* t) {
    std::vector<FlatGeomDev> tbl(m.count);
    std::vector<uint32_t> fp(m.count);
    uint32_t tot = 0;
    for (uint32_t k = 0; k < m.count; k++) {
        FlatGeomDev& f = tbl[k] = identity_geom();
        memcpy(&f.g, &c->scene.h_geoms[m.first + k], sizeof(f.g));
        f.geom = m.first + k;
        fp[k] = tot;
        tot += c->scene.h_prim_counts[m.first + k];
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
        e = lbvh_build(c->stream, mesh_tables(c, t), m.n_tris, c->opt.leaf_size, 4, 1, c->opt.collapse, c->opt.sah_top, c->accel.build_scratch, res,
                       c->accel.marked ? c->accel.d_geom_mask.get() : nullptr);
    uint32_t root[16];
    if (e == hipSuccess) e = hipMemcpyAsync(root, res->nodes.get(), 64, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (res->arena_need > kArenaMaxBytes) return fail_arena(c, "two-level: bottom tree", res->arena_need);
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

// The instance records and world boxes (host, a few KiB), then the top tree (GPU), over bottom trees that are in place: the tail of a
// two-level build, and what a refit redoes after the bottom trees' boxes moved.
static int tl_records_and_top(rt3_ctx* c) {
    TwoLevelState& tl = c->accel.tl;
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
        pack3x4(m, ff);
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
        c->accel.bvh.free_arena();
        c->accel.bvh.top.reset();
        tl.valid = false;
        tl.n_meshes = 0;
        tl.n_top = 0;
        c->accel.bvh.n_nodes = c->accel.bvh.n_tris = c->accel.bvh.n_top = 0;
        c->accel.bvh.max_depth = 0;
        c->accel.bvh.node_bytes = 64;
        c->accel.bvh.layout = kLayoutTwoLevel;
        return RT3_OK;
    }
    const size_t rec_bytes = rec.size() * 4;
    HIPC(c, hipMemcpyAsync(c->accel.bvh.nodes.get() + 4 * (size_t)top_cap, rec.data(), rec_bytes, hipMemcpyHostToDevice, c->stream));
    if (rec_bytes > (64u << 10)) c->accel.bulk_copies += 1;
    // the top build's inputs: boxes, degenerate triangles, a one-entry identity table, prim_geom = 0 and then first_prim = 0
    float *boxes_d = nullptr, *verts = nullptr;
    uint32_t *idx = nullptr, *zeros = nullptr;
    FlatGeomDev* tbl = nullptr;
    BufLayout plan;
    plan.add(&boxes_d, boxes.size()).add(&verts, (size_t)n_ne * 24).add(&idx, (size_t)n_ne * 3).add(&tbl, 1).add(&zeros, (size_t)n_ne + 1);
    HIPC(c, tl.scratch.grow_bytes(plan.bytes()));
    HIPC(c, plan.carve(tl.scratch));
    const FlatGeomDev tg = identity_geom();
    HIPC(c, hipMemcpyAsync(boxes_d, boxes.data(), boxes.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (boxes.size() * 4 > (64u << 10)) c->accel.bulk_copies += 1;
    HIPC(c, hipMemcpyAsync(tbl, &tg, sizeof(tg), hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemsetAsync(zeros, 0, ((size_t)n_ne + 1) * 4, c->stream));
    tlas_box_tris(c->stream, boxes_d, n_ne, verts, idx);
    LbvhResult top;
    hipError_t e = lbvh_build(c->stream, GeomTables{verts, idx, tbl, zeros, zeros + n_ne}, n_ne, 1u, 4u, 1u, c->opt.collapse, 1u, c->accel.build_scratch, &top);
    if (e == hipSuccess && top.n_nodes > top_cap) e = hipErrorInvalidValue;  // cannot happen (see top_cap); never write past the top's region
    if (e == hipSuccess) {
        tlas_emit_top(c->stream, top.nodes.get(), top.n_nodes, top.tris.get(), top_cap, c->accel.bvh.nodes.get());
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = lbvh_make_top(c->stream, c->accel.bvh.nodes.get(), tl.n_alloc_nodes, c->accel.bvh.top, &c->accel.bvh.n_top);
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
    c->accel.bvh.n_nodes = top_nodes + bottom_nodes;
    c->accel.bvh.n_tris = bottom_tris;
    c->accel.bvh.max_depth = top_depth + max_bottom;
    c->accel.bvh.node_bytes = 64;
    c->accel.bvh.layout = kLayoutTwoLevel;
    return RT3_OK;
}

static int build_two_level(rt3_ctx* c) {
    if (c->opt.node_width != 4 || c->opt.node_quant != 1)
        return fail(c, RT3_E_UNSUPPORTED, "instance mode 1 (two-level) needs the default node layout: RT3_OPT_NODE_WIDTH 4, RT3_OPT_NODE_QUANT 1");
    TwoLevelState& tl = c->accel.tl;
    if (!tl.valid) free_accel(c);  // what c->accel.bvh holds is a flattened tree (or nothing)
    rt3_instance whole;
    const auto [inst, n_inst] = placements(c, whole);

    // ---- matrices: the inverse (double, then fp32) and its conditioning; meshes = distinct geometry runs that hold triangles
    std::vector<TlInstance> ii(n_inst);
    std::vector<TlMesh> meshes;
    const std::vector<Placed>& placed = c->accel.placed;  // (flatten_world's, of this build: instance-major)
    size_t at = 0;
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
        for (; at < placed.size() && placed[at].instance == i; at++) cnt += placed[at].n_prims;
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
    bool same = tl.valid && tl.gen == c->scene.content_gen && tl.head == head && tl.meshes.size() == meshes.size();
    for (size_t q = 0; same && q < meshes.size(); q++) same = tl.meshes[q].first == meshes[q].first && tl.meshes[q].count == meshes[q].count;
    tl.n_built = 0;
    if (same) {
        meshes = tl.meshes;
    } else {
        const bool reuse = tl.valid && tl.gen == c->scene.content_gen;
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
        LbvhResult fresh;  // (only its arena is used: the combined node array, then the combined triangle records)
        hipError_t e = hipSuccess;
        if (rc == RT3_OK) {
            e = fresh.alloc_arena((size_t)nodes_total * 64, (size_t)tris_total, c->stream);
            if (fresh.arena_need > kArenaMaxBytes) rc = fail_arena(c, "two-level: bottom trees", fresh.arena_need);
        }
        if (rc == RT3_OK) {
            for (size_t q = 0; e == hipSuccess && q < meshes.size(); q++) {
                const TlMesh& m = meshes[q];
                if (from[q] >= 0) {
                    const TlMesh& om = tl.meshes[from[q]];
                    tlas_rebase_nodes(c->stream, c->accel.bvh.nodes.get() + 4 * (size_t)om.node_off, fresh.nodes.get() + 4 * (size_t)m.node_off, m.n_nodes, om.node_off,
                                      m.node_off, om.tri_off, m.tri_off);
                    e = hipMemcpyAsync(fresh.tris.get() + 3 * (size_t)m.tri_off, c->accel.bvh.tris.get() + 3 * (size_t)om.tri_off, (size_t)m.n_tris * 48, hipMemcpyDeviceToDevice,
                                       c->stream);
                } else {
                    tlas_rebase_nodes(c->stream, built[q].nodes.get(), fresh.nodes.get() + 4 * (size_t)m.node_off, m.n_nodes, 0u, m.node_off, 0u, m.tri_off);
                    e = hipMemcpyAsync(fresh.tris.get() + 3 * (size_t)m.tri_off, built[q].tris.get(), (size_t)m.n_tris * 48, hipMemcpyDeviceToDevice, c->stream);
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
        c->accel.bvh.take_arena(fresh);  // (the old arena, which kept bottom trees were copied from, goes here)
        tl.meshes = meshes;
        tl.head = head;
        tl.gen = c->scene.content_gen;
        tl.n_alloc_nodes = (uint32_t)nodes_total;
        tl.valid = true;
    }
    tl.inst = std::move(ii);
    tl.n_placed = n_ne;
    tl.top_cap = top_cap;
    return tl_records_and_top(c);
}

// ---- acceleration structure
// The alpha-mask tables of a build: per uploaded geometry the triangle records' last two words {cutoff bits, slot} and
// per masked geometry (slot) {texture index, base_color[3] bits}.  c->accel.masked: some placed geometry with triangles is masked.
static int make_alpha_tables(rt3_ctx* c) {
    c->accel.masked = c->accel.marked = false;
    c->accel.n_panes = c->accel.pane_first_slot = 0;
    // pane shadows: with the mode off, or without a placed pane, everything below is what it is without the mode
    std::vector<uint8_t> pane(c->scene.n_geoms, 0);
    for (const Placed& p : c->accel.placed)
        if (p.n_prims > 0 && pane_geometry(c, p.geom)) {
            pane[p.geom] = 1;
            c->accel.n_panes++;
        }
    if (!any_cutoff(c) && c->accel.n_panes == 0) return RT3_OK;
    if (c->opt.node_width != 4 || c->opt.node_quant != 1) {
        c->accel.n_panes = 0;
        return fail(c, RT3_E_UNSUPPORTED, any_cutoff(c) ? "alpha-masked geometry needs the default node layout (RT3_OPT_NODE_WIDTH 4, RT3_OPT_NODE_QUANT 1)"
                                                         : "pane shadows (rt3_scene_set_pane_shadows) need the default node layout (RT3_OPT_NODE_WIDTH 4, RT3_OPT_NODE_QUANT 1)");
    }
    std::vector<uint2> mask(c->scene.n_geoms, make_uint2(0u, 0u)), table;
    for (uint32_t g = 0; any_cutoff(c) && g < c->scene.n_geoms; g++) {
        if (!(c->scene.h_cutoffs[g] > 0.0f)) continue;
        uint32_t cb, ab;
        memcpy(&cb, &c->scene.h_cutoffs[g], 4);
        memcpy(&ab, &c->scene.h_geoms[g].base_color[3], 4);
        mask[g] = make_uint2(cb, (uint32_t)table.size());
        table.push_back(make_uint2((uint32_t)c->scene.h_geoms[g].base_color_texture_index, ab));
    }
    for (const Placed& p : c->accel.placed)
        if (mask[p.geom].x != 0u && p.n_prims > 0) c->accel.masked = true;
    // a pane's records: {0, 1} without a mask; with one {cutoff, a slot at or behind pane_first_slot that holds a copy of the geometry's entry},
    // which the MASK kernels read like any slot.  The words of every other record keep their bits.
    c->accel.pane_first_slot = (uint32_t)table.size();
    for (uint32_t g = 0; g < c->scene.n_geoms; g++) {
        if (!pane[g]) continue;
        if (mask[g].x != 0u) {
            table.push_back(table[mask[g].y]);
            mask[g].y = (uint32_t)table.size() - 1u;
        } else {
            mask[g] = make_uint2(0u, 1u);
        }
    }
    c->accel.marked = c->accel.masked || c->accel.n_panes != 0;
    if (int r = dev_alloc(c, c->accel.d_geom_mask, mask.size())) return r;
    if (int r = dev_alloc(c, c->accel.d_alpha, table.size())) return r;
    HIPC(c, hipMemcpy(c->accel.d_geom_mask.get(), mask.data(), mask.size() * sizeof(uint2), hipMemcpyHostToDevice));
    if (!table.empty()) HIPC(c, hipMemcpy(c->accel.d_alpha.get(), table.data(), table.size() * sizeof(uint2), hipMemcpyHostToDevice));
    return RT3_OK;
}
// ---- k_shadow's exit table (DESIGN.md sections 5 and 7; rt3_exit_table.hip).  Single-level structures of the default layout have room for it
// in their arena; it is (re)filled after a build, an import and a refit, and its counters start again.
static uint32_t exit_R(const rt3_ctx* c) {
    if (c->opt.instance_mode == 1 || c->opt.node_width != 4 || c->opt.node_quant != 1) return 0u;
    return kExitDefaultR;
}
static int make_exit_table(rt3_ctx* c) {
    LbvhResult& b = c->accel.bvh;
    b.exit.on = false;
    if (!b.exit.off || !b.exit.R || b.layout != kLayoutWide64Q || !b.n_nodes || !b.nodes || !c->accel.n_flat_prims) return RT3_OK;  // no table
    if (!c->accel.exit_counters) HIPC(c, c->accel.exit_counters.alloc_bytes(2 * sizeof(unsigned long long)));
    b.exit.counters = c->accel.exit_counters.get();
    HIPC(c, hipMemsetAsync(b.exit.counters, 0, 2 * sizeof(unsigned long long), c->stream));
    if (c->opt.exit_table == 0) return RT3_OK;
    uint32_t root[16];
    double box[6];
    HIPC(c, hipMemcpyAsync(root, b.nodes.get(), 64, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    quantised_node_box(root, box);
    for (int k = 0; k < 3; k++) {
        if (!(box[k] <= box[3 + k])) return RT3_OK;  // a root without children: nothing to lay cells on
        b.exit.lo[k] = round_down(box[k]);
        b.exit.hi[k] = round_up(box[3 + k]);
        const float ext = b.exit.hi[k] - b.exit.lo[k], s = (float)b.exit.R / ext;
        b.exit.scale[k] = (ext > 0.0f && std::isfinite(s)) ? s : 0.0f;  // a flat box: every ray falls in cell 0 of that axis
    }
    ExitScratch s;
    BufLayout plan;
    exit_table_plan(6u * b.exit.R * b.exit.R, c->accel.n_flat_prims, plan, &s);
    HIPC(c, c->accel.exit_scratch.grow_bytes(plan.bytes()));
    HIPC(c, plan.carve(c->accel.exit_scratch));
    const hipError_t e = exit_table_fill(c->stream, b, c->accel.n_flat_prims, s, c->opt.exit_table == 2);
    if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("exit table: ") + hipGetErrorString(e));
    b.exit.on = true;
    return RT3_OK;
}
extern "C++" {
namespace rt3 {
int exit_table_update(rt3_ctx* c) {
    if (!c->accel.built || c->accel.stale) return RT3_OK;  // the next build or refit fills it
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (int r = make_exit_table(c)) return r;
    HIPC(c, hipStreamSynchronize(c->stream));
    return RT3_OK;
}
void exit_counters_reset(rt3_ctx* c) {
    if (c->accel.exit_counters) (void)hipMemsetAsync(c->accel.exit_counters.get(), 0, 2 * sizeof(unsigned long long), c->stream);
}
}  // namespace rt3
}  // extern "C++"
// the structure's content changed (build, refit, import): what is made for one stamp (emitter table, motion tables) is remade at its next use
static void bump_stamp(rt3_ctx* c) { c->accel.stamp++; }
// the end of a successful build or refit: the shading records, then the structure goes live
static int accel_finish(rt3_ctx* c, uint32_t* out_handle) {
    if (int r = make_shade_records(c)) return r;
    if (int r = make_exit_table(c)) return r;
    HIPC(c, hipStreamSynchronize(c->stream));
    c->prof.stats.accel_bulk_copies += c->accel.bulk_copies;
    c->accel.bulk_copies = 0;
    c->accel.built = true;
    c->accel.stale = false;  // (read only while built: this is its one reset)
    bump_stamp(c);
    c->accel.topo_gen = c->scene.topo_gen;  // (unchanged by a refit, which needs the build's)
    if (out_handle) *out_handle = (RT3_TAG_ACCEL << 30) | 0u;
    return RT3_OK;
}
int rt3_accel_build(rt3_ctx* c, uint32_t* out_handle) {
    if (!c) return RT3_E_INVALID;
    HIPC(c, hipSetDevice(c->device));
    if (c->scene.n_prims && (!c->scene.d_verts || !c->scene.d_indices)) return fail(c, RT3_E_STATE, "set vertices, indices and geometry before rt3_accel_build");
    // the vertex / index buffers may have been replaced since rt3_scene_set_geometry checked its ranges against them
    if (int r = revalidate_geometry(c)) return r;
    HIPC(c, hipStreamSynchronize(c->stream));
    if (int r = check_skin_flags(c)) return r;  // a posed position out of range: nothing is built over it
    const auto t_build0 = std::chrono::steady_clock::now();
    // until the rebuild has succeeded: a failed one (the geometry tables reallocated by flatten_world included) must leave
    // RT3_E_STATE behind, not an empty tree or one that points at freed tables
    invalidate_accel(c);
    c->accel.refit_planned = false;
    if (int r = flatten_world(c)) return r;
    if (int r = make_alpha_tables(c)) return r;
    if (c->opt.instance_mode == 1) {
        if (int r = build_two_level(c)) return r;
    } else {
        free_accel(c);  // the old tree (two-level or not) goes before the new one is allocated
        hipError_t e = lbvh_build(c->stream, world_tables(c), c->accel.n_flat_prims, c->opt.leaf_size, c->opt.node_width, c->opt.node_quant, c->opt.collapse,
                                  c->opt.sah_top, c->accel.build_scratch, &c->accel.bvh, c->accel.marked ? c->accel.d_geom_mask.get() : nullptr, exit_R(c));
        if (c->accel.build_scratch.capacity_bytes() > ((size_t)1 << 30)) c->accel.build_scratch.reset();  // a big scene's scratch is not worth keeping resident
        if (e != hipSuccess) {
            const uint64_t need = c->accel.bvh.arena_need;
            free_accel(c);  // (what the failed build allocated)
            if (need > kArenaMaxBytes) return fail_arena(c, "lbvh_build", need);
            return fail(c, RT3_E_HIP, std::string("lbvh_build: ") + hipGetErrorString(e));
        }
        const uint32_t stack_need = stack_entries(c->opt.node_width, c->accel.bvh.max_depth);
        if (stack_need > kMaxStack) {
            const int rc = fail(c, RT3_E_DEPTH, "LBVH with " + std::to_string(c->accel.bvh.max_depth) + " levels needs " + std::to_string(stack_need) +
                                                    " stack entries, the traversal kernels hold " + std::to_string(kMaxStack));
            free_accel(c);  // (after the message: it clears max_depth)
            return rc;
        }
    }
    if (int r = accel_finish(c, out_handle)) return r;
    c->prof.stats.accel_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_build0).count();
    return RT3_OK;
}
int rt3_pane_shadow_info(rt3_ctx* c, uint32_t* n_panes) {
    if (!c || !c->accel.built) return fail(c, RT3_E_STATE, "no acceleration structure built");
    if (n_panes) *n_panes = c->accel.n_panes;
    return RT3_OK;
}
int rt3_rough_transmission_info(rt3_ctx* c, uint32_t* n_frosted) {
    if (!c || !c->accel.built) return fail(c, RT3_E_STATE, "no acceleration structure built");
    if (n_frosted) *n_frosted = c->accel.n_frosted;
    return RT3_OK;
}
int rt3_attenuation_info(rt3_ctx* c, uint32_t* n_absorbing) {
    if (!c || !c->accel.built) return fail(c, RT3_E_STATE, "no acceleration structure built");
    if (n_absorbing) *n_absorbing = c->accel.n_absorbing;
    return RT3_OK;
}
int rt3_accel_info(rt3_ctx* c, uint32_t* n_nodes, uint32_t* n_tris, uint32_t* max_depth, uint32_t* node_bytes) {
    if (!c || !c->accel.built) return fail(c, RT3_E_STATE, "no acceleration structure built");
    if (n_nodes) *n_nodes = c->accel.bvh.n_nodes;
    if (n_tris) *n_tris = c->accel.bvh.n_tris;
    if (max_depth) *max_depth = c->accel.bvh.max_depth;
    if (node_bytes) *node_bytes = c->accel.bvh.node_bytes;
    return RT3_OK;
}
int rt3_accel_levels(rt3_ctx* c, uint32_t* n_meshes, uint32_t* n_meshes_built, uint32_t* n_top_nodes, uint64_t* accel_bytes) {
    if (!c || !c->accel.built) return fail(c, RT3_E_STATE, "no acceleration structure built");
    const bool two = c->accel.bvh.layout == kLayoutTwoLevel;
    if (n_meshes) *n_meshes = two ? c->accel.tl.n_meshes : 0u;
    if (n_meshes_built) *n_meshes_built = two ? c->accel.tl.n_built : 0u;
    if (n_top_nodes) *n_top_nodes = two ? c->accel.tl.n_top : 0u;
    if (accel_bytes) {  // what the traversal kernels read: node array (two-level: top tree, instance records, bottom trees), triangle records, LDS top copy
        const uint64_t nodes = !c->accel.bvh.nodes ? 0u : (two ? (uint64_t)c->accel.tl.n_alloc_nodes * 64u : (uint64_t)c->accel.bvh.n_nodes * c->accel.bvh.node_bytes);
        *accel_bytes = nodes + (!c->accel.bvh.tris ? 0u : (uint64_t)c->accel.bvh.n_tris * 48u) + (uint64_t)c->accel.bvh.n_top * 64u;
    }
    return RT3_OK;
}
int rt3_accel_download(rt3_ctx* c, void* nodes, size_t nodes_bytes, void* tris, size_t tris_bytes) {
    if (int r = check_accel_current(c, "no acceleration structure built")) return r;
    if (c->accel.bvh.layout == kLayoutTwoLevel) return fail(c, RT3_E_UNSUPPORTED, "accel_download: not for the two-level structure (RT3_OPT_INSTANCE_MODE 1)");
    if (nodes) {
        if (nodes_bytes != (size_t)c->accel.bvh.n_nodes * c->accel.bvh.node_bytes) return fail(c, RT3_E_INVALID, "nodes_bytes mismatch");
        if (nodes_bytes) HIPC(c, hipMemcpy(nodes, c->accel.bvh.nodes.get(), nodes_bytes, hipMemcpyDeviceToHost));
    }
    if (tris) {
        if (tris_bytes != (size_t)c->accel.bvh.n_tris * 48) return fail(c, RT3_E_INVALID, "tris_bytes mismatch");
        if (tris_bytes) HIPC(c, hipMemcpy(tris, c->accel.bvh.tris.get(), tris_bytes, hipMemcpyDeviceToHost));
    }
    return RT3_OK;
}
// The counterpart of rt3_accel_download: install a tree somebody else built over the SAME flattened triangles (an offline builder,
// a cache of an earlier run; Vulkan's vkCmdCopyMemoryToAccelerationStructureKHR plays this role for the reference's driver).  Default
// layout only (64-byte quantised four-wide nodes, 48-byte triangle records).  Every reference is checked on the host before the
// kernels may follow it: in range, no node reachable twice (so the walk terminates), depth within the traversal stack.
int rt3_accel_import(rt3_ctx* c, const void* nodes, size_t nodes_bytes, const void* tris, size_t tris_bytes) {
    if (!c || !nodes || !tris) return fail(c, RT3_E_INVALID, "accel_import: NULL argument");
    if (!c->accel.built) return fail(c, RT3_E_STATE, "accel_import: build the scene's own structure first (rt3_accel_build makes the shading records)");
    if (c->accel.bvh.layout == kLayoutTwoLevel) return fail(c, RT3_E_UNSUPPORTED, "accel_import: not for the two-level structure (RT3_OPT_INSTANCE_MODE 1)");
    if (c->accel.bvh.layout != kLayoutWide64Q) return fail(c, RT3_E_UNSUPPORTED, "accel_import: default node layout only");
    if (any_cutoff(c)) return fail(c, RT3_E_UNSUPPORTED, "accel_import: not for a scene with alpha-masked geometry (rt3_scene_set_alpha_cutoffs)");
    if (c->accel.n_panes) return fail(c, RT3_E_UNSUPPORTED, "accel_import: not for a structure with panes (rt3_scene_set_pane_shadows): imported records carry no pane marks");
    if (nodes_bytes == 0 || nodes_bytes % 64 || tris_bytes % 48 || nodes_bytes / 64 > 0x3FFFFFFFull) return fail(c, RT3_E_INVALID, "accel_import: sizes must be multiples of 64 / 48 bytes");
    const uint32_t nn = (uint32_t)(nodes_bytes / 64), nt = (uint32_t)(tris_bytes / 48);
    const uint32_t* w = static_cast<const uint32_t*>(nodes);
    const uint32_t* tw = static_cast<const uint32_t*>(tris);
    for (uint32_t k = 0; k < nt; k++)
        if (tw[12 * (size_t)k + 9] >= c->accel.n_flat_prims) return fail(c, RT3_E_INVALID, "accel_import: triangle record " + std::to_string(k) + " names a primitive the scene does not have");
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
    LbvhResult fresh;  // (only its arena is used; the structure in place stays whole until the new one is complete)
    hipError_t e = fresh.alloc_arena(nodes_bytes, nt, c->stream, exit_R(c));  // (zeroes the over-read slack behind the last record)
    if (fresh.arena_need > kArenaMaxBytes) return fail_arena(c, "accel_import", fresh.arena_need);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(fresh.nodes.get(), nodes, nodes_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && tris_bytes) e = hipMemcpy(fresh.tris.get(), tris, tris_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("accel_import: ") + hipGetErrorString(e));
    c->accel.bvh.take_arena(fresh);
    c->accel.bvh.n_nodes = nn;
    c->accel.bvh.n_tris = nt;
    c->accel.bvh.max_depth = depth;
    c->accel.refit_planned = false;
    bump_stamp(c);
    e = lbvh_make_top(c->stream, c->accel.bvh.nodes.get(), nn, c->accel.bvh.top, &c->accel.bvh.n_top);
    if (e != hipSuccess) {
        invalidate_accel(c);
        return fail(c, RT3_E_HIP, std::string("accel_import: top-of-tree copy: ") + hipGetErrorString(e));
    }
    if (int r = make_exit_table(c)) {
        invalidate_accel(c);
        return r;
    }
    HIPC(c, hipStreamSynchronize(c->stream));
    return RT3_OK;
}
int rt3_accel_exit_table_info(rt3_ctx* c, uint32_t* cells, uint64_t* tried, uint64_t* occluded, uint32_t* in_use) {
    if (int r = check_accel_current(c, "no acceleration structure built")) return r;
    const ExitTable& t = c->accel.bvh.exit;
    unsigned long long cnt[2] = {0, 0};
    if (t.on) {
        HIPC(c, hipSetDevice(c->device));
        HIPC(c, hipStreamSynchronize(c->stream));
        HIPC(c, hipMemcpy(cnt, t.counters, sizeof(cnt), hipMemcpyDeviceToHost));
    }
    if (cells) *cells = t.on ? 6u * t.R * t.R : 0u;
    if (tried) *tried = cnt[0];
    if (occluded) *occluded = cnt[1];
    if (in_use) *in_use = (t.on && (cnt[0] < kExitWarmupTries || 4ull * cnt[1] >= cnt[0])) ? 1u : 0u;  // the launches' own decision
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
    HIPC(c, c->accel.refit_scratch.grow_bytes(plan.bytes()));
    HIPC(c, plan.carve(c->accel.refit_scratch));
    return RT3_OK;
}
static int refit_flat(rt3_ctx* c) {
    LbvhResult& b = c->accel.bvh;
    if (!b.n_nodes) return RT3_OK;
    if (!c->accel.refit_planned) {
        c->accel.refit_trees.clear();
        c->accel.refit_trees.resize(1);
        const hipError_t e = refit_plan(c->stream, b.nodes.get(), 0u, b.n_nodes, b.max_depth, &c->accel.refit_trees[0]);
        if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("accel_refit: plan: ") + hipGetErrorString(e));
        c->accel.refit_planned = true;
    }
    RefitScratch s;
    if (int r = refit_scratch(c, b.n_nodes, b.n_tris, &s)) return r;
    hipError_t e = refit_tree(c->stream, c->accel.refit_trees[0], world_tables(c), c->accel.n_flat_prims, 0u, b.n_tris, b.nodes.get(), b.tris.get(), s.bounds, s.nbox,
                              s.tbox);
    if (e == hipSuccess) e = lbvh_make_top(c->stream, b.nodes.get(), b.n_nodes, b.top, &b.n_top);
    if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("accel_refit: ") + hipGetErrorString(e));
    return RT3_OK;
}
// instance mode 1: every bottom tree in the combined arrays (object space, its own bounds and pad, as tl_build_mesh builds it), then the
// instance records and the top tree over the bottom trees' new root boxes
static int refit_two_level(rt3_ctx* c) {
    TwoLevelState& tl = c->accel.tl;
    tl.n_built = 0;
    if (!tl.valid) return RT3_OK;  // nothing placed: no trees
    const std::vector<TlMesh>& meshes = tl.meshes;
    const size_t nm = meshes.size();
    if (!c->accel.refit_planned) {
        c->accel.refit_trees.clear();
        c->accel.refit_trees.resize(nm);
        c->accel.refit_tables.clear();
        c->accel.refit_tables.resize(nm);
        for (size_t q = 0; q < nm; q++) {
            const TlMesh& m = meshes[q];
            hipError_t e = make_mesh_tables(c, m, &c->accel.refit_tables[q]);
            if (e == hipSuccess && m.count * sizeof(FlatGeomDev) > (64u << 10)) c->accel.bulk_copies += 1;
            if (e == hipSuccess) e = refit_plan(c->stream, c->accel.bvh.nodes.get(), m.node_off, m.n_nodes, m.depth, &c->accel.refit_trees[q]);
            if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("accel_refit: plan: ") + hipGetErrorString(e));
        }
        c->accel.refit_planned = true;
    }
    RefitScratch s;
    if (int r = refit_scratch(c, tl.n_alloc_nodes, c->accel.bvh.n_tris, &s)) return r;
    std::vector<uint32_t> roots(16 * nm);
    hipError_t e = hipSuccess;
    for (size_t q = 0; e == hipSuccess && q < nm; q++) {
        const TlMesh& m = meshes[q];
        e = refit_tree(c->stream, c->accel.refit_trees[q], mesh_tables(c, c->accel.refit_tables[q]), m.n_tris, m.tri_off, m.n_tris, c->accel.bvh.nodes.get(), c->accel.bvh.tris.get(),
                       s.bounds, s.nbox, s.tbox);
        if (e == hipSuccess) e = hipMemcpyAsync(&roots[16 * q], c->accel.bvh.nodes.get() + 4 * (size_t)m.node_off, 64, hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, RT3_E_HIP, std::string("accel_refit: bottom trees: ") + hipGetErrorString(e));
    for (size_t q = 0; q < nm; q++) quantised_node_box(&roots[16 * q], tl.meshes[q].box);
    tl.gen = c->scene.content_gen;  // the bottom trees now match the vertices: a later build that only moved instances keeps them
    return tl_records_and_top(c);
}
int rt3_accel_refit(rt3_ctx* c, uint32_t* out_handle) {
    if (!c) return RT3_E_INVALID;
    if (c->opt.node_width != 4 || c->opt.node_quant != 1)
        return fail(c, RT3_E_UNSUPPORTED, "accel_refit: default node layout only (RT3_OPT_NODE_WIDTH 4, RT3_OPT_NODE_QUANT 1)");
    if (!c->accel.built || c->accel.topo_gen != c->scene.topo_gen)
        return fail(c, RT3_E_STATE, "accel_refit: no acceleration structure for the current scene (only rt3_scene_update_vertices may come between rt3_accel_build and a refit)");
    const bool two = c->accel.bvh.layout == kLayoutTwoLevel;
    if (!two && c->accel.bvh.layout != kLayoutWide64Q) return fail(c, RT3_E_UNSUPPORTED, "accel_refit: default node layout only");
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (int r = check_skin_flags(c)) return r;  // (the structure stays stale: the skin's next valid pose and a refit recover)
    invalidate_accel(c);  // until the refit has succeeded: a failed one leaves boxes of neither the old nor the new vertices
    if (int r = two ? refit_two_level(c) : refit_flat(c)) return r;
    return accel_finish(c, out_handle);
}

// ---- emitter table of RT3_F_NEE_EMISSIVE
int rt3_light_info(rt3_ctx* c, uint32_t* n_emitters, uint64_t* cdf_total) {
    if (!c) return RT3_E_INVALID;
    if (int r = ensure_lights(c)) return r;
    if (n_emitters) *n_emitters = c->accel.lights.n;
    if (cdf_total) *cdf_total = c->accel.lights.total;
    return RT3_OK;
}
int rt3_light_download(rt3_ctx* c, uint32_t* prim, float* area, uint32_t* mass) {
    if (!c) return RT3_E_INVALID;
    if (int r = ensure_lights(c)) return r;
    const LightTable& t = c->accel.lights;  // (the table of RT3_F_NEE_EMISSIVE alone: emitters only)
    if (!t.n) return RT3_OK;
    if (prim) HIPC(c, hipMemcpy(prim, t.prim.get(), (size_t)t.n * 4, hipMemcpyDeviceToHost));
    if (area) HIPC(c, hipMemcpy(area, t.area.get(), (size_t)t.n * 4, hipMemcpyDeviceToHost));
    if (mass) {
        HIPC(c, hipMemcpy(mass, t.cdf.get(), (size_t)t.n * 4, hipMemcpyDeviceToHost));
        for (uint32_t k = t.n - 1; k > 0; k--) mass[k] -= mass[k - 1];  // inclusive CDF -> masses
    }
    return RT3_OK;
}

int rt3_light_masses(rt3_ctx* c, uint32_t flags, uint32_t* n_emitters, uint32_t* n_punctual, uint32_t* mass) {
    if (!c) return RT3_E_INVALID;
    const uint32_t combo = flags & (RT3_F_NEE_EMISSIVE | RT3_F_NEE_PUNCTUAL);
    if (int r = ensure_lights(c, combo ? combo : RT3_F_NEE_EMISSIVE)) return r;  // (no flag: nothing is sampled, but the state is still checked)
    const LightTable& t = c->accel.lights;
    const bool any = combo != 0u && t.n != 0u;
    if (n_emitters) *n_emitters = any ? t.n_emit : 0u;
    if (n_punctual) *n_punctual = any ? t.n_punct : 0u;
    if (!any || !mass) return RT3_OK;
    HIPC(c, hipMemcpy(mass, t.cdf.get(), (size_t)t.n * 4, hipMemcpyDeviceToHost));
    for (uint32_t k = t.n - 1; k > 0; k--) mass[k] -= mass[k - 1];  // inclusive CDF -> masses
    return RT3_OK;
}

int rt3_light_table(rt3_ctx* c, uint32_t flags, float* rec, uint32_t* cdf, uint32_t* guide, uint32_t* prim, float* area, uint32_t* cells, uint32_t* shift) {
    if (!c) return RT3_E_INVALID;
    const uint32_t combo = flags & (RT3_F_NEE_EMISSIVE | RT3_F_NEE_PUNCTUAL);
    if (int r = ensure_lights(c, combo ? combo : RT3_F_NEE_EMISSIVE)) return r;  // (rt3_light_masses' rule)
    const LightTable& t = c->accel.lights;
    const bool any = combo != 0u && t.n != 0u;
    if (cells) *cells = any ? t.n_guide : 0u;
    if (shift) *shift = any ? t.guide_shift : 0u;
    if (!any) return RT3_OK;
    if (rec) HIPC(c, hipMemcpy(rec, t.rec.get(), (size_t)t.n * 64, hipMemcpyDeviceToHost));
    if (cdf) HIPC(c, hipMemcpy(cdf, t.cdf.get(), (size_t)t.n * 4, hipMemcpyDeviceToHost));
    if (guide) HIPC(c, hipMemcpy(guide, t.guide.get(), ((size_t)t.n_guide + 1) * 4, hipMemcpyDeviceToHost));
    if (prim) HIPC(c, hipMemcpy(prim, t.prim.get(), (size_t)t.n * 4, hipMemcpyDeviceToHost));
    if (area) HIPC(c, hipMemcpy(area, t.area.get(), (size_t)t.n * 4, hipMemcpyDeviceToHost));
    return RT3_OK;
}

// the side array of a table with textured emitters: 8 words per entry {uv0, uv1, uv2, texture index or -1, pad}
int rt3_light_emit_tex(rt3_ctx* c, uint32_t flags, uint32_t* n_entries, void* out) {
    if (!c) return RT3_E_INVALID;
    const uint32_t combo = flags & (RT3_F_NEE_EMISSIVE | RT3_F_NEE_PUNCTUAL);
    if (int r = ensure_lights(c, combo ? combo : RT3_F_NEE_EMISSIVE)) return r;  // (rt3_light_masses' rule)
    const LightTable& t = c->accel.lights;
    const bool any = combo != 0u && t.n != 0u && t.textured;
    if (n_entries) *n_entries = any ? t.n : 0u;
    if (any && out) HIPC(c, hipMemcpy(out, t.emit_tex.get(), (size_t)t.n * sizeof(EmitTexDev), hipMemcpyDeviceToHost));
    return RT3_OK;
}

}  // extern "C"
