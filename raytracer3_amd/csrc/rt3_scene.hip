// rt3_scene.hip -- host layer, what the caller uploads: vertices, indices, geometry and its validation, alpha cutoffs, the sky and its
// sampling tables, blue noise, textures and their device atlas, instances, the previous frame's transforms and vertex positions
// (include/rt3.h: rt3_scene_*, rt3_sky_download).  Owns rt3_ctx::scene and rt3_ctx::deform.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "rt3_ctx.hpp"

using namespace rt3;

// bounds of every geometry's index / vertex range against the world buffers as they are NOW: the kernels index them without
// checks (a GPU fault would take the node down).  Run by rt3_scene_set_geometry and again by rt3_accel_build, because the vertex
// and index buffers may be replaced (by smaller ones) after the geometry was set.
// spans: per geometry the vertices [vertex_offset + least index, vertex_offset + largest index] its triangles lie in ({1, 0}: none)
static int validate_geometry(rt3_ctx* c, const rt3_geometry_info* g, const uint32_t* prim_counts, uint32_t n,
                             std::vector<std::pair<uint32_t, uint32_t>>* spans = nullptr) {
    for (uint32_t i = 0; i < n; i++) {
        if ((uint64_t)g[i].index_offset + 3ull * prim_counts[i] > c->scene.n_indices)
            return fail(c, RT3_E_INVALID, "geometry " + std::to_string(i) + ": index range exceeds the index buffer");
        uint32_t mx = 0, mn = 0xFFFFFFFFu;
        for (uint64_t k = 0; k < 3ull * prim_counts[i]; k++) {
            uint32_t v = c->scene.h_indices[g[i].index_offset + k];
            mx = v > mx ? v : mx;
            mn = v < mn ? v : mn;
        }
        if (prim_counts[i] && (uint64_t)g[i].vertex_offset + mx >= (uint64_t)c->scene.n_verts)
            return fail(c, RT3_E_INVALID, "geometry " + std::to_string(i) + ": vertex range exceeds the vertex buffer (set vertices and indices before geometry)");
        if (spans) spans->push_back(prim_counts[i] ? std::make_pair(g[i].vertex_offset + mn, g[i].vertex_offset + mx) : std::make_pair(1u, 0u));
    }
    return RT3_OK;
}

namespace rt3 {

// a change every tree's shape depends on: the structure goes, and a refit cannot bring it back
void invalidate_topology(rt3_ctx* c) {
    invalidate_accel(c);
    c->scene.topo_gen++;
    c->scene.content_gen++;
}

// (re)build the device texture atlas after rt3_scene_set_texture calls
int sync_textures(rt3_ctx* c) {
    if (!c->scene.tex_dirty) return RT3_OK;
    std::vector<uint4> table(c->scene.h_tex.size());
    size_t total = 0;
    for (size_t i = 0; i < c->scene.h_tex.size(); i++) {
        if (c->scene.h_tex[i].empty()) return fail(c, RT3_E_STATE, "texture " + std::to_string(i) + " was never set (indices must be dense)");
        table[i] = make_uint4((uint32_t)total, c->scene.tex_w[i], c->scene.tex_h[i], 0u);
        total += c->scene.h_tex[i].size();
    }
    if (total > 0xFFFFFFF0ull) return fail(c, RT3_E_INVALID, "textures exceed 4 GiB");
    std::vector<uint8_t> all(total);
    for (size_t i = 0; i < c->scene.h_tex.size(); i++) memcpy(all.data() + table[i].x, c->scene.h_tex[i].data(), c->scene.h_tex[i].size());
    if (int r = dev_alloc(c, c->scene.d_tex_pixels, total)) return r;
    if (int r = dev_alloc(c, c->scene.d_tex_table, table.size())) return r;
    HIPC(c, hipMemcpy(c->scene.d_tex_pixels.get(), all.data(), total, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->scene.d_tex_table.get(), table.data(), table.size() * sizeof(uint4), hipMemcpyHostToDevice));
    if (!c->scene.d_srgb_lut) {
        float lut[256];
        for (int i = 0; i < 256; i++) {  // sRGB EOTF (IEC 61966-2-1), evaluated in double
            double v = i / 255.0;
            lut[i] = (float)(v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4));
        }
        if (int r = dev_alloc(c, c->scene.d_srgb_lut, (size_t)256)) return r;
        HIPC(c, hipMemcpy(c->scene.d_srgb_lut.get(), lut, sizeof(lut), hipMemcpyHostToDevice));
    }
    c->scene.tex_dirty = false;
    return RT3_OK;
}
int revalidate_geometry(rt3_ctx* c) {
    std::vector<std::pair<uint32_t, uint32_t>> spans;  // (the indices may have been replaced since rt3_scene_set_geometry)
    if (int r = validate_geometry(c, c->scene.h_geoms.data(), c->scene.h_prim_counts.data(), (uint32_t)c->scene.h_geoms.size(), &spans)) return r;
    c->scene.h_geom_span.swap(spans);
    return RT3_OK;
}
// Which geometries are deformed: geometry g is when some vertex of its span differs from the snapshot in a position
// word.  Only vertices updated since the snapshot can differ, so the compare kernel runs over the spans' intersections with the dirty
// ranges, in chunks of at most kDeformChunk vertices; with none no kernel runs.  Leaves the flags in h_deformed and marks the motion
// tables for a rebuild.
int deform_flags(rt3_ctx* c) {
    if (!c->deform.dirty) return RT3_OK;
    c->deform.h_deformed.assign(c->scene.n_geoms, 0u);
    std::vector<uint4> chunks;
    if (c->deform.snapshot)
        for (uint32_t g = 0; g < c->scene.n_geoms && g < c->scene.h_geom_span.size(); g++) {
            const auto [lo, hi] = c->scene.h_geom_span[g];
            if (lo > hi) continue;
            for (const auto& r : c->deform.ranges) {  // (every range lies inside the vertex buffer and the snapshot: rt3_scene_update_vertices)
                const uint32_t a = std::max(lo, r.first), b = std::min(hi + 1u, r.second);
                for (uint32_t at = a; at < b; at += kDeformChunk) chunks.push_back(make_uint4(g, at, std::min(b, at + kDeformChunk), 0u));
            }
        }
    if (!chunks.empty()) {
        HIPC(c, hipSetDevice(c->device));
        HIPC(c, hipStreamSynchronize(c->stream));  // an earlier launch may still read the chunk table
        HIPC(c, c->deform.d_chunks.grow_bytes(chunks.size() * sizeof(uint4)));
        HIPC(c, c->deform.d_deformed.grow_bytes((size_t)c->scene.n_geoms * 4));
        HIPC(c, hipMemcpy(c->deform.d_chunks.get(), chunks.data(), chunks.size() * sizeof(uint4), hipMemcpyHostToDevice));
        HIPC(c, hipMemsetAsync(c->deform.d_deformed.get(), 0, (size_t)c->scene.n_geoms * 4, c->stream));
        {
            ScopedTimer t(c, CAT_OTHER);
            launch_compare_positions(c->stream, c->scene.d_verts.get(), c->deform.d_prev_pos.get(), c->deform.d_chunks.get(), (uint32_t)chunks.size(), c->deform.d_deformed.get());
        }
        HIPC(c, hipGetLastError());
        HIPC(c, hipMemcpyAsync(c->deform.h_deformed.data(), c->deform.d_deformed.get(), (size_t)c->scene.n_geoms * 4, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));
    }
    c->deform.dirty = false;
    motion_tables_stale(c);
    return RT3_OK;
}
int check_skin_flags(rt3_ctx* c) {
    auto& list = c->skin.list;
    if (std::none_of(list.begin(), list.end(), [](const Skin& s) { return s.flag_pending; })) return RT3_OK;
    std::vector<uint32_t> words(list.size());
    HIPC(c, hipMemcpy(words.data(), c->skin.d_flags.get(), words.size() * 4, hipMemcpyDeviceToHost));
    size_t bad = list.size();
    for (size_t s = 0; s < list.size(); s++) {
        if (!list[s].flag_pending) continue;
        if (words[s] == 0u) list[s].flag_pending = false;  // (a set flag stays pending: only the skin's next pose clears the word)
        else if (bad == list.size()) bad = s;
    }
    if (bad != list.size()) return fail(c, RT3_E_INVALID, "skin " + std::to_string(bad) + ": a posed position is not finite (or beyond 1e18)");
    return RT3_OK;
}

}  // namespace rt3

extern "C" {

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
    c->deform.snapshot = false;
    c->deform.ranges.clear();
    c->deform.dirty = true;
}
// a NaN / infinite position would poison the scene bounds, the Morton codes and every box above it: reject it here
// (bounded magnitude too, so that box extents and the quantisation grid cannot overflow to infinity).  v: n vertices, the first of them
// vertex `first` of the buffer
static int check_positions(rt3_ctx* c, const float* v, uint32_t first, uint32_t n) {
    for (size_t i = 0; i < (size_t)n; i++)
        for (int k = 0; k < 3; k++)
            if (!(std::fabs(v[8 * i + k]) <= 1.0e18f)) return fail(c, RT3_E_INVALID, "vertex " + std::to_string(first + i) + ": position is not finite (or beyond 1e18)");
    return RT3_OK;
}
// every skin goes; a launch in flight may still read them, so the stream is drained first -- only when there are any
static int forget_skins(rt3_ctx* c) {
    if (c->skin.list.empty()) return RT3_OK;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    c->skin.list.clear();
    for (PaletteSlot& s : c->skin.ring) s.in_flight = false;
    return RT3_OK;
}
int rt3_scene_set_vertices(rt3_ctx* c, const float* v, uint32_t n) {
    if (!c || (!v && n)) return fail(c, RT3_E_INVALID, "vertices NULL");
    if (int r = check_positions(c, v, 0u, n)) return r;
    HIPC(c, hipSetDevice(c->device));
    if (int r = forget_skins(c)) return r;  // the buffer they index is replaced
    if (int r = dev_alloc(c, c->scene.d_verts, (size_t)n * 8)) return r;
    if (n) HIPC(c, hipMemcpy(c->scene.d_verts.get(), v, (size_t)n * 32, hipMemcpyHostToDevice));
    c->scene.n_verts = n;
    invalidate_topology(c);
    forget_snapshot(c);
    return RT3_OK;
}
// vertices [first, first + n) in place; the shape of every tree stays, so a structure built before is stale, not gone (rt3_accel_refit)
int rt3_scene_update_vertices(rt3_ctx* c, const float* v, uint32_t first, uint32_t n) {
    if (!c || (!v && n)) return fail(c, RT3_E_INVALID, "vertices NULL");
    if ((uint64_t)first + n > c->scene.n_verts) return fail(c, RT3_E_INVALID, "update_vertices: [first, first + n) exceeds the vertex buffer (rt3_scene_set_vertices)");
    if (int r = check_positions(c, v, first, n)) return r;
    if (n == 0) return RT3_OK;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));  // work in flight may still read the old vertices
    c->scene.content_gen++;
    mark_accel_stale(c);
    HIPC(c, hipMemcpy(c->scene.d_verts.get() + 8 * (size_t)first, v, (size_t)n * 32, hipMemcpyHostToDevice));
    if (c->deform.snapshot) {
        add_dirty_range(c->deform.ranges, first, first + n);
        c->deform.dirty = true;
    }
    return RT3_OK;
}
// "the positions the vertex buffer holds now are the previous frame's" (DESIGN.md section 4i): a device-side copy of the ranges updated since
// the last snapshot (the first one: of every vertex) on the context's stream.  Nothing a build or refit reads changes.
int rt3_scene_snapshot_vertices(rt3_ctx* c) {
    if (!c) return fail(c, RT3_E_INVALID, "context NULL");
    if (!c->scene.d_verts || c->scene.n_verts == 0) return fail(c, RT3_E_STATE, "snapshot_vertices: no vertices (rt3_scene_set_vertices)");
    HIPC(c, hipSetDevice(c->device));
    if (!c->deform.snapshot) {
        HIPC(c, hipStreamSynchronize(c->stream));  // an earlier "motion" launch may still read the old records
        HIPC(c, c->deform.d_prev_pos.grow_bytes((size_t)c->scene.n_verts * sizeof(float4)));
        c->deform.ranges.assign(1, {0u, c->scene.n_verts});
    }
    for (const auto& r : c->deform.ranges) {
        ScopedTimer t(c, CAT_OTHER);
        launch_snapshot_positions(c->stream, c->scene.d_verts.get(), r.first, r.second - r.first, c->deform.d_prev_pos.get());
    }
    HIPC(c, hipGetLastError());
    c->deform.ranges.clear();
    c->deform.snapshot = true;
    c->deform.dirty = true;
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
    if (!c->deform.snapshot) return fail(c, RT3_E_STATE, "deformed_geometries: no snapshot (rt3_scene_snapshot_vertices)");
    if (n != c->scene.n_geoms) return fail(c, RT3_E_INVALID, "deformed_geometries: n must be the geometry count of rt3_scene_set_geometry (" + std::to_string(c->scene.n_geoms) + ")");
    if (int r = deform_flags(c)) return r;
    for (uint32_t i = 0; i < n; i++) flags[i] = c->deform.h_deformed[i] ? 1 : 0;
    return RT3_OK;
}
int rt3_scene_set_indices(rt3_ctx* c, const uint32_t* idx, uint32_t n) {
    if (!c || (!idx && n)) return fail(c, RT3_E_INVALID, "indices NULL");
    HIPC(c, hipSetDevice(c->device));
    if (int r = dev_alloc(c, c->scene.d_indices, (size_t)n)) return r;
    if (n) HIPC(c, hipMemcpy(c->scene.d_indices.get(), idx, (size_t)n * 4, hipMemcpyHostToDevice));
    c->scene.n_indices = n;
    c->scene.h_indices.assign(idx, idx + n);
    invalidate_topology(c);
    forget_snapshot(c);
    return RT3_OK;
}
int rt3_scene_set_geometry(rt3_ctx* c, const rt3_geometry_info* g, const uint32_t* prim_counts, uint32_t n) {
    if (!c || ((!g || !prim_counts) && n)) return fail(c, RT3_E_INVALID, "geometry NULL");
    HIPC(c, hipSetDevice(c->device));
    std::vector<std::pair<uint32_t, uint32_t>> spans;
    if (int r = validate_geometry(c, g, prim_counts, n, &spans)) return r;
    c->scene.h_geom_span.swap(spans);
    uint64_t total = 0;
    int64_t max_tex = -1;
    for (uint32_t i = 0; i < n; i++) {
        if (g[i].base_color_texture_index > max_tex) max_tex = g[i].base_color_texture_index;
        total += prim_counts[i];
    }
    if (total > 0x7FFFFFFFull) return fail(c, RT3_E_INVALID, "too many primitives");
    // (the device tables -- one entry per (instance, geometry) -- are made by rt3_accel_build, which knows the instances)
    c->scene.h_geoms.assign(g, g + n);
    c->scene.h_prim_counts.assign(prim_counts, prim_counts + n);
    c->scene.h_cutoffs.clear();  // every geometry opaque again
    c->scene.h_mat_tex.clear();  // and without material textures
    c->scene.h_transmission.clear();  // and without glass
    c->scene.h_attenuation.clear();   // and without absorption
    c->scene.n_geoms = n;
    c->scene.max_tex_index = max_tex;
    c->scene.n_prims = (uint32_t)total;
    invalidate_topology(c);
    forget_snapshot(c);
    return RT3_OK;
}
// alpha cutoffs of the geometries of the last rt3_scene_set_geometry; n = 0: all opaque
int rt3_scene_set_alpha_cutoffs(rt3_ctx* c, const float* cutoffs, uint32_t n) {
    if (!c || (!cutoffs && n)) return fail(c, RT3_E_INVALID, "alpha cutoffs NULL");
    if (n != 0 && n != c->scene.n_geoms)
        return fail(c, RT3_E_INVALID, "alpha cutoffs: n must be 0 or the geometry count of rt3_scene_set_geometry (" + std::to_string(c->scene.n_geoms) + ")");
    for (uint32_t i = 0; i < n; i++)
        if (!(cutoffs[i] >= 0.0f && cutoffs[i] <= 1.0f)) return fail(c, RT3_E_INVALID, "alpha cutoff " + std::to_string(i) + " is not in [0, 1]");
    c->scene.h_cutoffs.clear();
    if (std::any_of(cutoffs, cutoffs + n, [](float v) { return v > 0.0f; })) c->scene.h_cutoffs.assign(cutoffs, cutoffs + n);  // (kept only when some geometry is masked)
    invalidate_topology(c);  // the triangle records carry the masks: a new build, not a refit
    return RT3_OK;
}
// material textures of the geometries of the last rt3_scene_set_geometry; n = 0: none
int rt3_scene_set_material_textures(rt3_ctx* c, const rt3_material_textures* m, uint32_t n) {
    if (!c || (!m && n)) return fail(c, RT3_E_INVALID, "material textures NULL");
    if (n != 0 && n != c->scene.n_geoms)
        return fail(c, RT3_E_INVALID, "material textures: n must be 0 or the geometry count of rt3_scene_set_geometry (" + std::to_string(c->scene.n_geoms) + ")");
    for (uint32_t i = 0; i < n; i++) {
        if (m[i].metallic_roughness_texture < -1 || m[i].normal_texture < -1 || m[i].emissive_texture < -1)
            return fail(c, RT3_E_INVALID, "material textures: entry " + std::to_string(i) + " has a texture index below -1");
        if (!(std::fabs(m[i].normal_scale) <= kFloatMax)) return fail(c, RT3_E_INVALID, "material textures: normal_scale " + std::to_string(i) + " is not finite");
    }
    c->scene.h_mat_tex.clear();
    if (std::any_of(m, m + n, [](const rt3_material_textures& e) { return e.metallic_roughness_texture >= 0 || e.normal_texture >= 0 || e.emissive_texture >= 0; }))
        c->scene.h_mat_tex.assign(m, m + n);  // (kept only when some geometry names a texture)
    invalidate_topology(c);  // the side table and the tangent records are made by a build
    return RT3_OK;
}
// transmission of the geometries of the last rt3_scene_set_geometry; n = 0: no glass
int rt3_scene_set_transmission(rt3_ctx* c, const rt3_transmission* t, uint32_t n) {
    if (!c || (!t && n)) return fail(c, RT3_E_INVALID, "transmission NULL");
    if (n != 0 && n != c->scene.n_geoms)
        return fail(c, RT3_E_INVALID, "transmission: n must be 0 or the geometry count of rt3_scene_set_geometry (" + std::to_string(c->scene.n_geoms) + ")");
    for (uint32_t i = 0; i < n; i++) {
        if (!(t[i].transmission >= 0.0f && t[i].transmission <= 1.0f)) return fail(c, RT3_E_INVALID, "transmission " + std::to_string(i) + " is not in [0, 1]");
        if (!(t[i].ior >= 1.0f && t[i].ior <= kFloatMax)) return fail(c, RT3_E_INVALID, "transmission: ior " + std::to_string(i) + " is not a finite value >= 1");
        if (t[i].thin_walled > 1u) return fail(c, RT3_E_INVALID, "transmission: thin_walled " + std::to_string(i) + " is neither 0 nor 1");
        if (t[i].reserved != 0u) return fail(c, RT3_E_INVALID, "transmission: reserved " + std::to_string(i) + " must be 0");
    }
    c->scene.h_transmission.clear();
    if (std::any_of(t, t + n, [](const rt3_transmission& e) { return e.transmission > 0.0f; })) c->scene.h_transmission.assign(t, t + n);  // (kept only when some geometry is glass)
    invalidate_topology(c);  // the side table is made by a build
    return RT3_OK;
}
// absorption of the geometries of the last rt3_scene_set_geometry; n = 0: none
int rt3_scene_set_attenuation(rt3_ctx* c, const rt3_attenuation* a, uint32_t n) {
    if (!c || (!a && n)) return fail(c, RT3_E_INVALID, "attenuation NULL");
    if (n != 0 && n != c->scene.n_geoms)
        return fail(c, RT3_E_INVALID, "attenuation: n must be 0 or the geometry count of rt3_scene_set_geometry (" + std::to_string(c->scene.n_geoms) + ")");
    for (uint32_t i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++)
            if (!(a[i].sigma[k] >= 0.0f && a[i].sigma[k] <= kFloatMax))
                return fail(c, RT3_E_INVALID, "attenuation: sigma " + std::to_string(i) + " is not a finite value >= 0");
        if (a[i].reserved != 0u) return fail(c, RT3_E_INVALID, "attenuation: reserved " + std::to_string(i) + " must be 0");
    }
    c->scene.h_attenuation.clear();
    if (std::any_of(a, a + n, [](const rt3_attenuation& e) { return e.sigma[0] > 0.0f || e.sigma[1] > 0.0f || e.sigma[2] > 0.0f; }))
        c->scene.h_attenuation.assign(a, a + n);  // (kept only when some sigma is > 0)
    invalidate_topology(c);  // the side table is made by a build
    return RT3_OK;
}
// pane shadows: the mode is the context's, the classification is made by the next build
int rt3_scene_set_pane_shadows(rt3_ctx* c, int on) {
    if (!c) return RT3_E_INVALID;
    if (on != 0 && on != 1) return fail(c, RT3_E_INVALID, "pane shadows: the mode is 0 or 1");
    if ((on != 0) == c->pane_shadows) return RT3_OK;
    c->pane_shadows = on != 0;
    invalidate_topology(c);  // the triangle records carry the pane marks: a new build, not a refit
    return RT3_OK;
}
int rt3_scene_get_pane_shadows(rt3_ctx* c, int* on) {
    if (!c || !on) return fail(c, RT3_E_INVALID, "pane shadows: NULL");
    *on = c->pane_shadows ? 1 : 0;
    return RT3_OK;
}
// rough transmission: the mode is the context's, the classification is made by the next build
int rt3_scene_set_rough_transmission(rt3_ctx* c, int on) {
    if (!c) return RT3_E_INVALID;
    if (on != 0 && on != 1) return fail(c, RT3_E_INVALID, "rough transmission: the mode is 0 or 1");
    if ((on != 0) == c->rough_transmission) return RT3_OK;
    c->rough_transmission = on != 0;
    invalidate_topology(c);  // the glass side table carries the frost marks, and a frosted pane stops being a pane: a new build, not a refit
    return RT3_OK;
}
int rt3_scene_get_rough_transmission(rt3_ctx* c, int* on) {
    if (!c || !on) return fail(c, RT3_E_INVALID, "rough transmission: NULL");
    *on = c->rough_transmission ? 1 : 0;
    return RT3_OK;
}
// fog: the medium is the context's; the launches read it by value, so no structure or table depends on it
int rt3_scene_set_medium(rt3_ctx* c, const rt3_medium* m) {
    if (!c) return RT3_E_INVALID;
    if (!m) {
        c->medium.params = rt3_medium{};
        c->medium.set = c->medium.on = false;
        return RT3_OK;
    }
    bool any = false;
    for (int k = 0; k < 3; k++) {
        if (!(m->sigma_a[k] >= 0.0f && m->sigma_a[k] <= kFloatMax) || !(m->sigma_s[k] >= 0.0f && m->sigma_s[k] <= kFloatMax))
            return fail(c, RT3_E_INVALID, "medium: sigma_a and sigma_s must be finite values >= 0");
        if (!(m->sigma_a[k] + m->sigma_s[k] <= kFloatMax)) return fail(c, RT3_E_INVALID, "medium: sigma_a + sigma_s must be finite");
        any = any || m->sigma_a[k] + m->sigma_s[k] > 0.0f;
    }
    if (!(m->g > -1.0f && m->g < 1.0f)) return fail(c, RT3_E_INVALID, "medium: g must lie in (-1, 1)");
    for (int k = 0; k < 3; k++) {
        if (!(std::fabs(m->box_min[k]) <= kFloatMax && std::fabs(m->box_max[k]) <= kFloatMax)) return fail(c, RT3_E_INVALID, "medium: the box must be finite");
        if (!(m->box_min[k] < m->box_max[k])) return fail(c, RT3_E_INVALID, "medium: the box is empty (box_min must be below box_max on every axis)");
    }
    c->medium.params = *m;
    c->medium.set = true;
    c->medium.on = any;
    return RT3_OK;
}
int rt3_scene_get_medium(rt3_ctx* c, rt3_medium* out, int* enabled) {
    if (!c || (!out && !enabled)) return fail(c, RT3_E_INVALID, "medium: NULL");
    if (out) *out = c->medium.params;
    if (enabled) *enabled = c->medium.on ? 1 : 0;
    return RT3_OK;
}
// Sky storage and importance tables (north_star; the oracle's orc_scene_set_sky has the definitions and is built by the same
// arithmetic, in double, in the same order): radiance stored as RGB9E5 (packing.slang:99-162), marginal CDF over rows, one alias
// table per row with 16-bit keep-thresholds, pdf_uv = the density the quantised tables really realise.
static uint32_t host_rgb9e5(const float* c) {  // packing.slang:99-144 == rt3_math.hpp float3_to_rgb9e5
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
        if (!(rgb[i] >= 0.0f && rgb[i] <= kFloatMax))
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
    // Every density is positive: f = (lum + 1e-6) sin(theta_row) > 0 for every texel, so every row weight is above 0, and a realised column
    // weight is at least 1/65536 (Q >= 1/65536 for the column itself).  RT3_OPT_DEFER_SKY_LIGHT rests on it -- a light sample's pdf is positive
    // exactly when its sin(theta) is -- so the smallest stored value is kept, and path_setup checks it instead of assuming.
    float min_pdf = pdf[0];
    for (size_t i = 1; i < n; i++) min_pdf = std::min(min_pdf, pdf[i]);
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
    if (int r = dev_alloc(c, c->scene.d_guide_marg, gmarg.size())) return r;
    if (int r = dev_alloc(c, c->scene.d_sky_alias, alias.size())) return r;
    if (int r = dev_alloc(c, c->scene.d_sky, tiled.size())) return r;
    if (int r = dev_alloc(c, c->scene.d_cdf_marg, margp.size())) return r;
    HIPC(c, hipMemcpy(c->scene.d_guide_marg.get(), gmarg.data(), gmarg.size() * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->scene.d_sky_alias.get(), alias.data(), alias.size() * 4, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->scene.d_sky.get(), tiled.data(), tiled.size() * 8, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->scene.d_cdf_marg.get(), margp.data(), margp.size() * 4, hipMemcpyHostToDevice));
    c->scene.sky_w = w;
    c->scene.sky_h = h;
    c->scene.sky_wt = wt;
    c->scene.sky_min_pdf = min_pdf;
    exit_counters_reset(c);  // the shadow rays follow the sky's importance: the exit table's success rate is measured afresh
    return RT3_OK;
}
int rt3_scene_set_bluenoise(rt3_ctx* c, const uint8_t* rgba, uint32_t w, uint32_t h) {
    if (!c || !rgba || !w || !h) return fail(c, RT3_E_INVALID, "bluenoise NULL / empty");
    HIPC(c, hipSetDevice(c->device));
    if (int r = dev_alloc(c, c->scene.d_bn, (size_t)w * h * 4)) return r;
    HIPC(c, hipMemcpy(c->scene.d_bn.get(), rgba, (size_t)w * h * 4, hipMemcpyHostToDevice));
    c->scene.bn_w = w;
    c->scene.bn_h = h;
    c->scene.bn_stamp++;
    return RT3_OK;
}
// base-colour texture `index` (RGBA8, sRGB-encoded colour), sampled by hit_info when GeometryInfo.baseColorTextureIndex == index
int rt3_scene_set_texture(rt3_ctx* c, uint32_t index, const uint8_t* rgba, uint32_t w, uint32_t h) {
    if (!c || !rgba || !w || !h || w > 16384 || h > 16384 || index > 4096) return fail(c, RT3_E_INVALID, "texture: NULL / bad size / index");
    if (index >= c->scene.h_tex.size()) {
        c->scene.h_tex.resize(index + 1);
        c->scene.tex_w.resize(index + 1, 0);
        c->scene.tex_h.resize(index + 1, 0);
    }
    c->scene.h_tex[index].assign(rgba, rgba + (size_t)w * h * 4);
    c->scene.tex_w[index] = w;
    c->scene.tex_h[index] = h;
    c->scene.tex_dirty = true;
    c->scene.tex_stamp++;
    return RT3_OK;
}
int rt3_sky_download(rt3_ctx* c, uint32_t* alias, uint32_t* texels, float* marg, float* pdf) {
    if (!c || !c->scene.d_sky) return fail(c, RT3_E_STATE, "no sky set");
    const uint32_t w = c->scene.sky_w, h = c->scene.sky_h, wt = c->scene.sky_wt, ht = (h + 3) / 4;
    if (alias) HIPC(c, hipMemcpy(alias, c->scene.d_sky_alias.get(), (size_t)w * h * 4, hipMemcpyDeviceToHost));
    if (marg) HIPC(c, hipMemcpy(marg, c->scene.d_cdf_marg.get() + 1, (size_t)h * 4, hipMemcpyDeviceToHost));  // strip the padding
    if (texels || pdf) {  // un-tile
        std::vector<uint2> tiled((size_t)wt * ht * 16);
        HIPC(c, hipMemcpy(tiled.data(), c->scene.d_sky.get(), tiled.size() * 8, hipMemcpyDeviceToHost));
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) {
                const uint2 t = tiled[((size_t)(y >> 2) * wt + (x >> 2)) * 16 + (((y & 3u) << 2) | (x & 3u))];
                if (texels) texels[(size_t)y * w + x] = t.x;
                if (pdf) memcpy(&pdf[(size_t)y * w + x], &t.y, 4);
            }
    }
    return RT3_OK;
}

// matrix i of a list (column-major 4 x 4): finite and bounded, last row (0, 0, 0, 1); the error reads `what` i `not_finite` / `bad_row`
static int check_matrix(rt3_ctx* c, const float* m, uint32_t i, const char* what, const char* not_finite, const char* bad_row) {
    for (int k = 0; k < 16; k++)
        if (!(std::fabs(m[k]) <= 1.0e18f)) return fail(c, RT3_E_INVALID, what + std::to_string(i) + not_finite);
    if (m[3] != 0.0f || m[7] != 0.0f || m[11] != 0.0f || m[15] != 1.0f) return fail(c, RT3_E_INVALID, what + std::to_string(i) + bad_row);
    return RT3_OK;
}
// world/mod.rs:34-60,104-125: InstanceInfo{mesh_index, transform} + Transform{Mat4}, global instance / transform buffers
int rt3_scene_set_instances(rt3_ctx* c, const rt3_instance* inst, uint32_t n) {
    if (!c || (!inst && n)) return fail(c, RT3_E_INVALID, "instances NULL");
    for (uint32_t i = 0; i < n; i++)
        if (int r = check_matrix(c, inst[i].transform, i, "instance ", ": transform is not finite (or beyond 1e18)",
                                 ": the last row of the transform must be (0, 0, 0, 1) (VkTransformMatrixKHR is 3 x 4 too)"))
            return r;
    c->scene.h_instances.assign(inst, inst + n);
    invalidate_accel(c);
    return RT3_OK;
}
// The previous frame's matrices of the same instances, for the "motion" pass only: no build reads them and the structure stays as it is
int rt3_scene_set_prev_transforms(rt3_ctx* c, const float* transforms, uint32_t n) {
    if (!c || (!transforms && n)) return fail(c, RT3_E_INVALID, "previous transforms NULL");
    for (uint32_t i = 0; i < n; i++)
        if (int r = check_matrix(c, transforms + 16 * (size_t)i, i, "previous transform ", " is not finite (or beyond 1e18)",
                                 ": the last row must be (0, 0, 0, 1), as for an instance's matrix"))
            return r;
    c->scene.prev_transforms.assign(transforms, transforms + 16 * (size_t)n);
    motion_tables_stale(c);
    return RT3_OK;
}
// Punctual lights: no build reads them and the structure stays as it is; the light table follows lights_stamp
int rt3_scene_set_lights(rt3_ctx* c, const rt3_punctual_light* lights, uint32_t n) {
    if (!c || (!lights && n)) return fail(c, RT3_E_INVALID, "lights NULL");
    auto bad = [&](uint32_t i, const char* what) { return fail(c, RT3_E_INVALID, "light " + std::to_string(i) + ": " + what); };
    for (uint32_t i = 0; i < n; i++) {
        const rt3_punctual_light& l = lights[i];
        if (l.type > RT3_LIGHT_DIRECTIONAL) return bad(i, "unknown type");
        const float vals[] = {l.range, l.inner_cone, l.outer_cone, l.position[0], l.position[1], l.position[2], l.direction[0], l.direction[1], l.direction[2],
                              l.intensity[0], l.intensity[1], l.intensity[2]};
        for (float v : vals)
            if (!std::isfinite(v)) return bad(i, "a value is not finite");
        for (int k = 0; k < 3; k++)
            if (l.intensity[k] < 0.0f) return bad(i, "negative intensity");
        if (l.type != RT3_LIGHT_POINT && l.direction[0] == 0.0f && l.direction[1] == 0.0f && l.direction[2] == 0.0f) return bad(i, "zero direction");
        if (l.type == RT3_LIGHT_SPOT && !(0.0f <= l.inner_cone && l.inner_cone < l.outer_cone && l.outer_cone <= 1.57079637f))  // fp32(pi / 2)
            return bad(i, "cone angles must satisfy 0 <= inner < outer <= pi/2");
    }
    c->scene.lights.assign(lights, lights + n);
    for (rt3_punctual_light& l : c->scene.lights) l._pad0 = l._pad1 = l._pad2 = 0.0f;
    c->scene.lights_stamp++;
    return RT3_OK;
}
// Textured emitters: no build reads the mode and the structure stays as it is; the light table's key holds it
int rt3_scene_set_textured_emitters(rt3_ctx* c, int on) {
    if (!c) return RT3_E_INVALID;
    if (on != 0 && on != 1) return fail(c, RT3_E_INVALID, "textured emitters: the mode is 0 or 1");
    c->scene.textured_emitters = on != 0;
    return RT3_OK;
}
int rt3_scene_get_textured_emitters(rt3_ctx* c, int* on) {
    if (!c || !on) return fail(c, RT3_E_INVALID, "textured emitters: NULL");
    *on = c->scene.textured_emitters ? 1 : 0;
    return RT3_OK;
}

// ---- skins: the rest pose lives on the device; a pose sends the joint palette and the target weights
int rt3_scene_add_skin(rt3_ctx* c, const rt3_skin_desc* d, uint32_t* out_skin) {
    if (!c || !d) return fail(c, RT3_E_INVALID, "add_skin: NULL");
    if (!c->scene.d_verts) return fail(c, RT3_E_STATE, "add_skin: no vertices (rt3_scene_set_vertices)");
    auto bad = [&](const std::string& what) { return fail(c, RT3_E_INVALID, "add_skin: " + what); };
    const uint32_t first = d->first_vertex, n = d->n_vertices, nt = d->n_targets;
    if (n == 0 || (uint64_t)first + n > c->scene.n_verts) return bad("[first_vertex, first_vertex + n_vertices) is empty or exceeds the vertex buffer");
    for (size_t s = 0; s < c->skin.list.size(); s++)
        if (first < c->skin.list[s].first + c->skin.list[s].n && c->skin.list[s].first < first + n) return bad("the range overlaps skin " + std::to_string(s) + "'s");
    if (d->n_joints < 1u || d->n_joints > 65536u) return bad("n_joints must lie in 1 .. 65536");
    if (nt > RT3_SKIN_MAX_TARGETS) return bad("n_targets exceeds RT3_SKIN_MAX_TARGETS");
    if (!d->joints || !d->weights) return bad("joints or weights NULL");
    if ((d->target_dpos == nullptr) != (nt == 0u)) return bad("target_dpos must be NULL exactly when n_targets is 0");
    if (d->target_dnrm && nt == 0u) return bad("target_dnrm without targets");
    for (size_t i = 0; i < 4 * (size_t)n; i++) {
        if (d->joints[i] >= d->n_joints) return bad("vertex " + std::to_string(i / 4) + ": joint index " + std::to_string(d->joints[i]) + " is not below n_joints");
        if (!(d->weights[i] >= 0.0f && d->weights[i] <= kFloatMax)) return bad("vertex " + std::to_string(i / 4) + ": a weight is negative or not finite");
    }
    if (d->rest)
        if (int r = check_positions(c, d->rest, 0u, n)) return r;  // (the message counts from the skin's first vertex)
    for (const float* delta : {d->target_dpos, d->target_dnrm})
        for (size_t i = 0; delta && i < 3 * (size_t)nt * n; i++)
            if (!(std::fabs(delta[i]) <= kFloatMax)) return bad("target " + std::to_string(i / (3 * (size_t)n)) + ": a delta is not finite");
    HIPC(c, hipSetDevice(c->device));
    Skin s;
    s.first = first;
    s.n = n;
    s.n_joints = d->n_joints;
    s.n_targets = nt;
    const size_t delta_bytes = 12 * (size_t)nt * n;
    HIPC(c, s.rest.alloc_bytes(32 * (size_t)n));
    HIPC(c, s.joints.alloc_bytes(8 * (size_t)n));
    HIPC(c, s.weights.alloc_bytes(16 * (size_t)n));
    HIPC(c, s.palette.alloc_bytes(48 * (size_t)s.n_joints));
    if (nt) HIPC(c, s.dpos.alloc_bytes(delta_bytes));
    if (d->target_dnrm) HIPC(c, s.dnrm.alloc_bytes(delta_bytes));
    s.bytes = 32ull * n + 8ull * n + 16ull * n + 48ull * s.n_joints + (nt ? delta_bytes : 0) + (d->target_dnrm ? delta_bytes : 0) + 4ull;
    const size_t index = c->skin.list.size();
    if (index + 1 > c->skin.flags_cap) {  // more flag words: a launch in flight may hold the old ones
        const uint32_t cap = c->skin.flags_cap + 64u;
        DevBuf<uint32_t> grown;
        HIPC(c, hipStreamSynchronize(c->stream));
        HIPC(c, grown.alloc_bytes((size_t)cap * 4));
        HIPC(c, hipMemset(grown.get(), 0, (size_t)cap * 4));
        if (c->skin.flags_cap) HIPC(c, hipMemcpy(grown.get(), c->skin.d_flags.get(), (size_t)c->skin.flags_cap * 4, hipMemcpyDeviceToDevice));
        c->skin.d_flags = std::move(grown);
        c->skin.flags_cap = cap;
    }
    // the arrays go into allocations nothing reads yet; the buffer's own contents (rest NULL) are copied behind the work ahead in the stream
    if (d->rest) HIPC(c, hipMemcpy(s.rest.get(), d->rest, 32 * (size_t)n, hipMemcpyHostToDevice));
    else HIPC(c, hipMemcpyAsync(s.rest.get(), c->scene.d_verts.get() + 8 * (size_t)first, 32 * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    HIPC(c, hipMemcpy(s.joints.get(), d->joints, 8 * (size_t)n, hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(s.weights.get(), d->weights, 16 * (size_t)n, hipMemcpyHostToDevice));
    if (nt) HIPC(c, hipMemcpy(s.dpos.get(), d->target_dpos, delta_bytes, hipMemcpyHostToDevice));
    if (d->target_dnrm) HIPC(c, hipMemcpy(s.dnrm.get(), d->target_dnrm, delta_bytes, hipMemcpyHostToDevice));
    HIPC(c, hipMemsetAsync(c->skin.d_flags.get() + index, 0, 4, c->stream));  // (a cleared skin may have left its word set)
    c->skin.list.push_back(std::move(s));
    if (out_skin) *out_skin = (uint32_t)index;
    return RT3_OK;
}
int rt3_scene_clear_skins(rt3_ctx* c) {
    if (!c) return fail(c, RT3_E_INVALID, "context NULL");
    return forget_skins(c);
}
int rt3_scene_pose_skin(rt3_ctx* c, uint32_t skin, const float* joint_matrices, const float* target_weights) {
    if (!c) return fail(c, RT3_E_INVALID, "context NULL");
    if (skin >= c->skin.list.size()) return fail(c, RT3_E_INVALID, "pose_skin: no skin " + std::to_string(skin) + " (rt3_scene_add_skin)");
    Skin& s = c->skin.list[skin];
    if (!joint_matrices || (!target_weights && s.n_targets)) return fail(c, RT3_E_INVALID, "pose_skin: joint matrices or target weights NULL");
    // an instance's checks without the magnitude bound: what a large matrix makes of the positions is the range flag's to catch, on the device
    for (uint32_t i = 0; i < s.n_joints; i++) {
        const float* m = joint_matrices + 16 * (size_t)i;
        for (int k = 0; k < 16; k++)
            if (!(std::fabs(m[k]) <= kFloatMax)) return fail(c, RT3_E_INVALID, "pose_skin: joint matrix " + std::to_string(i) + " is not finite");
        if (m[3] != 0.0f || m[7] != 0.0f || m[11] != 0.0f || m[15] != 1.0f)
            return fail(c, RT3_E_INVALID, "pose_skin: joint matrix " + std::to_string(i) + ": the last row must be (0, 0, 0, 1), as for an instance's matrix");
    }
    SkinLaunch L = {};
    for (uint32_t t = 0; t < s.n_targets; t++) {
        if (!(std::fabs(target_weights[t]) <= kFloatMax)) return fail(c, RT3_E_INVALID, "pose_skin: target weight " + std::to_string(t) + " is not finite");
        L.a[t] = target_weights[t];
    }
    HIPC(c, hipSetDevice(c->device));
    // the palette, packed 3 x 4, into the ring's next pinned slot: the caller's array is free when this call returns, and the copy is
    // ordered behind the frames ahead of it in the stream.  No hipStreamSynchronize: only a slot whose copy of four poses ago still runs waits
    PaletteSlot& slot = c->skin.ring[c->skin.ring_next];
    c->skin.ring_next = (c->skin.ring_next + 1u) % 4u;
    if (slot.in_flight) HIPC(c, hipEventSynchronize(slot.done));
    slot.in_flight = false;
    const size_t bytes = 48 * (size_t)s.n_joints;
    if (slot.cap < bytes) {
        if (slot.host) (void)hipHostFree(slot.host);
        slot.host = nullptr;
        slot.cap = 0;
        HIPC(c, hipHostMalloc((void**)&slot.host, bytes, hipHostMallocDefault));
        slot.cap = bytes;
    }
    if (!slot.done) HIPC(c, hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
    for (uint32_t i = 0; i < s.n_joints; i++) pack3x4(joint_matrices + 16 * (size_t)i, slot.host + 12 * (size_t)i);
    HIPC(c, hipMemcpyAsync(s.palette.get(), slot.host, bytes, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipEventRecord(slot.done, c->stream));
    slot.in_flight = true;
    if (s.flag_pending) HIPC(c, hipMemsetAsync(c->skin.d_flags.get() + skin, 0, 4, c->stream));  // (not pending: the word is known to be 0)
    L.rest = s.rest.get();
    L.joints = s.joints.get();
    L.weights = s.weights.get();
    L.palette = s.palette.get();
    L.dpos = s.dpos.get();
    L.dnrm = s.dnrm.get();
    L.out = reinterpret_cast<float4*>(c->scene.d_verts.get() + 8 * (size_t)s.first);
    L.flag = c->skin.d_flags.get() + skin;
    L.n = s.n;
    L.n_targets = s.n_targets;
    {
        ScopedTimer t(c, CAT_OTHER);
        launch_skin_pose(c->stream, L);
    }
    HIPC(c, hipGetLastError());
    s.flag_pending = true;
    c->scene.content_gen++;  // what rt3_scene_update_vertices does to the state
    mark_accel_stale(c);
    if (c->deform.snapshot) {
        add_dirty_range(c->deform.ranges, s.first, s.first + s.n);
        c->deform.dirty = true;
    }
    return RT3_OK;
}
int rt3_skin_info(rt3_ctx* c, uint32_t* n_skins, uint64_t* device_bytes) {
    if (!c) return fail(c, RT3_E_INVALID, "context NULL");
    uint64_t total = 0;
    for (const Skin& s : c->skin.list) total += s.bytes;
    if (n_skins) *n_skins = (uint32_t)c->skin.list.size();
    if (device_bytes) *device_bytes = total;
    return RT3_OK;
}
int rt3_scene_download_vertices(rt3_ctx* c, float* out, uint32_t first, uint32_t n) {
    if (!c || (!out && n)) return fail(c, RT3_E_INVALID, "download_vertices: NULL");
    if (!c->scene.d_verts) return fail(c, RT3_E_STATE, "download_vertices: no vertices (rt3_scene_set_vertices)");
    if ((uint64_t)first + n > c->scene.n_verts) return fail(c, RT3_E_INVALID, "download_vertices: [first, first + n) exceeds the vertex buffer");
    if (n == 0) return RT3_OK;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));  // a pose may still be writing
    HIPC(c, hipMemcpy(out, c->scene.d_verts.get() + 8 * (size_t)first, (size_t)n * 32, hipMemcpyDeviceToHost));
    return RT3_OK;
}

}  // extern "C"
