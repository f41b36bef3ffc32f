/*
 * rt3.h -- C ABI of librt3.so: the MI355X (gfx950) wavefront path tracer that stands in for the reference's
 * Vulkan ray-tracing passes.  Plain pointers and sizes only; every entry point cites the reference interface it
 * replaces (paths relative to DerEchteKarsten/RayTracer3).  INTEGRATION.md shows the Rust `extern "C"` block a
 * maintainer would add on the reference side.
 *
 * Conventions:
 *  - every call returns 0 on success or a negative RT3_E_* code; rt3_last_error() gives the text; nothing aborts or
 *    throws across the ABI (the reference `.unwrap()`s on its frame path, render_graph/mod.rs:601-610);
 *  - a context is NOT re-entrant: call it from one thread at a time (the reference's renderer systems are chained on
 *    the main thread, renderer/mod.rs:108-116); one context drives one GPU on one HIP stream (multi-GPU: one context
 *    and one process per GPU, joined only by rt3_gather_tiles);
 *  - host pointers are borrowed for the duration of the call and copied synchronously (like DynamicBuffer::push,
 *    vulkan/buffer.rs:406-420); device memory is owned by the context and released by rt3_destroy();
 *  - resource handles are u32 `tag << 30 | index` exactly like DescriptorResourceHandle (bindless/mod.rs:67-77):
 *    tag 0 = storage buffer, 1 = storage image, 3 = acceleration structure.
 */
#ifndef RT3_H
#define RT3_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT3_OK 0
#define RT3_E_INVALID (-1)     /* bad argument / unknown pass / wrong binding count */
#define RT3_E_HIP (-2)         /* a HIP runtime call failed (text in rt3_last_error) */
#define RT3_E_NO_DEVICE (-3)   /* no gfx950 device visible */
#define RT3_E_STATE (-4)       /* call order (e.g. pass launched before rt3_accel_build) */
#define RT3_E_UNSUPPORTED (-5) /* a feature this build does not implement */
#define RT3_E_DEPTH (-6)       /* BVH deeper than the traversal stack supports */
#define RT3_E_COMM (-7)        /* an RCCL call of the frame-end gather failed (text in rt3_last_error) */

#define RT3_INVALID_HANDLE 0xFFFFFFFFu
#define RT3_TAG_BUFFER 0u
#define RT3_TAG_IMAGE 1u
#define RT3_TAG_ACCEL 3u
#define RT3_MISS 0xFFFFFFFFu
#define RT3_BACKGROUND_DEPTH 100000.0f /* shaders/include/datatypes.slang:3 */

/* image formats (subset of the vk::Format values the reference passes use) */
#define RT3_FORMAT_R32_SFLOAT 100u          /* depth / gbuffer_depth (renderer/mod.rs:80, gbuffer.slang:6) */
#define RT3_FORMAT_R32G32B32A32_SFLOAT 109u /* Light / PrevLight / color (refrence_mode.slang:10-11) */
#define RT3_FORMAT_R32G32B32A32_UINT 107u   /* packed G-buffer (gbuffer.slang:5) */
#define RT3_FORMAT_R8G8B8A8_UNORM 37u       /* display image */
#define RT3_FORMAT_R16_UINT 74u             /* probe ray directions (trace_probes.slang:10, structured_importance_sampling.slang:10) */

/* feature flags carried in GConst.pad[0]; 0 = the reference's estimator (diffuse BSDF, emissive-only transport, 2 random draws
 * per bounce, refrence_mode.slang:36-57) with ONE documented difference: the reference advances its RNG counter sequentially
 * (random.slang:49-79), a wavefront needs a closed form and uses counter = (sample * bounces + bounce) * 2 + dim -- the same
 * numbers whenever no path of the pixel ends early (a closed box), other samples of the same distribution otherwise
 * (DESIGN.md section 4 item 1).  The other flags are north_star additions. */
#define RT3_F_NEE_SKY 1u     /* next-event estimation + MIS against the equirect sky */
#define RT3_F_BLUENOISE 2u   /* Cranley-Patterson shift by resources/bluenoise.png */
#define RT3_F_SPECULAR 4u    /* layered BSDF: DiffuseBrdf under the GGX SpecularBrdf of brdf.slang:141-311 */
#define RT3_F_FACEFORWARD 8u /* flip the shading normal towards the incoming ray */
#define RT3_F_PROBE_RADIANCE 16u /* trace_probes: store lerp(prev, radiance, blendfactor) per ray, the store its line 74 keeps in a comment */
/* next-event estimation + MIS to emissive triangles.  The same integral as the frame without the flag: at every vertex
 * b <= B-2 one emitter is picked with probability p_sel ~ area x luminance(12 emission) (an integer CDF on the 2^-23 grid of the RNG: RNG dims
 * 5, 6, 7, no blue-noise shift), a point on it uniformly; its emission (two-sided) is added with the balance weight p_solid / (p_solid + p_bsdf)
 * behind a shadow ray that ends just short of the point.  A BSDF-sampled ray that hits an emitter at a vertex >= 1 adds its emission with
 * weight p_bsdf / (p_bsdf + p_solid).  No emitter NEE at the last vertex, so with B = 1 (or a scene without emission) nothing changes.  Only
 * refrence_mode reads the bit; the emitter table follows every rt3_accel_build / refit / import (rt3_light_info). */
#define RT3_F_NEE_EMISSIVE 32u
/* next-event estimation to the punctual lights of rt3_scene_set_lights (the block comment at rt3_scene_set_lights states
 * the estimator).  Only refrence_mode reads the bit.  Without lights, or with B = 1, the frame is the one without the bit, bit for bit, from the
 * same kernels: the bit is dropped from the flag word such a frame runs with, so RT3_F_NEE_PUNCTUAL alone is then flags = 0. */
#define RT3_F_NEE_PUNCTUAL 64u

/* src/renderer/mod.rs:47-63 == shaders/include/datatypes.slang:28-43.  304 bytes, 16-byte aligned, column-major
 * matrices.  Offsets 0,64,128,192,256,264,268,272,276,280,284,288,296. */
typedef struct rt3_gconst {
    float proj[16];
    float view[16];
    float proj_inverse[16];
    float view_inverse[16];
    float window_size[2];
    uint32_t frame;
    float blendfactor;
    uint32_t bounces;
    uint32_t samples;
    uint32_t proberng;
    float cell_size;
    uint32_t mouse[2];
    uint32_t pad[2]; /* pad[0] = RT3_F_* flags, pad[1] reserved (0) */
} rt3_gconst;

/* shaders/include/datatypes.slang:11-19 (52 bytes of fields, padded to 64 for float4 alignment) */
typedef struct rt3_geometry_info {
    float base_color[4];
    int32_t base_color_texture_index; /* -1 = none, else an index set with rt3_scene_set_texture (hit_logic.slang:31-33) */
    float metallic_factor;
    uint32_t index_offset;
    uint32_t vertex_offset;
    float emission[4];
    float roughness;
    uint32_t _pad[3];
} rt3_geometry_info;

/* One placed mesh of the world: `Instance{model}` + `Transform{Mat4}` of an entity (src/renderer/world/mod.rs:46-60), the rows
 * `InstanceInfo{mesh_index, transform}` of the global instance / transform buffers (world/mod.rs:34-38,104-125).  A mesh here is
 * a run of geometries [geometry_first, geometry_first + geometry_count) of rt3_scene_set_geometry; `transform` is column-major
 * like glam's Mat4 (object -> world), last row (0, 0, 0, 1) -- the 3 x 4 a VkAccelerationStructureInstanceKHR can hold. */
typedef struct rt3_instance {
    uint32_t geometry_first, geometry_count;
    float transform[16];
} rt3_instance;

/* frame statistics (no reference equivalent: the reference has no counters) */
typedef struct rt3_stats {
    uint64_t extension_rays; /* closest-hit rays traced since rt3_stats_reset (primary + bounce) */
    uint64_t shadow_rays;    /* any-hit rays traced */
    uint64_t nodes_visited;  /* by k_extend; only when counting is enabled (RT3_OPT_COUNT_TRAVERSAL) */
    uint64_t tris_tested;
    uint64_t shadow_nodes_visited; /* by k_shadow */
    uint64_t shadow_tris_tested;
    uint64_t extend_launches; /* k_extend launches */
    double extend_ms;         /* sum of HIP-event durations of k_extend launches (RT3_OPT_PROFILE) */
    uint64_t shadow_launches;
    double shadow_ms;
    double shade_ms;
    double other_ms;
    /* always 0 since the fused traversal launch (k_trace, option 10) was retired; kept so that the layout stays put */
    uint64_t trace_launches;
    double trace_ms;
    uint64_t trace_rays[2];
    uint64_t trace_nodes[2];
    uint64_t trace_tris[2];
    double gather_ms; /* RCCL send / grouped receives of rt3_gather_tiles (the pack / untile kernels are in other_ms) */
    uint64_t nodes_visited_lds;        /* of nodes_visited: served by the traversal kernels' LDS copy of the top of the tree, i.e. NOT */
    uint64_t shadow_nodes_visited_lds; /* requested from the vector-memory path (counting mode; default node layout only) */
    double accel_build_ms;       /* host wall clock of the last rt3_accel_build, stream synchronised on both sides */
    uint64_t accel_bulk_copies;  /* host <-> device copies of array size (> 64 KiB) made by rt3_accel_build calls since rt3_stats_reset:
                                    the build stays on the GPU, so only geometry tables over 64 KiB (many placements) count */
    uint64_t accel_arena_serial; /* which device allocation the structure's arena (node array + triangle records, what the traversal kernels
                                    address from one base) is: a process-wide serial number taken where an arena is allocated, 0 = no
                                    arena (empty scene).  It changes whenever the structure moves to a new allocation (a build that makes
                                    new trees, rt3_accel_import) and stays when it is rewritten in place (rt3_accel_refit). */
    uint64_t emit_tex_launches;  /* k_emit_tex launches (rt3_scene_set_textured_emitters) since rt3_stats_reset: 0 for every frame whose light
                                    table holds no textured emitter */
} rt3_stats;

typedef struct rt3_ctx rt3_ctx;

/* ---- context: Context::new + RayTracingContext::new + BindlessDescriptorHeap::new + RenderGraph::new
 *      (renderer/mod.rs:32-45, vulkan/mod.rs:86-231) -> hipSetDevice + one stream ---- */
int rt3_create(int device, rt3_ctx **out);
void rt3_destroy(rt3_ctx *ctx);
const char *rt3_last_error(rt3_ctx *ctx); /* ctx may be NULL: last creation error */
int rt3_device_name(rt3_ctx *ctx, char *buf, size_t buf_size);

#define RT3_OPT_BATCH_SPP 1       /* samples per wavefront batch (0 = auto) */
#define RT3_OPT_PROFILE 2         /* 1: bracket kernels with HIP events on the context's stream */
#define RT3_OPT_COUNT_TRAVERSAL 3 /* 1: k_extend/k_shadow also count nodes / triangles (slower; for roofline bytes) */
#define RT3_OPT_EXTEND_VARIANT 4  /* traversal tuning: idle lanes of a wave before it refills them from its ray pool (default 12) */
#define RT3_OPT_LEAF_SIZE 5       /* 1..8 triangles per BVH leaf (default 2); takes effect at the next rt3_accel_build */
#define RT3_OPT_NODE_WIDTH 6      /* 2 = binary nodes, 4 = four-wide nodes (default); next rt3_accel_build */
#define RT3_OPT_NODE_QUANT 7      /* width 4 only: 1 = 64 B nodes with 8-bit conservative child boxes (default), 0 = 128 B fp32 boxes, 2 = compact 48 B nodes (implied references) */
#define RT3_OPT_WIDE_COLLAPSE 8   /* width 4 only: how the binary tree becomes four-wide nodes: 2 = cost-driven (default since round 3: a bottom-up SAH dynamic
                                     programme also decides which subtrees become multi-triangle leaves; triangle records in tree order), 1 = greedy by surface
                                     area, 0 = even binary depth */
#define RT3_OPT_POOL_CHUNK 9      /* traversal tuning: rays a wave takes from the launch's ray pool per grab (default 256) */
/* 10: retired (was RT3_OPT_FUSED_TRACE, one k_trace launch per bounce for both ray queues; measured slower); not reused */
#define RT3_OPT_SAH_TOP 11       /* T > 0 (default 1 = binned SAH down to single triangles; collapse 0 / 1 use max(T, leaf size)): the tree above Karras subtrees of at most T triangles is re-linked by binned SAH
                                     (the reference asks its driver for PREFER_FAST_TRACE builds, raytracing.rs:103,131); 0 = plain LBVH */
#define RT3_OPT_TRACE_BLOCKS 12   /* traversal tuning: persistent workgroups (256 threads) per traversal launch (default 2048 = 8 per CU) */
/* 13: retired (was RT3_OPT_SAH_TOP_DEVICE, the host build of the SAH top); not reused */
#define RT3_OPT_INSTANCE_MODE 14  /* how rt3_accel_build treats instances: 0 = flatten (default), 1 = two-level (shared bottom trees under a top tree; default node
                                     layout only).  See the instances block below; next rt3_accel_build */
#define RT3_OPT_SHADOW_EXIT_TABLE 15 /* k_shadow's exit table (single-level structures of the default node layout): 1 = a shadow ray first tries the leaf
                                     recorded for the cell where it leaves the scene box (default), 0 = off, 2 = on with pseudo-random valid entries (a test aid:
                                     no result depends on the table's contents).  Takes effect at once; see rt3_accel_exit_table_info */
#define RT3_OPT_DEFER_SKY_LIGHT 16 /* sky next-event estimation of refrence_mode and adaptive: 1 = a light sample is evaluated (radiance texels, BSDF, weight)
                                     only once its shadow ray came through unoccluded, in a kernel of its own (default); 0 = before the ray is
                                     traced.  Same frame bit for bit.  Scenes with glass, punctual lights or material textures, and skies whose
                                     smallest texel density is below 2^-100, take the path of 0 whatever the option says.  Takes effect at once */
#define RT3_OPT_SHADE_EXIT_TEST 17 /* deferred sky light samples in a structure with an exit table: 1 = the shade kernel tries a sky shadow ray against the
                                     leaf of its exit-table entry itself and queues only the rays that leaf does not occlude (default); 0 = every
                                     ray is queued and k_shadow tries the entry.  Same frame and the same rt3_stats ray counts, bit for bit.
                                     Frames with emitter or punctual sampling, alpha masks, panes, a two-level structure, RT3_OPT_COUNT_TRAVERSAL
                                     or without deferral take the path of 0 whatever the option says.  Takes effect at once */
int rt3_set_option(rt3_ctx *ctx, int option, int64_t value);

/* ---- scene upload: DynamicBuffer::push (vulkan/buffer.rs:406-420) into the world buffers of
 *      world/mod.rs:103-125 (vertex / index / geometry), plus the two north_star inputs ---- */
int rt3_scene_set_vertices(rt3_ctx *ctx, const float *interleaved_p_n_t, uint32_t n_vertices); /* Vertex, assets/mod.rs:127-133 */
int rt3_scene_set_indices(rt3_ctx *ctx, const uint32_t *indices, uint32_t n_indices);
int rt3_scene_set_geometry(rt3_ctx *ctx, const rt3_geometry_info *infos, const uint32_t *prim_counts, uint32_t n);
/* equirect sky (main.rs:94, the commented skybox2.exr): finite, non-negative radiance.  Stored as RGB9E5 (packing.slang:99-162, the
 * format the reference's G-buffer keeps emissive in; values above 65408 clamp): every sky lookup reads the de-quantised texel */
int rt3_scene_set_sky(rt3_ctx *ctx, const float *rgb, uint32_t width, uint32_t height);
int rt3_scene_set_bluenoise(rt3_ctx *ctx, const uint8_t *rgba, uint32_t width, uint32_t height); /* resources/bluenoise.png */
/* base-colour texture `index` (dense indices 0..n-1): RGBA8 with sRGB-encoded colour, sampled bilinearly with repeat
 * addressing at mip 0 like Textures[i].SampleLevel(uvs, 0.0) (hit_logic.slang:31-33; bindless set 2, bindless/mod.rs:38-77) */
int rt3_scene_set_texture(rt3_ctx *ctx, uint32_t index, const uint8_t *rgba_srgb, uint32_t width, uint32_t height);
/* ---- alpha-masked cutout geometry: glTF alphaMode MASK (foliage, chains, fences).  No reference counterpart: the reference builds its
 *      acceleration structures opaque (hit_logic.slang).  DESIGN.md section 4e.  One cutoff c per geometry of the last
 *      rt3_scene_set_geometry (n = that count), or n = 0: all opaque.  c = 0 (the default, and what rt3_scene_set_geometry resets every
 *      geometry to) is opaque, today's behaviour; 0 < c <= 1 masks the geometry: one of its ray-triangle intersections counts only if
 *      alpha >= c, alpha = base_color[3] * tex_alpha(u, v) in fp32, where tex_alpha is the bilinear alpha of the base-colour texture at mip 0
 *      with repeat addressing (texture_sample's texel coordinates and weights; the byte times 1 / 255, linear) and 1 without a texture, at
 *      the uv that hit_finish interpolates with the candidate's barycentrics.  Hits are defined as sets: the closest hit is the minimum over
 *      (t, prim) of the intersections in (tmin, tmax) that count, an any hit "some intersection counts" -- for every ray the library traces
 *      (passes, rt3_trace_rays, both instance modes).  Shading is unchanged.  Masked geometries are left out of the emitter table of
 *      RT3_F_NEE_EMISSIVE (their emission still counts, with weight 1, where a BSDF-sampled ray hits them).
 *      A value that is not finite or not in [0, 1], or a wrong n, is RT3_E_INVALID and changes nothing.  The cutoffs take effect at the next
 *      rt3_accel_build; setting them leaves an existing structure unusable like a geometry change (rt3_pass_launch, rt3_trace_rays and
 *      rt3_accel_download return RT3_E_STATE, rt3_accel_refit RT3_E_STATE) until rt3_accel_build.  A masked geometry needs the default node
 *      layout (else RT3_E_UNSUPPORTED at build); rt3_accel_import is RT3_E_UNSUPPORTED while any cutoff is > 0.  Borrowed for the call. ---- */
int rt3_scene_set_alpha_cutoffs(rt3_ctx *ctx, const float *cutoffs, uint32_t n);
/* ---- material textures: glTF pbrMetallicRoughness.metallicRoughnessTexture, normalTexture and emissiveTexture.  No reference counterpart
 *      (hit_logic.slang:31-33 samples base colour only).  DESIGN.md section 4j.  One entry per geometry of the last rt3_scene_set_geometry
 *      (n = that count), or n = 0: none, which is also what rt3_scene_set_geometry resets every geometry to.  The indices name textures of
 *      the one pool of rt3_scene_set_texture (RGBA8); the slot that names a texture decides how its bytes are decoded.  -1, or an index at or
 *      above the number of uploaded textures, is "no texture" (as for base_color_texture_index).  All three lookups happen at the uv that
 *      hit_finish interpolates, with texture_sample's texel coordinates, repeat addressing and weights (fx, fy) at mip 0, and blend as
 *      lerp(a, b, f) = a + (b - a) * f, along x first, then along y -- so a constant texture returns its value exactly:
 *       - roughness = roughness_factor * G, metalness = metallic_factor * B, a byte decoded as (float)byte * (1.0f / 255.0f) (linear);
 *       - emissive = (emission * 12) * rgb, rgb decoded by the sRGB table of the base-colour lookup.  A geometry that names an emissive
 *         texture (index >= 0) is left out of the emitter table of RT3_F_NEE_EMISSIVE like a masked one: its emission counts with weight 1
 *         where a BSDF-sampled ray hits it;
 *       - normal map: every flattened primitive gets a tangent at build and at refit, from its object-space positions p and uvs:
 *         e1 = p1 - p0, e2 = p2 - p0, det = du1 dv2 - du2 dv1, T = normalise(e1 dv2 - e2 dv1) * sign(det), handedness
 *         h = sign(det) * sign(dot(cross(e1, e2), n0 + n1 + n2)) (a zero dot counts as positive); det == 0 or a T that is not finite: the
 *         primitive has no tangent.  T is stored octahedrally, 2 x 15 bits.  At a hit, with n the normalised blend of the vertex normals in
 *         object space: t = normalise(T - n dot(n, T)), b = h cross(n, t), c = 2 lerp(byte / 255) - 1 per channel,
 *         n' = normalise((s c.x) t + (s c.y) b + c.z n), s = normal_scale; n' replaces n ahead of the instance matrix.  n stays when the
 *         primitive has no tangent or when T - n dot(n, T) or the combined vector is zero or not finite.  Per-triangle tangents (no TANGENT
 *         accessor, no MikkTSpace) are the documented deviation; a mapped normal that faces away from the ray is treated as an interpolated
 *         one is.
 *      G-buffer packing, face-forward, the BSDF, the alpha test and the motion, temporal and denoise passes are unchanged.  Works in both
 *      instance modes and after rt3_accel_import.  A normal_scale that is not finite, an index below -1 or a wrong n is RT3_E_INVALID and
 *      changes nothing.  Takes effect at the next rt3_accel_build; until then an existing structure is unusable, as after
 *      rt3_scene_set_alpha_cutoffs.  Borrowed for the call. ---- */
typedef struct rt3_material_textures {
    int32_t metallic_roughness_texture; /* -1 = none; glTF channels: G = roughness, B = metalness, linear */
    int32_t normal_texture;             /* -1 = none; tangent-space normal map, linear */
    int32_t emissive_texture;           /* -1 = none; sRGB-encoded colour */
    float   normal_scale;               /* glTF normalTexture.scale */
} rt3_material_textures;                /* 16 bytes */
int rt3_scene_set_material_textures(rt3_ctx *ctx, const rt3_material_textures *m, uint32_t n);
/* ---- glass: transmissive dielectric surfaces, solid and thin-walled (glTF KHR_materials_transmission, _ior, _volume).  No reference
 *      counterpart.  DESIGN.md section 4n.  One entry per geometry of the last rt3_scene_set_geometry (n = that count), or n = 0: no glass,
 *      which is also what rt3_scene_set_geometry resets every geometry to.
 *       - Lobe selection: a path vertex on a geometry with transmission t > 0 is a glass vertex with probability t, decided by the draw at
 *         RNG index 0x40000000 + 2 (s B + b) of the pixel's stream (s the absolute sample index, b the bounce, B = GConst.bounces; no draw
 *         at t = 1, no blue-noise shift): glass when u < t.  Otherwise the vertex is shaded as without this call, from the same draws.
 *       - The glass vertex is a smooth, delta dielectric.  n: the shading normal, not face-forwarded (RT3_F_FACEFORWARD and RT3_F_SPECULAR
 *         do not affect it); d: the ray direction, normalised.  The ray enters when dot(n, d) < 0: eta = ior, else 1 / ior (every
 *         interface is air <-> ior; nested media are not modelled).  cos_i = |n.d|, cos_t^2 = 1 - (1 - cos_i^2) / eta^2; cos_t^2 <= 0:
 *         total internal reflection, F = 1; else F = (r_s^2 + r_p^2) / 2, r_s = (cos_i - eta cos_t) / (cos_i + eta cos_t),
 *         r_p = (eta cos_i - cos_t) / (eta cos_i + cos_t) (exact Fresnel).  thin_walled: eta = ior on both sides and
 *         F' = 2 F / (1 + F), the sum of a slab's inter-reflections; the transmitted direction is d.  The draw at index + 1 picks the
 *         event: u < F mirrors d about n, throughput unchanged; else transmission along d / eta + (cos_i / eta - cos_t) n' (n' the normal
 *         on the incoming side), throughput x albedo (base colour x base-colour texture).  Emission is collected as at any vertex.
 *       - A glass vertex takes no light sample (no sky, emitter or punctual shadow ray); what its extension ray finds counts with weight
 *         1 (an emitter under RT3_F_NEE_EMISSIVE, the sky under RT3_F_NEE_SKY).  At the last vertex (b = B - 1) under RT3_F_NEE_SKY the
 *         chosen direction goes out as the sky shadow ray, carrying throughput x the sky's bilinear radiance along it.
 *       - Without RT3_F_NEE_SKY a ray that escapes after nothing but glass vertices since the camera adds throughput x the sky's bilinear
 *         radiance, as an escaped camera ray of a lens frame does; after any other vertex it adds nothing, as without glass.
 *       - Shadow rays are unchanged: glass occludes them.  Light through glass arrives by BSDF-sampled paths only (unbiased for emitters
 *         and the sky); punctual lights do not shine through glass.  (rt3_scene_set_pane_shadows, below, changes this for thin-walled
 *         panes.)  Alpha cutoffs work independently on the same geometry.
 *       - The packed G-buffer has no room for a material class: in a built scene with glass "refrence_mode" needs per-sample camera rays
 *         (rt3_camera_set_lens; {0, f, 0} is the per-sample pinhole) and returns RT3_E_STATE without, as does "adaptive" ("adaptive" takes
 *         a lens only under rt3_adaptive_set_coverage); with samples * bounces * 8 > 2^30 either returns RT3_E_INVALID (the vertices' RNG indices would reach the glass draws').  "gbuffer",
 *         "denoise", "temporal", "motion", the probe passes and rt3_trace_rays see glass as the opaque surface its material describes.
 *      Works in both instance modes, after rt3_accel_import and across rt3_accel_refit.  A value that is not finite, a transmission outside
 *      [0, 1], ior < 1, thin_walled > 1, reserved != 0 or a wrong n is RT3_E_INVALID and changes nothing.  Takes effect at the next
 *      rt3_accel_build; until then an existing structure is unusable, as after rt3_scene_set_alpha_cutoffs.  Borrowed for the call. ---- */
typedef struct rt3_transmission {
    float    transmission; /* [0, 1]: the probability that a vertex on the geometry is a glass vertex */
    float    ior;          /* >= 1 */
    uint32_t thin_walled;  /* 0 = solid (refracts), 1 = thin-walled (a pane: passes straight through) */
    uint32_t reserved;     /* 0 */
} rt3_transmission;        /* 16 bytes */
int rt3_scene_set_transmission(rt3_ctx *ctx, const rt3_transmission *t, uint32_t n);
/* ---- pane shadows: light sampling through thin-walled glass.  No reference counterpart.  DESIGN.md section 4q.  A mode of the context, off
 *      by default, that survives rt3_scene_set_geometry.  A pane is a geometry with transmission > 0 that is thin_walled and names no
 *      normal texture; rt3_accel_build classifies.  With the mode on, in a built scene with at least one pane:
 *       - the shadow rays of "refrence_mode" (sky, last-vertex sky, emitter and punctual) are not occluded by a pane triangle they meet inside
 *         their range (after its alpha cutout test, if it has one); their contribution is multiplied by
 *         A = transmission (1 - F'(cos_i)) tint per crossing, cos_i = |n.d| / |d| with the interpolated shading normal n, F' = 2 F / (1 + F)
 *         at eta = ior, tint = base colour x base-colour texture: the expectation of what a glass vertex there does to a straight path;
 *       - a glass vertex on a pane that transmits hands the incoming pdf slot on unchanged (no delta marker), so that what the ray finds
 *         is weighted against the light samples of the vertex that chose the direction, with the emitter density taken over the whole
 *         distance back to that vertex; at the last vertex its sky ray carries that weight.  Reflection keeps the delta marker.
 *      Solid glass, and a thin-walled geometry with a normal texture, occlude as before.  "gbuffer", the probe passes and rt3_trace_rays
 *      see glass as opaque, as before.  A ray within the 2^-20 barycentric band of an edge shared by two pane triangles is attenuated twice.
 *      on other than 0 or 1 is RT3_E_INVALID and changes nothing.  A change takes effect at the next rt3_accel_build; until then an existing
 *      structure is unusable, as after rt3_scene_set_alpha_cutoffs; rt3_accel_refit keeps it.  With the mode on and a pane, rt3_accel_build
 *      needs the default node layout (either instance mode) and rt3_accel_import is refused: RT3_E_UNSUPPORTED.  With the mode on and no
 *      pane nothing differs from off.  rt3_pane_shadow_info: the flattened geometries with triangles that the built structure holds as
 *      panes, 0 while the mode is off; RT3_E_STATE before a build. ---- */
int rt3_scene_set_pane_shadows(rt3_ctx *ctx, int on);
int rt3_scene_get_pane_shadows(rt3_ctx *ctx, int *on);
int rt3_pane_shadow_info(rt3_ctx *ctx, uint32_t *n_panes);
/* ---- rough transmission: frosted glass, transmission through GGX microfacets.  No reference counterpart.  DESIGN.md section 4t.  A mode of
 *      the context, off by default, that survives rt3_scene_set_geometry.  A geometry is frosted when its transmission is > 0 and its material
 *      roughness factor is > 0 or it names a metallic-roughness texture, solid or thin-walled; rt3_accel_build classifies.  A frosted geometry is
 *      never a pane (rt3_scene_set_pane_shadows): shadow rays are occluded by it.  With the mode on, in a built scene with a frosted geometry,
 *      a glass vertex (selected as always) on such a geometry whose roughness alpha at the hit (factor x texture, as the opaque BSDF takes it:
 *      not squared, no floor) is > 0 follows this rule instead of the smooth one; alpha = 0 is the smooth vertex, bit for bit:
 *       - ud = d / |d|; enter = dot(n, ud) < 0 (n the shading normal, not face-forwarded); n_in = enter ? n : -n; wo = -ud in the tangent frame
 *         about n_in; wo.z <= 1e-5 ends the path.
 *       - m = the opaque BSDF's sample_vndf(alpha, wo, u2, u3): a GGX micro-normal visible from wo; u2, u3 are the draws at RNG indices
 *         0x50000000 + 2 (s B + b) + {0, 1} (no blue-noise shift).
 *       - cos_i = dot(wo, m); eta, cos_t^2, F and the thin-walled F' are the smooth vertex's expressions at this cos_i; the smooth vertex's
 *         event draw picks reflection when u < F.
 *       - reflection r = 2 cos_i m - wo, valid when r.z > 1e-5; solid transmission t = -wo / eta + (cos_i / eta - cos_t) m, valid when
 *         t.z < -1e-5; thin-walled transmission (r.x, r.y, -r.z), valid when r.z > 1e-5 (a thin rough slab as one lobe: an approximation).  An
 *         invalid sample ends the path: no extension ray, no last-vertex sky ray (single scattering: that energy is lost).
 *       - throughput x (tint when transmitted) x G1(|wi.z|, alpha^2), the separable Smith term left of f cos / pdf.
 *      Everything else is the glass vertex's: no light sample, the delta markers in the pdf slot, the last-vertex sky ray, emission.  So a
 *      frosted surface is lit by BSDF-sampled paths only and punctual lights never light it.
 *      on other than 0 or 1 is RT3_E_INVALID and changes nothing.  A change takes effect at the next rt3_accel_build; until then an existing
 *      structure is unusable; rt3_accel_refit and rt3_accel_import keep the classification (it lives in the glass side table).  Both instance
 *      modes.  With the mode on and no frosted geometry nothing differs from off.  rt3_rough_transmission_info: the flattened geometries with
 *      triangles that the built structure holds as frosted, 0 while the mode is off; RT3_E_STATE before a build. ---- */
int rt3_scene_set_rough_transmission(rt3_ctx *ctx, int on);
int rt3_scene_get_rough_transmission(rt3_ctx *ctx, int *on);
int rt3_rough_transmission_info(rt3_ctx *ctx, uint32_t *n_frosted);
/* ---- absorbing glass: Beer-Lambert attenuation inside solid dielectrics.  No reference counterpart.  DESIGN.md section 4s.  One entry per
 *      geometry of the last rt3_scene_set_geometry; n = 0: none, and rt3_scene_set_geometry resets every geometry to that.  sigma: the
 *      absorption coefficient per colour channel, per world-space unit of length (glTF KHR_materials_volume:
 *      sigma = -ln(attenuationColor) / attenuationDistance).  rt3_accel_build classifies a geometry as absorbing when its transmission is > 0,
 *      it is solid (thin_walled = 0) and some sigma is > 0, and keeps a table per flattened geometry only when some geometry is absorbing;
 *      a sigma on any other geometry is ignored.  With the table, "refrence_mode" and "adaptive" run a kernel of its own name (k_absorb)
 *      between the k_extend and the k_shade of every vertex b >= 1, which applies one rule to the closest hit {t, u, v, prim} of each
 *      extension ray {o, d}: a path segment is inside an absorbing solid when it ARRIVES AT A BACK FACE of it.
 *        n = the interpolated vertex normal of the hit as a geometry without a normal map gets it (through the geometry's matrix unless it
 *        is the identity; not face-forwarded; a normal map is deliberately ignored);
 *        if prim's geometry is absorbing and dot(n, d) > 0:  x = t sqrtf(dot(d, d));  T.c = T.c expf(-(sigma.c x)) per channel, in fp32, in
 *        this order.  A channel with sigma 0 keeps its bits (expf(-0) = 1).  The pdf slot, the ray and the hit are not touched; a miss, a
 *        front-face hit and a hit on any other geometry leave T bit for bit.
 *      So every internal segment counts, those between total internal reflections included; emission and light samples at the arrival
 *      vertex see the attenuated T; the per-crossing albedo tint of rt3_scene_set_transmission stays (glTF multiplies both).  Limits: media
 *      do not nest -- a segment belongs to the geometry whose back face ends it, so an opaque object embedded in glass ends the segment on
 *      its own front face and that segment is not attenuated; camera rays (vertex 0) are not attenuated: a camera inside a solid sees its
 *      first segment clear.  Shadow rays are unchanged: solid glass still occludes them.  Without an absorbing geometry in the built scene
 *      nothing is launched and every frame keeps its bits.
 *      Works in both instance modes, after rt3_accel_import and across rt3_accel_refit.  A sigma that is not finite or is negative,
 *      reserved != 0 or a wrong n is RT3_E_INVALID and changes nothing.  Takes effect at the next rt3_accel_build; until then an existing
 *      structure is unusable, as after rt3_scene_set_transmission.  Borrowed for the call.
 *      rt3_attenuation_info: the flattened geometries the built structure holds as absorbing (0: no table, no k_absorb); RT3_E_STATE
 *      before a build. ---- */
typedef struct rt3_attenuation {
    float    sigma[3];  /* >= 0, per world-space unit of length */
    uint32_t reserved;  /* 0 */
} rt3_attenuation;      /* 16 bytes */
int rt3_scene_set_attenuation(rt3_ctx *ctx, const rt3_attenuation *a, uint32_t n);
int rt3_attenuation_info(rt3_ctx *ctx, uint32_t *n_absorbing);

/* ---- instances: the reference's world is a list of placed meshes (add_instance / loaded_assets, world/mod.rs:50-101) under a
 *      top-level acceleration structure (create_acceleration_structure(.., level, ..), vulkan/raytracing.rs:88-148), and hit_info
 *      turns the shading normal by the instance matrix (hit_logic.slang:23).  Here: n = 0 (the default) places every geometry once
 *      under the identity.  Otherwise instance i places geometries [first, first + count) under its matrix; the same geometry may be
 *      placed many times.  Both instance modes (RT3_OPT_INSTANCE_MODE) give the same hits, bit for bit:
 *       - 0, flatten (default): rt3_accel_build FLATTENS the instances into world-space triangles (p' = ((x_axis x + y_axis y) + z_axis z)
 *         + w_axis in fp32, glam's transform_point3; identity matrices leave positions untouched) and builds one tree over them -- ~3 ms
 *         for 260 k triangles on the GPU, so re-building after an instance moved IS the TLAS update (rt3_stats.accel_build_ms);
 *       - 1, two-level: one bottom tree per distinct run (first, count), built in object space and shared by its placements, under a
 *         top tree over the instances' world boxes.  Triangles are still tested in world space, transformed by the same expression,
 *         so t, u, v and primitive ids equal mode 0's; only the box tests see an object-space ray (with conservatively widened boxes).
 *         A rebuild after only matrices changed rebuilds the instance records and the top tree, not the meshes (rt3_accel_levels).
 *         Needs the default node layout (else RT3_E_UNSUPPORTED at build) and an invertible, not too badly conditioned upper 3 x 3
 *         (else RT3_E_UNSUPPORTED at build); rt3_accel_download / rt3_accel_import are RT3_E_UNSUPPORTED.
 *      Primitive ids reported by hits (gbuffer, rt3_trace_rays) count through the placed geometries in instance order.  Normals:
 *      normalize(M3 * normalize(interpolated)), M3 = upper 3 x 3, as hit_logic.slang:22-23 writes it (no inverse transpose).  Call
 *      before rt3_accel_build; borrowed for the call. ---- */
int rt3_scene_set_instances(rt3_ctx *ctx, const rt3_instance *instances, uint32_t n);
/* The previous frame's object -> world matrices (n x 16 floats, column-major), one per instance of the current rt3_scene_set_instances
 * list, in its order: what the "motion" pass (below) compares the built structure's matrices with.  Validated like an instance's matrix
 * (finite, last row (0, 0, 0, 1)); a bad matrix returns RT3_E_INVALID and changes nothing.  (NULL, 0) forgets them: every instance counts
 * as unmoved.  The acceleration structure does not become stale and no build reads the matrices.  n is checked when "motion" is launched:
 * it must be the instance count of the built structure (1 when no instances were set) or 0, else RT3_E_STATE.  Borrowed for the call; the
 * device table (64 B per instance) is uploaded when the matrices or the structure changed. */
int rt3_scene_set_prev_transforms(rt3_ctx *ctx, const float *transforms /* n x 16, column-major */, uint32_t n);
/* ---- punctual lights (glTF KHR_lights_punctual): point, spot and directional lights, sampled by next-event estimation under
 *      RT3_F_NEE_PUNCTUAL.  DESIGN.md section 4k.
 *      A light is 64 bytes, in world space.  `intensity` is colour x intensity in W/sr (point, spot) or W/m^2 (directional): no 683 lm/W and
 *      no x12 is applied.  `direction` is the way the light shines and need not be of unit length (it is normalised on the device).
 *      range <= 0 means unlimited (glTF: undefined).
 *      rt3_scene_set_lights replaces the list; (NULL, 0) forgets it.  RT3_E_INVALID, with nothing changed, for an unknown type, a value that
 *      is not finite, a negative intensity component, a zero direction on a spot or directional light, or cone angles outside
 *      0 <= inner < outer <= pi/2.  Borrowed for the call.  The acceleration structure does not become stale and no build reads the lights;
 *      only the light table is remade before the next frame that samples it.  rt3_scene_set_geometry does not reset the lights: they belong
 *      to the world, not to a mesh.  rt3_light_info / rt3_light_download keep reporting the emitter triangles alone.
 *      The estimator: a light is a path vertex.  With the flag, a non-empty list and B > 1, every vertex b <= B-2 picks ONE entry of the
 *      light table with the draw of RNG dim 5 (the rule and the dim of RT3_F_NEE_EMISSIVE).  The table holds
 *        RT3_F_NEE_PUNCTUAL alone         : the punctual lights (emission keeps weight 1 where a BSDF-sampled ray hits it)
 *        with RT3_F_NEE_EMISSIVE          : the emitter triangles followed by the punctual lights, under one CDF
 *        RT3_F_NEE_EMISSIVE alone         : the emitter table as without this call, bit for bit
 *      and is remade when the combination changes.  Selection masses are in the emitters' unit, power / pi: a triangle has
 *      area x luminance(12 emission), a point or spot light 4 luminance(I) (the cone is ignored), a directional light luminance(E) R^2 with R
 *      half the diagonal of the box of the built world's triangles (the box every root box encloses: the same in both instance modes and
 *      every node layout; 0 for a world without triangles).  A light of zero mass is never sampled; p_sel is the realised mass / 2^23.
 *      At the vertex x with shading normal N (after face-forward), BSDF f (albedo / pi, or the layered BSDF under RT3_F_SPECULAR) and
 *      throughput T:
 *        point / spot : wv = P - x, d^2 = wv.wv, wl = wv / d, cs = N.wl; nothing unless d^2 > 0 and cs > 0.  I' = I cone window, cone = 1 for a
 *                       point light and c^2 for a spot, c = clamp((-wl.axis) a + o, 0, 1), a = 1 / max(0.001, cos inner - cos outer),
 *                       o = -cos outer a (glTF's recommended form); window = clamp(1 - (d / range)^4, 0, 1) when range > 0, else 1.
 *                       contribution = T f cs I' / (d^2 p_sel) behind a shadow ray (x, wl) that ends at d (1 - 2^-10).
 *        directional  : wl = -axis, contribution = T f cs E / p_sel behind a shadow ray to RT3_BACKGROUND_DEPTH.
 *      There is no MIS weight (a BSDF-sampled ray never hits a delta light); a zero contribution emits no shadow ray.
 *      rt3_light_masses: the selection masses, in CDF units, of the table that flags & (RT3_F_NEE_EMISSIVE | RT3_F_NEE_PUNCTUAL) samples:
 *      *n_emitters entries for the emitter triangles, then *n_punctual for the lights in call order (both 0 when the combination samples
 *      nothing); `mass` may be NULL, else it holds n_emitters + n_punctual words.  RT3_E_STATE where rt3_light_info returns it. ---- */
#define RT3_LIGHT_POINT 0u
#define RT3_LIGHT_SPOT 1u
#define RT3_LIGHT_DIRECTIONAL 2u
typedef struct rt3_punctual_light {
    uint32_t type;
    float range;                  /* <= 0: unlimited */
    float inner_cone, outer_cone; /* radians, spot only: 0 <= inner < outer <= pi/2 */
    float position[3];            /* point, spot */
    float _pad0;
    float direction[3];           /* spot, directional */
    float _pad1;
    float intensity[3];           /* colour x intensity */
    float _pad2;
} rt3_punctual_light;
int rt3_scene_set_lights(rt3_ctx *ctx, const rt3_punctual_light *lights, uint32_t n);
int rt3_light_masses(rt3_ctx *ctx, uint32_t flags, uint32_t *n_emitters, uint32_t *n_punctual, uint32_t *mass);
/* ---- previous vertex positions: what lets the "motion" pass (below) follow a mesh that rt3_scene_update_vertices deforms (skinning, cloth,
 *      morph targets).  DESIGN.md section 4i.
 *      rt3_scene_snapshot_vertices: the positions the vertex buffer holds now become "the previous frame's".  A device-side copy on the
 *      context's stream into a buffer of the context, one 16-byte record {x, y, z, 0} per vertex; the first snapshot copies every vertex, a
 *      later one only the ranges rt3_scene_update_vertices touched since the snapshot before it.  Call it before the frame's updates.
 *      RT3_E_STATE before rt3_scene_set_vertices.  The acceleration structure does not become stale; no build or refit reads the snapshot.
 *      rt3_scene_forget_prev_vertices: no previous positions; "motion" is what it is without them.  rt3_scene_set_vertices,
 *      rt3_scene_set_indices and rt3_scene_set_geometry forget them too (with another topology the previous hit point means nothing).
 *      Which geometries are deformed is defined by the data, not by the calls made: geometry g is deformed when some vertex of its span
 *      [vertex_offset + least index, vertex_offset + largest index] (over its triangles) differs from the snapshot in one of its three
 *      position words, compared as uint32 (-0 is not +0, as for matrices).  Normal and uv words do not count, so neither does sending the
 *      same positions again.  A vertex inside the span that no triangle of the geometry indexes still counts.  The flags are computed on
 *      the device when "motion" is launched (or here) after a snapshot, an update or a forget, over the updated ranges only.
 *      rt3_scene_deformed_geometries: introspection for tests, one byte (0 / 1) per geometry of rt3_scene_set_geometry.  RT3_E_STATE without
 *      a snapshot, RT3_E_INVALID when n is not the geometry count. ---- */
int rt3_scene_snapshot_vertices(rt3_ctx *ctx);
int rt3_scene_forget_prev_vertices(rt3_ctx *ctx);
int rt3_scene_deformed_geometries(rt3_ctx *ctx, uint8_t *flags, uint32_t n);

/* ---- acceleration structure: create_acceleration_structure (vulkan/raytracing.rs:88-148) -> GPU LBVH.
 *      Returns the handle (tag 3) in *out_handle, like the TLAS registered at bindless/mod.rs:314-337 ---- */
int rt3_accel_build(rt3_ctx *ctx, uint32_t *out_handle);
/* introspection for parity tests: copy the BVH to the host (nodes: n_nodes x node_bytes (64 | 128), tris: n_tris x 48 B) */
int rt3_accel_info(rt3_ctx *ctx, uint32_t *n_nodes, uint32_t *n_tris, uint32_t *max_depth, uint32_t *node_bytes);
int rt3_accel_download(rt3_ctx *ctx, void *nodes, size_t nodes_bytes, void *tris, size_t tris_bytes);
/* the levels of the last rt3_accel_build (any pointer may be NULL): distinct bottom trees, how many of them that build (re)built (the rest
 * were reused), nodes of the top tree, and the device bytes the traversal kernels read (nodes, triangle records, top tree, instance
 * records; not the shading tables).  Instance mode 0 reports 0, 0, 0 and the flattened tree's bytes.  In mode 1 rt3_accel_info gives the
 * summed node and triangle counts of both levels and the combined depth. */
int rt3_accel_levels(rt3_ctx *ctx, uint32_t *n_meshes, uint32_t *n_meshes_built, uint32_t *n_top_nodes, uint64_t *accel_bytes);
/* k_shadow's exit table (RT3_OPT_SHADOW_EXIT_TABLE; any pointer may be NULL): its entries (0 = none: option 0, two-level mode, another node
 * layout, an empty scene), the shadow rays that started at an entry and those an entry occluded since the last build / import / refit /
 * rt3_scene_set_sky, and whether the next launch starts every ray at its entry (1) or only every 32nd chunk of rays (0: fewer than a
 * quarter of more than 2^16 tries succeeded). */
int rt3_accel_exit_table_info(rt3_ctx *ctx, uint32_t *cells, uint64_t *tried, uint64_t *occluded, uint32_t *in_use);
/* the way back: install a tree built elsewhere over the same (flattened) triangles -- a better offline builder, a cache of an earlier run
 * (what vkCmdCopyMemoryToAccelerationStructureKHR is to the reference's driver).  Default layout only (64-byte nodes, 48-byte triangle
 * records, rt3_accel_download's format); call rt3_accel_build first (it makes the shading records).  Every reference is validated on
 * the host (range, no node reachable twice, depth) before a kernel may follow it.  Triangle records may repeat a primitive (spatial
 * splits): the closest hit is decided by (t, prim), not by the record.  Used by tests/experiments/tree_quality_gpu.py. */
int rt3_accel_import(rt3_ctx *ctx, const void *nodes, size_t nodes_bytes, const void *tris, size_t tris_bytes);
/* ---- update after the vertices moved (what VK_BUILD_ACCELERATION_STRUCTURE_MODE_UPDATE_KHR is to the reference's driver, raytracing.rs:88-148):
 *      skinning, cloth, morph targets, an editor dragging vertices.  DESIGN.md section 4c. ---- */
/* overwrite vertices [first, first + n) in place (same 32-byte Vertex layout as rt3_scene_set_vertices); the index buffer, geometry and
 * instances are untouched.  Marks an existing acceleration structure stale: rt3_pass_launch / rt3_trace_rays / rt3_accel_download return
 * RT3_E_STATE until rt3_accel_refit or rt3_accel_build.  A range past the vertex buffer, or a position that is not finite (or beyond 1e18),
 * is RT3_E_INVALID and changes nothing; n = 0 is a no-op. */
int rt3_scene_update_vertices(rt3_ctx *ctx, const float *interleaved_p_n_t, uint32_t first, uint32_t n);
/* update of the last build: same nodes, same references, same triangle-record order; every box, every triangle record, the shading records
 * and the LDS top-of-tree copy recomputed from the current vertices (leaf pad and all from the new bounds).  Hits equal those of a fresh
 * build over the same vertices bit for bit (closest hits are decided by (t, prim), not by the tree); only traversal visits differ.
 * RT3_E_STATE without a structure, or when anything but vertex contents changed since rt3_accel_build (vertex count, indices, geometry,
 * instances, a tree option); RT3_E_UNSUPPORTED for any node layout but the default.  Works after rt3_accel_import and in both instance
 * modes (mode 1: every bottom tree, then the instance records and the top tree; rt3_accel_levels then reports 0 meshes built).  Does not
 * change rt3_stats.accel_build_ms. */
int rt3_accel_refit(rt3_ctx *ctx, uint32_t *out_handle);
/* ---- skins: skinned and morphed meshes posed on the device (glTF skins and morph targets).  No reference counterpart; DESIGN.md section 4z.
 *      A skin owns a range of the vertex buffer and keeps what a pose needs resident on the device: the rest records, four joint indices
 *      and weights per vertex, and up to RT3_SKIN_MAX_TARGETS morph targets (position deltas, optionally normal deltas).  A pose sends the
 *      joint palette and the target weights only; k_skin_pose writes the range's records:
 *        morph  for t = 0 .. n_targets-1 with a_t != 0: p.k = p.k + a_t * dP[t][v].k, and n with dN when the skin has normal deltas
 *        blend  M = the sum of w_k * J[j_k] over the weights w_k != 0, in the order k = 0, 1, 2, 3, entry by entry (a product, then a sum);
 *               a vertex whose four weights are 0 keeps its morphed p and n as they are
 *        place  p' = ((M.x_axis p.x + M.y_axis p.y) + M.z_axis p.z) + M.w_axis;  n' = normalize(M's upper 3 x 3 applied to n), no inverse
 *               transpose, as for an instance;  uv is the rest record's
 *      fp32, singly rounded, equal to tests/ref_skin.py bit for bit.
 *      rt3_scene_add_skin: RT3_E_INVALID, with nothing changed, for an empty range, one past the vertex buffer or one that overlaps another
 *      skin's; n_joints outside 1 .. 65536; n_targets above RT3_SKIN_MAX_TARGETS; joints or weights NULL; target_dpos NULL with targets or
 *      set without; a joint index >= n_joints (whatever its weight); a weight that is negative or not finite; a rest position that is not
 *      finite or beyond 1e18; a delta that is not finite.  RT3_E_STATE before rt3_scene_set_vertices.  It touches neither the vertex buffer
 *      nor the acceleration structure.  The arrays are tight and borrowed for the call.  *out_skin: the skin's index, counted from 0.
 *      rt3_scene_clear_skins forgets every skin, and so does rt3_scene_set_vertices (the buffer they index is gone); rt3_scene_set_indices and
 *      rt3_scene_set_geometry keep them.  rt3_scene_update_vertices on a skinned range is allowed: the next pose overwrites it.
 *      rt3_scene_pose_skin: n_joints matrices, column-major 4 x 4, validated like an instance's (finite, last row (0, 0, 0, 1)), and n_targets
 *      finite weights (NULL when the skin has none); otherwise RT3_E_INVALID and nothing changes.  The palette is uploaded and the kernel
 *      launched on the context's stream, behind the frames already in it, without waiting for them.  Like rt3_scene_update_vertices it marks
 *      the acceleration structure stale (rt3_accel_refit next) and, after a rt3_scene_snapshot_vertices, counts the range as updated.  A
 *      second pose overwrites the first.  Borrowed for the call.
 *      A posed position that is not finite or beyond 1e18 is still written, and sets the skin's flag on the device: the next rt3_accel_refit
 *      or rt3_accel_build returns RT3_E_INVALID ("skin s: a posed position ...") and the structure stays stale, until that skin is posed
 *      again, which clears the flag.
 *      rt3_skin_info: the number of skins and the device bytes they hold.  rt3_scene_download_vertices: introspection for tests, records
 *      [first, first + n) of the vertex buffer as they are on the device; it waits for the stream.  RT3_E_STATE before
 *      rt3_scene_set_vertices, RT3_E_INVALID for a range past the buffer. ---- */
#define RT3_SKIN_MAX_TARGETS 8u
typedef struct rt3_skin_desc {
    uint32_t first_vertex, n_vertices; /* the range of the vertex buffer this skin writes */
    uint32_t n_joints;                 /* 1 .. 65536 */
    uint32_t n_targets;                /* 0 .. RT3_SKIN_MAX_TARGETS */
    const float *rest;                 /* n_vertices x 8 (Vertex layout); NULL: the range's current contents, copied on the device */
    const uint16_t *joints;            /* n_vertices x 4 */
    const float *weights;              /* n_vertices x 4 */
    const float *target_dpos;          /* n_targets x n_vertices x 3; NULL iff n_targets == 0 */
    const float *target_dnrm;          /* same shape, or NULL: normals are not morphed */
} rt3_skin_desc;
int rt3_scene_add_skin(rt3_ctx *ctx, const rt3_skin_desc *desc, uint32_t *out_skin);
int rt3_scene_clear_skins(rt3_ctx *ctx);
int rt3_scene_pose_skin(rt3_ctx *ctx, uint32_t skin, const float *joint_matrices /* n_joints x 16, column-major */,
                        const float *target_weights /* n_targets, may be NULL when 0 */);
int rt3_skin_info(rt3_ctx *ctx, uint32_t *n_skins, uint64_t *device_bytes);
int rt3_scene_download_vertices(rt3_ctx *ctx, float *out /* n x 8 */, uint32_t first, uint32_t n);
/* the emitter table of RT3_F_NEE_EMISSIVE for the current structure, built on the GPU on first use after rt3_accel_build / refit / import:
 * every flattened primitive of a geometry with non-zero emission, in primitive order.  *cdf_total = 2^23 (the selection grid), or 0 when no
 * emitter has power (the flag then changes nothing).  rt3_light_download (any pointer may be NULL; n_emitters entries each): primitive ids,
 * world-space areas, selection masses in CDF units (p_sel = mass / cdf_total; mass 0 = never sampled).  Both RT3_E_STATE before a build and
 * while vertices are stale. */
int rt3_light_info(rt3_ctx *ctx, uint32_t *n_emitters, uint64_t *cdf_total);
int rt3_light_download(rt3_ctx *ctx, uint32_t *prim, float *area, uint32_t *mass /* CDF units */);
/* the light table as the shading kernel reads it, for tests that pin it bit for bit (any pointer may be NULL): the table that
 * flags & (RT3_F_NEE_EMISSIVE | RT3_F_NEE_PUNCTUAL) samples, entries in rt3_light_masses' order, n = n_emitters + n_punctual of them.
 * rec: 16 floats per entry, {A xyz, p_sel / area} {E1 xyz, Le.r} {E2 xyz, Le.g} {unit normal, Le.b} for an emitter triangle A, A + E1, A + E2
 * with Le = 12 emission and p_sel = mass / 2^23 (0 for an entry of no mass or no area); a punctual light's record is {position, p_sel}
 * {unit axis, I.r} {cone scale, cone offset, 1 / range, I.g} {tag, 0, 0, I.b}.  cdf: n words, the inclusive integer CDF (cdf[n - 1] = 2^23, or
 * every word 0 when no entry has power).  guide: *cells + 1 words; *cells is the smallest power of two >= n, at most 2^20, *shift =
 * 23 - log2(*cells); guide[c] = the first entry with cdf > c << shift (n in a table without power: there is none), guide[*cells] = n - 1.  The entry that owns k in [0, 2^23) is the first
 * with cdf > k, searched between guide[k >> shift] and guide[(k >> shift) + 1].  prim, area: n words each, the flattened primitive and the
 * world-space area the selection divided by (0xFFFFFFFF and 1 for a punctual light).  A combination that samples nothing: *cells = *shift = 0 and no
 * array is written.  RT3_E_STATE where rt3_light_info returns it. */
int rt3_light_table(rt3_ctx *ctx, uint32_t flags, float *rec /* 16 per entry */, uint32_t *cdf, uint32_t *guide, uint32_t *prim, float *area,
                    uint32_t *cells, uint32_t *shift);

/* ---- textured emitters (no reference equivalent).  Off by default: RT3_F_NEE_EMISSIVE leaves out every geometry whose
 * rt3_material_textures entry names an emissive texture, and such a geometry is found by BSDF-sampled rays alone, with weight 1.
 * rt3_scene_set_textured_emitters(ctx, 1) makes those geometries entries of the light table too.  The mode moves only the light table's
 * key (as rt3_scene_set_lights does): the acceleration structure stays current, and the next frame or readback remakes the table.  The
 * key also holds the texture pool: a later rt3_scene_set_texture remakes the table of a context whose mode is on.
 *   Which tables change: only those of a built scene with at least one textured emitter -- a geometry with non-zero emission, triangles,
 * no alpha cutoff (masked geometries stay out, section 4e) and an emissive texture index below the number of uploaded textures.  Without
 * one (no material textures, or every emissive index not uploaded) table and frames are the mode-off ones bit for bit and nothing more is
 * launched.  With one, every emissive unmasked geometry is listed; an emitter whose emissive index is not uploaded is listed without
 * texture, as the hit side reads it.
 *   Records: unchanged, Le = 12 emission (the factor, as if the texture were 1).  A side array of 32 bytes per table entry holds
 * {uv0, uv1, uv2, emissive texture index or -1, 0}: the vertex uvs in the order the record's A, E1, E2 were made, so the point
 * A + b1 E1 + b2 E2 has uv = uv0 (1 - b1 - b2) + uv1 b1 + uv2 b2 -- the hit side's expression.  rt3_light_emit_tex reads it back
 * (*n_entries = 0 and nothing written for a table without textured emitter).
 *   Selection mass of a textured emitter: area x luminance(Le (*) mean_rgb), where mean_rgb is a fixed quadrature of the emissive lookup
 * (bilinear, repeat addressing, sRGB decode per texel: the hit side's) over the triangle:
 *     L = clamp(ceil(longest uv edge in texels), 1, 64); the edge (du, dv) of a W x H texture measures max(|du| W, |dv| H), all in fp32;
 *         a non-finite edge gives L = 1;
 *     the triangle is cut into L^2 congruent triangles by the lines b1 = i / L, b2 = j / L, b1 + b2 = k / L; the lookup is taken at their
 *         centroids: (b1, b2) = ((3 i + 1) / 3L, (3 j + 1) / 3L) for i + j < L and ((3 i + 2) / 3L, (3 j + 2) / 3L) for i + j < L - 1, each one fp32
 *         division of two exact integers;
 *     mean_rgb = the sum of the L^2 lookups / L^2 per channel.  Centroid number k = a L + c (a, c < L) is the first kind's (i, j) = (a, c) when
 *         a + c < L and the second kind's (L - 1 - a, L - 1 - c) otherwise; lane l of 64 adds centroids l, l + 64, ... in rising order and the
 *         lane sums meet in a butterfly (xor 32, 16, .. 1): the same bits on every run, in both instance modes and after a refit.
 * The mean steers variance only: a triangle whose quadrature finds nothing gets mass 0 and is never sampled (its hits keep weight 1), a
 * sampled point whose texel is black contributes 0, and all points of one triangle share one density (uniform on the triangle, not
 * proportional to the texel).
 *   The light sample: k_shade queues the emitter shadow ray with the factor as radiance; k_emit_tex, between it and the k_shadow launch,
 * redraws the path's RNG dims 5, 6, 7, finds the emitter and the point again and multiplies the ray's contribution by the texture there.
 * rt3_stats.emit_tex_launches counts its launches.  RT3_E_INVALID for a mode other than 0 or 1. */
int rt3_scene_set_textured_emitters(rt3_ctx *ctx, int on);
int rt3_scene_get_textured_emitters(rt3_ctx *ctx, int *on);
int rt3_light_emit_tex(rt3_ctx *ctx, uint32_t flags, uint32_t *n_entries, void *out /* 8 words per entry, may be NULL */);

/* ---- fog (no reference equivalent): one axis-aligned box of homogeneous medium with single scattering.  Off by
 * default; with it off every frame keeps its bits and nothing more is launched.  "refrence_mode" and "adaptive" read it.
 *   rt3_scene_set_medium(ctx, m): sigma_a and sigma_s are the absorption and scattering coefficients per colour channel (per world unit),
 * g the Henyey-Greenstein asymmetry, box_min / box_max the box.  NULL switches the medium off.  RT3_E_INVALID, and nothing changes, for a
 * sigma that is negative or not finite, |g| >= 1 or a g that is not finite, a box coordinate that is not finite, or box_min.k >= box_max.k
 * on some axis.  A medium whose sigma_a + sigma_s is 0 in every channel is stored and counts as off.  The call leaves the acceleration
 * structure and the light table as they are; rt3_scene_set_geometry leaves the medium as it is.
 *   The rule (csrc/rt3_fog.hpp states it once): every traced path segment o + s d, s in [0, t] (t = +inf on a miss) is cut by the box's
 * slabs to [t0, t1]; the throughput takes exp(-sigma_t (t1 - t0) |d|) per channel, sigma_t = sigma_a + sigma_s.  When some sigma_s > 0 and the
 * frame samples lights, one point of the segment is drawn (density proportional to exp(-mean(sigma_t) s)) and lit by one sky sample
 * (RT3_F_NEE_SKY with a sky) and one sample of the light table (RT3_F_NEE_EMISSIVE / RT3_F_NEE_PUNCTUAL, bounces >= 2), each a shadow ray
 * with the phase function and the transmittance towards the light in its contribution; and the shadow rays of surface vertices have their
 * contribution multiplied by the transmittance along them.  Light scattered out of a ray is lost (no multiple scattering): dense fog with
 * a high albedo renders too dark.
 *   Launches: a medium needs per-sample camera rays (rt3_camera_set_lens; {0, f, 0} is the per-sample pinhole): "refrence_mode" without a
 * lens is RT3_E_STATE, "adaptive" takes it in coverage mode (rt3_adaptive_set_coverage) and is RT3_E_STATE otherwise; a launch with
 * samples * bounces * 8 > 2^28 is RT3_E_INVALID (the fog draws' RNG indices start at 0x70000000 and end where the camera's start).
 * RT3_OPT_DEFER_SKY_LIGHT and RT3_OPT_SHADE_EXIT_TEST do not apply to a frame with a medium.  "gbuffer", "denoise", "temporal", "motion",
 * the guide images and the probe passes do not see the medium.
 *   rt3_medium_info (either pointer may be NULL; synchronises the stream): of the last "refrence_mode" or "adaptive" launch, the traced
 * segments that ran through the medium and the in-scatter shadow rays queued for them. */
typedef struct rt3_medium {
    float sigma_a[3];
    float sigma_s[3];
    float g;
    float box_min[3];
    float box_max[3];
} rt3_medium;           /* 52 bytes */
int rt3_scene_set_medium(rt3_ctx *ctx, const rt3_medium *m);   /* NULL: off, the default */
int rt3_scene_get_medium(rt3_ctx *ctx, rt3_medium *out, int *enabled);
int rt3_medium_info(rt3_ctx *ctx, uint64_t *segments, uint64_t *inscatter_rays);  /* of the last launch; synchronises */
/* sky tables for parity tests (any pointer may be NULL): per-row alias words q16 | alias << 16 (w*h), RGB9E5 texels (w*h),
 * marginal CDF (h), realised (u,v) density (w*h) */
int rt3_sky_download(rt3_ctx *ctx, uint32_t *alias, uint32_t *texels_rgb9e5, float *cdf_marg, float *pdf_uv);

/* ---- resources: RenderGraph::image / buffer / import (render_graph/mod.rs:422-483) ---- */
int rt3_buffer_create(rt3_ctx *ctx, size_t bytes, uint32_t *out_handle);
int rt3_image_create(rt3_ctx *ctx, uint32_t width, uint32_t height, uint32_t format, uint32_t *out_handle);
int rt3_image_import(rt3_ctx *ctx, void *device_ptr, uint32_t width, uint32_t height, uint32_t format, uint32_t *out_handle);
int rt3_resource_upload(rt3_ctx *ctx, uint32_t handle, const void *src, size_t bytes);
int rt3_resource_download(rt3_ctx *ctx, uint32_t handle, void *dst, size_t bytes); /* headless stand-in for present */
int rt3_resource_device_ptr(rt3_ctx *ctx, uint32_t handle, void **out_ptr, size_t *out_bytes);

/* ---- framebuffer partition (north_star): 64x64 tiles, Z-order over the tile grid, tile i -> rank i % n_ranks.
 *      Passes only touch the pixels owned by `rank`.  Default: rank 0 of 1. ---- */
int rt3_set_tile_partition(rt3_ctx *ctx, uint32_t width, uint32_t height, uint32_t rank, uint32_t n_ranks);
int rt3_tile_pixel_count(rt3_ctx *ctx, uint32_t rank, uint32_t n_ranks, uint32_t *out_count);
/* gather support: image (full window) <-> contiguous per-rank tile buffer (count x 16 bytes, device memory) */
int rt3_image_pack_tiles(rt3_ctx *ctx, uint32_t image, uint32_t rank, uint32_t n_ranks, void *dst_device);
int rt3_image_unpack_tiles(rt3_ctx *ctx, uint32_t image, uint32_t rank, uint32_t n_ranks, const void *src_device);

/* ---- frame-end gather (north_star: "the framebuffer is tile-partitioned across the 8 GPUs of one node with a single RCCL gather
 *      over xGMI at frame end").  No reference counterpart: the reference is single-device.  One context =
 *      one rank = one GPU = one process.  Rank 0 makes an id with rt3_comm_unique_id and the HOST carries its 128 bytes to the
 *      other ranks over whatever channel it already has (the ABI opens no sockets); then every rank calls rt3_comm_init
 *      (collective: ncclCommInitRank on the context's device) with the rank / n_ranks it gave rt3_set_tile_partition.
 *      rt3_gather_tiles is the one collective of a frame: enqueued on the context's stream behind the passes, no host
 *      synchronisation.  Non-root ranks pack their tiles of `image` and send them; `root` receives every rank's tiles at its exact
 *      offset of ONE contiguous buffer (all receives in one RCCL group: the root's inbound xGMI links run concurrently, nothing is
 *      forwarded) and scatters them into its `image` with ONE untile launch.  The root's own tiles never move.
 *      rt3_gather_layout / rt3_gather_unpack expose the root's half without the exchange (hosts that move the bytes themselves --
 *      the gloo rehearsal on a one-GPU box -- and the layout tests): offsets[r] .. offsets[r+1] is rank r's pixel range in the
 *      receive buffer (16 bytes per pixel, pixels in rt3_image_pack_tiles order, the root's range empty), n_ranks + 1 entries. ---- */
#define RT3_COMM_ID_BYTES 128
int rt3_comm_version(int *out); /* ncclGetVersion of the RCCL this library is linked against: major * 10000 + minor * 100 + patch */
int rt3_comm_unique_id(void *id_out /* RT3_COMM_ID_BYTES */);
int rt3_comm_init(rt3_ctx *ctx, const void *id /* RT3_COMM_ID_BYTES */, uint32_t rank, uint32_t n_ranks);
int rt3_comm_destroy(rt3_ctx *ctx);
int rt3_gather_tiles(rt3_ctx *ctx, uint32_t image, uint32_t root);
int rt3_gather_layout(rt3_ctx *ctx, uint32_t image, uint32_t root, uint32_t n_ranks, uint64_t *offsets /* n_ranks + 1 */);
int rt3_gather_unpack(rt3_ctx *ctx, uint32_t image, uint32_t root, uint32_t n_ranks, const void *recv_device);

/* ---- pass launch: ExecutionTrait::execute (render_graph/mod.rs:80-91) of a RayTracingPass / ComputePass node
 *      (render_graph/executions.rs:15-55,80-121) -> RayTracingPipelineHandle::launch(x, y) /
 *      ComputePipelineHandle::dispatch(x, y, z) (pipeline_cache/mod.rs:24-76).
 *      `pass_name` is the shader path the reference would load from ./shaders/bin/{path}.slang.spv
 *      (pipeline_cache/mod.rs:278-279); `constants` is the raw GConst blob (build.rs:66-94); `bindings` is the ordered
 *      handle list of the node's non-attachment edges (bake.rs:51-83):
 *        "gbuffer"       (x,y)=window   bindings {gbuffer RGBA32UI, gbuffer_depth R32F}                (gbuffer.slang:5-6)
 *        "refrence_mode" (x,y)=window   bindings {gbuffer, gbuffer_depth, Light, PrevLight}            (refrence_mode.slang:8-11)
 *        "postprocess"   (x,y,z)=groups of 8x8  bindings {Depth, Out RGBA32F, In RGBA32F}             (postprocess.slang:5-7)
 *        "denoise"       (x,y,z)=groups of 8x8 over the window  bindings {gbuffer, gbuffer_depth, In RGBA32F, Out RGBA32F}
 *                        (no reference counterpart: the edge-avoiding filter described at rt3_denoise_set_params below)
 *        "temporal"      (x,y,z)=groups of 8x8 over the window  bindings {gbuffer, gbuffer_depth, In RGBA32F, PrevGbuffer RGBA32UI,
 *                        PrevDepth R32F, PrevHistory RGBA32F, PrevMoments RGBA32F, Out RGBA32F, History RGBA32F, Moments RGBA32F}
 *                        (no reference counterpart: the reprojected accumulation described at rt3_temporal_set_params below)
 *        "motion"        (x,y)=window   bindings {Motion RGBA32F}
 *                        (no reference counterpart: where each surface point was one frame ago, rt3_temporal_set_motion_input below)
 *        "adaptive"      (x,y)=window   bindings {gbuffer, gbuffer_depth, Light, PrevLight, Moments RGBA32F}
 *                        (no reference counterpart: refrence_mode to a noise threshold, rt3_adaptive_set_params below)
 *      and the probe-GI passes (restated as written, debug stores included; rules for what the text leaves open are listed in
 *      DESIGN.md section 11).  A probe owns 16x16 pixels and an 8x8-texel cell of the atlas images; bindings are ordered by
 *      (descriptor set, binding) as the shaders declare them:
 *        "structured_importance_sampling" (x,y,1)=probes  {gbuffer, gbuffer_depth, out R16UI, debug R32F, probe_atlas RGBA32F}
 *        "trace_probes"                   (x,y)=atlas size {gbuffer, gbuffer_depth, directions R16UI, probe_atlas, prev_probe_atlas}
 *        "spherical_harmonic_conversion"  (x,y,1)=probes  {out buffer of float3x3 (48 B, rows padded to float4), probe_atlas}
 *        "interpolate_probes"             (x,y,1)=groups of 8x8 over the window  {gbuffer, gbuffer_depth, sh_coeficents buffer, Light}
 *      The checked form of this list (launch shape, bindings, formats, the images that may not alias) is the table kPasses in
 *      raytracer3_amd/csrc/rt3_passes.hip: where the two differ, the table is what the library does.
 *      Work is enqueued on the context's stream and returns immediately. ---- */
int rt3_pass_launch(rt3_ctx *ctx, const char *pass_name, const char *entry, uint32_t x, uint32_t y, uint32_t z,
                    const void *constants, size_t constants_size, const uint32_t *bindings, uint32_t n_bindings);
/* ---- "denoise": a G-buffer-guided, edge-avoiding a-trous wavelet filter (the spatial half of SVGF) for low-sample frames.  No reference
 *      counterpart; DESIGN.md section 4f.  Out = filtered In (linear radiance, e.g. the Light of refrence_mode) for foreground pixels; background
 *      pixels (gbuffer_depth == RT3_BACKGROUND_DEPTH) and every alpha are copied from In bit for bit, and background pixels never contribute.
 *      In is demodulated by the first-hit albedo and emission of the G-buffer (c = (In - emission) / max(albedo, 1/256)), filtered, and
 *      modulated again, so base-colour textures are preserved.  Stages: a 7 x 7 spatial variance estimate of luminance(c), then `iterations`
 *      passes of 5 x 5 B3-spline taps at step 2^i, each tap weighted by max(0, n_p . n_q)^(2^normal_squarings) (shading normals),
 *      exp(-sin(angle by which the tap leaves p's tangent plane) / sigma_z) (world positions from gbuffer_depth and GConst's camera) and
 *      exp(-|l_q - l_p| / (sigma_l * sqrt(3 x 3 blurred variance) + 1e-6)).  fp32, equal to tests/ref_denoise.py bit for bit.
 *      In and Out must be different images (RT3_E_INVALID); formats and sizes are checked like every pass.  iterations = 0 copies In to Out.
 *      A tap needs pixels that other ranks own: under a tile partition with more than one rank the pass returns RT3_E_STATE (filter the
 *      gathered image on the gather root with the partition switched off).  The scratch images (64 bytes per pixel) belong to the context,
 *      are reserved on first use and kept across frames.
 *      rt3_denoise_set_params: NULL restores the defaults {5, 7, 0.05, 4.0, 0}.  RT3_E_INVALID (nothing changed) for iterations > 8,
 *      normal_squarings > 16, a sigma that is not finite or not positive, or an unknown flag. ---- */
#define RT3_DENOISE_NO_DEMODULATION 1u /* In is not what refrence_mode wrote (the probe-GI Light, for one): filter it as it is */
typedef struct rt3_denoise_params {
    uint32_t iterations;       /* a-trous passes, step 1, 2, 4, ...: 0..8 */
    uint32_t normal_squarings; /* k: the normal weight's exponent is 2^k */
    float sigma_z;
    float sigma_l;
    uint32_t flags; /* RT3_DENOISE_* */
} rt3_denoise_params;
int rt3_denoise_set_params(rt3_ctx *ctx, const rt3_denoise_params *params);
/* The temporal variance for "denoise": with `moments_image` set to the Moments image {mu1, mu2, variance, N} that "temporal" wrote for the
 * same frame, the result of the 7 x 7 stage is replaced per foreground pixel by Moments.z where Moments.w >= 4 (SVGF's rule: a history of
 * at least four frames); elsewhere the spatial estimate stands.  0 (the default) = none: "denoise" computes what it always did.  The image
 * is checked when "denoise" is launched: a live RGBA32F image of the window's size that is not Out, else RT3_E_INVALID. */
int rt3_denoise_set_variance_input(rt3_ctx *ctx, uint32_t moments_image);

/* ---- "temporal": reprojected accumulation under a moving camera (the temporal half of SVGF).  No reference counterpart; DESIGN.md section
 *      4g.  Per foreground pixel: the surface record of "denoise" (world position P from gbuffer_depth and GConst's camera, 11:10:11 normal n,
 *      c = (In - emission) / max(albedo, 1/256), l = luminance(c)); q = prev.proj * prev.view * (P, 1) gives the position (sx, sy) in the
 *      previous frame, sx = (q.x / q.w * 0.5 + 0.5) * W - 0.5, sy = (-q.y / q.w * 0.5 + 0.5) * H - 0.5.  Its four bilinear taps count when they
 *      lie inside the window, are foreground in PrevDepth, have PrevHistory.w > 0, n . n_q >= normal_cos and
 *      |n . (P_q - P)| <= plane_tolerance * |P - eye| (P_q from PrevDepth and the previous camera).  With h, k the weight-normalised taps of
 *      PrevHistory and PrevMoments: N = min(h.w + 1, max_history), a = max(alpha, 1 / N), c_acc = h + a (c - h), likewise mu1, mu2 of l and
 *      l * l with alpha_moments; variance = max(0, mu2 - mu1^2).  Without a counted tap (or q.w <= 0, or (sx, sy) outside (-1, W) x (-1, H)):
 *      N = 1, c_acc = c, mu1 = l, mu2 = l * l.  History = {c_acc, N}, Moments = {mu1, mu2, variance, N}, Out = {emission + c_acc * albedo,
 *      In.a}: displayable, and a valid In for "denoise".  Background pixels: Out = In bit for bit, History = Moments = 0.
 *      PrevHistory.w > 0 is the reset rule: zeroed previous images mean "no history" (first frame, resize, new scene).  fp32, equal to
 *      tests/ref_temporal.py bit for bit.  Without a motion input (rt3_temporal_set_motion_input, below) the scene is taken as static between
 *      the two frames; with one, instances whose matrices changed keep their history, and so do meshes deformed by
 *      rt3_scene_update_vertices after a rt3_scene_snapshot_vertices; without a snapshot such a mesh has no previous vertices and is caught
 *      only as far as the plane test catches it.
 *      The three written images must differ from each other and from every image read (RT3_E_INVALID).  Under a tile partition with more
 *      than one rank the pass returns RT3_E_STATE, like "denoise".  A launch with no previous view set returns RT3_E_STATE; a previous
 *      window_size that differs from the launch's is RT3_E_INVALID.
 *      rt3_temporal_set_prev_view: the previous frame's 304-byte GConst, captured by value at each launch; only proj, view, proj_inverse,
 *      view_inverse and window_size are read.  size must be 304; (NULL, 0) forgets the view.
 *      rt3_temporal_set_params: NULL restores the defaults {0.2, 0.2, 32, 0.9, 0.01, 0}.  RT3_E_INVALID (nothing changed) for a value outside
 *      the ranges below, NaN included, or an unknown flag. ---- */
#define RT3_TEMPORAL_NO_DEMODULATION 1u /* same meaning as RT3_DENOISE_NO_DEMODULATION */
typedef struct rt3_temporal_params {
    float alpha;           /* floor of the colour blend weight, 0..1; 0 = plain running mean */
    float alpha_moments;   /* the same for the moments */
    uint32_t max_history;  /* N is clamped to this, 1..65535 */
    float normal_cos;      /* a tap is rejected when n_p . n_q < normal_cos; -1..1 */
    float plane_tolerance; /* ... or when |n_p . (P_q - P_p)| > plane_tolerance * |P_p - eye|; finite, > 0 */
    uint32_t flags;        /* RT3_TEMPORAL_* */
} rt3_temporal_params;
int rt3_temporal_set_prev_view(rt3_ctx *ctx, const void *prev_gconst, size_t size);
int rt3_temporal_set_params(rt3_ctx *ctx, const rt3_temporal_params *params);
/* ---- "motion": temporal history that follows moved instances.  No reference counterpart; DESIGN.md section 4h.  The pass traces the
 *      primary rays of GConst's camera (the launches of "gbuffer", so the hits are the G-buffer's) and writes one texel per pixel this rank
 *      owns; with i the instance of the hit geometry:
 *        miss                                                                       -> {0, 0, 0, 0}
 *        no previous transforms, or instance i's 3 x 4 matrix equals its previous
 *        one word for word (as uint32: -0 is not +0)                                -> {P, 1}, P = o + d t: the bits "denoise" and
 *                                                                                      "temporal" compute from gbuffer_depth
 *        otherwise                                                                  -> {P', 2}, P' = prev_i * p, p = (a w + b u) + c v with
 *                                                                                      w = (1 - u) - v and a, b, c the triangle's vertices
 *                                                                                      in object space (P' = p when prev_i is the identity)
 *        the hit geometry is deformed (rt3_scene_snapshot_vertices, above), whether or
 *        not instance i moved                                                       -> {P'', 3}, P'' = M * p'', p'' the same expression over
 *                                                                                      the triangle's three snapshot positions; M = prev_i, or
 *                                                                                      instance i's current matrix without previous
 *                                                                                      transforms (P'' = p'' when M is the identity)
 *      fp32, singly rounded, equal to tests/ref_motion.py and tests/ref_deform.py bit for bit.  RT3_E_STATE without a structure, while vertices are stale, or when
 *      the number of previous transforms is neither 0 nor the structure's instance count.  Works under a tile partition like "gbuffer".
 *      rt3_temporal_set_motion_input: the Motion image "temporal" reads; 0 (the default) = none, and every bit "temporal" writes is what it
 *      was.  With one, a foreground pixel whose texel has w < 1 gets no history (N = 1); otherwise the texel's xyz takes P's place in the
 *      reprojection and in P_q - P of the plane test, while the tolerance |P - eye|, the normal and the surface record stay this frame's.
 *      Checked when "temporal" is launched: a live RGBA32F image of the window's size that is none of Out, History, Moments, else
 *      RT3_E_INVALID.
 *      Limits: the normal test compares this frame's normal with the previous G-buffer's, so an instance that turns by more than
 *      acos(normal_cos) in one frame loses its history; light that moves (a moved object's shadow, a moved emitter) still lags on unmoved
 *      surfaces; "deformed" is per geometry, so the still part of a deformed mesh pays for the gather (its texel is its own point);
 *      there are no previous normals: a surface that bends by more than acos(normal_cos) in one frame loses its history. ---- */
int rt3_temporal_set_motion_input(rt3_ctx *ctx, uint32_t motion_image);
/* ---- "adaptive": refrence_mode "to a noise threshold, up to N samples".  No reference counterpart; DESIGN.md section 4l.  The pass traces the
 *      paths refrence_mode traces -- GConst.bounces, the flags, frame and blendfactor mean what they mean there -- but GConst.samples is the
 *      CAP: a pixel stops when the variance of its luminance says its mean is good enough.  Moments may be none of the other four images.
 *      Per foreground pixel of this rank's list the pass keeps n, the sample count; S1 = sum y and S2 = sum y * y in float32 and in sample
 *      order, y = luminance(sample rgb) = r 0.299 + g 0.587 + b 0.114; and the three colour sums exactly as refrence_mode forms them (from
 *      0.0f, in sample order).
 *      The loop:
 *       - round 0 gives every foreground pixel min(min_samples, cap) samples; each later round gives the still-active pixels
 *         min(step, cap - n) more, numbered n, n + 1, ...: n is the same for every active pixel, and the RNG counter
 *         (sample * bounces + bounce) * dims + dim does not know the cap;
 *       - after each round a pixel PASSES when, in this operation order, in float32, without contraction and with IEEE divides,
 *             mean = S1 / n
 *             var  = (S2 - S1 * mean) / (n - 1), replaced by 0 if negative
 *             rel  = threshold * (mean + dark)
 *             var <= (rel * rel) * n
 *         (the variance of the mean, var / n, against the square of a relative error; `dark` keeps black pixels from never passing);
 *       - a pixel STAYS ACTIVE if it fails or, with dilate = 1, if any foreground pixel of this rank's list in its 3 x 3 neighbourhood
 *         fails; background pixels, pixels outside the window and pixels of other ranks count as passing.  A pixel that has stopped never
 *         restarts: its state is frozen;
 *       - the loop ends when no pixel is active or n == cap.  An empty list launches nothing further.  A cap below min_samples runs
 *         `samples` for every pixel.
 *      At the end, per foreground pixel: Light = sums / (float)n, then refrence_mode's blend with PrevLight under blendfactor; Moments =
 *      {S1, S2, n, 1 if the pixel stopped before the cap else 0}.  So a pixel that stopped at n holds the bits refrence_mode writes for it
 *      in a frame of samples = n.  Background pixels: Light untouched (as refrence_mode leaves it), Moments = 0; they are in no traced
 *      list, round 0 included.  samples = 0 or bounces = 0 does nothing, like refrence_mode.
 *      The estimate is NOT unbiased: a pixel that draws a prefix of low variance stops early; min_samples and the dilation are the
 *      mitigations.  Works under a tile partition on the rank's own pixels; with dilate = 0 the result does not depend on the partition.
 *      The active count comes back to the host once per round (4 bytes, one stream synchronisation): the launch returns after the last
 *      round is enqueued, not at once.  RT3_OPT_BATCH_SPP splits a round as it splits refrence_mode's frame.
 *      rt3_adaptive_set_params: NULL restores the defaults {16, 16, 0.05, 0.01, 1, 0}.  RT3_E_INVALID (nothing changed) for min_samples < 2,
 *      step < 1, a threshold that is not finite or negative, a dark that is not finite or not positive, dilate > 1 or any flag bit (none
 *      is defined).
 *      rt3_adaptive_info (any pointer may be NULL): of the last "adaptive" launch, the rounds run, the first-vertex paths traced (the sum
 *      of n over this rank's foreground pixels; in coverage mode over all of this rank's pixels) and the pixels that reached the cap.
 *      Coverage mode (rt3_adaptive_set_coverage; 0, the default: "adaptive" refuses a lens).  A mode of the context that survives scene
 *      changes; on other than 0 or 1 is RT3_E_INVALID and changes nothing.  It matters only while a lens is set (rt3_camera_set_lens): then
 *      the pass starts every sample from its own camera ray, as "refrence_mode" does, and "foreground pixel" above reads "pixel of this
 *      rank's list": round 0 lists them all, in the list's order, without a depth test (and without a device-to-host read); pixels outside
 *      the window and pixels of other ranks still count as passing; every listed pixel gets Light and Moments at the end, one whose centre
 *      sees the background included, so n is never 0 on an owned pixel.  gbuffer and gbuffer_depth stay bound and validated and are not
 *      read.  A pixel that stopped at n holds the bits "refrence_mode" with the same lens writes for it at samples = n.  Glass, pane
 *      shadows and roulette work as there.  "refrence_mode"'s range rules hold with the cap as `samples`: RT3_E_INVALID for
 *      cap * bounces * 8 > 2^31, and > 2^30 in a built scene with glass.  Without a lens the mode is inert: the pass above, and
 *      RT3_E_STATE for a scene with glass.  With a lens and the mode off: RT3_E_STATE. ---- */
typedef struct rt3_adaptive_params {
    uint32_t min_samples; /* round 0; >= 2 (the variance divides by n - 1) */
    uint32_t step;        /* samples per later round; >= 1 */
    float threshold;      /* relative standard error of the pixel mean to stop at; finite, >= 0 (0: only var == 0 passes) */
    float dark;           /* added to the mean; finite, > 0 */
    uint32_t dilate;      /* 0, or 1: the 3 x 3 rule */
    uint32_t flags;       /* none defined: 0 */
} rt3_adaptive_params;
int rt3_adaptive_set_params(rt3_ctx *ctx, const rt3_adaptive_params *params);
int rt3_adaptive_info(rt3_ctx *ctx, uint32_t *rounds, uint64_t *paths_traced, uint32_t *pixels_capped);
int rt3_adaptive_set_coverage(rt3_ctx *ctx, int on);
int rt3_adaptive_get_coverage(rt3_ctx *ctx, int *on);
/* ---- per-sample camera rays: pixel-filter antialiasing and a thin lens.  No reference counterpart; DESIGN.md section 4m.  By default every
 *      sample of a pixel starts at the G-buffer's hit, the one through the pixel centre.  With a lens set, "refrence_mode" gives every sample
 *      its own camera ray instead: sample s (absolute index, 0 .. samples-1) of pixel (px, py) draws four numbers at the RNG indices
 *      0x80000000 + 4 s + k of the pixel's stream (seed as for the path's vertices, no blue-noise shift): k = 0, 1 place the film point in
 *      the box of width pixel_jitter pixels around the pixel centre, k = 2, 3 a point on the lens disk of radius aperture_radius around the
 *      eye, in the plane of view_inverse's columns 0 and 1 (uniform in area).  The ray leaves the lens point towards the point where the
 *      pinhole ray through the film point meets the plane of focus, at view depth focus_distance.  It is traced like every extension ray
 *      (from t = 0.001), and its hit is shaded as a path vertex from the shading records, not from the G-buffer: materials at vertex 0 are
 *      not quantised, so a lens frame is not the default frame plus jitter.  A camera ray that escapes adds the sky's bilinear radiance along
 *      its direction (nothing without a sky), once.  Every listed pixel is written: Light = (sum over samples) / samples, then the blend with
 *      PrevLight, on pixels whose centre sees the background too.
 *      A non-NULL call switches this on, {0, f, 0} included (a per-sample pinhole through the pixel centre); NULL switches it off, the
 *      default.  The state lives in the context; nothing is rebuilt.  RT3_E_INVALID (nothing changed) for a value that is not finite, an
 *      aperture_radius < 0, a pixel_jitter outside [0, 1], a focus_distance <= 0 with aperture_radius > 0, or reserved != 0.
 *      Coupled passes while a lens is set: "postprocess" takes every pixel from In (the Depth == background branch would put the pinhole sky
 *      over half of each antialiased silhouette); "adaptive" returns RT3_E_STATE (it selects pixels by G-buffer depth) unless
 *      rt3_adaptive_set_coverage lets it take every pixel; "refrence_mode", and "adaptive" then, with samples * bounces * 8 > 2^31 return RT3_E_INVALID (the vertices' RNG indices would reach the camera's).  "gbuffer", "denoise",
 *      "temporal", "motion" and the probe passes do not know the lens: they see the pinhole G-buffer at pixel centres.  "denoise" and
 *      "temporal" are guided by that G-buffer too unless they are given the lens frame's own guide images (rt3_camera_set_guide_output,
 *      rt3_denoise_set_guide_input and rt3_temporal_set_guide_input, below); guiding a depth-of-field frame by the pinhole G-buffer is not supported.
 *      rt3_camera_get_lens (either pointer may be NULL): the parameters last set (the defaults {0, 1, 1, 0} before any) and whether on. ---- */
typedef struct rt3_lens_params {
    float aperture_radius;  /* world units, >= 0; 0 = pinhole */
    float focus_distance;   /* > 0 when aperture_radius > 0: distance of the plane of focus along the view axis */
    float pixel_jitter;     /* in [0, 1]: width of the box the film point is drawn from, in pixels; 1 = the whole pixel, 0 = its centre */
    uint32_t reserved;      /* 0 */
} rt3_lens_params;
int rt3_camera_set_lens(rt3_ctx *ctx, const rt3_lens_params *p);   /* NULL: off, the default */
int rt3_camera_get_lens(rt3_ctx *ctx, rt3_lens_params *out, int *enabled);
/* ---- guide images: "denoise" for lens and glass frames.  No reference counterpart; DESIGN.md section 4u.
 *      rt3_camera_set_guide_output names four RGBA32F images of the window's size that "refrence_mode" writes while a lens is set, beside
 *      Light; the pass's bindings and GConst are untouched.  Per listed pixel, over all S = GConst.samples camera samples in ascending order,
 *      in fp32 with one rounding per operation and no contraction: a sample whose camera ray hit primitive prim at (t, bu, bv) adds
 *      P = o + d t (the camera ray's origin and direction) to sum_P, and of surf = the unquantised surface the path tracer shades at vertex
 *      0 (self-test op 29, with material textures where the scene has them) surf.normal to sum_n, surf.albedo to sum_a, surf.emissive to
 *      sum_e, and 1 to n_hit; a sample that escaped adds (1, 1, 1) to sum_a (the sky is not albedo-modulated) and nothing else.  Written:
 *        position = {sum_P / n_hit, n_hit / S}   (all zero when n_hit = 0: position.w is the pixel's coverage)
 *        normal   = {sum_n / n_hit, 0}           (zero when n_hit = 0; not normalised)
 *        albedo   = {sum_a / S, 0}
 *        emission = {sum_e / S, 0}
 *      The sums run in sample order whatever RT3_OPT_BATCH_SPP is (between batches the images hold them), so the bits do not depend on
 *      it, on RT3_OPT_INSTANCE_MODE or on the tile partition: a rank writes its own pixels only.  Light has the bits it has without the
 *      guide output.  Glass at vertex 0 contributes the glass surface's own features, not those of what is seen through it.
 *      NULL switches the output off, the default.  RT3_E_INVALID at set time (nothing changed) for a handle that is not a live RGBA32F
 *      image or for two equal handles.  At a "refrence_mode" launch: RT3_E_STATE when no lens is on; RT3_E_INVALID when an image has not the
 *      window's size or is Light or PrevLight, or when samples > 2^24 (the hit count is a float); nothing is enqueued.  "adaptive" returns
 *      RT3_E_STATE while a guide output is set: it writes no guide, and a stale one must not be filtered.
 *      rt3_camera_get_guide_output (either pointer may be NULL): the handles last set (zeros before any) and whether on.
 *      rt3_denoise_set_guide_input gives "denoise" such a set as its guide in the G-buffer's place; NULL (the default) = the G-buffer, and
 *      every bit the pass writes is what it was.  The bindings stay {gbuffer, gbuffer_depth, In, Out}; the first two are then validated and
 *      not read.  A pixel is foreground iff position.w == 1 (every sample hit) and l2 = normal . normal is finite and positive; then
 *      P = position.xyz, n = normal.xyz * (1 / sqrt(l2)), c = (In - emission) / max(albedo, 1/256), and at the end Out = emission +
 *      c * max(albedo, 1/256) (RT3_DENOISE_NO_DEMODULATION keeps its meaning).  Every other pixel is treated as a background pixel is:
 *      copied from In bit for bit, weight 0 as a tap.  So partly covered pixels -- a silhouette over the sky -- stay unfiltered, and nothing
 *      bleeds across them.  The variance and a-trous stages, the parameters, the variance input and the multi-rank refusal are those above.
 *      The four images are checked at each launch like the variance input: live RGBA32F images of the window's size, none of them Out,
 *      else RT3_E_INVALID.  fp32, equal to tests/ref_guide.py bit for bit. ---- */
typedef struct rt3_guide_images {
    uint32_t position, normal, albedo, emission; /* image handles */
} rt3_guide_images;
int rt3_camera_set_guide_output(rt3_ctx *ctx, const rt3_guide_images *images);  /* NULL: off, the default */
int rt3_camera_get_guide_output(rt3_ctx *ctx, rt3_guide_images *out, int *enabled);
int rt3_denoise_set_guide_input(rt3_ctx *ctx, const rt3_guide_images *images);  /* NULL: the G-buffer, the default */
/* ---- temporal accumulation for lens and glass frames.  No reference counterpart; DESIGN.md section 4v.
 *      rt3_temporal_set_guide_input gives "temporal" two guide sets -- the one this frame's "refrence_mode" wrote and the one the previous
 *      frame's wrote -- as its surface records in the G-buffer's place.  Both NULL (the default) = the G-buffer, and every bit the pass
 *      writes is what it was; exactly one NULL returns RT3_E_INVALID and changes nothing.  The pass keeps its ten bindings and its
 *      parameters; gbuffer, gbuffer_depth, PrevGbuffer and PrevDepth are then validated and not read.  rt3_temporal_set_prev_view is still
 *      required: its view, proj and window_size are read.  Per pixel, in fp32, one rounding per operation, no contraction:
 *        foreground iff current.position.w == 1 and l2 = (n.x n.x + n.y n.y) + n.z n.z of current.normal is finite and positive; every
 *          other pixel is treated as a background pixel is: Out = In bit for bit, History = Moments = 0;
 *        P = position.xyz, n = normal.xyz * (1 / sqrt(l2)), m = max(albedo, 1/256), e = emission, c = (In - e) / m
 *          (RT3_TEMPORAL_NO_DEMODULATION: m = 1, e = 0);
 *        P is projected into the previous view as above; a tap counts when it lies inside the window, the previous set is foreground
 *          there by the same rule, PrevHistory.w > 0, dot(n, n_q) >= normal_cos and |dot(n, P_q - P)| <= plane_tolerance |P - eye|,
 *          with n_q and P_q from previous.normal and previous.position (read, not reconstructed through the previous camera);
 *        the blend and the three images written are those above.  previous.albedo and previous.emission are not read.
 *      The eight images are checked at each "temporal" launch, before anything is enqueued: live RGBA32F images of the window's size,
 *      pairwise different, none of them Out, History or Moments, else RT3_E_INVALID.  A guide input together with a motion input
 *      (rt3_temporal_set_motion_input != 0) returns RT3_E_STATE: the "motion" image is made from pinhole primary hits and does not describe
 *      the samples; moved instances and deformed meshes take rt3_temporal_set_guide_motion_input, below.  The refusal under a
 *      tile partition of several ranks stays.  Equal to tests/ref_temporal_guide.py bit for bit. ---- */
int rt3_temporal_set_guide_input(rt3_ctx *ctx, const rt3_guide_images *current, const rt3_guide_images *previous);  /* NULL, NULL: the G-buffer */
/* ---- motion under a lens: the samples' mean previous position.  No reference counterpart; DESIGN.md section 4w.
 *      rt3_camera_set_guide_motion_output names a fifth guide image, one RGBA32F image of the window's size; rt3_guide_images keeps its
 *      layout.  While it, a lens and the four-image guide output are all set, "refrence_mode" also writes it: per listed pixel, over the
 *      S camera samples in ascending order, in fp32 with one rounding per operation and no contraction, a sample that escaped adds
 *      nothing, and a sample that hit prim at (t, bu, bv) adds 1 to n_hit and R to sum_R, R chosen by the hit geometry like the "motion"
 *      pass's texel (above):
 *        the instance did not move and the geometry is not deformed:  R = o + d t, the addend of the guide's sum_P, bit for bit
 *        the instance moved:      R = prev_i * ((a w + b u) + c v), w = (1 - u) - v, over the triangle's object-space corners (the point
 *                                 itself when prev_i is exactly the identity); rt3_scene_set_prev_transforms gives prev_i
 *        the geometry is deformed: the same expression over the three records of the snapshot (rt3_scene_snapshot_vertices); prev_i = the
 *                                 current matrix when there are no previous transforms
 *      Written: {sum_R / n_hit, n_hit / S}, all zero when n_hit = 0; between batches the image holds {sum_R, n_hit}, so the bits do not
 *      depend on RT3_OPT_BATCH_SPP, RT3_OPT_INSTANCE_MODE or the tile partition.  With nothing moved and nothing deformed the image is
 *      the guide's position image bit for bit.  Light and the four guide images keep their bits.  0 switches it off, the default.
 *      RT3_E_INVALID at set time (nothing changed) for a handle that is not a live RGBA32F image.  At a "refrence_mode" launch, before
 *      anything is enqueued: RT3_E_STATE when no four-image guide output is set, or when the number of previous transforms is neither 0 nor
 *      the built structure's instance count; RT3_E_INVALID when the image has not the window's size or is one of the four guide images,
 *      Light or PrevLight.  rt3_camera_get_guide_motion_output: the handle last set (0 before any).
 *      rt3_temporal_set_guide_motion_input gives "temporal" that image, beside the two guide sets: the point projected into the previous
 *      view, and P in the plane test's P_q - P, is image.xyz instead of position.xyz; the tolerance |P - eye|, the normal and the record
 *      stay this frame's.  A foreground pixel has n_hit = S, so the point always exists.  0 (the default) = none, and an image made with
 *      nothing moved gives the bits of no input.  At a "temporal" launch: RT3_E_STATE without a guide input; RT3_E_INVALID when the image is
 *      not a live RGBA32F image of the window's size, or is one of the eight guide images, Out, History or Moments.  The refusal of a guide
 *      input together with the pinhole rt3_temporal_set_motion_input stays.  Out of scope: previous normals (a surface that turns more than
 *      acos(normal_cos) per frame loses its history), partly covered pixels, and what is seen through glass.  Equal to
 *      tests/ref_guide_motion.py bit for bit. ---- */
int rt3_camera_set_guide_motion_output(rt3_ctx *ctx, uint32_t image);   /* 0: off, the default */
int rt3_camera_get_guide_motion_output(rt3_ctx *ctx, uint32_t *image);
int rt3_temporal_set_guide_motion_input(rt3_ctx *ctx, uint32_t image);  /* 0: none, the default */
/* ---- Russian roulette on extension rays.  No reference counterpart; DESIGN.md section 4o.  By default every path that still has an extension
 *      ray is traced and shaded for all GConst.bounces vertices.  With roulette set, "refrence_mode" and "adaptive" test the extension ray that
 *      a path emitted at vertex b, for start_bounce <= b < bounces - 1, between the shading of vertex b and the trace that follows, in a
 *      kernel of its own (k_roulette), which compacts the survivors into the free half of the queue pair:
 *        m = max(T.r, T.g, T.b) of the ray's throughput (a NaN in any component makes m a NaN); !(m > 0) ends the path, no number is drawn;
 *        q = min(1, max(m, min_survival)); q >= 1: the ray goes on unchanged, no number is drawn;
 *        q_g = ceil(q 2^23) 2^-23 (the random numbers are multiples of 2^-23, so u < q <=> u < q_g and P(u < q_g) = q_g exactly);
 *        u = the number at RNG index 0x60000000 + s * bounces + b of the pixel's stream (s: absolute sample index; seed as for the path's
 *        vertices, no blue-noise shift); the ray goes on iff u < q_g, with throughput T / q_g (three IEEE divisions); its origin, direction,
 *        pdf slot (the delta markers of lens and glass included) and path id keep their bits.
 *      The estimator stays unbiased; its variance rises.  The decision depends on (pixel, frame, sample, vertex, T) alone, so a frame's bits
 *      do not depend on RT3_OPT_BATCH_SPP, the tile partition or RT3_OPT_INSTANCE_MODE.  With start_bounce >= bounces - 1 nothing is tested
 *      and the frame is the one without roulette, bit for bit.  Shadow rays and the probe passes are not tested.
 *      A non-NULL call switches this on; NULL switches it off, the default.  The state lives in the context; nothing is rebuilt.
 *      RT3_E_INVALID (nothing changed) for a min_survival that is not finite or outside [2^-7, 1], or reserved != 0.
 *      While roulette is on, "refrence_mode" and "adaptive" with samples * bounces * 8 > 2^30 return RT3_E_INVALID (the vertices' RNG indices
 *      would reach the roulette draws').  rt3_stats.extension_rays counts the rays traced: the survivors.
 *      rt3_path_get_roulette (either pointer may be NULL): the parameters last set (the defaults {2, 0.0625, {0, 0}} before any) and whether on.
 *      rt3_path_roulette_info (either pointer may be NULL; synchronises the stream): of the last "refrence_mode" or "adaptive" launch, the
 *      extension rays tested and how many of them were ended; 0 and 0 after a launch without roulette. ---- */
typedef struct rt3_roulette_params {
    uint32_t start_bounce;  /* first vertex whose extension ray is tested; vertices 0 .. start_bounce-1 always continue */
    float min_survival;     /* in [2^-7, 1]: floor of the survival probability, so a survivor's weight grows by at most 128 */
    uint32_t reserved[2];   /* 0 */
} rt3_roulette_params;
int rt3_path_set_roulette(rt3_ctx *ctx, const rt3_roulette_params *p);  /* NULL: off, the default */
int rt3_path_get_roulette(rt3_ctx *ctx, rt3_roulette_params *out, int *enabled);  /* defaults {2, 0.0625} before any call */
int rt3_path_roulette_info(rt3_ctx *ctx, uint64_t *tested, uint64_t *ended);  /* of the last refrence_mode / adaptive launch; synchronises */

/* timeline-semaphore wait of begin_frame (render_graph/mod.rs:656-665) -> hipStreamSynchronize */
int rt3_frame_wait(rt3_ctx *ctx);

/* ---- traversal on a caller-supplied ray batch (`trace()` call sites gbuffer.slang:13, refrence_mode.slang:54):
 *      rays = 8 SoA arrays of n floats (ox,oy,oz,dx,dy,dz,tmin,tmax) in HOST memory; results to host.
 *      any_hit = 0: closest hit -> t,u,v,prim ; any_hit = 1: prim[i] = 1 if occluded else 0 (t,u,v untouched).
 *      n_nodes / n_tris (may be NULL) receive per-ray traversal counts.  `repeat` > 1 re-launches the kernel for timing;
 *      *kernel_ms (may be NULL) receives the average HIP-event duration of one launch. ---- */
int rt3_trace_rays(rt3_ctx *ctx, const float *rays, uint32_t n, int any_hit, float *t, float *u, float *v, uint32_t *prim,
                   uint32_t *n_nodes, uint32_t *n_tris, int repeat, double *kernel_ms);

/* ---- device self-test: evaluates one device function per element so known-answer tests can pin the GPU arithmetic.
 *      op: 0 hash(u32) 1 zcurve(x,y) 2 murmur3(seed,index) 3 uniform_float(seed,index) 4 gbuffer pack (11 f32 -> 4 u32)
 *      5 gbuffer unpack (4 u32 -> 11 f32) 6 diffuse sample (u0,u1 -> wi) 7 orthonormal basis (n -> b1,b2) 8 AgX (rgb -> rgb)
 *      9 sincos_2pi (u -> sin,cos) 10 atan2 (y,x) 11 rng_seed(px,py,frame)
 *      12 division-free integer helpers (n,d -> n/d, n%d, wrap(int(n), (d & 0xFFFF)+1))
 *      13 octa_decode (fx,fy -> n) 14 sh3Evaluate (dir -> 9 coefficients) 15 64-lane bitonic sort (64 keys -> 64 keys, 64 lane ids)
 *      16 64-lane sum (64 floats -> 1) 17 octa_encode16 (n -> the 2 x 16-bit word of a shading-record normal) 18 octa_decode16 (word -> n)
 *      layered BSDF, material = albedo rgb, roughness, metalness; directions in the tangent frame (z = shading normal):
 *      19 bsdf_setup + bsdf_eval (material, wo, wi -> value rgb, pdf in projected solid angle)
 *      20 bsdf_setup + bsdf_sample (material, wo, u0, u1, u2 -> valid, wi, value / pdf, pdf in solid angle; zeros if not valid)
 *      21 sample_vndf (alpha, wo, u0, u1 -> half vector) 22 direction_to_equirect_uv (dir -> u, v)
 *      23 float3_to_rgb9e5 (rgb -> word) 24 rgb9e5_to_float3 (word -> rgb)
 *      sky of the context (RT3_E_STATE without one): 25 light sample (u0, u1 -> dir, radiance, pdf in solid angle, texel x, texel y)
 *      26 sky_eval_and_pdf (u, v -> bilinear radiance, pdf in solid angle).
 *      textures of the context: 27 tex_alpha (base-colour texture index as int32, u, v -> alpha in [0, 1]; 1 for an index without a texture),
 *      the alpha-mask lookup of the traversal kernels (rt3_scene_set_alpha_cutoffs).
 *      28 expn (x >= 0 -> e^-x, the polynomial of the denoise pass's edge weights).
 *      29 hit_info, the surface stage (flattened primitive id as u32, bu, bv -> Surface in op 5's 11 words: albedo, emissive, normal,
 *      roughness, metalness), read from the shading tables of the current acceleration structure in either instance mode: RT3_E_STATE
 *      without a built, current structure; RT3_E_INVALID, before anything is launched, if a row's primitive id is not below the number
 *      of flattened primitives.
 *      30 the punctual-light function of RT3_F_NEE_PUNCTUAL (light index as u32, P xyz, N xyz -> wl xyz, shadow-range end, cs = N.wl, I' rgb) for
 *      the lights of the context, from their device records (unit directions made on the device); I' is I cone window for a point or spot
 *      light (everything zero when d = 0) and E for a directional one.  RT3_E_INVALID for an index the list does not have.
 *      31 the camera sample of rt3_camera_set_lens (proj_inverse[16], view_inverse[16], window_size[2], aperture_radius, focus_distance,
 *      pixel_jitter, px, py, frame, absolute sample index as u32: 41 words -> ray origin xyz, direction xyz, film point in pixels xy, lens
 *      point in view space xy: 10 words); reads no context state.
 *      32 the glass function of rt3_scene_set_transmission (ior, thin_walled as u32, d xyz, n xyz, u: 9 words -> event as u32 (0 reflect /
 *      1 transmit), direction xyz, reflection probability F: 5 words); reads no context state.
 *      33 the roulette rule of rt3_path_set_roulette (T rgb, min_survival, u: 5 words -> survived as u32, T' rgb, q_g: 5 words; an ended row
 *      has T' = 0, a row with !(m > 0) also q_g = 0; q_g = 1: T' = T and u is not read); reads no context state.
 *      34 k_roulette itself on a caller-made queue of n records; reads no context state.  in: the header {frame, bounces, b, s0 (first sample
 *      index), min_survival, npix >= 1, workgroups to launch (1 .. 65535)}, then npix pixel words x | y << 16, then n records of 11 words
 *      {o xyz, pdf, d xyz, path id, T rgb}; path id = sample_in_batch * npix + pixel index.  out: {new count, tested, ended}, then n records:
 *      the words the caller put there are the destination queue's contents before the launch, so on return the first `count` records are
 *      the survivors and the words behind them are the caller's unless the kernel wrote out of place.
 *      35 the list compaction of the "adaptive" pass (rt3_adaptive_set_params: count, scan, scatter) on a caller-made list of n records and a
 *      caller-made mask, with the pass's own scratch layout and launch shapes; reads no context state.  in: the header {W, H, dilate (0 / 1),
 *      n}, then the window-space mask, W H bytes, row-major (byte y W + x; non-zero: the pixel's test failed), padded with zero bytes to a
 *      whole word, then n records of 2 words {x | y << 16, blue-noise word}.  out: {count, n_blocks = ceil(n / 2048)}, then the n_blocks
 *      exclusive offsets the scan left (offset b: what the list's entries before 2048 b keep), then n words and behind them n records of 2
 *      words: the destination's xy list and {xy, blue-noise} list.  As with op 34 the caller's words in both are the destination's contents
 *      before the launch: on return the first `count` entries of each are the kept ones, in the list's order, and the rest is the caller's
 *      unless a kernel wrote out of place.  An entry is kept when its pixel's mask byte is non-zero or, with dilate, any byte of the 3 x 3
 *      neighbourhood inside the window is.  RT3_E_INVALID, before anything is launched, for W or H outside 1 .. 65535, dilate > 1, n = 0,
 *      n > 2^24, a header n that is not the call's n, or a record with x >= W or y >= H.
 *      36 the absorption rule of rt3_scene_set_attenuation (T rgb, sigma rgb, t, d xyz, n xyz: 13 words -> T' rgb, applied as u32: 4 words;
 *      applied = 0: dot(n, d) <= 0 or every sigma 0, and T' = T bit for bit); reads no context state.
 *      37 k_absorb itself on a caller-made queue of n records over the built scene's tables; RT3_E_STATE without an absorption table.
 *      in: the header {workgroups to launch (1 .. 65535)}, then n records of 10 words {d xyz, t, u, v, prim (0xFFFFFFFF: a miss), T rgb}.
 *      out: T' rgb per record.  RT3_E_INVALID, before anything is launched, for a primitive the flattened world does not have.  The
 *      queue's planes are made one record longer than n and filled with a pattern: RT3_E_STATE when the kernel changed a ray or hit
 *      record or wrote behind the queue's end.
 *      39 k_lens_guide itself (rt3_camera_set_guide_output) on a caller-made camera queue, hit queue and pixel list over the built scene's
 *      tables; n = nsb * npix records.  in: the header {npix, nsb (samples in this batch), S (the frame's samples, 1 .. 2^24), first (0 / 1),
 *      last (0 / 1), workgroups to launch (1 .. 65535)}, then npix pixel words x | y << 16 (all different), then n records of 10 words
 *      {o xyz, d xyz, t, bu, bv, prim (0xFFFFFFFF: a miss)}, record sample_in_batch * npix + pixel index.  out: 16 words per listed pixel
 *      {position, normal, albedo, emission}; the words the caller put there are the images' contents before the launch (the running sums
 *      when first = 0).  The images span the list's bounding box from (0, 0).  RT3_E_INVALID, before anything is launched, for a bad
 *      header, a repeated pixel or a primitive the flattened world does not have.  Queues and images are made one record longer and
 *      filled with a pattern: RT3_E_STATE when the kernel changed a ray or hit record, a pixel that is not listed, or a word behind an end.
 *      40 the selection part of the light table on the caller-made powers of n lights, through the function, the
 *      scratch layout and the launch shapes of the context's own table; reads no context state.  The steps: pm = the largest power;
 *      q = floor(double(power) / pm * 2^24 + 0.5) (all 0 when pm = 0); prefix = the inclusive sums of q, Q the last; cdf = floor(double(prefix) /
 *      double(Q) * 2^23) (all 0 when Q = 0); mass = cdf[e] - cdf[e - 1]; w = float(mass * 2^-23) / area in fp32 where mass > 0 and area > 0,
 *      else 0; cells = the smallest power of two >= n, at most 2^20, shift = 23 - log2(cells); guide[c] = the first e with cdf[e] > c << shift
 *      (n when there is none: every power 0), guide[cells] = n - 1; the entry found for k = the first e with cdf[e] > k.  in: the header {n, n_k}, then n power words, n area
 *      words (fp32), then n_k words k.  out: {cells, shift, total = cdf[n - 1]}, then cdf[n], w[n] (the .w a record would get),
 *      guide[cells + 1] and the n_k entries light_find returns.  RT3_E_INVALID, before anything is launched, for n = 0, n > 2^24, a header n
 *      that is not the call's n, a power that is negative or not finite, a k >= 2^23, or n_k > 0 when every power is 0 (total = 0: nothing
 *      may be looked up).  Every output array is made one element longer and filled with a pattern: RT3_E_STATE when a word behind an
 *      end, or a record word other than w, changed.
 *      41 k_lens_guide_prev itself (rt3_camera_set_guide_motion_output) on caller-made queues over the built scene and the context's current
 *      motion tables (rt3_scene_set_prev_transforms, rt3_scene_snapshot_vertices; RT3_E_STATE for a wrong transform count).  The header,
 *      pixel words, records, checks and guards are op 39's.  out: 4 words per listed pixel; the words the caller put there are the image's
 *      contents before the launch.
 *      42 the emitter-side radiance of a textured-emitter table (rt3_scene_set_textured_emitters).  in: {flags}, then n rows {table entry, b1,
 *      b2}.  out: 3 words per row, Le (*) the emissive texture at barycentrics (1 - b1 - b2, b1, b2) (Le itself for an entry without texture).
 *      Ops 42 - 44 run over the light table `flags` samples (RT3_F_NEE_EMISSIVE must be in it): RT3_E_STATE when it holds no textured emitter,
 *      RT3_E_INVALID for an entry the table does not have.
 *      43 k_emit_tex itself on a caller-made emitter shadow queue of n slots.  in: the header {frame, bounces, b, s0, dims (RNG dimensions per
 *      vertex, 1 .. 8), npix, workgroups to launch (1 .. 65535), count (<= n: the queue's length word), flags}, then npix pixel words
 *      x | y << 16, then n records of 4 words {contribution r, g, b, path id}.  out: 3 words per slot, the contributions after the launch.
 *      The queue's planes are one record longer than n and filled with a pattern: RT3_E_STATE when the kernel changed an origin, a
 *      direction, a path id or a word behind the end.  Slots at and behind `count` must come back as they went in.
 *      44 the mean texel k_emit_tex_power found for every entry of the table (1 1 1 for an entry without texture).  in: {flags}; n = the table's
 *      entries.  out: 3 words per entry.
 *      45 the fog rule (rt3_scene_set_medium; reads no context state): rows {o xyz, d xyz, t, box_min xyz, box_max xyz, sigma_a rgb, sigma_s
 *      rgb, u} -> {1 when the segment runs through the box, t0, t1, s of the drawn point, its density per unit length, the segment's
 *      transmittance rgb} (zeros behind a 0).
 *      46 k_fog_segment or k_fog_shadow themselves on caller-made queues of n records, with the context's medium (RT3_E_STATE without one)
 *      over the built scene.  in: the header {kind, workgroups to launch (1 .. 65535), flags, frame, bounces, segment, s0, npix, attenuate
 *      the radiance of missed records (0 / 1)}, then npix pixel words x | y << 16, then the records.  kind 0, k_fog_segment: records
 *      {o xyz, d xyz, t, prim (0xFFFFFFFF: a miss), T rgb, path id < max(n, 1), each once}; the sky sample is on with RT3_F_NEE_SKY in `flags`
 *      and a sky, the light table is the one `flags` and `bounces` give a frame.  out: {length of queue 0, of queue 1, segments in the
 *      medium, rays queued}, 3 n words T', 4 n words of radiance slots (path id p starts as {1, 1, 1, 0}), then for each queue n slots of 12
 *      words {x, c.r, w_l, c.g, c.b, path id, tmax, 0} (a slot behind the length holds the pattern).  kind 1 / 2, k_fog_shadow on a queue
 *      without / with range ends: records {o xyz, c.r, d xyz, c.g, c.b, path id, tmax}; out: 3 words per record, the contributions after
 *      the launch.  Queues are one record longer than n and filled with a pattern: RT3_E_STATE when a kernel wrote behind an end or changed
 *      a word that is not its to change.
 *      in/out: host arrays of 32-bit words. ---- */
int rt3_selftest_eval(rt3_ctx *ctx, int op, const void *in, uint32_t n, void *out);

int rt3_stats_reset(rt3_ctx *ctx);
int rt3_stats_get(rt3_ctx *ctx, rt3_stats *out); /* synchronises the stream */

/* ---- host helpers mirroring Camera::view_matrix / projection_matrix (components/camera.rs:52-58) and the GConst fill
 *      of renderer::commands (renderer/mod.rs:72-78) ---- */
void rt3_camera_gconst(const float position[3], const float direction[3], float fov_y_radians, float aspect,
                       float z_near, float z_far, float width, float height, rt3_gconst *out);

#ifdef __cplusplus
}
#endif
#endif
