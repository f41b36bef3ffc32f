"""ctypes binding of librt3.so (include/rt3.h).  There is no CPU fallback: if the HIP library is missing or no gfx950
device is visible, every entry point raises."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("RT3_LIBRARY", PKG / "librt3.so"))  # RT3_LIBRARY: another build of the same ABI (kernel experiments)

RT3_OK = 0
E_INVALID, E_HIP, E_NO_DEVICE, E_STATE, E_UNSUPPORTED, E_DEPTH, E_COMM = -1, -2, -3, -4, -5, -6, -7
COMM_ID_BYTES = 128
TAG_BUFFER, TAG_IMAGE, TAG_ACCEL = 0, 1, 3
MISS = 0xFFFFFFFF
BACKGROUND_DEPTH = 100000.0
FORMAT_R32_SFLOAT, FORMAT_R32G32B32A32_SFLOAT, FORMAT_R32G32B32A32_UINT, FORMAT_R8G8B8A8_UNORM, FORMAT_R16_UINT = 100, 109, 107, 37, 74
F_NEE_SKY, F_BLUENOISE, F_SPECULAR, F_FACEFORWARD, F_PROBE_RADIANCE = 1, 2, 4, 8, 16
F_NEE_EMISSIVE = 32  # next-event estimation + MIS to emissive triangles; off by default
F_NEE_PUNCTUAL = 64  # next-event estimation to the punctual lights of rt3_scene_set_lights; off by default
LIGHT_POINT, LIGHT_SPOT, LIGHT_DIRECTIONAL = 0, 1, 2
SELFTEST_LIGHT = 30  # rt3_selftest_eval op: {light index (u32), P, N} -> {wl, range end, cs, I'} (8 words), the punctual-light function
OPT_BATCH_SPP, OPT_PROFILE, OPT_COUNT_TRAVERSAL, OPT_EXTEND_VARIANT, OPT_LEAF_SIZE, OPT_NODE_WIDTH, OPT_NODE_QUANT = 1, 2, 3, 4, 5, 6, 7
OPT_WIDE_COLLAPSE, OPT_POOL_CHUNK, OPT_SAH_TOP, OPT_TRACE_BLOCKS = 8, 9, 11, 12
OPT_FUSED_TRACE = 10  # retired: rt3_set_option refuses it with E_INVALID (the name stays for callers that still pass it)
OPT_INSTANCE_MODE = 14  # 0 = flatten the instances (default), 1 = two-level: shared bottom trees under a top tree
OPT_SHADOW_EXIT_TABLE = 15  # k_shadow's exit table: 0 = off, 1 = on (default), 2 = on with pseudo-random valid entries (a test aid)
OPT_DEFER_SKY_LIGHT = 16  # sky NEE: 1 = light samples are evaluated after their shadow rays, for the unoccluded ones only (default), 0 = before
OPT_SHADE_EXIT_TEST = 17  # deferred sky shadow rays: 1 = the shade kernel tries a ray's exit-table leaf and queues only undecided rays (default), 0 = k_shadow does
DENOISE_NO_DEMODULATION = 1  # rt3_denoise_params.flags: filter In as it is (not refrence_mode's Light)
TEMPORAL_NO_DEMODULATION = 1  # rt3_temporal_params.flags: the same for the "temporal" pass
SELFTEST_EXPN = 28  # rt3_selftest_eval op: x >= 0 -> e^-x, the polynomial of the denoise pass
SELFTEST_HIT_INFO = 29  # rt3_selftest_eval op: {flattened primitive (u32), bu, bv} -> Surface (11 words), hit_info of the built world
SELFTEST_LENS = 31  # rt3_selftest_eval op: {proj_inverse, view_inverse, window, lens, px, py, frame, sample} (41 words) -> {o, d, film, lens point} (10)
SELFTEST_GLASS = 32  # rt3_selftest_eval op: {ior, thin_walled (u32), d, n, u} (9 words) -> {event (u32), direction, F} (5), the glass function
SELFTEST_ROULETTE = 33  # rt3_selftest_eval op: {T rgb, min_survival, u} (5 words) -> {survived (u32), T' rgb, q_g} (5), the roulette rule
SELFTEST_ROULETTE_QUEUE = 34  # rt3_selftest_eval op: k_roulette on a caller-made queue (Context.selftest_roulette_queue)
SELFTEST_ADAPTIVE_COMPACT = 35  # rt3_selftest_eval op: the "adaptive" pass's list compaction on a caller-made list and mask (Context.selftest_adaptive_compact)
ADAPTIVE_TILE = 2048  # list entries per compaction block (op 35 returns one offset per tile)
SELFTEST_ABSORB = 36  # rt3_selftest_eval op: {T rgb, sigma rgb, t, d xyz, n xyz} (13 words) -> {T' rgb, applied (u32)} (4), the absorption rule
SELFTEST_ABSORB_QUEUE = 37  # rt3_selftest_eval op: k_absorb on a caller-made queue over the built scene (Context.selftest_absorb_queue)
SELFTEST_FROST = 38  # rt3_selftest_eval op: {ior, thin_walled (u32), d, n, alpha, u_event, u2, u3} (12 words) -> {event (u32: 0 reflect, 1 transmit, 2 invalid), direction, F, weight} (6), the frosted vertex rule
SELFTEST_GUIDE_QUEUE = 39  # rt3_selftest_eval op: k_lens_guide on caller-made camera and hit queues over the built scene (Context.selftest_guide_queue)
SELFTEST_GUIDE_PREV_QUEUE = 41  # rt3_selftest_eval op: k_lens_guide_prev on caller-made camera and hit queues over the built scene and the current motion tables (Context.selftest_guide_prev_queue)
SELFTEST_EMIT_RADIANCE = 42  # rt3_selftest_eval op: {flags}, rows {table entry, b1, b2} -> the emitter-side radiance Le (*) texture (3 words) (Context.selftest_emit_radiance)
SELFTEST_EMIT_TEX_QUEUE = 43  # rt3_selftest_eval op: k_emit_tex on a caller-made emitter shadow queue over the built scene's light table (Context.selftest_emit_tex_queue)
SELFTEST_EMIT_MEAN = 44  # rt3_selftest_eval op: the mean texel of every light-table entry, as k_emit_tex_power found it (Context.selftest_emit_mean)
SELFTEST_FOG = 45  # rt3_selftest_eval op: {o, d, t, box_min, box_max, sigma_a, sigma_s, u} (20 words) -> {in medium (u32), t0, t1, s, pdf, Tr rgb} (8), the fog rule
SELFTEST_FOG_QUEUE = 46  # rt3_selftest_eval op: k_fog_segment / k_fog_shadow on caller-made queues with the context's medium (Context.selftest_fog_segment, selftest_fog_shadow)
SELFTEST_LIGHT_TABLE = 40  # rt3_selftest_eval op: the light table's quantise / scan / CDF / guide kernels and light_find on caller-made powers (Context.selftest_light_table)

EXPORTS = [
    "rt3_create", "rt3_destroy", "rt3_last_error", "rt3_device_name", "rt3_set_option",
    "rt3_scene_set_vertices", "rt3_scene_set_indices", "rt3_scene_set_geometry", "rt3_scene_set_sky", "rt3_scene_set_bluenoise", "rt3_scene_set_texture",
    "rt3_scene_set_alpha_cutoffs",
    "rt3_scene_set_material_textures",
    "rt3_scene_set_transmission", "rt3_scene_set_attenuation", "rt3_attenuation_info",
    "rt3_scene_set_pane_shadows", "rt3_scene_get_pane_shadows", "rt3_pane_shadow_info",
    "rt3_scene_set_rough_transmission", "rt3_scene_get_rough_transmission", "rt3_rough_transmission_info",
    "rt3_scene_set_instances",
    "rt3_accel_build", "rt3_accel_info", "rt3_accel_levels", "rt3_accel_exit_table_info", "rt3_accel_download", "rt3_accel_import", "rt3_sky_download",
    "rt3_scene_update_vertices", "rt3_accel_refit", "rt3_light_info", "rt3_light_download",
    "rt3_buffer_create", "rt3_image_create", "rt3_image_import", "rt3_resource_upload", "rt3_resource_download", "rt3_resource_device_ptr",
    "rt3_set_tile_partition", "rt3_tile_pixel_count", "rt3_image_pack_tiles", "rt3_image_unpack_tiles",
    "rt3_comm_version", "rt3_comm_unique_id", "rt3_comm_init", "rt3_comm_destroy", "rt3_gather_tiles", "rt3_gather_layout", "rt3_gather_unpack",
    "rt3_pass_launch", "rt3_denoise_set_params", "rt3_denoise_set_variance_input", "rt3_temporal_set_prev_view", "rt3_temporal_set_params",
    "rt3_scene_set_prev_transforms", "rt3_temporal_set_motion_input",
    "rt3_adaptive_set_params", "rt3_adaptive_info", "rt3_adaptive_set_coverage", "rt3_adaptive_get_coverage",
    "rt3_camera_set_lens", "rt3_camera_get_lens",
    "rt3_camera_set_guide_output", "rt3_camera_get_guide_output", "rt3_denoise_set_guide_input", "rt3_temporal_set_guide_input",
    "rt3_camera_set_guide_motion_output", "rt3_camera_get_guide_motion_output", "rt3_temporal_set_guide_motion_input",
    "rt3_path_set_roulette", "rt3_path_get_roulette", "rt3_path_roulette_info",
    "rt3_scene_set_lights", "rt3_light_masses", "rt3_light_table",
    "rt3_scene_set_textured_emitters", "rt3_scene_get_textured_emitters", "rt3_light_emit_tex",
    "rt3_scene_set_medium", "rt3_scene_get_medium", "rt3_medium_info",
    "rt3_scene_snapshot_vertices", "rt3_scene_forget_prev_vertices", "rt3_scene_deformed_geometries",
    "rt3_scene_add_skin", "rt3_scene_clear_skins", "rt3_scene_pose_skin", "rt3_skin_info", "rt3_scene_download_vertices",
    "rt3_frame_wait", "rt3_trace_rays", "rt3_selftest_eval", "rt3_stats_reset", "rt3_stats_get", "rt3_camera_gconst",
]


class GConst(C.Structure):
    """src/renderer/mod.rs:47-63 / shaders/include/datatypes.slang:28-43 (304 bytes, column-major matrices)."""

    _fields_ = [("proj", C.c_float * 16), ("view", C.c_float * 16), ("proj_inverse", C.c_float * 16), ("view_inverse", C.c_float * 16),
                ("window_size", C.c_float * 2), ("frame", C.c_uint32), ("blendfactor", C.c_float), ("bounces", C.c_uint32),
                ("samples", C.c_uint32), ("proberng", C.c_uint32), ("cell_size", C.c_float), ("mouse", C.c_uint32 * 2), ("pad", C.c_uint32 * 2)]


class Stats(C.Structure):
    _fields_ = [("extension_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("nodes_visited", C.c_uint64), ("tris_tested", C.c_uint64),
                ("shadow_nodes_visited", C.c_uint64), ("shadow_tris_tested", C.c_uint64),
                ("extend_launches", C.c_uint64), ("extend_ms", C.c_double), ("shadow_launches", C.c_uint64), ("shadow_ms", C.c_double),
                ("shade_ms", C.c_double), ("other_ms", C.c_double),
                ("trace_launches", C.c_uint64), ("trace_ms", C.c_double), ("trace_rays", C.c_uint64 * 2), ("trace_nodes", C.c_uint64 * 2),
                ("trace_tris", C.c_uint64 * 2), ("gather_ms", C.c_double), ("nodes_visited_lds", C.c_uint64), ("shadow_nodes_visited_lds", C.c_uint64), ("accel_build_ms", C.c_double), ("accel_bulk_copies", C.c_uint64),
                ("accel_arena_serial", C.c_uint64), ("emit_tex_launches", C.c_uint64)]


class Instance(C.Structure):
    """rt3_instance: Instance{model} + Transform{Mat4} (src/renderer/world/mod.rs:34-60); transform column-major like glam's Mat4."""

    _fields_ = [("geometry_first", C.c_uint32), ("geometry_count", C.c_uint32), ("transform", C.c_float * 16)]


class DenoiseParams(C.Structure):
    """rt3_denoise_params: the "denoise" pass.  The defaults are the library's."""

    _fields_ = [("iterations", C.c_uint32), ("normal_squarings", C.c_uint32), ("sigma_z", C.c_float), ("sigma_l", C.c_float), ("flags", C.c_uint32)]

    def __init__(self, iterations=5, normal_squarings=7, sigma_z=0.05, sigma_l=4.0, flags=0):
        super().__init__(iterations, normal_squarings, sigma_z, sigma_l, flags)


class TemporalParams(C.Structure):
    """rt3_temporal_params: the "temporal" pass.  The defaults are the library's."""

    _fields_ = [("alpha", C.c_float), ("alpha_moments", C.c_float), ("max_history", C.c_uint32), ("normal_cos", C.c_float),
                ("plane_tolerance", C.c_float), ("flags", C.c_uint32)]

    def __init__(self, alpha=0.2, alpha_moments=0.2, max_history=32, normal_cos=0.9, plane_tolerance=0.01, flags=0):
        super().__init__(alpha, alpha_moments, max_history, normal_cos, plane_tolerance, flags)


class AdaptiveParams(C.Structure):
    """rt3_adaptive_params: the "adaptive" pass.  The defaults are the library's."""

    _fields_ = [("min_samples", C.c_uint32), ("step", C.c_uint32), ("threshold", C.c_float), ("dark", C.c_float), ("dilate", C.c_uint32),
                ("flags", C.c_uint32)]

    def __init__(self, min_samples=16, step=16, threshold=0.05, dark=0.01, dilate=1, flags=0):
        super().__init__(min_samples, step, threshold, dark, dilate, flags)


class LensParams(C.Structure):
    """rt3_lens_params: per-sample camera rays.  The defaults are antialiasing over the whole pixel, no aperture."""

    _fields_ = [("aperture_radius", C.c_float), ("focus_distance", C.c_float), ("pixel_jitter", C.c_float), ("reserved", C.c_uint32)]

    def __init__(self, aperture_radius=0.0, focus_distance=1.0, pixel_jitter=1.0, reserved=0):
        super().__init__(aperture_radius, focus_distance, pixel_jitter, reserved)


class GuideImages(C.Structure):
    """rt3_guide_images: the handles of the four RGBA32F guide images of a lens frame."""

    _fields_ = [("position", C.c_uint32), ("normal", C.c_uint32), ("albedo", C.c_uint32), ("emission", C.c_uint32)]

    def __init__(self, position=0, normal=0, albedo=0, emission=0):
        super().__init__(position, normal, albedo, emission)

    def handles(self):
        return (self.position, self.normal, self.albedo, self.emission)


class RouletteParams(C.Structure):
    """rt3_roulette_params: Russian roulette on extension rays.  The defaults are the library's."""

    _fields_ = [("start_bounce", C.c_uint32), ("min_survival", C.c_float), ("reserved", C.c_uint32 * 2)]

    def __init__(self, start_bounce=2, min_survival=0.0625, reserved=(0, 0)):
        super().__init__(start_bounce, min_survival, (C.c_uint32 * 2)(*reserved))


class Medium(C.Structure):
    """rt3_medium: one axis-aligned box of homogeneous medium with single scattering: absorption and scattering
    coefficients per colour channel and world unit, the Henyey-Greenstein asymmetry g in (-1, 1), and the box."""

    _fields_ = [("sigma_a", C.c_float * 3), ("sigma_s", C.c_float * 3), ("g", C.c_float), ("box_min", C.c_float * 3), ("box_max", C.c_float * 3)]

    def __init__(self, sigma_a=(0.0, 0.0, 0.0), sigma_s=(0.0, 0.0, 0.0), g=0.0, box_min=(-1.0, -1.0, -1.0), box_max=(1.0, 1.0, 1.0)):
        def three(v):
            v = (v, v, v) if isinstance(v, (int, float)) else tuple(v)
            return (C.c_float * 3)(*[float(x) for x in v])
        super().__init__(three(sigma_a), three(sigma_s), float(g), three(box_min), three(box_max))


SKIN_MAX_TARGETS = 8  # RT3_SKIN_MAX_TARGETS


class SkinDesc(C.Structure):
    """rt3_skin_desc: one skin of rt3_scene_add_skin: the vertex range it writes, and tight host arrays borrowed for
    the call."""

    _fields_ = [("first_vertex", C.c_uint32), ("n_vertices", C.c_uint32), ("n_joints", C.c_uint32), ("n_targets", C.c_uint32),
                ("rest", C.c_void_p), ("joints", C.c_void_p), ("weights", C.c_void_p), ("target_dpos", C.c_void_p), ("target_dnrm", C.c_void_p)]


assert C.sizeof(SkinDesc) == 56
assert C.sizeof(Medium) == 52
assert C.sizeof(GConst) == 304


def kernel_source_hash() -> str:
    """sha256 (16 hex digits) over the sources librt3.so is built from.  tools/summarize_profile.py writes it into a counter profile,
    bench.py quotes a profile only when it matches the tree it runs from: counters of other kernels are not evidence for these."""
    import hashlib

    h = hashlib.sha256()
    files = sorted((PKG / "csrc").glob("*.hip")) + sorted((PKG / "csrc").glob("*.hpp")) + sorted((PKG / "csrc").glob("*.inc")) + [PKG / "csrc" / "Makefile", PKG.parent / "include" / "rt3.h"]
    for f in files:
        h.update(f.name.encode())
        h.update(f.read_bytes())
    return h.hexdigest()[:16]


class Rt3Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rt3 error {code}: {msg}")
        self.code = code


_lib = None


def load():
    """Load librt3.so (built by __graft_entry__.build() / `make -C raytracer3_amd/csrc`)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).  Import it first so that the
    # loader resolves librt3's NEEDED libamdhip64.so.7 to that already-loaded copy: two HIP runtimes in one process
    # cannot both open the GPU ("No HIP GPUs are available").  Without torch, librt3 uses /opt/rocm's runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not LIB_PATH.exists():
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C {PKG / 'csrc'}` (hipcc, gfx950). There is no CPU fallback.")
    L = C.CDLL(str(LIB_PATH))
    vp, u32, i32, f32, sz = C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_size_t
    pu32 = C.POINTER(C.c_uint32)
    sig = {
        "rt3_create": (i32, [i32, C.POINTER(vp)]),
        "rt3_destroy": (None, [vp]),
        "rt3_last_error": (C.c_char_p, [vp]),
        "rt3_device_name": (i32, [vp, C.c_char_p, sz]),
        "rt3_set_option": (i32, [vp, i32, C.c_int64]),
        "rt3_scene_set_vertices": (i32, [vp, vp, u32]),
        "rt3_scene_set_indices": (i32, [vp, vp, u32]),
        "rt3_scene_set_geometry": (i32, [vp, vp, vp, u32]),
        "rt3_scene_set_sky": (i32, [vp, vp, u32, u32]),
        "rt3_scene_set_bluenoise": (i32, [vp, vp, u32, u32]),
        "rt3_scene_set_texture": (i32, [vp, u32, vp, u32, u32]),
        "rt3_scene_set_alpha_cutoffs": (i32, [vp, vp, u32]),
        "rt3_scene_set_material_textures": (i32, [vp, vp, u32]),
        "rt3_scene_set_transmission": (i32, [vp, vp, u32]),
        "rt3_scene_set_attenuation": (i32, [vp, vp, u32]),
        "rt3_attenuation_info": (i32, [vp, pu32]),
        "rt3_scene_set_pane_shadows": (i32, [vp, i32]),
        "rt3_scene_get_pane_shadows": (i32, [vp, C.POINTER(i32)]),
        "rt3_pane_shadow_info": (i32, [vp, C.POINTER(u32)]),
        "rt3_scene_set_rough_transmission": (i32, [vp, i32]),
        "rt3_scene_get_rough_transmission": (i32, [vp, C.POINTER(i32)]),
        "rt3_rough_transmission_info": (i32, [vp, C.POINTER(u32)]),
        "rt3_scene_set_instances": (i32, [vp, vp, u32]),
        "rt3_accel_build": (i32, [vp, pu32]),
        "rt3_accel_info": (i32, [vp, pu32, pu32, pu32, pu32]),
        "rt3_accel_levels": (i32, [vp, pu32, pu32, pu32, C.POINTER(C.c_uint64)]),
        "rt3_accel_exit_table_info": (i32, [vp, pu32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), pu32]),
        "rt3_accel_download": (i32, [vp, vp, sz, vp, sz]),
        "rt3_accel_import": (i32, [vp, vp, sz, vp, sz]),
        "rt3_sky_download": (i32, [vp, vp, vp, vp, vp]),
        "rt3_scene_update_vertices": (i32, [vp, vp, u32, u32]),
        "rt3_accel_refit": (i32, [vp, pu32]),
        "rt3_light_info": (i32, [vp, pu32, C.POINTER(C.c_uint64)]),
        "rt3_light_download": (i32, [vp, vp, vp, vp]),
        "rt3_buffer_create": (i32, [vp, sz, pu32]),
        "rt3_image_create": (i32, [vp, u32, u32, u32, pu32]),
        "rt3_image_import": (i32, [vp, vp, u32, u32, u32, pu32]),
        "rt3_resource_upload": (i32, [vp, u32, vp, sz]),
        "rt3_resource_download": (i32, [vp, u32, vp, sz]),
        "rt3_resource_device_ptr": (i32, [vp, u32, C.POINTER(vp), C.POINTER(sz)]),
        "rt3_set_tile_partition": (i32, [vp, u32, u32, u32, u32]),
        "rt3_tile_pixel_count": (i32, [vp, u32, u32, pu32]),
        "rt3_image_pack_tiles": (i32, [vp, u32, u32, u32, vp]),
        "rt3_image_unpack_tiles": (i32, [vp, u32, u32, u32, vp]),
        "rt3_comm_version": (i32, [C.POINTER(i32)]),
        "rt3_comm_unique_id": (i32, [vp]),
        "rt3_comm_init": (i32, [vp, vp, u32, u32]),
        "rt3_comm_destroy": (i32, [vp]),
        "rt3_gather_tiles": (i32, [vp, u32, u32]),
        "rt3_gather_layout": (i32, [vp, u32, u32, u32, C.POINTER(C.c_uint64)]),
        "rt3_gather_unpack": (i32, [vp, u32, u32, u32, vp]),
        "rt3_pass_launch": (i32, [vp, C.c_char_p, C.c_char_p, u32, u32, u32, vp, sz, pu32, u32]),
        "rt3_denoise_set_params": (i32, [vp, C.POINTER(DenoiseParams)]),
        "rt3_denoise_set_variance_input": (i32, [vp, u32]),
        "rt3_temporal_set_prev_view": (i32, [vp, vp, sz]),
        "rt3_temporal_set_params": (i32, [vp, C.POINTER(TemporalParams)]),
        "rt3_scene_set_prev_transforms": (i32, [vp, vp, u32]),
        "rt3_scene_set_lights": (i32, [vp, vp, u32]),
        "rt3_light_masses": (i32, [vp, u32, pu32, pu32, vp]),
        "rt3_light_table": (i32, [vp, u32, vp, vp, vp, vp, vp, pu32, pu32]),
        "rt3_scene_set_textured_emitters": (i32, [vp, i32]),
        "rt3_scene_get_textured_emitters": (i32, [vp, C.POINTER(i32)]),
        "rt3_light_emit_tex": (i32, [vp, u32, pu32, vp]),
        "rt3_temporal_set_motion_input": (i32, [vp, u32]),
        "rt3_adaptive_set_params": (i32, [vp, C.POINTER(AdaptiveParams)]),
        "rt3_adaptive_info": (i32, [vp, pu32, C.POINTER(C.c_uint64), pu32]),
        "rt3_adaptive_set_coverage": (i32, [vp, i32]),
        "rt3_adaptive_get_coverage": (i32, [vp, C.POINTER(i32)]),
        "rt3_camera_set_lens": (i32, [vp, C.POINTER(LensParams)]),
        "rt3_camera_get_lens": (i32, [vp, C.POINTER(LensParams), C.POINTER(i32)]),
        "rt3_camera_set_guide_output": (i32, [vp, C.POINTER(GuideImages)]),
        "rt3_camera_get_guide_output": (i32, [vp, C.POINTER(GuideImages), C.POINTER(i32)]),
        "rt3_denoise_set_guide_input": (i32, [vp, C.POINTER(GuideImages)]),
        "rt3_temporal_set_guide_input": (i32, [vp, C.POINTER(GuideImages), C.POINTER(GuideImages)]),
        "rt3_camera_set_guide_motion_output": (i32, [vp, u32]),
        "rt3_camera_get_guide_motion_output": (i32, [vp, C.POINTER(u32)]),
        "rt3_temporal_set_guide_motion_input": (i32, [vp, u32]),
        "rt3_path_set_roulette": (i32, [vp, C.POINTER(RouletteParams)]),
        "rt3_path_get_roulette": (i32, [vp, C.POINTER(RouletteParams), C.POINTER(i32)]),
        "rt3_path_roulette_info": (i32, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "rt3_scene_set_medium": (i32, [vp, vp]),
        "rt3_scene_get_medium": (i32, [vp, vp, C.POINTER(C.c_int)]),
        "rt3_medium_info": (i32, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "rt3_scene_snapshot_vertices": (i32, [vp]),
        "rt3_scene_forget_prev_vertices": (i32, [vp]),
        "rt3_scene_deformed_geometries": (i32, [vp, vp, u32]),
        "rt3_scene_add_skin": (i32, [vp, C.POINTER(SkinDesc), pu32]),
        "rt3_scene_clear_skins": (i32, [vp]),
        "rt3_scene_pose_skin": (i32, [vp, u32, vp, vp]),
        "rt3_skin_info": (i32, [vp, pu32, C.POINTER(C.c_uint64)]),
        "rt3_scene_download_vertices": (i32, [vp, vp, u32, u32]),
        "rt3_frame_wait": (i32, [vp]),
        "rt3_trace_rays": (i32, [vp, vp, u32, i32, vp, vp, vp, vp, vp, vp, i32, C.POINTER(C.c_double)]),
        "rt3_selftest_eval": (i32, [vp, i32, vp, u32, vp]),
        "rt3_stats_reset": (i32, [vp]),
        "rt3_stats_get": (i32, [vp, C.POINTER(Stats)]),
        "rt3_camera_gconst": (None, [C.POINTER(f32), C.POINTER(f32), f32, f32, f32, f32, f32, f32, C.POINTER(GConst)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError here == a symbol include/rt3.h declares is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L
