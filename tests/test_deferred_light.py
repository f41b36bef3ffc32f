"""Deferred sky light samples (RT3_OPT_DEFER_SKY_LIGHT): with the option at 1, k_shade_defer sends a sky shadow ray with
nothing but the vertex's place in its queue, k_shadow reports occlusion, and k_light evaluates radiance, BSDF and weight for the rays that
came through.  The option may change no bit of a frame and no ray count: every comparison here is exact -- `Light` as uint32 and the
extension / shadow ray counts of rt3_stats between option 1 and option 0 (the parent's kernels and launch order), and one frame of each
family against the oracle's reference_mode as well.  The families: the bounce counts and estimator flag sets; the features that share the
queues k_light reads (emitter NEE, a lens, roulette from bounce 0, one sample per batch, a tile partition, the exit table, the LDS geometry
table and its global twin, the adaptive pass); the edges of k_light's packing (one pixel, queue lengths that are no multiple of a wave or a
workgroup, a closed room whose rays are occluded, an open floor whose rays all come through, no shadow ray at all); scenes outside the cover, which keep the parent's path; and the ledger of
the new kernels' instances."""
import functools
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import integrator_worlds as iw
import material_worlds as mw
import orc
import punctual_worlds as pw
from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from raytracer3_amd.renderer import Camera, PathTracer
from support import as_orc, bits

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HERE = "tests/test_deferred_light.py"
FULL = L.F_NEE_SKY | L.F_BLUENOISE | L.F_SPECULAR | L.F_FACEFORWARD
FLAG_SETS = {
    "full": FULL,
    "no_specular": FULL & ~L.F_SPECULAR,
    "no_bluenoise": FULL & ~L.F_BLUENOISE,
    "no_faceforward": FULL & ~L.F_FACEFORWARD,
}
SMALL = (37, 29)  # x 3 spp = 3219 paths: no multiple of 64 or 512, seven workgroups of k_shade_defer, one of k_light with seven trips
WIDE = (96, 64)   # x 3 spp = 18432 paths: five workgroups of k_light
LDS_GEOMS = 256   # kShadeGeomsLds (rt3_surface.hpp)


@functools.lru_cache(maxsize=None)
def world(name):
    """(mesh, camera dictionary)"""
    if name == "atrium":
        return scenes.atrium(0.2), scenes.ATRIUM_CAMERA
    if name == "cornell":
        return scenes.cornell(), scenes.CORNELL_CAMERA
    if name == "open_room":  # floor, two walls, a block and an emissive panel under an open sky
        return iw.open_room(True), iw.ROOM_CAMERA
    if name == "closed_box":  # the camera inside a closed room: the sky shadow rays of what the camera sees are all occluded (test_closed_room)
        room, _, cam = iw.furnace(1.0)
        return room, cam
    if name == "open_floor":  # one quad facing the sky, nothing above it: every sky shadow ray comes through
        return pw.floor_world(), pw.FLOOR_CAMERA
    if name == "background":  # the same quad behind the camera: no vertex, no shadow ray
        return pw.floor_world(), dict(position=(0.0, 2.4, 0.8), direction=(0.0, 1.0, 0.3), fov_deg=70.0)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def sky_and_noise():
    return scenes.sky(256, 128), assets.load_bluenoise()


def camera(cam_kw, window):
    return Camera(cam_kw["position"], cam_kw["direction"], math.radians(cam_kw["fov_deg"]), window[0] / window[1])


def by_option(name, window=SMALL, *, spp=3, bounces=4, flags=FULL, options=(), setup=None, rank=0, n_ranks=1, instances=None, mesh=None, adaptive=None):
    """{option: (Light, extension rays, shadow rays)} of one frame with RT3_OPT_DEFER_SKY_LIGHT at 1 and at 0, on one PathTracer, plus
    the frame's GConst and G-buffer: (frames, g, gbuffer, depth)"""
    base, cam_kw = world(name)
    sk, bn = sky_and_noise()
    pt = PathTracer(window, rank=rank, n_ranks=n_ranks)
    try:
        pt.set_scene(base if mesh is None else mesh, sk, bn, instances=instances, options=options)
        if setup:
            setup(pt)
        g = pt.make_gconst(camera(cam_kw, window), samples=spp, bounces=bounces, frame=1, flags=flags)
        out = {}
        for opt in (1, 0):
            pt.ctx.set_option(L.OPT_DEFER_SKY_LIGHT, opt)
            pt.ctx.stats_reset()
            pt.render(g, adaptive=adaptive)
            st = pt.ctx.stats()
            out[opt] = (pt.light(), int(st.extension_rays), int(st.shadow_rays))
        gb, depth = pt.gbuffer()
    finally:
        pt.close()
    return out, g, gb, depth


def same_by_option(tag, out):
    (l1, e1, s1), (l0, e0, s0) = out[1], out[0]
    print(f"{tag}: extension rays {e1} / {e0}, shadow rays {s1} / {s0}, mean {float(l1[..., :3].mean()):.6g}")
    assert (e1, s1) == (e0, s0), (tag, "ray counts", (e1, s1), (e0, s0))
    diff = (bits(l1) != bits(l0)).any(-1)
    assert not diff.any(), (tag, int(diff.sum()), "pixels differ, first at", np.argwhere(diff)[:3].tolist())
    return l1, e1, s1


def against_oracle(tag, name, light, g, depth, mesh=None, lit=True):
    sk, bn = sky_and_noise()
    osc = orc.Scene(world(name)[0] if mesh is None else mesh, sk, bn)
    og = as_orc(g)
    ogb, odepth = osc.gbuffer(og)
    assert np.array_equal(bits(depth), bits(odepth)), tag
    olight, _ = osc.reference_mode(og, ogb, odepth)
    assert np.array_equal(bits(light), bits(olight)), tag
    assert not lit or float(olight[..., :3].mean()) > 0.0, tag


# ---------------------------------------------------------------------------------------------------------------- 1. option 1 against option 0
@pytest.mark.parametrize("bounces", [1, 2, 4])
@pytest.mark.parametrize("flag_set", list(FLAG_SETS))
def test_option_changes_nothing(flag_set, bounces):
    for name in ("atrium", "cornell"):
        out, g, _, depth = by_option(name, bounces=bounces, flags=FLAG_SETS[flag_set])
        light, _, shadow = same_by_option((name, flag_set, bounces), out)
        assert shadow > 0, (name, flag_set, bounces)
        if flag_set == "full" and bounces == 4:
            against_oracle((name, flag_set, bounces), name, light, g, depth)


def test_several_workgroups_of_k_light():
    out, g, _, depth = by_option("atrium", WIDE)
    light, _, shadow = same_by_option("atrium wide", out)
    assert shadow > 4 * 4096  # more than four of k_light's workgroups have slots to look at
    against_oracle("atrium wide", "atrium", light, g, depth)


# ---------------------------------------------------------------------------------------------------------------- 2. with other features on
def test_emitter_nee_keeps_the_add_order():
    """the emitter queue's k_shadow adds into the same radiance slots after the sky's: k_light runs between the two"""
    for name in ("cornell", "atrium"):
        out, _, _, _ = by_option(name, flags=FULL | L.F_NEE_EMISSIVE)
        same_by_option((name, "emitter NEE"), out)
    out, _, _, _ = by_option("open_room", (48, 32), flags=FULL | L.F_NEE_EMISSIVE)  # an emitter that is sampled and seen under an open sky
    light, _, _ = same_by_option("open room, emitter NEE", out)
    assert float(light[..., :3].mean()) > 0.0


def test_lens_frame():
    """vertex 0 through the FIRST = false instances, its queue's length read on the device"""
    for name in ("atrium", "cornell"):
        out, _, _, _ = by_option(name, setup=lambda pt: pt.set_lens(0.05, 3.0, 1.0))
        _, _, shadow = same_by_option((name, "lens"), out)
        assert shadow > 0


def test_roulette_from_bounce_0():
    """k_roulette overwrites the half of the ray pair k_shade_defer read: k_light has read it by then"""
    for name in ("atrium", "cornell"):
        out, _, _, _ = by_option(name, setup=lambda pt: pt.set_roulette(0, 0.0625))
        same_by_option((name, "roulette"), out)
        out, _, _, _ = by_option(name, flags=FULL | L.F_NEE_EMISSIVE, setup=lambda pt: (pt.set_roulette(0, 0.0625), pt.set_lens(0.05, 3.0, 1.0)))
        same_by_option((name, "roulette, lens, emitter NEE"), out)


def test_one_sample_per_batch():
    out, g, _, depth = by_option("atrium", options=[(L.OPT_BATCH_SPP, 1)])
    light, _, _ = same_by_option("batch spp 1", out)
    against_oracle("batch spp 1", "atrium", light, g, depth)


def test_three_rank_tile_partition():
    window = (160, 96)  # 3 x 2 tiles of 64 x 64 (the right column and the lower row cut), two per rank
    whole = None
    for rank in range(3):
        out, g, _, _ = by_option("atrium", window, spp=2, rank=rank, n_ranks=3)
        light, _, shadow = same_by_option(("rank", rank), out)
        assert shadow > 0, rank
        whole = light.copy() if whole is None else np.where(light != 0, light, whole)
    out, _, _, _ = by_option("atrium", window, spp=2)
    assert np.array_equal(bits(whole), bits(out[1][0]))


@pytest.mark.parametrize("table", [0, 1])
def test_exit_table(table):
    out, g, _, depth = by_option("atrium", options=[(L.OPT_SHADOW_EXIT_TABLE, table)])
    light, _, _ = same_by_option(("exit table", table), out)
    against_oracle(("exit table", table), "atrium", light, g, depth)


@pytest.mark.parametrize("mode", [0, 1])
def test_geometry_table_outside_lds(mode):
    """more flattened geometries than the LDS table holds: the GLDS = false instances; mode 1: under the two-level structure"""
    base, _ = world("cornell")
    big, inst = mw.padded(base, LDS_GEOMS + 1)
    for flags in (FULL, FULL | L.F_NEE_EMISSIVE):
        out, g, _, depth = by_option("cornell", mesh=big, instances=inst, flags=flags, options=[(L.OPT_INSTANCE_MODE, mode)])
        light, _, shadow = same_by_option(("padded", mode, flags), out)
        assert shadow > 0
    small, _, _, _ = by_option("cornell", flags=FULL | L.F_NEE_EMISSIVE)
    assert np.array_equal(bits(light), bits(small[1][0]))  # the padding changes no frame


def test_adaptive_pass():
    p = L.AdaptiveParams(min_samples=2, step=2, threshold=0.05, dark=0.01, dilate=1)
    out, _, _, _ = by_option("atrium", spp=6, adaptive=p)
    _, _, shadow = same_by_option("adaptive", out)
    assert shadow > 0


# ---------------------------------------------------------------------------------------------------------------- 3. the edges of the packing
def test_one_pixel():
    for name in ("atrium", "open_floor"):
        out, g, _, depth = by_option(name, (1, 1))
        light, _, shadow = same_by_option((name, "1 x 1"), out)
        assert shadow > 0, name
        against_oracle((name, "1 x 1"), name, light, g, depth, lit=False)  # (three samples of one pixel may all find shade)


@pytest.mark.parametrize("window,spp", [((9, 7), 1), ((13, 5), 1), ((31, 17), 1), ((37, 29), 3), ((64, 8), 1), ((64, 64), 1)])
def test_queue_lengths(window, spp):
    """63, 65, 527 and 3219 paths, and exactly one and eight workgroups' worth"""
    out, g, _, depth = by_option("atrium", window, spp=spp)
    light, _, _ = same_by_option(("atrium", window, spp), out)
    against_oracle(("atrium", window, spp), "atrium", light, g, depth)


def test_closed_room():
    out, g, _, depth = by_option("closed_box")
    light, _, shadow = same_by_option("closed box", out)
    assert shadow > 0
    against_oracle("closed box", "closed_box", light, g, depth)
    # one vertex per path: every surface emits E = (3, 1.5, 6), so a pixel is exactly E unless a sky shadow ray came through and added to it.
    # It is E everywhere: k_light found no survivor in any of its trips.
    out, _, _, depth = by_option("closed_box", bounces=1)
    light, _, shadow = same_by_option("closed box, one vertex", out)
    assert shadow > 0 and (depth != np.float32(L.BACKGROUND_DEPTH)).all()
    assert (light[..., :3] == np.float32([3.0, 1.5, 6.0])).all()


def test_every_ray_survives():
    out, g, _, depth = by_option("open_floor", bounces=1)
    light, _, shadow = same_by_option("open floor", out)
    against_oracle("open floor", "open_floor", light, g, depth)
    lit = depth != np.float32(L.BACKGROUND_DEPTH)
    assert shadow > 0 and lit.any() and float(light[..., :3][lit].sum()) > 0.0


def test_no_shadow_ray_at_all():
    out, _, _, depth = by_option("background")
    light, _, shadow = same_by_option("background", out)
    assert (depth == np.float32(L.BACKGROUND_DEPTH)).all() and shadow == 0 and not light.any()


# ---------------------------------------------------------------------------------------------------------------- 4. outside the cover
def test_glass_and_punctual_scenes_keep_their_frames():
    out, _, _, _ = by_option("cornell", (48, 36), mesh=scenes.glass_cornell(), flags=FULL | L.F_NEE_EMISSIVE)
    light, _, _ = same_by_option("glass", out)
    assert float(light[..., :3].mean()) > 0.0
    mesh, _ = pw.room("spot_sun_b4")
    out, _, _, _ = by_option("open_room", (48, 32), mesh=mesh, flags=FULL | L.F_NEE_PUNCTUAL)
    light, _, _ = same_by_option("punctual", out)
    plain, _, _, _ = by_option("open_room", (48, 32), mesh=mesh, flags=FULL)
    assert (bits(light) != bits(plain[1][0])).any()  # the lights are sampled


def test_material_textures_keep_their_frames():
    out, _, _, _ = by_option("cornell", (48, 36), mesh=scenes.material_cornell())
    light, _, shadow = same_by_option("material textures", out)
    assert shadow > 0 and float(light[..., :3].mean()) > 0.0


def test_option_values():
    pt = PathTracer((8, 8))
    try:
        for bad in (-1, 2):
            assert pt.ctx.lib.rt3_set_option(pt.ctx.h, L.OPT_DEFER_SKY_LIGHT, bad) == L.E_INVALID
        for good in (0, 1):
            pt.ctx.set_option(L.OPT_DEFER_SKY_LIGHT, good)
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 5. the new kernels' instances
# name -> (what selects it, the test here that runs it).  FIRST: vertex 0 from the G-buffer; GLDS: at most 256 flattened geometries;
# EMIT: RT3_F_NEE_EMISSIVE with emitters.  k_light has no EMIT: the emitter sample is k_shade_defer's.
LEDGER = {
    "k_shade_defer<true, false, false>": ("vertex 0 of a frame without a lens", f"{HERE}::test_option_changes_nothing"),
    "k_shade_defer<true, false, true>": ("the same with emitter NEE", f"{HERE}::test_emitter_nee_keeps_the_add_order"),
    "k_shade_defer<false, true, false>": ("later vertices, and vertex 0 of a lens frame", f"{HERE}::test_lens_frame"),
    "k_shade_defer<false, true, true>": ("the same with emitter NEE", f"{HERE}::test_roulette_from_bounce_0"),
    "k_shade_defer<false, false, false>": ("later vertices of a scene of more than 256 geometries", f"{HERE}::test_geometry_table_outside_lds"),
    "k_shade_defer<false, false, true>": ("the same with emitter NEE", f"{HERE}::test_geometry_table_outside_lds"),
    "k_light<true, false>": ("behind k_shade_defer<true, false, *>", f"{HERE}::test_option_changes_nothing"),
    "k_light<false, true>": ("behind k_shade_defer<false, true, *>", f"{HERE}::test_lens_frame"),
    "k_light<false, false>": ("behind k_shade_defer<false, false, *>", f"{HERE}::test_geometry_table_outside_lds"),
}


def library_instances():
    lib = ROOT / "raytracer3_amd" / "librt3.so"
    out = None
    for nm in ("nm", "/opt/rocm/llvm/bin/llvm-nm"):
        try:
            out = subprocess.run([nm, "-C", str(lib)], capture_output=True, text=True, check=True).stdout
            break
        except (OSError, subprocess.CalledProcessError):
            continue
    assert out is not None, "neither nm nor llvm-nm could read the library"
    return set(re.findall(r"__device_stub__((?:k_shade_defer|k_light)<[^>]*>)\(", out))


def test_own_instance_ledger():
    """fails when an instance of k_shade_defer or k_light is added without an entry here, or an entry outlives its instance or its test"""
    have = library_instances()
    assert not have - set(LEDGER), f"instances without a ledger entry: {sorted(have - set(LEDGER))}"
    assert not set(LEDGER) - have, f"ledger entries without an instance: {sorted(set(LEDGER) - have)}"
    text = (ROOT / HERE).read_text()
    for name, (conditions, credit) in LEDGER.items():
        assert conditions and re.search(rf"^def {re.escape(credit.partition('::')[2])}\(", text, re.M), (name, credit)
