"""The exit test in the shade kernel (RT3_OPT_SHADE_EXIT_TEST): with the option at 1, k_shade_defer_exit tries a sky shadow
ray against the leaf of its exit-table entry before it queues the ray, the plain k_shadow walks the rays that leaf did not occlude from the
root, and k_light finishes those that came through.  With 0 every ray is queued and k_shadow_exit tries the entry -- the parent's launch
order.  The option may change no bit of a frame, no ray count of rt3_stats and, while every ray tries its entry, no count of
rt3_accel_exit_table_info: every comparison here is exact, `Light` as uint32, and one frame of each family against the oracle's
reference_mode as well.  The families: bounce counts and estimator flag sets; the 512-thread append boundaries; one sample per batch, a tile
partition, a lens, roulette from bounce 0, the adaptive pass, the LDS geometry table and its global twin; leaves of 1 .. 8 triangles, before
and after a refit that moves the shell; the launch-start switch to sampling; and the frames that keep the parent's order whatever the option
says (alpha masks, panes, two-level mode, emitter NEE, counting)."""
import dataclasses
import functools
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import material_worlds as mw
import orc
import pane_worlds as pn
from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from raytracer3_amd.renderer import Camera, PathTracer
from support import as_orc, bits
from test_traversal_exactness_cpu import base_mesh

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HERE = "tests/test_shade_exit_test.py"
FULL = L.F_NEE_SKY | L.F_BLUENOISE | L.F_SPECULAR | L.F_FACEFORWARD
FLAG_SETS = {
    "full": FULL,
    "no_specular": FULL & ~L.F_SPECULAR,
    "no_bluenoise": FULL & ~L.F_BLUENOISE,
    "no_faceforward": FULL & ~L.F_FACEFORWARD,
}
WINDOW = (64, 48)
SMALL = (37, 29)  # x 3 spp = 3219 paths: no multiple of 64 or 512
LDS_GEOMS = 256   # kShadeGeomsLds (rt3_surface.hpp)
WARMUP = 1 << 16  # kExitWarmupTries


@functools.lru_cache(maxsize=None)
def world(name):
    """(mesh, camera dictionary)"""
    if name == "atrium":
        return scenes.atrium(0.2), scenes.ATRIUM_CAMERA
    if name == "cornell":
        return scenes.cornell(), scenes.CORNELL_CAMERA
    if name == "cutout":
        return scenes.cutout_cornell(), scenes.CORNELL_CAMERA
    if name == "cloud":  # a triangle soup: an entry's leaf occludes fewer than a quarter of the rays
        return base_mesh("cloud"), dict(position=(0.0, 0.0, 7.0), direction=(0.0, 0.0, -1.0), fov_deg=60.0)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def sky_and_noise():
    return scenes.sky(256, 128), assets.load_bluenoise()


def camera(cam_kw, window):
    return Camera(cam_kw["position"], cam_kw["direction"], math.radians(cam_kw["fov_deg"]), window[0] / window[1])


def frames(pt, g, adaptive=None):
    """{option: (Light, extension rays, shadow rays, tried, occluded)} of one frame with RT3_OPT_SHADE_EXIT_TEST at 1 and at 0; the last
    two are what the frame added to the exit table's counters"""
    out = {}
    for opt in (1, 0):
        pt.ctx.set_option(L.OPT_SHADE_EXIT_TEST, opt)
        pt.ctx.stats_reset()
        _, t0, o0, _ = pt.ctx.exit_table_info()
        pt.render(g, adaptive=adaptive)
        st = pt.ctx.stats()
        _, t1, o1, _ = pt.ctx.exit_table_info()
        out[opt] = (pt.light(), int(st.extension_rays), int(st.shadow_rays), int(t1 - t0), int(o1 - o0))
    return out


def by_option(name, window=SMALL, *, spp=3, bounces=4, flags=FULL, options=(), setup=None, rank=0, n_ranks=1, instances=None, mesh=None, adaptive=None):
    """(frames(), the frame's GConst, G-buffer depth) on a PathTracer of its own"""
    base, cam_kw = world(name)
    sk, bn = sky_and_noise()
    pt = PathTracer(window, rank=rank, n_ranks=n_ranks)
    try:
        pt.set_scene(base if mesh is None else mesh, sk, bn, instances=instances, options=options)
        if setup:
            setup(pt)
        g = pt.make_gconst(camera(cam_kw, window), samples=spp, bounces=bounces, frame=1, flags=flags)
        out = frames(pt, g, adaptive)
        _, depth = pt.gbuffer()
    finally:
        pt.close()
    return out, g, depth


def same_by_option(tag, out, counters=False):
    (l1, e1, s1, t1, o1), (l0, e0, s0, t0, o0) = out[1], out[0]
    print(f"{tag}: extension rays {e1} / {e0}, shadow rays {s1} / {s0}, tried {t1} / {t0}, occluded {o1} / {o0}, mean {float(l1[..., :3].mean()):.6g}")
    assert (e1, s1) == (e0, s0), (tag, "ray counts", (e1, s1), (e0, s0))
    if counters:
        assert (t1, o1) == (t0, o0), (tag, "exit table counters", (t1, o1), (t0, o0))
    diff = (bits(l1) != bits(l0)).any(-1)
    assert not diff.any(), (tag, int(diff.sum()), "pixels differ, first at", np.argwhere(diff)[:3].tolist())
    return l1, s1, t1, o1


def against_oracle(tag, mesh, light, g, depth, count=None):
    sk, bn = sky_and_noise()
    osc = orc.Scene(mesh, sk, bn)
    og = as_orc(g)
    ogb, odepth = osc.gbuffer(og)
    assert np.array_equal(bits(depth), bits(odepth)), tag
    olight, ocounts = osc.reference_mode(og, ogb, odepth)
    assert np.array_equal(bits(light), bits(olight)), tag
    assert float(olight[..., :3].mean()) > 0.0, tag
    return ocounts


# ---------------------------------------------------------------------------------------------------------------- 1. option 1 against option 0
@pytest.mark.parametrize("bounces", [1, 2, 4])
def test_option_changes_nothing(bounces):
    out, g, depth = by_option("atrium", WINDOW, spp=4, bounces=bounces, options=[(L.OPT_SHADOW_EXIT_TABLE, 1)])
    light, shadow, tried, occluded = same_by_option(("atrium", bounces), out, counters=True)
    assert 0 < tried == shadow < WARMUP and 0 < occluded < tried  # every ray tried its entry, and some entries decided
    if bounces == 4:
        against_oracle(("atrium", bounces), world("atrium")[0], light, g, depth)


@pytest.mark.parametrize("flag_set", list(FLAG_SETS))
def test_flag_sets(flag_set):
    for name in ("atrium", "cornell"):
        out, _, _ = by_option(name, flags=FLAG_SETS[flag_set])
        _, shadow, tried, _ = same_by_option((name, flag_set), out, counters=True)
        assert 0 < tried == shadow, (name, flag_set)


@pytest.mark.parametrize("window,spp", [((9, 7), 1), ((13, 5), 1), ((31, 17), 1), ((37, 29), 3), ((64, 8), 1), ((64, 64), 1)])
def test_queue_lengths(window, spp):
    """63, 65, 527 and 3219 paths, and exactly one and eight workgroups' worth"""
    out, g, depth = by_option("atrium", window, spp=spp)
    light, _, _, _ = same_by_option(("atrium", window, spp), out, counters=True)
    against_oracle(("atrium", window, spp), world("atrium")[0], light, g, depth)


def test_ray_counts_equal_the_oracles():
    """rt3_stats.shadow_rays stays the number of shadow rays the estimator generated, the decided ones included"""
    out, g, depth = by_option("atrium", SMALL)
    light, shadow, tried, occluded = same_by_option("atrium counts", out, counters=True)
    counts = against_oracle("atrium counts", world("atrium")[0], light, g, depth)
    # (the oracle's counts: [0] extension rays behind the primary ones, [1] shadow rays -- test_gpu_parity's comparison)
    assert shadow == int(counts[1]) and out[1][1] == SMALL[0] * SMALL[1] + int(counts[0]), (shadow, out[1][1], counts)
    assert occluded > 0


# ---------------------------------------------------------------------------------------------------------------- 2. with other features on
def test_one_sample_per_batch():
    out, g, depth = by_option("atrium", options=[(L.OPT_BATCH_SPP, 1)])
    light, _, _, _ = same_by_option("batch spp 1", out, counters=True)
    against_oracle("batch spp 1", world("atrium")[0], light, g, depth)


def test_three_rank_tile_partition():
    window = (160, 96)  # 3 x 2 tiles of 64 x 64 (the right column and the lower row cut), two per rank
    whole = None
    for rank in range(3):
        out, _, _ = by_option("atrium", window, spp=2, rank=rank, n_ranks=3)
        light, shadow, _, _ = same_by_option(("rank", rank), out)
        assert shadow > 0, rank
        whole = light.copy() if whole is None else np.where(light != 0, light, whole)
    out, _, _ = by_option("atrium", window, spp=2)
    assert np.array_equal(bits(whole), bits(out[1][0]))


def test_lens_frame():
    """vertex 0 through the FIRST = false instance, its queue's length read on the device"""
    for name in ("atrium", "cornell"):
        out, _, _ = by_option(name, setup=lambda pt: pt.set_lens(0.05, 3.0, 1.0))
        _, shadow, tried, _ = same_by_option((name, "lens"), out, counters=True)
        assert 0 < tried == shadow


def test_roulette_from_bounce_0():
    for name in ("atrium", "cornell"):
        out, _, _ = by_option(name, setup=lambda pt: pt.set_roulette(0, 0.0625))
        same_by_option((name, "roulette"), out, counters=True)
        out, _, _ = by_option(name, setup=lambda pt: (pt.set_roulette(0, 0.0625), pt.set_lens(0.05, 3.0, 1.0)))
        same_by_option((name, "roulette, lens"), out, counters=True)


def test_adaptive_pass():
    p = L.AdaptiveParams(min_samples=2, step=2, threshold=0.05, dark=0.01, dilate=1)
    out, _, _ = by_option("atrium", spp=6, adaptive=p)
    _, shadow, tried, _ = same_by_option("adaptive", out, counters=True)
    assert 0 < tried == shadow


def test_geometry_table_outside_lds():
    """more flattened geometries than the LDS table holds: the GLDS = false instance"""
    base, _ = world("cornell")
    big, inst = mw.padded(base, LDS_GEOMS + 1)
    out, _, _ = by_option("cornell", mesh=big, instances=inst)
    light, shadow, tried, _ = same_by_option("padded", out, counters=True)
    assert 0 < tried == shadow
    small, _, _ = by_option("cornell")
    assert np.array_equal(bits(light), bits(small[1][0]))  # the padding changes no frame


# ---------------------------------------------------------------------------------------------------------------- 3. leaves of 1 .. 8 records
@pytest.mark.parametrize("leaf", [1, 2, 4, 8])
def test_leaf_sizes_and_refit(leaf):
    rest, cam_kw = world("atrium")
    v = rest.vertices.copy()  # the shell moves: the scene grows about its centre, by another factor along each axis
    p = v[:, :3].astype(np.float64)
    c = (p.min(0) + p.max(0)) / 2
    v[:, :3] = (c + (p - c) * np.array([1.1, 1.2, 0.95])).astype(np.float32)
    moved = dataclasses.replace(rest, vertices=v)
    sk, bn = sky_and_noise()
    pt = PathTracer(WINDOW)
    try:
        pt.set_scene(rest, sk, bn, options=[(L.OPT_LEAF_SIZE, leaf)])
        g = pt.make_gconst(camera(cam_kw, WINDOW), samples=2, bounces=3, frame=1, flags=FULL)
        for tag, mesh in (("rest", rest), ("moved", moved)):
            if tag == "moved":
                pt.update_vertices(v)
                assert pt.ctx.exit_table_info()[1] == 0  # the counters start again
            light, shadow, tried, occluded = same_by_option((tag, "leaf", leaf), frames(pt, g), counters=True)
            assert 0 < tried == shadow and occluded > 0, (tag, leaf)
            _, depth = pt.gbuffer()
            against_oracle((tag, "leaf", leaf), mesh, light, g, depth)
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 4. the switch
def test_switch_to_sampling_and_back():
    """a soup whose entries occlude fewer than a quarter of the rays, rendered past 2^16 tries: every 32nd trip of the shade kernel's loop
    goes on trying, the frames stay what they are; then the atrium on the same context, whose counters start again with its build"""
    mesh, cam_kw = world("cloud")
    sk, bn = sky_and_noise()
    window = (128, 96)
    pt = PathTracer(window)
    try:
        pt.set_scene(mesh, sk, bn)
        g = pt.make_gconst(camera(cam_kw, window), samples=4, bounces=4, frame=1, flags=FULL)
        first = frames(pt, g)
        want, _, _, _ = same_by_option("cloud, warm-up", first)
        for k in range(12):
            _, tried, occluded, in_use = pt.ctx.exit_table_info()
            if tried >= WARMUP:
                break
            pt.render(g)
        print("cloud: tried %d, occluded %d, rate %.4f, in_use %d" % (tried, occluded, occluded / max(tried, 1), in_use))
        assert tried >= WARMUP and in_use == 0 and 4 * occluded < tried
        after = frames(pt, g)
        light, shadow, _, _ = same_by_option("cloud, sampling", after)
        assert np.array_equal(bits(light), bits(want))
        for opt in (0, 1):  # a sample: some rays tried, far from all
            assert 0 < after[opt][3] < shadow // 4, (opt, after[opt][3], shadow)
        atrium, cam_kw = world("atrium")
        pt.set_scene(atrium, sk, bn)
        g = pt.make_gconst(camera(cam_kw, window), samples=1, bounces=4, frame=1, flags=FULL)
        out = frames(pt, g)
        light, shadow, tried, _ = same_by_option("atrium after the cloud", out, counters=True)
        assert 0 < tried == shadow and pt.ctx.exit_table_info()[3] == 1 and float(light[..., :3].mean()) > 0.0
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 5. the parent's order
def decides_nothing(tag, out):
    """the frame kept k_shadow_exit (or has no table): the option changes neither frame nor any count"""
    same_by_option(tag, out, counters=True)


def test_masked_scene_keeps_its_frames():
    out, _, _ = by_option("cutout", (48, 36))
    decides_nothing("cutout", out)
    assert out[1][3] > 0  # k_shadow_exit<true> tried


def test_pane_scene_keeps_its_frames():
    sk, bn = sky_and_noise()
    pt = PathTracer(pn.CANOPY_WINDOW)
    try:
        pt.set_pane_shadows(True)
        pt.set_scene(pn.canopy_world(), sk, bn)
        pt.set_lens(*pn.CANOPY_LENS)
        g = pt.make_gconst(camera(pn.CAMERA, pn.CANOPY_WINDOW), samples=4, bounces=3, frame=1, flags=FULL)
        out = frames(pt, g)
    finally:
        pt.close()
    decides_nothing("canopy", out)
    assert float(out[1][0][..., :3].mean()) > 0.0


def test_two_level_mode_keeps_its_frames():
    out, _, _ = by_option("cornell", options=[(L.OPT_INSTANCE_MODE, 1)])
    decides_nothing("two-level", out)
    assert out[1][3] == 0 and out[1][2] > 0  # no table, shadow rays all the same
    flat, _, _ = by_option("cornell")
    assert np.array_equal(bits(out[1][0]), bits(flat[1][0]))


def test_emitter_nee_keeps_the_add_order():
    for name in ("cornell", "atrium"):
        out, _, _ = by_option(name, flags=FULL | L.F_NEE_EMISSIVE)
        decides_nothing((name, "emitter NEE"), out)
        assert out[1][3] > 0


def test_counting_keeps_its_frames():
    out, _, _ = by_option("atrium", options=[(L.OPT_COUNT_TRAVERSAL, 1)])
    decides_nothing("counting", out)
    assert out[1][3] == 0  # the counting walk starts at the root
    plain, _, _ = by_option("atrium")
    assert np.array_equal(bits(out[1][0]), bits(plain[1][0]))


def test_without_deferral_or_table():
    for options in ([(L.OPT_DEFER_SKY_LIGHT, 0)], [(L.OPT_SHADOW_EXIT_TABLE, 0)]):
        out, _, _ = by_option("atrium", options=options)
        decides_nothing(options, out)
    plain, _, _ = by_option("atrium")
    assert np.array_equal(bits(out[1][0]), bits(plain[1][0]))


def test_option_values():
    pt = PathTracer((8, 8))
    try:
        for bad in (-1, 2):
            assert pt.ctx.lib.rt3_set_option(pt.ctx.h, L.OPT_SHADE_EXIT_TEST, bad) == L.E_INVALID
        for good in (0, 1):
            pt.ctx.set_option(L.OPT_SHADE_EXIT_TEST, good)
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 6. the new kernel's instances
# name -> (what selects it, the test here that runs it).  FIRST: vertex 0 from the G-buffer; GLDS: at most 256 flattened geometries.
LEDGER = {
    "k_shade_defer_exit<true, false>": ("vertex 0 of a frame without a lens", f"{HERE}::test_option_changes_nothing"),
    "k_shade_defer_exit<false, true>": ("later vertices, and vertex 0 of a lens frame", f"{HERE}::test_lens_frame"),
    "k_shade_defer_exit<false, false>": ("later vertices of a scene of more than 256 geometries", f"{HERE}::test_geometry_table_outside_lds"),
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
    return set(re.findall(r"__device_stub__(k_shade_defer_exit<[^>]*>)\(", out))


def test_own_instance_ledger():
    """fails when an instance of k_shade_defer_exit is added without an entry here, or an entry outlives its instance or its test"""
    have = library_instances()
    assert not have - set(LEDGER), f"instances without a ledger entry: {sorted(have - set(LEDGER))}"
    assert not set(LEDGER) - have, f"ledger entries without an instance: {sorted(set(LEDGER) - have)}"
    text = (ROOT / HERE).read_text()
    for name, (conditions, credit) in LEDGER.items():
        assert conditions and re.search(rf"^def {re.escape(credit.partition('::')[2])}\(", text, re.M), (name, credit)
