"""k_shade on both sides of its two data-size switches.

kShadeGeomsLds = 256: up to 256 flattened geometries the material table is staged in LDS (k_shade<false, true, *>), above that it is read
from global memory (k_shade<false, false, *>).  kMargRows = 2048: the sky's marginal tables are staged in LDS up to 2048 rows and read
through the global pointers above.  Frames of tests/surface_worlds.py's many_geometries(n) at n = 255, 256, 257 and 300 and of the atrium
under skies of 2047, 2048, 2049 and 4096 rows are compared with the oracle bit for bit; and, without the oracle, the frame of a 256-entry
world (LDS) with the frame of the same world plus one placed geometry of zero triangles (257 entries, global memory), which must not
differ in one bit (premise: test_surface_cpu.py).

RT3_F_NEE_EMISSIVE: the oracle has no emitter next-event estimation (tests/test_nee_emissive.py pins that estimator without it), so for
the flag set with that bit the k_shade<false, *, true> variants are held to what does exist: the G-buffer equals the oracle's, the frame
across the switch equals the LDS frame bit for bit (the empty-geometry pairs), instance mode 1 equals mode 0, and the frame's mean agrees
with the oracle's flag-less frame of the same integral within five standard errors."""
import ctypes as C
import math

import numpy as np
import pytest

import orc
import surface_worlds as SW
from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from raytracer3_amd.renderer import Camera, PathTracer
from support import bits

pytestmark = pytest.mark.gpu

W, H, SPP, BOUNCES = 64, 48, 4, 3
FULL = L.F_NEE_SKY | L.F_BLUENOISE | L.F_FACEFORWARD | L.F_SPECULAR
FLAG_SETS = (0, FULL, FULL | L.F_NEE_EMISSIVE)


@pytest.fixture(scope="module")
def env():
    """(sky, blue noise): shared, never modified"""
    return scenes.sky(128, 64), assets.load_bluenoise()


class Gpu:
    """one context over a world; frames by flag set"""

    def __init__(self, mesh, instances, sky, bn, mode=0):
        self.pt = PathTracer((W, H))
        ctx = self.pt.ctx
        ctx.set_option(L.OPT_INSTANCE_MODE, mode)
        ctx.upload_mesh(mesh)
        if instances:
            ctx.set_instances(instances)
        ctx.set_sky(sky)
        ctx.set_bluenoise(bn)
        ctx.build_accel()
        self.n_tris = ctx.accel_info()[1]

    def gconst(self, camera, flags):
        cam = Camera(camera["position"], camera["direction"], math.radians(camera["fov_deg"]), W / H)
        return self.pt.make_gconst(cam, SPP, BOUNCES, frame=1, flags=flags)

    def frame(self, camera, flags):
        self.pt.render(self.gconst(camera, flags))
        return (self.pt.light(), *self.pt.gbuffer())

    def close(self):
        self.pt.close()


def oracle_frame(osc, g):
    og = orc.GConst()
    C.memmove(C.byref(og), C.byref(g), 304)
    gb, depth = osc.gbuffer(og)
    light, _ = osc.reference_mode(og, gb, depth)
    return light, gb, depth


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def same_mean(light_e, light_0, depth):
    """two unbiased estimates of one image: their means differ by less than five standard errors.  The spatial variance of a frame is
    at least the mean variance of its pixels' estimators (it adds the image's own structure), so this standard error is an upper bound."""
    m = depth != L.BACKGROUND_DEPTH
    a, b = light_e[..., :3][m].astype(np.float64).sum(1), light_0[..., :3][m].astype(np.float64).sum(1)
    assert np.isfinite(a).all() and a.mean() > 0
    se = math.sqrt((a.var() + b.var()) / len(a))
    return abs(a.mean() - b.mean()) <= 5.0 * se, (a.mean(), b.mean(), se)


# ------------------------------------------------------------------------------------------------ the geometry table
@pytest.mark.parametrize("n", [255, 256, 257, 300])
def test_frames_equal_the_oracle(env, n):
    sky, bn = env
    mesh, inst, cam = SW.many_geometries(n)
    osc = orc.Scene(mesh, sky, bn, instances=inst)
    modes = (0, 1) if n == 257 else (0,)
    frames = {}
    for mode in modes:
        gpu = Gpu(mesh, inst, sky, bn, mode)
        try:
            if mode == 0:
                assert gpu.n_tris == 2 + 12 * (n - 1) == mesh.n_triangles  # the floor and n - 1 boxes: n flattened entries
            for flags in FLAG_SETS:
                frames[mode, flags] = gpu.frame(cam, flags)
            g = {flags: gpu.gconst(cam, flags) for flags in FLAG_SETS}
        finally:
            gpu.close()
    want = {flags: oracle_frame(osc, g[flags]) for flags in FLAG_SETS[:2]}
    for mode in modes:
        for flags in FLAG_SETS[:2]:
            light, gb, depth = frames[mode, flags]
            olight, ogb, odepth = want[flags]
            assert np.array_equal(bits(depth), bits(odepth)) and np.array_equal(gb, ogb), (n, mode, flags)
            assert np.array_equal(bits(light), bits(olight)), (n, mode, flags, int((bits(light) != bits(olight)).any(2).sum()))
        light, gb, depth = frames[mode, FLAG_SETS[2]]  # emitter NEE: see the module docstring
        assert np.array_equal(bits(depth), bits(want[FULL][2])) and np.array_equal(gb, want[FULL][1])
        assert not np.array_equal(bits(light), bits(want[FULL][0]))  # the flag found emitters to sample
        ok, figures = same_mean(light, want[FULL][0], depth)
        assert ok, (n, mode, figures)
    if len(modes) == 2:
        for flags in FLAG_SETS:
            assert same(frames[0, flags], frames[1, flags]), flags
    olight, _, odepth = want[FULL]
    assert olight[..., :3].mean() > 0 and (odepth != L.BACKGROUND_DEPTH).mean() > 0.6


@pytest.mark.parametrize("at", [None, 128], ids=["empty entry last", "empty entry in the middle"])
@pytest.mark.parametrize("n", [256, 255], ids=["256 (LDS) -> 257 (global)", "255 -> 256 (both LDS, the control)"])
def test_lds_table_equals_global_table(env, n, at):
    """the same triangles behind n and n + 1 table entries; in the middle, the empty entry shifts the index of every later one"""
    sky, bn = env
    mesh, inst, cam = SW.many_geometries(n)
    mesh1, inst1 = SW.with_empty_geometry(mesh, inst, at)
    assert sum(c for _, c, _ in inst1) == n + 1
    frames = []
    for m, i in ((mesh, inst), (mesh1, inst1)):
        gpu = Gpu(m, i, sky, bn)
        try:
            assert gpu.n_tris == mesh.n_triangles
            frames.append([gpu.frame(cam, flags) for flags in FLAG_SETS])
        finally:
            gpu.close()
    for flags, a, b in zip(FLAG_SETS, *frames):
        assert same(a, b), (flags, int((bits(a[0]) != bits(b[0])).any(2).sum()))
        assert a[0][..., :3].mean() > 0
    assert not np.array_equal(bits(frames[0][1][0]), bits(frames[0][2][0]))  # and emitter NEE really ran


# ------------------------------------------------------------------------------------------------ the sky's marginal tables
ATRIUM_DETAIL = 0.2


@pytest.fixture(scope="module")
def atrium():
    """(mesh, blue noise, the oracle's frame under a dark sky): what no sky lights"""
    mesh, bn = scenes.atrium(ATRIUM_DETAIL), assets.load_bluenoise()
    g = orc.camera_gconst(scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], scenes.ATRIUM_CAMERA["fov_deg"], W, H)
    g.bounces, g.samples, g.blendfactor, g.frame = BOUNCES, SPP, 1.0, 1
    g.pad[0] = FULL
    osc = orc.Scene(mesh, np.full((8, 8, 3), 1e-6, np.float32), bn)
    gb, depth = osc.gbuffer(g)
    return mesh, bn, osc.reference_mode(g, gb, depth)[0]


@pytest.mark.parametrize("rows", [2047, 2048, 2049, 4096])
def test_sky_rows_equal_the_oracle(atrium, rows):
    mesh, bn, dark = atrium
    sky = SW.banded_sky(rows)
    gpu = Gpu(mesh, None, sky, bn)
    try:
        g = gpu.gconst(scenes.ATRIUM_CAMERA, FULL)
        light, gb, depth = gpu.frame(scenes.ATRIUM_CAMERA, FULL)
    finally:
        gpu.close()
    olight, ogb, odepth = oracle_frame(orc.Scene(mesh, sky, bn), g)
    assert np.array_equal(bits(depth), bits(odepth)) and np.array_equal(gb, ogb)
    assert np.array_equal(bits(light), bits(olight)), int((bits(light) != bits(olight)).any(2).sum())
    lit = olight[..., :3].sum(2) > 2.0 * dark[..., :3].sum(2) + 1e-3  # pixels the sky lights: not passing on black
    assert olight[..., :3].mean() > 0 and lit.mean() > 0.05, (olight[..., :3].mean(), lit.mean())


def test_both_tables_in_global_memory(env):
    """300 flattened geometries under a sky of 2049 rows: k_shade<false, false> reading both tables through global pointers equals the
    oracle; with emitter NEE on top (k_shade<false, false, true>), see the module docstring"""
    _, bn = env
    sky = SW.banded_sky(2049)
    mesh, inst, cam = SW.many_geometries(300)
    frames = {}
    for mode in (0, 1):
        gpu = Gpu(mesh, inst, sky, bn, mode)
        try:
            frames[mode] = [gpu.frame(cam, flags) for flags in FLAG_SETS[1:]]
            g = gpu.gconst(cam, FULL)
        finally:
            gpu.close()
    want = oracle_frame(orc.Scene(mesh, sky, bn, instances=inst), g)
    for mode in (0, 1):
        full, emissive = frames[mode]
        assert same(full, want), mode
        assert same(emissive[1:], want[1:]) and not np.array_equal(bits(emissive[0]), bits(want[0]))
        ok, figures = same_mean(emissive[0], want[0], emissive[2])
        assert ok, (mode, figures)
    assert same(frames[0][1], frames[1][1])
    assert want[0][..., :3].mean() > 0
