"""The composed float64 tracer of tests/ref_combined.py and its fixture tests/golden/combined_ref.npz, without a GPU.

ref_combined is trusted on feature combinations only after it has reproduced its three parents: with one feature set switched on it
must give the stored prefix statistics of integrator_ref.npz (ref_pathtrace), punctual_ref.npz (ref_lights) and lens_ref.npz (ref_lens
with the surfaces of ref_materials).  Cutouts, which no parent knows, are pinned on their two exact ends: a screen that is transparent
everywhere gives the samples of the room without it, one that is opaque everywhere the samples of the unmasked room, random number for
random number.

The CPU oracle (tests/orc.py) has neither alpha cutouts nor material textures, so it cannot render `cutout_textures` or any other case
of combined_worlds.CASES: there is no oracle-against-fixture test here, and the GPU is the first implementation the fixture meets."""
import functools
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import combined_worlds as CW
import integrator_worlds as IW
import lens_worlds as LW
import punctual_worlds as PW
import ref_combined as RC
import ref_lens as RLE
import ref_pathtrace as RP
from test_integrator_cpu import Z_MAX

GOLDEN = Path(__file__).resolve().parent / "golden" / "combined_ref.npz"


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def _generator(name):
    spec = importlib.util.spec_from_file_location(name, GOLDEN.parent / f"{name}.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def _stored(npz):
    with np.load(GOLDEN.parent / npz) as f:
        return {k: f[k] for k in f.files}


# ---------------------------------------------------------------------------------------------------------------- the three reductions
def _parent_pathtrace():
    name = "spec_b2"
    flags, bounces, specular, _, _, _ = IW.ROOM_CASES[name]
    scene = _generator("gen_integrator_ref").room_scene(specular)
    return "integrator_ref.npz", name, lambda seed: RC.render(scene, IW.ROOM_CAMERA, IW.WINDOW_ROOM, flags, bounces, RP.CHUNK_SPP, seed)


def _parent_lights():
    name = "spot_sun_b4"
    flags, bounces, _, _, _, _, _ = PW.CASES[name]
    mesh, sky = PW.room(name)
    scene = RP.Scene(mesh, sky=sky)
    return "punctual_ref.npz", name, lambda seed: RC.render(scene, IW.ROOM_CAMERA, IW.WINDOW_ROOM, flags, bounces, RP.CHUNK_SPP, seed, lights=mesh.lights)


def _parent_lens():
    name = "lens_mat_b2"
    flags, bounces, _, _, _, _ = LW.MATERIAL_CASES[name]
    mesh, cam = LW.material_room()
    scene = RP.Scene(mesh, sky=LW.constant_sky(LW.MATERIAL_SKY_C))
    surface = RLE.textured_surface(mesh, scene)
    return "lens_ref.npz", name, lambda seed: RC.render(scene, cam, IW.WINDOW_ROOM, flags, bounces, RP.CHUNK_SPP, seed, lens=LW.MATERIAL_LENS, surface=surface)


@pytest.mark.parametrize("parent", (_parent_pathtrace, _parent_lights, _parent_lens), ids=("ref_pathtrace", "ref_lights", "ref_lens"))
def test_reduces_to_its_parent(parent):
    """the first CHUNK_SPP samples of one case of the parent's fixture, rendered by the composed tracer with the stored seed"""
    npz, name, render = parent()
    fx = _stored(npz)
    mean, var = render(int(fx[f"{name}_seed"].item()))
    bm, se = RP.block_stats(mean, var, RP.CHUNK_SPP)
    assert np.allclose(bm, fx[f"{name}_prefix_mean"], rtol=1e-9, atol=0.0)
    assert np.allclose(se, fx[f"{name}_prefix_se"], rtol=1e-9, atol=0.0)


# ---------------------------------------------------------------------------------------------------------------- cutouts
def _samples(mesh, cutouts, seed=7, n=2, **kw):
    scene = RP.Scene(mesh, sky=CW.sky())
    return RC.radiance_samples(scene, CW.CAMERA, CW.WINDOW, CW.REF_FULL, 3, n, np.random.default_rng(seed), lights=mesh.lights,
                               cutouts=RC.Cutouts(mesh, scene) if cutouts else None, **kw)


@pytest.mark.parametrize("lens", (None, CW.LENS), ids=("pinhole", "lens"))
def test_cutout_ends_are_exact(lens):
    """alpha 0 everywhere: the room without the screen (the screen is the last geometry, so no other index moves); alpha 255 everywhere:
    the room with the opaque screen; the checker: neither.  Same random numbers, so the samples are equal, not close."""
    gone = _samples(CW.room(False, True, screen_texture=CW.constant_alpha(0)), True, lens=lens)
    assert np.array_equal(gone, _samples(CW.room(False, screen=False), False, lens=lens))
    solid = _samples(CW.room(False, True, screen_texture=CW.constant_alpha(255)), True, lens=lens)
    plain = _samples(CW.room(False, False), False, lens=lens)
    assert np.array_equal(solid, plain)
    checker = _samples(CW.room(False, True), True, lens=lens)
    differs_from_gone, differs_from_solid = np.any(checker != gone, (0, 3)), np.any(checker != solid, (0, 3))
    assert differs_from_gone.sum() > 30 and differs_from_solid.sum() > 30, "the checker's cells are seen and cast their shadows"
    assert gone.sum() > 0 and np.isfinite(checker).all()


def test_cutout_hits_are_the_next_closest():
    """rays straight down through the screen's cells: an opaque cell stops them on the screen, an open one on what lies below; the occlusion
    test towards a point above the screen follows the same cells"""
    mesh = CW.room(False, True)
    scene = RP.Scene(mesh)
    cut = RC.Cutouts(mesh, scene)
    o, eu, ev = (np.asarray(a, np.float64) for a in CW.SCREEN)
    s, t = np.meshgrid((np.arange(4) + 0.5) / 4, (np.arange(4) + 0.5) / 4)  # the centres of the checker's cells
    on_screen = o + s.reshape(-1, 1) * eu + t.reshape(-1, 1) * ev
    up = np.tile([0.0, 1.0, 0.0], (16, 1))
    tri, dist, _ = cut.trace(on_screen + 0.5 * up, -up)
    is_screen = scene.geom[tri] == mesh.names.index("screen")
    opaque = CW.checker()[..., 3].reshape(-1) == 255  # texel (y, x) <-> cell (t, s)
    assert np.array_equal(is_screen, opaque) and opaque.sum() == 8
    below_screen = RP.Scene(CW.room(False, screen=False)).trace(on_screen + 0.5 * up, -up)[1]  # the slab, the box or the floor
    assert np.allclose(dist[opaque], 0.5) and np.array_equal(dist[~opaque], below_screen[~opaque]) and np.all(below_screen > 0.5 + 0.5)
    assert np.all(scene.trace(on_screen + 0.5 * up, -up)[1] < 0.5 + 1e-6), "(the unmasked scene stops every one of them)"
    below = on_screen - 0.25 * up
    assert np.array_equal(cut.occluded(below, up, np.full(16, 0.75)), opaque)
    assert not cut.occluded(below, up, np.full(16, 0.2)).any(), "the segment ends below the screen"


# ---------------------------------------------------------------------------------------------------------------- worlds
def test_world_conditions():
    """the light is further from every triangle than 1 % of the room's diagonal; the screen is in view and the camera sees through it"""
    mesh = CW.room(True, True)
    scene = RP.Scene(mesh)
    P = mesh.lights[0]["position"].astype(np.float64)
    pts = scene.p.reshape(-1, 3)
    far = np.linalg.norm(pts - P, axis=1).max()
    s, t = np.meshgrid(np.linspace(0, 1, 33), np.linspace(0, 1, 33))
    keep = s + t <= 1.0
    grid = scene.v0[:, None] + s[keep][None, :, None] * scene.e1[:, None] + t[keep][None, :, None] * scene.e2[:, None]
    near = np.linalg.norm(grid - P, axis=-1).min()
    assert near - 0.1 > 0.01 * far, (near, far)  # (0.1: more than the sampling's spacing on these triangles' 2-unit edges / 32)
    k = mesh.names.index("screen")
    rays = RP.primary_rays(CW.CAMERA, CW.WINDOW)
    seen_masked = scene.geom[np.maximum(RC.Cutouts(mesh, scene).trace(*rays)[0], 0)] == k
    seen_solid = scene.geom[np.maximum(scene.trace(*rays)[0], 0)] == k
    assert seen_solid.sum() >= 60 and 0.3 * seen_solid.sum() < seen_masked.sum() < 0.7 * seen_solid.sum()
    for n, at in ((256, None), (257, None), (257, 4), (300, None)):
        big, inst = CW.padded(mesh, n, at)
        assert sum(c for _, c, _ in inst) == n == len(big.geometries) and big.n_triangles == mesh.n_triangles
        assert np.array_equal(big.alpha_cutoffs[:len(mesh.geometries)], mesh.alpha_cutoffs) and len(big.lights) == 1


# ---------------------------------------------------------------------------------------------------------------- fixture
def test_fixture_is_sized_and_arrays_only():
    fx = fixture()
    assert GOLDEN.stat().st_size < 64 * 1024
    for name, (_, _, has, _, spp, seed, _) in CW.CASES.items():
        assert int(fx[f"{name}_spp"].item()) == spp and int(fx[f"{name}_seed"].item()) == seed and spp % RP.CHUNK_SPP == 0
        assert fx[f"{name}_mean"].shape == fx[f"{name}_se"].shape == (2, 3, 3)
        assert np.all(fx[f"{name}_mean"] > 0) and np.all(fx[f"{name}_se"] > 0)
        assert fx[f"{name}_cover"].all(), "the room is closed: every pixel is covered, with and without a lens"
        # the fixture alone resolves 2 %: 0.02 x mean is beyond the band (by the margin the noise of the code under test may take)
        assert np.mean(0.02 * fx[f"{name}_mean"] > (Z_MAX + 1.0) * fx[f"{name}_se"]) >= 0.9, name


def test_generator_has_not_drifted():
    """the first CHUNK_SPP samples of the case with every feature on, rendered again with the stored seed, give the stored prefix statistics"""
    gen = _generator("gen_combined_ref")
    fx = fixture()
    name = "lens_lights_textures_cutout"
    assert int(fx[f"{name}_seed"].item()) == CW.CASES[name][5]
    bm, se = gen.stats([gen.chunk((name, 0))])
    assert np.allclose(bm, fx[f"{name}_prefix_mean"], rtol=1e-9, atol=0.0)
    assert np.allclose(se, fx[f"{name}_prefix_se"], rtol=1e-9, atol=0.0)
