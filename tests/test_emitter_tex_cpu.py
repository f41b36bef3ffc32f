"""Textured emitters without a GPU: the references of tests/ref_emitter_tex.py against hand-worked answers, the
worlds' own conditions, and the bindings."""
import re
from pathlib import Path

import numpy as np

import emitter_tex_worlds as EW
import ref_emitter_tex as R
from raytracer3_amd import _lib as L
from raytracer3_amd import render_graph, renderer, scenes
from support import constant

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
TRI = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])


# ---------------------------------------------------------------------------------------------------------------- reference
def test_one_texel_texture_is_its_colour_everywhere():
    tex = constant((255, 128, 0, 9), 1, 1)
    want = R.RS.srgb_eotf([255, 128, 0])
    assert want[0] == 1.0 and want[2] == 0.0 and abs(want[1] - 0.2158605) < 1e-6
    u, v = np.array([0.0, 0.3, -7.25, 1.0, 123.5]), np.array([0.0, 0.9, 2.5, 1.0, -0.01])
    assert np.array_equal(R.lookup32(tex, u, v), np.tile(want.astype(F), (5, 1)))
    assert np.allclose(R.lookup64(tex, u, v), want, rtol=0, atol=1e-15)
    le = (3.0, 0.5, 2.0)
    got = R.radiance32(le, TRI, tex, [0.0, 1.0, 0.25], [0.0, 0.0, 0.5])
    assert np.array_equal(got, np.tile(np.asarray(le, F) * want.astype(F), (3, 1)))
    m32, L1 = R.mean32(TRI * 40.0, tex)
    assert L1 == 40 and np.array_equal(m32[[0, 2]], F([1.0, 0.0])) and abs(float(m32[1]) - want[1]) <= 1600 * 2.0**-24  # 1 is summed exactly
    assert R.mean32(TRI * 40.0, constant((255, 255, 255, 255), 4, 4))[0].tolist() == [1.0, 1.0, 1.0]


def test_two_texel_texture_under_repeat_addressing():
    u = np.array([0.25, 0.75, 0.5, 0.0, 1.0, -0.125, 1.375, 0.125, 2.25])
    want = np.array([1.0, 0.0, 0.5, 0.5, 0.5, 0.25, 0.75, 0.75, 1.0])  # by hand: centres at 0.25 and 0.75, linear between, the seam at 0 = 1
    assert np.array_equal(EW.profile(u), want)
    for v in (0.0, 0.5, -3.7):  # one row: v does not matter
        assert np.array_equal(R.lookup64(EW.HALF, u, np.full_like(u, v))[:, 0], want)
        assert np.array_equal(R.lookup32(EW.HALF, u, np.full_like(u, v))[:, 1], want.astype(F))  # all exact in float32
    # the rule's mean over the unit uv square's two triangles, L = 2, by hand: u at the four centroids is 1/3, 5/6, 5/6, 2/3 on the first
    # (u = b1 + b2) and 1/6, 1/6, 2/3, 1/3 on the second (u = b1); the profile there is 5/6, 1/6, 1/6, 1/6 and 5/6, 5/6, 1/6, 5/6
    for tri, want_mean in (([[0, 0], [1, 0], [1, 1]], 1.0 / 3.0), ([[0, 0], [1, 1], [0, 1]], 2.0 / 3.0)):
        m, Lq = R.mean64(np.array(tri, float), EW.HALF)
        assert Lq == 2 and abs(m[0] - want_mean) < 1e-7
        m32, _ = R.mean32(np.array(tri, F), EW.HALF)
        assert abs(float(m32[0]) - want_mean) < 1e-6


def test_subdivision_of_known_edges():
    assert [R.subdiv_of_edge(e) for e in (0.5, 1.0, 1.01, 64.0, 1000.0)] == [1, 1, 2, 64, 64]
    assert [R.subdiv_of_edge(e) for e in (0.0, 63.0, 63.5, np.nan, np.inf)] == [1, 63, 64, 1, 1]
    assert R.subdiv([[0, 0], [0.5, 0], [0, 0.25]], 4, 8) == 2 and R.subdiv([[0, 0], [np.nan, 0], [0, 1]], 4, 4) == 1
    assert R.subdiv([[0.25, 0.5], [0.25, 0.5], [0.25, 0.5]], 64, 64) == 1  # a point in uv


def test_centroids_tile_the_triangle():
    for Lq in (1, 2, 3, 7, 64):
        b1, b2 = (x.astype(np.float64) for x in R.centroids(Lq))
        assert len(b1) == Lq * Lq and len({(round(a * 3 * Lq), round(b * 3 * Lq)) for a, b in zip(b1, b2)}) == Lq * Lq  # all different
        assert (b1 > 0).all() and (b2 > 0).all() and (b1 + b2 < 1).all()
        assert abs(b1.mean() - 1 / 3) < 1e-6 and abs(b2.mean() - 1 / 3) < 1e-6  # the centroid of the centroids
        ups = np.sum(np.isclose((b1 * 3 * Lq) % 3, 1.0))
        assert ups == Lq * (Lq + 1) // 2
    assert [x.tolist() for x in R.centroids(1)] == [[F(1) / F(3)], [F(1) / F(3)]]


def test_mean32_is_near_mean64_and_sums_in_the_stated_order():
    rng = np.random.default_rng(5)
    tex = rng.integers(0, 256, (8, 8, 4)).astype(np.uint8)
    for scale in (0.1, 0.4, 3.0, 9.0):
        uv = rng.uniform(-1.0, 1.0, (3, 2)) * scale
        (m32, L32), (m64, L64) = R.mean32(uv.astype(F), tex), R.mean64(uv.astype(F), tex)
        assert L32 == L64 and np.abs(m32.astype(np.float64) - m64).max() <= R.mean_bound(L32, np.abs(uv).max(), 8)
    assert 10 * 2.0**-24 < R.mean_bound(1, 1.0, 1) < 64 * 2.0**-24 and R.mean_bound(64, 1.0, 1) > 4096 * 2.0**-24


def test_queue_reference_by_hand():
    """two entries of equal mass, the second textured with the 1 x 1 colour: a ray whose dim-5 draw picks it is scaled, the others are not"""
    tex = constant((255, 128, 0, 255), 1, 1)
    rgb = R.lut32()[[255, 128, 0]]
    cdf = np.array([1 << 22, 1 << 23], np.uint32)
    emit_uv, emit_tex = np.zeros((2, 3, 2), F), np.array([-1, 0], np.int32)
    pixels = np.array([3 | (5 << 16), 900 | (7 << 16)], np.uint32)
    rec = np.zeros((40, 4), np.uint32)
    rec[:, :3] = F([2.0, 3.0, 4.0]).view(np.uint32)
    rec[:, 3] = np.arange(40)
    out, e = R.queue32(cdf, emit_uv, emit_tex, [tex], 9, 4, 1, 3, 8, pixels, rec, count=30)
    seed = R.RR.rng_seed(np.uint64(3), np.uint64(5), 9)
    u5 = R.RR.uniform_float(seed, np.uint64(((3 + 0) * 4 + 1) * 8 + 5))
    assert e[0] == (1 if u5 >= 0.5 else 0)  # path 0: pixel 0, sample 3
    assert 0 < e[:30].sum() < 30  # both entries are picked
    want = np.where(e[:, None] == 1, (F([2.0, 3.0, 4.0]) * rgb)[None, :], F([2.0, 3.0, 4.0])[None, :]).astype(F)
    assert np.array_equal(out[:30].view(F), want) and np.array_equal(out[30:], rec[30:, :3])  # behind the count: untouched


# ---------------------------------------------------------------------------------------------------------------- worlds
def test_neon_room_conditions():
    mesh = scenes.neon_room()
    sign = mesh.names.index("sign")
    assert mesh.material_textures["emissive_texture"][sign] == 0 and (mesh.geometries["emission"][sign, :3] > 0).all()
    assert [n for n, g in zip(mesh.names, mesh.geometries) if (g["emission"][:3] != 0).any()] == ["sign"]  # lit only by the sign
    tex = mesh.textures[0]
    assert tex.shape == (16, 64, 4) and 0.02 < (tex[..., :3] > 0).any(-1).mean() < 0.25  # mostly black
    prim = np.concatenate([[0], np.cumsum(mesh.prim_counts)])[sign] + np.arange(mesh.prim_counts[sign])
    uv, t = EW.expected_side_array(mesh, None, prim)
    assert (t == 0).all() and uv[..., 0].min() < 0 and uv[..., 0].max() > 1  # uvs outside [0, 1]
    means = np.array([R.mean64(x, tex)[0] for x in uv])
    dark = (means == 0).all(1)
    assert dark.any() and (~dark).any() and means.max() <= 1.0  # some sub-triangles see no stroke at all, some do


def test_soup_conditions():
    mesh, inst = EW.soup()
    assert len(inst) == 3 and np.linalg.det(np.asarray(inst[2][2])[:3, :3]) < 0  # a mirror
    names = mesh.names
    t = mesh.material_textures["emissive_texture"]
    assert t[names.index("missing")] >= len(mesh.textures) and t[names.index("plain")] == -1 and mesh.alpha_cutoffs[names.index("masked")] > 0
    assert [tuple(x.shape[:2]) for x in mesh.textures] == [(8, 8), (3, 5)]
    lad = names.index("ladder")
    prim = np.concatenate([[0], np.cumsum(mesh.prim_counts)])[lad] + np.arange(mesh.prim_counts[lad])
    uv, tex = EW.expected_side_array(mesh, None, prim)
    assert [R.subdiv(x, 8, 8) for x in uv] == list(EW.LADDER_L)
    g8 = names.index("tex8")
    uv8 = mesh.vertices[:3 * int(mesh.prim_counts[g8]), 6:8]
    assert uv8.min() < -1 and uv8.max() > 2  # beyond [0, 1]


def test_striped_light_profile_integrates_to_half():
    x = (np.arange(4096) + 0.5) / 4096
    assert abs(EW.profile(x).mean() - 0.5) < 1e-6 and EW.profile(0.25) == 1 and EW.profile(0.75) == 0


# ---------------------------------------------------------------------------------------------------------------- bindings
def test_abi_is_declared_and_bound():
    header = (ROOT / "include" / "rt3.h").read_text()
    for name in ("rt3_scene_set_textured_emitters", "rt3_scene_get_textured_emitters", "rt3_light_emit_tex"):
        assert re.search(r"\bint %s\(" % name, header) and name in L.EXPORTS
    assert "emit_tex_launches" in header and "emit_tex_launches" in [f[0] for f in L.Stats._fields_]
    assert (L.SELFTEST_EMIT_RADIANCE, L.SELFTEST_EMIT_TEX_QUEUE, L.SELFTEST_EMIT_MEAN) == (42, 43, 44)
    for name in ("set_textured_emitters", "get_textured_emitters", "light_emit_tex", "selftest_emit_radiance", "selftest_emit_tex_queue", "selftest_emit_mean"):
        assert callable(getattr(render_graph.Context, name))
    assert callable(renderer.PathTracer.set_textured_emitters)


def test_python_layer_passes_the_mode_through():
    class Lib:
        def __init__(self):
            self.mode = 0

        def rt3_scene_set_textured_emitters(self, h, on):
            self.mode = on
            return 0

        def rt3_scene_get_textured_emitters(self, h, ref):
            ref._obj.value = self.mode
            return 0

    ctx = render_graph.Context.__new__(render_graph.Context)
    ctx.lib, ctx.h = Lib(), None
    ctx.check = lambda rc: None
    assert ctx.get_textured_emitters() is False
    ctx.set_textured_emitters()
    assert ctx.get_textured_emitters() is True
    ctx.set_textured_emitters(False)
    assert ctx.get_textured_emitters() is False
