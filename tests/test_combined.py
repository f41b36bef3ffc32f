"""The features together on the GPU: punctual lights, material textures, alpha cutouts and the thin lens in one
frame, against the composed float64 tracer of tests/ref_combined.py (tests/golden/combined_ref.npz), and every compiled instance of
k_shade, k_shade_punct, k_extend, k_shadow and k_shadow_exit accounted for in LEDGER below.

  a. every case of combined_worlds.CASES against the fixture, in both instance modes;
  b. k_shade_punct's geometry table in LDS against global memory: the same triangles behind 11 / 300 and 256 / 257 table entries;
  c. constant material maps against the factors they fold into, under a light;
  d. a closed form at a normal-mapped vertex 0 that only a lens frame shades with the punctual light function;
  e. the traversal instances a masked, lit, two-level or counted frame takes: counting on and off, the shadow exit table on and off,
     batches, the tile partition; and the range rays in every node layout;
  f. per-sample camera rays through cutouts: a transparent quad is not there, a checker passes its open share;
  g. the ledger: the library's symbol table holds exactly the instances LEDGER names, and every test LEDGER credits exists."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import combined_worlds as CW
import integrator_worlds as IW
import lens_worlds as LW
import material_worlds as MW
import punctual_worlds as PW
import ref_lens as RLE
import ref_lights as RLI
import ref_materials as RM
import ref_pathtrace as RP
from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from raytracer3_amd.assets import LIGHT_POINT, Material, MeshBuilder, make_light
from support import bits, camera
from test_combined_cpu import fixture
from test_integrator_cpu import check_against_fixture
from test_lens import check_binomial, lens_frame
from test_materials import mapped_room
from test_nee_emissive import FULL, frame, make_pt, owned_mask
from test_punctual_lights import EPS, check_closed_form, device_rays

pytestmark = pytest.mark.gpu

P, E = L.F_NEE_PUNCTUAL, L.F_NEE_EMISSIVE
ROOT = Path(__file__).resolve().parent.parent
LDS_GEOMS = 256  # kShadeGeomsLds (rt3_surface.hpp)


# ---------------------------------------------------------------------------------------------------------------- helpers
def build_pt(mesh, window=CW.WINDOW, instances=None, lens=None, options=(), sky=True, **kw):
    """make_pt with options that must precede the build (RT3_OPT_* name -> value)"""
    pt = make_pt(mesh, window, sky=CW.sky() if sky else None, instances=instances, options=dict(options).items(),
                 rank=kw.get("rank", 0), n_ranks=kw.get("n_ranks", 1))
    if lens is not None:
        pt.set_lens(*lens)
    return pt


def shot(pt, flags, spp=4, bounces=3, index=1, window=CW.WINDOW, cam=CW.CAMERA):
    """one frame's radiance, through the lens if the tracer has one"""
    c = camera(cam, window)
    if pt.ctx.get_lens()[1]:
        return lens_frame(pt, c, flags, spp, bounces, index=index)[0]
    return frame(pt, c, flags, spp, bounces, index=index)


def assert_instance_conditions(pt, mesh, flags, *, punct, mat, lds, masked=None):
    """what dispatch_shade and dispatch_traversal look at, read back from the built context and the mesh it was given"""
    n_e, n_p, _ = pt.ctx.light_masses(flags)
    assert (n_p > 0) == punct, "a punctual record in the table the flags sample"
    assert bool(np.any([np.any(mesh.material_textures[k] >= 0) for k in ("metallic_roughness_texture", "normal_texture", "emissive_texture")])) == mat
    assert (len(mesh.geometries) <= LDS_GEOMS) == lds, "flattened entries (every geometry once, or the padded list)"
    if masked is not None:
        assert bool(np.any(mesh.alpha_cutoffs > 0)) == masked


# ---------------------------------------------------------------------------------------------------------------- a. fixture
def case_frames(name, mode):
    flags, bounces, has, extra, _, _, n_frames = CW.CASES[name]
    mesh, lens = CW.world(name)
    pt = build_pt(mesh, lens=lens, options={L.OPT_INSTANCE_MODE: mode})
    try:
        kernel_flags = FULL | extra
        assert_instance_conditions(pt, mesh, kernel_flags, punct=has["lights"], mat=has["textures"], lds=True, masked=has["cutout"])
        pt.ctx.stats_reset()
        out = np.stack([shot(pt, kernel_flags, IW.FRAME_SPP, bounces, index=k) for k in range(n_frames)])
        st = pt.ctx.stats()
        assert st.extension_rays > 0 and (st.shadow_rays > 0) == bool(kernel_flags & (L.F_NEE_SKY | P | E))
        return out, pt.gbuffer()[1] != L.BACKGROUND_DEPTH
    finally:
        pt.close()


@pytest.mark.parametrize("mode", (0, 1), ids=("flat", "two_level"))
@pytest.mark.parametrize("name", list(CW.CASES))
def test_against_fixture(name, mode):
    frames, cov = case_frames(name, mode)
    assert cov.all(), "the room is closed"
    check_against_fixture(frames, cov, fixture(), name)


# ---------------------------------------------------------------------------------------------------------------- b. table switch
def padded_frames(name, n, at, flag_sets, mode=0):
    mesh, lens = CW.world(name)
    big, inst = (mesh, None) if n is None else CW.padded(mesh, n, at)
    pt = build_pt(big, instances=inst, lens=lens, options={L.OPT_INSTANCE_MODE: mode})
    try:
        assert pt.ctx.accel_info()[1] == mesh.n_triangles
        for flags in flag_sets:
            assert_instance_conditions(pt, big, flags, punct=True, mat=CW.CASES[name][2]["textures"], lds=len(big.geometries) <= LDS_GEOMS)
        return [shot(pt, flags) for flags in flag_sets]
    finally:
        pt.close()


SWITCH_FLAGS = (FULL | P, FULL | P | E)


@pytest.mark.parametrize("name", ("lights_textures", "lens_lights"))
def test_table_switch_under_lights_11_and_300(name):
    """k_shade_punct<false, true, MAT> against k_shade_punct<false, false, MAT>: MAT with lights_textures, plain with lens_lights (whose
    vertex 0 is shaded by the same instance)"""
    small, big = padded_frames(name, None, None, SWITCH_FLAGS), padded_frames(name, 300, None, SWITCH_FLAGS)
    for flags, a, b in zip(SWITCH_FLAGS, small, big):
        assert a.mean() > 0 and np.array_equal(bits(a), bits(b)), (flags, int((bits(a) != bits(b)).any(2).sum()))
    assert not np.array_equal(bits(small[0]), bits(small[1])), "emitter NEE ran"


@pytest.mark.parametrize("at", (None, 4), ids=("empty entry last", "empty entry in the middle"))
@pytest.mark.parametrize("name", ("lights_textures", "lens_lights"))
def test_table_switch_under_lights_256_to_257(name, at):
    lds, glob = padded_frames(name, 256, None, SWITCH_FLAGS), padded_frames(name, 257, at, SWITCH_FLAGS)
    for flags, a, b in zip(SWITCH_FLAGS, lds, glob):
        assert a.mean() > 0 and np.array_equal(bits(a), bits(b)), (flags, int((bits(a) != bits(b)).any(2).sum()))


# ---------------------------------------------------------------------------------------------------------------- c. folded factors
ROOM_LAMP = assets.lights_array([make_light(LIGHT_POINT, (6.0, 5.5, 4.5), position=(0.3, 2.2, 0.1))])  # inside material_worlds.room()


@pytest.mark.parametrize("lens", (None, (0.05, 3.0, 1.0)), ids=("pinhole", "lens"))
def test_constant_maps_equal_folded_factors_under_a_light(lens):
    """test_materials' idiom with a light in the room: k_shade_punct<false, true, true> on constant maps gives the bits of
    k_shade_punct<false, true, false> on the factors the maps fold into"""
    mapped, folded, cam = mapped_room(np.random.default_rng(31), emissive=False)
    removed = MW.with_tables(mapped, material_textures=assets.no_material_textures(len(mapped.geometries)))
    out = []
    for mesh, mat in ((mapped, True), (folded, False), (removed, False)):
        mesh.lights = ROOM_LAMP.copy()
        pt = build_pt(mesh, (64, 48), lens=lens)
        try:
            assert_instance_conditions(pt, mesh, FULL | P, punct=True, mat=mat, lds=True)
            out.append(shot(pt, FULL | P, window=(64, 48), cam=cam))
            unlit = shot(pt, FULL, window=(64, 48), cam=cam)
            assert out[-1].mean() > 1.2 * unlit.mean(), "the lamp lights the room"
        finally:
            pt.close()
    assert np.array_equal(bits(out[0]), bits(out[1])), int((bits(out[0]) != bits(out[1])).any(2).sum())
    assert not np.array_equal(bits(out[0]), bits(out[2])), "the maps matter"


# ---------------------------------------------------------------------------------------------------------------- d. closed form
FLOOR_LAMP = PW.FLOOR_LIGHTS["point"]  # its range ends inside the view


def mapped_floor():
    """punctual_worlds' floor and occluder, the floor with uvs (cells 3 x 1.5: ref_materials' tangent condition) and a normal map"""
    mb = MeshBuilder()
    mb.add("floor", *scenes._grid([-3, 0, 3], [6, 0, 0], [0, 0, -6], 2, 4), Material(PW.FLOOR_ALBEDO, 0.0, 1.0, normal_texture=0))
    (x0, x1), h, (z0, z1) = PW.OCCLUDER
    mb.add("occluder", *scenes._grid([x0, h, z1], [x1 - x0, 0, 0], [0, 0, z0 - z1], 1, 2), Material((0.5, 0.5, 0.5), 0.0, 1.0))
    mesh = mb.build()
    mesh.textures = MW.normal_textures(np.random.default_rng(61), [(16, 16)])
    return mesh


def barycentrics(scene, tri, x):
    """of the points x in the planes of the triangles tri, kept inside them as ref_lens.textured_surface keeps them"""
    w, e1, e2 = x - scene.v0[tri], scene.e1[tri], scene.e2[tri]
    d11, d12, d22 = np.sum(e1 * e1, -1), np.sum(e1 * e2, -1), np.sum(e2 * e2, -1)
    w1, w2 = np.sum(w * e1, -1), np.sum(w * e2, -1)
    den = d11 * d22 - d12 * d12
    bu, bv = np.clip((d22 * w1 - d12 * w2) / den, 0.0, 1.0), np.clip((d11 * w2 - d12 * w1) / den, 0.0, 1.0)
    s = np.maximum(bu + bv, 1.0) * (1.0 + 1e-6)
    return bu / s, bv / s


@pytest.mark.parametrize("samples", (1, 4))
def test_closed_form_at_a_textured_lens_vertex(samples):
    """Lens (0, 1, 0): every sample is the pixel centre's ray and vertex 0 is shaded by k_shade_punct<false, true, true> from hit_info's
    unquantised surface.  One point light, B = 2, no sky, no emission, flags = PUNCTUAL alone (Lambert): a pixel is
        albedo / pi x I' max(0, n' . wl) / d^2, or 0 in the occluder's shadow,
    n' the normal-mapped shading normal (ref_materials), albedo the fp32 factor (no G-buffer in a lens frame: nothing is quantised).

    The bound is test_punctual_lights.closed_form_bound's, derived the same way, without its G-buffer terms and with one term more:
      * 32 fp32 roundings on the way from the hit point to the sample, one per sample added and the division: (33 + S) eps, relative;
      * the range window 1 - (d / range)^4: |dw| <= 32 eps, taken at both ends of its clamp (exactly 0 beyond the range);
      * the normal: hit_info's n' is within ref_materials' derived angle `normal_bound` of the float64 one, and |d max(0, n . wl)| is at
        most that angle: albedo / pi x I' / d^2 x normal_bound wherever the light is not occluded;
      * the hit point: the kernels reach it through under 64 roundings of magnitudes up to |o| + t; the closed form -- normal map lookup
        included -- is evaluated at x -+ that distance along each axis, and twice the summed change covers any direction and the curvature.
    A pixel whose shadow test changes within 1e-3 of its hit point lies on the shadow's edge and is left out (at most 5 %)."""
    window = (64, 48)
    mesh, light = mapped_floor(), FLOOR_LAMP
    mesh.lights = assets.lights_array([light])
    pt = build_pt(mesh, window, lens=(0.0, 1.0, 0.0), sky=False)
    try:
        assert_instance_conditions(pt, mesh, P, punct=True, mat=True, lds=True)
        got = shot(pt, P, samples, 2, window=window, cam=PW.FLOOR_CAMERA).reshape(-1, 3)
    finally:
        pt.close()
    scene = RP.Scene(mesh)
    surface = RLE.textured_surface(mesh, scene)
    o, d = device_rays(PW.FLOOR_CAMERA, window)
    tri, t, n0 = scene.trace(o, d)
    assert (tri >= 0).all()
    x = o + t[:, None] * d
    on_floor = scene.geom[tri] == mesh.names.index("floor")
    alb = scene.albedo[scene.geom[tri]]
    plain = light.copy()  # the same light without its window: what the factor multiplies
    plain["range"] = 0.0

    def at(points, lamp=light):
        Ei, wl, dist = RLI.irradiance(lamp, points, surface(tri, points, n0)[2])
        lit = np.any(Ei > 0.0, -1)
        if lit.any():
            lit[lit] = ~RLI.occluded(scene, points[lit], wl[lit], dist[lit])
        return np.where(lit[:, None], alb / np.pi * Ei, 0.0)

    ref, base = at(x), at(x, plain)
    wl, dist, _, geo = RLI.light_sample(plain, x)
    occluded = RLI.occluded(scene, x, wl, dist)
    _, w = RLI.cone_window_raw(light, x)
    k, k_hi, k_lo = np.clip(w, 0, 1), np.clip(w + 32 * EPS, 0, 1), np.clip(w - 32 * EPS, 0, 1)
    bound = (33 + samples) * EPS * base * k_hi[:, None] + base * np.maximum(k_hi - k, k - k_lo)[:, None]
    angle = RM.reference(mesh, None, tri, *barycentrics(scene, tri, x)).normal_bound
    intensity = light["intensity"].astype(np.float64)
    bound += np.where(occluded[:, None], 0.0, alb / np.pi * intensity * (geo * k_hi * angle)[:, None])
    delta = 64.0 * EPS * (np.abs(np.asarray(PW.FLOOR_CAMERA["position"])).max() + t)
    edge = np.zeros(len(x), bool)
    for axis in range(3):
        step = np.zeros((len(x), 3))
        step[:, axis] = delta
        bound += 2.0 * np.maximum(np.abs(at(x + step) - ref), np.abs(at(x - step) - ref))
        if axis != 1:  # along the floor: does the shadow test change within 1e-3?
            for s in (-1e-3, 1e-3):
                moved = x.copy()
                moved[:, axis] += s
                wl_m, dist_m, _, _ = RLI.light_sample(plain, moved)
                edge |= RLI.occluded(scene, moved, wl_m, dist_m) != occluded
    use = ~edge
    assert edge.mean() <= 0.05
    lit = use & ~occluded & (k > 0) & np.any(ref > 0, -1)
    assert (use & occluded & on_floor & (k > 0)).sum() > 30 and (lit & on_floor).sum() > 500 and (k_hi == 0).sum() > 50, "umbra, lit floor and the range's end are in view"
    check_closed_form(got, ref, bound, use, f"lens vertex 0, S={samples}")
    assert ref.max() > 0.1
    flat = alb / np.pi * RLI.irradiance(light, x, n0)[0]  # the same pixel under the vertex normal
    assert np.mean((np.abs(flat - ref) > 4.0 * bound).any(-1)[lit & on_floor]) > 0.5, "the bound tells the mapped normal from the vertex normal"


# ---------------------------------------------------------------------------------------------------------------- e. traversal
EVERYTHING = "lens_lights_textures_cutout"
ALL_FLAGS = FULL | P | E


def everything_frame(mode=0, options=(), window=CW.WINDOW, after=None, spp=4, **kw):
    """(radiance, stats) of one frame of the world with every feature on"""
    mesh, lens = CW.world(EVERYTHING)
    pt = build_pt(mesh, window, lens=lens, options={L.OPT_INSTANCE_MODE: mode, **dict(options)}, **kw)
    try:
        assert_instance_conditions(pt, mesh, ALL_FLAGS, punct=True, mat=True, lds=True, masked=True)
        if after:
            after(pt)
        pt.ctx.stats_reset()
        light = shot(pt, ALL_FLAGS, spp, window=window)
        return light, pt.ctx.stats(), pt.ctx.exit_table_info()
    finally:
        pt.close()


@pytest.mark.parametrize("mode", (0, 1), ids=("flat", "two_level"))
def test_counting_keeps_the_masked_lit_frame(mode):
    """RT3_OPT_COUNT_TRAVERSAL 0 against 1 on a masked scene with range rays: k_extend<COUNT, L, true>, k_shadow<COUNT, L, RANGE, true>
    for L = the default layout (mode 0) and the two-level one (mode 1)"""
    profile = lambda pt: pt.ctx.set_option(L.OPT_PROFILE, 1)  # noqa: E731  (launches are counted under RT3_OPT_PROFILE)
    (a, sa, _), (b, sb, _) = everything_frame(mode, {L.OPT_COUNT_TRAVERSAL: 0}, after=profile), everything_frame(mode, {L.OPT_COUNT_TRAVERSAL: 1}, after=profile)
    assert a.mean() > 0 and np.array_equal(bits(a), bits(b))
    assert sa.extension_rays == sb.extension_rays > 0 and sa.shadow_rays == sb.shadow_rays > 0
    assert sa.extend_launches == sb.extend_launches >= 3 and sa.shadow_launches == sb.shadow_launches  # (camera rays, then one per vertex but the last)
    assert sa.shadow_launches >= 4, "sky and range shadow rays are launched apart at the two vertices that sample lights"
    for f in ("nodes_visited", "tris_tested", "shadow_nodes_visited", "shadow_tris_tested"):
        assert getattr(sb, f) > 0, f


def test_exit_table_keeps_the_masked_lit_frame():
    """k_shadow_exit<true> (the sky's shadow rays, table on) against k_shadow<false, 2, false, true> (table off), with lights in the frame"""
    on, _, info_on = everything_frame()
    off, _, info_off = everything_frame(after=lambda pt: pt.ctx.set_option(L.OPT_SHADOW_EXIT_TABLE, 0))
    assert info_on[0] != 0 and info_on[1] > 0 and info_off[:2] == (0, 0)
    assert on.mean() > 0 and np.array_equal(bits(on), bits(off))


def test_batches_keep_the_masked_lit_frame():
    auto, _, _ = everything_frame(spp=6)
    one, _, _ = everything_frame(spp=6, options={L.OPT_BATCH_SPP: 1})
    assert np.array_equal(bits(auto), bits(one))


def test_tile_partition_keeps_the_masked_lit_frame():
    window = (128, 48)  # two 64 x 64 tiles: the smallest window in which both of two ranks own pixels
    whole, _, _ = everything_frame(window=window)
    for r in range(2):
        part, _, _ = everything_frame(window=window, rank=r, n_ranks=2)
        m = owned_mask(window[0], window[1], r, 2)
        assert m.any() and not m.all() and np.array_equal(bits(part[m]), bits(whole[m]))


# (RT3_OPT_NODE_WIDTH, RT3_OPT_NODE_QUANT) -> the layout number in the instance names: kLayoutBinary64, kLayoutWide128, kLayoutWide48Q
OTHER_LAYOUTS = {0: (2, 0), 1: (4, 0), 3: (4, 2)}


@pytest.mark.parametrize("count", (0, 1), ids=("plain", "counting"))
@pytest.mark.parametrize("layout", sorted(OTHER_LAYOUTS))
def test_range_rays_in_every_node_layout(layout, count):
    """A hit is a set's minimum over (t, prim), whatever the walk: every node layout gives the default layout's
    frame bit for bit -- which test_against_fixture[lens_lights] pins -- with light and emitter range rays in it:
    k_extend<COUNT, L, false>, k_shadow<COUNT, L, false, false> and k_shadow<COUNT, L, true, false>"""
    width, quant = OTHER_LAYOUTS[layout]
    mesh, lens = CW.world("lens_lights")
    out = []
    for options in ({}, {L.OPT_NODE_WIDTH: width, L.OPT_NODE_QUANT: quant, L.OPT_COUNT_TRAVERSAL: count}):
        pt = build_pt(mesh, lens=lens, options=options)
        try:
            assert_instance_conditions(pt, mesh, ALL_FLAGS, punct=True, mat=False, lds=True, masked=False)
            pt.ctx.stats_reset()
            out.append((shot(pt, ALL_FLAGS), pt.ctx.stats(), pt.ctx.accel_info()[3]))
        finally:
            pt.close()
    (a, sa, bytes_a), (b, sb, bytes_b) = out
    assert bytes_a == 64 and bytes_b == {0: 64, 1: 128, 3: 48}[layout], "the node size names the layout"
    assert a.mean() > 0 and np.array_equal(bits(a), bits(b))
    assert sa.shadow_rays == sb.shadow_rays > 0 and sa.extension_rays == sb.extension_rays
    assert (sb.shadow_nodes_visited > 0) == bool(count)


# ---------------------------------------------------------------------------------------------------------------- f. lens rays and cutouts
def rect_behind(front_px, material, texture=None, depth=2.0):
    """lens_worlds' emissive rectangle at depth 4 and, in front of it, a quad whose corners show at the pixel coordinates front_px
    (x0, x1, y0, y1), with uvs (0, 0) .. (1, 1): (mesh, world corners of the rectangle, world corners of the front quad)"""
    x0, x1, y0, y1 = front_px
    c = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]])
    mb = MeshBuilder()
    mb.add("rect", LW.pixel_to_world(*LW.rect_corners().T, LW.RECT_DEPTH), np.tile([0.0, 0.0, 1.0], (4, 1)), None, [[0, 1, 2], [0, 2, 3]],
           Material((0.0, 0.0, 0.0), 0.0, 1.0, emission=LW.EMISSION))
    if material is not None:
        mb.add("front", LW.pixel_to_world(c[:, 0], c[:, 1], depth), np.tile([0.0, 0.0, 1.0], (4, 1)), [[0, 0], [1, 0], [1, 1], [0, 1]],
               [[0, 1, 2], [0, 2, 3]], material)
    mesh = mb.build()
    if texture is not None:
        mesh.textures = [texture]
    return mesh, mesh.vertices[:4, :3].astype(np.float64), mesh.vertices[4:8, :3].astype(np.float64)


FRONT_PX = (6.2, 24.6, 3.3, 19.1)  # fractional bounds; it covers the rectangle (9.3 .. 20.65 x 5.4 .. 16.25) from every point of the lens


def lens_shot(mesh, lens, spp):
    pt = make_pt(mesh, LW.WINDOW)
    try:
        pt.set_lens(*lens)
        masked = bool(np.any(mesh.alpha_cutoffs > 0))
        light, g = lens_frame(pt, camera(LW.CAMERA, LW.WINDOW), 0, spp, 1)
        return light, g, masked
    finally:
        pt.close()


@pytest.mark.parametrize("how", ("texture", "base_alpha"))
def test_lens_rays_pass_a_transparent_quad(how):
    """k_lens_rays' rays through k_extend<false, 2, true>: with R > 0 and jitter 1 the frame has the bits of the frame without the quad"""
    lens = (0.3, LW.RECT_DEPTH, 1.0)
    if how == "texture":
        mesh = rect_behind(FRONT_PX, Material((0.9, 0.9, 0.9), texture_offset=0, alpha_cutoff=0.5), CW.constant_alpha(0))[0]
    else:
        mesh = rect_behind(FRONT_PX, Material((0.9, 0.9, 0.9), alpha_cutoff=0.5, alpha=0.0))[0]
    a, _, masked = lens_shot(mesh, lens, 64)
    b, _, plain = lens_shot(rect_behind(FRONT_PX, None)[0], lens, 64)
    assert masked and not plain
    assert a.max() > 0 and np.array_equal(bits(a), bits(b))
    solid, _, _ = lens_shot(rect_behind(FRONT_PX, Material((0.0, 0.0, 0.0)))[0], lens, 64)
    assert not solid.any(), "(opaque, the quad hides the rectangle from the whole lens)"


def test_lens_rays_pass_the_open_cells_of_a_checker():
    """R = 0, jitter 1, B = 1: a sample is Le when its film point lies in the rectangle's image and in an open cell of the checker in front
    (bilinear alpha of 0 / 255 texels against the cutoff 0.5: the cells are the texels' own squares), else 0.  Both are axis-aligned in the
    image, so a pixel's lit share is the sum over the open cells of the area of pixel box x rectangle x cell: test_antialiasing_closed_form's
    binomial band around it."""
    S = 1024
    tex = CW.checker()
    mesh, rect_w, front_w = rect_behind(FRONT_PX, Material((0.0, 0.0, 0.0), texture_offset=0, alpha_cutoff=0.5), tex)
    light, g, masked = lens_shot(mesh, (0.0, 1.0, 1.0), S)
    assert masked
    pinv, vinv = RLE.gconst_matrices(g)
    r, f = LW.project(pinv, vinv, rect_w), LW.project(pinv, vinv, front_w)
    rx0, rx1, ry0, ry1 = r[:, 0].min(), r[:, 0].max(), r[:, 1].min(), r[:, 1].max()
    fx0, fx1, fy0, fy1 = f[:, 0].min(), f[:, 0].max(), f[:, 1].min(), f[:, 1].max()
    assert f[0, 0] < f[1, 0] and f[0, 1] < f[3, 1], "u runs right and v runs down in the image"
    a = np.zeros((LW.WINDOW[1], LW.WINDOW[0]))
    n = tex.shape[0]
    for ty in range(n):
        for tx in range(n):
            if tex[ty, tx, 3] == 0:
                cx0, cx1 = fx0 + (fx1 - fx0) * tx / n, fx0 + (fx1 - fx0) * (tx + 1) / n
                cy0, cy1 = fy0 + (fy1 - fy0) * ty / n, fy0 + (fy1 - fy0) * (ty + 1) / n
                if min(cx1, rx1) > max(cx0, rx0) and min(cy1, ry1) > max(cy0, ry0):
                    a += RLE.box_coverage(max(cx0, rx0), min(cx1, rx1), max(cy0, ry0), min(cy1, ry1), LW.WINDOW)
    whole = RLE.box_coverage(rx0, rx1, ry0, ry1, LW.WINDOW)
    assert 0.35 < a.sum() / whole.sum() < 0.65 and np.all(a <= whole + 1e-12), "about half of the rectangle shows"
    check_binomial(light, a, LW.LE, np.zeros(3), S, "checker in front of the rectangle")
    assert not light[a == 0.0].any()


# ---------------------------------------------------------------------------------------------------------------- g. the ledger
# instance (as the demangled symbol names it) -> (what selects it, the test that launches it under a reference).  Template arguments:
#   k_shade<FIRST, GLDS, EMIT, MAT>, k_shade_punct<FIRST, GLDS, MAT> (EMIT and PUNCT on), k_extend<COUNT, LAYOUT, MASK>,
#   k_shadow<COUNT, LAYOUT, RANGE, MASK>, k_shadow_exit<MASK>;  LAYOUT 0 binary, 1 wide 128 B, 2 wide 64 B quantised (default), 3 wide
#   48 B, 4 two-level.
# FIRST: the pinhole frame's vertex 0, from the G-buffer; a lens frame shades vertex 0 with the FIRST = false instances.  GLDS: at most 256
# flattened geometries.  EMIT: RT3_F_NEE_EMISSIVE (or PUNCTUAL) with a non-empty table.  MAT: the scene has a material-texture table.
# COUNT: RT3_OPT_COUNT_TRAVERSAL.  RANGE: emitter and punctual shadow rays, which end at their light.  MASK: a built alpha cutout.
HERE = "tests/test_combined.py"
LEDGER = {
    "k_shade<true, false, false, false>": ("pinhole vertex 0", "tests/test_gpu_parity.py::test_frame_parity_atrium"),
    "k_shade<true, false, true, false>": ("pinhole vertex 0, emitter NEE", "tests/test_nee_emissive.py::test_floor_under_square_light"),
    "k_shade<false, true, false, false>": ("later vertices, LDS table", "tests/test_gpu_parity.py::test_frame_parity_atrium"),
    "k_shade<false, true, true, false>": ("LDS table, emitter NEE", "tests/test_nee_emissive.py::test_same_expectation"),
    "k_shade<false, true, false, true>": ("LDS table, material textures", "tests/test_lens.py::test_textured_first_vertex_against_fixture"),
    "k_shade<false, true, true, true>": ("LDS table, emitter NEE, material textures", "tests/test_materials.py::test_constant_maps_equal_folded_factors"),
    "k_shade<false, false, false, false>": ("more than 256 geometries", "tests/test_shade_tables.py::test_frames_equal_the_oracle"),
    "k_shade<false, false, true, false>": ("more than 256 geometries, emitter NEE", "tests/test_shade_tables.py::test_lds_table_equals_global_table"),
    "k_shade<false, false, false, true>": ("more than 256 geometries, material textures", "tests/test_materials.py::test_normal_maps_across_the_lds_table_limit"),
    "k_shade<false, false, true, true>": ("more than 256 geometries, emitter NEE, material textures", "tests/test_materials.py::test_normal_maps_across_the_lds_table_limit"),
    "k_shade_punct<true, false, false>": ("pinhole vertex 0, a punctual record in the table", "tests/test_punctual_lights.py::test_closed_form"),
    "k_shade_punct<false, true, false>": ("LDS table, punctual record; vertex 0 of a lit lens frame", f"{HERE}::test_against_fixture"),
    "k_shade_punct<false, true, true>": ("LDS table, punctual record, material textures", f"{HERE}::test_closed_form_at_a_textured_lens_vertex"),
    "k_shade_punct<false, false, false>": ("more than 256 geometries, punctual record", f"{HERE}::test_table_switch_under_lights_256_to_257"),
    "k_shade_punct<false, false, true>": ("more than 256 geometries, punctual record, material textures", f"{HERE}::test_table_switch_under_lights_256_to_257"),
    "k_shadow_exit<false>": ("sky shadow rays, default layout, exit table on, not counting", "tests/test_shadow_exit_table.py::test_frames_do_not_depend_on_the_table"),
    "k_shadow_exit<true>": ("the same in a scene with a cutout", f"{HERE}::test_exit_table_keeps_the_masked_lit_frame"),
}
for _count in ("false", "true"):
    _c = "counting, " if _count == "true" else ""
    for _layout, _what in ((0, "binary nodes"), (1, "128-byte nodes"), (3, "48-byte nodes")):
        LEDGER[f"k_extend<{_count}, {_layout}, false>"] = (f"{_c}{_what}", f"{HERE}::test_range_rays_in_every_node_layout")
        LEDGER[f"k_shadow<{_count}, {_layout}, false, false>"] = (f"{_c}{_what}, sky shadow rays", f"{HERE}::test_range_rays_in_every_node_layout")
        LEDGER[f"k_shadow<{_count}, {_layout}, true, false>"] = (f"{_c}{_what}, range rays", f"{HERE}::test_range_rays_in_every_node_layout")
    for _layout, _what, _plain in ((2, "default layout", "tests/test_gpu_parity.py::test_traversal_counting_keeps_the_frame"),
                                   (4, "two-level", "tests/test_instances_two_level.py::test_two_level_frame_bit_identical")):
        _masked = f"{HERE}::test_counting_keeps_the_masked_lit_frame"
        _ranged = "tests/test_nee_emissive.py::test_same_expectation" if _layout == 2 else "tests/test_punctual_lights.py::test_gpu_against_fixture_two_level"
        _sky = "tests/test_shadow_exit_table.py::test_frames_do_not_depend_on_the_table" if _layout == 2 else _plain  # (the table switched off)
        if _count == "true":
            _ranged = "tests/test_alpha_mask.py::test_opaque_mask_walks_like_unmasked"  # (its unmasked twin scene, counted, with emitter NEE)
            _plain = _sky = _plain if _layout == 2 else _ranged
        LEDGER[f"k_extend<{_count}, {_layout}, false>"] = (f"{_c}{_what}", _plain)
        LEDGER[f"k_extend<{_count}, {_layout}, true>"] = (f"{_c}{_what}, cutout", _masked)
        LEDGER[f"k_shadow<{_count}, {_layout}, false, false>"] = (f"{_c}{_what}, sky shadow rays (default layout: exit table off or counting)", _sky)
        LEDGER[f"k_shadow<{_count}, {_layout}, true, false>"] = (f"{_c}{_what}, range rays", _ranged)
        LEDGER[f"k_shadow<{_count}, {_layout}, false, true>"] = (f"{_c}{_what}, sky shadow rays, cutout", _masked if (_layout == 4 or _count == "true") else f"{HERE}::test_exit_table_keeps_the_masked_lit_frame")
        LEDGER[f"k_shadow<{_count}, {_layout}, true, true>"] = (f"{_c}{_what}, range rays, cutout", _masked)
# No instance is unreachable: MASK exists only for the two layouts rt3_accel_build accepts with cutouts (it refuses the others:
# tests/test_alpha_mask.py::test_errors), so there is no k_extend<*, 0 | 1 | 3, true> to list.
UNREACHABLE = {}


def library_instances():
    """the template instances of the five kernels in librt3.so's symbol table (their host stubs; names only)"""
    lib = ROOT / "raytracer3_amd" / "librt3.so"
    out = None
    for nm in ("nm", "/opt/rocm/llvm/bin/llvm-nm"):
        try:
            out = subprocess.run([nm, "-C", str(lib)], capture_output=True, text=True, check=True).stdout
            break
        except (OSError, subprocess.CalledProcessError):
            continue
    assert out is not None, "neither nm nor llvm-nm could read the library"
    return set(re.findall(r"__device_stub__((?:k_shade|k_shade_punct|k_extend|k_shadow|k_shadow_exit)<[^>]*>)\(", out))


def test_instance_ledger():
    """fails when a kernel instance is added without an entry here, or an entry outlives its instance, or a credited test is gone"""
    have = library_instances()
    assert len(have) >= 59, sorted(have)
    listed = set(LEDGER) | set(UNREACHABLE)
    assert not have - listed, f"instances without a ledger entry: {sorted(have - listed)}"
    assert not listed - have, f"ledger entries without an instance: {sorted(listed - have)}"
    for name, (conditions, credit) in LEDGER.items():
        path, _, test = credit.partition("::")
        assert conditions and re.search(rf"^def {re.escape(test)}\(", (ROOT / path).read_text(), re.M), (name, credit)
