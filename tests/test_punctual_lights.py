"""RT3_F_NEE_PUNCTUAL on the GPU: point, spot and directional lights as entries of the light table.

A frame with one light, B = 2, no sky and no emission is deterministic (p_sel = 1, the first vertex from the G-buffer), so it is compared
pixel by pixel with the float64 closed form of tests/ref_lights.py inside a derived rounding bound; shadows, range and cone borders are
exact zeros.  Then: the bit-exact no-op cases, the table's masses against numpy, unbiased selection between two lights, the union with the
emitter triangles, the whole integrator against tests/golden/punctual_ref.npz, and the plumbing (instance modes, tile partition, batches,
statistics, late rt3_scene_set_lights, refusals)."""
import math

import numpy as np
import pytest

import integrator_worlds as IW
import punctual_worlds as PW
import ref_lights as RL
import ref_pathtrace as RP
from raytracer3_amd import _lib as L
from raytracer3_amd import scenes
from raytracer3_amd.assets import LIGHT_DIRECTIONAL, LIGHT_POINT, LIGHT_SPOT, make_light
from raytracer3_amd.render_graph import Context
from support import bits, camera
from test_alpha_mask_cpu import tex_alpha_f64
from test_integrator_cpu import check_against_fixture
from test_nee_emissive import FULL, SPEC_FF, block_z, frame, make_pt, owned_mask
from test_nee_emissive_cpu import CDF_TOTAL
from test_punctual_lights_cpu import fixture

pytestmark = pytest.mark.gpu

P, E = L.F_NEE_PUNCTUAL, L.F_NEE_EMISSIVE
EPS = 2.0**-24
WINDOW = (64, 48)


def lit_pt(mesh, lights, window=WINDOW, **kw):
    pt = make_pt(mesh, window, **kw)
    if lights is not None and len(lights):
        pt.ctx.set_lights(lights)
    return pt


def gpu_frame(mesh, lights, cam, flags, spp, bounces, window=WINDOW, index=0, gbuffer=False, **kw):
    """the frame's radiance; with `gbuffer` also the G-buffer words it started from"""
    pt = lit_pt(mesh, lights, window, **kw)
    try:
        light = frame(pt, camera(cam, window), flags, spp, bounces, index=index)
        return (light, pt.gbuffer()[0].copy()) if gbuffer else light
    finally:
        pt.close()


def device_rays(cam, window):
    """the primary rays as the kernels define them (primary_ray, rt3_camera.hpp), evaluated in float64 from the fp32 matrices of the
    frame's GConst -- inputs, taken as exact like the fp32 vertices: origins and (not renormalised) directions per pixel, row by row"""
    W, H = window
    g = camera(cam, window).gconst(window)
    pinv = np.array(g.proj_inverse[:], np.float64).reshape(4, 4).T
    vinv = np.array(g.view_inverse[:], np.float64).reshape(4, 4).T
    py, px = np.mgrid[0:H, 0:W]
    dx, dy = (px + 0.5) / W * 2 - 1, -((py + 0.5) / H * 2 - 1)
    t = np.stack([dx, dy, np.ones_like(dx), np.ones_like(dx)], -1) @ pinv.T
    t = t[..., :3] / np.linalg.norm(t[..., :3], axis=-1, keepdims=True)
    d = (t @ vinv[:3, :3].T).reshape(-1, 3)
    return np.broadcast_to(vinv[:3, 3], d.shape).copy(), d


# ---------------------------------------------------------------------------------------------------------------- the rounding bound
def closed_form_bound(scene, light, cam, window, samples, gb, shadows=True):
    """(closed form (H, W, 3), bound (H, W, 3), covered (H, W), float64 hit points (H W, 3)) of a one-light B = 2 frame whose first vertex
    has the normal and albedo of the G-buffer words `gb`.

    The bound has three parts, none of them measured:
      * products and sums in fp32, one rounding each: the G-buffer albedo (2), P - x (1), d^2 (3), sqrt, 1 / d, wl (3), N . wl (3),
        1 / d^2 (1), cs / d^2, / p_sel, / pi with pi's own rounding (4), c^2 window and I' (3), T f, I' scale, their product (3), and the
        rounding of every intermediate these feed: 32 in all, plus one per sample added and the division by S;
      * the clamped factors: c is a difference of terms of size a = 1 / (cos inner - cos outer), whose own relative rounding is amplified
        by the same cancellation, so |dc| <= 16 eps a; in 1 - (d / range)^4 the relative rounding of d (4 eps) and of 1 / range and
        the product (2) is raised to the fourth power with one rounding per squaring, 27 eps, and the difference adds one: |dw| <= 32 eps.
        The bound takes clamp(c -+ dc)^2 clamp(w -+ dw) at both ends, so it is exactly 0 wherever both clamp to 0;
      * the hit point: the reference follows the kernels' own ray (device_rays) in float64; the kernels evaluate it through two fp32
        4 x 4 products, a normalisation, the traversal's Moeller-Trumbore t and x = o + t d -- under 64 roundings of magnitudes up to
        |o| + t.  The closed form is evaluated at x -+ that distance along each axis; twice the summed first-order change covers an
        error in any direction and the curvature."""
    W, H = window
    rays = device_rays(cam, window)
    ref, cov, x, at = RL.direct_light(scene, [light], cam, window, shadows, rays, gb)
    ref = ref.reshape(-1, 3)
    c, w = RL.cone_window_raw(light, x)
    a = 0.0
    if int(light["type"]) == LIGHT_SPOT:
        a = 1.0 / max(0.001, math.cos(float(light["inner_cone"])) - math.cos(float(light["outer_cone"])))
    dc, dw = 16.0 * EPS * a, (32.0 * EPS if float(light["range"]) > 0.0 and int(light["type"]) != LIGHT_DIRECTIONAL else 0.0)
    k = np.clip(c, 0, 1) ** 2 * np.clip(w, 0, 1)
    k_hi = np.clip(c + dc, 0, 1) ** 2 * np.clip(w + dw, 0, 1)
    k_lo = np.clip(c - dc, 0, 1) ** 2 * np.clip(w - dw, 0, 1)
    plain = light.copy()  # the same light without cone and window: what the factors multiply
    if int(light["type"]) == LIGHT_SPOT:
        plain["type"] = LIGHT_POINT
    plain["range"] = 0.0
    base = RL.direct_light(scene, [plain], cam, window, shadows, rays, gb)[0].reshape(-1, 3)
    bound = (32 + samples + 1) * EPS * base * k_hi[:, None] + base * np.maximum(k_hi - k, k - k_lo)[:, None]
    o = np.asarray(cam["position"], np.float64)
    delta = 64.0 * EPS * (np.abs(o).max() + np.linalg.norm(x - o, axis=1))
    for axis in range(3):
        step = np.zeros((len(x), 3))
        step[:, axis] = delta
        bound += 2.0 * np.maximum(np.abs(at(x + step) - ref), np.abs(at(x - step) - ref))
    return ref.reshape(H, W, 3), bound.reshape(H, W, 3), cov, x


def check_closed_form(got, ref, bound, use, label):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err[use] / np.maximum(ref[use], 1e-30)).max()) if use.any() else 0.0
    zero = use[..., None] & (bound == 0.0)
    print(f"{label}: {int(use.sum())} pixels, largest relative error {worst:.2e}, largest error / bound "
          f"{float((err[use] / np.maximum(bound[use], 1e-300))[bound[use] > 0].max()):.3f}, {int(zero.all(-1).sum())} pixels exactly black")
    assert np.all(err[use] <= bound[use])
    assert np.all(got[zero] == 0.0), "outside the cone, beyond the range and in shadow a pixel is exactly 0.0"


# ---------------------------------------------------------------------------------------------------------------- 1 closed form
@pytest.mark.parametrize("samples", (1, 4))
@pytest.mark.parametrize("kind", ("point", "spot", "directional"))
def test_closed_form(kind, samples):
    mesh, light = PW.floor_world(), PW.FLOOR_LIGHTS[kind]
    got, gb = gpu_frame(mesh, PW.lights(light), PW.FLOOR_CAMERA, P, samples, 2, gbuffer=True)
    ref, bound, cov, _ = closed_form_bound(RP.Scene(mesh), light, PW.FLOOR_CAMERA, WINDOW, samples, gb)
    assert cov.all()
    check_closed_form(got, ref, bound, cov, f"{kind} S={samples}")
    assert ref.max() > 0.1
    black = (ref == 0.0).all(-1) & (bound == 0.0).all(-1)
    if kind != "directional":  # the point light's range and the spot's outer cone both end inside the view
        assert black.sum() > 50 and (~black).sum() > 50


# ---------------------------------------------------------------------------------------------------------------- 2 shadows
def edge_distance(x, rect):
    """distance of floor points (x, z) to the outline of the rectangle ((x0, x1), (z0, z1))"""
    (x0, x1), (z0, z1) = rect
    dx, dz = np.maximum(np.maximum(x0 - x[:, 0], x[:, 0] - x1), 0.0), np.maximum(np.maximum(z0 - x[:, 2], x[:, 2] - z1), 0.0)
    outside = np.hypot(dx, dz)
    inside = np.minimum(np.minimum(x[:, 0] - x0, x1 - x[:, 0]), np.minimum(x[:, 2] - z0, z1 - x[:, 2]))
    return np.where(outside > 0.0, outside, inside)


@pytest.mark.parametrize("kind", ("point", "spot", "directional"))
def test_shadow_of_a_quad(kind):
    mesh, light = PW.floor_world(occluder=True), PW.FLOOR_LIGHTS[kind].copy()
    light["range"] = 0.0
    got, gb = gpu_frame(mesh, PW.lights(light), PW.FLOOR_CAMERA, P, 1, 2, gbuffer=True)
    scene = RP.Scene(mesh)
    ref, bound, cov, x = closed_form_bound(scene, light, PW.FLOOR_CAMERA, WINDOW, 1, gb)
    H, W = cov.shape
    on_floor = np.abs(x[:, 1]) < 1e-9
    near_edge = (on_floor & (edge_distance(x, PW.shadow_rect(light)) < 1e-3)).reshape(H, W)
    assert cov.all() and near_edge.sum() <= 0.05 * cov.sum()
    use = cov & ~near_edge
    # off the edge the hit point's rounding cannot change which side a pixel is on: the bound there is the lit or the dark one
    umbra = use & (ref == 0.0).all(-1) & on_floor.reshape(H, W) & (edge_distance(x, PW.shadow_rect(light)).reshape(H, W) >= 1e-3)
    inside = np.array([PW.shadow_rect(light)[0][0] < p[0] < PW.shadow_rect(light)[0][1] and PW.shadow_rect(light)[1][0] < p[2] < PW.shadow_rect(light)[1][1] for p in x]).reshape(H, W)
    check_closed_form(got, ref, np.where((umbra & inside)[..., None], 0.0, bound), use, f"shadow {kind}")
    assert (umbra & inside).sum() > 30, "the camera sees the umbra"
    assert np.all(got[umbra & inside] == 0.0)
    # lit pixels equal the frame without the occluder, where the camera sees the floor in both
    free = gpu_frame(PW.floor_world(), PW.lights(light), PW.FLOOR_CAMERA, P, 1, 2)
    lit_floor = use & on_floor.reshape(H, W) & ~inside
    assert lit_floor.sum() > 500 and np.array_equal(bits(got[lit_floor]), bits(free[lit_floor]))


def test_wall_behind_the_point_light_changes_nothing():
    light = PW.lights(PW.FLOOR_LIGHTS["point"])
    a = gpu_frame(PW.floor_world(), light, PW.FLOOR_CAMERA, P, 2, 2)
    b = gpu_frame(PW.floor_world(ceiling=3.0), light, PW.FLOOR_CAMERA, P, 2, 2)  # above the light (y = 1.5) and the camera (y = 2.4)
    assert a.max() > 0.1 and np.array_equal(bits(a), bits(b))


def test_directional_light_is_occluded_from_any_distance():
    light = PW.lights(PW.FLOOR_LIGHTS["directional"])
    a = gpu_frame(PW.floor_world(), light, PW.FLOOR_CAMERA, P, 1, 2)
    b = gpu_frame(PW.floor_world(ceiling=900.0), light, PW.FLOOR_CAMERA, P, 1, 2)
    assert a.min() > 0.01 and not b.any()


def test_mask_cutout_casts_its_checker():
    mesh, light = PW.floor_world(cutout=True), PW.FLOOR_LIGHTS["point"].copy()
    light["range"] = 0.0
    got, gb = gpu_frame(mesh, PW.lights(light), PW.FLOOR_CAMERA, P, 1, 2, gbuffer=True)
    floor = PW.floor_world()
    # the unshadowed floor (pixels that show the cutout itself carry its words and are not compared: `seen_direct` below)
    ref, bound, cov, x = closed_form_bound(RP.Scene(floor), light, PW.FLOOR_CAMERA, WINDOW, 1, gb)
    H, W = cov.shape
    (x0, x1), h, (z0, z1) = PW.OCCLUDER

    def crossing(a, b):  # where the segments a -> b cross the cutout's plane: (u, v) of the quad, metres per unit of u and v at the floor
        s = (h - a[:, 1]) / (b[:, 1] - a[:, 1])
        p = a + s[:, None] * (b - a)
        return (p[:, 0] - x0) / (x1 - x0), (z1 - p[:, 2]) / (z1 - z0)

    def edge_metres(u, v, scale):  # distance to the nearest border of a checker cell or of the quad, in metres on the floor
        du = np.minimum.reduce([np.abs(u - e) for e in (0.0, 0.5, 1.0)]) * (x1 - x0) * scale
        dv = np.minimum.reduce([np.abs(v - e) for e in (0.0, 0.5, 1.0)]) * (z1 - z0) * scale
        inside = (u > 0) & (u < 1) & (v > 0) & (v < 1)
        out = np.hypot(np.maximum(np.maximum(-u, u - 1.0), 0.0) * (x1 - x0), np.maximum(np.maximum(-v, v - 1.0), 0.0) * (z1 - z0)) * scale
        return np.where(inside, np.minimum(du, dv), out), inside

    Pl = np.broadcast_to(light["position"].astype(np.float64), x.shape)
    cam_o = np.broadcast_to(np.asarray(PW.FLOOR_CAMERA["position"], np.float64), x.shape)
    cu, cv = crossing(cam_o, x)
    seen_direct = ~((cu > -0.01) & (cu < 1.01) & (cv > -0.01) & (cv < 1.01))  # the primary ray passes beside the cutout: the pixel is floor
    lu, lv = crossing(x, Pl)
    dist, inside = edge_metres(lu, lv, float(light["position"][1]) / (float(light["position"][1]) - h))
    near_edge = (seen_direct & (dist < 1e-3)).reshape(H, W)
    assert near_edge.sum() <= 0.05 * cov.sum()
    opaque = inside & (tex_alpha_f64(mesh.textures[0], lu, lv) >= 0.5)
    use = cov & seen_direct.reshape(H, W) & ~near_edge
    umbra = use & opaque.reshape(H, W)
    lit_in_hole = use & (inside & ~opaque).reshape(H, W)
    assert umbra.sum() > 20 and lit_in_hole.sum() > 20, "both kinds of checker cell are seen"
    check_closed_form(got, np.where(umbra[..., None], 0.0, ref), np.where(umbra[..., None], 0.0, bound), use, "cutout")
    assert np.all(got[umbra] == 0.0)


# ---------------------------------------------------------------------------------------------------------------- 3 bit-exact no-ops
THREE_LIGHTS = PW.lights(make_light(LIGHT_POINT, (6.0, 5.0, 4.0), position=(0.1, 1.2, 0.2)),
                         make_light(LIGHT_SPOT, (20.0, 20.0, 16.0), position=(-0.4, 1.7, 0.3), direction=(0.3, -1.0, -0.4), inner_cone=0.3, outer_cone=0.8),
                         make_light(LIGHT_DIRECTIONAL, (0.8, 0.7, 0.6), direction=(-0.2, -1.0, -0.3)))


def test_noops_are_bit_exact():
    mesh, sky = scenes.cornell(), scenes.sky(64, 32)
    pt = make_pt(mesh, WINDOW, sky=sky)
    try:
        cam = camera(scenes.CORNELL_CAMERA, WINDOW)
        plain, plain_e, one = frame(pt, cam, FULL, 4, 4), frame(pt, cam, FULL | E, 4, 4), frame(pt, cam, FULL, 4, 1)
        bare, bare_one = frame(pt, cam, 0, 4, 4), frame(pt, cam, 0, 4, 1)  # no flag at all: two RNG dimensions per vertex, not eight
        assert np.array_equal(bits(frame(pt, cam, FULL | P, 4, 4)), bits(plain)), "the flag without lights"
        assert np.array_equal(bits(frame(pt, cam, P, 4, 4)), bits(bare)) and bare.mean() > 0, "the flag alone without lights is flags = 0"
        pt.ctx.set_lights(THREE_LIGHTS)
        assert np.array_equal(bits(frame(pt, cam, FULL, 4, 4)), bits(plain)), "lights without the flag"
        assert np.array_equal(bits(frame(pt, cam, FULL | E, 4, 4)), bits(plain_e)), "RT3_F_NEE_EMISSIVE alone samples today's table"
        assert np.array_equal(bits(frame(pt, cam, FULL | P, 4, 1)), bits(one)), "B = 1: no vertex samples a light"
        assert np.array_equal(bits(frame(pt, cam, P, 4, 1)), bits(bare_one)), "B = 1 with the flag alone is flags = 0"
        lit = frame(pt, cam, FULL | P, 4, 4)
        assert lit.mean() > 1.05 * plain.mean(), "and with the flag the lights are there"
        pt.ctx.set_lights(None)
        assert np.array_equal(bits(frame(pt, cam, FULL | P, 4, 4)), bits(plain)), "(NULL, 0) forgets them"
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 4 table
def world_radius2(mesh):
    """R^2 as DESIGN.md section 4k defines it: a quarter of the squared diagonal of the box of the world's triangles (fp32 corners, the
    arithmetic in float64, the result rounded to fp32)"""
    tp = mesh.triangle_positions().reshape(-1, 3).astype(np.float64)
    return float(np.float32(0.25 * np.sum((tp.max(0) - tp.min(0)) ** 2)))


# instance mode, RT3_OPT_NODE_WIDTH: both instance modes and a node layout without quantised boxes
TABLE_BUILDS = {"flat": (0, None), "two_level": (1, None), "binary_nodes": (0, 2)}


def test_masses_match_numpy():
    mesh = scenes.cornell()
    want = RL.cdf_masses(RL.powers(THREE_LIGHTS, world_radius2(mesh)))
    assert want.min() > 1000, "every light has a mass the grid resolves"
    results = {}
    for name, (mode, width) in TABLE_BUILDS.items():
        ctx = Context()
        try:
            ctx.set_option(L.OPT_INSTANCE_MODE, mode)
            if width is not None:
                ctx.set_option(L.OPT_NODE_WIDTH, width)
            ctx.upload_mesh(mesh)
            ctx.set_lights(THREE_LIGHTS)
            ctx.build_accel()
            _, _, e_mass = ctx.light_download()
            got = {f: ctx.light_masses(f) for f in (P, E | P, E, 0)}
            if width is None:  # (a refit needs the default node layout)
                ctx.refit_accel()
                for f in (P, E | P, E):
                    again = ctx.light_masses(f)
                    assert again[:2] == got[f][:2] and np.array_equal(again[2], got[f][2]), "a refit of unmoved vertices leaves the table as it is"
        finally:
            ctx.close()
        n_e = len(e_mass)
        assert got[0][0] == got[0][1] == 0 and got[E][:2] == (n_e, 0) and np.array_equal(got[E][2], e_mass), "RT3_F_NEE_EMISSIVE: today's table"
        assert got[P][:2] == (0, 3) and got[E | P][:2] == (n_e, 3) and n_e > 0
        for f in (P, E | P):
            assert int(got[f][2].astype(np.int64).sum()) == CDF_TOTAL
        # the punctual table: 4 lum(I), 4 lum(I), lum(E) R^2 on 2^23 units (quantisation to 2^-24 of the largest, then the floor: 3 units)
        assert np.all(np.abs(got[P][2].astype(np.int64) - want) <= 3 + 2e-5 * want), (name, got[P][2], want)
        # the union: the emitters keep their ratios (area x luminance(12 e)), to the grid, and so do the lights
        m = got[E | P][2].astype(np.float64)
        e_only = got[E][2].astype(np.float64)
        share = m[:n_e].sum() / CDF_TOTAL
        assert np.all(np.abs(m[:n_e] - e_only * share) <= 3.0 + 2e-5 * e_only)
        assert np.all(np.abs(m[n_e:] / m[n_e:].sum() - want / want.sum()) <= 4.0 / m[n_e:].sum() + 2e-5)
        results[name] = got
    for name in ("two_level", "binary_nodes"):  # the same table whatever the structure
        for f in (P, E | P, E):
            assert results[name][f][:2] == results["flat"][f][:2] and np.array_equal(results[name][f][2], results["flat"][f][2]), (name, f)


def test_selftest_light_function():
    rng = np.random.default_rng(11)
    n = 512
    ctx = Context()
    try:
        ctx.set_lights(THREE_LIGHTS)
        rows = np.zeros((n, 7), np.float32)
        rows[:, 1:4] = rng.uniform(-2.0, 2.0, (n, 3)) * [1.0, 0.5, 1.0] - [0.0, 1.0, 0.0]
        nrm = rng.normal(size=(n, 3))
        rows[:, 4:7] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
        words = rows.view(np.uint32).copy()
        words[:, 0] = rng.integers(0, 3, n)
        out = np.zeros((n, 8), np.uint32)
        ctx.check(ctx.lib.rt3_selftest_eval(ctx.h, L.SELFTEST_LIGHT, words.ctypes.data, n, out.ctypes.data))
        bad = words[:1].copy()
        bad[0, 0] = 3
        spare = np.zeros((1, 8), np.uint32)
        assert ctx.lib.rt3_selftest_eval(ctx.h, L.SELFTEST_LIGHT, bad.ctypes.data, 1, spare.ctypes.data) == L.E_INVALID
    finally:
        ctx.close()
    got = out.view(np.float32).astype(np.float64)
    x, nr = rows[:, 1:4].astype(np.float64), rows[:, 4:7].astype(np.float64)
    for k, light in enumerate(THREE_LIGHTS):
        s = words[:, 0] == k
        wl, dist, Ic, _ = RL.light_sample(light, x[s])
        # wl: P - x (1 rounding of values up to 4), d^2, sqrt, 1 / d, the product: 8 eps relative to |P - x| / d <= 1, plus the
        # cancellation in P - x: eps |P| / d
        d = np.where(np.isinf(dist), 1.0, dist)
        tol_wl = 8 * EPS + 4 * EPS * 4.0 / d
        assert np.all(np.abs(got[s, :3] - wl) <= tol_wl[:, None])
        end = np.where(np.isinf(dist), L.BACKGROUND_DEPTH, dist * (1.0 - 2.0**-10))
        assert np.all(np.abs(got[s, 3] - end) <= 8 * EPS * end + 4 * EPS * 4.0)
        assert np.all(np.abs(got[s, 4] - np.sum(nr[s] * wl, -1)) <= 3 * tol_wl + 4 * EPS)
        c, w = RL.cone_window_raw(light, x[s])
        a = 1.0 / max(0.001, math.cos(float(light["inner_cone"])) - math.cos(float(light["outer_cone"]))) if k == 1 else 0.0
        dc = 16 * EPS * a + a * 3 * tol_wl  # the rounding of c (test_closed_form's bound) and of the wl it is made of
        hi, lo = np.clip(c + dc, 0, 1) ** 2 * np.clip(w, 0, 1), np.clip(c - dc, 0, 1) ** 2 * np.clip(w, 0, 1)
        I = light["intensity"].astype(np.float64)
        assert np.all(got[s, 5:8] <= I * hi[:, None] * (1 + 4 * EPS)) and np.all(got[s, 5:8] >= I * lo[:, None] * (1 - 4 * EPS))


# ---------------------------------------------------------------------------------------------------------------- 5 selection
def test_selection_between_two_lights_is_unbiased():
    """two point lights, 1 : 15 in power, the weak one low over the floor so that it owns part of the frame.  A sample is C_k / p_k with
    probability p_k, so it lies in [0, C / min p] (C = C_1 + C_2, the closed form) and its standard deviation is at most C / (2 min p):
    the frame mean lies within 5 sqrt(sum C_i^2) / (2 min p sqrt(S)) of sum C_i.  Derived, not measured."""
    S = 256
    mesh = PW.floor_world()
    ls = PW.lights(make_light(LIGHT_POINT, (0.5, 0.5, 0.5), position=(-0.5, 0.25, 0.2)), make_light(LIGHT_POINT, (7.5, 7.5, 7.5), position=(0.6, 1.6, -0.4)))
    pt = lit_pt(mesh, ls)
    try:
        got = frame(pt, camera(PW.FLOOR_CAMERA, WINDOW), P, S, 2).astype(np.float64)
        gb = pt.gbuffer()[0].copy()
        _, n_p, mass = pt.ctx.light_masses(P)
    finally:
        pt.close()
    want = RL.cdf_masses(RL.powers(ls, 1.0))
    assert n_p == 2 and np.all(np.abs(mass.astype(np.int64) - want) <= 3)
    p_min = want.min() / CDF_TOTAL
    scene = RP.Scene(mesh)
    rays = device_rays(PW.FLOOR_CAMERA, WINDOW)
    ref = RL.direct_light(scene, ls, PW.FLOOR_CAMERA, WINDOW, True, rays, gb)[0]
    each = [RL.direct_light(scene, ls[k:k + 1], PW.FLOOR_CAMERA, WINDOW, True, rays, gb)[0] for k in range(2)]
    assert (each[0] > each[1]).mean() > 0.02, "the weak light dominates part of the frame"
    band = 5.0 * np.sqrt((ref**2).sum((0, 1))) / (2.0 * p_min * math.sqrt(S)) / ref.sum((0, 1))
    ratio = got.sum((0, 1)) / ref.sum((0, 1))
    print(f"two lights: frame / closed form {ratio}, band +-{band}; min p_sel {p_min:.4f}")
    assert np.all(np.abs(ratio - 1.0) <= band + 64 * EPS)
    assert np.all(each[0].sum((0, 1)) / ref.sum((0, 1)) > 2.0 * band), "the band can see the weak light's share going wrong"


# ---------------------------------------------------------------------------------------------------------------- 6 union with emitters
CORNELL_LAMP = PW.lights(make_light(LIGHT_POINT, (7.5, 7.0, 6.0), position=(0.1, 1.0, 0.2)))  # about two thirds of the frame's light


def test_union_with_emitters_has_the_same_expectation():
    window = (64, 48)
    K, S = 16, 256

    def frames(flags, lights):
        pt = lit_pt(scenes.cornell(), lights, window)
        try:
            cam = camera(scenes.CORNELL_CAMERA, window)
            return np.stack([frame(pt, cam, flags, S, 4, index=k) for k in range(K)]).astype(np.float64)
        finally:
            pt.close()

    both, punct = frames(SPEC_FF | E | P, CORNELL_LAMP), frames(SPEC_FF | P, CORNELL_LAMP)
    z = block_z(both, punct)
    brighter = CORNELL_LAMP.copy()
    brighter["intensity"] *= np.float32(1.05)
    z_off = block_z(frames(SPEC_FF | E | P, brighter), punct)
    print(f"union: max |z| {np.abs(z).max():.2f} over {z.size} block-channels; with the lamp 5 % brighter on one side max |z| {np.abs(z_off).max():.2f}")
    assert np.abs(z).max() < 4.5
    assert np.abs(z_off).max() > 4.5, "the statistic must be able to see a 5 % brighter lamp"


# ---------------------------------------------------------------------------------------------------------------- 7 whole integrator
def room_frames(name, extra=0, mode=0):
    flags, bounces, _, _, _, _, n_frames = PW.CASES[name]
    mesh, sky = PW.room(name)
    pt = lit_pt(mesh, mesh.lights, IW.WINDOW_ROOM, sky=sky, mode=mode)
    try:
        cam = camera(IW.ROOM_CAMERA, IW.WINDOW_ROOM)
        out = np.stack([frame(pt, cam, flags | P | extra, IW.FRAME_SPP, bounces, index=k) for k in range(n_frames)])
        return out, pt.gbuffer()[1] != L.BACKGROUND_DEPTH
    finally:
        pt.close()


@pytest.mark.parametrize("extra", (0, E), ids=("punctual", "with_emitters"))
@pytest.mark.parametrize("name", sorted(PW.CASES))
def test_gpu_against_fixture(name, extra):
    frames, cov = room_frames(name, extra)
    check_against_fixture(frames, cov, fixture(), name)


def test_gpu_against_fixture_two_level():
    frames, cov = room_frames("spot_sun_b4", mode=1)
    check_against_fixture(frames, cov, fixture(), "spot_sun_b4")


# ---------------------------------------------------------------------------------------------------------------- 8 plumbing
def test_instance_modes_give_the_same_frame():
    a = gpu_frame(scenes.cornell(), THREE_LIGHTS, scenes.CORNELL_CAMERA, FULL | E | P, 4, 4, mode=0)
    b = gpu_frame(scenes.cornell(), THREE_LIGHTS, scenes.CORNELL_CAMERA, FULL | E | P, 4, 4, mode=1)
    assert a.mean() > 0 and np.array_equal(bits(a), bits(b))


def test_tile_partition_stitches_to_one_rank():
    window = (128, 48)  # two 64 x 64 tiles: the smallest window in which both of two ranks own pixels
    whole = gpu_frame(scenes.cornell(), THREE_LIGHTS, scenes.CORNELL_CAMERA, FULL | E | P, 4, 4, window)
    for r in range(2):
        part = gpu_frame(scenes.cornell(), THREE_LIGHTS, scenes.CORNELL_CAMERA, FULL | E | P, 4, 4, window, rank=r, n_ranks=2)
        m = owned_mask(window[0], window[1], r, 2)
        assert m.any() and np.array_equal(bits(part[m]), bits(whole[m]))


def test_batches_give_the_same_bits():
    pt = lit_pt(scenes.cornell(), THREE_LIGHTS)
    try:
        cam = camera(scenes.CORNELL_CAMERA, WINDOW)
        auto = frame(pt, cam, FULL | E | P, 6, 4)
        pt.ctx.set_option(L.OPT_BATCH_SPP, 1)
        one = frame(pt, cam, FULL | E | P, 6, 4)
    finally:
        pt.close()
    assert np.array_equal(bits(auto), bits(one))


def test_shadow_rays_are_counted_and_lights_need_no_rebuild():
    pt = make_pt(PW.floor_world(), WINDOW)
    try:
        cam = camera(PW.FLOOR_CAMERA, WINDOW)
        dark = frame(pt, cam, P, 2, 2)
        pt.ctx.stats_reset()
        frame(pt, cam, P, 2, 2)
        none = pt.ctx.stats().shadow_rays
        pt.ctx.set_lights(PW.lights(PW.FLOOR_LIGHTS["directional"]))  # after the build: no rebuild, the next frame has it
        pt.ctx.stats_reset()
        lit = frame(pt, cam, P, 2, 2)
        some = pt.ctx.stats().shadow_rays
    finally:
        pt.close()
    assert not dark.any() and lit.min() > 0.01
    assert none == 0 and some == 2 * WINDOW[0] * WINDOW[1], "one light shadow ray per sample at vertex 0 of B = 2: the sun reaches every pixel"


def test_refusals_leave_the_previous_lights():
    good = PW.lights(PW.FLOOR_LIGHTS["spot"])
    nan, inf = float("nan"), float("inf")

    def broken(**kw):
        l = PW.FLOOR_LIGHTS["spot"].copy()
        for k, v in kw.items():
            l[k] = v
        return PW.lights(l)

    bad = [broken(type=3), broken(range=nan), broken(position=(0.0, inf, 0.0)), broken(intensity=(1.0, -0.5, 1.0)), broken(intensity=(nan, 0.0, 0.0)),
           broken(direction=(0.0, 0.0, 0.0)), broken(type=LIGHT_DIRECTIONAL, direction=(0.0, 0.0, 0.0)), broken(inner_cone=0.5, outer_cone=0.5),
           broken(inner_cone=-0.1), broken(outer_cone=1.6), broken(inner_cone=0.6, outer_cone=0.4), broken(direction=(nan, 1.0, 0.0))]
    pt = lit_pt(PW.floor_world(), good)
    try:
        cam = camera(PW.FLOOR_CAMERA, WINDOW)
        before = frame(pt, cam, P, 1, 2)
        for b in bad:
            two = np.concatenate([good, b])  # a bad light anywhere in the list refuses the whole call
            assert pt.ctx.lib.rt3_scene_set_lights(pt.ctx.h, two.ctypes.data, 2) == L.E_INVALID
        assert pt.ctx.lib.rt3_scene_set_lights(pt.ctx.h, None, 1) == L.E_INVALID
        assert pt.ctx.light_masses(P)[:2] == (0, 1)
        after = frame(pt, cam, P, 1, 2)
        # a point light ignores direction and cone words altogether
        pt.ctx.set_lights(broken(type=LIGHT_POINT, direction=(0.0, 0.0, 0.0), inner_cone=0.9, outer_cone=0.1))
    finally:
        pt.close()
    assert before.max() > 0.1 and np.array_equal(bits(before), bits(after))


def test_light_masses_state_errors():
    ctx = Context()
    try:
        ctx.upload_mesh(scenes.cornell())
        ctx.set_lights(THREE_LIGHTS)
        with pytest.raises(L.Rt3Error) as e:
            ctx.light_masses(P)
        assert e.value.code == L.E_STATE
        ctx.build_accel()
        assert ctx.light_masses(P)[:2] == (0, 3)
        ctx.upload_mesh(scenes.cornell())  # rt3_scene_set_geometry does not reset the lights
        ctx.build_accel()
        assert ctx.light_masses(P)[:2] == (0, 3)
    finally:
        ctx.close()
