"""Per-sample camera rays on the GPU (rt3_camera_set_lens): the camera function against tests/ref_lens.py, closed
forms for antialiasing, escaped samples and the thin lens, the furnace and the float64 fixture through the new first vertex, invariance
under the batch size, the instance mode and the tile partition, "lens off is the code as it was", and the contract of the new calls.

Bounds are derived: a pixel of the flat emitters of lens_worlds is a binomial mean (5 sigma, exact where the coverage is 0 or 1); fp32
results carry one unit of 2^-24 per rounding of the longest chain."""
import numpy as np
import pytest

import integrator_worlds as IW
import lens_worlds as LW
import ref_lens as RL
from raytracer3_amd import _lib as L
from support import bits, camera
from test_integrator_cpu import FURNACE_BS, LOW_CAP, check_against_fixture, furnace_tolerance
from test_lens_cpu import band, fixture
from test_nee_emissive import make_pt, owned_mask

pytestmark = pytest.mark.gpu

U = 2.0**-24
FF = L.F_FACEFORWARD
CAM = camera(LW.CAMERA, LW.WINDOW)


def as_f32(words):
    return np.ascontiguousarray(words).view(np.float32)


def lens_frame(pt, cam, flags, spp, bounces, index=0, blend=1.0, postprocess=False):
    """(Light rgb of every pixel, the frame's GConst)"""
    g = pt.make_gconst(cam, spp, bounces, frame=index, blendfactor=blend, flags=flags)
    pt.render(g, postprocess=postprocess)
    return pt.light()[..., :3].copy(), g


def op31(ctx, g, window, lens, px, py, sm, frame=0):
    """lens_ray on the device: (o, d, film point in pixels, lens point in view space), float32"""
    n = len(px)
    rows = np.zeros((n, 41), np.uint32)
    rows[:, 0:16] = bits(np.array(g.proj_inverse[:], np.float32))
    rows[:, 16:32] = bits(np.array(g.view_inverse[:], np.float32))
    rows[:, 32:34] = bits(np.array(window, np.float32))
    rows[:, 34:37] = bits(np.array(lens, np.float32))
    rows[:, 37], rows[:, 38], rows[:, 39], rows[:, 40] = px, py, frame, sm
    out = as_f32(ctx.selftest(L.SELFTEST_LENS, rows, 10))
    return out[:, 0:3], out[:, 3:6], out[:, 6:8], out[:, 8:10]


def camera_uniforms(ctx, px, py, sm, frame=0):
    """the four numbers of the RNG index rule, from the device's own rng_seed and uniform_float (ops 11 and 3, pinned by test_oracle_kat)"""
    seed = ctx.selftest(11, np.stack([px, py, np.full_like(px, frame)], -1).astype(np.uint32), 1)[:, 0]
    idx = (np.uint64(0x80000000) + 4 * sm.astype(np.uint64)).astype(np.uint32)
    return np.stack([as_f32(ctx.selftest(3, np.stack([seed, idx + np.uint32(k)], -1).astype(np.uint32), 1))[:, 0] for k in range(4)], -1)


@pytest.fixture(scope="module")
def rect_pt():
    """the emissive rectangle of lens_worlds before a constant sky, at 32 x 24"""
    mesh, world = LW.quad(LW.rect_corners(), LW.RECT_DEPTH)
    pt = make_pt(mesh, LW.WINDOW, sky=LW.constant_sky())
    yield pt, world
    pt.close()


def scene_pt(corners_or_mesh, sky=None, window=LW.WINDOW, **kw):
    mesh, world = corners_or_mesh
    return make_pt(mesh, window, sky=sky, **kw), world


# ---------------------------------------------------------------------------------------------------------------- 1 camera function
N_OPS_D, N_OPS_O = 64, 24  # roundings on the way to d (film 3, /W 1, ndc 2, proj_inverse 4, normalise 8, disk 16, focus 4, normalise 8, rotate 5:
#                            51, rounded up) and to o (disk 16, rotate and translate 5), each at most one unit of 2^-24 of the result's scale


def primary_ray_f32(g, window, px, py):
    """primary_ray (rt3_camera.hpp) restated in numpy's fp32: the same operations in the same order, IEEE divide and square root, no
    contraction"""
    f = np.float32
    m, w = np.array(g.proj_inverse[:], f), np.array(g.view_inverse[:], f)
    cx, cy = (px.astype(f) + f(0.5)) / f(window[0]), (py.astype(f) + f(0.5)) / f(window[1])
    dx, dy = cx * f(2.0) - f(1.0), -(cy * f(2.0) - f(1.0))
    one, zero = f(1.0), f(0.0)
    tx, ty, tz = (m[k] * dx + m[4 + k] * dy + m[8 + k] * one + m[12 + k] * one for k in range(3))
    inv = one / np.sqrt(tx * tx + ty * ty + tz * tz)
    tx, ty, tz = tx * inv, ty * inv, tz * inv
    return np.stack([w[k] * tx + w[4 + k] * ty + w[8 + k] * tz + w[12 + k] * zero for k in range(3)], -1)


def test_degenerate_lens_is_the_primary_ray(rect_pt):
    """R = 0, jitter = 0: the ray op 31 returns is the one the "gbuffer" pass traced -- the same depth word in every pixel, the eye as origin"""
    pt, _ = rect_pt
    W, H = LW.WINDOW
    g = pt.make_gconst(CAM, 1, 1)
    pt.render(g)
    depth = pt.gbuffer()[1]
    py, px = (a.reshape(-1) for a in np.mgrid[0:H, 0:W])
    o, d, film, lens = op31(pt.ctx, g, LW.WINDOW, (0.0, 1.0, 0.0), px, py, np.arange(W * H) % 7)
    rays = np.concatenate([o.T, d.T, np.zeros((1, W * H), np.float32), np.full((1, W * H), L.BACKGROUND_DEPTH, np.float32)])
    t, _, _, prim, _ = pt.ctx.trace_rays(rays)
    t = np.where(prim == L.MISS, np.float32(L.BACKGROUND_DEPTH), t)
    assert np.array_equal(bits(t.reshape(H, W)), bits(depth))
    assert (depth != L.BACKGROUND_DEPTH).any() and (depth == L.BACKGROUND_DEPTH).any()
    assert np.array_equal(bits(o), np.tile(bits(np.array(g.view_inverse[12:15], np.float32)), (W * H, 1)))
    assert np.array_equal(film, np.stack([px + 0.5, py + 0.5], -1).astype(np.float32)) and not lens.any()
    # and the direction itself, word for word, against the host restatement
    want = primary_ray_f32(g, LW.WINDOW, px, py)
    assert want.dtype == np.float32 and np.array_equal(bits(d), bits(want))


@pytest.mark.parametrize("lens", ((0.0, 1.0, 1.0), (0.3, 4.0, 1.0), (0.3, 4.0, 0.0), (0.05, 0.7, 0.5)))
def test_camera_function_against_float64(rect_pt, lens):
    pt, _ = rect_pt
    W, H = LW.WINDOW
    g = pt.make_gconst(CAM, 1, 1)
    rng = np.random.default_rng(5)
    n = 4096
    px, py, sm = rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 1 << 20, n)
    frame = 3
    u = camera_uniforms(pt.ctx, px, py, sm, frame)
    o, d, film, lp = (a.astype(np.float64) for a in op31(pt.ctx, g, LW.WINDOW, lens, px, py, sm, frame))
    pinv, vinv = RL.gconst_matrices(g)
    ro, rd, rfilm, rlp = RL.camera_sample(pinv, vinv, LW.WINDOW, lens, px, py, u)
    Rl, F, j = lens
    scale_o = np.abs(vinv[:3, 3]).max() + Rl
    err_d, err_o = np.abs(d - rd).max() / U, np.abs(o - ro).max() / (U * scale_o)
    print(f"lens {lens}: worst |d - ref| {err_d:.2f} units of 2^-24 (bound {N_OPS_D}), |o - ref| {err_o:.2f} units of its scale (bound {N_OPS_O})")
    assert err_d <= N_OPS_D and err_o <= N_OPS_O
    assert np.abs(film - rfilm).max() <= 3 * U * 64.0 and np.abs(lp - rlp).max() <= 16 * U * max(Rl, 1e-30)
    # film points lie in the pixel's jitter box (half an ulp of a coordinate below 64 for the sum's rounding)
    assert np.all(np.abs(film - np.stack([px + 0.5, py + 0.5], -1)) <= 0.5 * j + 2.0**-19)
    # lens points lie in the disk of radius R, in the plane of view_inverse's columns 0 and 1
    assert np.all(np.hypot(lp[:, 0], lp[:, 1]) <= Rl * (1.0 + 4 * U))
    off = o - vinv[:3, 3]
    assert np.abs(off - (lp[:, :1] * vinv[:3, 0] + lp[:, 1:] * vinv[:3, 1])).max() <= N_OPS_O * U * scale_o
    assert np.abs(off @ vinv[:3, 2]).max() <= N_OPS_O * U * scale_o
    if j == 0.0 and Rl > 0.0:  # all rays of a pixel pass the one focus point: the error of d over the distance, plus the origin's
        P = RL.focus_point(pinv, vinv, LW.WINDOW, F, px, py)
        w = P - o
        dist = np.linalg.norm(w - np.sum(w * d, -1, keepdims=True) * d, axis=-1)
        assert np.all(dist <= (N_OPS_D * np.linalg.norm(w, axis=-1) + N_OPS_O * scale_o) * U)
    if j > 0.0:  # u0 - 1/2 has mean 0 and a standard deviation of at most 1/2
        assert abs(np.mean((film[:, 0] - px - 0.5) / j)) <= 5.0 * 0.5 / np.sqrt(n)
    if Rl > 0.0:  # |l|^2 / R^2 is uniform: mean 1/2, standard deviation sqrt(1/12)
        assert abs(np.mean(np.sum(lp * lp, -1) / Rl**2) - 0.5) <= 5.0 * np.sqrt(1.0 / 12.0 / n)


# ---------------------------------------------------------------------------------------------------------------- 2 per-sample pinhole
def room_world():
    return IW.open_room(), None, IW.ROOM_CAMERA


def material_room_world():
    import material_worlds as MW

    # an emissive map on the box the camera looks at, a normal map and a metallic-roughness map on the floor: k_shade's MAT instance at vertex 0
    mesh, cam = MW.room()
    names = mesh.names
    rng = np.random.default_rng(41)
    textures = MW.colour_textures(rng, [(8, 8), (5, 3)]) + MW.normal_textures(rng, [(16, 16)])
    t = MW.table(len(names), emissive_texture={names.index("box1"): 0, names.index("panel"): 1}, normal_texture={names.index("floor"): 2},
                 metallic_roughness_texture={names.index("floor"): 1})
    return MW.with_tables(mesh, material_textures=t, textures=textures), None, cam


@pytest.mark.parametrize("world", (room_world, material_room_world), ids=("open_room", "material_textures"))
def test_per_sample_pinhole_is_exact(world):
    """lens {0, 1, 0}, flags 0, B = 1: every sample is the emission hit_info (op 29) reports for the pixel centre's hit -- unquantised, and
    with material textures where the scene has them -- or 0 where the camera ray escapes; S = 16 adds one rounding per sum and the division"""
    mesh, inst, cam_d = world()
    W, H = window = (64, 48)
    pt = make_pt(mesh, window, instances=inst)
    try:
        cam = camera(cam_d, window)
        pt.set_lens(0.0, 1.0, 0.0)
        one, g = lens_frame(pt, cam, 0, 1, 1)
        many, _ = lens_frame(pt, cam, 0, 16, 1)
        depth = pt.gbuffer()[1]
        py, px = (a.reshape(-1) for a in np.mgrid[0:H, 0:W])
        o, d, _, _ = op31(pt.ctx, g, window, (0.0, 1.0, 0.0), px, py, np.zeros(W * H, np.int64))
        rays = np.concatenate([o.T, d.T, np.full((1, W * H), 1e-3, np.float32), np.full((1, W * H), L.BACKGROUND_DEPTH, np.float32)])
        t, bu, bv, prim, _ = pt.ctx.trace_rays(rays)
        hit = prim != L.MISS
        assert np.array_equal(hit.reshape(H, W), depth != L.BACKGROUND_DEPTH) and hit.any()
        want = np.zeros((W * H, 3), np.float32)
        rows = np.stack([prim[hit], bits(bu[hit]), bits(bv[hit])], -1).astype(np.uint32)
        want[hit] = as_f32(pt.ctx.selftest(L.SELFTEST_HIT_INFO, rows, 11))[:, 3:6]
    finally:
        pt.close()
    want = want.reshape(H, W, 3)
    assert want.max() > 0.0
    assert np.array_equal(bits(one), bits(want))
    assert np.all(np.abs(many.astype(np.float64) - want) <= 17 * U * want)


# ---------------------------------------------------------------------------------------------------------------- 3, 4 antialiasing
def gpu_coverage(g, world, jitter):
    pinv, vinv = RL.gconst_matrices(g)
    return RL.polygon_coverage(LW.project(pinv, vinv, world), LW.WINDOW, jitter)


def check_binomial(light, a, lit, dark, S, label, rounding=0.0):
    """every sample is `lit` (share a) or `dark`: |mean - expectation| within 5 sigma per pixel and channel, exact where a is 0 or 1 (but for
    `rounding`, relative)"""
    a = a[..., None]
    want = a * lit + (1.0 - a) * dark
    dev = np.abs(light.astype(np.float64) - want)
    tol = band(a, S) * np.abs(lit - dark) + rounding * want
    part = (a[..., 0] > 0.0) & (a[..., 0] < 1.0)
    z = dev[part] / np.maximum(tol[part] / 5.0, 1e-300)
    print(f"{label}: {int(part.sum())} partly covered pixels, worst {z.max():.2f} sigma; fully covered / uncovered pixels off by at most {dev[~part].max():.3e}")
    assert np.all(dev <= tol + 1e-12 * np.abs(want))
    assert part.sum() >= 20


@pytest.mark.parametrize("rot,jitter", ((0.0, 1.0), (25.0, 1.0), (0.0, 0.5)), ids=("aligned", "rotated", "half_box"))
def test_antialiasing_closed_form(rot, jitter):
    """B = 1, flags 0, no sky, S = 1024: a pixel is Le x the share of its jitter box inside the rectangle's image -- pixels whose centre
    sees the background included"""
    S = 1024
    pt, world = scene_pt(LW.quad(LW.rect_corners(rot_deg=rot), LW.RECT_DEPTH))
    try:
        pt.set_lens(0.0, 1.0, jitter)
        light, g = lens_frame(pt, CAM, 0, S, 1)
        centre_bg = pt.gbuffer()[1] == L.BACKGROUND_DEPTH
    finally:
        pt.close()
    a = gpu_coverage(g, world, jitter)
    if jitter == 1.0:  # (the half-width boxes of this rectangle's partly covered pixels all hold their pixel's centre)
        assert (centre_bg & (a > 0.05)).any(), "some partly covered pixel has a background centre"
    check_binomial(light, a, LW.LE, np.zeros(3), S, f"antialiasing rot={rot} jitter={jitter}")
    assert np.array_equal(light[a == 0.0], np.zeros_like(light[a == 0.0])) and np.all(light[a == 1.0] == LW.LE.astype(np.float32))


@pytest.mark.parametrize("flags", (0, L.F_NEE_SKY), ids=("lens_miss", "shade_miss"))
def test_escaped_samples_are_counted_once(rect_pt, flags):
    """a constant sky c behind the rectangle (albedo 0, so that under NEE the hit samples gather nothing): a Le + (1 - a) c by either route.
    The bilinear lookup of a constant rounds (1 - f) and the two sums: 4 units; the S sums and the division: S + 1."""
    S = 1024
    pt, world = rect_pt
    try:
        pt.set_lens(0.0, 1.0, 1.0)
        light, g = lens_frame(pt, CAM, flags, S, 1, index=flags)
    finally:
        pt.set_lens(None)
    a = gpu_coverage(g, world, 1.0)
    check_binomial(light, a, LW.LE, np.asarray(LW.SKY_C, np.float64), S, f"escaped samples flags={flags}", rounding=(S + 5) * U)


# ---------------------------------------------------------------------------------------------------------------- 5 thin lens
@pytest.mark.parametrize("name,z", LW.HALF_PLANE_DEPTHS)
def test_thin_lens_closed_form(name, z):
    """an emissive half-plane x >= e at view depth z: the column means follow the edge response of a uniform disk of the circle of
    confusion's radius, integrated over the pixel (ref_lens.disk_edge_G); the frame's sum is the pinhole's"""
    W, H = LW.WINDOW
    S = 256
    pt, world = scene_pt(LW.half_plane(z))
    try:
        pt.set_lens(LW.LENS_R, LW.LENS_F, 1.0)
        light, g = lens_frame(pt, CAM, 0, S, 1)
    finally:
        pt.close()
    pinv, vinv = RL.gconst_matrices(g)
    e = LW.project(pinv, vinv, world)[0, 0]
    r = RL.coc_radius_px(LW.LENS_R, LW.LENS_F, z, LW.CAMERA["fov_deg"], H)
    a = RL.half_plane_columns(e, r, W)
    col = light.astype(np.float64).mean(0) / LW.LE  # (W, 3): every channel counts the same hits
    assert np.array_equal(col[:, 0], col[:, 1]) and np.array_equal(col[:, 0], col[:, 2])
    got = col[:, 0]
    part = (a > 0.0) & (a < 1.0)
    sig = np.sqrt(a * (1.0 - a) / (S * H))
    print(f"half-plane {name}: circle of confusion {r:.3f} px, edge at {e:.4f}, {int(part.sum())} columns in transition, worst "
          f"{np.abs((got - a)[part] / sig[part]).max():.2f} sigma")
    assert np.all(np.abs(got - a) <= 5.0 * sig + 1e-12)
    assert abs(got.sum() - (W - e)) <= 5.0 * np.sqrt(np.sum(sig**2)) + 1e-9
    assert part.sum() == 1 if r == 0.0 else part.sum() >= 4


# ---------------------------------------------------------------------------------------------------------------- 6 furnace
@pytest.mark.parametrize("flags", (0, FF))
def test_furnace_through_the_lens(flags):
    """every vertex of a lens path has the fp32 material: L = E sum_{k < B} rho^k in every pixel, no G-buffer quantisation"""
    mesh, _, cam_d = IW.furnace(10.0)
    pt = make_pt(mesh, IW.WINDOW_FURNACE)
    rho = np.asarray(IW.FURNACE_ALBEDO, np.float32).astype(np.float64)
    E = 12.0 * np.asarray(IW.FURNACE_EMISSION, np.float32).astype(np.float64)
    try:
        cam = camera(cam_d, IW.WINDOW_FURNACE)
        pt.set_lens(0.2, 5.0, 1.0)  # the eye is 1 from the nearest wall: the disk is well inside the room
        for bounces, samples in FURNACE_BS:
            light, _ = lens_frame(pt, cam, flags, samples, bounces)
            want = E * sum((rho**k for k in range(bounces)), np.zeros(3))
            rel = light.astype(np.float64) / want - 1.0
            tol = furnace_tolerance(bounces, samples)
            high, low = (rel > tol).any(-1), (rel < -tol).any(-1)
            print(f"lens furnace flags={flags} B={bounces} S={samples}: {int(low.sum())} of {low.size} pixels low, {int(high.sum())} high, "
                  f"others within {np.abs(rel[~high & ~low]).max():.2e} (bound {tol:.2e})")
            assert not high.any()
            assert low.mean() <= LOW_CAP
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 7 float64 fixture
@pytest.mark.parametrize("extra", (0, L.F_NEE_EMISSIVE), ids=("plain", "nee_emissive"))
@pytest.mark.parametrize("name", sorted(LW.ROOM_CASES))
def test_lens_frames_against_fixture(name, extra):
    """the open room through the thin lens against tests/ref_lens.py's float64 tracer, by test_integrator_cpu's statistics over every
    pixel; with RT3_F_NEE_EMISSIVE the panel the camera sees directly takes the FLT_MAX weight"""
    flags, bounces, specular, _, _, n_frames = LW.ROOM_CASES[name]
    pt = make_pt(IW.open_room(specular), IW.WINDOW_ROOM, sky=IW.room_sky())
    try:
        cam = camera(IW.ROOM_CAMERA, IW.WINDOW_ROOM)
        pt.set_lens(*LW.ROOM_LENS)
        frames = np.stack([lens_frame(pt, cam, flags | extra, IW.FRAME_SPP, bounces, index=k)[0] for k in range(n_frames)])
    finally:
        pt.close()
    W, H = IW.WINDOW_ROOM
    check_against_fixture(frames, np.ones((H, W), bool), fixture(), name)


@pytest.mark.parametrize("name", sorted(LW.MATERIAL_CASES))
def test_textured_first_vertex_against_fixture(name):
    """lens_worlds.material_room(): normal maps and metallic-roughness maps on everything the camera sees, B = 2, so a pixel's expectation
    is the vertex-0 BSDF -- tangent frame, perturbed normal, textured roughness and metalness -- integrated against the emitters:
    k_shade<false, .., MAT> at bounce 0 against the float64 surfaces of tests/ref_materials.py"""
    flags, bounces, _, _, _, n_frames = LW.MATERIAL_CASES[name]
    mesh, cam_d = LW.material_room()
    pt = make_pt(mesh, IW.WINDOW_ROOM, sky=LW.constant_sky(LW.MATERIAL_SKY_C))
    try:
        cam = camera(cam_d, IW.WINDOW_ROOM)
        pt.set_lens(*LW.MATERIAL_LENS)
        frames = np.stack([lens_frame(pt, cam, flags, IW.FRAME_SPP, bounces, index=k)[0] for k in range(n_frames)])
        assert (pt.gbuffer()[1] != L.BACKGROUND_DEPTH).all(), "no camera ray escapes"
    finally:
        pt.close()
    W, H = IW.WINDOW_ROOM
    check_against_fixture(frames, np.ones((H, W), bool), fixture(), name)


# ---------------------------------------------------------------------------------------------------------------- 8 invariance
FULL = L.F_NEE_SKY | L.F_FACEFORWARD | L.F_SPECULAR


def room_lens_frame(window=IW.WINDOW_ROOM, flags=FULL, spp=8, bounces=3, blend=1.0, setup=None, **kw):
    pt = make_pt(IW.open_room(True), window, sky=IW.room_sky(), **kw)
    try:
        pt.set_lens(*LW.ROOM_LENS)
        if setup:
            setup(pt)
        return lens_frame(pt, camera(IW.ROOM_CAMERA, window), flags, spp, bounces, index=2, blend=blend)[0]
    finally:
        pt.close()


def test_same_bits_for_every_batch_size_and_instance_mode():
    whole = room_lens_frame()
    assert whole.max() > 0.0
    by_sample = room_lens_frame(setup=lambda pt: pt.ctx.set_option(L.OPT_BATCH_SPP, 1))
    assert np.array_equal(bits(whole), bits(by_sample))
    two_level = room_lens_frame(mode=1)
    assert np.array_equal(bits(whole), bits(two_level))
    with_emitters = room_lens_frame(flags=FULL | L.F_NEE_EMISSIVE)
    by_sample_e = room_lens_frame(flags=FULL | L.F_NEE_EMISSIVE, setup=lambda pt: pt.ctx.set_option(L.OPT_BATCH_SPP, 3))
    assert np.array_equal(bits(with_emitters), bits(by_sample_e))


def test_tile_partition_renders_the_same_pixels():
    W, H = window = (128, 48)
    whole = room_lens_frame(window)
    for r in range(2):
        part = room_lens_frame(window, rank=r, n_ranks=2)
        m = owned_mask(W, H, r, 2)
        assert m.any() and not m.all()
        assert np.array_equal(bits(part[m]), bits(whole[m]))


def test_blend_with_prev_light_on_every_pixel(rect_pt):
    pt, world = rect_pt
    bf = np.float32(0.25)
    try:
        pt.set_lens(0.0, 1.0, 1.0)
        first, _ = lens_frame(pt, CAM, 0, 16, 1, index=0)
        pt.copy_light_to_prev()
        fresh, _ = lens_frame(pt, CAM, 0, 16, 1, index=1)
        blended, _ = lens_frame(pt, CAM, 0, 16, 1, index=1, blend=float(bf))
        centre_bg = pt.gbuffer()[1] == L.BACKGROUND_DEPTH
    finally:
        pt.set_lens(None)
    want = first + (fresh - first) * bf  # fp32, the kernel's expression
    assert np.array_equal(bits(blended), bits(want))
    assert (blended[centre_bg] != fresh[centre_bg]).any(), "background-centred pixels are blended too"


# ---------------------------------------------------------------------------------------------------------------- 9 lens off
def test_lens_off_is_the_frame_without_one():
    mesh, _ = LW.quad(LW.rect_corners(), LW.RECT_DEPTH, albedo=(0.6, 0.5, 0.4))
    out = []
    for touch in (False, True):
        pt = make_pt(mesh, LW.WINDOW, sky=LW.constant_sky())
        try:
            if touch:
                pt.set_lens(0.3, 2.0, 1.0)
                pt.set_lens(None)
                assert pt.ctx.get_lens()[1] is False
            g = pt.make_gconst(CAM, 8, 3, frame=4, flags=FULL)
            pt.rg.upload(pt.commands(g)["light"], np.full((LW.WINDOW[1], LW.WINDOW[0], 4), 0.125, np.float32))  # background pixels keep it
            pt.render(g, postprocess=True)
            out.append((pt.light(), pt.color()))
        finally:
            pt.close()
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1]))
    assert out[0][0][..., :3].max() > 0.125


def test_postprocess_shows_light_everywhere(rect_pt):
    """with a lens set, "postprocess" is AgX (op 8) of In in every pixel: a silhouette pixel with a background centre is not the pinhole sky"""
    pt, world = rect_pt
    try:
        pt.set_lens(0.0, 1.0, 1.0)
        light, g = lens_frame(pt, CAM, 0, 64, 1, postprocess=True)
        color = pt.color()
        centre_bg = pt.gbuffer()[1] == L.BACKGROUND_DEPTH
        H, W = centre_bg.shape
        want = as_f32(pt.ctx.selftest(8, bits(light.reshape(-1, 3)), 3)).reshape(H, W, 3)
    finally:
        pt.set_lens(None)
    a = gpu_coverage(g, world, 1.0)
    assert (centre_bg & (a > 0.05)).any()
    assert np.array_equal(bits(color[..., :3]), bits(want)) and np.all(color[..., 3] == 1.0)


# ---------------------------------------------------------------------------------------------------------------- 10 contract
BAD_PARAMS = [
    dict(aperture_radius=float("nan")), dict(aperture_radius=float("inf")), dict(aperture_radius=-0.1),
    dict(focus_distance=float("nan")), dict(focus_distance=float("inf")), dict(aperture_radius=0.1, focus_distance=0.0),
    dict(aperture_radius=0.1, focus_distance=-2.0), dict(pixel_jitter=float("nan")), dict(pixel_jitter=-0.01), dict(pixel_jitter=1.01),
    dict(reserved=1),
]


def lens_tuple(ctx):
    p, on = ctx.get_lens()
    return (p.aperture_radius, p.focus_distance, p.pixel_jitter, p.reserved, on)


def test_contract():
    pt, _ = scene_pt(LW.quad(LW.rect_corners(), LW.RECT_DEPTH))
    ctx = pt.ctx
    try:
        assert lens_tuple(ctx) == (0.0, 1.0, 1.0, 0, False), "off by default"
        ctx.set_lens(aperture_radius=0.25, focus_distance=3.0, pixel_jitter=0.5)
        kept = lens_tuple(ctx)
        assert kept == (0.25, 3.0, 0.5, 0, True)
        for bad in BAD_PARAMS:
            with pytest.raises(L.Rt3Error) as e:
                ctx.set_lens(L.LensParams(**bad))
            assert e.value.code == L.E_INVALID, bad
            assert lens_tuple(ctx) == kept, bad
        ctx.set_lens(aperture_radius=0.0, focus_distance=-1.0, pixel_jitter=0.0)  # the focus distance of a pinhole is not read
        assert lens_tuple(ctx) == (0.0, -1.0, 0.0, 0, True)
        # "adaptive" selects pixels by G-buffer depth
        with pytest.raises(L.Rt3Error) as e:
            pt.render(pt.make_gconst(CAM, 32, 2), adaptive=True)
        assert e.value.code == L.E_STATE and "lens" in str(e.value)
        # the vertices' RNG indices may not reach the camera's
        with pytest.raises(L.Rt3Error) as e:
            pt.render(pt.make_gconst(CAM, (1 << 26) + 1, 4))
        assert e.value.code == L.E_INVALID and "2^31" in str(e.value)
        # the extra extension rays are counted: the G-buffer's primary rays, then one camera ray per sample
        W, H = LW.WINDOW
        ctx.stats_reset()
        pt.render(pt.make_gconst(CAM, 3, 1))
        assert ctx.stats().extension_rays == W * H + 3 * W * H
        ctx.set_lens(None)
        assert lens_tuple(ctx) == (0.0, -1.0, 0.0, 0, False)
        pt.render(pt.make_gconst(CAM, 32, 2), adaptive=True)  # and works again without one
    finally:
        pt.close()
