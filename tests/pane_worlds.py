"""Worlds of the pane-shadow tests (tests/test_pane_shadows_cpu.py, tests/test_pane_shadows.py): the floor of
punctual_worlds seen by its camera, with horizontal glass quads ABOVE the camera -- the camera sees only floor, a punctual light shines
down through the glass, and with B = 2, no sky and no emission every sample of a pixel is the same number.  The closed form of a floor
pixel is the frame without the glass times the product of A = transmission (1 - F'(cos_i)) tint over the panes that the segment from the
floor point to the light crosses."""
import numpy as np

import punctual_worlds as PW
import ref_glass as RG
from raytracer3_amd import assets
from raytracer3_amd.assets import LIGHT_DIRECTIONAL, LIGHT_POINT, Material, MeshBuilder, make_light
from support import camera

WINDOW = (64, 48)
CAMERA = PW.FLOOR_CAMERA  # at y = 2.4, looking down: every pixel is floor
PINHOLE = (0.0, 1.0, 0.0)  # glass needs per-sample camera rays; this lens sends every sample through its pixel's centre
IOR = 1.5
TINT = (0.5, 0.25, 0.75)
TINT2 = (0.75, 0.5, 1.0)
ALBEDO = PW.FLOOR_ALBEDO
# the directional light makes 20 degrees with the floor's normal; the point light hangs 5 above the floor, 2 above the lower pane, whose
# projection then covers a quadrant of the view with incidence angles from 9 to 37 degrees
LIGHTS = {
    "directional": make_light(LIGHT_DIRECTIONAL, (2.0, 1.5, 1.0), direction=(0.3, -1.0, 0.2)),
    "point": make_light(LIGHT_POINT, (30.0, 24.0, 18.0), position=(0.4, 5.0, -0.3)),
}
# (x range, height, z range) of the glass quads: both above the camera (y = 2.4)
PANE = ((-1.5, 0.1), 3.0, (-1.6, -0.2))
PANE_UPPER = ((-1.3, 0.5), 3.5, (-1.9, -0.3))
EDGE_MARGIN = 1e-3  # metres on the floor: pixels whose floor point is nearer to a projected outline are left out


def glass(tint=(1.0, 1.0, 1.0), thin=True, tau=1.0, ior=IOR, **kw):
    return Material(tint, 0.0, 1.0, transmission=tau, ior=ior, thin_walled=1 if thin else 0, **kw)


def checker():
    """punctual_worlds' cutout texture: 2 x 2 texels, white, alpha 255 on the diagonal and 0 off it"""
    tex = np.full((2, 2, 4), 255, np.uint8)
    tex[0, 1, 3] = tex[1, 0, 3] = 0
    return tex


def flat_normal_map():
    """a 2 x 2 tangent-space normal map that says (0, 0, 1) everywhere"""
    return np.ascontiguousarray(np.tile(np.array([128, 128, 255, 255], np.uint8), (2, 2, 1)))


# case -> the glass quads [(rect, material, textures the quad needs)]; every world also has the floor
def case_quads(case):
    if case == "pane":
        return [(PANE, glass(TINT))]
    if case == "stacked":
        return [(PANE, glass(TINT)), (PANE_UPPER, glass(TINT2, tau=0.5))]
    if case == "cutout":
        return [(PANE, glass(TINT, texture_offset=0, alpha_cutoff=0.5))]
    if case == "solid":
        return [(PANE, glass(TINT, thin=False))]
    if case == "normal_mapped":
        return [(PANE, glass(TINT, normal_texture=0))]
    if case == "index_matched":
        return [(PANE, glass(ior=1.0))]
    if case == "none":
        return []
    raise KeyError(case)


def world(case, light="directional", n_extra=0):
    """the floor, the case's glass quads above the camera, the light: at most 6 triangles; and n_extra more geometries of one small triangle
    each UNDER the floor, where no ray of these frames goes: they only bring the geometry count past the 256 entries of k_shade's LDS table"""
    mb = MeshBuilder()
    PW._quad(mb, "floor", (-3.0, 3.0), 0.0, (-3.0, 3.0), Material(ALBEDO, 0.0, 1.0))
    for k, (rect, mat) in enumerate(case_quads(case)):
        PW._quad(mb, f"glass{k}", rect[0], rect[1], rect[2], mat, uv=True)
    for k in range(n_extra):
        x, z = -2.5 + 0.25 * (k % 20), -2.5 + 0.25 * (k // 20)
        mb.add(f"chip{k}", [[x, -0.5, z], [x + 0.1, -0.5, z], [x, -0.5, z - 0.1]], np.tile([0.0, 1.0, 0.0], (3, 1)), None, [[0, 1, 2]], Material((0.5, 0.5, 0.5), 0.0, 1.0))
    mesh = mb.build()
    if case == "cutout":
        mesh.textures = [checker()]
    if case == "normal_mapped":
        mesh.textures = [flat_normal_map()]
    mesh.lights = assets.lights_array([LIGHTS[light]])
    return mesh


# ---------------------------------------------------------------------------------------------------------------- float64 geometry
def floor_points(window=WINDOW):
    """(H W, 3) float64: where the pixel centres' rays (the kernels' primary_ray, from the frame's fp32 matrices) meet the floor y = 0"""
    W, H = window
    g = camera(CAMERA, window).gconst(window)
    pinv = np.array(g.proj_inverse[:], np.float64).reshape(4, 4).T
    vinv = np.array(g.view_inverse[:], np.float64).reshape(4, 4).T
    py, px = np.mgrid[0:H, 0:W]
    dx, dy = (px + 0.5) / W * 2 - 1, -((py + 0.5) / H * 2 - 1)
    t = np.stack([dx, dy, np.ones_like(dx), np.ones_like(dx)], -1) @ pinv.T
    t = t[..., :3] / np.linalg.norm(t[..., :3], axis=-1, keepdims=True)
    d = (t @ vinv[:3, :3].T).reshape(-1, 3)
    o = vinv[:3, 3]
    s = -o[1] / d[:, 1]
    assert np.all(s > 0.0)
    return o + s[:, None] * d


def to_light(light, x):
    """unit directions from the points x towards the light, float64 from its fp32 fields"""
    if int(light["type"]) == LIGHT_DIRECTIONAL:
        a = -np.asarray(light["direction"], np.float32).astype(np.float64)
        return np.broadcast_to(a / np.linalg.norm(a), x.shape).copy()
    w = np.asarray(light["position"], np.float32).astype(np.float64) - x
    return w / np.linalg.norm(w, axis=1, keepdims=True)


def crossing(rect, x, w):
    """where the rays x + s w (w.y > 0) cross the plane of the quad `rect`: (inside (m,) bool, distance to the quad's outline measured on the
    floor (m,), (u, v) of the quad's uv (m, 2))"""
    (x0, x1), h, (z0, z1) = rect
    s = h / w[:, 1]
    p = x + s[:, None] * w
    dx, dz = np.minimum(p[:, 0] - x0, x1 - p[:, 0]), np.minimum(p[:, 2] - z0, z1 - p[:, 2])
    inside = (dx > 0.0) & (dz > 0.0)
    outside = np.hypot(np.minimum(dx, 0.0), np.minimum(dz, 0.0))
    edge = np.where(inside, np.minimum(dx, dz), outside)
    # a step on the floor moves the crossing by at most as much (parallel projection: as much; central: less, the pane lies nearer the light)
    # PW._quad: origin (x0, z1), du along +x, dv along -z
    uv = np.stack([(p[:, 0] - x0) / (x1 - x0), (z1 - p[:, 2]) / (z1 - z0)], -1)
    return inside, edge, uv


def pass_fraction(cos_i, ior, thin_slab=True):
    """1 - F' of a pane (or, thin_slab = False, 1 - F of one interface: what a wrong implementation would use)"""
    F = RG.fresnel(cos_i, ior)
    return 1.0 - (RG.thin_fresnel(F) if thin_slab else F)


def closed_form(case, light_name, window=WINDOW, thin_slab=True):
    """Per pixel, row by row: (factor (H W, 3) that multiplies the frame without glass, use (H W,) bool: the pixel is further than EDGE_MARGIN
    from every projected outline and cutout border, crossed (H W,) int: how many panes the light's ray crosses attenuated).  `solid` and
    `normal_mapped` glass occludes: factor 0."""
    light = LIGHTS[light_name]
    x = floor_points(window)
    w = to_light(light, x)
    factor, use, crossed = np.ones((len(x), 3)), np.ones(len(x), bool), np.zeros(len(x), int)
    for rect, mat in case_quads(case):
        inside, edge, uv = crossing(rect, x, w)
        use &= edge >= EDGE_MARGIN
        if case == "cutout":
            from test_alpha_mask_cpu import tex_alpha_f64

            alpha = tex_alpha_f64(checker(), uv[:, 0], uv[:, 1])
            # alpha is bilinear with slope 2 per unit of u or v; a unit of u or v is at least 1.4 m on the floor
            use &= ~inside | (np.abs(alpha - mat.alpha_cutoff) >= 2.0 * EDGE_MARGIN / 1.4)
            inside = inside & (alpha >= mat.alpha_cutoff)
        if case in ("solid", "normal_mapped"):
            A = np.zeros(3)[None, :] * np.ones((len(x), 1))
        else:
            A = (mat.transmission * pass_fraction(w[:, 1], mat.ior, thin_slab))[:, None] * np.asarray(mat.color, np.float64)[None, :]
            crossed += inside
        factor = np.where(inside[:, None], factor * A, factor)
    return factor, use, crossed


# ---------------------------------------------------------------------------------------------------------------- the canopy
CANOPY = ((-40.0, 40.0), 3.0, (-40.0, 40.0))  # a pane over everything the floor can see but a sliver at the horizon
CANOPY_EMITTER = ((-1.0, 1.0), 5.0, (-1.5, 0.5))
CANOPY_WINDOW = (32, 32)
CANOPY_LENS = (0.0, 1.0, 1.0)


def canopy_world(emitter=False, tau=1.0):
    """the floor under one wide tinted pane, optionally with an emissive quad above the pane: every path from the floor to the sky or the
    emitter crosses the pane, and a path needs one floor vertex per reflection off it, so paths longer than a few vertices carry next to
    nothing (F' is under 0.1 but at grazing angles): estimators that count vertices differently agree long before B = 6"""
    mb = MeshBuilder()
    PW._quad(mb, "floor", (-3.0, 3.0), 0.0, (-3.0, 3.0), Material(ALBEDO, 0.0, 1.0))
    PW._quad(mb, "canopy", CANOPY[0], CANOPY[1], CANOPY[2], glass(TINT2, tau=tau))
    if emitter:
        PW._quad(mb, "lamp", CANOPY_EMITTER[0], CANOPY_EMITTER[1], CANOPY_EMITTER[2], Material((0.0, 0.0, 0.0), 0.0, 1.0, emission=(0.5, 0.4, 0.3)))
    return mb.build()


# ---------------------------------------------------------------------------------------------------------------- the window room
import integrator_worlds as IW  # noqa: E402
from raytracer3_amd import scenes  # noqa: E402

F_NEE_SKY, F_SPECULAR, F_FACEFORWARD, F_NEE_EMISSIVE, F_NEE_PUNCTUAL = 1, 4, 8, 32, 64  # RT3_F_* of include/rt3.h
ROOM_WINDOW_TINT = (0.9, 0.7, 0.5)
ROOM_CAMERA = dict(position=(1.5, 1.6, 1.7), direction=(-0.6, -0.45, -1.0), fov_deg=60.0)
ROOM_LENS = (0.0, 1.0, 1.0)  # the pinhole, antialiased over the pixel
ROOM_LIGHTS = assets.lights_array([
    make_light(LIGHT_DIRECTIONAL, (1.6, 1.4, 1.1), direction=(0.25, -1.0, 0.15)),
    make_light(LIGHT_POINT, (40.0, 34.0, 28.0), position=(0.5, 6.0, -0.4)),
])
# name -> (flags of the code under test, bounces, specular material set, transmission of the pane, emitter outside, punctual lights outside,
# reference samples per pixel, seed, frames of IW.FRAME_SPP samples of the code under test)
WINDOW_CASES = {
    "window_sky_b4": (F_FACEFORWARD | F_NEE_SKY, 4, False, 1.0, False, False, 3072, 401, 12),
    "window_emit_spec_b6": (F_SPECULAR | F_FACEFORWARD | F_NEE_SKY | F_NEE_EMISSIVE, 6, True, 0.5, True, False, 1024, 402, 8),
    "window_sun_b4": (F_NEE_SKY | F_NEE_PUNCTUAL, 4, False, 1.0, False, True, 1024, 403, 20),
}


def window_room(specular=False, tau=1.0, emitter=False, lights=False):
    """A closed room, 4 x 3 x 4, whose only opening is a 2.6 x 2.6 roof light closed by a thin-walled tinted pane: all light enters through
    the pane.  Optionally an emissive quad and two punctual lights (a directional and a point light) above it, outside.  At most 22 triangles."""
    rough, metal = (0.4, 0.0) if specular else (1.0, 0.0)

    def mat(c, emission=(0.0, 0.0, 0.0)):
        return Material(c, metal, rough, emission=emission)
    a, h, o = 2.0, 3.0, 1.3
    g = scenes._grid
    mb = MeshBuilder()
    mb.add("floor", *g([-a, 0, a], [2 * a, 0, 0], [0, 0, -2 * a], 1, 1), mat((0.6, 0.55, 0.5)))
    mb.add("back", *g([-a, 0, -a], [2 * a, 0, 0], [0, h, 0], 1, 1), mat((0.7, 0.7, 0.7)))
    mb.add("front", *g([a, 0, a], [-2 * a, 0, 0], [0, h, 0], 1, 1), mat((0.7, 0.7, 0.7)))
    mb.add("left", *g([-a, 0, a], [0, 0, -2 * a], [0, h, 0], 1, 1), mat((0.7, 0.3, 0.25)))
    mb.add("right", *g([a, 0, -a], [0, 0, 2 * a], [0, h, 0], 1, 1), mat((0.3, 0.5, 0.7)))
    for name, (x0, x1, z0, z1) in (("roof_w", (-a, -o, -a, a)), ("roof_e", (o, a, -a, a)), ("roof_n", (-o, o, -a, -o)), ("roof_s", (-o, o, o, a))):
        mb.add(name, *g([x0, h, z0], [x1 - x0, 0, 0], [0, 0, z1 - z0], 1, 1), mat((0.75, 0.75, 0.75)))
    mb.add("window", *g([-o, h, -o], [2 * o, 0, 0], [0, 0, 2 * o], 1, 1), Material(ROOM_WINDOW_TINT, metal, rough, transmission=tau, ior=IOR, thin_walled=1))
    if emitter:
        mb.add("lamp", *g([-0.8, 4.5, -0.6], [1.6, 0, 0], [0, 0, 1.6], 1, 1), Material((0.0, 0.0, 0.0), 0.0, 1.0, emission=(1.5, 1.2, 0.9)))
    mesh = mb.build()
    if lights:
        mesh.lights = ROOM_LIGHTS.copy()
    return mesh


def window_case(name):
    """(mesh, flags of the float64 reference, its punctual lights) of a case"""
    flags, _, specular, tau, emitter, lights, _, _, _ = WINDOW_CASES[name]
    return window_room(specular, tau, emitter, lights), flags & ~F_NEE_PUNCTUAL, (list(ROOM_LIGHTS) if lights else [])


# ---------------------------------------------------------------------------------------------------------------- the very wide pane
WIDE = ((-300.0, 300.0), 3.0, (-300.0, 300.0))
# from any floor point in view (|x|, |z| < 3) the pane's edge is at least 297 away: a ray can pass beside it only at cos(theta) < 3 / 297
WIDE_MISSED_COS = 3.0 / 297.0


def wide_pane_world():
    """the floor under a 600 x 600 tinted pane: under a constant sky a floor pixel is rho L c 2 int (1 - F'(theta)) cos(theta) sin(theta) d theta"""
    mb = MeshBuilder()
    PW._quad(mb, "floor", (-3.0, 3.0), 0.0, (-3.0, 3.0), Material(ALBEDO, 0.0, 1.0))
    PW._quad(mb, "wide", WIDE[0], WIDE[1], WIDE[2], glass(TINT))
    return mb.build()


def wide_pane_moments(sky_h, thin_slab=True, n=200001):
    """(K, M2): K = 2 int_0^{pi/2} (1 - F') cos sin d theta, so that the expectation of a B = 1 sample is rho L c K; and M2 with
    E[X^2] = (rho L c)^2 M2 for the sky sampler of a CONSTANT sky of sky_h rows as rt3_scene_set_sky defines it: texel density proportional
    to sin(theta) at the row's centre, so the solid-angle density of a direction in row r is p = s_r / (mean_r s_r) / (2 pi^2 sin(theta)),
    and X = (rho / pi) L c (1 - F') cos(theta) / p above the horizon, 0 below."""
    th = (np.arange(n) + 0.5) / n * (np.pi / 2.0)
    dth = (np.pi / 2.0) / n
    pf = pass_fraction(np.cos(th), IOR, thin_slab)
    K = float(np.sum(2.0 * pf * np.cos(th) * np.sin(th)) * dth)
    rows = np.minimum((th / np.pi * sky_h).astype(int), sky_h - 1)
    s_c = np.sin(np.pi * (np.arange(sky_h) + 0.5) / sky_h)
    p = s_c[rows] / s_c.mean() / (2.0 * np.pi * np.pi * np.sin(th))
    M2 = float(np.sum((pf * np.cos(th) / np.pi) ** 2 / p * 2.0 * np.pi * np.sin(th)) * dth)
    return K, M2
