"""Scenes of the fog tests (tests/test_fog_cpu.py, tests/test_fog.py): a camera that looks down -z at nothing, a
slab-shaped box of medium across the view, a sun straight above it, a lamp above it, and an occluder over a part of it.  Every quantity a
closed form needs is computed here in float64."""
import math

import numpy as np

import lens_worlds as LW
import ref_fog as RF
from raytracer3_amd.assets import LIGHT_DIRECTIONAL, LIGHT_POINT, Material, MeshBuilder, lights_array, make_light

WINDOW = (48, 31)  # an odd height: the rays of row 15 are horizontal
CENTRE_ROW = 15
CAMERA = dict(position=(0.5, 1.0, 3.0), direction=(0.0, 0.0, -1.0), fov_deg=40.0)
PINHOLE = (0.0, 1.0, 0.0)  # the per-sample pinhole: no jitter
SKY = (0.5, 1.0, 0.25)  # a constant sky whose texels RGB9E5 holds exactly

# the slab: every view ray enters through z = 1 and most leave through z = -1; the top and bottom rows leave through y = 2 or y = 0
SLAB = ((-50.0, 0.0, -1.0), (50.0, 2.0, 1.0))
SIGMA_A, SIGMA_S = 0.1, 0.3  # grey
SUN_E = (3.0, 2.0, 1.0)
LAMP_P, LAMP_I = (0.8, 3.0, 0.2), (30.0, 20.0, 10.0)
EDGE_X = 0.2  # the occluder covers x < EDGE_X from the sun


def medium(sigma_a=SIGMA_A, sigma_s=SIGMA_S, g=0.0, box=SLAB):
    """(L.Medium, the tuple ref_fog takes: sigma_t, sigma_s, g, lo, hi with sigma_t the fp32 sum)"""
    from raytracer3_amd import _lib as L

    three = lambda v: np.full(3, v, np.float32) if np.isscalar(v) else np.asarray(v, np.float32)
    sa, ss = three(sigma_a), three(sigma_s)
    lo, hi = np.asarray(box[0], np.float32), np.asarray(box[1], np.float32)
    m = L.Medium(tuple(sa), tuple(ss), g, tuple(lo), tuple(hi))
    return m, ((sa + ss).astype(np.float64), ss.astype(np.float64), float(np.float32(g)), lo.astype(np.float64), hi.astype(np.float64))


CANOPY_TINT, CANOPY_TAU, CANOPY_IOR = (0.5, 0.25, 0.75), 0.5, 1.5


def hidden_world(occluder=False, canopy=False):
    """one black triangle behind the camera, which no view ray meets; with `occluder` a black quad at y = 2.5 over x < EDGE_X; with
    `canopy` a thin-walled pane at y = 2.5 over everything the slab's points can see of the sun"""
    mb = MeshBuilder()
    black = Material((0.0, 0.0, 0.0), 0.0, 1.0)
    mb.add("hidden", np.array([[0.0, 0.0, 10.0], [1.0, 0.0, 10.0], [0.0, 1.0, 10.0]]), np.tile([0.0, 0.0, -1.0], (3, 1)), None, [[0, 1, 2]], black)
    if occluder:
        pos = np.array([[-60.0, 2.5, -6.0], [EDGE_X, 2.5, -6.0], [EDGE_X, 2.5, 6.0], [-60.0, 2.5, 6.0]])
        mb.add("occluder", pos, np.tile([0.0, -1.0, 0.0], (4, 1)), None, [[0, 1, 2], [0, 2, 3]], black)
    if canopy:
        pos = np.array([[-60.0, 2.5, -6.0], [60.0, 2.5, -6.0], [60.0, 2.5, 6.0], [-60.0, 2.5, 6.0]])
        mb.add("canopy", pos, np.tile([0.0, 1.0, 0.0], (4, 1)), None, [[0, 2, 1], [0, 3, 2]],
               Material(CANOPY_TINT, 0.0, 1.0, transmission=CANOPY_TAU, ior=CANOPY_IOR, thin_walled=1))
    return mb.build()


PANEL = ((0.0, 3.2, -0.6), (1.2, 0.0, 0.0), (0.0, 0.0, 1.0))  # A, E1, E2 of the emissive quad above the slab, out of every view
PANEL_EMISSION = (1.0, 0.5, 0.25)  # x 12 in hit_info


def panel_world():
    """hidden_world with an emissive quad above the slab: two emitter triangles of equal area"""
    mb = MeshBuilder()
    black = Material((0.0, 0.0, 0.0), 0.0, 1.0)
    mb.add("hidden", np.array([[0.0, 0.0, 10.0], [1.0, 0.0, 10.0], [0.0, 1.0, 10.0]]), np.tile([0.0, 0.0, -1.0], (3, 1)), None, [[0, 1, 2]], black)
    A, E1, E2 = (np.asarray(v, np.float64) for v in PANEL)
    mb.add("panel", np.array([A, A + E1, A + E1 + E2, A + E2]), np.tile([0.0, -1.0, 0.0], (4, 1)), None, [[0, 1, 2], [0, 2, 3]],
           Material((0.0, 0.0, 0.0), 0.0, 1.0, emission=PANEL_EMISSION))
    return mb.build()


def sun():
    return lights_array([make_light(LIGHT_DIRECTIONAL, SUN_E, direction=(0.0, -1.0, 0.0))])


def lamp():
    return lights_array([make_light(LIGHT_POINT, LAMP_I, position=LAMP_P)])


TILTED_CAMERA = dict(position=(0.5, 1.8, 3.0), direction=(0.0, -0.5, -1.0), fov_deg=40.0)  # looks down into the slab: four rays in ten leave through y = 0


def pixel_dirs(window=WINDOW, cam=CAMERA):
    """(H, W, 3) unit directions of the pixel centres' rays, from the frame's fp32 matrices (pane_worlds.floor_points' construction)"""
    from support import camera

    W, H = window
    g = camera(cam, window).gconst(window)
    pinv = np.array(g.proj_inverse[:], np.float64).reshape(4, 4).T
    vinv = np.array(g.view_inverse[:], np.float64).reshape(4, 4).T
    py, px = np.mgrid[0:H, 0:W]
    dx, dy = (px + 0.5) / W * 2 - 1, -((py + 0.5) / H * 2 - 1)
    t = np.stack([dx, dy, np.ones_like(dx), np.ones_like(dx)], -1) @ pinv.T
    t = t[..., :3] / np.linalg.norm(t[..., :3], axis=-1, keepdims=True)
    return t @ vinv[:3, :3].T


def chords(box=SLAB, window=WINDOW, cam=CAMERA):
    """(H, W) length of every pixel ray inside the box"""
    d = pixel_dirs(window, cam).reshape(-1, 3)
    ok, t0, t1 = RF.span(cam["position"], d, np.inf, box[0], box[1])
    return np.where(ok, t1 - t0, 0.0).reshape(window[1], window[0])


def occluder_t_end(window=WINDOW, cam=CAMERA):
    """(H W,) where a pixel ray meets the occluder's plane inside its rectangle (inf otherwise): above the box, so no segment is cut"""
    d = pixel_dirs(window, cam).reshape(-1, 3)
    o = np.asarray(cam["position"], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (2.5 - o[1]) / d[:, 1]
        x = o + t[:, None] * d
    hit = (t > 0) & (x[:, 0] < EDGE_X) & (x[:, 0] > -60.0) & (np.abs(x[:, 2]) < 6.0)
    return np.where(hit, t, np.inf)


def lit(x):
    """the sun reaches x past the occluder"""
    return (x[:, 0] > EDGE_X).astype(np.float64)


def shaft_centre_row(g, sigma_a=SIGMA_A, sigma_s=SIGMA_S):
    """(W, 3) the closed form of the horizontal row under the sun: sigma_s p_HG(0) E e^(-sigma_t h) (1 - e^(-sigma_t l)) / sigma_t, and (l,
    h): the rays are horizontal, so every point of one is h = 1 below the slab's top and the estimator is constant"""
    _, (st, ss, gg, lo, hi) = medium(sigma_a, sigma_s, g)
    l = chords()[CENTRE_ROW]
    h = hi[1] - CAMERA["position"][1]
    val = ss * RF.phase(gg, 0.0) * np.asarray(SUN_E) * np.exp(-st * h) * (1.0 - np.exp(-st[None, :] * l[:, None])) / st
    return val, l, h


def shadowed_centre_row(sigma_a=SIGMA_A, sigma_s=SIGMA_S):
    """(W, 3) the same with the occluder: only the part of a ray with x > EDGE_X is lit.  The ray enters the slab at distance r0 with
    x = ox + r0 dx and crosses x = EDGE_X at r_e: the lit part is [a, b] of [0, l] (measured from the entry), and the integral of
    e^(-sigma_t r) over it replaces (1 - e^(-sigma_t l)) / sigma_t."""
    _, (st, ss, gg, lo, hi) = medium(sigma_a, sigma_s, 0.0)
    d = pixel_dirs()[CENTRE_ROW]
    o = np.asarray(CAMERA["position"], np.float64)
    ok, t0, t1 = RF.span(o, d, np.inf, lo, hi)
    with np.errstate(divide="ignore"):
        te = (EDGE_X - o[0]) / d[:, 0]  # where the ray crosses the edge's plane
    right = d[:, 0] > 0
    a = np.where(right, np.clip(te, t0, t1), t0) - t0
    b = np.where(right, t1, np.clip(te, t0, t1)) - t0
    h = hi[1] - o[1]
    integral = (np.exp(-st[None, :] * a[:, None]) - np.exp(-st[None, :] * b[:, None])) / st
    return ss * RF.phase(gg, 0.0) * np.asarray(SUN_E) * np.exp(-st * h) * integral, (b - a) / (t1 - t0)


# ---------------------------------------------------------------------------------------------------------------- the fogged room
F_NEE_SKY, F_FACEFORWARD, F_NEE_EMISSIVE, F_NEE_PUNCTUAL = 1, 8, 32, 64  # RT3_F_* of include/rt3.h
ROOM_BOX = ((-2.5, 0.0, -2.5), (2.5, 4.0, 2.5))  # the room of pane_worlds.window_room() and a metre of the air above its roof light
ROOM_SIGMA_A, ROOM_SIGMA_S, ROOM_G = (0.04, 0.05, 0.06), (0.25, 0.2, 0.15), 0.4
# name -> (flags of the code under test, bounces, reference samples per pixel, seed, frames of IW.FRAME_SPP samples of the code under test)
ROOM_CASES = {"fog_room_b5": (F_FACEFORWARD | F_NEE_SKY | F_NEE_EMISSIVE | F_NEE_PUNCTUAL, 5, 768, 501, 12)}


def fog_room():
    """pane_worlds.window_room(): a closed room lit through the half-transmitting tinted pane of its roof light by the sky, a sun, a point
    lamp and an emissive quad above it, the quad carrying emitter_tex_worlds.HALF as its emissive texture (one textured emitter)"""
    import emitter_tex_worlds as EW
    import pane_worlds as PN

    mesh = EW.with_emissive_texture(PN.window_room(False, 0.5, True, False), "lamp", [EW.HALF])
    mesh.lights = PN.ROOM_LIGHTS.copy()
    return mesh


def room_medium():
    return medium(ROOM_SIGMA_A, ROOM_SIGMA_S, ROOM_G, ROOM_BOX)


def room_surface(mesh, scene):
    """a `surface` for ref_fog.room_radiance_samples: the per-geometry constants of `scene` = ref_pathtrace.Scene(mesh), and on the lamp
    its emission times the emissive texture at the hit (bilinear, repeat addressing, sRGB decode: ref_materials' lookup)"""
    import ref_materials as RM
    import ref_surface as RS
    from test_alpha_mask_cpu import tri_uvs

    uv = tri_uvs(mesh)[0].astype(np.float64)
    lamp, tex = mesh.names.index("lamp"), np.asarray(mesh.textures[0], np.uint8)

    def surface(tri, x, nrm):
        g = scene.geom[tri]
        emi = scene.emission[g].copy()
        k = np.flatnonzero(g == lamp)
        if len(k):
            t = tri[k]
            w, e1, e2 = x[k] - scene.v0[t], scene.e1[t], scene.e2[t]
            d11, d12, d22 = np.sum(e1 * e1, -1), np.sum(e1 * e2, -1), np.sum(e2 * e2, -1)
            w1, w2 = np.sum(w * e1, -1), np.sum(w * e2, -1)
            den = d11 * d22 - d12 * d12
            bu, bv = (d22 * w1 - d12 * w2) / den, (d11 * w2 - d12 * w1) / den
            u = uv[t, 0, 0] * (1.0 - bu - bv) + uv[t, 1, 0] * bu + uv[t, 2, 0] * bv
            v = uv[t, 0, 1] * (1.0 - bu - bv) + uv[t, 1, 1] * bu + uv[t, 2, 1] * bv
            emi[k] = emi[k] * RM.linear_bilinear(tex, u, v, RS.srgb_eotf)[:, :3]
        return scene.albedo[g], emi, nrm, scene.roughness[g], scene.metalness[g]

    return surface
