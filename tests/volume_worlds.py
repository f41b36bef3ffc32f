"""Scenes of the absorption tests (tests/test_volume_cpu.py, tests/test_volume.py, tests/golden/gen_volume_ref.py): glass_worlds' solid slab with
absorption coefficients, so that a pixel's expectation has a closed form; three small bodies for k_absorb's queue test; and glass_worlds'
room with an absorbing block and an absorbing sphere for the float64 fixture."""
import math

import numpy as np

import glass_worlds as GW
import integrator_worlds as IW
from raytracer3_amd import assets, scenes
from raytracer3_amd.assets import Material, MeshBuilder

WINDOW, CAMERA, PINHOLE, SKY_L = GW.WINDOW, GW.CAMERA, GW.PINHOLE, GW.SKY_L
THICKNESS = GW.SLAB_THICKNESS
# sigma x thickness = 0.5 / 1 / 2 per channel
SLAB_SIGMA = (0.5 / THICKNESS, 1.0 / THICKNESS, 2.0 / THICKNESS)


def with_sigma(mesh, sigmas):
    """`mesh` with the absorption coefficients {geometry name: sigma rgb}; every other geometry keeps 0"""
    at = assets.no_attenuation(len(mesh.geometries))
    for name, s in sigmas.items():
        at["sigma"][mesh.names.index(name)] = s
    mesh.attenuation = at
    mesh.attenuation_source = None
    return mesh


# ---------------------------------------------------------------------------------------------------------------- the absorbing slab
def slab_world(ior=GW.IOR, tilt_deg=0.0, sigma=SLAB_SIGMA):
    """glass_worlds.slab_world whose two faces (one geometry each) absorb.  Returns (mesh, unit normal of the front face, a point on it)."""
    mesh, n, centre = GW.slab_world(ior=ior, tilt_deg=tilt_deg)
    return with_sigma(mesh, {"slab_front": sigma, "slab_back": sigma}), n, centre


def slab_geometry(mesh, n, window=WINDOW):
    """Per pixel centre's ray, in float64, against the slab's triangles as the mesh stores them (float32 vertices: the two faces are
    parallel and THICKNESS apart to a few 1e-6 only, and a face's two triangles are not exactly coplanar): cos of the incidence angle on
    the ideal front face, the distances from the camera to the front and to the back face along the straight ray, and the largest
    coordinate magnitude of the two hit points.  (H, W) each, the last a scalar."""
    import ref_pathtrace as RP

    cam = np.asarray(CAMERA["position"], np.float64)
    r = GW.pixel_dirs(window)
    H, W = r.shape[:2]
    scene = RP.Scene(mesh)
    o, d = np.tile(cam, (H * W, 1)), r.reshape(-1, 3)
    tri, t_front, _ = scene.trace(o, d)
    assert (tri >= 0).all() and all(mesh.names[g] == "slab_front" for g in np.unique(scene.geom[tri]))
    tri2, seg, _ = scene.trace(o + t_front[:, None] * d, d)
    assert (tri2 >= 0).all() and all(mesh.names[g] == "slab_back" for g in np.unique(scene.geom[tri2]))
    t_back = t_front + seg
    p = np.concatenate([o + t_front[:, None] * d, o + t_back[:, None] * d])
    return -np.sum(r * n, -1), t_front.reshape(H, W), t_back.reshape(H, W), float(np.abs(p).max())


def slab_outline_share(n, centre, window=WINDOW):
    """(share of the window's pixels that lie on the slab, share of those within one pixel of its outline): the slab's quads reach 40 m to
    every side, so every pixel's ray meets both faces far from their edges"""
    cam = np.asarray(CAMERA["position"], np.float64)
    r = GW.pixel_dirs(window)
    u, v = np.array([n[2], 0.0, -n[0]]), np.array([0.0, 1.0, 0.0])
    cos_i = -np.sum(r * n, -1)
    t_front, t_back = np.sum((centre - cam) * n) / np.sum(r * n, -1), np.sum((centre - THICKNESS * n - cam) * n) / np.sum(r * n, -1)
    on = np.ones(cos_i.shape, bool)
    near = np.zeros(cos_i.shape, bool)
    pixel = 2.0 * math.tan(math.radians(CAMERA["fov_deg"]) / 2.0) / window[1]  # a pixel's width at distance 1
    for t, c in ((t_front, centre), (t_back, centre - THICKNESS * n)):
        p = cam + t[..., None] * r - c
        a, b = np.abs(np.sum(p * u, -1)), np.abs(np.sum(p * v, -1))
        on &= (t > 0.0) & (a < 40.0) & (b < 40.0)
        near |= (40.0 - np.maximum(a, b)) < 2.0 * pixel * t / np.maximum(cos_i, 1e-3)
    return float(on.mean()), float((near & on).sum() / max(int(on.sum()), 1))


# ---------------------------------------------------------------------------------------------------------------- the queue test's bodies
BODY_SIGMA = (1.5, 0.0, 4.0)  # a channel with sigma 0 keeps its bits


def _rounded_box(mb, name, lo, hi, mat, roundness=0.3):
    """scenes._box with vertex normals leaning outwards from the centre, so that a hit's normal depends on its barycentrics"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    sub = MeshBuilder()
    scenes._box(sub, name, lo, hi, mat)
    m = sub.build()
    pos, nrm = m.vertices[:, :3].astype(np.float64), m.vertices[:, 3:6].astype(np.float64)
    radial = pos - 0.5 * (lo + hi)
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    mb.add(name, pos, nrm + roundness * radial, None, m.indices.reshape(-1, 3), mat)


def bodies():
    """an absorbing box, a solid glass box with sigma 0 and an opaque quad: 26 triangles in three geometries"""
    mb = MeshBuilder()
    _rounded_box(mb, "amber", [-1.0, 0.0, -1.0], [0.0, 1.0, 0.0], GW.glass(thin=False))
    _rounded_box(mb, "clear", [0.5, 0.0, -1.0], [1.5, 1.0, 0.0], GW.glass(thin=False))
    mb.add("wall", *scenes._grid([-2.0, 0.0, -2.0], [4.0, 0.0, 0.0], [0.0, 2.0, 0.0], 1, 1), Material((0.5, 0.5, 0.5), 0.0, 1.0))
    return with_sigma(mb.build(), {"amber": BODY_SIGMA})


def bodies_matrix():
    """a rotation about (1, 2, 3) by 40 degrees, a uniform scale of 1.5 and a translation: 4 x 4, object -> world"""
    k = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = math.radians(40.0)
    R = np.eye(3) + math.sin(a) * K + (1.0 - math.cos(a)) * (K @ K)
    M = np.eye(4)
    M[:3, :3] = 1.5 * R
    M[:3, 3] = (0.3, -0.2, 0.1)
    return M.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the fixture's room
ROOM_SIGMA = {"block": (3.0, 0.9, 0.15), "ball": (0.4, 2.5, 1.2)}  # an amber block, a green sphere
BALL = dict(centre=(1.0, 0.45, 0.9), radius=0.4)
# name -> (flags, bounces, specular material set, transmission of the glass, reference samples per pixel, seed, frames of the code under test)
ROOM_CASES = {
    "amber_b6": (GW.F_FACEFORWARD | GW.F_NEE_SKY, 6, False, 1.0, 3072, 401, 12),
}
ROOM_LENS = GW.ROOM_LENS


def absorbing_room(specular=False, tau=1.0, sigmas=ROOM_SIGMA):
    """glass_worlds.glass_room() with a solid glass sphere standing in front of the pane; the block and the sphere absorb"""
    room = GW.glass_room(specular, tau)
    mb = MeshBuilder()
    scenes._sphere(mb, "ball", list(BALL["centre"]), BALL["radius"], 10, 5, GW.glass(thin=False, tau=tau))
    add = mb.build()
    g = add.geometries.copy()
    g["index_offset"] += len(room.indices)
    g["vertex_offset"] += len(room.vertices)
    mesh = assets.Mesh(np.ascontiguousarray(np.concatenate([room.vertices, add.vertices]), np.float32),
                       np.ascontiguousarray(np.concatenate([room.indices, add.indices]), np.uint32), np.concatenate([room.geometries, g]),
                       np.concatenate([room.prim_counts, add.prim_counts]).astype(np.uint32), room.names + add.names,
                       transmission=np.concatenate([room.transmission, add.transmission]))
    return with_sigma(mesh, sigmas)


def sigma_table(mesh):
    """(g, 3) float64 absorption coefficients of the geometries the build classifies as absorbing, 0 for every other"""
    s = np.asarray(mesh.attenuation["sigma"], np.float64).copy()
    s[~mesh.absorbing()] = 0.0
    return s
