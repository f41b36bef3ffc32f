"""Scenes of the glass tests (tests/test_glass_cpu.py, tests/test_glass.py, tests/golden/gen_glass_ref.py): flat glass facing the camera of
lens_worlds (which looks down -z) so that a pixel's expectation has a closed form, a sealed box for "opaque vertices keep their bits",
and the open room of integrator_worlds with a glass block and a tinted pane for the float64 fixture."""
import math

import numpy as np

import integrator_worlds as IW
import lens_worlds as LW
from raytracer3_amd import assets, scenes
from raytracer3_amd.assets import Material, MeshBuilder

WINDOW = (64, 48)
CAMERA = dict(position=(0.5, 1.0, 3.0), direction=(0.0, 0.0, -1.0), fov_deg=30.0)  # lens_worlds' camera with half its field of view
PINHOLE = (0.0, 1.0, 0.0)  # the per-sample pinhole: every sample of a pixel is its centre's ray
SKY_L = (0.5, 1.0, 0.25)  # a constant sky whose texels RGB9E5 holds exactly
IOR = 1.5
TINT = (0.5, 0.25, 0.75)
LE = LW.LE


def glass(tint=(1.0, 1.0, 1.0), thin=True, tau=1.0, ior=IOR):
    return Material(tint, 0.0, 1.0, transmission=tau, ior=ior, thin_walled=1 if thin else 0)


def _facing_quad(mb, name, x0, x1, y0, y1, depth, mat, window=WINDOW, towards_camera=True):
    """a quad parallel to the film whose edges show at the pixel coordinates x0, x1 (columns) and y0, y1 (rows), at view depth `depth`"""
    c = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)
    pos = LW.pixel_to_world(c[:, 0], c[:, 1], depth, window, CAMERA)
    n = [0.0, 0.0, 1.0] if towards_camera else [0.0, 0.0, -1.0]
    mb.add(name, pos, np.tile(n, (4, 1)), None, [[0, 1, 2], [0, 2, 3]], mat)


# ---------------------------------------------------------------------------------------------------------------- the pane
PANE_COLS, WALL_COLS = (6.75, 30.25), (40.75, 58.0)  # pixel columns of the pane and of the diffuse wall beside it (no edge through a pixel centre)
PANE_ROWS = (5.75, 41.75)
PANE_DEPTH = 4.0
WALL_ALBEDO = (0.5, 0.5, 0.5)


def pane_world(tint=(1.0, 1.0, 1.0), ior=IOR):
    """a thin-walled pane facing the camera and, beside it at the same depth, a diffuse wall that sees nothing but sky: 4 triangles"""
    mb = MeshBuilder()
    _facing_quad(mb, "pane", *PANE_COLS, *PANE_ROWS, PANE_DEPTH, glass(tint, ior=ior))
    _facing_quad(mb, "wall", *WALL_COLS, *PANE_ROWS, PANE_DEPTH, Material(WALL_ALBEDO, 0.0, 1.0))
    return mb.build()


def inside(cols, rows, window=WINDOW, margin=0.0):
    """(H, W) bool: the pixels whose centres lie inside the rectangle of pixel coordinates, `margin` pixels in from its edges"""
    W, H = window
    py, px = np.mgrid[0:H, 0:W]
    return ((px + 0.5 > cols[0] + margin) & (px + 0.5 < cols[1] - margin) & (py + 0.5 > rows[0] + margin) & (py + 0.5 < rows[1] - margin))


def pixel_dirs(window=WINDOW):
    """(H, W, 3) unit directions of the pixel centres' rays"""
    W, H = window
    py, px = np.mgrid[0:H, 0:W]
    p = LW.pixel_to_world(px + 0.5, py + 0.5, 1.0, window, CAMERA) - np.asarray(CAMERA["position"], np.float64)
    return p / np.linalg.norm(p, axis=-1, keepdims=True)


# ---------------------------------------------------------------------------------------------------------------- the slab
SLAB_DEPTH, SLAB_THICKNESS = 3.0, 0.5


def slab_world(ior=IOR, tilt_deg=0.0, emitter_edge_px=None, emitter_depth=6.0, with_slab=True):
    """a solid slab: two parallel quads SLAB_THICKNESS apart that reach far past the view, the front one's normal towards the camera,
    turned by tilt_deg about the vertical axis through the point at SLAB_DEPTH on the camera's axis.  With emitter_edge_px a black,
    emissive half-plane behind it whose left edge shows (without the slab) at that pixel column.  Returns (mesh, unit normal of the
    front face, a point on the front face)."""
    cam = np.asarray(CAMERA["position"], np.float64)
    a = math.radians(tilt_deg)
    n = np.array([math.sin(a), 0.0, math.cos(a)])
    u, v = np.array([math.cos(a), 0.0, -math.sin(a)]), np.array([0.0, 1.0, 0.0])
    centre = cam + np.array([0.0, 0.0, -SLAB_DEPTH])
    mb = MeshBuilder()
    if with_slab:
        for name, c, nn in (("slab_front", centre, n), ("slab_back", centre - SLAB_THICKNESS * n, -n)):
            E = 40.0
            pos = np.array([c - E * u - E * v, c + E * u - E * v, c + E * u + E * v, c - E * u + E * v])
            mb.add(name, pos, np.tile(nn, (4, 1)), None, [[0, 1, 2], [0, 2, 3]], glass(thin=False, ior=ior))
    if emitter_edge_px is not None:
        W, H = WINDOW
        c = [[emitter_edge_px, -3.0 * H], [4.0 * W, -3.0 * H], [4.0 * W, 4.0 * H], [emitter_edge_px, 4.0 * H]]
        c = np.asarray(c, np.float64)
        pos = LW.pixel_to_world(c[:, 0], c[:, 1], emitter_depth, WINDOW, CAMERA)
        mb.add("emitter", pos, np.tile([0.0, 0.0, 1.0], (4, 1)), None, [[0, 1, 2], [0, 2, 3]], Material((0.0, 0.0, 0.0), 0.0, 1.0, emission=LW.EMISSION))
    return mb.build(), n, centre


def slab_displacement(r, n, thickness, ior):
    """The closed form of a ray through a plane-parallel slab: it leaves parallel to itself, displaced by t sin(theta_i - theta_t) /
    cos(theta_t) across its direction, in the plane of incidence, towards the side the normal's far end lies on.  r: (..., 3) unit ray
    directions; n: the unit normal of the face the rays meet, pointing at them.  Returns (the offset vectors, theta_i, theta_t)."""
    cos_i = -np.sum(r * n, -1)
    th_i = np.arccos(np.clip(cos_i, -1.0, 1.0))
    th_t = np.arcsin(np.sin(th_i) / ior)
    size = thickness * np.sin(th_i - th_t) / np.cos(th_t)
    w = -n - cos_i[..., None] * r  # across r, in the plane of incidence, into the slab
    ln = np.linalg.norm(w, axis=-1, keepdims=True)
    w = np.where(ln > 1e-300, w / np.maximum(ln, 1e-300), 0.0)
    return size[..., None] * w, th_i, th_t


def edge_distance(n, ior, emitter_edge_px, emitter_depth=6.0):
    """(H, W): x of the point where each pixel centre's ray, displaced by the slab, meets the emitter's plane, minus the emitter's edge
    (metres; >= 0: the pixel sees the emitter), and the incidence angles theta_i"""
    cam = np.asarray(CAMERA["position"], np.float64)
    r = pixel_dirs()
    off, th_i, _ = slab_displacement(r, n, SLAB_THICKNESS, ior)
    o = cam + off
    s = (cam[2] - emitter_depth - o[..., 2]) / r[..., 2]
    x = o[..., 0] + s * r[..., 0]
    edge = LW.pixel_to_world(np.array([emitter_edge_px]), np.array([0.0]), emitter_depth, WINDOW, CAMERA)[0, 0]
    return x - np.float64(np.float32(edge)), th_i


# ---------------------------------------------------------------------------------------------------------------- the sealed box
def sealed_world(n_extra=0, textured=False, emissive=False):
    """A closed diffuse room (the furnace room's box, inward normals) with an opaque block, and inside a second, closed box a triangle
    that no path can reach: geometry `sealed`.  n_extra more geometries (one small triangle each, on the floor, visible) bring the
    flattened geometry count past the LDS table's 256; textured: the room's walls get a metallic-roughness map (the side table of
    section 4j); emissive: the block emits (something for RT3_F_NEE_EMISSIVE to sample).  Returns (mesh, index of `sealed`)."""
    s = 2.0
    mb = MeshBuilder()
    scenes._box(mb, "room", [-s] * 3, [s] * 3, Material((0.6, 0.5, 0.7), 0.2, 0.6, metallic_roughness_texture=0 if textured else -1), inward=True)
    scenes._box(mb, "block", [-0.9, -2.0, -1.2], [-0.1, -0.8, -0.4], Material((0.7, 0.7, 0.3), 0.0, 0.8, emission=(0.3, 0.25, 0.2) if emissive else (0.0, 0.0, 0.0)))
    scenes._box(mb, "casket", [0.5, -2.0, -1.0], [1.1, -1.4, -0.4], Material((0.3, 0.6, 0.4), 0.5, 0.5))
    mb.add("sealed", [[0.6, -1.9, -0.9], [1.0, -1.9, -0.9], [0.8, -1.5, -0.5]], np.tile([0.0, 0.0, 1.0], (3, 1)), None, [[0, 1, 2]], glass(thin=False))
    rng = np.random.default_rng(11)
    for k in range(n_extra):
        x, z = -1.8 + 3.6 * ((k % 20) + 0.2) / 20.0, -1.8 + 3.0 * ((k // 20) + 0.2) / 20.0
        col = tuple(rng.uniform(0.2, 0.9, 3))
        mb.add(f"chip{k}", [[x, -1.99, z], [x + 0.1, -1.99, z], [x, -1.99, z - 0.1]], np.tile([0.0, 1.0, 0.0], (3, 1)), None, [[0, 1, 2]], Material(col, 0.0, 0.9))
    mesh = mb.build()
    if textured:
        yy, xx = np.mgrid[0:8, 0:8]
        mesh.textures = [np.ascontiguousarray(np.stack([np.zeros_like(xx), 90 + 12 * xx, 30 + 20 * yy, np.full_like(xx, 255)], -1).astype(np.uint8))]
    return mesh, mesh.names.index("sealed")


SEALED_CAMERA = dict(position=(0.2, 0.3, 1.8), direction=(0.05, -0.45, -1.0), fov_deg=70.0)
SEALED_LIGHT = dict(position=(0.5, 1.2, 0.4), intensity=(6.0, 5.0, 4.0))


# ---------------------------------------------------------------------------------------------------------------- the fixture's room
ROOM_PANE_TINT = (0.9, 0.55, 0.35)
F_NEE_SKY, F_SPECULAR, F_FACEFORWARD = IW.F_NEE_SKY, IW.F_SPECULAR, IW.F_FACEFORWARD
# name -> (flags, bounces, specular material set, transmission of the glass, reference samples per pixel, seed, frames of the code under test)
ROOM_CASES = {
    "glass_b4": (0, 4, False, 1.0, 12288, 301, 40),
    "glass_spec_b6": (F_SPECULAR | F_FACEFORWARD | F_NEE_SKY, 6, True, 1.0, 4096, 302, 16),
    "glass_half_b4": (F_FACEFORWARD | F_NEE_SKY, 4, False, 0.5, 3072, 303, 12),
}
ROOM_LENS = (0.0, 1.0, 1.0)  # the pinhole, antialiased over the pixel


def glass_room(specular=False, tau=1.0):
    """integrator_worlds.open_room() whose block is solid glass, with a thin-walled, tinted pane standing on the floor between the block
    and the camera: 20 triangles.  `tau` is the transmission of both."""
    room = IW.open_room(specular)
    mb = MeshBuilder()
    rough, metal = (0.4, 0.0) if specular else (1.0, 0.0)
    mb.add("pane", *scenes._grid([0.2, 0.0, 0.6], [1.6, 0.0, -1.0], [0.0, 1.8, 0.0], 1, 1), Material(ROOM_PANE_TINT, metal, rough))
    add = mb.build()
    g = add.geometries.copy()
    g["index_offset"] += len(room.indices)
    g["vertex_offset"] += len(room.vertices)
    mesh = assets.Mesh(np.ascontiguousarray(np.concatenate([room.vertices, add.vertices]), np.float32),
                       np.ascontiguousarray(np.concatenate([room.indices, add.indices]), np.uint32), np.concatenate([room.geometries, g]),
                       np.concatenate([room.prim_counts, add.prim_counts]).astype(np.uint32), room.names + add.names)
    for name, thin in (("block", 0), ("pane", 1)):
        k = mesh.names.index(name)
        mesh.transmission[k] = (tau, IOR, thin, 0)
    return mesh
