"""Scenes of the lens tests (tests/test_lens_cpu.py, tests/test_lens.py, tests/golden/gen_lens_ref.py): flat emitters facing a camera
that looks down -z, placed by the pixel coordinates their edges are to have, so that a pixel's expectation has a closed form."""
import math

import numpy as np

from raytracer3_amd.assets import Material, MeshBuilder

WINDOW = (32, 24)
CAMERA = dict(position=(0.5, 1.0, 3.0), direction=(0.0, 0.0, -1.0), fov_deg=60.0)
EMISSION = (0.25, 0.125, 0.5)  # x 12 in hit_info: Le = (3, 1.5, 6), and every multiple of it up to 4096 is an fp32 number
LE = np.array([3.0, 1.5, 6.0])
RECT_PX = (9.3, 20.65, 5.4, 16.25)  # x0, x1, y0, y1 in pixels: fractional bounds
RECT_DEPTH = 4.0
SKY_C = (0.5, 0.25, 1.0)  # a constant sky whose texels RGB9E5 holds exactly

# the thin-lens cases: half-plane x >= EDGE_PX at view depth z, lens radius and focus; (name, z)
# (circle of confusion at 24 rows and 60 degrees: 0.8 |1/4 - 1/z| 24 / (2 tan 30 deg) = 2.5 pixels at z = 2.5, 2.3 at z = 9)
LENS_R, LENS_F, EDGE_PX = 0.8, 4.0, 14.4
HALF_PLANE_DEPTHS = (("near", 2.5), ("sharp", 4.0), ("far", 9.0))

# the lens of the float64 fixture (open room of integrator_worlds): focused on the block, 6 away; the circle of confusion of the near floor
# (depth 3) is 0.4 |1/6 - 1/3| 32 / (2 tan 30 deg) = 1.8 pixels of the 48 x 32 window
ROOM_LENS = (0.4, 6.0, 1.0)
# name -> (flags, bounces, specular material set, reference samples per pixel, seed, frames of the code under test)
F_NEE_SKY, F_SPECULAR, F_FACEFORWARD = 1, 4, 8
ROOM_CASES = {
    "lens_sky_b4": (F_NEE_SKY | F_FACEFORWARD, 4, False, 3072, 201, 8),
    "lens_spec_b4": (F_NEE_SKY | F_FACEFORWARD | F_SPECULAR, 4, True, 3584, 202, 8),
}


# The textured room of the fixture: material_worlds.room() with normal maps and metallic-roughness maps on what the camera sees (floor,
# back and left wall, both boxes) and an emitting ceiling, so that with B = 2 a pixel's expectation is the vertex-0 BSDF -- textured
# normal, roughness and metalness -- integrated against the emitters.  The box is closed to straight lines, not to shading: where a normal
# map tilts the shading normal, directions above it lie below the wall itself, and rays along them leave the scene (the walls are single
# quads).  Those see the sky, by BSDF sampling and by sky NEE alike; the scene has a dim constant sky for them (a bright one behind the
# low-roughness texels of the metallic-roughness maps is what the reference's cosine sampling is noisiest at).
MATERIAL_SKY_C = (0.0625, 0.03125, 0.125)
MATERIAL_LENS = (0.05, 3.0, 1.0)  # the eye is 0.1 in front of the wall behind it; the disk, tilted by 14 degrees, reaches 0.012 towards it
MATERIAL_CEILING_EMISSION = (0.1, 0.1, 0.1)
MATERIAL_CASES = {"lens_mat_b2": (F_NEE_SKY | F_FACEFORWARD | F_SPECULAR, 2, True, 2560, 203, 10)}


def material_room():
    """(mesh, camera)"""
    import material_worlds as MW

    from raytracer3_amd import scenes

    # material_worlds.room()'s box, panel and camera, with a leaning slab for its two boxes.  Every quad's cells are at most 3/4 as long
    # along v as along u: the condition under which ref_materials vouches for a triangle's tangent (no cancellation in e1 dv2 - e2 dv1).
    q = scenes._grid
    parts = {
        "floor": q([-2, 0, 2], [4, 0, 0], [0, 0, -4], 2, 4), "ceiling": q([-2, 3, -2], [4, 0, 0], [0, 0, 4], 2, 4),
        "back": q([-2, 0, -2], [4, 0, 0], [0, 3, 0], 2, 2), "front": q([2, 0, 2], [-4, 0, 0], [0, 3, 0], 2, 2),
        "left": q([-2, 0, 2], [0, 0, -4], [0, 3, 0], 2, 2), "right": q([2, 0, -2], [0, 0, 4], [0, 3, 0], 2, 2),
        "panel": q([-0.8, 2.95, -0.8], [1.6, 0, 0], [0, 0, 1.6], 2, 4), "slab": q([-1.2, 0.0, -0.2], [1.6, 0, 0], [0, 0.8, -0.9], 2, 4),
    }
    rng = np.random.default_rng(21)
    mb = MeshBuilder()
    for name, part in parts.items():
        emission = {"panel": (0.25, 0.23, 0.2), "ceiling": MATERIAL_CEILING_EMISSION}.get(name, (0.0, 0.0, 0.0))
        mb.add(name, *part, Material(tuple(rng.uniform(0.4, 0.9, 3)), float(rng.uniform(0.2, 1.0)), float(rng.uniform(0.3, 1.0)), emission))
    mesh = mb.build()
    names = mesh.names
    textures = MW.colour_textures(rng, [(8, 8), (5, 3)]) + MW.normal_textures(rng, [(16, 16), (7, 5), (1, 1)])
    nm = {names.index("floor"): 2, names.index("back"): 3, names.index("left"): 2, names.index("slab"): 3}
    mr = {names.index("floor"): 0, names.index("back"): 1, names.index("slab"): 0, names.index("right"): 1}
    t = MW.table(len(names), normal_texture=nm, metallic_roughness_texture=mr, normal_scale={names.index("floor"): 1.5, names.index("back"): 0.5})
    cam = dict(position=(0.0, 1.5, 1.9), direction=(0.0, -0.25, -1.0), fov_deg=70.0)
    return MW.with_tables(mesh, material_textures=t, textures=textures), cam


def pixel_to_world(px, py, depth, window=WINDOW, cam=CAMERA):
    """the world point at view depth `depth` that the pinhole shows at pixel coordinates (px, py); the camera looks down -z, +y up"""
    W, H = window
    th = math.tan(0.5 * math.radians(cam["fov_deg"]))
    pos = np.asarray(cam["position"], np.float64)
    x = (2.0 * np.asarray(px, np.float64) / W - 1.0) * th * (W / H) * depth
    y = -(2.0 * np.asarray(py, np.float64) / H - 1.0) * th * depth
    return np.stack([pos[0] + x, pos[1] + y, np.full_like(x, pos[2] - depth)], -1)


def project(pinv, vinv, pts, window=WINDOW):
    """pixel coordinates (n, 2) of world points under the camera of the two inverse matrices (4 x 4, float64)"""
    W, H = window
    p = np.concatenate([np.asarray(pts, np.float64), np.ones((len(pts), 1))], -1)
    clip = p @ np.linalg.inv(vinv).T @ np.linalg.inv(pinv).T
    ndc = clip[:, :2] / clip[:, 3:]
    return np.stack([(ndc[:, 0] + 1.0) * 0.5 * W, (1.0 - ndc[:, 1]) * 0.5 * H], -1)


def quad(corners_px, depth, albedo=(0.0, 0.0, 0.0), emission=EMISSION, window=WINDOW):
    """(mesh, the fp32 world corners): an emissive quad facing the camera whose corners show at the pixel coordinates (4, 2), in order
    around the quad"""
    c = np.asarray(corners_px, np.float64)
    pos = pixel_to_world(c[:, 0], c[:, 1], depth, window)
    mb = MeshBuilder()
    mb.add("quad", pos, np.tile([0.0, 0.0, 1.0], (4, 1)), None, [[0, 1, 2], [0, 2, 3]], Material(albedo, 0.0, 1.0, emission=emission))
    mesh = mb.build()
    return mesh, mesh.vertices[:4, :3].astype(np.float64)


def rect_corners(bounds=RECT_PX, rot_deg=0.0):
    """corner pixel coordinates of the rectangle, turned in the image plane about its centre (pixels are square, the plane is parallel to
    the film: the image of the turned rectangle is the turned image)"""
    x0, x1, y0, y1 = bounds
    c = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]])
    if rot_deg:
        m = c.mean(0)
        a = math.radians(rot_deg)
        r = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
        c = (c - m) @ r.T + m
    return c


def half_plane(depth, edge_px=EDGE_PX, window=WINDOW):
    """an emissive quad whose left edge shows at pixel column edge_px and which reaches three frame widths past the other three sides"""
    W, H = window
    return quad([[edge_px, -3.0 * H], [4.0 * W, -3.0 * H], [4.0 * W, 4.0 * H], [edge_px, 4.0 * H]], depth, window=window)


def constant_sky(c=SKY_C, w=64, h=32):
    return np.broadcast_to(np.asarray(c, np.float32), (h, w, 3)).copy()
