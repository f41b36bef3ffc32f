"""Worlds of the punctual-light tests, shared by the fixture generator, the CPU tests and the GPU tests."""
import numpy as np

import integrator_worlds as IW
from raytracer3_amd import assets
from raytracer3_amd.assets import LIGHT_DIRECTIONAL, LIGHT_POINT, LIGHT_SPOT, Material, MeshBuilder, make_light
from raytracer3_amd import scenes

F_NEE_SKY, F_SPECULAR, F_FACEFORWARD, F_NEE_EMISSIVE, F_NEE_PUNCTUAL = 1, 4, 8, 32, 64  # RT3_F_* of include/rt3.h


def lights(*records):
    return assets.lights_array(records)


# ---------------------------------------------------------------------------------------------------------------- open room with lights
# No triangle is nearer to the point or spot light than 1 % of its distance to any lit point: the room is 8 x 8 x 4, so no lit point is
# further than 12 from a light inside it, and the nearest surfaces (the panel at y = 3.5, the block's top at y = 1.2) are more than
# 0.5 away.  The kernels' shadow range end d (1 - 2^-10) and the reference's d then see the same occluders.
ROOM_POINT = lights(make_light(LIGHT_POINT, (30.0, 26.0, 20.0), position=(1.0, 2.0, 1.5)))
ROOM_SPOT_SUN = lights(
    make_light(LIGHT_SPOT, (60.0, 50.0, 40.0), position=(2.0, 3.0, 2.0), direction=(-1.0, -1.0, -1.0), range=12.0, inner_cone=0.3, outer_cone=0.6),
    make_light(LIGHT_DIRECTIONAL, (1.5, 1.4, 1.2), direction=(-0.3, -1.0, -0.4)),
)
# The cases of tests/golden/punctual_ref.npz: name -> (reference flags, bounces, specular material set, lights, reference samples per pixel,
# seed, frames of IW.FRAME_SPP samples of the code under test).  The kernels' flags are the reference's | F_NEE_PUNCTUAL.  The reference adds
# every light at every vertex without noise; the kernels pick one entry per vertex, so they render more frames to get under half of the
# fixture's standard error.
CASES = {
    "point_b3": (F_FACEFORWARD, 3, False, ROOM_POINT, 4096, 201, 16),
    "spot_sun_b4": (F_NEE_SKY | F_FACEFORWARD | F_SPECULAR, 4, True, ROOM_SPOT_SUN, 4096, 202, 32),
}


def room(name):
    """(mesh with its lights, sky or None) of a case"""
    flags, _, specular, lts, _, _, _ = CASES[name]
    mesh = IW.open_room(specular)
    mesh.lights = lts.copy()
    return mesh, (IW.room_sky() if flags & F_NEE_SKY else None)


# ---------------------------------------------------------------------------------------------------------------- floor under a light
FLOOR_CAMERA = dict(position=(0.0, 2.4, 0.8), direction=(0.0, -1.0, -0.3), fov_deg=70.0)
FLOOR_ALBEDO = (0.8, 0.6, 0.4)
FLOOR_LIGHTS = {
    "point": make_light(LIGHT_POINT, (10.0, 8.0, 6.0), position=(0.4, 1.5, -0.3), range=2.5),
    "spot": make_light(LIGHT_SPOT, (10.0, 8.0, 6.0), position=(0.4, 1.5, -0.3), direction=(0.2, -1.0, 0.1), inner_cone=0.2, outer_cone=0.5),
    "directional": make_light(LIGHT_DIRECTIONAL, (2.0, 1.5, 1.0), direction=(0.3, -1.0, 0.2)),
}
OCCLUDER = ((-0.2, 0.6), 0.8, (-0.7, 0.1))  # x range, height, z range of the quad between the lights and the floor


def _quad(mb, name, x, y, z, mat, uv=False):
    """a horizontal quad at height y facing up (normal (0, 1, 0)), two triangles"""
    pos, nrm, uvs, tris = scenes._grid([x[0], y, z[1]], [x[1] - x[0], 0, 0], [0, 0, z[0] - z[1]], 1, 1)
    mb.add(name, pos, nrm, uvs if uv else None, tris, mat)


def floor_world(occluder=False, ceiling=None, cutout=False):
    """a 6 x 6 floor at y = 0 with normal (0, 1, 0); optionally the occluder quad, a ceiling quad at height `ceiling`, or the occluder as a
    MASK cutout with a 2 x 2 checker alpha texture"""
    mb = MeshBuilder()
    _quad(mb, "floor", (-3.0, 3.0), 0.0, (-3.0, 3.0), Material(FLOOR_ALBEDO, 0.0, 1.0))
    if occluder or cutout:
        mat = Material((0.5, 0.5, 0.5), 0.0, 1.0, texture_offset=0, alpha_cutoff=0.5) if cutout else Material((0.5, 0.5, 0.5), 0.0, 1.0)
        _quad(mb, "occluder", OCCLUDER[0], OCCLUDER[1], OCCLUDER[2], mat, uv=cutout)
    if ceiling is not None:
        r = 30.0 + 0.5 * ceiling  # wide enough for every slanted light direction of FLOOR_LIGHTS to meet it from any floor point in view
        _quad(mb, "ceiling", (-r, r), ceiling, (-r, r), Material((0.5, 0.5, 0.5), 0.0, 1.0))
    mesh = mb.build()
    if cutout:
        tex = np.full((2, 2, 4), 255, np.uint8)
        tex[0, 1, 3] = tex[1, 0, 3] = 0
        mesh.textures = [tex]
    return mesh


def shadow_rect(light, y=None):
    """the occluder's shadow on the floor (y = 0) as ((x0, x1), (z0, z1)): a rectangle, by central (point, spot) or parallel projection"""
    (x0, x1), h, (z0, z1) = OCCLUDER
    if int(light["type"]) == LIGHT_DIRECTIONAL:
        d = np.asarray(light["direction"], np.float32).astype(np.float64)
        s = h / -d[1]
        return (x0 + s * d[0], x1 + s * d[0]), (z0 + s * d[2], z1 + s * d[2])
    P = np.asarray(light["position"], np.float32).astype(np.float64)
    k = P[1] / (P[1] - h)
    return (P[0] + k * (x0 - P[0]), P[0] + k * (x1 - P[0])), (P[2] + k * (z0 - P[2]), P[2] + k * (z1 - P[2]))
