"""Worlds of the feature-combination tests (tests/test_combined_cpu.py, tests/test_combined.py, tests/golden/gen_combined_ref.py;
DESIGN.md section 2): one room in which material textures, a punctual light, an alpha cutout and a thin lens all matter to the same
pixels, and its variants with a feature taken away.

The room is lens_worlds.material_room()'s closed 4 x 3 x 4 box seen from inside (every quad's cells at most 3/4 as long along v as
along u, the condition under which ref_materials vouches for a tangent), with
  * normal maps and metallic-roughness maps on the floor, the back and left wall and the leaning slab, an emissive map on the box;
  * a spot light under the ceiling that shines down on the floor, the box and the lower part of the walls;
  * a screen: one quad that leans between the light and the floor, facing the camera.  As a cutout its base-colour texture is a 4 x 4
    checker of alpha 0 / 255 and its cutoff 0.5, so that half of its cells let the light (and the view) through; the light throws the
    checker on the floor and up the back wall.  Without the cutout the same quad is an opaque occluder.
Light leaves the closed box only above a normal-mapped wall's tilted shading normal (the walls are single quads); a dim constant sky
is behind them, as in lens_worlds."""
import numpy as np

import integrator_worlds as IW
import lens_worlds as LW
import material_worlds as MW
import surface_worlds as SW
from raytracer3_amd import scenes
from raytracer3_amd.assets import LIGHT_SPOT, Material, MeshBuilder, lights_array, make_light, no_material_textures

F_NEE_SKY, F_SPECULAR, F_FACEFORWARD, F_NEE_EMISSIVE, F_NEE_PUNCTUAL = 1, 4, 8, 32, 64  # RT3_F_* of include/rt3.h
REF_FULL = F_NEE_SKY | F_FACEFORWARD | F_SPECULAR  # the reference's share of the kernels' FULL (blue noise only reorders the kernels' samples)
WINDOW = IW.WINDOW_ROOM
CAMERA = dict(position=(0.0, 1.5, 1.9), direction=(0.0, -0.25, -1.0), fov_deg=70.0)
SKY_C = LW.MATERIAL_SKY_C
LENS = (0.05, 2.7, 1.0)  # focused on the screen; the eye is 0.1 in front of the wall behind it, the tilted disk reaches 0.012 towards it
# No triangle is nearer to the light than 1 % of its distance to any lit point (the panel, 0.45 above it, is the nearest; no point of the
# room is further than 6): the kernels' shadow range end d (1 - 2^-10) and the reference's d see the same occluders.
SPOT = lights_array([make_light(LIGHT_SPOT, (30.0, 26.0, 20.0), position=(0.8, 2.5, -0.5), direction=(0.0, -1.0, -0.1), range=9.0, inner_cone=0.5, outer_cone=1.0)])
SCREEN = ([0.2, 0.9, -0.2], [1.2, 0.0, 0.0], [0.0, 0.7, -1.0])  # origin, u edge, v edge: it faces up and towards the camera
SCREEN_CUTOFF = 0.5


def checker(cells=4, alpha=(0, 255)):
    """cells x cells texels, white, alpha[(x + y) % 2]"""
    tex = np.full((cells, cells, 4), 255, np.uint8)
    y, x = np.mgrid[0:cells, 0:cells]
    tex[..., 3] = np.asarray(alpha, np.uint8)[(x + y) % 2]
    return tex


def constant_alpha(a, cells=4):
    return checker(cells, (a, a))


def _box(mb, name, lo, hi, mat):
    """scenes._box without its bottom, every face 1 x 2 cells (the cell condition of the module docstring)"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    e = hi - lo
    faces = [(lo + [0, 0, e[2]], [e[0], 0, 0], [0, e[1], 0]), (lo + [e[0], 0, 0], [-e[0], 0, 0], [0, e[1], 0]),
             (lo + [e[0], 0, e[2]], [0, 0, -e[2]], [0, e[1], 0]), (lo, [0, 0, e[2]], [0, e[1], 0]), (lo + [0, e[1], e[2]], [e[0], 0, 0], [0, 0, -e[2]])]
    P, N, U, T, off = [], [], [], [], 0
    for o, du, dv in faces:
        p, nn, uv, t = scenes._grid(o, du, dv, 1, 2)
        P.append(p), N.append(nn), U.append(uv), T.append(t + off)
        off += len(p)
    mb.add(name, np.concatenate(P), np.concatenate(N), np.concatenate(U), np.concatenate(T), mat)


def room(textures=True, cutout=False, lights=True, screen_texture=None, screen=True):
    """the mesh.  `textures`: the material textures; `cutout`: the screen is a MASK cutout with the checker (or `screen_texture`) as its
    base-colour texture; `lights`: mesh.lights holds the spot light; `screen` = False leaves the quad out altogether."""
    q = scenes._grid
    parts = {
        "floor": q([-2, 0, 2], [4, 0, 0], [0, 0, -4], 2, 4), "ceiling": q([-2, 3, -2], [4, 0, 0], [0, 0, 4], 2, 4),
        "back": q([-2, 0, -2], [4, 0, 0], [0, 3, 0], 2, 2), "front": q([2, 0, 2], [-4, 0, 0], [0, 3, 0], 2, 2),
        "left": q([-2, 0, 2], [0, 0, -4], [0, 3, 0], 2, 2), "right": q([2, 0, -2], [0, 0, 4], [0, 3, 0], 2, 2),
        "panel": q([-0.8, 2.95, -0.8], [1.6, 0, 0], [0, 0, 1.6], 2, 4), "slab": q([-1.2, 0.0, -0.2], [1.6, 0, 0], [0, 0.8, -0.9], 2, 4),
    }
    rng = np.random.default_rng(51)
    mb = MeshBuilder()
    for name, part in parts.items():
        emission = {"panel": (0.25, 0.23, 0.2), "ceiling": LW.MATERIAL_CEILING_EMISSION}.get(name, (0.0, 0.0, 0.0))
        mb.add(name, *part, Material(tuple(rng.uniform(0.4, 0.9, 3)), float(rng.uniform(0.2, 1.0)), float(rng.uniform(0.3, 1.0)), emission))
    _box(mb, "box", [1.0, 0.0, -1.6], [1.7, 0.6, -0.9], Material((0.2, 0.5, 0.8), 0.5, 0.7, (0.3, 0.1, 0.05)))
    tex = []
    if textures:
        tex = MW.colour_textures(rng, [(8, 8), (5, 3)]) + MW.normal_textures(rng, [(16, 16), (7, 5), (1, 1)])
    if screen:
        mat = Material((0.7, 0.7, 0.6), 0.0, 0.8)
        if cutout:
            mat = Material((0.7, 0.7, 0.6), 0.0, 0.8, texture_offset=len(tex), alpha_cutoff=SCREEN_CUTOFF)
            tex = tex + [checker() if screen_texture is None else screen_texture]
        mb.add("screen", *q(*SCREEN, 1, 2), mat)
    mesh = mb.build()
    names = mesh.names
    t = no_material_textures(len(names))
    if textures:
        nm = {names.index("floor"): 2, names.index("back"): 3, names.index("left"): 2, names.index("slab"): 3}
        mr = {names.index("floor"): 0, names.index("back"): 1, names.index("slab"): 0, names.index("right"): 1}
        t = MW.table(len(names), normal_texture=nm, metallic_roughness_texture=mr, emissive_texture={names.index("box"): 1},
                     normal_scale={names.index("floor"): 1.5, names.index("back"): 0.5})
    mesh = MW.with_tables(mesh, material_textures=t, textures=tex)
    if lights:
        mesh.lights = SPOT.copy()
    return mesh


def sky():
    return LW.constant_sky(SKY_C)


# The cases of tests/golden/combined_ref.npz: name -> (reference flags, bounces, what the world and the camera have, the flags the kernels
# add to their FULL, reference samples per pixel, seed, frames of IW.FRAME_SPP samples of the code under test).
# The reference's sample count is the smallest multiple of ref_pathtrace.CHUNK_SPP at which the fixture meets the sizing condition of
# test_fixture_is_sized_and_arrays_only (found by  python tests/golden/gen_combined_ref.py --find-spp); the frames are what the kernels
# need to get under half of the fixture's standard error.
# "cutout_textures" is the exception.  The three channels of a block share their paths, so one block whose fixture mean is off by chance
# is 3 of the 18 block-channels at once.  At the smallest sized count, 1088, and again at 1856 (the condition with two standard errors of
# margin), the fixture's darkest block lay 1.5 of its standard errors above an independent 4096-sample render of the same tracer (seed 9001)
# and check_against_fixture's power condition (a frame scaled by 1.02 is rejected in 90 % of the block-channels) came to 83 % on frames
# whose own error was under a quarter of the fixture's, largest |z| 2.6.  The case is rendered to the smallest count at which *every*
# block-channel has three standard errors of margin (--find-spp --margin 3 --share 1), 3392: a narrower band, never a wider one.
CASES = {
    "lights_textures": (REF_FULL, 3, dict(lens=False, lights=True, textures=True, cutout=False), F_NEE_PUNCTUAL, 704, 301, 16),
    "lights_textures_emitters": (REF_FULL, 3, dict(lens=False, lights=True, textures=True, cutout=False), F_NEE_PUNCTUAL | F_NEE_EMISSIVE, 704, 302, 16),
    "lens_lights": (REF_FULL, 3, dict(lens=True, lights=True, textures=False, cutout=False), F_NEE_PUNCTUAL, 576, 303, 16),
    "lens_lights_textures_cutout": (REF_FULL, 3, dict(lens=True, lights=True, textures=True, cutout=True), F_NEE_PUNCTUAL | F_NEE_EMISSIVE, 768, 304, 16),
    "cutout_textures": (REF_FULL, 3, dict(lens=False, lights=False, textures=True, cutout=True), 0, 3392, 305, 16),
}


def world(name):
    """(mesh, lens or None) of a case"""
    has = CASES[name][2]
    return room(has["textures"], has["cutout"], has["lights"]), (LENS if has["lens"] else None)


def padded(mesh, n, at=None):
    """(mesh, instances): the same triangles behind n flattened geometries (material_worlds.padded: every geometry once under the
    identity, then empty ones).  With `at`, one of the empty entries is placed by an instance of its own at position `at` of the table
    instead of at its end (surface_worlds.with_empty_geometry's idea, keeping the cutoffs and the material-texture table): the index of
    every later entry shifts by one and no primitive id changes."""
    out, inst = MW.padded(mesh, n)
    out.lights = mesh.lights.copy()
    if at is None:
        return out, inst
    last = n - 1
    assert int(out.prim_counts[last]) == 0 and 0 < at < len(mesh.geometries)
    return out, [(0, at, SW.EYE), (last, 1, SW.affine(np.diag([1.0, 2.0, 0.5]), (0.3, 0.2, 0.1))), (at, last - at, SW.EYE)]
