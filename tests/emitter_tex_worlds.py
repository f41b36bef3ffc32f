"""Worlds for textured emitters, shared by tests/test_emitter_tex_cpu.py and tests/test_emitter_tex.py.  Test
infrastructure only."""
import dataclasses

import numpy as np

import ref_surface as RS
import surface_worlds as SW
from raytracer3_amd import scenes
from raytracer3_amd.assets import Material, MeshBuilder
from support import constant

F = np.float32
ALBEDO = 0.64  # tests/test_nee_emissive.py's floor: its square root survives the G-buffer's 8-bit encoding exactly
EMISSION = 1.0
HALF = np.ascontiguousarray(np.array([[[255, 255, 255, 255], [0, 0, 0, 255]]], np.uint8))  # 2 x 1: [255, 0]
LADDER_EDGES = (0.8, 2.0, 62.5, 64.0, 100.0)  # longest uv edge in texels of the 8 x 8 texture: L = 1, 2, 63, 64 and the cap
LADDER_L = (1, 2, 63, 64, 64)


def with_emissive_texture(mesh, name, textures, index=0):
    """`mesh` with geometry `name` naming emissive texture `index` of `textures`"""
    t = mesh.material_textures.copy()
    t["emissive_texture"][mesh.names.index(name)] = index
    return dataclasses.replace(mesh, geometries=mesh.geometries.copy(), names=list(mesh.names), textures=list(textures), material_textures=t)


def lit_cornell(texture):
    """scenes.cornell() whose panel carries `texture` as its emissive map"""
    return with_emissive_texture(scenes.cornell(), "panel", [texture])


def soup(seed=41):
    """(mesh, instances): emitters for the table, the lookup and the masses.  Geometries: two with random 8 x 8 and 5 x 3 emissive textures
    and uvs in [-2.5, 3], one emitter without texture, one whose emissive index is not uploaded, one textured geometry without emission, a
    ladder of triangles whose longest uv edge is LADDER_EDGES texels, and a masked textured emitter (left out).  Instances: identity, a
    rotation, a mirror with a non-uniform scale."""
    rng = np.random.default_rng(seed)
    textures = SW.random_textures(rng, [(8, 8), (5, 3)])
    mb = MeshBuilder()

    def tris(n, x0):
        p = rng.uniform(-0.5, 0.5, (n, 3, 3)) + [x0, 0.0, 0.0]
        return p.reshape(-1, 3), np.tile([0.0, 0.0, 1.0], (3 * n, 1)), np.arange(3 * n).reshape(-1, 3)

    def add(name, n, x0, uv, **mat):
        p, nn, idx = tris(n, x0)
        mb.add(name, p, nn, uv, idx, Material((0.5, 0.5, 0.5), **mat))

    em = lambda: tuple(rng.uniform(0.2, 2.0, 3))  # noqa: E731
    add("tex8", 12, 0.0, rng.uniform(-2.5, 3.0, (36, 2)), emission=em(), emissive_texture=0)
    add("tex53", 9, 2.0, rng.uniform(-2.5, 3.0, (27, 2)), emission=em(), emissive_texture=1)
    add("plain", 5, 4.0, rng.uniform(0.0, 1.0, (15, 2)), emission=em())
    add("missing", 4, 6.0, rng.uniform(0.0, 1.0, (12, 2)), emission=em(), emissive_texture=7)
    add("dark", 6, 8.0, rng.uniform(0.0, 1.0, (18, 2)), emissive_texture=0)
    lad = np.zeros((len(LADDER_EDGES), 3, 2))
    for k, e in enumerate(LADDER_EDGES):
        o = rng.uniform(-1.0, 1.0, 2)
        lad[k] = [o, o + [e / 8.0, 0.0], o + [0.3 * e / 8.0, -0.5 * e / 8.0]]
    add("ladder", len(LADDER_EDGES), 10.0, lad.reshape(-1, 2), emission=em(), emissive_texture=0)
    add("masked", 3, 12.0, rng.uniform(0.0, 1.0, (9, 2)), emission=em(), emissive_texture=0, alpha_cutoff=0.5)
    mesh = mb.build()
    mesh.textures = textures
    ng = len(mesh.geometries)
    mirror = np.diag([-1.0, 1.0, 1.0]) @ SW.rotation(rng) @ np.diag([0.7, 1.3, 2.1])
    instances = [(0, ng, SW.EYE), (0, ng, SW.affine(SW.rotation(rng), (0.0, 5.0, 0.0))), (0, ng, SW.affine(mirror, (0.0, 10.0, 0.0)))]
    return mesh, instances


def entries(mesh, instances, prim):
    """per flattened primitive of `prim`: (geometry, instance, vertex indices (n, 3))"""
    geom, inst, first, counts, _ = RS.flatten(mesh, instances)
    k = np.searchsorted(first, np.asarray(prim, np.int64), side="right") - 1
    assert (counts[k] > 0).all()
    g = geom[k]
    tri = np.asarray(prim, np.int64) - first[k]
    io, vo = mesh.geometries["index_offset"][g].astype(np.int64), mesh.geometries["vertex_offset"][g].astype(np.int64)
    idx = np.stack([mesh.indices[io + 3 * tri + c].astype(np.int64) + vo for c in range(3)], 1)
    return g, inst[k], idx


def expected_side_array(mesh, instances, prim):
    """(uv (n, 3, 2) float32, texture (n,) int32) the side array must hold for the emitters `prim`"""
    g, _, idx = entries(mesh, instances, prim)
    tex = mesh.material_textures["emissive_texture"][g].astype(np.int32)
    tex = np.where((tex >= 0) & (tex < len(mesh.textures)), tex, -1).astype(np.int32)
    uv = mesh.vertices[idx][:, :, 6:8].astype(F)
    uv[tex < 0] = 0.0
    return uv, tex


def floor_and_striped_light():
    """tests/test_nee_emissive.py's floor under the unit square light at height 1, the light carrying HALF: its u runs along world x from
    -0.5 to 0.5 and its v along z, so the radiance across x is 12 e profile(x + 0.5)"""
    mb = MeshBuilder()
    mb.add("floor", *scenes._grid([-3, 0, -3], [0, 0, 6], [6, 0, 0], 4, 4), Material((ALBEDO,) * 3))
    mb.add("light", *scenes._grid([-0.5, 1, -0.5], [1, 0, 0], [0, 0, 1], 1, 1), Material((0.5,) * 3, emission=(EMISSION,) * 3, emissive_texture=0))
    mesh = mb.build()
    mesh.textures = [HALF]
    return mesh


def profile(u):
    """the bilinear profile of HALF across u under repeat addressing: texel centres at u = 0.25 (value 1) and 0.75 (value 0), linear
    between them and across the seam"""
    x = np.mod(np.asarray(u, np.float64), 1.0)
    return np.where(x < 0.25, 0.5 + 2.0 * x, np.where(x < 0.75, 1.5 - 2.0 * x, 2.0 * x - 1.5))


def constant_maps():
    return [constant((255, 255, 255, 255), 1, 1), constant((255, 255, 255, 255), 4, 4)]
