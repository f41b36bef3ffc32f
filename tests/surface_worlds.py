"""Worlds for the surface stage (hit_info) and for k_shade's table-size switches, shared by tests/test_surface_cpu.py, tests/test_surface.py
and tests/test_shade_tables.py.  Test infrastructure only."""
import math

import numpy as np

import ref_surface
from raytracer3_amd import scenes
from raytracer3_amd.assets import GEOMETRY_DTYPE, Material, Mesh, MeshBuilder
from support import rotation

F = np.float32
EYE = np.eye(4, dtype=F)
TEXTURE_SIZES = [(1, 1), (1, 7), (3, 5), (64, 64), (257, 2)]  # W x H
SOUP_TRIANGLES = [37, 400, 113, 64, 150, 1, 18]  # per geometry: all different, so a wrong first_prim or 3 * prim offset lands in a neighbour


def affine(m3, t=(0.0, 0.0, 0.0)):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = m3, t
    return m.astype(F)


def random_textures(rng, sizes=TEXTURE_SIZES):
    return [np.ascontiguousarray(rng.integers(0, 256, (h, w, 4), dtype=np.uint8)) for w, h in sizes]


def uv_pool(rng, n, size):
    """n texture coordinates for an axis of `size` texels: texel centres and edges (multiples of 0.5 / size), exactly 0, 1 and -0.0,
    negative values, values several periods out, the seam (x0 = size - 1, x1 wrapping to 0) and generic values"""
    half = rng.integers(-6 * size, 6 * size + 1, n) * (0.5 / size)  # centres (odd multiples) and edges (even multiples), |u| <= 3
    special = np.array([0.0, 1.0, -0.0, -1.0, 2.0, 1.0 - 0.25 / size, -0.25 / size, 3.0 - 0.25 / size, 0.5 / size, -0.5 / size, 1.0 - 0.5 / size])
    generic = rng.uniform(-5.0, 5.0, n)
    kind = rng.integers(0, 3, n)
    return np.where(kind == 0, half, np.where(kind == 1, special[rng.integers(0, len(special), n)], generic)).astype(F)


def soup_normals(rng, n):
    """(n, 3, 3) vertex normals: per triangle within asin(0.8) = 53 degrees of a common direction, so any blend is at least 0.6 long;
    every eighth triangle has one axis direction at all three vertices"""
    m = rng.normal(size=(n, 1, 3))
    m /= np.linalg.norm(m, axis=2, keepdims=True)
    r = rng.normal(size=(n, 3, 3))
    r *= rng.uniform(0.0, 0.8, (n, 3, 1)) / np.linalg.norm(r, axis=2, keepdims=True)
    v = m + r
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    k = np.arange(0, n, 8)
    v[k] = axes[rng.integers(0, 6, len(k))][:, None, :]
    return v


def surface_world(seed=1):
    """(mesh, instances): a triangle soup for hit_info only (it has to build, it is never ray traced).  Seven geometries of different
    sizes: one per texture of TEXTURE_SIZES, one untextured (index -1) and one whose texture index is past the textures, which reads as
    untextured; every material distinct, some emissive.  Placed under the identity, a pure rotation, a non-uniform scale of 0.3 .. 3 and
    a mirrored matrix; geometry 2 is placed twice more under two further matrices."""
    rng = np.random.default_rng(seed)
    textures = random_textures(rng)
    tex_index = [0, 1, 2, 3, 4, -1, len(textures) + 2]
    mb = MeshBuilder()
    for g, (n, tex) in enumerate(zip(SOUP_TRIANGLES, tex_index)):
        w, h = TEXTURE_SIZES[tex] if 0 <= tex < len(textures) else (16, 16)
        corner = rng.uniform(-1.0, 1.0, (n, 1, 3)) + [3.0 * g, 0.0, 0.0]
        pos = corner + rng.uniform(0.05, 0.3, (n, 3, 3)) * np.eye(3)  # three points off the corner along x, y, z: never degenerate
        uv = np.stack([uv_pool(rng, 3 * n, w), uv_pool(rng, 3 * n, h)], 1)
        mat = Material(tuple(rng.uniform(0.05, 1.0, 3)), float(g % 2), float(rng.uniform(0.05, 1.0)),
                       tuple(rng.uniform(0.1, 2.0, 3)) if g % 3 == 1 else (0.0, 0.0, 0.0), tex)
        mb.add(f"soup{g}", pos.reshape(-1, 3), soup_normals(rng, n).reshape(-1, 3), uv, np.arange(3 * n).reshape(-1, 3), mat)
    mesh = mb.build()
    mesh.textures = textures
    ng = len(mesh.geometries)
    mirror = np.diag([-1.0, 1.0, 1.0]) @ rotation(rng) @ np.diag([0.7, 1.3, 2.1])
    assert np.linalg.det(mirror) < 0
    instances = [
        (0, ng, EYE),                                                                     # the identity shortcut
        (0, ng, affine(rotation(rng), (0.0, 5.0, 0.0))),                                  # a pure rotation
        (0, ng, affine(rotation(rng) @ np.diag([0.3, 1.0, 3.0]), (0.0, 10.0, 0.0))),      # non-uniform scale, kappa = 10
        (0, ng, affine(mirror, (0.0, 15.0, 0.0))),                                        # negative determinant
        (2, 1, affine(rotation(rng) @ np.diag([3.0, 0.3, 0.5]), (0.0, 20.0, 0.0))),       # one geometry twice more,
        (2, 1, affine(np.diag([1.0, -2.0, 0.4]) @ rotation(rng), (0.0, 25.0, 0.0))),      # under different matrices
    ]
    return mesh, instances


def surface_hits(mesh, instances, seed=2, per_entry=40, interior=6):
    """(prim uint32, bu, bv fp32): for every flattened entry its first and last triangle and `per_entry` random ones; on each the three
    corners (bu = bv = 0 makes the uv exactly vertex 0's; (1, 0) makes b0 exactly 0), the edge midpoints and `interior` random points"""
    rng = np.random.default_rng(seed)
    _, _, first, counts, _ = ref_surface.flatten(mesh, instances)
    prim, bary = [], []
    fixed = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0], [0, 0.5], [0.5, 0.5]], np.float64)
    for f, c in zip(first, counts):
        if c == 0:
            continue
        tris = np.unique(np.concatenate([[0, c - 1], rng.integers(0, c, per_entry)])) + f
        for t in tris:
            r = rng.random((interior, 2))
            r = np.where(r.sum(1, keepdims=True) > 1.0, 1.0 - r, r) * 0.999  # folded into the triangle, off the far edge
            bary.append(np.concatenate([fixed, r]))
            prim.append(np.full(len(fixed) + interior, t))
    prim, bary = np.concatenate(prim).astype(np.uint32), np.concatenate(bary).astype(F)
    assert (bary[:, 0].astype(np.float64) + bary[:, 1] <= 1.0).all()
    return prim, bary[:, 0].copy(), bary[:, 1].copy()


def hit_rows(prim, bu, bv):
    """the hits as rows of three 32-bit words {prim, bu, bv}: the input of self-test op 29"""
    rows = np.zeros((len(prim), 3), np.uint32)
    rows[:, 0] = prim
    rows[:, 1], rows[:, 2] = np.asarray(bu, F).view(np.uint32), np.asarray(bv, F).view(np.uint32)
    return rows


# ------------------------------------------------------------------------------------------------ many geometries
def _hash(k):
    k = (k ^ 61) ^ (k >> 16)
    k = (k * 9) & 0xFFFFFFFF
    k ^= k >> 4
    k = (k * 0x27D4EB2D) & 0xFFFFFFFF
    return k ^ (k >> 15)


def many_geometries(n, seed=3):
    """(mesh, instances, camera): a floor quad and n - 1 small boxes on a grid, each box its own geometry under its own instance (a
    rotation about y, a non-uniform scale, its place on the grid), so the flattened table has exactly n entries.  The material is a
    function of the geometry's index: base colour from a hash, roughness in [0.2, 1], metalness 0 or 1, every 16th box emissive, every
    8th textured (two small textures in turn).  The camera looks down on the grid from one side and sees most boxes."""
    rng = np.random.default_rng(seed)
    side = int(math.ceil(math.sqrt(n - 1)))
    half = 0.5 * side
    mb = MeshBuilder()
    floor = scenes._grid([-half - 1.0, 0.0, half + 1.0], [side + 2.0, 0, 0], [0, 0, -(side + 2.0)], 1, 1)
    mb.add("floor", *floor, Material((0.6, 0.6, 0.55), 0.0, 0.9))
    instances = [(0, 1, EYE)]
    for k in range(1, n):
        h = _hash(k)
        color = tuple(0.15 + 0.8 * ((h >> s) & 0xFF) / 255.0 for s in (0, 8, 16))
        mat = Material(color, float((h >> 24) & 1), 0.2 + 0.8 * ((h >> 25) & 0x3F) / 63.0,
                       (0.5, 0.4, 0.3) if k % 16 == 0 else (0.0, 0.0, 0.0), (k // 8) % 2 if k % 8 == 0 else -1)
        scenes._box(mb, f"box{k}", [-0.5, 0.0, -0.5], [0.5, 1.0, 0.5], mat)
        a = rng.uniform(0.0, 2.0 * math.pi)
        rot = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        cx, cz = (k - 1) % side, (k - 1) // side
        instances.append((k, 1, affine(rot @ np.diag(rng.uniform(0.25, 0.7, 3)), (cx + 0.5 - half, 0.0, cz + 0.5 - half))))
    mesh = mb.build()
    mesh.textures = random_textures(np.random.default_rng(seed + 1), [(8, 8), (5, 3)])
    assert len(mesh.geometries) == n and sum(c for _, c, _ in instances) == n
    camera = dict(position=(0.0, 0.9 * side, 0.6 * side), direction=(0.0, -1.6, -1.0), fov_deg=50.0)
    return mesh, instances, camera


def with_empty_geometry(mesh, instances, at=None):
    """the same world plus one geometry of zero triangles placed by one more instance: appended (at = None) or inserted at position
    `at` of the instance list, which shifts the table index of every later entry.  No primitive id changes."""
    g = np.zeros(1, GEOMETRY_DTYPE)
    g["base_color"], g["roughness"] = (0.9, 0.1, 0.9, 1.0), 0.37
    g["base_color_texture_index"] = -1
    out = Mesh(mesh.vertices, mesh.indices, np.concatenate([mesh.geometries, g]), np.concatenate([mesh.prim_counts, np.zeros(1, np.uint32)]).astype(np.uint32),
               list(mesh.names) + ["empty"], list(mesh.textures))
    placed = (len(mesh.geometries), 1, affine(np.diag([1.0, 2.0, 0.5]), (0.3, 0.2, 0.1)))
    inst = list(instances)
    inst.insert(len(inst) if at is None else at, placed)
    return out, inst


def banded_sky(rows, width=8):
    """an equirect sky of `rows` rows: a dim gradient and one bright group of rows above the horizon, so the marginal distribution over
    rows decides where the light samples go"""
    v = (np.arange(rows) + 0.5) / rows
    sky = np.zeros((rows, width, 3), F)
    sky[:] = (0.15 + 0.25 * np.clip(np.cos(np.pi * v), 0.0, 1.0))[:, None, None] * np.array([0.8, 0.9, 1.0])
    a = rows // 6
    sky[a:a + max(rows // 48, 2)] += np.array([30.0, 27.0, 21.0], F)
    sky[:, width // 2] *= 1.5
    return sky
