"""The oracle's tree traversal pinned to brute force away from the origin, at other scales, on adversarial rays.

The parity tests compare the GPU with the oracle, and the oracle builds the same boxes and runs the same slab test, so a box test
that culls a triangle the triangle test would accept shows up on both sides.  Only brute force -- the same fp32 triangle test over
every triangle, no tree -- catches it.  Here every scene is also moved far from the origin (±1e3, ±1e4, 3e4, mixed per axis) and
scaled by 1e-3 and 1e3, and traced with random rays, rays aimed at vertices and at shared-edge midpoints, axis-parallel rays whose
origins lie on vertex coordinates (so on leaf-box planes) with exact +0.0 / -0.0 direction components, and rays whose tmin or tmax is
exactly a known hit's t.

Pass criterion (for every node layout, closest hit and any hit):
1. A ray is *disputed* when the fp32 and the fp64 brute force choose different primitives.  For an undisputed ray the tree equals the
   fp32 brute force bit for bit in prim, t, u and v, and any hit equals (brute prim != MISS).
2. For a disputed ray the tree's primitive is one of the two, and disputed rays stay below DISPUTED_MAX of each batch (per family).
3. The fp32 triangle test is itself inexact when a triangle is tiny next to its distance from the ray origin (fp32 and fp64
   disagree 1 % inside the edges from size / distance 2^-9 on).  That is not a traversal fault and is not changed here: test_fp32_triangle_test_exact_above_ratio
   characterises it, DESIGN.md records the threshold, and the ray families here keep origins within a few scene sizes.
"""
import zlib

import numpy as np
import pytest

import orc
from raytracer3_amd import assets, scenes

# Ceiling on disputed rays per family.  Rays aimed at vertices and shared edges, and rays whose tmin is a hit's own fp32 t, land on
# ties (several triangles at the same t within rounding), where the fp64 test legitimately picks another primitive.
DISPUTED_MAX = {"random": 0.01, "axis": 0.15, "edge": 0.45, "vertex": 0.9, "interval": 0.9}
SOUP_KINDS = ("cloud", "slivers", "grid")
SCENES = ("cornell", "atrium") + SOUP_KINDS
# (scale, offset): at the origin, far from it with mixed signs per axis, and scaled
PLACEMENTS = (
    (1.0, (0.0, 0.0, 0.0)),
    (1.0, (1e3, -1e3, 1e3)),
    (1.0, (-1e4, 1e4, -1e4)),
    (1.0, (1e4, 1e4, 1e4)),
    (1.0, (3e4, -3e4, 3e4)),
    (1e-3, (0.0, 0.0, 0.0)),
    (1e3, (0.0, 0.0, 0.0)),
)
# (leaf_size, node_width, quantized, collapse): binary and four-wide x quantisation 0/1/2, leaf sizes, both collapses
LAYOUTS = (
    (1, 2, 0, 2), (4, 2, 0, 2),
    (1, 4, 0, 2), (2, 4, 0, 0), (8, 4, 0, 2),
    (2, 4, 1, 2), (1, 4, 1, 0), (4, 4, 1, 2),
    (2, 4, 2, 2), (1, 4, 2, 2), (8, 4, 2, 0),
)


def soup(kind, n=1500, seed=7):
    """'cloud' = small random triangles, 'slivers' = long thin ones, 'grid' = a planar lattice of unit squares split on the diagonal
    (every triangle coplanar, edges shared within and across cells: ties in t everywhere)"""
    rng = np.random.default_rng(seed)
    if kind == "grid":
        side = int(np.ceil(np.sqrt(n / 2)))
        ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2).astype(np.float32)
        b = np.concatenate([ij, np.zeros((len(ij), 1), np.float32)], 1) - [side / 2, side / 2, 0]
        x, y = np.float32([1, 0, 0]), np.float32([0, 1, 0])
        v = np.concatenate([np.stack([b, b + x, b + y], 1), np.stack([b + x + y, b + y, b + x], 1)])
    elif kind == "slivers":
        c = rng.uniform(-4, 4, (n, 1, 3))
        d = rng.normal(size=(n, 1, 3)) * [8.0, 0.05, 0.05]
        v = c + np.concatenate([np.zeros((n, 1, 3)), d, rng.normal(size=(n, 1, 3)) * 0.05], 1)
    else:
        c = rng.uniform(-4, 4, (n, 1, 3))
        v = c + rng.normal(size=(n, 3, 3)) * 0.2
    verts = np.asarray(v, np.float32).reshape(-1, 3)
    mb = assets.MeshBuilder()
    mb.add(kind, verts, np.tile([0, 0, 1], (len(verts), 1)), None, np.arange(len(verts), dtype=np.uint32).reshape(-1, 3), assets.Material())
    return mb.build()


_BASE = {}


def base_mesh(name):
    if name not in _BASE:
        _BASE[name] = scenes.cornell() if name == "cornell" else scenes.atrium(0.2) if name == "atrium" else soup(name)
    return _BASE[name]


def placed(mesh, scale, offset):
    """the mesh with every position p replaced by fp32(p * scale + offset)"""
    v = mesh.vertices.copy()
    v[:, :3] = (v[:, :3].astype(np.float64) * scale + np.asarray(offset, np.float64)).astype(np.float32)
    return assets.Mesh(v, mesh.indices, mesh.geometries, mesh.prim_counts, list(mesh.names), list(mesh.textures))


def _pack(o, d, tmin, tmax):
    n = len(o)
    return np.ascontiguousarray(np.concatenate([np.asarray(o, np.float32).T, np.asarray(d, np.float32).T,
                                                np.broadcast_to(np.float32(tmin), (1, n)), np.broadcast_to(np.float32(tmax), (1, n))]), np.float32)


def _unit(d):
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def ray_families(mesh, n=1500, seed=0):
    """{family: (8, m) float32 rays} in the mesh's own coordinates; origins stay within about one scene size of the scene's box"""
    rng = np.random.default_rng(seed)
    tri = mesh.triangle_positions().astype(np.float32)
    verts = np.unique(tri.reshape(-1, 3), axis=0)
    lo, hi = tri.reshape(-1, 3).min(0).astype(np.float64), tri.reshape(-1, 3).max(0).astype(np.float64)
    ext = float((hi - lo).max())
    ctr = (lo + hi) / 2

    def origins(m):
        return (ctr + rng.uniform(-0.75, 0.75, (m, 3)) * np.maximum(hi - lo, 0.2 * ext)).astype(np.float32)

    out = {}
    o = origins(n)
    out["random"] = _pack(o, _unit(rng.normal(size=(n, 3))), 0.0, 1e30)
    o = origins(n)
    tgt = verts[rng.integers(0, len(verts), n)]
    out["vertex"] = _pack(o, _unit(tgt.astype(np.float64) - o), 0.0, 1e30)
    er, _ = orc.shared_edge_rays(mesh, h=0.02 * ext, seed=seed, limit=n // 2)
    er[6] = 0.0
    er[7] = 1e30
    out["edge"] = er
    # axis-parallel: the two transverse coordinates are a vertex's (leaf-box planes); the direction's zero components are +0.0 or
    # -0.0; the origin starts outside the scene's box or at a random place inside it
    v = verts[rng.integers(0, len(verts), n)].copy()
    ax = rng.integers(0, 3, n)
    sgn = rng.choice([-1.0, 1.0], n)
    zeros = np.where(rng.random((n, 3)) < 0.5, np.float32(0.0), np.float32(-0.0))
    d = zeros.copy()
    d[np.arange(n), ax] = sgn
    o = v.copy()
    inside = rng.random(n) < 0.5
    start = np.where(sgn > 0, lo[ax] - 0.1 * ext, hi[ax] + 0.1 * ext)
    start = np.where(inside, lo[ax] + rng.random(n) * (hi[ax] - lo[ax]), start)
    o[np.arange(n), ax] = start.astype(np.float32)
    # half of them take one transverse coordinate from another vertex: planes of two different leaf boxes
    mix = rng.random(n) < 0.5
    w = verts[rng.integers(0, len(verts), n)]
    tr = (ax + 1 + rng.integers(0, 2, n)) % 3
    o[mix, tr[mix]] = w[mix, tr[mix]]
    out["axis"] = _pack(o, d, 0.0, 1e30)
    return out


def interval_rays(sc, rays):
    """rays whose tmin, or tmax, is exactly the fp32 brute-force hit distance of a hitting ray"""
    t, _, _, p = sc.trace_brute(rays, 0)
    hit = p != orc.MISS
    a, b = rays[:, hit].copy(), rays[:, hit].copy()
    a[6] = t[hit]
    b[7] = t[hit]
    b[6] = 0.0
    return np.ascontiguousarray(np.concatenate([a, b], 1))


def brute(sc, rays):
    t, u, v, p = sc.trace_brute(rays, 0)
    _, _, _, dp = sc.trace_brute(rays, 1)
    return (t, u, v, p), dp


def check_against_brute(tag, hits, occ, ref, dp, disputed_max):
    """criteria 1 and 2 of the module docstring; returns the number of disputed rays"""
    t, u, v, p = hits
    bt, bu, bv, bp = ref
    disputed = bp != dp
    ok = ~disputed
    same = (p == bp) & (t.view(np.uint32) == bt.view(np.uint32)) & (u.view(np.uint32) == bu.view(np.uint32)) & (v.view(np.uint32) == bv.view(np.uint32))
    bad = ok & ~same
    if bad.any():
        i = np.flatnonzero(bad)
        farther = int(((p[i] == orc.MISS) | (t[i] > bt[i])).sum())
        raise AssertionError(f"{tag}: {bad.sum()} of {len(p)} undisputed rays differ from fp32 brute force ({farther} farther or missing); "
                             f"first: ray {i[0]} tree prim {p[i[0]]} t {t[i[0]]!r}, brute prim {bp[i[0]]} t {bt[i[0]]!r}")
    assert ((p == bp) | (p == dp))[disputed].all(), f"{tag}: a disputed ray picked neither brute-force primitive"
    assert disputed.sum() <= disputed_max * len(p), f"{tag}: {disputed.sum()} of {len(p)} rays disputed"
    if occ is not None:
        anyok = (occ != 0) == (bp != orc.MISS)
        assert anyok[ok].all(), f"{tag}: any hit differs from fp32 brute force on {int((~anyok[ok]).sum())} undisputed rays"
        assert ((occ != 0) == ((bp != orc.MISS) | (dp != orc.MISS)))[disputed & (bp != orc.MISS) & (dp != orc.MISS)].all()
    return int(disputed.sum())


@pytest.mark.parametrize("scale,offset", PLACEMENTS, ids=lambda x: str(x))
@pytest.mark.parametrize("name", SCENES)
def test_tree_equals_brute_force(name, scale, offset):
    mesh = placed(base_mesh(name), scale, offset)
    fams = ray_families(mesh, seed=zlib.crc32(repr((name, scale, offset)).encode()))
    ref_sc = orc.Scene(mesh)  # brute force walks its triangle array, not its tree
    batches = {}
    for fam, rays in fams.items():
        batches[fam] = (rays, *brute(ref_sc, rays))
    irays = interval_rays(ref_sc, np.concatenate([fams["random"], fams["vertex"]], 1))
    batches["interval"] = (irays, *brute(ref_sc, irays))
    report = {}
    for leaf, width, quant, collapse in LAYOUTS:
        sc = orc.Scene(mesh, leaf_size=leaf, node_width=width, quantized=quant, collapse=collapse)
        for fam, (rays, ref, dp) in batches.items():
            tag = f"{name} x{scale} +{offset} layout {(leaf, width, quant, collapse)} {fam}"
            report[fam] = check_against_brute(tag, sc.trace_closest(rays), sc.trace_any(rays), ref, dp, DISPUTED_MAX[fam])
    # the interval rays: tmin is exclusive (t > tmin), tmax inclusive (the search starts at (tmax, MISS) and a tie at the same t goes
    # to the lower primitive id), so tmax = t finds that hit again
    rays, (bt, _, _, bp), _ = batches["interval"]
    h = bp != orc.MISS
    assert (bt[h] > rays[6][h]).all() and (bt[h] <= rays[7][h]).all()
    half = rays.shape[1] // 2
    assert (bp[half:] != orc.MISS).all() and np.array_equal(bt[half:], rays[7][half:])
    print(name, scale, offset, "disputed per family:", report)


def test_axis_parallel_origin_on_leaf_plane_far_from_origin():
    """The case that made the padding scale with coordinate magnitude: at 1e4 an fp32 ulp (9.8e-4) exceeds the extent-only pad of
    the atrium (2.8e-4), so fl(bmin - pad) == bmin; an axis-parallel ray whose origin lies on that plane then gets the slab
    interval [-huge, 0] on that axis and the leaf is culled although the triangle test accepts the hit."""
    mesh = placed(base_mesh("atrium"), 1.0, (1e4, 1e4, 1e4))
    rays = ray_families(mesh, n=6000, seed=11)["axis"]
    sc = orc.Scene(mesh)
    ref, dp = brute(sc, rays)
    assert (ref[3] != orc.MISS).mean() > 0.5
    check_against_brute("atrium +1e4 axis-parallel", sc.trace_closest(rays), sc.trace_any(rays), ref, dp, DISPUTED_MAX["axis"])


def test_padding_unchanged_at_the_origin():
    """At the origin the extent term dominates, so the padding, hence the node arrays, of the scenes the golden fixtures and the
    benchmark use are those of an extent-only pad: the leaf boxes sit exactly ext * 1e-5 outside the triangles' boxes."""
    for mesh in (scenes.atrium(0.2), scenes.cornell()):
        sc = orc.Scene(mesh, leaf_size=1, node_width=2, quantized=0, sah_top=0)
        tri = sc.tris()[:, :9].view(np.float32).reshape(-1, 3, 3)
        ext = np.float32((tri.reshape(-1, 3).max(0) - tri.reshape(-1, 3).min(0)).max())
        pad = np.float32(ext * np.float32(1e-5))
        nodes = sc.nodes().view(np.float32)
        refs = sc.nodes()[:, 12:14]
        for slot in range(2):
            leaf = (refs[:, slot] & 0x80000000) != 0
            k = refs[leaf, slot] & 0x0FFFFFFF
            box = nodes[leaf, 6 * slot:6 * slot + 6]
            assert np.array_equal(box[:, :3], (tri[k].min(1) - pad).astype(np.float32))
            assert np.array_equal(box[:, 3:], (tri[k].max(1) + pad).astype(np.float32))


FP32_EXACT_RATIO_LOG2 = 8  # DESIGN.md, "Leaf padding": exact down to triangle size / origin distance 2^-8 at a 1 % barycentric margin
EDGE_MARGIN = 0.01


@pytest.mark.parametrize("k", list(range(2, FP32_EXACT_RATIO_LOG2 + 1)))
def test_fp32_triangle_test_exact_above_ratio(k):
    """Characterisation of the fp32 triangle test (not of the traversal).  64 triangles of size 2^-k, spread over the unit sphere,
    traced from the origin at points whose barycentrics are at least EDGE_MARGIN from every edge, inside and outside.  The edge
    functions are triple products of size ~ ratio^2 computed from vectors of length ~1, so their rounding error is ~ 2^-24 and the
    barycentric error ~ 2^-24 / ratio^2; that reaches the 1 % margin near ratio 2^-8.7 (fp32 and fp64 disagree from 2^-9 on).  Above
    it fp32 and fp64 brute force pick the same primitive for every ray."""
    rng = np.random.default_rng(k)
    s, n = 2.0 ** -k, 64
    i = np.arange(n) + 0.5
    phi, th = np.arccos(1 - 2 * i / n), np.pi * (1 + 5 ** 0.5) * i  # Fibonacci sphere: the triangles do not overlap
    c = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)[:, None, :]
    v = (c + rng.normal(size=(n, 3, 3)) * s).astype(np.float32)
    mb = assets.MeshBuilder()
    mb.add("tiny", v.reshape(-1, 3), np.tile([0, 0, 1], (3 * n, 1)), None, np.arange(3 * n, dtype=np.uint32).reshape(n, 3), assets.Material())
    sc = orc.Scene(mb.build())
    m = 8000
    pick = rng.integers(0, n, m)
    b = rng.dirichlet([1, 1, 1], m) * 1.3 - 0.1  # sums to 1; about half the targets lie outside the triangle
    keep = np.abs(b).min(1) > EDGE_MARGIN
    tgt = np.einsum("mi,mij->mj", b[keep], v[pick[keep]].astype(np.float64))
    rays = _pack(np.zeros((len(tgt), 3), np.float32), _unit(tgt), 0.0, 1e30)
    (_, _, _, p32), p64 = brute(sc, rays)
    assert 0.3 < (p32 != orc.MISS).mean() < 0.9
    assert np.array_equal(p32, p64), f"size/distance 2^-{k}: fp32 != fp64 on {int((p32 != p64).sum())} of {len(p32)} rays"
