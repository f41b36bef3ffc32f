"""The traversal kernels address a structure as one arena -- node array, then the triangle records at a 128-byte aligned offset, then
128 bytes of slack -- through one base and a 32-bit byte offset per lane.  Pinned here at the smallest scenes at
which that addressing can go wrong, every GPU result against the oracle bit for bit in the way of test_traversal_exactness.py: closest
hits (t, u, v, prim), any hits, and the per-ray node / triangle counts of the counted closest-hit launch.

(a) one triangle: a single root, the records right behind it; (b) a mesh whose LAST leaf holds eight triangles, so the fetch of the last
record over-reads into the slack; (c) the same tree through rt3_accel_import; (d) a refit after a vertex update: no new arena, the hits
of a fresh build; (e) instance mode 1, two instances of one mesh, one rotated; (f) every other node layout the library builds;
(g) non-finite rays and an empty scene."""
import numpy as np
import pytest

import orc
from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from raytracer3_amd.render_graph import Context
from support import bits, soup_mesh

pytestmark = pytest.mark.gpu

N_RAYS = 4096


def rays_at(tri, n=N_RAYS, seed=1):
    """n seeded rays (8, n) towards world-space triangles (m, 3, 3): three quarters aimed at points of the triangles (interiors, and every
    eighth ray at a vertex), a quarter in random directions; origins up to two scene sizes away; a tenth of them with a short tmax"""
    rng = np.random.default_rng(seed)
    tri = np.asarray(tri, np.float64)
    lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
    ext = max(float((hi - lo).max()), 1e-3)
    o = (lo + hi) / 2 + rng.uniform(-2, 2, (n, 3)) * ext
    pick = tri[rng.integers(0, len(tri), n)]
    tgt = np.einsum("ni,nij->nj", rng.dirichlet([1.0, 1.0, 1.0], n), pick)
    tgt[::8] = pick[::8, 0]
    d = tgt - o
    rnd = rng.random(n) < 0.25
    d[rnd] = rng.normal(size=(int(rnd.sum()), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmax = np.where(rng.random(n) < 0.1, rng.uniform(0.2, 2.0, n) * ext, 1e30)
    return np.ascontiguousarray(np.concatenate([o.T, d.T, np.zeros((1, n)), tmax[None]]), np.float32)


def check(tag, ctx, osc, rays, min_hit=0.2):
    t, u, v, p, cn, ct, _ = ctx.trace_rays(rays, counts=True)
    ot, ou, ov, op, ocn, oct_ = osc.trace_closest(rays, counts=True)
    assert (op != orc.MISS).mean() >= min_hit, (tag, float((op != orc.MISS).mean()))  # the rays do reach the triangles
    assert np.array_equal(p, op) and np.array_equal(bits(t), bits(ot)) and np.array_equal(bits(u), bits(ou)) and np.array_equal(bits(v), bits(ov)), tag
    assert np.array_equal(cn, ocn) and np.array_equal(ct, oct_), tag
    t2, u2, v2, p2, _ = ctx.trace_rays(rays)  # the non-counting kernel instance
    assert np.array_equal(p2, op) and np.array_equal(bits(t2), bits(ot)) and np.array_equal(bits(u2), bits(ou)) and np.array_equal(bits(v2), bits(ov)), tag
    occ = ctx.trace_rays(rays, any_hit=True)[3]
    assert np.array_equal(occ != 0, osc.trace_any(rays) != 0), tag
    return t, u, v, p


def built(mesh, leaf=None, width=None, quant=None, collapse=None, instances=None, mode=None):
    ctx = Context(0)
    for opt, val in ((L.OPT_LEAF_SIZE, leaf), (L.OPT_NODE_WIDTH, width), (L.OPT_NODE_QUANT, quant), (L.OPT_WIDE_COLLAPSE, collapse), (L.OPT_INSTANCE_MODE, mode)):
        if val is not None:
            ctx.set_option(opt, val)
    ctx.upload_mesh(mesh)
    if instances is not None:
        ctx.set_instances(instances)
    ctx.build_accel()
    return ctx


def same_arrays(ctx, osc):
    nodes, tris = ctx.accel_download()
    return ctx.accel_info()[:3] == (osc.n_nodes, osc.n_tris, osc.max_depth) and np.array_equal(nodes, osc.nodes()) and np.array_equal(tris, osc.tris())


def last_leaf_count(nodes):
    """triangles in the leaf that holds the last record of a default-layout (64-byte quantised) tree"""
    refs = nodes[:, 10:14].ravel()
    leaves = refs[(refs != 0xFFFFFFFF) & ((refs & 0x80000000) != 0)]
    first = leaves & 0x0FFFFFFF
    return int(((leaves[np.argmax(first)] >> 28) & 7) + 1)


def tail_mesh():
    """a small cloud plus eight triangles fanned around one far point on +x, the end of the Morton order: with leaves of up to eight
    (range collapse) the fan is the leaf of the last eight records"""
    rng = np.random.default_rng(5)
    c = rng.uniform(-1, 1, (61, 1, 3))
    cloud = c + rng.normal(size=(61, 3, 3)) * 0.1
    ang = np.arange(8) * (2 * np.pi / 8)
    fan = np.tile([40.0, 0.0, 0.0], (8, 3, 1))
    fan[:, 1, 1] += 0.02 * np.cos(ang)
    fan[:, 1, 2] += 0.02 * np.sin(ang)
    fan[:, 2, 1] += 0.02 * np.cos(ang + 0.7)
    fan[:, 2, 2] += 0.02 * np.sin(ang + 0.7)
    tri = np.concatenate([cloud, fan]).astype(np.float32)
    mesh = soup_mesh(tri)
    osc = orc.Scene(mesh, **TAIL_ORC)
    assert last_leaf_count(osc.nodes()) == 8 and set(osc.tris()[-8:, 9]) == set(range(61, 69))
    return mesh, osc, tri


TAIL_OPTS = dict(leaf=8, collapse=0)  # the library's options for the tail mesh, and the oracle's
TAIL_ORC = dict(leaf_size=8, collapse=0)
_TAIL = []


def tail():
    if not _TAIL:
        _TAIL.append(tail_mesh())
    return _TAIL[0]


def test_one_triangle():
    tri = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
    mesh = soup_mesh(tri)
    osc = orc.Scene(mesh)
    ctx = built(mesh)
    try:
        assert ctx.accel_info()[:2] == (1, 1) and same_arrays(ctx, osc)
        check("one triangle", ctx, osc, rays_at(tri))
    finally:
        ctx.close()


def test_last_leaf_of_eight_reads_into_the_slack():
    mesh, osc, tri = tail()
    ctx = built(mesh, **TAIL_OPTS)
    try:
        assert same_arrays(ctx, osc)
        rays = rays_at(tri, seed=2)
        check("tail, whole scene", ctx, osc, rays)
        # and a batch that only looks at the fan: every ray walks into the last leaf and tests its last record
        check("tail, fan only", ctx, osc, rays_at(tri[-8:], seed=3), min_hit=0.5)
    finally:
        ctx.close()


def test_imported_tree():
    mesh, osc, tri = tail()
    ctx = built(mesh)  # the library's own default tree (leaves of two) ...
    try:
        before = ctx.stats().accel_arena_serial
        ctx.accel_import(osc.nodes(), osc.tris())  # ... replaced by the oracle's leaves-of-eight tree over the same triangles
        assert before != 0 and ctx.stats().accel_arena_serial > before  # a new allocation
        assert ctx.accel_info()[:2] == (osc.n_nodes, osc.n_tris)
        nodes, tris = ctx.accel_download()
        assert np.array_equal(nodes, osc.nodes()) and np.array_equal(tris, osc.tris())
        check("imported", ctx, osc, rays_at(tri, seed=4))
        check("imported, fan only", ctx, osc, rays_at(tri[-8:], seed=5), min_hit=0.5)
    finally:
        ctx.close()


def test_refit_keeps_the_arena():
    mesh, _, tri = tail()
    v = mesh.vertices.copy()
    v[:, :3] = (v[:, :3].astype(np.float64) * [1.0, 1.25, 0.8] + [0.3, -0.2, 0.1]).astype(np.float32)
    moved = assets.Mesh(v, mesh.indices, mesh.geometries, mesh.prim_counts, list(mesh.names), list(mesh.textures))
    mtri = moved.triangle_positions().astype(np.float32)
    ctx, fresh = built(mesh, **TAIL_OPTS), built(moved, **TAIL_OPTS)
    try:
        arena = ctx.stats().accel_arena_serial  # taken where an arena is allocated: any allocation, by whatever path, moves it
        assert arena != 0
        ctx.update_vertices(v)
        ctx.refit_accel()
        assert ctx.stats().accel_arena_serial == arena  # refitted in place
        osc = orc.Scene(moved, **TAIL_ORC)
        rays = rays_at(mtri, seed=6)
        want = check("fresh build", fresh, osc, rays)
        got = ctx.trace_rays(rays)[:4]
        for g, w in zip(got, want):
            assert np.array_equal(bits(g), bits(w))
        assert np.array_equal(ctx.trace_rays(rays, any_hit=True)[3] != 0, osc.trace_any(rays) != 0)
        ctx.refit_accel()  # and again, from the same vertices
        assert ctx.stats().accel_arena_serial == arena
        assert np.array_equal(ctx.trace_rays(rays)[3], want[3])
    finally:
        ctx.close()
        fresh.close()


def test_two_level_two_instances():
    room = scenes.cornell()
    g = room.names.index("tall")
    rot = np.eye(4, dtype=np.float32)
    c, s = np.cos(0.6), np.sin(0.6)
    rot[:3, :3] = np.float32([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.float32([[1, 0, 0], [0, c, -s], [0, s, c]])
    rot[:3, 3] = [1.5, -0.5, 0.75]
    inst = [(g, 1, np.eye(4, dtype=np.float32)), (g, 1, rot)]
    osc = orc.Scene(room, instances=inst)
    world = osc.tris()[:, :9].copy().view(np.float32).reshape(-1, 3, 3)
    flat, two = built(room, instances=inst, mode=0), built(room, instances=inst, mode=1)
    try:
        assert same_arrays(flat, osc)
        assert two.accel_levels()[0] == 1  # one shared bottom tree
        rays = rays_at(world, seed=7)
        t, u, v, p = check("flattened", flat, osc, rays)
        t1, u1, v1, p1, _ = two.trace_rays(rays)
        assert np.array_equal(p1, p) and np.array_equal(bits(t1), bits(t)) and np.array_equal(bits(u1), bits(u)) and np.array_equal(bits(v1), bits(v))
        c1 = two.trace_rays(rays, counts=True)
        assert np.array_equal(c1[3], p) and np.array_equal(bits(c1[0]), bits(t))
        assert np.array_equal(two.trace_rays(rays, any_hit=True)[3] != 0, osc.trace_any(rays) != 0)
    finally:
        flat.close()
        two.close()


# (leaf_size, node_width, quantized, collapse): binary, four-wide fp32 (128-byte nodes), 48-byte quantised
OTHER_LAYOUTS = {"binary": (2, 2, 0, 2), "wide-128": (2, 4, 0, 2), "quantised-48": (2, 4, 2, 2), "quantised-48, leaves of eight": (8, 4, 2, 0)}


@pytest.mark.parametrize("name", OTHER_LAYOUTS)
def test_other_layouts(name):
    leaf, width, quant, collapse = OTHER_LAYOUTS[name]
    mesh = scenes.cornell()
    osc = orc.Scene(mesh, leaf_size=leaf, node_width=width, quantized=quant, collapse=collapse)
    ctx = built(mesh, leaf=leaf, width=width, quant=quant, collapse=collapse)
    try:
        assert same_arrays(ctx, osc)
        check(name, ctx, osc, rays_at(mesh.triangle_positions(), seed=8))
    finally:
        ctx.close()


def test_non_finite_rays_and_empty_scene():
    mesh, osc, tri = tail()
    rays = rays_at(tri, seed=9)
    bad = rays.copy()
    rng = np.random.default_rng(10)
    bad[rng.integers(0, 6, N_RAYS), np.arange(N_RAYS)] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), N_RAYS)
    ctx = built(mesh, **TAIL_OPTS)
    try:
        for any_hit in (False, True):
            assert np.all(ctx.trace_rays(bad, any_hit=any_hit)[3] == (0 if any_hit else L.MISS))
        t, u, v, p, cn, ct, _ = ctx.trace_rays(bad, counts=True)
        assert np.all(p == L.MISS) and not cn.any() and not ct.any()
        mixed = rays.copy()
        mixed[:, ::2] = bad[:, ::2]  # finite and non-finite rays side by side in every wave
        t, u, v, p, _ = ctx.trace_rays(mixed)
        ot, ou, ov, op = osc.trace_closest(rays)
        assert np.all(p[::2] == L.MISS) and np.array_equal(p[1::2], op[1::2]) and np.array_equal(bits(t[1::2]), bits(ot[1::2]))
    finally:
        ctx.close()
    mb = assets.MeshBuilder()
    mb.add("none", np.zeros((0, 3)), np.zeros((0, 3)), None, np.zeros((0, 3), np.uint32), assets.Material())
    ctx = Context(0)
    try:
        ctx.upload_mesh(mb.build())
        ctx.build_accel()
        assert ctx.accel_info()[:2] == (0, 0) and ctx.stats().accel_arena_serial == 0
        assert np.all(ctx.trace_rays(rays)[3] == L.MISS) and not ctx.trace_rays(rays, any_hit=True)[3].any()
    finally:
        ctx.close()
