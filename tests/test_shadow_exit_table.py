"""k_shadow's exit table (DESIGN.md sections 5 and 7; RT3_OPT_SHADOW_EXIT_TABLE): a shadow ray first tries the leaf recorded for the cell where
it leaves the scene box, then walks as before.  Occlusion does not depend on which occluder is found, so nothing a launch reports may depend
on the option -- off (0), on (1), or on with pseudo-random valid entries (2).  Every comparison here is exact: frames bit for bit between the
three settings and against the oracle's reference_mode (the alpha-masked scene, which the oracle does not model, between the settings only); any-hit flags between the three settings and against orc.trace_any, on the ray
families of test_traversal_exactness_cpu at the origin and at (1e4, 1e4, 1e4), on the edges of the cell computation (flat boxes, an empty
scene, origins outside, directions away, signed zeros on box planes, non-finite rays, short ranges), after a refit that moves the shell,
through the launch-start switch, and in two-level mode (no table)."""
import math

import numpy as np
import pytest

import deform_worlds as dw
import integrator_worlds as iw
import orc
from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from raytracer3_amd.render_graph import Context
from raytracer3_amd.renderer import Camera, PathTracer
from support import as_orc, bits, soup_mesh
from test_traversal_exactness_cpu import SOUP_KINDS, _pack, _unit, base_mesh, interval_rays, placed, ray_families

pytestmark = pytest.mark.gpu

FULL = L.F_NEE_SKY | L.F_BLUENOISE | L.F_SPECULAR | L.F_FACEFORWARD  # the flags of the frame-parity tests (the oracle's reference_mode has these)
EMIT = FULL | L.F_NEE_EMISSIVE  # and with the emitter queue beside the sky's: compared between the settings only
OPTIONS = (0, 1, 2)
WARMUP = 1 << 16  # tries below which every ray uses the table (kExitWarmupTries)


def built(mesh, **opts):
    ctx = Context(0)
    for k, v in opts.items():
        ctx.set_option(getattr(L, "OPT_" + k.upper()), v)
    ctx.upload_mesh(mesh)
    ctx.build_accel()
    return ctx


def flags_by_option(ctx, rays):
    """{option: occlusion flags} of one ray batch; the getter must report a table exactly when the option asks for one"""
    out = {}
    for opt in OPTIONS:
        ctx.set_option(L.OPT_SHADOW_EXIT_TABLE, opt)
        assert (ctx.exit_table_info()[0] != 0) == (opt != 0), opt
        out[opt] = ctx.trace_rays(rays, any_hit=True)[3] != 0
    return out


def check_flags(tag, ctx, osc, rays):
    want = osc.trace_any(rays) != 0
    got = flags_by_option(ctx, rays)
    for opt in OPTIONS:
        bad = np.flatnonzero(got[opt] != want)
        assert bad.size == 0, (tag, "option", opt, "rays", bad[:8].tolist(), "of", rays.shape[1])
    return want


# ---------------------------------------------------------------------------------------------------------------- 1. frames
def frame_scenes():
    room, _, room_cam = iw.furnace(1.0)
    return {
        "closed_room": (room, room_cam),
        "cornell": (scenes.cornell(), scenes.CORNELL_CAMERA),
        "cutout_cornell": (scenes.cutout_cornell(), scenes.CORNELL_CAMERA),
        "atrium": (scenes.atrium(0.2), scenes.ATRIUM_CAMERA),
    }


@pytest.mark.parametrize("name", ["closed_room", "cornell", "cutout_cornell", "atrium"])
def test_frames_do_not_depend_on_the_table(name):
    mesh, cam_kw = frame_scenes()[name]
    sky, bn = scenes.sky(256, 128), assets.load_bluenoise()
    W, H = 64, 48
    pt = PathTracer((W, H))
    try:
        pt.set_scene(mesh, sky, bn)
        cam = Camera(cam_kw["position"], cam_kw["direction"], math.radians(cam_kw["fov_deg"]), W / H)
        g = pt.make_gconst(cam, samples=4, bounces=3, frame=1, flags=FULL)
        ge = pt.make_gconst(cam, samples=4, bounces=3, frame=1, flags=EMIT)
        lights, emit = {}, {}
        for opt in (1, 0, 2):  # (the first render builds the structure with the default, 1)
            if lights:
                pt.ctx.set_option(L.OPT_SHADOW_EXIT_TABLE, opt)
            pt.render(g)
            lights[opt] = pt.light()
            cells, tried, _, _ = pt.ctx.exit_table_info()
            assert (cells != 0) == (opt != 0) and (tried != 0) == (opt != 0), (name, opt, cells, tried)
            pt.render(ge)
            emit[opt] = pt.light()
        gb, depth = pt.gbuffer()
    finally:
        pt.close()
    assert np.array_equal(bits(lights[0]), bits(lights[1])) and np.array_equal(bits(lights[0]), bits(lights[2])), name
    assert np.array_equal(bits(emit[0]), bits(emit[1])) and np.array_equal(bits(emit[0]), bits(emit[2])), name
    if name == "cutout_cornell":
        return  # the oracle has no alpha test: a masked scene is held to "the three settings agree" alone
    osc = orc.Scene(mesh, sky, bn)
    og = as_orc(g)
    ogb, odepth = osc.gbuffer(og)
    assert np.array_equal(bits(depth), bits(odepth))
    olight, _ = osc.reference_mode(og, ogb, odepth)
    assert np.array_equal(bits(lights[1]), bits(olight)), name
    assert float(olight[..., :3].mean()) > 0.0


# ---------------------------------------------------------------------------------------------------------------- 2. any-hit flags
@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), (1e4, 1e4, 1e4)], ids=["origin", "far"])
@pytest.mark.parametrize("name", ("cornell", "atrium") + SOUP_KINDS)
def test_any_hit_flags(name, offset):
    mesh = placed(base_mesh(name), 1.0, offset)
    osc = orc.Scene(mesh)
    fam = ray_families(mesh, n=1500, seed=11)
    fam["interval"] = interval_rays(osc, fam["random"])
    ctx = built(mesh)
    try:
        assert ctx.exit_table_info()[0] == 6 * 256 * 256
        for kind, rays in fam.items():
            want = check_flags((name, offset, kind), ctx, osc, rays)
            assert want.any() or kind == "interval" or rays.shape[1] == 0  # the family does meet the scene (a soup has no shared edges: no "edge" rays)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 3. edges of the cell computation


def root_box(osc):
    """the box the table's cells are laid on: the union of the root's child boxes as the walk decodes them (origin + byte * step, fp32 steps),
    rounded outward to fp32 -- rt3_accel.hip's make_exit_table"""
    w = osc.nodes()[0]
    org = w[:3].copy().view(np.float32).astype(np.float64)
    step = np.float64([w[3:4].copy().view(np.float32)[0], w[14:15].copy().view(np.float32)[0], w[15:16].copy().view(np.float32)[0]])
    by = w[4:10].copy().view(np.uint8).astype(np.float64)
    live = [k for k in range(4) if w[10 + k] != 0xFFFFFFFF]
    lo = np.min([org + by[6 * k:6 * k + 3] * step for k in live], 0)
    hi = np.max([org + by[6 * k + 3:6 * k + 6] * step for k in live], 0)
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    lo32 = np.where(lo32.astype(np.float64) > lo, np.nextafter(lo32, np.float32(-np.inf)), lo32)
    hi32 = np.where(hi32.astype(np.float64) < hi, np.nextafter(hi32, np.float32(np.inf)), hi32)
    return lo32, hi32


def root_plane_rays(osc, tri, seed):
    """rays whose origins lie exactly on planes of the table's own box (root_box): axis-parallel ones with signed zeros that run IN a face or
    along an edge of it, and oblique ones that start on a face or a corner and aim at the triangles or away from them"""
    rng = np.random.default_rng(seed)
    lo, hi = root_box(osc)
    tri = np.asarray(tri, np.float64)
    n = 512
    o = np.where(rng.random((n, 3)) < 0.5, lo, hi).astype(np.float32)  # corners ...
    free = rng.integers(0, 3, n)
    inner = rng.random(n) < 0.5
    k = np.arange(n)
    o[k[inner], free[inner]] = (lo[free[inner]] + rng.random(int(inner.sum())).astype(np.float32) * (hi - lo)[free[inner]]).astype(np.float32)  # ... or points of an edge
    ax = rng.integers(0, 3, n)
    d = np.where(rng.random((n, 3)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    d[k, ax] = rng.choice(np.float32([-1.0, 1.0]), n)
    tgt = np.einsum("ni,nij->nj", rng.dirichlet([1.0, 1.0, 1.0], n), tri[rng.integers(0, len(tri), n)])
    aim = _unit(tgt - o.astype(np.float64))
    return {"root box planes, axis-parallel": _pack(o, d, 0.0, 1e30), "root box planes, towards": _pack(o, aim, 0.0, 1e30),
            "root box planes, away": _pack(o, -aim, 0.0, 1e30)}


def edge_rays(tri, seed):
    """rays around world-space triangles (m, 3, 3): aimed at them from outside the box and from inside; pointing away from the box; axis-parallel
    with +0.0 / -0.0 components, origins and transverse coordinates on the planes of the triangles' own bounding box (root_plane_rays has the
    table's box); non-finite; tmax short of every hit, tmin beyond"""
    rng = np.random.default_rng(seed)
    tri = np.asarray(tri, np.float64)
    p = tri.reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    ext = max(float((hi - lo).max()), 1e-3)
    ctr = (lo + hi) / 2
    n = 512
    tgt = np.einsum("ni,nij->nj", rng.dirichlet([1.0, 1.0, 1.0], n), tri[rng.integers(0, len(tri), n)])
    out = {}
    o = ctr + _unit(rng.normal(size=(n, 3))) * ext * rng.uniform(1.5, 4.0, (n, 1))
    out["outside, towards"] = _pack(o, _unit(tgt - o), 0.0, 1e30)
    out["outside, away"] = _pack(o, _unit(o - tgt), 0.0, 1e30)
    o = lo + rng.random((n, 3)) * (hi - lo)
    out["inside"] = _pack(o, _unit(rng.normal(size=(n, 3))), 0.0, 1e30)
    ax = rng.integers(0, 3, n)
    sgn = rng.choice([-1.0, 1.0], n)
    d = np.where(rng.random((n, 3)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    d[np.arange(n), ax] = sgn
    o = np.where(rng.random((n, 3)) < 0.5, lo, hi)  # a corner of the box: every transverse coordinate on a box plane ...
    mid = rng.random(n) < 0.5
    o[mid] = tgt[mid]  # ... or through a point of a triangle
    o[np.arange(n), ax] = np.where(rng.random(n) < 0.5, np.where(sgn > 0, lo[ax] - 0.5 * ext, hi[ax] + 0.5 * ext), np.where(sgn > 0, lo[ax], hi[ax]))
    out["axis, signed zeros, on planes"] = _pack(o, d, 0.0, 1e30)
    base = out["outside, towards"].copy()
    dist = np.linalg.norm(tgt - base[:3].T.astype(np.float64), axis=1)
    short = base.copy()
    short[7] = (0.5 * dist).astype(np.float32)  # ends before the triangle it aims at
    out["tmax short of the hit"] = short
    beyond = base.copy()
    beyond[6] = (dist + 4.0 * ext).astype(np.float32)  # starts behind everything
    out["tmin beyond the scene"] = beyond
    bad = base.copy()
    bad[rng.integers(0, 6, n), np.arange(n)] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), n)
    out["non-finite"] = bad
    return out


EDGE_SCENES = {
    "one triangle": np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]]),
    "two coplanar triangles": np.float32([[[2, 1, -3], [3, 1, -3], [2, 1, -2]], [[3, 1, -2], [2, 1, -2], [3, 1, -3]]]),
}


@pytest.mark.parametrize("name", list(EDGE_SCENES))
def test_flat_boxes(name):
    tri = EDGE_SCENES[name]
    mesh = soup_mesh(tri)
    osc = orc.Scene(mesh)
    ctx = built(mesh)
    try:
        assert ctx.exit_table_info()[0] == 6 * 256 * 256
        for kind, rays in root_plane_rays(osc, tri, seed=24).items():
            check_flags((name, kind), ctx, osc, rays)
        for kind, rays in edge_rays(tri, seed=21).items():
            want = check_flags((name, kind), ctx, osc, rays)
            if kind == "outside, towards":
                assert want.mean() > 0.9, (name, kind)
            if kind in ("outside, away", "tmax short of the hit", "tmin beyond the scene", "non-finite"):
                assert not want.any(), (name, kind)
    finally:
        ctx.close()


def test_room_edges():
    mesh = scenes.cornell()
    osc = orc.Scene(mesh)
    ctx = built(mesh)
    try:
        for kind, rays in {**edge_rays(mesh.triangle_positions(), seed=22), **root_plane_rays(osc, mesh.triangle_positions(), seed=25)}.items():
            check_flags(("cornell", kind), ctx, osc, rays)
    finally:
        ctx.close()


def test_empty_scene_has_no_table():
    mb = assets.MeshBuilder()
    mb.add("none", np.zeros((0, 3)), np.zeros((0, 3)), None, np.zeros((0, 3), np.uint32), assets.Material())
    rays = edge_rays(EDGE_SCENES["one triangle"], seed=23)["inside"]
    ctx = built(mb.build())
    try:
        for opt in OPTIONS:
            ctx.set_option(L.OPT_SHADOW_EXIT_TABLE, opt)
            assert ctx.exit_table_info() == (0, 0, 0, 0)
            assert not ctx.trace_rays(rays, any_hit=True)[3].any()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 4. refit
def test_refit_moves_the_shell():
    rest = dw.mesh_at(0)
    v = dw.mesh_at(1).vertices.copy()  # the cloth and the blocks deform ...
    a, b = dw.vertex_range(rest, "ceiling")
    v[a:b, 1] += np.float32(0.5)  # ... and the shell moves: the ceiling goes up, the right wall out
    a, b = dw.vertex_range(rest, "right")
    v[a:b, 0] += np.float32(0.3)
    moved = assets.Mesh(v, rest.indices, rest.geometries, rest.prim_counts, list(rest.names), list(rest.textures))
    rng = np.random.default_rng(31)
    n = 4096
    o = np.float32([-0.9, 0.05, -0.9]) + rng.random((n, 3)).astype(np.float32) * np.float32([1.8, 1.9, 4.8])
    rays = _pack(o, _unit(rng.normal(size=(n, 3))), 1e-3, 1e30)
    ctx = built(rest)
    try:
        arena = ctx.stats().accel_arena_serial
        check_flags("rest", ctx, orc.Scene(rest), rays)
        ctx.set_option(L.OPT_SHADOW_EXIT_TABLE, 1)
        ctx.trace_rays(rays, any_hit=True)
        assert ctx.exit_table_info()[1] > 0
        ctx.update_vertices(v)
        ctx.refit_accel()
        assert ctx.stats().accel_arena_serial == arena and arena != 0  # the table was rewritten in place
        cells, tried, occluded, in_use = ctx.exit_table_info()
        assert (cells, tried, occluded, in_use) == (6 * 256 * 256, 0, 0, 1)  # the counters start again
        want = check_flags("moved", ctx, orc.Scene(moved), rays)
        assert 0.2 < want.mean() < 1.0
        ctx.set_option(L.OPT_SHADOW_EXIT_TABLE, 1)
        ctx.trace_rays(rays, any_hit=True)
        assert ctx.exit_table_info()[1] > 0  # tries again after the reset
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 5. the switch
def test_switch_turns_the_table_off_in_a_cloud():
    mesh = base_mesh("cloud")
    osc = orc.Scene(mesh)
    rng = np.random.default_rng(41)
    n = 20000
    rays = _pack(rng.uniform(-4, 4, (n, 3)), _unit(rng.normal(size=(n, 3))), 0.0, 1e30)
    want = osc.trace_any(rays) != 0
    ctx = built(mesh)
    try:
        first = ctx.trace_rays(rays, any_hit=True)[3] != 0  # (two launches: 40000 tries)
        assert ctx.exit_table_info()[3] == 1
        ctx.trace_rays(rays, any_hit=True)
        cells, tried, occluded, in_use = ctx.exit_table_info()
        print("cloud: tried %d, occluded %d, rate %.4f, in_use %d" % (tried, occluded, occluded / max(tried, 1), in_use))
        assert tried >= WARMUP and in_use == 0 and 4 * occluded < tried
        after = ctx.trace_rays(rays, any_hit=True)[3] != 0  # every 32nd chunk only
        t2 = ctx.exit_table_info()[1]
        assert tried < t2 < tried + 2 * n  # the rate stays known, from a sample
        assert np.array_equal(first, want) and np.array_equal(after, want)
    finally:
        ctx.close()


def test_switch_keeps_the_table_on_in_a_closed_room():
    mesh, _, _ = iw.furnace(1.0)
    osc = orc.Scene(mesh)
    rng = np.random.default_rng(42)
    n = 20000
    rays = _pack(rng.uniform(-0.95, 0.95, (n, 3)), _unit(rng.normal(size=(n, 3))), 0.0, 1e30)
    want = osc.trace_any(rays) != 0
    ctx = built(mesh)
    try:
        for _ in range(3):
            got = ctx.trace_rays(rays, any_hit=True)[3] != 0
            assert np.array_equal(got, want)
        cells, tried, occluded, in_use = ctx.exit_table_info()
        print("closed room: tried %d, occluded %d, rate %.4f, in_use %d" % (tried, occluded, occluded / max(tried, 1), in_use))
        assert tried == 6 * n and in_use == 1 and 4 * occluded >= tried
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 6. two-level mode
def test_two_level_mode_has_no_table():
    room = scenes.cornell()
    g = room.names.index("tall")
    shift = np.eye(4, dtype=np.float32)
    shift[:3, 3] = [1.5, -0.5, 0.75]
    inst = [(0, len(room.names), np.eye(4, dtype=np.float32)), (g, 1, shift)]
    osc = orc.Scene(room, instances=inst)
    rays = ray_families(room, n=1500, seed=51)["random"]
    want = osc.trace_any(rays) != 0
    ctx = Context(0)
    try:
        ctx.set_option(L.OPT_INSTANCE_MODE, 1)
        ctx.upload_mesh(room)
        ctx.set_instances(inst)
        ctx.build_accel()
        for opt in OPTIONS:
            ctx.set_option(L.OPT_SHADOW_EXIT_TABLE, opt)
            assert ctx.exit_table_info() == (0, 0, 0, 0)
            assert np.array_equal(ctx.trace_rays(rays, any_hit=True)[3] != 0, want)
    finally:
        ctx.close()
