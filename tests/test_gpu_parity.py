"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same seeded inputs.

Bars: bit-exact for integer / index / packed data (BVH arrays, hits, traversal counts, G-buffer); linear radiance is
expected bit-exact too (arithmetic contract) and must at least meet the north_star bar RMSE <= 1e-3;
the display transform (log2/pow from libm vs device) is compared with tolerance 2e-5."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import orc
from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from raytracer3_amd.renderer import Camera, PathTracer
from raytracer3_amd.render_graph import Context
from support import as_orc

pytestmark = pytest.mark.gpu

FULL = L.F_NEE_SKY | L.F_BLUENOISE | L.F_FACEFORWARD
SPEC = FULL | L.F_SPECULAR  # + layered GGX BSDF (brdf.slang:141-311)


@pytest.fixture(scope="module")
def small():
    mesh = scenes.atrium(0.3)
    sky = scenes.sky(512, 256)
    bn = assets.load_bluenoise()
    return mesh, sky, bn, orc.Scene(mesh, sky, bn)


@pytest.fixture(scope="module")
def cornell():
    mesh = scenes.cornell()
    return mesh, orc.Scene(mesh)


def rays_random(n, seed, lo, hi):
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, (n, 3)).T
    d = rng.normal(size=(3, n))
    d /= np.linalg.norm(d, axis=0)
    return np.concatenate([o, d, np.full((1, n), 0.001), np.full((1, n), 1e5)]).astype(np.float32)


def test_device_is_gfx950():
    ctx = Context(0)
    assert "gfx950" in ctx.device_name
    ctx.close()


@pytest.mark.parametrize("leaf,width,quant", [(2, 4, 2), (2, 4, 1), (2, 4, 0), (1, 2, 0), (4, 4, 1), (8, 4, 0), (4, 2, 0), (1, 4, 1), (1, 4, 2), (8, 4, 2)])
def test_lbvh_bit_identical_to_oracle(small, leaf, width, quant):
    """every layout: 64 B binary / 128 B four-wide / 64 B quantised / 48 B compact four-wide nodes x 1..8 triangles per leaf"""
    mesh, sky, bn, _ = small
    osc = orc.Scene(mesh, leaf_size=leaf, node_width=width, quantized=quant)
    ctx = Context(0)
    ctx.set_option(L.OPT_LEAF_SIZE, leaf)
    ctx.set_option(L.OPT_NODE_WIDTH, width)
    ctx.set_option(L.OPT_NODE_QUANT, quant)
    ctx.upload_mesh(mesh)
    handle = ctx.build_accel()
    assert handle >> 30 == L.TAG_ACCEL
    nn, nt, levels, nb = ctx.accel_info()
    assert (nn, nt, levels, nb) == (osc.n_nodes, osc.n_tris, osc.max_depth, 64 if width == 2 else {0: 128, 1: 64, 2: 48}[quant])
    nodes, tris = ctx.accel_download()
    assert np.array_equal(tris, osc.tris())
    assert np.array_equal(nodes, osc.nodes())
    # traversal (hits AND per-ray node / triangle counts) agrees in this layout too
    rays = rays_random(20000, 5, [-14, 0.2, -8], [14, 12, 8])
    t, u, v, p, cn, ct, _ = ctx.trace_rays(rays, counts=True)
    ot, ou, ov, op, ocn, oct = osc.trace_closest(rays, counts=True)
    assert np.array_equal(p, op) and np.array_equal(t[p != L.MISS], ot[p != L.MISS]) and np.array_equal(cn, ocn) and np.array_equal(ct, oct)
    occ, _, _, o_occ = None, None, None, osc.trace_any(rays)
    assert np.array_equal(ctx.trace_rays(rays, any_hit=True)[3] != 0, o_occ != 0)
    ctx.close()


def test_lbvh_even_depth_collapse_still_available(small):
    """RT3_OPT_WIDE_COLLAPSE = 0 (four-wide nodes from even binary depths, the first design) stays bit-identical too."""
    mesh, sky, bn, _ = small
    osc = orc.Scene(mesh, collapse=0)
    ctx = Context(0)
    ctx.set_option(L.OPT_WIDE_COLLAPSE, 0)
    ctx.upload_mesh(mesh)
    ctx.build_accel()
    nodes, tris = ctx.accel_download()
    assert ctx.accel_info()[:3] == (osc.n_nodes, osc.n_tris, osc.max_depth)
    assert np.array_equal(nodes, osc.nodes()) and np.array_equal(tris, osc.tris())
    rays = rays_random(5000, 6, [-14, 0.2, -8], [14, 12, 8])
    t, u, v, p, cn, ct, _ = ctx.trace_rays(rays, counts=True)
    ot, ou, ov, op, ocn, oct = osc.trace_closest(rays, counts=True)
    assert np.array_equal(p, op) and np.array_equal(cn, ocn) and np.array_equal(ct, oct)
    ctx.close()


@pytest.mark.parametrize("collapse,T,leaf", [(2, 1, 2), (2, 1, 4), (2, 3, 3), (2, 0, 2), (1, 2, 2), (1, 8, 2)])
def test_lbvh_collapse_rules_bit_identical(small, collapse, T, leaf):
    """RT3_OPT_WIDE_COLLAPSE: the cost-driven collapse (2, default: binned SAH down to T = 1, triangle records in tree order, a bottom-up
    dynamic programme choosing four-wide groups and multi-triangle leaves) and the greedy surface-area rule (1) against the oracle's arrays
    for several cluster and leaf sizes; the hits do not depend on the rule, the cost-driven tree is smaller and no slower to walk."""
    mesh, sky, bn, _ = small
    osc = orc.Scene(mesh, sah_top=T, collapse=collapse, leaf_size=leaf)
    ctx = Context(0)
    ctx.set_option(L.OPT_SAH_TOP, T)
    ctx.set_option(L.OPT_WIDE_COLLAPSE, collapse)
    ctx.set_option(L.OPT_LEAF_SIZE, leaf)
    ctx.upload_mesh(mesh)
    ctx.build_accel()
    assert ctx.accel_info()[:3] == (osc.n_nodes, osc.n_tris, osc.max_depth)
    nodes, tris = ctx.accel_download()
    assert np.array_equal(nodes, osc.nodes()) and np.array_equal(tris, osc.tris())
    rays = rays_random(20000, 9, [-14, 0.2, -8], [14, 12, 8])
    t, u, v, p, cn, ct, _ = ctx.trace_rays(rays, counts=True)
    ot, ou, ov, op, ocn, oct = osc.trace_closest(rays, counts=True)
    assert np.array_equal(p, op) and np.array_equal(t[p != L.MISS], ot[p != L.MISS]) and np.array_equal(cn, ocn) and np.array_equal(ct, oct)
    bt, bu, bv, bp = osc.trace_brute(rays, 0)
    assert np.array_equal(p, bp) and np.array_equal(t[p != L.MISS], bt[p != L.MISS])  # the fp32 brute force over all triangles
    if collapse == 2 and T == 1 and leaf == 2:
        area = orc.Scene(mesh, sah_top=2, collapse=1)
        an = area.trace_closest(rays, counts=True)[4]
        assert osc.n_nodes < 0.9 * area.n_nodes and cn.mean() <= an.mean()
    ctx.close()


@pytest.mark.parametrize("T", [0, 8, 64])
def test_lbvh_sah_top_bit_identical(small, T):
    """RT3_OPT_SAH_TOP: the tree above Karras subtrees of <= T triangles re-linked by binned SAH on the host -- same arrays as
    the oracle's restatement, same hits as the plain LBVH, fewer node visits."""
    mesh, sky, bn, _ = small
    plain = orc.Scene(mesh, sah_top=0)
    osc = orc.Scene(mesh, sah_top=T)
    ctx = Context(0)
    ctx.set_option(L.OPT_SAH_TOP, T)
    ctx.upload_mesh(mesh)
    ctx.build_accel()
    assert ctx.accel_info()[:3] == (osc.n_nodes, osc.n_tris, osc.max_depth)
    nodes, tris = ctx.accel_download()
    assert np.array_equal(nodes, osc.nodes()) and np.array_equal(tris, osc.tris())
    rays = rays_random(20000, 8, [-14, 0.2, -8], [14, 12, 8])
    t, u, v, p, cn, ct, _ = ctx.trace_rays(rays, counts=True)
    ot, ou, ov, op, ocn, oct = osc.trace_closest(rays, counts=True)
    assert np.array_equal(p, op) and np.array_equal(t[p != L.MISS], ot[p != L.MISS]) and np.array_equal(cn, ocn) and np.array_equal(ct, oct)
    pt_, pu_, pv_, pp_, pcn, pct = plain.trace_closest(rays, counts=True)
    assert np.array_equal(pp_, p) and np.array_equal(pt_[p != L.MISS], t[p != L.MISS])
    if 0 < T <= 8:
        assert cn.mean() < pcn.mean()
    assert np.array_equal(ctx.trace_rays(rays, any_hit=True)[3] != 0, osc.trace_any(rays) != 0)
    ctx.close()


@pytest.mark.parametrize("T", [2, 5, 200])
def test_sah_top_device_bit_identical_collapse1(small, T):
    """The binned-SAH top built on the GPU (level-synchronous for big segments, one thread per small one) under the surface-area
    collapse, against the oracle's: every reduction in it is a min, a max or an integer sum and the partitions are stable, so the
    trees are the same arrays bit for bit."""
    mesh, sky, bn, _ = small
    osc = orc.Scene(mesh, sah_top=T, collapse=1)
    ctx = Context(0)
    ctx.set_option(L.OPT_SAH_TOP, T)
    ctx.set_option(L.OPT_WIDE_COLLAPSE, 1)
    ctx.upload_mesh(mesh)
    ctx.build_accel()
    assert ctx.accel_info()[:3] == (osc.n_nodes, osc.n_tris, osc.max_depth)
    nodes, tris = ctx.accel_download()
    ctx.close()
    assert np.array_equal(nodes, osc.nodes()) and np.array_equal(tris, osc.tris())


def test_one_context_rebuilds_scenes_of_different_sizes(small, cornell):
    """The builder's scratch is one arena the context keeps (BuildArena): a small scene, a large one, the small one again with another
    SAH cluster size and with the full-refit path (T = 0), all on ONE context -- every build equals the oracle's arrays, so nothing
    of an earlier build survives in the reused block."""
    ctx = Context(0)
    for mesh, T in ((cornell[0], 2), (small[0], 2), (cornell[0], 5), (small[0], 0), (small[0], 100), (cornell[0], 2)):
        osc = orc.Scene(mesh, sah_top=T)
        ctx.set_option(L.OPT_SAH_TOP, T)
        ctx.upload_mesh(mesh)
        ctx.build_accel()
        assert ctx.accel_info()[:3] == (osc.n_nodes, osc.n_tris, osc.max_depth)
        nodes, tris = ctx.accel_download()
        assert np.array_equal(nodes, osc.nodes()) and np.array_equal(tris, osc.tris())
    ctx.close()


def test_accel_build_makes_no_bulk_copies():
    """the default build (LBVH + device SAH top + four-wide emit) of the 260 k-triangle bench scene moves
    no array between host and device -- counted by the library itself (rt3_stats.accel_bulk_copies), not inferred from a wall clock that
    a busy box would stretch -- and neither does collapse 1 with T = 2.  The counter does see the geometry tables of a world with many
    placements (over 64 KiB).  The build time is reported (5 - 6 ms on an idle box for the cost-driven default, 3 - 4 ms for collapse 1),
    not asserted."""
    mesh = scenes.atrium(1.0)
    ctx = Context(0)
    ctx.upload_mesh(mesh)
    ctx.build_accel()
    ctx.stats_reset()
    for _ in range(3):
        ctx.build_accel()
    st = ctx.stats()
    assert st.accel_bulk_copies == 0
    assert 0.0 < st.accel_build_ms < 10_000.0
    print(f"rt3_accel_build, {mesh.n_triangles} triangles, warm context: {st.accel_build_ms:.2f} ms")
    ctx.set_option(L.OPT_WIDE_COLLAPSE, 1)
    ctx.set_option(L.OPT_SAH_TOP, 2)
    ctx.stats_reset()
    ctx.build_accel()
    assert ctx.stats().accel_bulk_copies == 0
    ctx.close()
    # positive control: one cornell geometry placed 600 times flattens to 600 x 128 B of geometry tables, more than 64 KiB
    ctx = Context(0)
    ctx.upload_mesh(scenes.cornell())
    ctx.set_instances([(0, 1, _trs((0.0, 0.0, 0.01 * k))) for k in range(600)])
    ctx.stats_reset()
    ctx.build_accel()
    assert ctx.stats().accel_bulk_copies >= 3
    ctx.close()


def _trs(t=(0, 0, 0), ry=0.0, s=(1, 1, 1)):
    c, sn = math.cos(ry), math.sin(ry)
    m = np.array([[c * s[0], 0, sn * s[2], t[0]], [0, s[1], 0, t[1]], [-sn * s[0], 0, c * s[2], t[2]], [0, 0, 0, 1]], np.float32)
    return m


def test_instances_two_placements_one_moved_between_frames():
    """Instance + Transform through the ABI (world/mod.rs:46-60, hit_logic.slang:23).  A room (placed once, identity)
    and ONE mesh placed twice under different matrices (rotation, non-uniform scale, translation); between the two frames one matrix
    changes and the acceleration structure is rebuilt (the TLAS update).  Arrays, G-buffer and radiance of both frames bit for bit
    against the oracle, which flattens the same instances; the build time is reported."""
    room = scenes.cornell()
    sky, bn = scenes.sky(128, 64), assets.load_bluenoise()
    names = list(room.names)
    n_room = names.index("tall")  # geometries [0, n_room) = the walls, [n_room, n_room + 2) = the two blocks
    W, H = 112, 96
    cam = Camera(scenes.CORNELL_CAMERA["position"], scenes.CORNELL_CAMERA["direction"], math.radians(scenes.CORNELL_CAMERA["fov_deg"]), W / H)
    pt = PathTracer((W, H))
    pt.ctx.upload_mesh(room)
    pt.ctx.set_sky(sky)
    pt.ctx.set_bluenoise(bn)
    osc = orc.Scene(room, sky, bn, build=False)
    m_b0 = _trs((0.9, 0.0, 0.9), 0.6, (0.5, 1.3, 0.5))
    for frame, m_b in enumerate((m_b0, _trs((0.75, 0.25, 1.2), -0.35, (0.6, 0.9, 0.45)))):
        inst = [(0, n_room, np.eye(4, dtype=np.float32)), (n_room, 1, _trs((0.2, 0.0, 0.1), 0.3)), (n_room, 1, m_b), (n_room + 1, 1, np.eye(4, dtype=np.float32))]
        pt.ctx.set_instances(inst)
        pt.ctx.stats_reset()
        pt.ctx.build_accel()
        build_ms = pt.ctx.stats().accel_build_ms
        osc.set_instances(inst)
        assert pt.ctx.accel_info()[:3] == (osc.n_nodes, osc.n_tris, osc.max_depth)
        nodes, tris = pt.ctx.accel_download()
        assert np.array_equal(nodes, osc.nodes()) and np.array_equal(tris, osc.tris())
        assert osc.n_tris == room.n_triangles + int(room.prim_counts[n_room])  # the tall block's triangles twice
        g = pt.make_gconst(cam, 8, 3, frame=frame, flags=SPEC)
        pt.render(g)
        light = pt.light()
        gb, depth = pt.gbuffer()
        og = as_orc(g)
        ogb, odepth = osc.gbuffer(og)
        assert np.array_equal(depth.view(np.uint32), odepth.view(np.uint32)) and np.array_equal(gb, ogb)
        olight, _ = osc.reference_mode(og, ogb, odepth)
        assert np.array_equal(light.view(np.uint32), olight.view(np.uint32))
        print(f"frame {frame}: rt3_accel_build with 4 instances {build_ms:.2f} ms")
        if frame == 0:
            first = light.copy()
    assert not np.array_equal(first, light)  # the moved instance shows
    # back to the default: no instances = every geometry once under the identity = the plain scene
    pt.ctx.set_instances([])
    pt.ctx.build_accel()
    plain = orc.Scene(room, sky, bn)
    nodes, tris = pt.ctx.accel_download()
    assert np.array_equal(nodes, plain.nodes()) and np.array_equal(tris, plain.tris())
    # an instance list that places nothing is an empty world: every ray misses, on both sides
    pt.ctx.set_instances([(0, 0, np.eye(4, dtype=np.float32))])
    pt.ctx.build_accel()
    rays = rays_random(2000, 3, [-0.9, 0.1, -0.9], [0.9, 1.9, 0.9])
    assert (pt.ctx.trace_rays(rays)[3] == L.MISS).all() and pt.ctx.accel_info()[1] == 0
    osc.set_instances([(0, 0, np.eye(4, dtype=np.float32))])
    assert (osc.trace_closest(rays)[3] == L.MISS).all()
    # bad instances are refused, not dereferenced
    lib = pt.ctx.lib
    bad = (L.Instance * 1)()
    bad[0].geometry_first, bad[0].geometry_count = 0, len(room.geometries) + 1
    bad[0].transform[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    assert lib.rt3_scene_set_instances(pt.ctx.h, C.byref(bad), 1) == 0 and lib.rt3_accel_build(pt.ctx.h, None) == L.E_INVALID
    bad[0].geometry_count = 1
    bad[0].transform[3] = 0.5  # projective last row
    assert lib.rt3_scene_set_instances(pt.ctx.h, C.byref(bad), 1) == L.E_INVALID
    bad[0].transform[3] = 0.0
    bad[0].transform[12] = float("nan")
    assert lib.rt3_scene_set_instances(pt.ctx.h, C.byref(bad), 1) == L.E_INVALID
    pt.close()


def test_shading_record_normals_device_equals_oracle():
    """The 2 x 16-bit octahedral normals of the 16-byte shading records (packing.slang:64-86): device encode / decode against the
    oracle's on axes, octant borders, tiny / zero vectors and 4096 random directions."""
    rng = np.random.default_rng(5)
    n = rng.normal(size=(4096, 3)).astype(np.float32)
    special = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 0], [1, 0, -1], [0, 0, 0], [1e-30, 0, 0],
                        [1, 1, 1], [-1, -1, -1], [3e38, 3e38, 3e38]], np.float32)
    n = np.concatenate([special, n])
    ctx = Context(0)
    enc = ctx.selftest(17, n.view(np.uint32), 1)[:, 0]
    dec = ctx.selftest(18, enc.reshape(-1, 1), 3).view(np.float32)
    ctx.close()
    oenc = np.array([orc.lib().orc_octa_encode16(orc.ptr(np.ascontiguousarray(v))) for v in n], np.uint32)
    odec = np.zeros((len(n), 3), np.float32)
    for k, w in enumerate(oenc):
        orc.lib().orc_octa_decode16(int(w), orc.ptr(odec[k]))
    assert np.array_equal(enc, oenc) and np.array_equal(dec.view(np.uint32), odec.view(np.uint32))


def test_accel_import_installs_a_foreign_tree_and_refuses_a_broken_one(small):
    """rt3_accel_import (the way back of rt3_accel_download): a tree built elsewhere over the same triangles -- here the oracle's, with a
    different builder setting than the device's own -- is installed and walked: hits and per-ray visit counts are the oracle's for THAT tree,
    frames stay bit-exact; every reference is validated on the host before a kernel may follow it."""
    mesh, sky, bn, _ = small
    other = orc.Scene(mesh, sky, bn, sah_top=4, collapse=1, tree_order=1)  # not the device's default tree
    ctx = Context(0)
    ctx.upload_mesh(mesh)
    lib = ctx.lib
    n, t = np.ascontiguousarray(other.nodes()), np.ascontiguousarray(other.tris())
    assert lib.rt3_accel_import(ctx.h, n.ctypes.data, n.nbytes, t.ctypes.data, t.nbytes) == L.E_STATE  # rt3_accel_build first
    ctx.build_accel()
    own_nodes, _ = ctx.accel_download()
    assert not np.array_equal(own_nodes.shape, n.shape) or not np.array_equal(own_nodes, n)
    ctx.accel_import(n, t)
    assert ctx.accel_info()[:3] == (other.n_nodes, other.n_tris, other.max_depth)
    rays = rays_random(30000, 21, [-14, 0.2, -8], [14, 12, 8])
    tt, u, v, p, cn, ct, _ = ctx.trace_rays(rays, counts=True)
    ot, ou, ov, op, ocn, oct = other.trace_closest(rays, counts=True)
    assert np.array_equal(p, op) and np.array_equal(tt[p != L.MISS], ot[p != L.MISS]) and np.array_equal(cn, ocn) and np.array_equal(ct, oct)
    assert np.array_equal(ctx.trace_rays(rays, any_hit=True)[3] != 0, other.trace_any(rays) != 0)
    # broken trees: a reference out of range, a node reachable twice (a cycle would never end), a triangle range beyond the array, a foreign primitive id
    for what, mutate in (("node out of range", lambda a, b: a.__setitem__((0, 10), np.uint32(other.n_nodes + 5))),
                         ("cycle", lambda a, b: a.__setitem__((1, 10), np.uint32(0))),
                         ("triangles beyond the array", lambda a, b: a.__setitem__((0, 10), np.uint32(0x80000000 | (1 << 28) | (other.n_tris - 1)))),
                         ("foreign primitive", lambda a, b: b.__setitem__((3, 9), np.uint32(mesh.n_triangles + 7)))):
        bad_n, bad_t = n.view(np.uint32).reshape(-1, 16).copy(), t.view(np.uint32).reshape(-1, 12).copy()
        mutate(bad_n, bad_t)
        assert lib.rt3_accel_import(ctx.h, bad_n.ctypes.data, bad_n.nbytes, bad_t.ctypes.data, bad_t.nbytes) == L.E_INVALID, what
    assert lib.rt3_accel_import(ctx.h, n.ctypes.data, n.nbytes - 4, t.ctypes.data, t.nbytes) == L.E_INVALID
    # the refused imports left the installed tree alone
    assert np.array_equal(ctx.trace_rays(rays)[3], op)
    ver = C.c_int(0)
    assert lib.rt3_comm_version(C.byref(ver)) == 0 and ver.value >= 20000  # the RCCL this library links (NCCL API level)
    ctx.close()


def test_bounce1_batch_of_the_cpu_baseline_is_what_the_gpu_traces(small):
    """bench.py's CPU baseline walks "the C2 primary batch + the bounce-1 batch" (SURVEY 8d); the bounce-1 batch comes from the oracle
    (orc_bounce1_rays).  It must be the rays the product traces after the first shade: same number (ray accounting of a 1-spp, 2-bounce
    frame) and, traced through rt3_trace_rays, the same hits as the oracle's traversal."""
    mesh, sky, bn, osc = small
    W, H = 160, 96
    pt = PathTracer((W, H))
    pt.set_scene(mesh, sky, bn)
    cam = Camera(scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], math.radians(scenes.ATRIUM_CAMERA["fov_deg"]), W / H)
    for flags in (0, SPEC):
        g = pt.make_gconst(cam, 1, 2, frame=5, flags=flags)
        pt.ctx.stats_reset()
        pt.render(g)
        st = pt.ctx.stats()
        og = as_orc(g)
        ogb, odepth = osc.gbuffer(og)
        b1 = osc.bounce1_rays(og, ogb, odepth)
        assert st.extension_rays - W * H == b1.shape[1] > 0.5 * W * H
        gt, gu, gv, gp, _ = pt.ctx.trace_rays(b1)
        ot, ou, ov, op = osc.trace_closest(b1)
        assert np.array_equal(gp, op) and np.array_equal(gt[gp != L.MISS], ot[op != L.MISS])
    pt.close()


def test_lbvh_edge_cases():
    """empty scene, one triangle, duplicate triangles (identical Morton codes)."""
    ctx = Context(0)
    mb = assets.MeshBuilder()
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    nrm = np.tile([0, 0, 1], (3, 1))
    mb.add("one", tri, nrm, None, [[0, 1, 2]], assets.Material())
    one = mb.build()
    ctx.upload_mesh(one)
    ctx.build_accel()
    o1 = orc.Scene(one)
    rays = np.array([[0.2, 0.2, 1, 0, 0, -1, 0, 1e5], [2, 2, 1, 0, 0, -1, 0, 1e5]], np.float32).T.copy()
    t, u, v, p, _ = ctx.trace_rays(rays)
    ot, ou, ov, op = o1.trace_closest(rays)
    assert np.array_equal(p, op) and p[0] == 0 and p[1] == L.MISS and t[0] == ot[0] and abs(float(t[0]) - 1.0) < 2e-7
    # 5 coincident copies: equal t -> lowest primitive id wins, on both sides
    mb = assets.MeshBuilder()
    for k in range(5):
        mb.add(f"c{k}", tri, nrm, None, [[0, 1, 2]], assets.Material())
    dup = mb.build()
    ctx.upload_mesh(dup)
    ctx.build_accel()
    od = orc.Scene(dup)
    nodes, tris = ctx.accel_download()
    assert np.array_equal(tris, od.tris()) and np.array_equal(nodes, od.nodes())
    t, u, v, p, _ = ctx.trace_rays(rays)
    assert p[0] == 0 and p[1] == L.MISS
    # empty scene: everything misses, passes are no-ops
    mb = assets.MeshBuilder()
    mb.add("none", np.zeros((0, 3)), np.zeros((0, 3)), None, np.zeros((0, 3), np.uint32), assets.Material())
    ctx.upload_mesh(mb.build())
    ctx.build_accel()
    t, u, v, p, _ = ctx.trace_rays(rays)
    assert (p == L.MISS).all()
    ctx.close()


def _random_soup(n, seed, kind):
    """n triangles: 'cloud' = uniform small triangles, 'grid' = a regular lattice (equal SAH costs, coincident centroids along axes),
    'dups' = a few distinct triangles repeated many times (identical Morton codes, ties everywhere), 'slivers' = long thin ones."""
    rng = np.random.default_rng(seed)
    if kind == "grid":
        side = int(np.ceil(np.sqrt(n)))
        ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n].astype(np.float32)
        base = np.concatenate([ij, np.zeros((n, 1), np.float32)], 1)
        v = np.stack([base, base + [0.9, 0, 0], base + [0, 0.9, 0]], 1)
    elif kind == "dups":
        proto = rng.uniform(-1, 1, (max(2, n // 40), 3, 3)).astype(np.float32)
        v = proto[rng.integers(0, len(proto), n)]
    elif kind == "slivers":
        c = rng.uniform(-4, 4, (n, 1, 3))
        d = rng.normal(size=(n, 1, 3)) * [8.0, 0.05, 0.05]
        v = (c + np.concatenate([np.zeros((n, 1, 3)), d, rng.normal(size=(n, 1, 3)) * 0.05], 1)).astype(np.float32)
    else:
        c = rng.uniform(-4, 4, (n, 1, 3))
        v = (c + rng.normal(size=(n, 3, 3)) * 0.2).astype(np.float32)
    mb = assets.MeshBuilder()
    verts = v.reshape(-1, 3)
    mb.add("soup", verts, np.tile([0, 0, 1], (len(verts), 1)), None, np.arange(3 * n, dtype=np.uint32).reshape(n, 3), assets.Material())
    return mb.build()


@pytest.mark.parametrize("kind", ["cloud", "grid", "dups", "slivers"])
def test_lbvh_random_soups_bit_identical(kind):
    """The builder against the oracle's on triangle soups sized around every hand-over of the device SAH top (one 16-lane group up to
    16 clusters, one workgroup up to 4096, tiles beyond) and with the inputs that make its choices hard: lattices (equal costs, so the
    first minimum in (axis, plane) order decides), repeated triangles (identical Morton codes, coincident centroids -> halved in
    index order), slivers (boxes that overlap everything)."""
    ctx = Context(0)
    for n, T in ((3, 2), (4, 2), (5, 1), (17, 1), (33, 2), (34, 1), (35, 2), (64, 2), (130, 1), (513, 2), (1000, 3), (4097, 1), (8200, 1), (8300, 2), (20000, 1)):
        mesh = _random_soup(n, 1000 + n, kind)
        osc = orc.Scene(mesh, sah_top=T, leaf_size=min(2, T) if T > 1 else 1)
        ctx.set_option(L.OPT_SAH_TOP, T)
        ctx.set_option(L.OPT_LEAF_SIZE, min(2, T) if T > 1 else 1)
        ctx.upload_mesh(mesh)
        ctx.build_accel()
        assert ctx.accel_info()[:3] == (osc.n_nodes, osc.n_tris, osc.max_depth), (kind, n, T)
        nodes, tris = ctx.accel_download()
        assert np.array_equal(tris, osc.tris()) and np.array_equal(nodes, osc.nodes()), (kind, n, T)
    ctx.close()


def test_trace_closest_and_any_exact(small):
    mesh, sky, bn, osc = small
    ctx = Context(0)
    ctx.upload_mesh(mesh)
    ctx.build_accel()
    W, H = 192, 108
    cam = Camera((-10, 2, 0), (1, 0.1, 0), math.radians(65.0), W / H)
    g = as_orc(cam.gconst((W, H)))
    ys, xs = np.mgrid[0:H, 0:W]
    prim_rays = orc.primary_rays(g, xs.ravel(), ys.ravel())
    rnd = rays_random(50000, 1, [-14, 0.2, -8], [14, 12, 8])
    for rays in (prim_rays, rnd):
        t, u, v, p, cn, ct, _ = ctx.trace_rays(rays, counts=True)
        ot, ou, ov, op, ocn, oct = osc.trace_closest(rays, counts=True)
        assert np.array_equal(p, op)
        hit = p != L.MISS
        assert np.array_equal(t[hit].view(np.uint32), ot[hit].view(np.uint32))
        assert np.array_equal(u[hit].view(np.uint32), ou[hit].view(np.uint32))
        assert np.array_equal(v[hit].view(np.uint32), ov[hit].view(np.uint32))
        assert np.array_equal(cn, ocn) and np.array_equal(ct, oct)  # same traversal order -> same algorithmic bytes
        # without counting: same hits
        t2, u2, v2, p2, _ = ctx.trace_rays(rays)
        assert np.array_equal(p2, p) and np.array_equal(t2.view(np.uint32), t.view(np.uint32))
        occ = ctx.trace_rays(rays, any_hit=True)[3]
        assert np.array_equal(occ != 0, osc.trace_any(rays) != 0)
    # pinned against the brute-force fp32 intersector on a subset
    sub = rnd[:, :3000]
    bt, bu, bv, bp = osc.trace_brute(sub, 0)
    t, u, v, p, _ = ctx.trace_rays(sub)
    assert np.array_equal(p, bp) and np.array_equal(t[p != L.MISS], bt[p != L.MISS])
    ctx.close()


def render_both(mesh, sky, bn, osc, W, H, cam_kw, samples, bounces, flags, frame=0, batch_spp=0, rank=0, n_ranks=1):
    pt = PathTracer((W, H), rank=rank, n_ranks=n_ranks)
    pt.set_scene(mesh, sky, bn)
    if batch_spp:
        pt.ctx.set_option(L.OPT_BATCH_SPP, batch_spp)
    cam = Camera(cam_kw["position"], cam_kw["direction"], math.radians(cam_kw["fov_deg"]), W / H)
    g = pt.make_gconst(cam, samples, bounces, frame=frame, flags=flags)
    pt.render(g, postprocess=True)
    light = pt.light()
    gb, depth = pt.gbuffer()
    color = pt.color()
    st = pt.ctx.stats()
    pt.close()
    return g, light, gb, depth, color, st


@pytest.mark.parametrize("flags", [0, FULL, SPEC, L.F_SPECULAR])
def test_frame_parity_atrium(small, flags):
    mesh, sky, bn, osc = small
    W, H = 160, 90
    g, light, gb, depth, color, st = render_both(mesh, sky, bn, osc, W, H, scenes.ATRIUM_CAMERA, 8, 4, flags, frame=3)
    og = as_orc(g)
    ogb, odepth = osc.gbuffer(og)
    assert np.array_equal(depth.view(np.uint32), odepth.view(np.uint32))
    hit = depth != L.BACKGROUND_DEPTH
    assert hit.mean() > 0.5
    assert np.array_equal(gb[hit], ogb[hit])
    olight, counts = osc.reference_mode(og, ogb, odepth)
    diff = light[..., :3].astype(np.float64) - olight[..., :3]
    rmse = float(np.sqrt(np.mean(diff**2)))
    assert rmse <= 1e-3, rmse  # north_star bar
    assert np.array_equal(light.view(np.uint32), olight.view(np.uint32)), f"max abs diff {np.abs(diff).max()}"
    # ray accounting: primary rays + bounce rays, shadow rays
    assert st.extension_rays == W * H + int(counts[0])
    assert st.shadow_rays == int(counts[1])
    # display transform: libm log2f/powf vs device -> tolerance
    ocolor = osc.postprocess(og, odepth, olight)
    assert np.allclose(color, ocolor, atol=2e-5, rtol=1e-4)


@pytest.mark.parametrize("spp,bounces", [(1, 1), (3, 1), (2, 2), (1, 6)])
def test_frame_parity_direct_light_and_depths(small, spp, bounces):
    """BASELINE configs[1] (1 spp, traversal + direct light only = one bounce with NEE) and other path depths."""
    mesh, sky, bn, osc = small
    W, H = 128, 72
    g, light, gb, depth, color, st = render_both(mesh, sky, bn, osc, W, H, scenes.ATRIUM_CAMERA, spp, bounces, SPEC, frame=1)
    og = as_orc(g)
    ogb, odepth = osc.gbuffer(og)
    olight, counts = osc.reference_mode(og, ogb, odepth)
    assert np.array_equal(light.view(np.uint32), olight.view(np.uint32))
    assert st.extension_rays == W * H + int(counts[0]) and st.shadow_rays == int(counts[1])
    if bounces == 1:
        assert int(counts[0]) == 0 and st.shadow_rays > 0  # direct light: primary rays + shadow rays only


def test_frame_parity_cornell_reference_semantics(cornell):
    """Closed scene: no path ever misses, so the RNG counters coincide with the reference's sequential index++."""
    mesh, osc = cornell
    W, H = 128, 128
    g, light, gb, depth, color, st = render_both(mesh, None, None, osc, W, H, scenes.CORNELL_CAMERA, 16, 4, 0, frame=11)
    og = as_orc(g)
    ogb, odepth = osc.gbuffer(og)
    assert (depth != L.BACKGROUND_DEPTH).all()
    assert np.array_equal(gb, ogb) and np.array_equal(depth, odepth)
    olight, counts = osc.reference_mode(og, ogb, odepth)
    assert np.array_equal(light.view(np.uint32), olight.view(np.uint32))
    assert light[..., :3].mean() > 0.01
    assert st.extension_rays == W * H + int(counts[0])
    # (almost) nothing escapes a closed box: hit points are not offset along the normal (refrence_mode.slang:47), so a bounce ray
    # that starts exactly on a wall and grazes it can still leave
    assert int(counts[0]) >= 0.999 * W * H * 16 * 3
    # rays aimed exactly at shared edges and vertices do not leak (2^-20 edge tolerance of the triangle test)
    from test_oracle_bvh import edge_rays

    rays = edge_rays(mesh, [0.0137, 1.0071, 0.3])
    ctx = Context(0)
    ctx.upload_mesh(mesh)
    ctx.build_accel()
    t, u, v, p, _ = ctx.trace_rays(rays)
    ot, ou, ov, op = osc.trace_closest(rays)
    assert (p != L.MISS).all() and np.array_equal(p, op) and np.array_equal(t, ot)
    ctx.close()


def test_shared_edge_sweep_is_watertight_on_the_gpu():
    """SURVEY 8a row a4 / VERDICT r1: the driver traversal the reference relies on is watertight.  Every edge two triangles of the
    FULL atrium share and every vertex surrounded by shared edges, from both sides of the surface (~1.4 M rays aimed exactly at them):
    none slips between two triangles, closest hit and any hit; a sample is compared with the oracle bit for bit."""
    mesh = scenes.atrium(1.0)
    ctx = Context(0)
    ctx.upload_mesh(mesh)
    ctx.build_accel()
    rays, h = orc.shared_edge_rays(mesh)
    assert rays.shape[1] > 1_000_000
    t, u, v, p, _ = ctx.trace_rays(rays)
    odd = np.nonzero((p == L.MISS) | (t > h + 1e-3))[0]
    assert len(odd) < 1e-3 * rays.shape[1]  # folds of the arch tubes, where an exact intersector finds nothing at distance h either
    osc = orc.Scene(mesh)
    if len(odd):
        td, _, _, pd = osc.trace_brute(rays[:, odd[:400]], mode=1, threads=16)
        assert ((pd == orc.MISS) | (td > h + 1e-3)).all()
    occ = ctx.trace_rays(rays, any_hit=True)[3]
    assert occ.all()
    sub = rays[:, ::53]
    ot, ou, ov, op = osc.trace_closest(sub, threads=16)
    assert np.array_equal(p[::53], op) and np.array_equal(t[::53], ot) and np.array_equal(u[::53], ou) and np.array_equal(v[::53], ov)
    ctx.close()


def test_frame_parity_cornell_ref():
    """The box rebuilt from the reference's processed asset (scenes.cornell_ref), direct light as in resources/refrence.png
    (reference semantics, B = 2): radiance and the display image against the oracle."""
    mesh = scenes.cornell_ref()
    osc = orc.Scene(mesh)
    g, light, gb, depth, col, _ = render_both(mesh, None, None, osc, 160, 90, scenes.CORNELL_REF_CAMERA, 8, 2, 0)
    ogb, odepth = osc.gbuffer(as_orc(g))
    olight, _ = osc.reference_mode(as_orc(g), ogb, odepth)
    assert np.array_equal(depth, odepth) and np.array_equal(light.view(np.uint32), olight.view(np.uint32))
    assert light[..., :3].max() > 1.0 and (depth < 1e5).mean() > 0.2


def test_frame_parity_textured_cornell():
    """base-colour textures (hit_logic.slang:31-33): sRGB decode, bilinear, repeat addressing -- bit-exact vs the oracle"""
    mesh = scenes.textured_cornell()
    osc = orc.Scene(mesh)
    W, H = 128, 96
    g, light, gb, depth, color, st = render_both(mesh, None, None, osc, W, H, scenes.CORNELL_CAMERA, 8, 3, L.F_SPECULAR | L.F_FACEFORWARD, frame=2)
    og = as_orc(g)
    ogb, odepth = osc.gbuffer(og)
    assert np.array_equal(gb, ogb) and np.array_equal(depth, odepth)
    olight, _ = osc.reference_mode(og, ogb, odepth)
    assert np.array_equal(light.view(np.uint32), olight.view(np.uint32))
    # the texture really modulates the albedo: the floor pixels are not uniform any more
    plain = orc.Scene(scenes.cornell())
    pgb, _ = plain.gbuffer(og)
    assert (pgb[..., 0] != ogb[..., 0]).mean() > 0.2


def test_batching_and_blend_do_not_change_the_image(small):
    mesh, sky, bn, osc = small
    W, H = 96, 54
    a = render_both(mesh, sky, bn, osc, W, H, scenes.ATRIUM_CAMERA, 8, 3, FULL, batch_spp=0)[1]
    b = render_both(mesh, sky, bn, osc, W, H, scenes.ATRIUM_CAMERA, 8, 3, FULL, batch_spp=3)[1]  # ragged batches 3+3+2
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_progressive_blend_matches_oracle(small):
    mesh, sky, bn, osc = small
    W, H = 64, 36
    pt = PathTracer((W, H))
    pt.set_scene(mesh, sky, bn)
    cam = Camera(scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], math.radians(65.0), W / H)
    prev = None
    for frame in range(3):
        g = pt.make_gconst(cam, 2, 3, frame=frame, blendfactor=1.0 / (frame + 1), flags=FULL)
        pt.render(g)
        light = pt.light()
        og = as_orc(g)
        if frame == 0:
            ogb, odepth = osc.gbuffer(og)
        olight, _ = osc.reference_mode(og, ogb, odepth, prev=prev)
        assert np.array_equal(light.view(np.uint32), olight.view(np.uint32))
        prev = olight
        pt.copy_light_to_prev()
    pt.close()


def test_tile_partition_is_bit_identical(small):
    """the image must not depend on the GPU count (RNG is seeded by global pixel coordinates)."""
    mesh, sky, bn, osc = small
    W, H = 200, 150  # ragged: 4 x 3 tiles, partial right / bottom tiles
    full = render_both(mesh, sky, bn, osc, W, H, scenes.ATRIUM_CAMERA, 4, 3, FULL)[1]
    acc = np.zeros_like(full)
    owned = np.zeros((H, W), np.int32)
    for r in range(3):
        part = render_both(mesh, sky, bn, osc, W, H, scenes.ATRIUM_CAMERA, 4, 3, FULL, rank=r, n_ranks=3)[1]
        xy = orc.tile_pixels(W, H, r, 3)
        acc[xy[:, 1], xy[:, 0]] = part[xy[:, 1], xy[:, 0]]
        owned[xy[:, 1], xy[:, 0]] += 1
        other = np.ones((H, W), bool)
        other[xy[:, 1], xy[:, 0]] = False
        assert (part[other] == 0).all()  # a rank never touches pixels it does not own
    assert (owned == 1).all()
    assert np.array_equal(acc.view(np.uint32), full.view(np.uint32))


def test_pack_unpack_tiles_roundtrip(small):
    import torch

    mesh, sky, bn, osc = small
    W, H = 200, 150
    pt = PathTracer((W, H))
    pt.set_scene(mesh, sky, bn)
    cam = Camera(scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], math.radians(65.0), W / H)
    pt.render(pt.make_gconst(cam, 1, 2, flags=FULL))
    ref = pt.light()
    bufs = []
    for r in range(4):
        n = pt.ctx.tile_pixel_count(r, 4)
        assert n == len(orc.tile_pixels(W, H, r, 4))
        t = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # the zero fill runs on torch's stream, the pack kernel on librt3's
        pt.ctx.check(pt.ctx.lib.rt3_image_pack_tiles(pt.ctx.h, pt.handles["light"], r, 4, C.c_void_p(t.data_ptr())))
        bufs.append(t)
    pt.ctx.wait()
    pt.rg.upload(pt.handles["light"], np.zeros_like(ref))
    for r, t in enumerate(bufs):
        pt.ctx.check(pt.ctx.lib.rt3_image_unpack_tiles(pt.ctx.h, pt.handles["light"], r, 4, C.c_void_p(t.data_ptr())))
    assert np.array_equal(pt.light().view(np.uint32), ref.view(np.uint32))
    pt.close()


def test_sky_tables_match_oracle(small):
    mesh, sky, bn, osc = small
    ctx = Context(0)
    ctx.set_sky(sky)
    al, tx, cm, pu = ctx.sky_download(sky.shape[1], sky.shape[0])
    oal, otx, ocm, opu = osc.sky_tables(sky.shape[1], sky.shape[0])
    assert np.array_equal(al, oal) and np.array_equal(tx, otx) and np.array_equal(cm, ocm) and np.array_equal(pu, opu)
    ctx.close()


def test_error_behaviour(small):
    """Every failure is a negative status + message, never an abort (SURVEY 8b 'Errors')."""
    mesh, sky, bn, osc = small
    ctx = Context(0)
    lib = ctx.lib
    g = L.GConst()
    g.window_size[0], g.window_size[1] = 64, 64
    b = (C.c_uint32 * 2)(0, 0)
    # pass before accel build
    assert ctx.pass_launch("gbuffer", 64, 64, 1, g, b) == L.E_STATE
    ctx.upload_mesh(mesh)
    ctx.build_accel()
    assert ctx.pass_launch("nope", 64, 64, 1, g, b) == L.E_INVALID
    assert "unknown pass" in ctx.last_error()
    assert ctx.pass_launch("gbuffer", 64, 64, 1, g, b, entry="other_entry") == L.E_INVALID
    assert lib.rt3_pass_launch(ctx.h, b"gbuffer", b"main", 64, 64, 1, C.byref(g), 300, b, 2) == L.E_INVALID  # (the raw call: a wrong constants size)
    assert ctx.pass_launch("gbuffer", 64, 64, 1, g, b) == L.E_INVALID  # handles are not images
    img = C.c_uint32()
    assert lib.rt3_image_create(ctx.h, 64, 64, 12345, C.byref(img)) == L.E_INVALID
    assert lib.rt3_image_create(ctx.h, 64, 64, L.FORMAT_R32_SFLOAT, C.byref(img)) == 0
    assert img.value >> 30 == L.TAG_IMAGE
    # options 13 (the retired host SAH top) and 10 (the retired fused traversal launch) are unknown
    assert lib.rt3_set_option(ctx.h, 13, 0) == L.E_INVALID and lib.rt3_set_option(ctx.h, 13, 1) == L.E_INVALID
    assert lib.rt3_set_option(ctx.h, 10, 0) == L.E_INVALID and lib.rt3_set_option(ctx.h, 10, 1) == L.E_INVALID
    # sky radiance must be finite and non-negative (a NaN would poison every CDF entry after it); the oracle applies the same contract
    for bad_value in (np.nan, np.inf, -1.0):
        bad_sky = np.ones((4, 8, 3), np.float32)
        bad_sky[2, 3, 1] = bad_value
        assert lib.rt3_scene_set_sky(ctx.h, bad_sky.ctypes.data, 8, 4) == L.E_INVALID and "sky texel 19" in ctx.last_error()
        assert orc.lib().orc_scene_set_sky(osc.h, orc.ptr(bad_sky), 8, 4) == -1
    # a geometry that references a texture nobody uploaded is refused at launch time, not dereferenced on the GPU
    gi = mesh.geometries.copy()
    gi["base_color_texture_index"][0] = 0
    pc = np.ascontiguousarray(mesh.prim_counts)
    assert lib.rt3_scene_set_geometry(ctx.h, gi.ctypes.data, pc.ctypes.data, len(gi)) == 0
    out = C.c_uint32()
    assert lib.rt3_accel_build(ctx.h, C.byref(out)) == 0
    i0, i1 = C.c_uint32(), C.c_uint32()
    assert lib.rt3_image_create(ctx.h, 64, 64, L.FORMAT_R32G32B32A32_UINT, C.byref(i0)) == 0 and lib.rt3_image_create(ctx.h, 64, 64, L.FORMAT_R32_SFLOAT, C.byref(i1)) == 0
    bb = (C.c_uint32 * 2)(i0.value, i1.value)
    assert ctx.pass_launch("gbuffer", 64, 64, 1, g, bb) == L.E_STATE
    assert "texture" in ctx.last_error()
    # non-finite positions are rejected at upload
    bad = np.zeros((3, 8), np.float32)
    bad[1, 2] = np.nan
    assert lib.rt3_scene_set_vertices(ctx.h, bad.ctypes.data, 3) == L.E_INVALID and "not finite" in ctx.last_error()
    bad[1, 2] = np.inf
    assert lib.rt3_scene_set_vertices(ctx.h, bad.ctypes.data, 3) == L.E_INVALID
    # out-of-range geometry is rejected on the host instead of faulting on the GPU
    gi = mesh.geometries.copy()
    gi["index_offset"][-1] = 2**31
    assert lib.rt3_scene_set_geometry(ctx.h, gi.ctypes.data, pc.ctypes.data, len(gi)) == L.E_INVALID
    # ... also when the world buffers are replaced by smaller ones AFTER the geometry was accepted: rt3_accel_build re-checks
    ctx.upload_mesh(mesh)
    assert lib.rt3_accel_build(ctx.h, C.byref(out)) == 0
    fewer = np.ascontiguousarray(mesh.vertices[: len(mesh.vertices) // 2], np.float32)
    assert lib.rt3_scene_set_vertices(ctx.h, fewer.ctypes.data, len(fewer)) == 0
    assert lib.rt3_accel_build(ctx.h, C.byref(out)) == L.E_INVALID and "vertex range" in ctx.last_error()
    assert ctx.pass_launch("gbuffer", 64, 64, 1, g, bb) == L.E_STATE  # no stale BVH is used
    ctx.upload_mesh(mesh)
    short_idx = np.ascontiguousarray(mesh.indices[: len(mesh.indices) // 2], np.uint32)
    assert lib.rt3_scene_set_indices(ctx.h, short_idx.ctypes.data, len(short_idx)) == 0
    assert lib.rt3_accel_build(ctx.h, C.byref(out)) == L.E_INVALID and "index range" in ctx.last_error()
    ctx.close()


def test_cpp_host_renders_the_same_frame(small, tmp_path):
    """A compiled host (raytracer3_amd/host/example_frame.cpp, the C++ mirror of the reference's builder chain) must
    produce the oracle's image too."""
    import struct
    import subprocess
    from pathlib import Path

    exe = Path(__file__).resolve().parent.parent / "raytracer3_amd" / "host" / "example_frame"
    if not exe.exists():
        subprocess.check_call(["make", "-C", str(exe.parent)])
    mesh, sky, bn, osc = small
    W, H, spp, bounces, frame = 96, 54, 4, 3, 9
    cam = Camera(scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], math.radians(65.0), W / H)
    scene = tmp_path / "scene.bin"
    with open(scene, "wb") as f:
        f.write(struct.pack("<8I", len(mesh.vertices), len(mesh.indices), len(mesh.geometries), sky.shape[1], sky.shape[0], bn.shape[1], bn.shape[0], 0))
        for arr in (mesh.vertices.astype("<f4"), mesh.indices.astype("<u4"), mesh.geometries, mesh.prim_counts.astype("<u4"), sky.astype("<f4"), bn):
            f.write(np.ascontiguousarray(arr).tobytes())
        f.write(np.array([*cam.position, *cam.direction, cam.fov, cam.aspect_ratio], "<f4").tobytes())
    out = tmp_path / "out.bin"
    subprocess.check_call([str(exe), str(scene), str(W), str(H), str(spp), str(bounces), str(SPEC), str(frame), str(out)])
    data = np.fromfile(out, "<f4").reshape(2, H, W, 4)
    g = cam.gconst((W, H))
    g.samples, g.bounces, g.frame, g.blendfactor = spp, bounces, frame, 1.0
    g.pad[0] = SPEC
    og = as_orc(g)
    ogb, odepth = osc.gbuffer(og)
    olight, _ = osc.reference_mode(og, ogb, odepth)
    assert np.array_equal(data[0].view(np.uint32), olight.view(np.uint32))
    assert np.allclose(data[1], osc.postprocess(og, odepth, olight), atol=2e-5, rtol=1e-4)
    # the same host as one rank of a multi-GPU frame (RT3_RANKS): tile partition, RCCL communicator from an id carried over a file,
    # rt3_gather_tiles at frame end -- with one rank (all a one-GPU box allows) the gathered frame is the same frame
    out1 = tmp_path / "out_rank.bin"
    # a file left behind by an earlier run (other nonce) must be replaced, never handed out: rank 0 publishes {this run's nonce, id}
    (tmp_path / "uid.bin").write_bytes(b"\x01" * (8 + L.COMM_ID_BYTES))
    env = dict(os.environ, RT3_RANKS="1", RT3_RANK="0", RT3_UID_FILE=str(tmp_path / "uid.bin"), RT3_UID_NONCE="4242")
    subprocess.check_call([str(exe), str(scene), str(W), str(H), str(spp), str(bounces), str(SPEC), str(frame), str(out1)], env=env)
    blob = (tmp_path / "uid.bin").read_bytes()
    assert len(blob) == 8 + L.COMM_ID_BYTES and int.from_bytes(blob[:8], "little") == 4242
    assert np.array_equal(np.fromfile(out1, "<f4").view(np.uint32), data.ravel().view(np.uint32))


def test_native_asset_pipeline_renders_the_oracle_frame(tmp_path):
    """Files in, pixels out, no Python in between: asset_tool (C++: glTF + PNG + EXR decoders -> C ABI -> pass graph) renders
    a textured scene from a .glb, a PIZ-compressed HALF .exr (what HDRI tools usually write) and the reference's bluenoise.png;
    the oracle, fed by the Python loaders from the same files, must agree bit for bit."""
    import subprocess
    from pathlib import Path

    host = Path(__file__).resolve().parent.parent / "raytracer3_amd" / "host"
    subprocess.check_call(["make", "-C", str(host), "asset_tool"], stdout=subprocess.DEVNULL)
    mesh = scenes.textured_cornell()
    glb, exr = tmp_path / "scene.glb", tmp_path / "sky.exr"
    assets.write_glb(glb, mesh)
    assets.write_exr(exr, scenes.sky(128, 64), "piz", half=True)
    bn_png = Path(__file__).resolve().parent.parent / "resources" / "bluenoise.png"
    W, H, spp, bounces = 80, 60, 4, 3
    c = scenes.CORNELL_CAMERA
    out = tmp_path / "out.bin"
    args = [str(host / "asset_tool"), "render", str(glb), str(exr), str(bn_png), W, H, spp, bounces, SPEC, *c["position"], *c["direction"], 65.0, str(out)]
    subprocess.check_call([str(a) for a in args])
    data = np.fromfile(out, "<f4").reshape(2, H, W, 4)
    ref_mesh, ref_sky, bn = assets.GltfMeshLoader.load(glb), assets.read_exr(exr), assets.load_bluenoise()
    osc = orc.Scene(ref_mesh, ref_sky, bn)
    cam = Camera(c["position"], c["direction"], math.radians(65.0), W / H)
    g = cam.gconst((W, H))
    g.samples, g.bounces, g.frame, g.blendfactor = spp, bounces, 0, 1.0
    g.pad[0] = SPEC
    og = as_orc(g)
    ogb, odepth = osc.gbuffer(og)
    olight, _ = osc.reference_mode(og, ogb, odepth)
    assert (odepth != L.BACKGROUND_DEPTH).mean() > 0.5 and olight[..., :3].mean() > 0
    assert np.array_equal(data[0].view(np.uint32), olight.view(np.uint32))


def test_full_size_frame_properties():
    """BASELINE's C3 window (1920x1080, full atrium, 2048x1024 sky) through size-independent properties, where the oracle
    would need minutes: (1) determinism -- out-of-order ray completion, atomics-based queue compaction and the dynamic ray
    pool must not leak into the image; (2) the frame does not depend on the rank count (1 vs 4 ranks, tiles merged);
    (3) linearity of the reference estimator: doubling every emission doubles the radiance exactly (power-of-two scaling
    is exact in fp32); (4) sample batching (one batch of 64 vs 4 x 16) leaves the bits alone; (5) closed-form bounds: finite,
    non-negative, background pixels untouched; (6) a 64 x 64 window of the frame against the oracle, bit for bit."""
    W, H, spp, B = 1920, 1080, 64, 4  # BASELINE configs[2] at its own size
    mesh, sky, bn = scenes.atrium(1.0), scenes.sky(2048, 1024), assets.load_bluenoise()
    cam = Camera(scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], math.radians(scenes.ATRIUM_CAMERA["fov_deg"]), W / H)

    def render(flags, mesh_=mesh, rank=0, n_ranks=1, batch=0, frame=3):
        pt = PathTracer((W, H), rank=rank, n_ranks=n_ranks)
        if batch:
            pt.ctx.set_option(L.OPT_BATCH_SPP, batch)
        pt.set_scene(mesh_, sky, bn)
        g = pt.make_gconst(cam, spp, B, frame=frame, flags=flags)
        pt.render(g)
        out = pt.light(), pt.gbuffer()[1]
        st = pt.ctx.stats()
        pt.close()
        return out[0], out[1], st, g

    a, depth, st, g = render(SPEC)
    b = render(SPEC)[0]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))  # (1)
    assert st.extension_rays > 1e8 and st.shadow_rays > 5e7
    merged = np.zeros_like(a)
    for r in range(4):  # (2)
        part = render(SPEC, rank=r, n_ranks=4)[0]
        xy = orc.tile_pixels(W, H, r, 4)
        merged[xy[:, 1], xy[:, 0]] = part[xy[:, 1], xy[:, 0]]
    assert np.array_equal(merged.view(np.uint32), a.view(np.uint32))
    assert np.array_equal(render(SPEC, batch=16)[0].view(np.uint32), a.view(np.uint32))  # (4)
    bg = depth == L.BACKGROUND_DEPTH
    assert np.isfinite(a).all() and (a[..., :3] >= 0).all() and (a[bg] == 0).all() and 0.02 < bg.mean() < 0.9  # (5)
    e1 = render(0)[0]  # (3) reference estimator: emissive only
    import copy
    mesh2 = copy.deepcopy(mesh)
    mesh2.geometries["emission"] *= 2.0
    e2 = render(0, mesh_=mesh2)[0]
    assert e1[..., :3].max() > 0 and np.array_equal((e1[..., :3] * 2.0).view(np.uint32), e2[..., :3].view(np.uint32))
    # (6) oracle on a window in the middle of the frame
    osc = orc.Scene(mesh, sky, bn)
    og = as_orc(g)
    x0, y0 = 928, 508
    ogb, odepth = osc.gbuffer(og, rect=(x0, y0, x0 + 64, y0 + 64), threads=16)
    olight, _ = osc.reference_mode(og, ogb, odepth, rect=(x0, y0, x0 + 64, y0 + 64), threads=16)
    assert np.array_equal(olight[y0:y0 + 64, x0:x0 + 64].view(np.uint32), a[y0:y0 + 64, x0:x0 + 64].view(np.uint32))


def test_traversal_counting_keeps_the_frame(small):
    """RT3_OPT_COUNT_TRAVERSAL 0 vs 1: the same image bit for bit and the same ray counts; the counting run fills every traversal
    total (the LDS-served visits are a part of their kind's node visits); k_shadow (NEE on) and k_extend are launched exactly as
    pass_reference_mode issues them, and the stats of the retired fused launch stay 0."""
    mesh, sky, bn, osc = small
    W, H, B = 128, 72, 4
    assert SPEC & L.F_NEE_SKY
    out = {}
    for count in (0, 1):
        pt = PathTracer((W, H))
        pt.ctx.set_option(L.OPT_COUNT_TRAVERSAL, count)
        pt.set_scene(mesh, sky, bn)
        cam = Camera(scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], math.radians(65.0), W / H)
        g = pt.make_gconst(cam, 4, B, frame=2, flags=SPEC)
        pt.ctx.set_option(L.OPT_PROFILE, 1)
        pt.render(g)
        out[count] = (pt.light(), pt.ctx.stats())
        pt.close()
    (la, sa), (lb, sb) = out[0], out[1]
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32))
    assert sa.extension_rays == sb.extension_rays and sa.shadow_rays == sb.shadow_rays
    for f in ("extension_rays", "shadow_rays", "nodes_visited", "tris_tested", "shadow_nodes_visited", "shadow_tris_tested"):
        assert getattr(sb, f) > 0, f
    assert 0 < sb.nodes_visited_lds < sb.nodes_visited and 0 < sb.shadow_nodes_visited_lds < sb.shadow_nodes_visited
    for s in (sa, sb):
        # the gbuffer pass's extend, one extend per bounce but the last, one shadow per bounce
        assert s.extend_launches == 1 + (B - 1) and s.shadow_launches == B
        assert s.trace_launches == 0 and s.trace_ms == 0.0
        assert list(s.trace_rays) == list(s.trace_nodes) == list(s.trace_tris) == [0, 0]


def test_multi_rank_gather_rehearsal(tmp_path):
    """`python bench.py --gpus 3` exactly as the driver invokes it (no launcher on the command line): bench.py starts its three
    ranks itself.  Rehearsal mode for a 1-GPU box (RT3_DIST_BACKEND=gloo: the ranks share GPU 0 and the gather's bytes move
    through host tensors, laid out and untiled exactly like rt3_gather_tiles): the frame assembled on rank 0 from three ranks'
    tiles must be bit-identical to a single-rank render of it."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(RT3_DIST_BACKEND="gloo", RT3_CHECK_GATHER="1")
    cmd = [sys.executable, str(root / "bench.py"), "--gpus", "3", "--steps", "1", "--warmup", "1", "--no-cpu", "--width", "328", "--height", "200", "--spp", "4", "--detail", "0.3"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 3 and d["gather_bit_identical_to_single_rank"] is True and d["value"] > 0
    assert "REHEARSAL" in d["config"]["gather"] and d["gather_is_rccl"] is False  # host-moved bytes are never reported as the RCCL gather
    pr = d["per_rank_ms_per_frame"]  # every rank's per-kernel times ride on the N > 1 line
    assert len(pr["by_rank"]) == 3 and all(len(r) == len(pr["keys"]) for r in pr["by_rank"]) and pr["slowest_rank_sum"] >= pr["mean_rank_sum"] > 0


def test_bench_falls_back_when_the_communicator_cannot_be_built():
    """The RCCL communicator has never met more than one GPU before the driver's node.  If rt3_comm_init fails on any rank, every rank
    of bench.py must drop to the host-moved exchange and SAY SO on the JSON line, rather than die without a number.  Provoked for real
    here: two self-launched ranks share GPU 0 (gloo rehearsal) and are told to try RCCL, which refuses the duplicate device."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(RT3_DIST_BACKEND="gloo", RT3_TRY_RCCL="1", RT3_CHECK_GATHER="1")
    cmd = [sys.executable, str(root / "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu", "--width", "200", "--height", "150", "--spp", "2", "--detail", "0.3"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["config"]["gather"].startswith("FALLBACK") and d["gather_bit_identical_to_single_rank"] is True and d["gather_is_rccl"] is False
    assert "rt3_comm_init failed" in r.stderr


def test_bench_default_command_prints_the_contract_line():
    """`python bench.py` exactly as the driver runs it at N = 1 (default workload: the branch that looks up the committed counter
    profiles), shortened only in steps and the CPU leg: ONE JSON line with the contract's keys, a roofline whose fraction is one,
    and per-kernel times that add up to the step."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "RT3_DIST_BACKEND", "RT3_SKY_W")}
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--steps", "2", "--warmup", "1", "--no-cpu"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    js = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(js) == 1, r.stdout[-2000:]
    d = json.loads(js[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["value"] > 0 and d["config"]["workload"].startswith("C3")
    rf = d["roofline"]
    assert rf["unit"] == "GB/s" and rf["bound"] == "hbm" and 0.0 < rf["frac"] <= 1.0 and rf["achieved"] <= rf["peak"]
    # every ratio to a ceiling is <= 1 and follows from counters of the kernels that are timed.  frac = measured fabric bytes
    # (only from a profile whose source hash is this tree's), frac_8d = SURVEY 8d's algorithmic bytes (may exceed 1: cache-served, and says so),
    # vector_memory.frac = requested bytes without the LDS-served node visits over the measured gather ceiling
    from raytracer3_amd._lib import kernel_source_hash

    assert d["source_hash"] == rf["source_hash"] == kernel_source_hash()
    assert rf["frac_8d"] > 0 and "8d" in rf["frac_8d_is"].lower() and abs(rf["achieved_8d"] / rf["peak"] - rf["frac_8d"]) < 1e-3
    vm = rf["vector_memory"]
    assert 0.0 < vm["frac"] <= 1.0 and 0.2 < vm["node_visits_served_from_lds"] < 0.8
    if rf["traffic"] is not None:  # quoted counters must be those of THESE kernels
        import json as _json

        prof = _json.loads((root / rf["traffic_source"]).read_text())
        assert prof["source_hash"] == d["source_hash"] and rf["binding"]["frac"] <= 1.0
        assert "measured" in rf["frac_is"]
    else:
        assert "LOWER BOUND" in rf["frac_is"] and rf["binding"] is None
    ms = rf["ms_per_frame"]
    assert abs(sum(ms.values()) - d["ms_per_step"]) < 0.05 * d["ms_per_step"]


def test_bench_dump_outputs_is_the_last_timed_frame(tmp_path):
    """`bench.py --dump-outputs DIR` writes the frame its last timed step rendered (frame index warmup + steps - 1): the same bits on
    two runs with the same arguments, and the same bits as a PathTracer rendering that frame directly."""
    import json
    import subprocess
    import sys
    from pathlib import Path

    from raytracer3_amd.renderer import DEFAULT_FLAGS

    root = Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "RT3_DIST_BACKEND", "RT3_SKY_W")}
    W, H, spp, steps, warmup = 200, 150, 2, 3, 1
    for d in ("a", "b"):
        cmd = [sys.executable, str(root / "bench.py"), "--steps", str(steps), "--warmup", str(warmup), "--no-cpu", "--width", str(W), "--height", str(H),
               "--spp", str(spp), "--detail", "0.3", "--dump-outputs", str(tmp_path / d)]
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=500)
        assert r.returncode == 0, r.stderr[-2000:]
        assert json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["steps"] == steps
    a, b = np.load(tmp_path / "a" / "light.npy"), np.load(tmp_path / "b" / "light.npy")
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["light.npy"]
    assert a.dtype == np.float32 and a.shape == (H, W, 4) and a[..., :3].mean() > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    pt = PathTracer((W, H))
    pt.set_scene(scenes.atrium(0.3), scenes.sky(2048, 1024), assets.load_bluenoise())
    cam = Camera(scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], math.radians(scenes.ATRIUM_CAMERA["fov_deg"]), W / H)
    pt.render(pt.make_gconst(cam, spp, 4, frame=warmup + steps - 1, flags=DEFAULT_FLAGS))
    want = pt.light()
    pt.close()
    assert np.array_equal(a.view(np.uint32), want.view(np.uint32))


def test_bench_refuses_more_ranks_than_devices():
    """The same command on the real backend (RCCL cannot put two ranks on one GPU): with fewer than N visible devices it must exit
    non-zero with a message, never report a 1-GPU number as the N-GPU point."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    import torch

    n = torch.cuda.device_count() + 1
    root = Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "RT3_DIST_BACKEND")}
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "0", "--no-cpu"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0
    assert "visible devices" in r.stderr and not any(ln.startswith("{") for ln in r.stdout.splitlines())


def test_gather_layout_and_single_untile(small):
    """The root's half of rt3_gather_tiles on one GPU (RCCL cannot put several ranks on one device, so the exchange itself stays
    unmeasured here): every rank of a 3-rank partition renders its tiles in its own context, the non-root ranks pack them at the
    EXACT offsets rt3_gather_layout reports into one receive buffer, and ONE rt3_gather_unpack launch on the root reassembles
    the frame -- bit-identical to the single-rank render.  Root 1 of 3 (not rank 0) and a ragged window."""
    from raytracer3_amd.renderer import gather_offsets

    mesh, sky, bn, osc = small
    W, H, n, root = 200, 150, 3, 1
    cam = Camera(scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], math.radians(65.0), W / H)
    solo = PathTracer((W, H))
    solo.set_scene(mesh, sky, bn)
    g = solo.make_gconst(cam, 2, 3, frame=2, flags=FULL)
    solo.render(g)
    ref = solo.light()
    solo.close()
    pts = [PathTracer((W, H), rank=r, n_ranks=n) for r in range(n)]
    for pt in pts:
        pt.set_scene(mesh, sky, bn)
        pt.render(g)
    rootpt = pts[root]
    img = rootpt.handles["light"]
    off = rootpt.ctx.gather_layout(img, root, n)
    counts = [rootpt.ctx.tile_pixel_count(r, n) for r in range(n)]
    assert off == gather_offsets(counts, root) and off[-1] == W * H - counts[root]
    recv = rootpt.rg.buffer(off[-1] * 16, "recv")
    ptr, nbytes = rootpt.rg.device_ptr(recv)
    assert nbytes == off[-1] * 16
    for r, pt in enumerate(pts):
        if r == root:
            continue
        pt.ctx.check(pt.ctx.lib.rt3_image_pack_tiles(pt.ctx.h, pt.handles["light"], r, n, C.c_void_p(ptr + off[r] * 16)))
        pt.ctx.wait()
    before = rootpt.light()
    assert not np.array_equal(before.view(np.uint32), ref.view(np.uint32))  # the root alone holds only its own tiles
    rootpt.ctx.gather_unpack(img, root, n, ptr)
    assert np.array_equal(rootpt.light().view(np.uint32), ref.view(np.uint32))
    for pt in pts:
        pt.close()


def test_rccl_communicator_single_rank(small):
    """The RCCL entry points on the one GPU a test box has: unique id, ncclCommInitRank with one rank, the (trivial) gather,
    destroy -- and the state errors around them."""
    mesh, sky, bn, osc = small
    W, H = 128, 64
    pt = PathTracer((W, H))
    pt.set_scene(mesh, sky, bn)
    cam = Camera(scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], math.radians(65.0), W / H)
    pt.render(pt.make_gconst(cam, 1, 2, flags=FULL))
    ref = pt.light()
    lib, h, img = pt.ctx.lib, pt.ctx.h, pt.handles["light"]
    assert lib.rt3_gather_tiles(h, img, 0) == L.E_STATE and "rt3_comm_init" in pt.ctx.last_error()
    uid = pt.ctx.comm_unique_id()
    assert len(uid) == L.COMM_ID_BYTES and any(uid)
    assert lib.rt3_comm_init(h, uid, 1, 1) == L.E_INVALID  # rank must be < n_ranks
    pt.init_comm(uid)
    assert lib.rt3_comm_init(h, uid, 0, 1) == L.E_STATE   # already has a communicator
    assert lib.rt3_gather_tiles(h, img, 1) == L.E_INVALID  # root out of range
    pt.ctx.gather_tiles(img, 0)  # one rank: the frame is already whole
    assert np.array_equal(pt.light().view(np.uint32), ref.view(np.uint32))
    pt.ctx.set_tile_partition(W, H, 1, 2)  # the partition and the communicator must agree
    assert lib.rt3_gather_tiles(h, img, 0) == L.E_STATE and "disagree" in pt.ctx.last_error()
    pt.ctx.comm_destroy()
    pt.ctx.comm_destroy()  # idempotent
    assert lib.rt3_gather_tiles(h, img, 0) == L.E_STATE
    pt.close()


def test_rccl_rendezvous_of_two_processes(tmp_path):
    """As far as one GPU lets the multi-rank path go: two PROCESSES, each with its own context on GPU 0, carry rank 0's unique id
    over a file and both call rt3_comm_init(id, rank, 2).  RCCL's bootstrap must bring the two together -- and then refuse, on
    BOTH ranks, because they sit on the same device ("Duplicate GPU detected", RCCL cannot place two ranks on one GPU): the ABI
    reports that as RT3_E_COMM with RCCL's text instead of hanging or aborting.  The exchange itself needs N GPUs."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    code = (
        "import sys, os, time, ctypes as C\n"
        f"sys.path.insert(0, {str(root)!r})\n"
        "from raytracer3_amd.render_graph import Context\n"
        "r = int(sys.argv[1]); path = sys.argv[2]\n"
        "ctx = Context(0)\n"
        "if r == 0:\n"
        "    uid = ctx.comm_unique_id(); open(path + '.tmp', 'wb').write(uid); os.rename(path + '.tmp', path)\n"
        "else:\n"
        "    t0 = time.time()\n"
        "    while not os.path.exists(path) and time.time() - t0 < 60: time.sleep(0.05)\n"
        "    uid = open(path, 'rb').read()\n"
        "rc = ctx.lib.rt3_comm_init(ctx.h, C.c_char_p(uid), r, 2)\n"
        "print('RESULT', r, rc, ctx.last_error())\n"
    )
    uid_file = str(tmp_path / "uid.bin")
    env = dict(os.environ, NCCL_DEBUG="WARN")
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r), uid_file], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in (0, 1)]
    outs = [p.communicate(timeout=180)[0] for p in procs]
    for r, out in enumerate(outs):
        line = [ln for ln in out.splitlines() if ln.startswith("RESULT")]
        assert line, out[-1500:]
        assert line[-1].split()[1:3] == [str(r), str(L.E_COMM)] and "ncclCommInitRank" in line[-1], line[-1]
    assert any("uplicate GPU" in o for o in outs), outs[0][-1500:]


@pytest.mark.parametrize("collapse,quant,leaf,T", [(2, 1, 2, 1), (2, 2, 8, 1)], ids=["default", "compact_leaf8"])
def test_lbvh_large_scene_bit_identical(collapse, quant, leaf, T):
    """0.9 M triangles (atrium at 3x tessellation): GPU build (Morton sort, Karras hierarchy, cluster boxes, device SAH top with its
    tiled levels, collapse, quantisation) against the oracle's arrays, and 100 k rays with their visit counts.  The default options,
    and the configuration that takes the most builder scratch (cost-driven collapse, compact 48 B nodes, T = 1): its bound in
    lbvh_build must hold."""
    mesh = scenes.atrium(3.0)
    assert mesh.n_triangles > 900_000
    osc = orc.Scene(mesh, leaf_size=leaf, quantized=quant, collapse=collapse, sah_top=T)
    ctx = Context(0)
    for opt, value in ((L.OPT_WIDE_COLLAPSE, collapse), (L.OPT_NODE_QUANT, quant), (L.OPT_LEAF_SIZE, leaf), (L.OPT_SAH_TOP, T)):
        ctx.set_option(opt, value)
    ctx.upload_mesh(mesh)
    ctx.build_accel()
    assert ctx.accel_info()[:3] == (osc.n_nodes, osc.n_tris, osc.max_depth)
    nodes, tris = ctx.accel_download()
    assert np.array_equal(nodes, osc.nodes()) and np.array_equal(tris, osc.tris())
    rays = rays_random(100_000, 12, [-14, 0.2, -8], [14, 12, 8])
    t, u, v, p, cn, ct, _ = ctx.trace_rays(rays, counts=True)
    ot, ou, ov, op, ocn, oct = osc.trace_closest(rays, counts=True, threads=16)
    assert np.array_equal(p, op) and np.array_equal(t[p != L.MISS], ot[p != L.MISS]) and np.array_equal(cn, ocn) and np.array_equal(ct, oct)
    ctx.close()


# ---- BASELINE.json configs, by name (C3 = test_full_size_frame_properties + the bit-exact crop of bench.py)
def test_config_c1_primary_visibility_256():
    """configs[0]: primary visibility only, 256 x 256 @ 1 spp -- the gbuffer pass against the oracle, every texel."""
    mesh = scenes.atrium(1.0)
    osc = orc.Scene(mesh)
    pt = PathTracer((256, 256))
    pt.set_scene(mesh)
    cam = Camera(scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], math.radians(scenes.ATRIUM_CAMERA["fov_deg"]), 1.0)
    g = pt.make_gconst(cam, 1, 1, flags=0)
    h = pt.commands(g, postprocess=False)
    pt.ctx.check(pt.ctx.pass_launch("gbuffer", 256, 256, 1, g, [h["gbuffer"], h["depth"]]))  # the gbuffer node alone
    pt.ctx.wait()
    gb, depth = pt.gbuffer()
    st = pt.ctx.stats()
    pt.close()
    ogb, odepth = osc.gbuffer(as_orc(g), threads=16)
    hit = odepth != orc.BACKGROUND_DEPTH
    assert np.array_equal(depth.view(np.uint32), odepth.view(np.uint32)) and np.array_equal(gb[hit], ogb[hit])
    assert st.extension_rays == 256 * 256 and st.shadow_rays == 0 and 0.5 < hit.mean() < 1.0


def test_config_c2_1080p_direct_light_whole_frame():
    """configs[1]: 1920 x 1080 @ 1 spp, BVH traversal + direct light only (one bounce: emission + sky NEE with its shadow ray),
    the WHOLE frame bit for bit against the oracle (2.07 M primary + ~1 M shadow rays: about a second on the host cores)."""
    W, H = 1920, 1080
    mesh, sky, bn = scenes.atrium(1.0), scenes.sky(2048, 1024), assets.load_bluenoise()
    g, light, gb, depth, _, st = render_both(mesh, sky, bn, None, W, H, scenes.ATRIUM_CAMERA, 1, 1, SPEC, frame=11)
    osc = orc.Scene(mesh, sky, bn)
    og = as_orc(g)
    ogb, odepth = osc.gbuffer(og, threads=16)
    assert np.array_equal(depth.view(np.uint32), odepth.view(np.uint32))
    olight, counts = osc.reference_mode(og, ogb, odepth, threads=16)
    assert np.array_equal(light.view(np.uint32), olight.view(np.uint32))
    assert st.extension_rays == W * H + int(counts[0]) and st.shadow_rays == int(counts[1]) and st.shadow_rays > 500_000


def test_config_c4_one_rank_of_eight_at_4k_256spp():
    """configs[3]: 3840 x 2160 @ 256 spp tile-split over 8 GPUs -- the share of ONE rank at full size (1.04 M pixels, 265 M paths,
    a single wavefront batch), two of its 64 x 64 tiles bit for bit against the oracle, and nothing written outside its tiles."""
    W, H, spp, B, rank, n_ranks = 3840, 2160, 256, 4, 3, 8
    mesh, sky, bn = scenes.atrium(1.0), scenes.sky(2048, 1024), assets.load_bluenoise()
    pt = PathTracer((W, H), rank=rank, n_ranks=n_ranks)
    pt.set_scene(mesh, sky, bn)
    cam = Camera(scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], math.radians(scenes.ATRIUM_CAMERA["fov_deg"]), W / H)
    g = pt.make_gconst(cam, spp, B, frame=2, flags=SPEC)
    pt.render(g)
    light = pt.light()
    st = pt.ctx.stats()
    pt.close()
    xy = orc.tile_pixels(W, H, rank, n_ranks)
    assert abs(len(xy) - W * H / n_ranks) < 0.02 * W * H / n_ranks
    mine = np.zeros((H, W), bool)
    mine[xy[:, 1], xy[:, 0]] = True
    assert (light[~mine] == 0).all() and np.isfinite(light).all() and st.extension_rays > 5e8
    osc = orc.Scene(mesh, sky, bn)
    og = as_orc(g)
    for k in (0, len(xy) // 2):  # the first pixel of a tile in render order is its top-left corner
        x0, y0 = int(xy[k, 0]) // 64 * 64, int(xy[k, 1]) // 64 * 64
        rect = (x0, y0, min(x0 + 64, W), min(y0 + 64, H))
        ogb, odepth = osc.gbuffer(og, rect=rect, threads=16)
        olight, _ = osc.reference_mode(og, ogb, odepth, rect=rect, threads=16)
        assert mine[y0:rect[3], x0:rect[2]].all()
        assert np.array_equal(olight[y0:rect[3], x0:rect[2]].view(np.uint32), light[y0:rect[3], x0:rect[2]].view(np.uint32))


def test_config_c5_progressive_accumulation_is_a_running_mean():
    """configs[4]: progressive accumulation (Light = lerp(PrevLight, pass, 1 / (p + 1))) at 4K.  Property at full size: after P passes
    the image equals the sequentially blended per-pass images (each pass rendered on its own with blendfactor 1), in fp32 with the
    shader's own lerp -- so the 4096-spp curve of tools/render.py is the running mean it claims to be."""
    W, H, spp, P = 3840, 2160, 2, 3
    mesh, sky, bn = scenes.atrium(1.0), scenes.sky(2048, 1024), assets.load_bluenoise()
    cam = Camera(scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], math.radians(scenes.ATRIUM_CAMERA["fov_deg"]), W / H)
    pt = PathTracer((W, H))
    pt.set_scene(mesh, sky, bn)
    singles = []
    for p in range(P):
        pt.render(pt.make_gconst(cam, spp, 3, frame=p, blendfactor=1.0, flags=SPEC))
        singles.append(pt.light()[..., :3].copy())
    pt.rg.upload(pt.handles["prev"], np.zeros((H, W, 4), np.float32))
    for p in range(P):
        pt.render(pt.make_gconst(cam, spp, 3, frame=p, blendfactor=1.0 / (p + 1), flags=SPEC))
        pt.copy_light_to_prev()
    acc = pt.light()[..., :3]
    pt.close()
    want = np.zeros_like(singles[0])
    for p in range(P):
        f = np.float32(1.0 / (p + 1))
        want = want + (singles[p] - want) * f
    assert np.allclose(acc, want, rtol=2e-6, atol=1e-7) and np.abs(acc - np.mean(singles, 0)).max() < 1e-3 * max(1.0, float(acc.max()))


def test_config_c5_convergence_at_length_4k():
    """configs[4] at its own size and at length, inside the GPU suite (tools/convergence.py is the 4096-spp version kept
    under profiles/): 3840 x 2160, 16 passes of 4 spp with Light / PrevLight trading names and blendfactor 1 / (pass + 1)
    (refrence_mode.slang:59-65), per-pixel RMSE of LINEAR radiance after 1, 2, 4, 8, 16 passes against an INDEPENDENT render (other frame
    seeds) of 4 x the samples.  A Monte-Carlo running mean of n samples against an independent mean of N has
    RMSE^2 = sigma^2 (1 / n + 1 / N): with the reference's own share sigma^2 / N taken off, the curve must fall by 2^-0.5 per doubling
    (slope -0.5 +- 0.06).  And the accumulation buffer after pass 8 + the pass counter are the whole state: a fresh context loaded with
    it reproduces passes 9 .. 16 bit for bit."""
    W, H, spp, P, k = 3840, 2160, 4, 16, 8
    mesh, sky, bn = scenes.atrium(1.0), scenes.sky(2048, 1024), assets.load_bluenoise()
    cam = Camera(scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], math.radians(scenes.ATRIUM_CAMERA["fov_deg"]), W / H)

    def progressive(first, last, seed0, per_pass_spp, start=None, keep=()):
        pt = PathTracer((W, H))
        pt.set_scene(mesh, sky, bn)
        if start is not None:
            pt.load_prev(start)
        kept = {}
        for p in range(first, last):
            pt.render(pt.make_gconst(cam, per_pass_spp, 4, frame=seed0 + p, blendfactor=1.0 / (p + 1), flags=SPEC), postprocess=False, wait=False)
            if p + 1 in keep:
                kept[p + 1] = pt.light()
            if p != last - 1:
                pt.swap_light_prev()
        img = pt.light()
        pt.close()
        return img, kept

    marks = (1, 2, 4, 8, 16)
    full, kept = progressive(0, P, 0, spp, keep=marks)
    n_ref = 4 * P * spp  # 256 spp as 16 passes of 16, seeds far from the first render's
    ref, _ = progressive(0, 16, 1000, n_ref // 16)
    ref = ref[..., :3].astype(np.float64)
    mse = {m: float(np.mean((kept[m][..., :3].astype(np.float64) - ref) ** 2)) for m in marks}
    sigma2 = mse[16] / (1.0 / (16 * spp) + 1.0 / n_ref)  # per-sample variance, from the finest mark
    own = {m: mse[m] - sigma2 / n_ref for m in marks}      # the running mean's own error, the reference's share removed
    slopes = [0.5 * math.log2(own[b] / own[a]) for a, b in zip(marks[:-1], marks[1:])]
    print("C5 4K: RMSE vs independent 256 spp at 4..64 spp", [round(math.sqrt(mse[m]), 4) for m in marks], "slopes per doubling", [round(x, 3) for x in slopes])
    assert all(abs(x + 0.5) <= 0.06 for x in slopes), (slopes, mse)
    assert np.array_equal(kept[16].view(np.uint32), full.view(np.uint32))
    resumed, _ = progressive(k, P, 0, spp, start=kept[k])
    assert np.array_equal(resumed.view(np.uint32), full.view(np.uint32)) and full[..., :3].mean() > 0


def test_progressive_restart_from_a_dumped_accumulation_buffer(small):
    """SURVEY 5 (checkpoint / resume) for BASELINE configs[4]: the accumulation buffer after pass k plus the pass counter are the whole
    state of a progressive render -- a fresh context loaded with that buffer as PrevLight reproduces the remaining passes bit for bit
    (tools/convergence.py does this at 4K; here a small window, Light / PrevLight trading names between passes)."""
    mesh, sky, bn, _ = small
    W, H, spp, passes, k = 128, 72, 4, 6, 3
    cam = Camera(scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], math.radians(65.0), W / H)

    def run(first, last, start=None):
        pt = PathTracer((W, H))
        pt.set_scene(mesh, sky, bn)
        if start is not None:
            pt.load_prev(start)
        dump = None
        for p in range(first, last):
            pt.render(pt.make_gconst(cam, spp, 3, frame=p, blendfactor=1.0 / (p + 1), flags=SPEC), wait=False)
            if p + 1 == k:
                dump = pt.light()
            if p != last - 1:
                pt.swap_light_prev()
        img = pt.light()
        pt.close()
        return img, dump

    full, dump = run(0, passes)
    resumed, _ = run(k, passes, start=dump)
    assert dump is not None and np.array_equal(resumed.view(np.uint32), full.view(np.uint32)) and full[..., :3].mean() > 0


def test_non_finite_rays_and_a_nan_camera(cornell):
    """Non-finite rays miss at once on both sides of the ABI; a frame whose camera matrix holds a NaN therefore comes back
    promptly with every pixel on the background instead of walking the whole tree two million times."""
    mesh, osc = cornell
    ctx = Context(0)
    ctx.upload_mesh(mesh)
    ctx.build_accel()
    rays = rays_random(4096, 5, [-0.9, 0.1, -0.9], [0.9, 1.9, 0.9])
    rng = np.random.default_rng(6)
    idx = rng.choice(4096, 600, replace=False)
    rays[rng.integers(0, 6, 600), idx] = rng.choice([np.nan, np.inf, -np.inf], 600)
    t, u, v, p, cn, ct, _ = ctx.trace_rays(rays, counts=True)
    ot, ou, ov, op, on, ont = osc.trace_closest(rays, counts=True)
    assert np.array_equal(p, op) and np.array_equal(cn, on) and np.array_equal(ct, ont) and (p[idx] == L.MISS).all() and (cn[idx] == 0).all()
    hit = p != L.MISS
    assert hit.sum() > 3000 and np.array_equal(t[hit].view(np.uint32), ot[hit].view(np.uint32))
    occ = ctx.trace_rays(rays, any_hit=True)[3]
    assert np.array_equal(occ, osc.trace_any(rays)) and (occ[idx] == 0).all()
    ctx.close()
    pt = PathTracer((320, 200))
    pt.set_scene(mesh)
    cam = Camera(scenes.CORNELL_CAMERA["position"], scenes.CORNELL_CAMERA["direction"], math.radians(40.0), 1.6)
    g = pt.make_gconst(cam, 4, 3, flags=0)
    g.view_inverse[5] = float("nan")
    pt.render(g)
    assert (pt.gbuffer()[1] == L.BACKGROUND_DEPTH).all() and (pt.light() == 0).all()
    pt.close()
