"""The HIP traversal pinned to brute force away from the origin, at other scales, on adversarial rays (GPU side of
test_traversal_exactness_cpu.py, whose docstring states the pass criterion).

On top of that criterion every GPU result equals the oracle's bit for bit: node and triangle arrays, closest hits, any hits and the
per-ray node / triangle counts.  Covered: Context.trace_rays in every node layout the options allow, instance mode 1 (shared
bottom trees under a top tree) with placements around 1e4 against mode 0 and the oracle, one path-traced frame of the atrium moved by
1e4 (k_extend, k_shadow), and trees deep enough to need the spill part of the traversal stack, plus the depth error one level deeper."""
import numpy as np
import pytest

import orc
from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from raytracer3_amd.render_graph import Context
from support import as_orc, bits, rotation, soup_mesh
from test_gpu_parity import render_both
from test_traversal_exactness_cpu import (DISPUTED_MAX, LAYOUTS, PLACEMENTS, SCENES, base_mesh, brute, check_against_brute,
                                          interval_rays, placed, ray_families)

pytestmark = pytest.mark.gpu


def all_rays(mesh, osc, seed):
    fams = ray_families(mesh, n=1000, seed=seed)
    fams["interval"] = interval_rays(osc, np.concatenate([fams["random"], fams["vertex"]], 1))
    return fams


def check_gpu(tag, ctx, osc, rays, ref, dp, disputed_max):
    """closest, any and counted closest hit: GPU = oracle bit for bit, and the oracle's criterion against brute force"""
    t, u, v, p, _ = ctx.trace_rays(rays)
    ot, ou, ov, op = osc.trace_closest(rays)
    assert np.array_equal(p, op) and np.array_equal(bits(t), bits(ot)) and np.array_equal(bits(u), bits(ou)) and np.array_equal(bits(v), bits(ov)), tag
    occ = ctx.trace_rays(rays, any_hit=True)[3]
    assert np.array_equal(occ != 0, osc.trace_any(rays) != 0), tag
    ct_, cu, cv, cp, cn, cnt, _ = ctx.trace_rays(rays, counts=True)
    _, _, _, _, ocn, ocnt = osc.trace_closest(rays, counts=True)
    assert np.array_equal(cp, p) and np.array_equal(bits(ct_), bits(t)) and np.array_equal(cn, ocn) and np.array_equal(cnt, ocnt), tag
    return check_against_brute(tag, (t, u, v, p), occ, ref, dp, disputed_max)


def layout_context(leaf, width, quant, collapse):
    ctx = Context(0)
    ctx.set_option(L.OPT_LEAF_SIZE, leaf)
    ctx.set_option(L.OPT_NODE_WIDTH, width)
    ctx.set_option(L.OPT_NODE_QUANT, quant)
    ctx.set_option(L.OPT_WIDE_COLLAPSE, collapse)
    return ctx


@pytest.mark.parametrize("scale,offset", PLACEMENTS, ids=lambda x: str(x))
@pytest.mark.parametrize("name", SCENES)
def test_trace_rays_equal_brute_force(name, scale, offset):
    mesh = placed(base_mesh(name), scale, offset)
    ref_sc = orc.Scene(mesh)
    batches = {fam: (rays, *brute(ref_sc, rays)) for fam, rays in all_rays(mesh, ref_sc, seed=17).items()}
    for lay in LAYOUTS:
        osc = orc.Scene(mesh, leaf_size=lay[0], node_width=lay[1], quantized=lay[2], collapse=lay[3])
        ctx = layout_context(*lay)
        try:
            ctx.upload_mesh(mesh)
            ctx.build_accel()
            assert ctx.accel_info()[:3] == (osc.n_nodes, osc.n_tris, osc.max_depth)
            nodes, tris = ctx.accel_download()
            assert np.array_equal(tris, osc.tris()) and np.array_equal(nodes, osc.nodes()), (name, scale, offset, lay)
            for fam, (rays, ref, dp) in batches.items():
                check_gpu(f"{name} x{scale} +{offset} layout {lay} {fam}", ctx, osc, rays, ref, dp, DISPUTED_MAX[fam])
        finally:
            ctx.close()


def far_instances(seed=9, n=12, at=(1e4, 1.2e4, -1e4)):
    """the Cornell `tall` block placed n times around `at`: random rotations, non-uniform scales, translations a few units apart"""
    room = scenes.cornell()
    t = room.names.index("tall")
    rng = np.random.default_rng(seed)
    inst = []
    for _ in range(n):
        m = np.eye(4)
        m[:3, :3] = rotation(rng) @ np.diag(rng.uniform(0.3, 1.7, 3))
        m[:3, 3] = np.asarray(at) + rng.uniform(-3, 3, 3)
        inst.append((t, 1, m.astype(np.float32)))
    return room, inst


def test_two_level_far_from_origin_equals_flattened_and_brute_force():
    """instance mode 1 (object-space bottom trees, widened boxes, tl_pad) against mode 0, the oracle and brute force"""
    room, inst = far_instances()
    osc = orc.Scene(room, instances=inst)
    world = osc.tris()[:, :9].copy().view(np.float32).reshape(-1, 3, 3)
    fams = all_rays(soup_mesh(world), osc, seed=23)
    c0, c1 = Context(0), Context(0)
    try:
        for c, mode in ((c0, 0), (c1, 1)):
            c.upload_mesh(room)
            c.set_instances(inst)
            c.set_option(L.OPT_INSTANCE_MODE, mode)
            c.build_accel()
        nodes, tris = c0.accel_download()
        assert np.array_equal(tris, osc.tris()) and np.array_equal(nodes, osc.nodes())
        assert c1.accel_levels()[0] == 1  # one shared bottom tree
        for fam, rays in fams.items():
            ref, dp = brute(osc, rays)
            check_gpu(f"mode 0 {fam}", c0, osc, rays, ref, dp, DISPUTED_MAX[fam])
            t0, u0, v0, p0, _ = c0.trace_rays(rays)
            t1, u1, v1, p1, _ = c1.trace_rays(rays)
            assert np.array_equal(p1, p0) and np.array_equal(bits(t1), bits(t0)) and np.array_equal(bits(u1), bits(u0)) and np.array_equal(bits(v1), bits(v0)), fam
            assert np.array_equal(c1.trace_rays(rays, any_hit=True)[3] != 0, c0.trace_rays(rays, any_hit=True)[3] != 0), fam
            cp1 = c1.trace_rays(rays, counts=True)
            assert np.array_equal(cp1[3], p0) and np.array_equal(bits(cp1[0]), bits(t0)), fam
            check_against_brute(f"mode 1 {fam}", (t1, u1, v1, p1), None, ref, dp, DISPUTED_MAX[fam])
    finally:
        c0.close()
        c1.close()


def test_frame_parity_atrium_far_from_origin():
    """the atrium and its camera moved by 1e4: G-buffer and radiance equal the oracle's bit for bit (k_extend and k_shadow)"""
    off = np.array([1e4, 1e4, 1e4])
    mesh = placed(scenes.atrium(0.3), 1.0, off)
    sky, bn = scenes.sky(512, 256), assets.load_bluenoise()
    osc = orc.Scene(mesh, sky, bn)
    cam = dict(scenes.ATRIUM_CAMERA)
    cam["position"] = tuple(float(np.float32(p + o)) for p, o in zip(cam["position"], off))
    W, H = 128, 72
    flags = L.F_NEE_SKY | L.F_BLUENOISE | L.F_FACEFORWARD | L.F_SPECULAR
    g, light, gb, depth, color, st = render_both(mesh, sky, bn, osc, W, H, cam, 4, 4, flags, frame=2)
    og = as_orc(g)
    ogb, odepth = osc.gbuffer(og)
    assert np.array_equal(bits(depth), bits(odepth))
    hit = depth != L.BACKGROUND_DEPTH
    assert hit.mean() > 0.5
    assert np.array_equal(gb[hit], ogb[hit])
    olight, counts = osc.reference_mode(og, ogb, odepth)
    assert np.array_equal(bits(light), bits(olight))
    assert st.extension_rays == W * H + int(counts[0]) and st.shadow_rays == int(counts[1])


def deep_stack(n_clusters, per=256, seed=3):
    """the same cluster of `per` triangles stacked at geometric scales 2^-k, k = 0 .. n_clusters - 1, each in the corner of the
    previous one: every cluster adds levels to the tree"""
    rng = np.random.default_rng(seed)
    proto = rng.uniform(-0.3, 0.3, (per, 1, 3)) + rng.normal(size=(per, 3, 3)) * 0.02
    v = np.concatenate([(proto + 1.0) * 0.5 ** k for k in range(n_clusters)]).astype(np.float32)
    return soup_mesh(v), v


def deep_stack_rays(v, n_clusters, per=256, m=400, seed=4):
    """rays from 1.5 to 6 cluster sizes outside each cluster (away from the smaller ones), aimed at its triangles' vertices and
    interiors, with tmax a tenth of a cluster size past the target: the ray never reaches a cluster so much smaller than its distance
    that the fp32 triangle test is inexact there (criterion 3 of test_traversal_exactness_cpu.py)"""
    rng = np.random.default_rng(seed)
    rays = []
    for k in range(n_clusters):
        s = 0.5 ** k
        tri = v[k * per:(k + 1) * per][rng.integers(0, per, m)].astype(np.float64)
        tgt = np.einsum("mi,mij->mj", rng.dirichlet([0.5, 0.5, 0.5], m), tri)
        tgt[: m // 4] = tri[: m // 4, 0]
        out = np.abs(rng.normal(size=(m, 3)))
        o = (s + out / np.linalg.norm(out, axis=1, keepdims=True) * rng.uniform(1.5, 6, (m, 1)) * s).astype(np.float32)
        d = tgt - o
        dist = np.linalg.norm(d, axis=1)
        d = (d / dist[:, None]).astype(np.float32)
        rays.append(np.concatenate([o.T, d.T, np.zeros((1, m)), (dist + 0.1 * s)[None]]).astype(np.float32))
    return np.ascontiguousarray(np.concatenate(rays, 1))


def test_deep_tree_uses_the_spill_stack_and_depth_error():
    mesh, v = deep_stack(20)
    osc = orc.Scene(mesh)
    ctx = Context(0)
    try:
        ctx.upload_mesh(mesh)
        ctx.build_accel()
        depth = ctx.accel_info()[2]
        assert depth == osc.max_depth and 40 <= 3 * (depth - 1) <= 64, depth  # beyond the 12 LDS entries, within the 64
        nodes, tris = ctx.accel_download()
        assert np.array_equal(nodes, osc.nodes()) and np.array_equal(tris, osc.tris())
        rays = deep_stack_rays(v, 20)
        ref, dp = brute(osc, rays)
        assert (ref[3] != orc.MISS).mean() > 0.5
        check_gpu("deep stack", ctx, osc, rays, ref, dp, DISPUTED_MAX["vertex"])
        cn = ctx.trace_rays(rays, counts=True)[4]
        assert cn.max() > 12
        # one level deeper: the build refuses it with a clean message, and the same context goes on with a normal scene
        deeper, _ = deep_stack(28)
        assert orc.Scene(deeper).max_depth > 22
        ctx.upload_mesh(deeper)
        with pytest.raises(L.Rt3Error) as e:
            ctx.build_accel()
        assert e.value.code == L.E_DEPTH and "stack entries" in str(e.value), e.value
        cornell = scenes.cornell()
        ocn = orc.Scene(cornell)
        ctx.upload_mesh(cornell)
        ctx.build_accel()
        fams = ray_families(cornell, n=500, seed=2)
        for fam, r in fams.items():
            ref, dp = brute(ocn, r)
            check_gpu(f"after depth error {fam}", ctx, ocn, r, ref, dp, DISPUTED_MAX[fam])
    finally:
        ctx.close()
