"""Skinning on the MI355X: k_skin_pose equals tests/ref_skin.py bit for bit through rt3_scene_download_vertices, over
skin sizes around the wave and group sizes, vertex offsets, joint and target counts, guards that keep every word, a NULL rest and a second
pose; every refusal leaves the vertices and rt3_skin_info as they were; an out-of-range pose stops the refit until a valid one; a posed and
refitted structure traces like a fresh one given the same vertices, in both instance modes; the deformation history sees the pose like an
update; and PathTracer.pose equals update_vertices with the reference's vertices over a temporal sequence."""
import ctypes as C

import numpy as np
import pytest

import motion_worlds as mw
import orc
import ref_deform as rdf
import ref_motion as rm
import skin_worlds as sw
from raytracer3_amd import _lib as L
from raytracer3_amd import scenes
from raytracer3_amd.assets import Material, MeshBuilder
from raytracer3_amd.render_graph import Context
from support import as_orc, bits, err, launch, same, tracer
from test_motion import gconst, motion_image, run_motion

pytestmark = pytest.mark.gpu
F = np.float32
# a guard record: finite position words (rt3_scene_set_vertices checks those), arbitrary words behind them
GUARD = np.array([0x3F9D70A4, 0xC0123456, 0x40490FDB, 0x7FC12345, 0xFFC54321, 0x12345678, 0x9ABCDEF0, 0x0BADF00D], np.uint32).view(F)


def soup(n_vertices):
    """a mesh of n_vertices guard records and one triangle (the skins of these tests index vertices, not triangles)"""
    mb = MeshBuilder()
    mb.add("soup", np.zeros((n_vertices, 3)), np.tile([0, 0, 1.0], (n_vertices, 1)), None, [[0, 1, 2]] if n_vertices >= 3 else np.zeros((0, 3)), Material())
    m = mb.build()
    m.vertices = np.tile(GUARD, (n_vertices, 1))
    return m


def add(ctx, first, r, rest=True):
    return ctx.add_skin(first, r["joints"], r["weights"], r["n_joints"], r["rest"] if rest else None, r["dpos"], r["dnrm"])


# ------------------------------------------------------------------------------------------------ 1. the kernel equals the reference
@pytest.mark.parametrize("n,first,n_joints,n_targets,with_dnrm", [(1, 0, 1, 0, False), (63, 7, 2, 1, False), (64, 0, 300, 8, True), (65, 7, 2, 1, True),
                                                                 (255, 0, 300, 0, False), (257, 7, 1, 8, False), (1025, 7, 300, 1, True)])
def test_kernel_equals_the_reference_bit_for_bit(n, first, n_joints, n_targets, with_dnrm):
    ra = sw.rows(n, n_joints, n_targets, with_dnrm, seed=n)
    rb = sw.rows(65, 2, 0, seed=n + 1)
    first_b = first + n + 5
    total = first_b + 65 + 3
    mesh = soup(total)
    mesh.vertices[first_b:first_b + 65] = rb["rest"]  # skin B takes its rest pose from the buffer (rest = NULL)
    ctx = Context()
    ctx.upload_mesh(mesh)
    a, b = add(ctx, first, ra), add(ctx, first_b, rb, rest=False)
    assert (a, b) == (0, 1) and ctx.skin_info()[0] == 2
    want = mesh.vertices.copy()
    assert np.array_equal(bits(ctx.download_vertices(0, total)), bits(want))  # rt3_scene_add_skin does not touch the buffer
    pal_a, pal_b = sw.palette(n_joints, seed=2, spread=2.0), sw.palette(2, seed=3)
    other = pal_a.copy()
    other[:, :3, :] *= F(1.5)
    ctx.pose_skin(a, other, None if ra["a"] is None else ra["a"] * F(0.5))  # a first pose, overwritten by the second
    ctx.pose_skin(a, pal_a, ra["a"])
    ctx.pose_skin(b, pal_b)
    want[first:first + n] = sw.pose_rows(ra, pal_a)
    want[first_b:first_b + 65] = sw.pose_rows(rb, pal_b)
    got = ctx.download_vertices(0, total)
    diff = (bits(got) != bits(want)).any(1)
    assert not diff.any(), f"{int(diff.sum())} records differ, first at {np.flatnonzero(diff)[:5].tolist()}"
    guards = np.ones(total, bool)
    guards[first:first + n] = guards[first_b:first_b + 65] = False
    assert guards.sum() == first + 5 + 3 and np.array_equal(bits(got[guards]), np.broadcast_to(bits(GUARD), (int(guards.sum()), 8)))
    # posing B again from the same rest: the pose does not accumulate; rest = NULL was the buffer's contents at rt3_scene_add_skin
    ctx.pose_skin(b, pal_b)
    assert np.array_equal(bits(ctx.download_vertices(first_b, 65)), bits(want[first_b:first_b + 65]))
    # a partial download
    assert np.array_equal(bits(ctx.download_vertices(first + n - 1, 3)), bits(want[first + n - 1:first + n + 2]))
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. refusals
def desc(first, r, **kw):
    keep = [np.ascontiguousarray(r["rest"], F), np.ascontiguousarray(r["joints"], np.uint16), np.ascontiguousarray(r["weights"], F),
            None if r["dpos"] is None else np.ascontiguousarray(r["dpos"], F), None if r["dnrm"] is None else np.ascontiguousarray(r["dnrm"], F)]
    d = L.SkinDesc(first, len(keep[0]), r["n_joints"], 0 if keep[3] is None else len(keep[3]), *[None if k is None else k.ctypes.data for k in keep])
    for k, v in kw.items():
        setattr(d, k, v)
    d._keep = keep
    return d


def test_refusals_change_nothing():
    total = 200
    mesh = soup(total)
    fresh = Context()
    r = sw.rows(40, 4, 2, True, seed=1)
    out = C.c_uint32(99)
    assert fresh.lib.rt3_scene_add_skin(fresh.h, C.byref(desc(0, r)), C.byref(out)) == L.E_STATE and "rt3_scene_set_vertices" in fresh.last_error()
    assert fresh.lib.rt3_scene_download_vertices(fresh.h, None, 0, 0) == L.E_STATE
    fresh.close()
    ctx = Context()
    lib = ctx.lib
    ctx.upload_mesh(mesh)
    s0 = add(ctx, 10, r)
    ctx.pose_skin(s0, sw.palette(4), r["a"])
    before, info = ctx.download_vertices(0, total), ctx.skin_info()
    assert info == (1, 40 * (32 + 8 + 16) + 2 * 2 * 40 * 12 + 4 * 48 + 4)  # rest, joints, weights; two targets' dP and dN; the palette; the flag

    def refused(code, call, what):
        assert call() == code, (what, ctx.last_error())
        assert np.array_equal(bits(ctx.download_vertices(0, total)), bits(before)) and ctx.skin_info() == info, what

    def bad(what, first=60, **change):
        rr = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}
        for k, (index, value) in change.items():
            rr[k][index] = value
        refused(L.E_INVALID, lambda: lib.rt3_scene_add_skin(ctx.h, C.byref(desc(first, rr)), None), what)

    bad("a range past the vertex buffer", first=total - 39)
    bad("a range that overlaps another skin's (its last vertex)", first=49)
    bad("a range that overlaps another skin's (its first vertex)", first=0)
    bad("a joint index >= n_joints", joints=((5, 2), 4))
    bad("a negative weight", weights=((7, 1), F(-0.25)))
    bad("a weight that is not finite", weights=((7, 1), F(np.inf)))
    bad("a NaN weight", weights=((0, 0), F(np.nan)))
    bad("a rest position that is not finite", rest=((39, 2), F(np.nan)))
    bad("a rest position beyond 1e18", rest=((0, 0), F(2e18)))
    bad("a position delta that is not finite", dpos=((1, 39, 2), F(np.inf)))
    bad("a normal delta that is not finite", dnrm=((0, 0, 0), F(np.nan)))
    for what, kw in (("n_joints 0", dict(n_joints=0)), ("n_joints 65537", dict(n_joints=65537)), ("nine targets", dict(n_targets=9)),
                     ("an empty range", dict(n_vertices=0)), ("joints NULL", dict(joints=None)), ("weights NULL", dict(weights=None)),
                     ("targets without deltas", dict(target_dpos=None)), ("deltas without targets", dict(n_targets=0))):
        refused(L.E_INVALID, lambda: lib.rt3_scene_add_skin(ctx.h, C.byref(desc(60, r, **kw)), None), what)
    refused(L.E_INVALID, lambda: lib.rt3_scene_add_skin(ctx.h, None, None), "a NULL description")
    # a rest record may carry any normal and uv words
    ok = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}
    ok["rest"][3, 4] = F(np.nan)
    s1 = add(ctx, 60, ok)
    info = ctx.skin_info()
    assert s1 == 1 and info[0] == 2
    # poses
    pal = np.ascontiguousarray(sw.palette(4).transpose(0, 2, 1))  # column-major
    a = np.ascontiguousarray(r["a"], F)

    def pose(skin, m, w):
        return lib.rt3_scene_pose_skin(ctx.h, skin, None if m is None else m.ctypes.data, None if w is None else w.ctypes.data)

    for what, change in (("a matrix that is not finite", ((2, 1, 1), np.nan)), ("a last row that is not (0, 0, 0, 1)", ((3, 0, 3), 0.5)),
                         ("a last row whose 1 is not 1", ((0, 3, 3), 2.0)), ("an infinite translation", ((1, 3, 0), np.inf))):
        m = pal.copy()
        m[change[0]] = change[1]
        refused(L.E_INVALID, lambda: pose(s0, m, a), what)
    refused(L.E_INVALID, lambda: pose(s0, pal, np.array([0.5, np.inf], F)), "a target weight that is not finite")
    refused(L.E_INVALID, lambda: pose(s0, pal, None), "target weights NULL for a skin with targets")
    refused(L.E_INVALID, lambda: pose(s0, None, a), "matrices NULL")
    refused(L.E_INVALID, lambda: pose(2, pal, a), "a skin that does not exist")
    assert lib.rt3_scene_pose_skin(None, 0, pal.ctypes.data, a.ctypes.data) == L.E_INVALID
    buf = np.zeros((4, 8), F)
    refused(L.E_INVALID, lambda: lib.rt3_scene_download_vertices(ctx.h, buf.ctypes.data, total - 3, 4), "a download past the buffer")
    # rt3_scene_update_vertices on a skinned range is allowed, and the next pose overwrites it
    ctx.update_vertices(np.tile(GUARD, (40, 1)), 10)
    assert np.array_equal(bits(ctx.download_vertices(10, 40)), np.broadcast_to(bits(GUARD), (40, 8)))
    ctx.pose_skin(s0, sw.palette(4), r["a"])
    assert np.array_equal(bits(ctx.download_vertices(0, total)), bits(before))
    # rt3_scene_set_indices and rt3_scene_set_geometry keep the skins; rt3_scene_clear_skins and rt3_scene_set_vertices drop them
    i, geo, pc = np.ascontiguousarray(mesh.indices, np.uint32), np.ascontiguousarray(mesh.geometries), np.ascontiguousarray(mesh.prim_counts, np.uint32)
    assert lib.rt3_scene_set_indices(ctx.h, i.ctypes.data, len(i)) == 0 and lib.rt3_scene_set_geometry(ctx.h, geo.ctypes.data, pc.ctypes.data, len(geo)) == 0
    assert ctx.skin_info() == info
    v = np.ascontiguousarray(mesh.vertices, F)
    assert lib.rt3_scene_set_vertices(ctx.h, v.ctypes.data, len(v)) == 0
    assert ctx.skin_info() == (0, 0) and pose(0, pal, a) == L.E_INVALID
    assert np.array_equal(bits(ctx.download_vertices(0, total)), bits(v))
    assert add(ctx, 10, r) == 0  # (the indices start over)
    ctx.clear_skins()
    assert ctx.skin_info() == (0, 0)
    ctx.close()


def test_a_pose_out_of_range_stops_the_refit_until_a_valid_one():
    W, H = 64, 48
    arm = scenes.skinned_arm()
    pt = tracer(arm, (W, H))
    g = gconst(pt, scenes.SKINNED_ARM_CAMERA)
    img = motion_image(pt)
    (pal, w), = arm.pose(0.6)
    assert launch(pt, "motion", W, H, 1, g, [img]) == 0
    huge = pal.copy()
    huge[:, :3, :] *= F(1e30)  # (finite, so the pose is accepted; the positions it makes are not within 1e18)
    assert np.isfinite(huge).all()
    pt.ctx.pose_skin(0, huge, w)
    for _ in range(2):  # the flag stays set until the skin is posed again
        assert pt.ctx.lib.rt3_accel_refit(pt.ctx.h, None) == L.E_INVALID and "skin 0: a posed position is not finite" in err(pt)
        assert launch(pt, "motion", W, H, 1, g, [img]) == L.E_STATE and "vertices were updated" in err(pt)
    assert pt.ctx.lib.rt3_accel_build(pt.ctx.h, None) == L.E_INVALID and "skin 0" in err(pt)
    assert launch(pt, "motion", W, H, 1, g, [img]) == L.E_STATE
    pt.ctx.pose_skin(0, pal, w)
    pt.ctx.refit_accel()
    assert launch(pt, "motion", W, H, 1, g, [img]) == 0
    assert np.array_equal(bits(pt.ctx.download_vertices(0, len(arm.vertices))), bits(sw.arm_vertices(arm, 0.6)))
    pt.close()


# ------------------------------------------------------------------------------------------------ 3. the structure
def arm_instances(arm, twice):
    """the room under the identity and the arm once, or twice: once where it stands and once to its left, turned and scaled (with the CPU
    oracle the two placements cover 9.5 % and 5.9 % of the 128 x 128 rays at t = 0.8)"""
    g = len(arm.geometries) - 1
    inst = [(0, g, mw.EYE), (g, 1, mw.EYE)]
    if twice:
        inst.append((g, 1, mw.f32(mw.translate(-0.75, 0.0, 0.1) @ mw.rot_y(40.0) @ mw.scale(0.8, 0.9, 0.8))))
    return inst


@pytest.mark.parametrize("mode,twice", [(0, False), (0, True), (1, False), (1, True)])
def test_posed_structure_traces_like_one_given_the_same_vertices(mode, twice):
    arm = scenes.skinned_arm()
    inst = arm_instances(arm, twice)
    t = 0.8
    posed = tracer(arm, (128, 128), instances=inst, mode=mode)
    for k, (pal, w) in enumerate(arm.pose(t)):
        posed.ctx.pose_skin(k, pal, w)
    posed.ctx.refit_accel()
    fed = tracer(arm, (128, 128), instances=inst, mode=mode)
    fed.ctx.update_vertices(sw.arm_vertices(arm, t))
    fed.ctx.refit_accel()
    g = as_orc(gconst(posed, scenes.SKINNED_ARM_CAMERA))
    ys, xs = np.meshgrid(np.arange(128, dtype=np.uint32), np.arange(128, dtype=np.uint32), indexing="ij")
    rays = orc.primary_rays(g, xs.ravel(), ys.ravel())
    assert rays.shape[1] == 1 << 14
    a, b = posed.ctx.trace_rays(rays)[:4], fed.ctx.trace_rays(rays)[:4]
    for x, y, name in zip(a, b, "tuvp"):
        assert np.array_equal(bits(x), bits(y)), name
    first_arm = int(arm.prim_counts[:-1].sum())
    on_arm = (a[3] != L.MISS) & (a[3] >= first_arm)
    assert on_arm.mean() > 0.02
    if twice:
        second = on_arm & (a[3] >= first_arm + int(arm.prim_counts[-1]))
        assert second.mean() > 0.02 and (on_arm & ~second).mean() > 0.02  # both placements are seen
    # ... and not like the rest pose
    rest = tracer(arm, (128, 128), instances=inst, mode=mode)
    assert not np.array_equal(bits(rest.ctx.trace_rays(rays)[0]), bits(a[0]))
    for pt in (posed, fed, rest):
        pt.close()


# ------------------------------------------------------------------------------------------------ 4. the history
def test_a_pose_after_a_snapshot_is_a_deformation():
    W, H = 96, 64
    arm = scenes.skinned_arm()
    ng = len(arm.geometries)
    inst = [(0, ng, mw.EYE)]
    pt = tracer(arm, (W, H), instances=inst)
    pt.ctx.snapshot_vertices()
    assert not pt.ctx.deformed_geometries(ng).any()
    for k, (pal, w) in enumerate(arm.pose(1.0)):
        pt.ctx.pose_skin(k, pal, w)
    pt.ctx.refit_accel()
    assert pt.ctx.deformed_geometries(ng).tolist() == [name == "arm" for name in arm.names]
    now = sw.posed(arm, 1.0)
    g = gconst(pt, scenes.SKINNED_ARM_CAMERA)
    og = as_orc(g)
    hits = rm.primary_hits(orc.Scene(now, instances=inst), og)
    want = rdf.motion(now, arm.vertices, inst, None, og, hits)
    got = run_motion(pt, g)
    assert (want[..., 3] == 3).mean() >= 0.02
    same(got, want, "Motion after snapshot and pose")
    # the next snapshot copies the posed range: nothing is deformed, and a pose back to the rest pose is a deformation again
    pt.ctx.snapshot_vertices()
    assert not pt.ctx.deformed_geometries(ng).any()
    pt.close()


# ------------------------------------------------------------------------------------------------ 5. PathTracer.pose
def test_pathtracer_pose_equals_update_vertices_with_the_reference_vertices():
    W, H = 96, 64
    arm = scenes.skinned_arm()
    times = [0.3, 0.7, 1.1, 1.6]
    first_arm = int(arm.prim_counts[:-1].sum())
    frames = {}
    for how in ("pose", "update"):
        pt = tracer(arm, (W, H))
        frames[how] = []
        for k, t in enumerate(times):
            if how == "pose":
                pt.pose(t)
            else:
                pt.update_vertices(sw.arm_vertices(arm, t))
            g = gconst(pt, scenes.SKINNED_ARM_CAMERA, 1, k + 1, k)
            h = pt.render(g, temporal=True)
            assert ("motion" in h) == (k > 0)
            hist, mom = pt.history()
            frames[how].append((pt.accumulated(), hist, mom, pt.motion() if k else None))
            if how == "pose":  # the arm is in view, in every frame: the comparison is not one of empty images
                prim = rm.primary_hits(orc.Scene(sw.posed(arm, t)), as_orc(g))[3]
                share = float(((prim != orc.MISS) & (prim >= first_arm)).mean())
                print(f"frame {k} (t = {t}): the arm covers {share:.3f} of the pixels")
                assert share >= 0.02
        pt.close()
    for k, (a, b) in enumerate(zip(frames["pose"], frames["update"])):
        for x, y, name in zip(a, b, ("Out", "History", "Moments", "Motion")):
            if x is not None:
                same(x, y, f"frame {k} {name}")
        if k:
            assert (a[3][..., 3] == 3).mean() >= 0.02  # the arm keeps its history as a deformed geometry
