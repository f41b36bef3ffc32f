"""Previous vertex positions for the "motion" pass on the MI355X: the compare kernel's flags equal
ref_deform.deformed_flags in every case of the span rule; Motion equals tests/ref_deform.py bit for bit in both instance modes, at two
windows, under a tile partition, with and without previous transforms; without a snapshot nothing changes; sequences of a waving cloth,
bending blocks, moving instances and a moving camera, chained into "denoise", equal the reference and each other across the instance
modes; the cloth keeps more history with the feature than without; the documented errors; determinism; and the PathTracer path.  The hits
come from the oracle's traversal of the deformed world, which test_refit.py pins the GPU's primary trace to."""
import copy

import numpy as np
import pytest

import deform_worlds as dw
import motion_worlds as mw
import orc
import ref_deform as rdf
import ref_motion as rm
import ref_temporal as rt
from raytracer3_amd import _lib as L
from raytracer3_amd.assets import Material, MeshBuilder
from support import as_orc, bits, err, launch, same, tracer
from test_motion import SENTINEL, gconst, motion_image, run_motion

pytestmark = pytest.mark.gpu
BG = np.float32(orc.BACKGROUND_DEPTH)
F = np.float32


# ------------------------------------------------------------------------------------------------ 1. the compare kernel
def chunk_mesh():
    """3000 vertices (about three chunks of the compare kernel) under five geometries: `short` spans 36 vertices (less than a wave),
    `long` 1501 (it crosses a chunk boundary wherever its chunks start), `left` and `right` share the vertices 2200..2300, `offset`
    reaches its span through a vertex offset"""
    rng = np.random.default_rng(5)
    n = 3000
    pos = rng.uniform(-1.0, 1.0, (n, 3))
    pos[20] = (0.0, 0.25, 0.5)  # a zero word inside `short`
    mb = MeshBuilder()
    mb.add("all", pos, np.tile([0, 0, 1.0], (n, 1)), None, [[0, 1, 2]], Material())
    m = mb.build()
    spans = [("short", 0, 5, 40), ("long", 0, 100, 1600), ("left", 0, 1700, 2300), ("right", 0, 2200, 2900), ("offset", 2900, 10, 90)]
    idx, geoms, counts = [], [], []
    for name, vo, lo, hi in spans:
        g = m.geometries[0].copy()
        g["index_offset"], g["vertex_offset"] = len(idx), vo
        idx += [lo, lo + 1, hi, lo + 2, lo + 3, hi - 1]
        geoms.append(g)
        counts.append(2)
    m.indices, m.geometries, m.prim_counts, m.names = np.array(idx, np.uint32), np.array(geoms, m.geometries.dtype), np.array(counts, np.uint32), [s[0] for s in spans]
    m.alpha_cutoffs = np.zeros(len(spans), F)
    return m


def test_compare_kernel_follows_the_span_rule():
    from raytracer3_amd.render_graph import Context

    mesh = chunk_mesh()
    assert rdf.spans(mesh) == [(5, 40), (100, 1600), (1700, 2300), (2200, 2900), (2910, 2990)]
    ng = len(mesh.geometries)
    ctx = Context()
    lib = ctx.lib
    flags = np.zeros(ng, np.uint8)
    assert lib.rt3_scene_snapshot_vertices(ctx.h) == L.E_STATE  # before any vertices
    ctx.upload_mesh(mesh)
    assert lib.rt3_scene_deformed_geometries(ctx.h, flags.ctypes.data, ng) == L.E_STATE  # no snapshot yet
    cur = mesh.vertices.copy()
    state = dict(snap=None)

    def snapshot():
        ctx.snapshot_vertices()
        state["snap"] = cur.copy()

    def update(first, rows):
        rows = np.ascontiguousarray(rows, F).reshape(-1, 8)
        cur[first:first + len(rows)] = rows
        ctx.update_vertices(rows, first)

    def poke(vertex, word, value=None, lo=None, hi=None):
        """change one word and send the rows [lo, hi) (default: the vertex alone)"""
        lo, hi = (vertex, vertex + 1) if lo is None else (lo, hi)
        rows = cur[lo:hi].copy()
        rows[vertex - lo, word] = rows[vertex - lo, word] + F(0.5) if value is None else value
        update(lo, rows)

    def check(want_names, what):
        now = copy.copy(mesh)
        now.vertices = cur
        want = rdf.deformed_flags(now, state["snap"])
        assert [mesh.names[i] for i in np.flatnonzero(want)] == want_names, what  # the case is the one meant
        got = ctx.deformed_geometries(ng)
        assert got.tolist() == want.tolist(), (what, got.tolist(), want.tolist())

    snapshot()
    check([], "a snapshot, no update")
    for vertex, names, what in ((5, ["short"], "first vertex of a span"), (40, ["short"], "last vertex of a span"), (4, [], "just below a span"),
                                (41, [], "just above a span"), (1600, ["long"], "last vertex of the long span"), (99, [], "just below the long span"),
                                (2250, ["left", "right"], "a shared vertex"), (2200, ["left", "right"], "first shared vertex"),
                                (2301, ["right"], "just above `left`"), (2910, ["offset"], "first vertex through a vertex offset"),
                                (2909, [], "just below it"), (2991, [], "just above it"), (2950, ["offset"], "inside the span, indexed by no triangle")):
        poke(vertex, vertex % 3)
        check(names, what)
        snapshot()
        check([], what + ", after the next snapshot")
    poke(20, 0, F(-0.0))
    assert cur[20, 0] == 0 and np.signbit(cur[20, 0])
    check(["short"], "-0 for +0")
    snapshot()
    for word in (3, 5, 7):
        poke(30, word)
    check([], "normal and uv words only")
    # the whole buffer again with equal words, then with one change far into it: the spans' chunks cover every vertex
    update(0, cur.copy())
    check([], "the whole buffer re-sent")
    poke(1600, 2, lo=0, hi=len(cur))
    check(["long"], "the whole buffer, the change in the long span's second chunk")
    snapshot()
    # a partial range that starts inside the long span and crosses two chunk boundaries of its own
    poke(1599, 1, lo=300, hi=2750)
    check(["long"], "a partial range")
    snapshot()
    poke(2899, 0, lo=2250, hi=2950)
    check(["right"], "a partial range over three spans, the change in one")
    snapshot()
    # two updates before one launch, then a third that touches the first two ranges
    poke(10, 1)
    poke(2500, 2)
    check(["short", "right"], "two updates before one launch")
    poke(1000, 0, lo=8, hi=2600)
    check(["short", "long", "right"], "three updates, merged ranges")
    # the data decides, not the calls: the old words again
    update(0, state["snap"].copy())
    check([], "the snapshot's words sent back")
    # a snapshot taken twice
    poke(2000, 1)
    snapshot()
    snapshot()
    check([], "a snapshot taken twice")
    poke(2000, 1)
    check(["left"], "an update after the two snapshots")
    # errors and forgetting
    assert lib.rt3_scene_deformed_geometries(ctx.h, flags.ctypes.data, ng - 1) == L.E_INVALID
    assert lib.rt3_scene_deformed_geometries(ctx.h, flags.ctypes.data, ng + 1) == L.E_INVALID
    assert lib.rt3_scene_deformed_geometries(ctx.h, None, ng) == L.E_INVALID
    ctx.forget_prev_vertices()
    assert lib.rt3_scene_deformed_geometries(ctx.h, flags.ctypes.data, ng) == L.E_STATE and "snapshot" in ctx.last_error()
    snapshot()
    check([], "a first snapshot again: every vertex copied")
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. Motion equals the reference
def deformed_tracer(W, H, mode, snapshot=True):
    """a tracer built for frame 0 of the parity world whose vertices then become frame 1's (the whole buffer is sent) behind a snapshot"""
    mesh, prev_v, inst, prev = dw.parity_world()
    before = copy.copy(mesh)
    before.vertices = prev_v
    pt = tracer(before, (W, H), instances=inst, mode=mode)
    if snapshot:
        pt.ctx.snapshot_vertices()
    pt.ctx.update_vertices(mesh.vertices)
    pt.ctx.refit_accel()
    return pt, mesh, prev_v, inst, prev


@pytest.mark.parametrize("mode", [0, 1])
def test_motion_parity_windows_partition_and_previous_transforms(mode):
    for W, H in ((192, 108), (250, 187)):
        pt, mesh, prev_v, inst, prev = deformed_tracer(W, H, mode)
        assert [mesh.names[i] for i in np.flatnonzero(pt.ctx.deformed_geometries(len(mesh.geometries)))] == ["cloth", "bender", "bend2"]
        osc = orc.Scene(mesh, instances=inst)
        g = gconst(pt, dw.CAMERA)
        og = as_orc(g)
        hits = rm.primary_hits(osc, og)
        for pm in (prev, None):
            pt.ctx.set_prev_transforms(pm)
            want = rdf.motion(mesh, prev_v, inst, pm, og, hits)
            got = run_motion(pt, g)
            kinds = [float((got[..., 3] == k).mean()) for k in (0, 1, 2, 3)]
            print(f"mode {mode} {W}x{H}, previous transforms {'set' if pm else 'not set'}: miss {kinds[0]:.3f}, unmoved {kinds[1]:.3f}, "
                  f"moved {kinds[2]:.3f}, deformed {kinds[3]:.3f}")
            assert kinds[3] >= 0.02 and abs(sum(kinds) - 1.0) < 1e-12 and (min(kinds) >= 0.02 or pm is None)
            same(got, want, f"Motion, mode {mode}, {W}x{H}, previous transforms {'set' if pm else 'not set'}")
            # rank 1 of 3: its own pixels get the one-rank values, no other texel is touched
            pt.ctx.set_tile_partition(W, H, 1, 3)
            part = run_motion(pt, g)
            pt.ctx.set_tile_partition(W, H, 0, 1)
            own = np.zeros((H, W), bool)
            xy = orc.tile_pixels(W, H, 1, 3)
            own[xy[:, 1], xy[:, 0]] = True
            assert 0.1 < own.mean() < 0.6
            assert np.array_equal(bits(part[own]), bits(want[own]))
            assert np.array_equal(bits(part[~own]), np.broadcast_to(bits(SENTINEL), (int((~own).sum()), 4)))
        pt.close()


# ------------------------------------------------------------------------------------------------ 3. nothing changes without a snapshot
def test_without_a_snapshot_motion_is_what_it_was():
    W, H = 192, 108
    pt, mesh, prev_v, inst, prev = deformed_tracer(W, H, 0, snapshot=False)
    osc = orc.Scene(mesh, instances=inst)
    g = gconst(pt, dw.CAMERA)
    og = as_orc(g)
    hits = rm.primary_hits(osc, og)
    for pm in (prev, None):
        pt.ctx.set_prev_transforms(pm)
        want = rm.motion(mesh, inst, pm, og, hits)
        same(run_motion(pt, g), want, "update and refit, no snapshot")
        # a snapshot with no later update: the same bits
        pt.ctx.snapshot_vertices()
        assert not pt.ctx.deformed_geometries(len(mesh.geometries)).any()
        same(run_motion(pt, g), want, "a snapshot with no later update")
        # deformed, then forgotten
        pt.ctx.update_vertices(prev_v)
        pt.ctx.update_vertices(mesh.vertices)  # (the words of before: the data decides)
        pt.ctx.refit_accel()
        same(run_motion(pt, g), want, "the old words sent back")
        a, b = dw.vertex_range(mesh, "cloth")
        moved = mesh.vertices[a:b].copy()
        moved[:, 2] -= F(0.001)
        pt.ctx.update_vertices(moved, a)
        pt.ctx.update_vertices(mesh.vertices[a:b], a)
        pt.ctx.snapshot_vertices()
        pt.ctx.update_vertices(moved, a)
        pt.ctx.update_vertices(mesh.vertices[a:b], a)
        pt.ctx.refit_accel()
        same(run_motion(pt, g), want, "changed and restored after the snapshot")
        pt.ctx.update_vertices(moved, a)
        pt.ctx.refit_accel()
        assert pt.ctx.deformed_geometries(len(mesh.geometries)).tolist() == [n == "cloth" for n in mesh.names]
        pt.ctx.update_vertices(mesh.vertices[a:b], a)
        pt.ctx.refit_accel()
        pt.ctx.snapshot_vertices()
        pt.ctx.update_vertices(prev_v)
        pt.ctx.update_vertices(mesh.vertices)
        pt.ctx.refit_accel()
        pt.ctx.forget_prev_vertices()
        same(run_motion(pt, g), want, "after rt3_scene_forget_prev_vertices")
    pt.close()


# ------------------------------------------------------------------------------------------------ 4. and 5. sequences
def run_sequence(mode, K=4, W=160, H=120, feature=True, check=True):
    """K frames of deform_worlds.world(k) through PathTracer.update_vertices + set_instances + render(temporal=True, denoise=True); every
    frame is compared with the reference chain on the frame's own Light and the previous frame's (GPU) History and Moments.  Without
    `feature` the vertices go up past PathTracer (no snapshot).  Returns the frames' images and the last frame's cloth mask."""
    mesh, inst = dw.world(0)
    pt = tracer(mesh, (W, H), instances=inst, mode=mode)
    prev = prev_inst = prev_mesh = None
    frames = []
    for k in range(K):
        mesh, inst = dw.world(k)
        if k:
            if feature:
                pt.update_vertices(mesh.vertices)
            else:
                pt.ctx.update_vertices(mesh.vertices)
                pt.ctx.refit_accel()
            pt.set_instances(inst)
        g = gconst(pt, dw.CAMERA, 1, k + 1, k)
        h = pt.render(g, temporal=True, denoise=True)
        og = as_orc(g)
        light, out = pt.light(), pt.accumulated()
        hist, mom = pt.history()
        gb, depth = pt.gbuffer()
        M, st = None, {}
        osc = orc.Scene(mesh, instances=inst)
        if k:
            assert "motion" in h
            hits = rm.primary_hits(osc, og)
            M = rdf.motion(mesh, prev_mesh.vertices if feature else None, inst, [m for _, _, m in prev_inst], og, hits, stages=st)
            if check:
                same(pt.motion(), M, f"mode {mode} frame {k} Motion")
                assert ((M[..., 3] == 3).mean() > 0.05) == feature and (M[..., 3] == 2).mean() > 0.02
        else:
            assert "motion" not in h
            prev = (og, gb, depth, np.zeros((H, W, 4), F), np.zeros((H, W, 4), F))
        if check:
            want = rm.temporal(og, gb, depth, light, *prev, motion=M)
            for got, ref, name in zip((out, hist, mom), want, ("Out", "History", "Moments")):
                same(got, ref, f"mode {mode} frame {k} {name}")
            same(pt.denoised(), rt.denoise(og, gb, depth, out, moments=mom), f"mode {mode} frame {k} denoised")
        prev, prev_inst, prev_mesh = (og, gb, depth, hist, mom), inst, mesh
        frames.append((light, out, hist, mom, pt.denoised()))
    cloth = rm.motion(mesh, inst, None, og, rm.primary_hits(osc, og), stages=st)[..., 3] > 0
    cloth &= st["instance"] == 1
    pt.close()
    return frames, cloth


def test_sequence_parity_both_instance_modes_agree_and_the_cloth_keeps_its_history():
    K = 4
    a, cloth = run_sequence(0, K)
    b, _ = run_sequence(1, K)
    for k, (fa, fb) in enumerate(zip(a, b)):
        for x, y, name in zip(fa, fb, ("Light", "Out", "History", "Moments", "denoised")):
            same(x, y, f"frame {k} {name}, instance mode 0 against 1")
    plain, cloth2 = run_sequence(0, K, feature=False, check=False)
    assert np.array_equal(cloth, cloth2) and cloth.mean() > 0.02
    n_fed, n_plain = float(a[-1][2][..., 3][cloth].mean()), float(plain[-1][2][..., 3][cloth].mean())
    print(f"cloth, {int(cloth.sum())} pixels after {K} frames: mean N with the snapshot {n_fed:.3f}, without {n_plain:.3f}")
    assert n_fed > n_plain
    same(a[0][2], plain[0][2], "the first frame's History")


# ------------------------------------------------------------------------------------------------ 6. errors and state
def test_errors_and_forgetting():
    W, H = 100, 60
    pt, mesh, prev_v, inst, prev = deformed_tracer(W, H, 0)
    lib = pt.ctx.lib
    ng = len(mesh.geometries)
    g = gconst(pt, dw.CAMERA)
    img = motion_image(pt)
    flags = np.zeros(ng, np.uint8)
    assert lib.rt3_scene_snapshot_vertices(None) == L.E_INVALID and lib.rt3_scene_forget_prev_vertices(None) == L.E_INVALID
    assert lib.rt3_scene_deformed_geometries(None, flags.ctypes.data, ng) == L.E_INVALID
    assert lib.rt3_scene_deformed_geometries(pt.ctx.h, flags.ctypes.data, ng + 1) == L.E_INVALID and "geometry count" in err(pt)
    assert launch(pt, "motion", W, H, 1, g, [img]) == 0
    # a snapshot does not make the structure stale; an update does, whether or not a snapshot exists
    pt.ctx.snapshot_vertices()
    assert launch(pt, "motion", W, H, 1, g, [img]) == 0
    pt.ctx.update_vertices(prev_v)
    assert launch(pt, "motion", W, H, 1, g, [img]) == L.E_STATE and "vertices were updated" in err(pt)
    pt.ctx.refit_accel()
    assert launch(pt, "motion", W, H, 1, g, [img]) == 0
    assert pt.ctx.deformed_geometries(ng).any()
    # set_vertices, set_indices and set_geometry forget the snapshot
    v = np.ascontiguousarray(mesh.vertices, F)
    i = np.ascontiguousarray(mesh.indices, np.uint32)
    geo = np.ascontiguousarray(mesh.geometries)
    pc = np.ascontiguousarray(mesh.prim_counts, np.uint32)
    for call in (lambda: lib.rt3_scene_set_vertices(pt.ctx.h, v.ctypes.data, len(v)), lambda: lib.rt3_scene_set_indices(pt.ctx.h, i.ctypes.data, len(i)),
                 lambda: lib.rt3_scene_set_geometry(pt.ctx.h, geo.ctypes.data, pc.ctypes.data, len(geo))):
        pt.ctx.snapshot_vertices()
        assert lib.rt3_scene_deformed_geometries(pt.ctx.h, flags.ctypes.data, ng) == 0
        assert call() == 0
        assert lib.rt3_scene_deformed_geometries(pt.ctx.h, flags.ctypes.data, ng) == L.E_STATE and "snapshot" in err(pt)
    # ... and after the rebuild "motion" is the pass without deformation
    pt.ctx.build_accel()
    pt.ctx.set_prev_transforms(prev)
    og = as_orc(g)
    same(run_motion(pt, g), rm.motion(mesh, inst, prev, og, rm.primary_hits(orc.Scene(mesh, instances=inst), og)), "Motion after the snapshot was forgotten")
    pt.close()
    # a snapshot before any vertices
    from raytracer3_amd.render_graph import Context

    fresh = Context()
    assert fresh.lib.rt3_scene_snapshot_vertices(fresh.h) == L.E_STATE and "rt3_scene_set_vertices" in fresh.last_error()
    assert fresh.lib.rt3_scene_forget_prev_vertices(fresh.h) == 0
    fresh.close()


# ------------------------------------------------------------------------------------------------ 7. determinism
def test_two_launches_give_identical_bits():
    pt, mesh, prev_v, inst, prev = deformed_tracer(250, 187, 1)
    pt.ctx.set_prev_transforms(prev)
    g = gconst(pt, dw.CAMERA)
    a = run_motion(pt, g)
    b = run_motion(pt, g)
    assert np.array_equal(bits(a), bits(b)) and (a[..., 3] == 3).any() and (a[..., 3] == 2).any()
    pt.close()


# ------------------------------------------------------------------------------------------------ 8. the PathTracer path
def test_pathtracer_snapshots_inserts_skips_and_resets():
    W, H = 128, 96
    mesh0, inst = dw.world(0)
    pt = tracer(mesh0, (W, H), instances=inst)
    gs = [gconst(pt, dw.CAMERA, 1, k + 1, k) for k in range(6)]
    ng = len(mesh0.geometries)
    flags = np.zeros(ng, np.uint8)

    def has_snapshot():
        return pt.ctx.lib.rt3_scene_deformed_geometries(pt.ctx.h, flags.ctypes.data, ng) == 0

    def nodes():
        return [n.name for n in pt.rg.nodes].count("motion")

    pt.update_vertices(dw.mesh_at(1).vertices)  # no temporal frame yet: no snapshot
    assert not has_snapshot()
    pt.render(gs[0])                            # not a temporal frame
    pt.update_vertices(dw.mesh_at(0).vertices)
    assert not has_snapshot()
    h = pt.render(gs[0], temporal=True)
    assert "motion" not in h and nodes() == 0 and not has_snapshot()
    # vertices updated (in two pieces) between two temporal frames: one snapshot, before the first upload, and the node
    v1 = dw.mesh_at(1).vertices
    a, b = dw.vertex_range(mesh0, "cloth")
    pt.update_vertices(v1[:b])
    pt.update_vertices(v1[b:], b)
    assert has_snapshot() and [mesh0.names[i] for i in np.flatnonzero(flags)] == ["cloth", "bender", "bend2"]
    h = pt.render(gs[1], temporal=True)
    assert "motion" in h and nodes() == 1
    M = pt.motion()
    og = as_orc(gs[1])
    mesh1 = dw.mesh_at(1)
    same(M, rdf.motion(mesh1, mesh0.vertices, inst, None, og, rm.primary_hits(orc.Scene(mesh1, instances=inst), og)), "Motion of the frame after the update")
    on = M[..., 3] == 3
    assert on.mean() > 0.05 and (pt.history()[0][..., 3][on] > 1.5).mean() > 0.7
    # a frame without an update: no node, no deformed geometry (the positions of two frames ago are gone)
    h = pt.render(gs[2], temporal=True)
    assert "motion" not in h and nodes() == 0
    assert has_snapshot() and not flags.any()
    M = run_motion(pt, gs[2], fill=False)
    assert set(np.unique(M[..., 3]).tolist()) == {0.0, 1.0}
    # an update and moved instances in one interval
    pt.update_vertices(dw.mesh_at(3).vertices)
    pt.set_instances(dw.instances_at(3))
    h = pt.render(gs[3], temporal=True)
    assert "motion" in h
    mesh3, og = dw.mesh_at(3), as_orc(gs[3])
    want = rdf.motion(mesh3, mesh1.vertices, dw.instances_at(3), [m for _, _, m in inst], og, rm.primary_hits(orc.Scene(mesh3, instances=dw.instances_at(3)), og))
    same(pt.motion(), want, "Motion after an update and moved instances")
    assert set(np.unique(want[..., 3]).tolist()) == {0.0, 1.0, 2.0, 3.0}
    # reset_history starts over: no snapshot is kept, the next update takes none
    pt.reset_history()
    assert not has_snapshot()
    pt.update_vertices(dw.mesh_at(4).vertices)
    assert not has_snapshot()
    h = pt.render(gs[4], temporal=True)
    assert "motion" not in h
    fg = pt.gbuffer()[1] != BG
    assert np.all(pt.history()[0][..., 3][fg] == 1)
    # ... and so does set_scene
    pt.update_vertices(dw.mesh_at(5).vertices)
    assert has_snapshot()
    pt.set_scene(dw.mesh_at(5))
    assert not has_snapshot()
    pt.set_instances(dw.instances_at(5))
    h = pt.render(gs[5], temporal=True)
    assert "motion" not in h and np.all(pt.history()[0][..., 3][pt.gbuffer()[1] != BG] == 1)
    pt.close()
