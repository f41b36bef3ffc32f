"""Previous vertex positions for the "motion" pass, CPU half: tests/ref_deform.py -- the numpy float32 restatement the
GPU must equal bit for bit (tests/test_deform.py) -- is pinned here by what a user who deforms meshes is owed, on oracle frames: without a
deformation the pass is the one it was; "deformed" follows the span rule word for word; the world of the GPU parity test shows every texel
kind; the point a deformed pixel reports belongs to the point the ray hit; a surface that slides by its vertices keeps the history of its
own points; and a waving cloth and a bending block converge instead of starting over every frame."""
import math
import re
from pathlib import Path

import numpy as np

import deform_worlds as dw
import motion_worlds as mw
import orc
import ref_deform as rdf
import ref_motion as rm
import ref_temporal as rt
from raytracer3_amd import _lib as L
from raytracer3_amd.assets import Material, MeshBuilder
from support import bits, zeros
from test_motion_cpu import QUALITY_MOVE, erode, frame, gconst, rmse

BG = np.float32(orc.BACKGROUND_DEPTH)
F = np.float32
WINDOWS = ((192, 108), (250, 187))


def current_points(mesh, inst, hits, mask):
    """the CURRENT positions interpolated at the hits of the pixels in `mask` and put under the current matrices, float64"""
    instances, flat, _ = rm.flatten(mesh, inst)
    p, ii = rm.object_points(mesh, flat, hits[3][mask].astype(np.int64), hits[1][mask].astype(F), hits[2][mask].astype(F))
    cur = np.stack([np.asarray(m, F) for _, _, m in instances])
    return rm.transform_point(cur[ii], p).astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1. no deformation: the pass it was
def test_equal_previous_vertices_change_no_bit():
    mesh, _, inst, prev = dw.parity_world()
    osc = orc.Scene(mesh, instances=inst)
    for W, H in WINDOWS:
        g = gconst(dw.CAMERA, W, H)
        hits = rm.primary_hits(osc, g)
        for pt in (prev, None):
            want = rm.motion(mesh, inst, pt, g, hits)
            assert np.array_equal(bits(rdf.motion(mesh, mesh.vertices.copy(), inst, pt, g, hits)), bits(want))
            assert np.array_equal(bits(rdf.motion(mesh, None, inst, pt, g, hits)), bits(want))
        assert not (want[..., 3] == 2).any() and (rm.motion(mesh, inst, prev, g, hits)[..., 3] == 2).any()
    # ... and words that are not positions do not count
    other = mesh.vertices.copy()
    other[:, 3:] += F(0.25)
    assert not rdf.deformed_flags(mesh, other).any()


# ------------------------------------------------------------------------------------------------ 2. the span rule
def span_mesh():
    """three geometries over one vertex buffer of 12: A indexes 2..5 of its offset 0, B indexes {0, 1, 3} of its offset 6 (vertex 8 lies
    inside its span and is not indexed), C shares A's vertices 4..6"""
    mb = MeshBuilder()
    pos = np.arange(36, dtype=np.float64).reshape(12, 3) * 0.01
    pos[7] = (0.0, 0.5, 1.0)  # a zero word
    mb.add("all", pos, np.tile([0, 0, 1.0], (12, 1)), None, [[0, 1, 2]], Material())
    m = mb.build()
    m.indices = np.array([2, 3, 4, 3, 4, 5, 0, 1, 3, 4, 5, 6], np.uint32)
    m.geometries = np.repeat(m.geometries, 3)
    m.geometries["index_offset"] = (0, 6, 9)
    m.geometries["vertex_offset"] = (0, 6, 0)
    m.prim_counts = np.array([2, 1, 1], np.uint32)
    m.names = ["A", "B", "C"]
    return m


def test_span_rule():
    m = span_mesh()
    assert rdf.spans(m) == [(2, 5), (6, 9), (4, 6)]

    def flags(vertex, word, value=None):
        prev = m.vertices.copy()
        if value is None:
            prev[vertex, word] += F(1.0)
        else:
            prev[vertex, word] = value
        return rdf.deformed_flags(m, prev).tolist()

    assert flags(2, 0) == [True, False, False]       # A's first vertex
    assert flags(5, 2) == [True, False, True]        # A's last vertex, inside C's span too
    assert flags(1, 1) == [False, False, False]      # just below A's span
    assert flags(6, 0) == [False, True, True]        # just above A's span: B's first, C's last
    assert flags(9, 2) == [False, True, False]       # B's last vertex
    assert flags(10, 0) == [False, False, False]     # just above B's span
    assert flags(8, 1) == [False, True, False]       # inside B's span, indexed by none of its triangles
    assert m.vertices[7, 0] == 0 and flags(7, 0, F(-0.0)) == [False, True, False]  # -0 is not +0
    for word in (3, 4, 5, 6, 7):                     # normal and uv words
        assert flags(4, word) == [False, False, False]
    assert rdf.deformed_flags(m, m.vertices.copy()).tolist() == [False, False, False]
    m.prim_counts = np.array([2, 0, 1], np.uint32)   # a geometry without triangles has no span
    assert rdf.spans(m)[1] == (1, 0) and flags(8, 1) == [False, False, False]


# ------------------------------------------------------------------------------------------------ 3. the world of the GPU parity test
def test_texel_kinds_of_the_parity_world():
    """every texel kind on at least 2 % of the pixels at both windows, every placement in view; the deformed geometries are the cloth and
    the two bending blocks, not the re-sent block and not the one whose normal word changed"""
    mesh, prev_v, inst, prev = dw.parity_world()
    names = [mesh.names[i] for i in np.flatnonzero(rdf.deformed_flags(mesh, prev_v))]
    assert names == ["cloth", "bender", "bend2"]
    a, b = dw.vertex_range(mesh, "normals")
    assert not np.array_equal(bits(mesh.vertices[a:b, 3:6]), bits(prev_v[a:b, 3:6])) and np.array_equal(bits(mesh.vertices[a:b, :3]), bits(prev_v[a:b, :3]))
    assert rm.moved_flags(inst, prev).tolist() == [False, False, True, False, True, True, False]
    assert np.array_equal(prev[4], mw.EYE) and np.array_equal(inst[1][2], mw.EYE)
    osc = orc.Scene(mesh, instances=inst)
    for W, H in WINDOWS:
        g = gconst(dw.CAMERA, W, H)
        st = {}
        M = rdf.motion(mesh, prev_v, inst, prev, g, rm.primary_hits(osc, g), stages=st)
        kinds = [float((M[..., 3] == k).mean()) for k in range(4)]
        print(f"{W}x{H}: miss {kinds[0]:.3f}, unmoved {kinds[1]:.3f}, moved {kinds[2]:.3f}, deformed {kinds[3]:.3f}")
        assert min(kinds) >= 0.02 and abs(sum(kinds) - 1.0) < 1e-12
        assert all((st["instance"] == i).sum() > 100 for i in range(len(inst)))
        assert set(np.unique(st["instance"][M[..., 3] == 3]).tolist()) == {1, 2, 3, 4}  # both placements of `bender` follow
        assert set(np.unique(st["instance"][M[..., 3] == 2]).tolist()) == {5}
        # without previous transforms the deformed pixels stay deformed, under the current matrices
        M0 = rdf.motion(mesh, prev_v, inst, None, g, rm.primary_hits(osc, g))
        assert np.array_equal(M0[..., 3] == 3, M[..., 3] == 3) and not (M0[..., 3] == 2).any()


# ------------------------------------------------------------------------------------------------ 4. the point the ray hit
SELF_CONSISTENCY_MEASURED = 9.79e-6  # largest |M_cur p_cur - (o + d t)| / |o + d t| over the deformed pixels of the parity world, both windows


def test_deformed_points_agree_with_the_ray():
    """On deformed pixels the CURRENT positions, interpolated with the hit's (u, v) and put under the current matrix, are the hit point
    o + d t up to the rounding of the intersection; the texel differs from that point by the surface's own motion.  Largest relative
    deviation measured on the parity world at both windows: 9.79e-6 (section 4h measured 7.31e-6 on its worlds); held to 4 x that."""
    mesh, prev_v, inst, prev = dw.parity_world()
    osc = orc.Scene(mesh, instances=inst)
    worst = 0.0
    for W, H in WINDOWS:
        g = gconst(dw.CAMERA, W, H)
        hits = rm.primary_hits(osc, g)
        st = {}
        M = rdf.motion(mesh, prev_v, inst, prev, g, hits, stages=st)
        df = st["deformed"]
        assert np.array_equal(df, M[..., 3] == 3) and df.mean() > 0.02
        P = rt.positions(g, hits[0])[df].astype(np.float64)
        dev = float((np.linalg.norm(current_points(mesh, inst, hits, df) - P, axis=1) / np.linalg.norm(P, axis=1)).max())
        print(f"self-consistency {W}x{H}: {int(df.sum())} deformed pixels, largest relative deviation {dev:.3e}")
        worst = max(worst, dev)
        # the texel is the previous positions under the previous matrix, in exact arithmetic too
        prv = np.stack([np.asarray(m, F) for m in prev]).astype(np.float64)
        o, i = st["prev_object_point"][df].astype(np.float64), st["instance"][df]
        exact = np.einsum("nij,nj->ni", prv[i][:, :3, :3], o) + prv[i][:, :3, 3]
        assert np.abs(M[..., :3][df] - exact).max() < 1e-5
    assert worst <= 4 * SELF_CONSISTENCY_MEASURED


# ------------------------------------------------------------------------------------------------ 5. a quad slides by its vertices
SLIDE_MEASURED = 1.18e-5  # pixels


def test_quad_slid_by_its_vertices_keeps_the_history_of_its_own_points():
    """motion_worlds' sliding quad, moved by (0.12, -0.05) through rt3_scene_update_vertices instead of its matrix, under a fixed camera:
    every quad pixel whose previous place is inside the previous quad has N = 2 after the two frames, and its position in the previous
    frame differs from its own pixel by the analytic screen shift (test_motion_cpu.py): largest deviation measured 1.18e-5 pixels, as for
    the matrix, held to 4 x that.  The texels equal those of the same slide done by the matrix, up to the kind."""
    W, H, shift = 160, 120, (0.12, -0.05)
    cam = mw.QUAD_CAMERA
    rest, slid, inst = dw.slid_quad(shift)
    assert rdf.deformed_flags(slid, rest.vertices).tolist() == [False, True, False]
    f = []
    for k, mesh in enumerate((rest, slid)):
        osc = orc.Scene(mesh, instances=inst)
        g = gconst(cam, W, H, 32, k + 1)
        gb, depth, light = frame(osc, g)
        st = {}
        M = rdf.motion(mesh, rest.vertices if k else None, inst, None, g, rm.primary_hits(osc, g), stages=st)
        f.append(dict(g=g, gb=gb, depth=depth, light=light, M=M, quad=st["instance"] == 1, wall=st["instance"] == 0))
    f0, f1 = f
    assert np.all(f0["M"][..., 3] == 1) and np.array_equal(f1["M"][..., 3] == 3, f1["quad"]) and np.all(f1["M"][..., 3][f1["wall"]] == 1)
    _, h0, m0 = rt.temporal(f0["g"], f0["gb"], f0["depth"], f0["light"], f0["g"], f0["gb"], f0["depth"], zeros(H, W), zeros(H, W))
    prev = (f0["g"], f0["gb"], f0["depth"], h0, m0)
    sm = {}
    _, hm, _ = rm.temporal(f1["g"], f1["gb"], f1["depth"], f1["light"], *prev, motion=f1["M"], stages=sm)
    _, hp, _ = rt.temporal(f1["g"], f1["gb"], f1["depth"], f1["light"], *prev)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ppu = (H / 2) / (3.0 * math.tan(math.radians(cam["fov_deg"]) / 2))
    want_dx, want_dy = -shift[0] * ppu, shift[1] * ppu
    inner0 = erode(f0["quad"], 2)
    py0, px0 = np.clip(np.rint(ys + want_dy).astype(int), 0, H - 1), np.clip(np.rint(xs + want_dx).astype(int), 0, W - 1)
    both = f1["quad"] & inner0[py0, px0]
    assert both.sum() > 0.5 * f1["quad"].sum() > 300
    assert np.all(hm[..., 3][both] == 2)
    dev = max(float(np.abs(sm["sx"][both] - xs[both] - want_dx).max()), float(np.abs(sm["sy"][both] - ys[both] - want_dy).max()))
    print(f"quad slid by its vertices: {int(both.sum())} pixels, screen shift ({want_dx:.3f}, {want_dy:.3f}) px, largest deviation {dev:.3e} px")
    assert dev <= 4 * SLIDE_MEASURED
    assert ((bits(hm)[both] != bits(hp)[both]).any(-1)).mean() > 0.9  # without the input: another point's history, or none
    uncovered = f1["wall"] & inner0
    assert uncovered.sum() > 50 and np.all(hm[..., 3][uncovered] == 1)
    # the same slide by the matrix: the same previous points (the quad's matrix there is a translation, here the identity)
    mesh_m, inst_m = mw.sliding_quad(shift)
    g1 = f1["g"]
    Mm = rm.motion(mesh_m, inst_m, [m for _, _, m in inst], g1, rm.primary_hits(orc.Scene(mesh_m, instances=inst_m), g1))
    q = f1["quad"] & (Mm[..., 3] == 2)
    assert q.sum() > 0.95 * f1["quad"].sum() and np.abs(Mm[..., :3][q] - f1["M"][..., :3][q]).max() < 2e-6


# ------------------------------------------------------------------------------------------------ 6. quality: a waving cloth, bending blocks
def test_deformed_meshes_converge():
    """deform_worlds.world(k), eight 1-spp frames at 128 x 128: the cloth waves, the blocks bend and slide, the camera drifts as in section 7.
    Ground truth: the mean of two independent 512-spp frames of the last view.  On the pixels the deformed geometries cover in the last
    frame the fed RMSE is below the plain pass's and one sample's, and the mean N is larger; on all other foreground pixels the fed RMSE
    is not worse.  Figures: DESIGN.md section 7."""
    W = H = 128
    K = 8
    cam = dw.CAMERA
    prev_p = prev_f = prev_inst = prev_mesh = None
    for k in range(K):
        mesh, inst = dw.world(k)
        osc = orc.Scene(mesh, instances=inst)
        g = gconst(cam, W, H, 1, k + 1, move=QUALITY_MOVE, step=k)
        gb, depth, light = frame(osc, g)
        if prev_p is None:
            prev_p = prev_f = (g, gb, depth, zeros(H, W), zeros(H, W))
        st = {}
        M = rdf.motion(mesh, prev_mesh.vertices if prev_mesh else None, inst, [m for _, _, m in prev_inst] if prev_inst else None, g,
                       rm.primary_hits(osc, g), stages=st)
        out_p, hp, mp = rt.temporal(g, gb, depth, light, *prev_p)
        out_f, hf, mf = rm.temporal(g, gb, depth, light, *prev_f, motion=M)
        prev_p, prev_f, prev_inst, prev_mesh = (g, gb, depth, hp, mp), (g, gb, depth, hf, mf), inst, mesh
    a = frame(osc, gconst(cam, W, H, 512, 1000, move=QUALITY_MOVE, step=K - 1))[2]
    b = frame(osc, gconst(cam, W, H, 512, 2000, move=QUALITY_MOVE, step=K - 1))[2]
    truth = ((a.astype(np.float64) + b) / 2).astype(F)
    fg = depth != BG
    on = st["deformed"] & fg
    others = fg & ~on
    assert on.mean() > 0.05 and np.array_equal(on, M[..., 3] == 3)
    noise = rmse(a, b, on) / 2
    e1, ep, ef = rmse(light, truth, on), rmse(out_p, truth, on), rmse(out_f, truth, on)
    np_, nf = float(hp[..., 3][on].mean()), float(hf[..., 3][on].mean())
    op, of = rmse(out_p, truth, others), rmse(out_f, truth, others)
    print(f"deforming meshes, {int(on.sum())} deformed pixels: noise of the truth {noise:.4f}; RMSE one sample {e1:.4f}, plain temporal {ep:.4f}, "
          f"fed {ef:.4f}; mean N plain {np_:.3f}, fed {nf:.3f}; other pixels: plain {op:.7f}, fed {of:.7f}")
    assert noise < 0.1 * e1
    assert ef < ep and ef < e1
    assert nf > np_
    assert of <= op


# ------------------------------------------------------------------------------------------------ 7. the public surface
def test_exports_match_the_header():
    root = Path(__file__).resolve().parent.parent
    header = (root / "include" / "rt3.h").read_text()
    host = (root / "raytracer3_amd" / "host" / "render_graph.hpp").read_text()
    for name in ("rt3_scene_snapshot_vertices", "rt3_scene_forget_prev_vertices", "rt3_scene_deformed_geometries"):
        assert name in L.EXPORTS and re.search(r"\bint " + name + r"\(", header) and name + "(ctx_" in host
