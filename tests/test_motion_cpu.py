"""The "motion" pass and the motion input of "temporal" (DESIGN.md section 4h), CPU half: tests/ref_motion.py -- the numpy float32 restatement
the GPU must equal bit for bit (tests/test_motion.py) -- is pinned here by what a user who moves instances is owed, on oracle frames: a
world in which nothing moved gives the pass it always was; a surface that slides in its own plane keeps the history of its own points and
not of the points now behind the same pixels; the previous position it reports belongs to the point the ray hit; and in a room of moving
blocks the moved pixels converge instead of starting over every frame."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

import motion_worlds as mw
import orc
import ref_denoise as rd
import ref_motion as rm
import ref_temporal as rt
from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from raytracer3_amd.render_graph import RenderGraph
from support import bits, zeros

BG = np.float32(orc.BACKGROUND_DEPTH)
F = np.float32


def gconst(cam, W, H, spp=1, frame=1, flags=L.F_FACEFORWARD, move=((0, 0, 0), (0, 0, 0)), step=0):
    pos = np.asarray(cam["position"], np.float64) + step * np.asarray(move[0], np.float64)
    dirn = np.asarray(cam["direction"], np.float64) + step * np.asarray(move[1], np.float64)
    g = orc.camera_gconst(position=pos, direction=dirn, fov_deg=cam["fov_deg"], width=W, height=H)
    g.bounces, g.samples, g.frame, g.blendfactor = 4, spp, frame, 1.0
    g.pad[0] = flags
    return g


def frame(osc, g):
    gb, depth = osc.gbuffer(g, threads=16)
    return gb, depth, osc.reference_mode(g, gb, depth, threads=16)[0]


def rmse(a, ref, mask):
    return float(np.sqrt((((a[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64))[mask]) ** 2).mean()))


def erode(mask, r=1):
    """pixels whose (2r + 1)^2 neighbourhood lies inside the mask"""
    H, W = mask.shape
    p = np.pad(mask, r, constant_values=False)
    out = np.ones_like(mask)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out &= p[dy:dy + H, dx:dx + W]
    return out


# ------------------------------------------------------------------------------------------------ 1. nothing moved: the pass it was
@pytest.mark.parametrize("name", ["cornell", "atrium"])
def test_all_unmoved_motion_input_changes_no_bit(name):
    """Three frames under a moving camera, no instance list (one identity instance): every hit texel is {P, 1} with the bits of the surface
    record's P, and "temporal" fed with it equals ref_temporal.temporal bit for bit -- also when previous transforms are given that equal
    the current ones."""
    if name == "cornell":
        W, H, cam, flags, mesh, extra = 128, 128, scenes.CORNELL_CAMERA, L.F_FACEFORWARD, scenes.cornell(), ()
        move = ((0.01, 0.0, 0.0), (0.0105, 0.0, 0.0))
    else:
        W, H, cam, flags, mesh = 192, 108, scenes.ATRIUM_CAMERA, L.F_NEE_SKY | L.F_BLUENOISE | L.F_SPECULAR | L.F_FACEFORWARD, scenes.atrium(0.25)
        extra, move = (scenes.sky(512, 256), assets.load_bluenoise()), ((0.02, 0.0, 0.01), (0.0, 0.0, 0.012))
    osc = orc.Scene(mesh, *extra)
    prev = None
    for k in range(3):
        g = gconst(cam, W, H, 1, k + 1, flags, move, k)
        gb, depth, light = frame(osc, g)
        hits = rm.primary_hits(osc, g)
        M = rm.motion(mesh, None, None, g, hits)
        fg = depth != BG
        assert np.array_equal(M[..., 3] == 1, fg) and np.all(M[..., 3][~fg] == 0) and not M[~fg].any()
        assert np.array_equal(bits(M[..., :3][fg]), bits(rd.prepare(g, gb, depth, light)["P"][fg]))
        assert np.array_equal(bits(rm.motion(mesh, [(0, len(mesh.geometries), mw.EYE)], [mw.EYE], g, hits)), bits(M))
        if prev is None:
            prev = (g, gb, depth, zeros(H, W), zeros(H, W))
        want = rt.temporal(g, gb, depth, light, *prev)
        got = rm.temporal(g, gb, depth, light, *prev, motion=M)
        for a, b, what in zip(got, want, ("Out", "History", "Moments")):
            assert np.array_equal(bits(a), bits(b)), (name, k, what)
        for a, b in zip(rm.temporal(g, gb, depth, light, *prev, motion=None), want):
            assert np.array_equal(bits(a), bits(b))
        prev = (g, gb, depth, want[1], want[2])
    assert (want[1][..., 3][fg] == 3).mean() > 0.5  # ... and it did reproject


# ------------------------------------------------------------------------------------------------ 2. a quad slides in its own plane
def test_sliding_quad_keeps_the_history_of_its_own_points():
    """A 1 x 1 quad one unit in front of a wall slides by (0.12, -0.05) in its own plane between two frames under a fixed camera.  With the
    motion input every quad pixel whose previous place is inside the previous quad has N = 2 and its position in the previous frame differs
    from its own pixel by the analytic screen shift -shift * (H / 2) / (3 tan(fov / 2)) (the quad is 3 units from the eye): measured
    largest deviation 1.18e-5 pixels on this scene (fp32 rounding of the hit point and of the projection, at coordinates up to 160), held
    to 4 x that, 4.8e-5.  Without the motion input the same pixels look at their own place in the previous frame: the plane test passes where
    the quad was there too, so they take the history of another point of the quad, or none where the wall was there.  Wall pixels that the
    quad uncovered have N = 1 both ways."""
    W, H, shift = 160, 120, (0.12, -0.05)
    cam = mw.QUAD_CAMERA
    frames = []
    for k, s in enumerate(((0.0, 0.0), shift)):
        mesh, inst = mw.sliding_quad(s)
        osc = orc.Scene(mesh, instances=inst)
        g = gconst(cam, W, H, 32, k + 1)  # 32 spp: a signal that differs from point to point
        gb, depth, light = frame(osc, g)
        st = {}
        prev_m = [m for _, _, m in frames[0]["inst"]] if frames else None
        M = rm.motion(mesh, inst, prev_m, g, rm.primary_hits(osc, g), stages=st)
        frames.append(dict(g=g, gb=gb, depth=depth, light=light, M=M, inst=inst, quad=st["instance"] == 1, wall=st["instance"] == 0))
    f0, f1 = frames
    assert np.all(f0["M"][..., 3] == 1) and np.array_equal(f1["M"][..., 3] == 2, f1["quad"]) and np.all(f1["M"][..., 3][f1["wall"]] == 1)
    _, h0, m0 = rt.temporal(f0["g"], f0["gb"], f0["depth"], f0["light"], f0["g"], f0["gb"], f0["depth"], zeros(H, W), zeros(H, W))
    prev = (f0["g"], f0["gb"], f0["depth"], h0, m0)
    sm, sp = {}, {}
    _, hm, _ = rm.temporal(f1["g"], f1["gb"], f1["depth"], f1["light"], *prev, motion=f1["M"], stages=sm)
    _, hp, _ = rt.temporal(f1["g"], f1["gb"], f1["depth"], f1["light"], *prev, stages=sp)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ppu = (H / 2) / (3.0 * math.tan(math.radians(cam["fov_deg"]) / 2))  # pixels per world unit at the quad's distance
    want_dx, want_dy = -shift[0] * ppu, shift[1] * ppu                  # image y points down
    # quad pixels whose previous place (rounded) lies well inside the previous quad: all four taps are on it
    inner0 = erode(f0["quad"], 2)
    py0, px0 = np.clip(np.rint(ys + want_dy).astype(int), 0, H - 1), np.clip(np.rint(xs + want_dx).astype(int), 0, W - 1)
    both = f1["quad"] & inner0[py0, px0]
    assert both.sum() > 0.5 * f1["quad"].sum() > 300
    assert np.all(hm[..., 3][both] == 2)
    dev = max(float(np.abs(sm["sx"][both] - xs[both] - want_dx).max()), float(np.abs(sm["sy"][both] - ys[both] - want_dy).max()))
    print(f"sliding quad: {int(both.sum())} pixels, screen shift ({want_dx:.3f}, {want_dy:.3f}) px, largest deviation {dev:.3e} px")
    assert dev <= 4.8e-5
    # without the input: the same pixel of the previous frame, whatever was there
    assert float(np.abs(sp["sx"][both] - xs[both]).max()) < 1e-3 and float(np.abs(sp["sy"][both] - ys[both]).max()) < 1e-3
    differ = (bits(hm)[both] != bits(hp)[both]).any(-1)
    print(f"sliding quad: History differs on {int(differ.sum())} of {int(both.sum())} pixels; plain N == 1 on {int((hp[..., 3][both] == 1).sum())}")
    assert differ.mean() > 0.9
    on_wall_before = both & erode(f0["wall"], 1)
    assert on_wall_before.any() and np.all(hp[..., 3][on_wall_before] == 1)  # none
    on_quad_before = both & inner0
    assert on_quad_before.any() and np.all(hp[..., 3][on_quad_before] == 2)  # another point's
    # the wall the quad uncovered
    uncovered = f1["wall"] & inner0
    assert uncovered.sum() > 50
    assert np.all(hm[..., 3][uncovered] == 1) and np.all(hp[..., 3][uncovered] == 1)
    # wall pixels away from the quad in both frames are untouched by the input
    far = erode(f1["wall"], 2) & erode(f0["wall"], 2)
    assert np.array_equal(bits(hm[far]), bits(hp[far])) and (hm[..., 3][far] == 2).mean() > 0.99


# ------------------------------------------------------------------------------------------------ 3. the point the ray hit
SELF_CONSISTENCY_MEASURED = 7.31e-6  # largest |M_cur p - (o + d t)| / |o + d t| over the three worlds below


def test_moved_points_agree_with_the_ray():
    """For moved pixels the object-space point under the CURRENT matrix, transform_point(current_i, p), is the hit point o + d t up to the
    rounding of the intersection (t, u and v carry the fp32 error of the triangle test, largest at grazing angles).  Largest relative
    deviation measured on the parity world at both windows and on the moving world: 7.31e-6; held to 4 x that."""
    worst = 0.0
    worlds = [(mw.parity_world(), mw.PARITY_CAMERA, (192, 108)), (mw.parity_world(), mw.PARITY_CAMERA, (250, 187))]
    mesh, inst = mw.moving_world(3)
    worlds.append(((mesh, inst, [m for _, _, m in mw.moving_world(2)[1]]), scenes.CORNELL_CAMERA, (128, 128)))
    for (mesh, cur, prev), cam, (W, H) in worlds:
        osc = orc.Scene(mesh, instances=cur)
        g = gconst(cam, W, H)
        hits = rm.primary_hits(osc, g)
        st = {}
        M = rm.motion(mesh, cur, prev, g, hits, stages=st)
        mv = M[..., 3] == 2
        assert mv.mean() > 0.02
        curm = np.stack([np.asarray(m, F) for _, _, m in cur])
        Pc = rm.transform_point(curm[st["instance"][mv]], st["object_point"][mv]).astype(np.float64)
        P = rt.positions(g, hits[0])[mv].astype(np.float64)
        dev = float((np.linalg.norm(Pc - P, axis=1) / np.linalg.norm(P, axis=1)).max())
        print(f"self-consistency {W}x{H}: {int(mv.sum())} moved pixels, largest relative deviation {dev:.3e}")
        worst = max(worst, dev)
        # the previous point differs from the current one by the instance's own motion, never by more
        prv = np.stack([np.asarray(m, F) for m in prev]).astype(np.float64)
        o = st["object_point"][mv].astype(np.float64)
        i = st["instance"][mv]
        exact = np.einsum("nij,nj->ni", prv[i][:, :3, :3], o) + prv[i][:, :3, 3]
        assert np.abs(M[..., :3][mv] - exact).max() < 1e-5
    assert worst <= 4 * SELF_CONSISTENCY_MEASURED


def test_texel_kinds_of_the_parity_world():
    """the world of the GPU parity test shows every texel kind on at least 2 % of the pixels, every instance, an identity previous matrix
    on a moved instance and an identity current one"""
    mesh, cur, prev = mw.parity_world()
    moved = rm.moved_flags(cur, prev)
    assert moved.tolist() == [False, False, True, True, False, True, True, True, True]
    assert np.array_equal(cur[2][2], mw.EYE) and np.array_equal(prev[3], mw.EYE) and not np.array_equal(cur[3][2], mw.EYE)
    osc = orc.Scene(mesh, instances=cur)
    for W, H in ((192, 108), (250, 187)):
        st = {}
        M = rm.motion(mesh, cur, prev, gconst(mw.PARITY_CAMERA, W, H), rm.primary_hits(osc, gconst(mw.PARITY_CAMERA, W, H)), stages=st)
        for kind in (0, 1, 2):
            assert (M[..., 3] == kind).mean() >= 0.02
        assert all((st["instance"] == i).sum() > 100 for i in range(len(cur)))


# ------------------------------------------------------------------------------------------------ 4. quality in a room of moving blocks
QUALITY_MOVE = ((0.004, 0.0, 0.0), (0.004, 0.0, 0.0))  # the camera, per frame


def test_moved_instances_converge():
    """The instanced Cornell world (the room and its blocks, the tall block placed six more times), eight 1-spp frames: three placed blocks
    translate, one turns by 3 degrees a frame, the camera drifts.  Ground truth: the mean of two independent 512-spp frames of the last
    view; its own noise, estimated from their difference, is below a tenth of the 1-spp RMSE (measured 0.034 against 1.118 on the moved
    pixels).  On the pixels the moved instances cover in the last frame: RMSE motion-fed 0.298 < plain temporal 0.392 and < one sample
    1.118; mean N 7.81 against 5.19 (the plain pass keeps a history there too, but of the points the blocks slid away from).  On all
    other foreground pixels the motion-fed RMSE is not worse than the plain one (0.45729 both).  """
    W = H = 128
    K = 8
    cam = scenes.CORNELL_CAMERA
    prev_p = prev_m = None
    prev_inst = None
    for k in range(K):
        mesh, inst = mw.moving_world(k)
        osc = orc.Scene(mesh, instances=inst)
        g = gconst(cam, W, H, 1, k + 1, move=QUALITY_MOVE, step=k)
        gb, depth, light = frame(osc, g)
        if prev_p is None:
            prev_p = prev_m = (g, gb, depth, zeros(H, W), zeros(H, W))
        st = {}
        M = rm.motion(mesh, inst, [m for _, _, m in prev_inst] if prev_inst else None, g, rm.primary_hits(osc, g), stages=st)
        out_p, hp, mp = rt.temporal(g, gb, depth, light, *prev_p)
        out_m, hm, mm = rm.temporal(g, gb, depth, light, *prev_m, motion=M)
        prev_p, prev_m, prev_inst = (g, gb, depth, hp, mp), (g, gb, depth, hm, mm), inst
    a = frame(osc, gconst(cam, W, H, 512, 1000, move=QUALITY_MOVE, step=K - 1))[2]
    b = frame(osc, gconst(cam, W, H, 512, 2000, move=QUALITY_MOVE, step=K - 1))[2]
    truth = ((a.astype(np.float64) + b) / 2).astype(F)
    fg = depth != BG
    on_moved = np.isin(st["instance"], mw.moving_world_moved()) & fg
    others = fg & ~on_moved
    assert on_moved.mean() > 0.05 and np.array_equal(on_moved, M[..., 3] == 2)
    noise = rmse(a, b, on_moved) / 2  # of the mean of the two: sigma_512 / sqrt(2) = rms(a - b) / 2
    e1, ep, em = rmse(light, truth, on_moved), rmse(out_p, truth, on_moved), rmse(out_m, truth, on_moved)
    np_, nm = float(hp[..., 3][on_moved].mean()), float(hm[..., 3][on_moved].mean())
    op, om = rmse(out_p, truth, others), rmse(out_m, truth, others)
    print(f"moving blocks, {int(on_moved.sum())} moved pixels: noise of the truth {noise:.4f}; RMSE one sample {e1:.4f}, plain temporal {ep:.4f}, "
          f"motion-fed {em:.4f}; mean N plain {np_:.3f}, motion-fed {nm:.3f}; other pixels: plain {op:.7f}, motion-fed {om:.7f}")
    assert noise < 0.1 * e1
    assert em < ep and em < e1
    assert nm > np_
    assert om <= op


# ------------------------------------------------------------------------------------------------ 5. the Python surface
def test_frame_graph_places_the_motion_node():
    from raytracer3_amd.renderer import frame_nodes, motion_node
    from support import RecordingCtx

    W, H = 250, 187
    ctx = RecordingCtx()
    rg = RenderGraph(ctx, (W, H))
    rg.begin_frame()
    h = frame_nodes(rg, L.GConst(), postprocess=True, temporal=True, motion=True)
    rg.draw_frame(h["motion"])  # a root of its own: "temporal" reads the image as context state
    rg.draw_frame(h["color"])
    assert [c[0] for c in ctx.calls] == ["motion", "gbuffer", "refrence_mode", "temporal", "postprocess"]
    assert ctx.calls[0][1] == (W, H, 1) and ctx.calls[0][2] == [h["motion"]] and h["motion"] not in ctx.calls[3][2]
    # without `motion` the graph is the one it was
    ctx.calls.clear()
    rg.begin_frame()
    h = frame_nodes(rg, L.GConst(), postprocess=True, temporal=True)
    assert "motion" not in h
    rg.draw_frame(h["color"])
    assert [c[0] for c in ctx.calls] == ["gbuffer", "refrence_mode", "temporal", "postprocess"]
    rg.begin_frame()
    node, img = motion_node(rg, L.GConst())
    assert rg.nodes[node].kind == "raytracing" and [e.resource for e in rg.nodes[node].edges] == [img]


def test_exports_match_the_header():
    header = (Path(__file__).resolve().parent.parent / "include" / "rt3.h").read_text()
    for name in ("rt3_scene_set_prev_transforms", "rt3_temporal_set_motion_input"):
        assert name in L.EXPORTS and re.search(r"\bint " + name + r"\(", header)
    assert '"motion"        (x,y)=window   bindings {Motion RGBA32F}' in header
    assert "there are no motion vectors" not in header
