"""Motion under a lens, without a GPU: tests/ref_guide_motion.py -- the numpy float32 restatement that
tests/test_guide_motion.py holds the MI355X to -- against an independently written scalar loop and a float64 sum; its invariance under the
batch split; what it must equal where nothing moved (the guide's position image) and at one pinhole sample (the "motion" pass's texel);
the sliding quad of section 4h under a pinhole lens; the all-unmoved input; the condition on the test world; and the Python surface."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

import guide_motion_worlds as GM
import motion_worlds as mw
import orc
import ref_deform as rdf
import ref_guide as rgd
import ref_guide_motion as rgm
import ref_motion as rm
import ref_temporal_guide as rtg
import temporal_guide_worlds as TW
from raytracer3_amd import _lib as L
from raytracer3_amd.render_graph import RenderGraph
from support import RecordingCtx, bits, zeros
from test_motion_cpu import erode, frame
from test_motion_cpu import gconst as pinhole_gconst

F = np.float32
U = 2.0 ** -24
S = GM.S_MAX


@pytest.fixture(scope="module")
def world():
    """the parity world and the CPU samples of its antialiased frame at 67 x 45, S = 5"""
    w = GM.parity()
    g = GM.gconst(GM.WINDOW)
    return w, g, GM.cpu_samples(w["mesh"], w["instances"], g, GM.WINDOW, GM.LENSES["antialiased"], S, seed=1)


# ------------------------------------------------------------------------------------------------ 0. the condition on the world
def test_world_holds_every_kind_of_sample(world):
    """each of escaped, unmoved, moved and deformed holds at least 2 % of the samples, and at least 8 pixels mix two kinds"""
    w, _, f = world
    shares, mixed = GM.kind_shares(w, f)
    print("antialiased 67 x 45, S = 5: escaped {:.3f}, unmoved {:.3f}, moved {:.3f}, deformed {:.3f}; {} pixels mix kinds".format(*shares, mixed))
    assert min(shares) >= 0.02 and abs(sum(shares) - 1.0) < 1e-12
    assert mixed >= 8


# ------------------------------------------------------------------------------------------------ 1. the definition
def scalar_previous_point(w, pv, pm, o, d, t, u, v, prim):
    """one sample, one scalar float32 operation at a time, with its own walk through the instance list"""
    mesh, inst = w["mesh"], w["instances"]
    base = 0
    for i, (first, count, m) in enumerate(inst):
        for geom in range(int(first), int(first) + int(count)):
            n = int(mesh.prim_counts[geom])
            if prim < base + n:
                break
            base += n
        else:
            continue
        break
    m = np.asarray(m, F)
    moved = pm is not None and bool((bits(np.asarray(pm[i], F)[:3]) != bits(m[:3])).any())
    io, vo = int(mesh.geometries["index_offset"][geom]), int(mesh.geometries["vertex_offset"][geom])
    own = np.asarray(mesh.indices, np.int64)[io:io + 3 * int(mesh.prim_counts[geom])]
    cur = np.asarray(mesh.vertices, F).reshape(-1, 8)
    deformed = False
    if pv is not None:
        old = np.asarray(pv, F).reshape(-1, 8)
        lo, hi = vo + int(own.min()), vo + int(own.max())
        deformed = bool((bits(cur[lo:hi + 1, :3]) != bits(old[lo:hi + 1, :3])).any())
    if not moved and not deformed:
        return [F(o[k] + F(d[k] * t)) for k in range(3)]
    verts = old if deformed else cur
    tri = own[3 * (prim - base): 3 * (prim - base) + 3]
    a, b, c = (verts[vo + int(j), :3] for j in tri)
    wgt = F(F(F(1) - u) - v)
    p = [F(F(F(a[k] * wgt) + F(b[k] * u)) + F(c[k] * v)) for k in range(3)]
    M = np.asarray(pm[i], F) if pm is not None else m
    if np.array_equal(bits(M), bits(np.eye(4, dtype=F))):
        return p
    return [F(M[k, 3] + F(F(M[k, 2] * p[2]) + F(F(M[k, 1] * p[1]) + F(M[k, 0] * p[0])))) for k in range(3)]


def pick_pixels(w, f, n=72):
    """pixels of every kind, mixed ones first"""
    kinds = rgm.sample_kinds(w["mesh"], w["prev_vertices"], w["instances"], w["prev_transforms"], f["hit"], f["prim"])
    mixed = np.flatnonzero((kinds != kinds[0]).any(0))
    pure = [np.flatnonzero((kinds == k).all(0))[:10] for k in (rgm.ESCAPED, rgm.UNMOVED, rgm.MOVED, rgm.DEFORMED)]
    assert all(len(p) for p in pure) and len(mixed) >= 8
    return np.concatenate([mixed[:n - 40], *pure])


@pytest.mark.parametrize("case", GM.CASES)
def test_accumulation_is_the_scalar_loop_and_close_to_float64(world, case):
    w, _, f = world
    pick = pick_pixels(w, f)
    sub = {k: v[:, pick] for k, v in f.items()}
    pv, pm = GM.case_args(w, case)
    R = GM.previous_points(w, case, sub)
    got = rgm.accumulate_prev(sub["hit"], R, S)
    assert got.dtype == F and got.shape == (len(pick), 4)
    want = np.zeros((len(pick), 4), F)
    R64 = np.zeros((S, len(pick), 3))
    for i in range(len(pick)):
        acc, nh = [F(0)] * 3, F(0)
        for s in range(S):
            if not sub["hit"][s, i]:
                continue
            r = scalar_previous_point(w, pv, pm, sub["o"][s, i], sub["d"][s, i], sub["t"][s, i], sub["bu"][s, i], sub["bv"][s, i], int(sub["prim"][s, i]))
            R64[s, i] = [float(x) for x in r]
            acc = [F(acc[k] + r[k]) for k in range(3)]
            nh = F(nh + F(1))
        if nh > 0:
            want[i] = [F(acc[0] / nh), F(acc[1] / nh), F(acc[2] / nh), F(nh / F(S))]
    assert np.array_equal(bits(got), bits(want)), case
    # S - 1 roundings of the running sum and one of the division: (S + 1) 2^-24 of the sum of magnitudes
    nh = sub["hit"].sum(0)
    some = nh > 0
    mean = R64.sum(0)[some] / nh[some, None]
    mag = np.abs(R64).sum(0)[some] / nh[some, None]
    assert np.all(np.abs(got[some, :3].astype(np.float64) - mean) <= (S + 1) * U * mag + 1e-300)
    assert np.array_equal(got[:, 3], (nh / S).astype(F)) and not got[~some].any()
    if case != "neither":  # the points did move
        assert not np.array_equal(bits(R[sub["hit"]]), bits(GM.previous_points(w, "neither", sub)[sub["hit"]]))


def test_accumulation_does_not_depend_on_the_batch_split(world):
    w, _, f = world
    R = GM.previous_points(w, "both", f)
    whole = rgm.accumulate_prev(f["hit"], R, S)
    for batch in (1, 2, 3, S):
        assert np.array_equal(bits(rgm.accumulate_prev_split(f["hit"], R, batch)), bits(whole)), batch
    mid = rgm.accumulate_prev(f["hit"][:2], R[:2], S, first=True, last=False)  # between batches: the sums, the count in .w
    assert np.array_equal(mid[:, 3], f["hit"][:2].sum(0).astype(F))


def test_nothing_moved_is_the_position_image(world):
    """equal matrices and an equal snapshot, and no previous state at all: ref_guide.accumulate's `position`, bit for bit"""
    w, _, f = world
    z = np.zeros(f["o"].shape, F)
    position = rgd.accumulate(f["hit"], f["o"], f["d"], f["t"], z, z, z, S)["position"]
    same = rgm.previous_points(w["mesh"], w["mesh"].vertices, w["instances"], [m for _, _, m in w["instances"]], *GM.prev_args(f))
    assert np.array_equal(bits(rgm.accumulate_prev(f["hit"], same, S)), bits(position))
    assert np.array_equal(bits(rgm.accumulate_prev(f["hit"], GM.previous_points(w, "neither", f), S)), bits(position))
    assert not np.array_equal(bits(rgm.accumulate_prev(f["hit"], GM.previous_points(w, "both", f), S)), bits(position))


@pytest.mark.parametrize("case", GM.CASES)
def test_one_pinhole_sample_is_the_motion_texel(world, case):
    """S = 1, fed the primary rays and their hits: every hit pixel's xyz is ref_deform.motion's texel, two restatements of one rule"""
    w, g, _ = world
    W, H = GM.WINDOW
    pv, pm = GM.case_args(w, case)
    osc = orc.Scene(w["mesh"], instances=w["instances"])
    ys, xs = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    rays = orc.primary_rays(g, xs.ravel(), ys.ravel())
    t, u, v, prim = rm.primary_hits(osc, g)
    M = rdf.motion(w["mesh"], pv, w["instances"], pm, g, (t, u, v, prim))
    hit = (prim != np.uint32(orc.MISS)).reshape(1, -1)
    one = lambda a: a.reshape(1, W * H)  # noqa: E731
    R = rgm.previous_points(w["mesh"], pv, w["instances"], pm, hit, rays[0:3].T[None], rays[3:6].T[None], one(t), one(u), one(v), one(prim))
    img = rgm.accumulate_prev(hit, R, 1).reshape(H, W, 4)
    fg = hit.reshape(H, W)
    assert np.array_equal(bits(img[fg][:, :3]), bits(M[fg][:, :3])) and np.array_equal(img[..., 3] == 1, fg) and not img[~fg].any()
    kinds = sorted(set(M[..., 3][fg].tolist()))
    assert kinds == {"both": [1, 2, 3], "transforms": [1, 2], "snapshot": [1, 3], "neither": [1]}[case]


# ------------------------------------------------------------------------------------------------ 2. a quad slides in its own plane
QUAD_DEVIATION_MEASURED = 1.18e-5  # pixels: test_motion_cpu.test_sliding_quad_keeps_the_history_of_its_own_points derives it


def test_sliding_quad_under_a_pinhole_lens():
    """Section 4h's quad, guided: the guide of each frame is one pinhole sample per pixel (the primary rays, the oracle's hits and
    hit_info).  With the input the reprojected point differs from the pixel's own by the analytic screen shift within 4 x the figure
    derived there, and N = 2 after two frames; without it the same pixels take another point's history, or none."""
    W, H, shift = 160, 120, (0.12, -0.05)
    cam = mw.QUAD_CAMERA
    ys, xs = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    frames = []
    for k, s in enumerate(((0.0, 0.0), shift)):
        mesh, inst = mw.sliding_quad(s)
        osc = orc.Scene(mesh, instances=inst)
        g = pinhole_gconst(cam, W, H, 32, k + 1)
        _, _, light = frame(osc, g)
        rays = orc.primary_rays(g, xs.ravel(), ys.ravel())
        t, u, v, prim = (a.reshape(1, -1) for a in rm.primary_hits(osc, g))
        hit = prim != np.uint32(orc.MISS)
        assert hit.all()
        surf = osc.hit_info(prim[0], u[0], v[0])
        o, d = rays[0:3].T[None], rays[3:6].T[None]
        guide = {key: img.reshape(H, W, 4) for key, img in rgd.accumulate(hit, o, d, t, surf[None, :, 6:9], surf[None, :, 0:3], surf[None, :, 3:6], 1).items()}
        prev_m = [m for _, _, m in frames[0]["inst"]] if frames else None
        image = rgm.accumulate_prev(hit, rgm.previous_points(mesh, None, inst, prev_m, hit, o, d, t, u, v, prim), 1).reshape(H, W, 4)
        st = {}
        rm.motion(mesh, inst, prev_m, g, (t.reshape(H, W), u.reshape(H, W), v.reshape(H, W), prim.reshape(H, W)), stages=st)
        frames.append(dict(g=g, guide=guide, light=light, image=image, inst=inst, quad=st["instance"] == 1, wall=st["instance"] == 0))
    f0, f1 = frames
    assert np.array_equal(bits(f0["image"]), bits(f0["guide"]["position"])), "nothing moved in frame 0"
    _, h0, m0 = rtg.temporal(f0["g"], f0["guide"], f0["light"], f0["g"], f0["guide"], zeros(H, W), zeros(H, W))
    prev = (f0["g"], f0["guide"], h0, m0)
    sm, sp = {}, {}
    _, hm, _ = rgm.temporal(f1["g"], f1["guide"], f1["light"], *prev, f1["image"], stages=sm)
    _, hp, _ = rtg.temporal(f1["g"], f1["guide"], f1["light"], *prev, stages=sp)
    ppu = (H / 2) / (3.0 * math.tan(math.radians(cam["fov_deg"]) / 2))
    want_dx, want_dy = -shift[0] * ppu, shift[1] * ppu
    inner0 = erode(f0["quad"], 2)
    py0, px0 = np.clip(np.rint(ys + want_dy).astype(int), 0, H - 1), np.clip(np.rint(xs + want_dx).astype(int), 0, W - 1)
    both = f1["quad"] & inner0[py0, px0]
    assert both.sum() > 0.5 * f1["quad"].sum() > 300
    assert np.all(hm[..., 3][both] == 2)
    dev = max(float(np.abs(sm["sx"][both] - xs[both] - want_dx).max()), float(np.abs(sm["sy"][both] - ys[both] - want_dy).max()))
    print(f"sliding quad under a pinhole lens: {int(both.sum())} pixels, largest deviation from the screen shift {dev:.3e} px")
    assert dev <= 4 * QUAD_DEVIATION_MEASURED
    assert float(np.abs(sp["sx"][both] - xs[both]).max()) < 1e-3 and float(np.abs(sp["sy"][both] - ys[both]).max()) < 1e-3
    on_wall_before = both & erode(f0["wall"], 1)
    assert on_wall_before.any() and np.all(hp[..., 3][on_wall_before] == 1), "without the input: no history where the wall was"
    on_quad_before = both & inner0
    differ = (bits(hm)[on_quad_before] != bits(hp)[on_quad_before]).any(-1)
    assert on_quad_before.any() and np.all(hp[..., 3][on_quad_before] == 2) and differ.mean() > 0.9, "... and another point's where the quad was"
    far = erode(f1["wall"], 2) & erode(f0["wall"], 2)
    assert np.array_equal(bits(hm[far]), bits(hp[far])), "the wall away from the quad is untouched by the input"


# ------------------------------------------------------------------------------------------------ 3. the all-unmoved input
@pytest.mark.parametrize("make", (lambda: TW.edge_case_frame(), lambda: TW.random_frame((33, 9), 3)), ids=("edge cases", "random"))
def test_an_all_unmoved_input_is_no_input(make):
    f = make()
    want = rtg.temporal(*TW.ref_args(f))
    for flags in (0, rtg.NO_DEMODULATION):
        want = rtg.temporal(*TW.ref_args(f), flags=flags)
        got = rgm.temporal(*TW.ref_args(f), f["guide"]["position"], flags=flags)
        for a, b, name in zip(got, want, ("Out", "History", "Moments")):
            assert np.array_equal(bits(a), bits(b)), name
        for a, b in zip(rgm.temporal(*TW.ref_args(f), None, flags=flags), want):
            assert np.array_equal(bits(a), bits(b))
    assert (want[1][..., 3] > 1).any(), "it did reproject"


# ------------------------------------------------------------------------------------------------ 4. the Python surface
def test_frame_graph_declares_the_image_as_context_state():
    from raytracer3_amd.renderer import frame_nodes, guide_prev_position_image

    ctx = RecordingCtx()
    rg = RenderGraph(ctx, GM.WINDOW)
    rg.begin_frame()
    h = frame_nodes(rg, L.GConst(), postprocess=True, denoise=True, temporal=True, motion=True, guide=True)
    assert "motion" not in h and h["guide_motion"] == guide_prev_position_image(rg)
    assert h["guide_motion"] not in {*h["guide"].values(), *h["prev_guide"].values()}
    nodes = {n.name: n for n in rg.nodes}
    assert "motion" not in nodes
    state = lambda name, typ: [e.resource for e in nodes[name].edges if e.edge_type == typ]  # noqa: E731
    assert state("refrence_mode", "StateWrite") == [*h["guide"].values(), h["guide_motion"]]
    assert state("temporal", "StateRead") == [*h["guide"].values(), *h["prev_guide"].values(), h["guide_motion"]]
    read = next(e for e in nodes["temporal"].edges if e.resource == h["guide_motion"])
    assert rg.nodes[read.origin].name == "refrence_mode"
    rg.draw_frame(h["color"])
    assert [c[0] for c in ctx.calls] == ["gbuffer", "refrence_mode", "temporal", "denoise", "postprocess"]
    assert all(h["guide_motion"] not in c[2] for c in ctx.calls), "no binding"
    # nothing moved, or no guide: the frames of before
    rg.begin_frame()
    h = frame_nodes(rg, L.GConst(), True, True, True, guide=True)
    assert "guide_motion" not in h and "motion" not in h
    rg.begin_frame()
    h = frame_nodes(rg, L.GConst(), True, True, True, motion=True)
    assert "guide_motion" not in h and "motion" in h


def test_exports_and_header():
    header = (Path(__file__).resolve().parent.parent / "include" / "rt3.h").read_text()
    for name, args in (("rt3_camera_set_guide_motion_output", r"rt3_ctx \*ctx, uint32_t image"),
                       ("rt3_camera_get_guide_motion_output", r"rt3_ctx \*ctx, uint32_t \*image"),
                       ("rt3_temporal_set_guide_motion_input", r"rt3_ctx \*ctx, uint32_t image")):
        assert name in L.EXPORTS
        assert re.search(rf"\bint {name}\({args}\);", header), name
    assert L.SELFTEST_GUIDE_PREV_QUEUE == 41
