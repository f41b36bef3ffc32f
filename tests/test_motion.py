"""The "motion" pass and the motion input of "temporal" on the MI355X: bit-for-bit parity of Motion with
tests/ref_motion.py in both instance modes, at two windows and under a tile partition; "temporal" fed with an all-unmoved image equals
"temporal" without one; sequences of moving instances under a moving camera, fed back into each other and chained into "denoise", equal
the reference and each other across the instance modes; the documented errors; determinism; and the PathTracer path.  The hits come from
the GPU's own primary trace, which test_gpu_parity.py and test_instances_two_level.py pin to the oracle's."""
import math

import numpy as np
import pytest

import motion_worlds as mw
import orc
import ref_motion as rm
import ref_temporal as rt
from raytracer3_amd import _lib as L
from raytracer3_amd import scenes
from support import as_orc, bits, camera, err, launch, same, tracer

pytestmark = pytest.mark.gpu
BG = np.float32(orc.BACKGROUND_DEPTH)
F = np.float32
FLAGS = L.F_FACEFORWARD
CAMERA_MOVE = ((0.004, 0.0, 0.0), (0.004, 0.0, 0.0))


def gconst(pt, cam, spp=1, frame=1, step=0, move=CAMERA_MOVE):
    return pt.make_gconst(camera(cam, pt.window, step, move), spp, 4, frame=frame, flags=FLAGS)


def motion_image(pt):
    from raytracer3_amd.render_graph import ImageSize

    return pt.rg.image(ImageSize.FullScreen, L.FORMAT_R32G32B32A32_SFLOAT, "Motion")


SENTINEL = np.array([0x7FC12345, 0xFFC54321, 0x12345678, 0x9ABCDEF0], np.uint32).view(F)


def run_motion(pt, g, fill=True):
    """launch "motion" over the window and download the image (prefilled with a sentinel)"""
    W, H = pt.window
    img = motion_image(pt)
    if fill:
        pt.rg.upload(img, np.broadcast_to(SENTINEL, (H, W, 4)).copy())
    pt.ctx.check(launch(pt, "motion", W, H, 1, g, [img]))
    pt.ctx.wait()
    return pt.rg.download(img, (H, W, 4), F)


# ------------------------------------------------------------------------------------------------ 1. Motion equals the reference
@pytest.mark.parametrize("mode", [0, 1])
def test_motion_parity_windows_and_partition(mode):
    mesh, cur, prev = mw.parity_world()
    osc = orc.Scene(mesh, instances=cur)
    for W, H in ((192, 108), (250, 187)):
        pt = tracer(mesh, (W, H), instances=cur, mode=mode)
        pt.ctx.set_prev_transforms(prev)
        g = gconst(pt, mw.PARITY_CAMERA)
        want = rm.motion(mesh, cur, prev, as_orc(g), rm.primary_hits(osc, as_orc(g)))
        got = run_motion(pt, g)
        kinds = [float((got[..., 3] == k).mean()) for k in (0, 1, 2)]
        print(f"mode {mode} {W}x{H}: miss {kinds[0]:.3f}, unmoved {kinds[1]:.3f}, moved {kinds[2]:.3f}")
        assert min(kinds) >= 0.02 and abs(sum(kinds) - 1.0) < 1e-12
        same(got, want, f"Motion, mode {mode}, {W}x{H}")
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


# ------------------------------------------------------------------------------------------------ 2. an all-unmoved input changes no bit
def test_temporal_with_all_unmoved_motion_equals_temporal_without():
    mesh, cur, _ = mw.parity_world()
    W, H = 192, 108
    pt = tracer(mesh, (W, H), instances=cur)
    gs = [gconst(pt, mw.PARITY_CAMERA, 1, k + 1, k) for k in range(3)]
    for g in gs:
        h = pt.render(g, temporal=True)
    plain = (pt.accumulated(), *pt.history())
    assert "motion" not in h and (plain[1][..., 3] == 3).mean() > 0.3
    M = run_motion(pt, gs[-1])
    assert set(np.unique(M[..., 3]).tolist()) == {0.0, 1.0}
    names = ["gbuffer", "depth", "light", "prev_gbuffer", "prev_depth", "prev_history", "prev_moments", "accumulated", "history", "moments"]
    nan = np.full((H, W, 4), np.nan, F)
    for with_input in (True, False):
        for n in names[7:]:
            pt.rg.upload(h[n], nan)
        pt.ctx.set_temporal_motion_input(motion_image(pt) if with_input else 0)
        pt.ctx.check(launch(pt, "temporal", math.ceil(W / 8), math.ceil(H / 8), 1, gs[-1], [h[n] for n in names]))
        pt.ctx.wait()
        for got, want, what in zip((pt.accumulated(), *pt.history()), plain, ("Out", "History", "Moments")):
            same(got, want, f"{what}, motion input {'set' if with_input else 'cleared'}")
    pt.close()


# ------------------------------------------------------------------------------------------------ 3. sequences of moving instances
def run_sequence(mode, K=5, W=160, H=120, denoise=True):
    """K frames of the moving world through PathTracer.set_instances + render(temporal=True); every frame is compared with the reference
    chain on the frame's own Light and the previous frame's (GPU) History and Moments.  Returns the frames' images."""
    mesh, inst = mw.moving_world(0)
    pt = tracer(mesh, (W, H), instances=inst, mode=mode)
    prev, prev_inst, frames = None, None, []
    for k in range(K):
        mesh, inst = mw.moving_world(k)
        if k:
            pt.set_instances(inst)
        g = gconst(pt, scenes.CORNELL_CAMERA, 1, k + 1, k)
        h = pt.render(g, temporal=True, denoise=denoise)
        og = as_orc(g)
        light, out = pt.light(), pt.accumulated()
        hist, mom = pt.history()
        gb, depth = pt.gbuffer()
        M = None
        if k:
            assert "motion" in h
            osc = orc.Scene(mesh, instances=inst)
            M = rm.motion(mesh, inst, [m for _, _, m in prev_inst], og, rm.primary_hits(osc, og))
            same(pt.motion(), M, f"mode {mode} frame {k} Motion")
            assert (M[..., 3] == 2).mean() > 0.05
        else:
            assert "motion" not in h
            prev = (og, gb, depth, np.zeros((H, W, 4), F), np.zeros((H, W, 4), F))
        want = rm.temporal(og, gb, depth, light, *prev, motion=M)
        for got, ref, name in zip((out, hist, mom), want, ("Out", "History", "Moments")):
            same(got, ref, f"mode {mode} frame {k} {name}")
        den = None
        if denoise:
            den = pt.denoised()
            same(den, rt.denoise(og, gb, depth, out, moments=mom), f"mode {mode} frame {k} denoised")
        if k:
            moved = M[..., 3] == 2
            plain = rt.temporal(og, gb, depth, light, *prev)[1]
            print(f"mode {mode} frame {k}: moved pixels {int(moved.sum())}, mean N {hist[..., 3][moved].mean():.2f} "
                  f"(without the input {plain[..., 3][moved].mean():.2f})")
            assert not np.array_equal(bits(plain), bits(hist))  # the input is what made the frame
        prev, prev_inst = (og, gb, depth, hist, mom), inst
        frames.append((light, out, hist, mom, den))
    pt.close()
    return frames


def test_sequence_parity_and_both_instance_modes_agree():
    a = run_sequence(0)
    b = run_sequence(1)
    for k, (fa, fb) in enumerate(zip(a, b)):
        for x, y, name in zip(fa, fb, ("Light", "Out", "History", "Moments", "denoised")):
            same(x, y, f"frame {k} {name}, instance mode 0 against 1")
    assert (a[-1][2][..., 3] > 4.5).mean() > 0.5  # the last frame carries five frames of history on most pixels


# ------------------------------------------------------------------------------------------------ 4. errors and state
def test_errors_and_state():
    from raytracer3_amd.render_graph import ImageSize
    from raytracer3_amd.renderer import PathTracer

    mesh, cur, prev = mw.parity_world()
    W, H = 100, 60
    lib = L.load()
    # before a build
    fresh = PathTracer((W, H))
    g = gconst(fresh, mw.PARITY_CAMERA)
    assert launch(fresh, "motion", W, H, 1, g, [motion_image(fresh)]) == L.E_STATE and "rt3_accel_build" in err(fresh)
    fresh.ctx.upload_mesh(mesh)
    fresh.ctx.set_instances(cur)
    fresh.ctx.set_prev_transforms(prev)
    assert launch(fresh, "motion", W, H, 1, g, [motion_image(fresh)]) == L.E_STATE
    fresh.close()

    pt = tracer(mesh, (W, H), instances=cur)
    osc = orc.Scene(mesh, instances=cur)
    og = as_orc(g)
    hits = rm.primary_hits(osc, og)
    img = motion_image(pt)
    pt.ctx.set_prev_transforms(prev)
    first = run_motion(pt, g)
    same(first, rm.motion(mesh, cur, prev, og, hits), "Motion")
    # rt3_scene_set_prev_transforms leaves the built structure usable: no rebuild was needed above, and the other passes still run
    assert pt.ctx.accel_info()[1] > 0
    pt.render(g)
    # the count is checked at launch
    pt.ctx.set_prev_transforms(prev[:-1])
    assert launch(pt, "motion", W, H, 1, g, [img]) == L.E_STATE and "previous transforms" in err(pt)
    pt.ctx.set_prev_transforms(prev + [mw.EYE])
    assert launch(pt, "motion", W, H, 1, g, [img]) == L.E_STATE and "previous transforms" in err(pt)
    pt.ctx.set_prev_transforms(prev)
    # a bad matrix is refused and changes nothing
    for bad_value, k in ((np.nan, 5), (np.inf, 12), (1e19, 0), (0.5, 3), (1.0, 7), (2.0, 15)):
        arr = np.stack([np.asarray(m, F).T.ravel() for m in prev]).astype(F)
        arr[4, k] = bad_value
        assert lib.rt3_scene_set_prev_transforms(pt.ctx.h, arr.ctypes.data, len(arr)) == L.E_INVALID and "previous transform 4" in err(pt), (bad_value, k)
    assert lib.rt3_scene_set_prev_transforms(pt.ctx.h, None, 3) == L.E_INVALID
    assert lib.rt3_scene_set_prev_transforms(None, None, 0) == L.E_INVALID
    same(run_motion(pt, g), first, "Motion after refused transforms")
    # bindings and launch size
    small = pt.rg.image(ImageSize.XY(W - 4, H), L.FORMAT_R32G32B32A32_SFLOAT, "small")
    as_uint = pt.rg.image(ImageSize.FullScreen, L.FORMAT_R32G32B32A32_UINT, "as_uint")
    as_depth = pt.rg.image(ImageSize.FullScreen, L.FORMAT_R32_SFLOAT, "as_depth")
    buf = pt.rg.buffer(W * H * 16, "not_an_image")
    assert launch(pt, "motion", W, H, 1, g, []) == L.E_INVALID and "1 binding" in err(pt)
    assert launch(pt, "motion", W, H, 1, g, [img, as_depth]) == L.E_INVALID and "1 binding" in err(pt)
    for bad in (small, as_uint, as_depth, buf, 0, 0x7FFFFFFF):
        assert launch(pt, "motion", W, H, 1, g, [bad]) == L.E_INVALID and "'Motion'" in err(pt), bad
    for x, y in ((W - 1, H), (W, H + 1), (math.ceil(W / 8), math.ceil(H / 8))):
        assert launch(pt, "motion", x, y, 1, g, [img]) == L.E_INVALID and "launch size" in err(pt)
    # the motion input of "temporal" is checked at its launch
    g1 = gconst(pt, mw.PARITY_CAMERA, 1, 2, 1)
    pt.reset_history()
    pt.render(g, temporal=True)
    h = pt.render(g1, temporal=True)
    pt.ctx.set_prev_transforms(prev)  # (render() handed over its own: nothing had moved between its two frames)
    names = ["gbuffer", "depth", "light", "prev_gbuffer", "prev_depth", "prev_history", "prev_moments", "accumulated", "history", "moments"]
    good = [h[n] for n in names]
    X, Y = math.ceil(W / 8), math.ceil(H / 8)
    run_motion(pt, g1)
    keep = (pt.accumulated(), *pt.history())
    for bad in (h["accumulated"], h["history"], h["moments"]):
        pt.ctx.set_temporal_motion_input(bad)
        assert launch(pt, "temporal", X, Y, 1, g1, good) == L.E_INVALID and "motion input" in err(pt)
    for bad in (small, as_uint, as_depth, buf, 0x7FFFFFFF):
        pt.ctx.set_temporal_motion_input(bad)
        assert launch(pt, "temporal", X, Y, 1, g1, good) == L.E_INVALID and "motion input" in err(pt)
    assert lib.rt3_temporal_set_motion_input(None, 0) == L.E_INVALID
    for got, want in zip((pt.accumulated(), *pt.history()), keep):  # refused launches wrote nothing
        assert np.array_equal(bits(got), bits(want))
    pt.ctx.set_temporal_motion_input(img)
    assert launch(pt, "temporal", X, Y, 1, g1, good) == 0
    pt.ctx.wait()
    want = rm.temporal(as_orc(g1), *pt.gbuffer(), pt.light(), as_orc(g), *[pt.rg.download(h[n], s, t) for n, s, t in (
        ("prev_gbuffer", (H, W, 4), np.uint32), ("prev_depth", (H, W), F), ("prev_history", (H, W, 4), F), ("prev_moments", (H, W, 4), F))],
        motion=rm.motion(mesh, cur, prev, as_orc(g1), rm.primary_hits(osc, as_orc(g1))))
    for got, ref, what in zip((pt.accumulated(), *pt.history()), want, ("Out", "History", "Moments")):
        same(got, ref, what + " with the motion input")
    assert not np.array_equal(bits(pt.history()[0]), bits(keep[1]))
    pt.ctx.set_temporal_motion_input(0)
    # (NULL, 0): every instance counts as unmoved again
    pt.ctx.set_prev_transforms(None)
    unmoved = run_motion(pt, g)
    same(unmoved, rm.motion(mesh, cur, None, og, hits), "Motion without previous transforms")
    assert set(np.unique(unmoved[..., 3]).tolist()) == {0.0, 1.0}
    # stale vertices
    pt.ctx.set_prev_transforms(prev)
    pt.ctx.update_vertices(mesh.vertices[:3])
    assert launch(pt, "motion", W, H, 1, g, [img]) == L.E_STATE and "vertices were updated" in err(pt)
    pt.ctx.refit_accel()
    same(run_motion(pt, g), first, "Motion after the refit")
    assert launch(pt, "nonesuch", W, H, 1, g, [img]) == L.E_INVALID and "motion" in err(pt)
    pt.close()


def test_world_without_an_instance_list():
    """no rt3_scene_set_instances call: one identity instance of everything, so one previous transform moves the whole scene"""
    mesh = scenes.cornell()
    W, H = 96, 96
    pt = tracer(mesh, (W, H))
    g = gconst(pt, scenes.CORNELL_CAMERA)
    og = as_orc(g)
    hits = rm.primary_hits(orc.Scene(mesh), og)
    same(run_motion(pt, g), rm.motion(mesh, None, None, og, hits), "Motion, nothing set")
    prev = [mw.f32(mw.translate(0.01, 0.0, -0.02))]
    pt.ctx.set_prev_transforms(prev)
    got = run_motion(pt, g)
    same(got, rm.motion(mesh, None, prev, og, hits), "Motion, the whole scene moved")
    assert np.all(got[..., 3] == 2)
    pt.ctx.set_prev_transforms([mw.EYE, mw.EYE])
    assert launch(pt, "motion", W, H, 1, g, [motion_image(pt)]) == L.E_STATE
    pt.close()


# ------------------------------------------------------------------------------------------------ 5. determinism
def test_two_launches_give_identical_bits():
    mesh, cur, prev = mw.parity_world()
    pt = tracer(mesh, (250, 187), instances=cur, mode=1)
    pt.ctx.set_prev_transforms(prev)
    g = gconst(pt, mw.PARITY_CAMERA)
    a = run_motion(pt, g)
    b = run_motion(pt, g)
    assert np.array_equal(bits(a), bits(b)) and (a[..., 3] == 2).any()
    pt.close()


# ------------------------------------------------------------------------------------------------ 6. the PathTracer path
def test_pathtracer_inserts_skips_and_resets():
    W, H = 128, 96
    mesh, inst0 = mw.moving_world(0)
    pt = tracer(mesh, (W, H), instances=inst0)
    other = tracer(mesh, (W, H), instances=inst0)  # the same frames through render() + denoise(temporal=True), the multi-rank root's path
    gs = [gconst(pt, scenes.CORNELL_CAMERA, 1, k + 1, k) for k in range(4)]

    def both(g, inst=None):
        for p in (pt, other):
            if inst is not None:
                p.set_instances(inst)
        h = pt.render(g, temporal=True, denoise=True)
        other.render(g)
        h2 = other.denoise(g, temporal=True)
        assert ("motion" in h) == ("motion" in h2)
        for a, b, what in zip((pt.accumulated(), *pt.history(), pt.denoised()), (other.accumulated(), *other.history(), other.denoised()),
                              ("Out", "History", "Moments", "denoised")):
            same(a, b, what + ": render() against denoise(temporal=True)")
        return h

    h = both(gs[0])
    assert "motion" not in h and [n.name for n in pt.rg.nodes].count("motion") == 0  # no history yet
    h = both(gs[1], mw.moving_world(1)[1])  # moved instances: the node is there and "temporal" reads its image
    assert "motion" in h and [n.name for n in pt.rg.nodes].count("motion") == 1
    M = pt.motion()
    assert (M[..., 3] == 2).mean() > 0.05
    moved = M[..., 3] == 2
    assert (pt.history()[0][..., 3][moved] > 1.5).mean() > 0.7
    same(other.motion(), M, "Motion of the denoise() path")
    h = both(gs[2], mw.moving_world(1)[1])  # the same list again: skipped, and the input is cleared
    assert "motion" not in h and [n.name for n in pt.rg.nodes].count("motion") == 0
    hist = pt.history()[0]
    assert (hist[..., 3] > 2.5).mean() > 0.5
    og = as_orc(gs[2])
    gb, depth = pt.gbuffer()
    prev = [pt.rg.download(h[n], s, t) for n, s, t in (("prev_gbuffer", (H, W, 4), np.uint32), ("prev_depth", (H, W), F),
                                                       ("prev_history", (H, W, 4), F), ("prev_moments", (H, W, 4), F))]
    same(hist, rt.temporal(og, gb, depth, pt.light(), as_orc(gs[1]), *prev)[1], "History of the frame without the node")
    h = both(gs[3], mw.moving_world(3, n_placed=5)[1])  # another count: the history starts over
    assert "motion" not in h
    fg = pt.gbuffer()[1] != BG
    assert np.all(pt.history()[0][..., 3][fg] == 1)
    pt.close()
    other.close()
