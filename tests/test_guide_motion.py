"""Motion under a lens on the MI355X: k_lens_guide_prev alone (self-test op 41) and inside the frame against
tests/ref_guide_motion.py's accumulate_prev, bit for bit, with the per-sample features rebuilt from the camera function and a closest-hit
trace (guide_worlds.sample_features) over the moving and deforming world of tests/guide_motion_worlds.py; Light and the four guide images
untouched by the fifth; the guided "temporal" with the input against ref_guide_motion.temporal, bit for bit, on caller-made images and over
frame sequences chained into the guided "denoise"; every refusal; the PathTracer surface; and what the input gains, measured."""
import numpy as np
import pytest

import deform_worlds as dw
import guide_motion_worlds as GM
import guide_worlds as GW
import motion_worlds as mw
import ref_guide as rgd
import ref_guide_motion as rgm
import ref_temporal_guide as rtg
import temporal_guide_worlds as TW
from raytracer3_amd import _lib as L
from raytracer3_amd.render_graph import ImageSize
from raytracer3_amd.renderer import guide_images, guide_prev_position_image
from support import as_orc, bits, camera, launch, same, zeros
from test_nee_emissive import make_pt, owned_mask
from test_temporal_guide import RawPass, compare

pytestmark = pytest.mark.gpu

F = np.float32
W, H = GM.WINDOW
S_MAX = GM.S_MAX
FLAGS = L.F_FACEFORWARD | L.F_SPECULAR
LENSES = GM.LENSES
SENTINEL = np.array([-123.25, 7.5, -0.0, 3.0], F)


def parity_pt(w, window=GM.WINDOW, **kw):
    """a tracer built for frame 0 of the parity world whose vertices then become frame 1's behind a snapshot, previous transforms set"""
    pt = make_pt(w["before"], window, instances=w["instances"], **kw)
    set_case(pt, w, "both", fresh=True)
    return pt


def set_case(pt, w, case, fresh=False):
    """previous transforms and snapshot of the context as GM.case_args(w, case) names them; the structure is frame 1's afterwards"""
    pv, pm = GM.case_args(w, case)
    ctx = pt.ctx
    ctx.set_prev_transforms(pm)
    if pv is None:
        ctx.forget_prev_vertices()
    else:
        if not fresh:
            ctx.update_vertices(w["prev_vertices"])
            ctx.refit_accel()
        ctx.snapshot_vertices()
    ctx.update_vertices(w["mesh"].vertices)
    ctx.refit_accel()


def window_pixels(w=W, h=H):
    py, px = (a.reshape(-1) for a in np.mgrid[0:h, 0:w])
    return px, py


def raw_frame(pt, g, motion=True):
    """gbuffer -> refrence_mode with the guide output on and, with `motion`, the fifth image: (Light, the four images, the fifth)"""
    rg = pt.rg
    image = guide_prev_position_image(rg)
    pt.ctx.set_guide_output(guide_images(rg))
    pt.ctx.set_guide_motion_output(image if motion else 0)
    h = pt.commands(g, postprocess=False, guide=True)
    rg.draw_frame(h["light"])
    pt.ctx.set_guide_motion_output(0)
    pt.ctx.set_guide_output(None)
    w, hh = pt.window
    return pt.light(), pt.guide(), rg.download(image, (hh, w, 4), F)


def want_image(w, case, f, S, shape=(H, W)):
    R = GM.previous_points(w, case, f, slice(0, S))
    return rgm.accumulate_prev(f["hit"][:S], R, S).reshape(*shape, 4)


@pytest.fixture(scope="module")
def world():
    """the parity world at 67 x 45, one build, and per lens the rebuilt features of samples 0 .. 4 of every pixel of frame 4"""
    w = GM.parity()
    pt = parity_pt(w)
    cam = camera(GM.CAMERA, GM.WINDOW)
    g = pt.make_gconst(cam, S_MAX, 3, frame=4, flags=FLAGS)
    px, py = window_pixels()
    feats = {name: GW.sample_features(pt, g, GM.WINDOW, lens, px, py, S_MAX) for name, lens in LENSES.items()}
    shares, mixed = GM.kind_shares(w, feats["antialiased"])
    print("GPU samples, antialiased: escaped {:.3f}, unmoved {:.3f}, moved {:.3f}, deformed {:.3f}; {} pixels mix kinds".format(*shares, mixed))
    assert min(shares) >= 0.02 and mixed >= 8
    yield pt, cam, w, feats
    pt.close()


# ---------------------------------------------------------------------------------------------------------------- 1 the kernel alone
@pytest.mark.parametrize("npix", (1, 63, 64, 65, 257, W * H))
def test_kernel_on_caller_made_queues(world, npix):
    """op 41 over the world's own hits, with previous transforms only, a snapshot only, both and neither: one, two and three batches, one
    workgroup and three; every intermediate state and the end against the reference, bit for bit.  With neither the words are op 39's
    position words."""
    pt, _, w, feats = world
    f = feats["antialiased"]
    rng = np.random.default_rng(npix)
    px, py = window_pixels()
    kinds = rgm.sample_kinds(w["mesh"], w["prev_vertices"], w["instances"], w["prev_transforms"], f["hit"], f["prim"])
    mixed = np.flatnonzero((kinds != kinds[0]).any(0))
    if npix == 1:
        pick = mixed[:1]
    elif npix == W * H:
        pick = np.arange(W * H)
    else:  # mixed pixels and some of every kind, in no order
        head = np.unique(np.concatenate([mixed[:8], *[np.flatnonzero((kinds == k).all(0))[:6] for k in (rgm.ESCAPED, rgm.UNMOVED, rgm.MOVED, rgm.DEFORMED)]]))
        rest = np.setdiff1d(np.arange(W * H), head)
        pick = rng.permutation(np.concatenate([head, rng.choice(rest, npix - len(head), replace=False)]))
    assert len(pick) == npix
    sub = {k: v[:, pick] for k, v in f.items()}
    if npix > 1:
        assert {rgm.ESCAPED, rgm.UNMOVED, rgm.MOVED, rgm.DEFORMED} <= set(kinds[:, pick].ravel().tolist())
    pixels = (px[pick] | (py[pick] << 16)).astype(np.uint32)
    garbage = rng.integers(0, 1 << 32, (npix, 4), dtype=np.uint64).astype(np.uint32)  # a first batch does not read what the image holds
    try:
        for case in ("both", "transforms", "neither", "snapshot"):
            set_case(pt, w, case)
            R = GM.previous_points(w, case, sub)
            for plan in ((5,), (2, 3), (1, 2, 2)):
                for groups in (1, 3):
                    state, words, s0 = None, garbage, 0
                    for nsb in plan:
                        sl = slice(s0, s0 + nsb)
                        first, last = s0 == 0, s0 + nsb == S_MAX
                        state = rgm.accumulate_prev(sub["hit"][sl], R[sl], S_MAX, state, first=first, last=last)
                        words = pt.ctx.selftest_guide_prev_queue(pixels, GW.queue_records(sub, sl), nsb, S_MAX, first, last, groups, prefill=words)
                        bad = (words != bits(state)).any(-1)
                        assert not bad.any(), (f"{case} npix {npix} plan {plan} groups {groups} batch at {s0}: {int(bad.sum())} pixels differ, "
                                               f"first {np.flatnonzero(bad)[:3].tolist()}")
                        s0 += nsb
            if case == "neither":
                guide = pt.ctx.selftest_guide_queue(pixels, GW.queue_records(sub), S_MAX, S_MAX, True, True, 1)
                assert np.array_equal(words, guide[:, :4]), "nothing moved: the position image"
            elif npix > 1:
                assert not np.array_equal(words, bits(rgm.accumulate_prev(sub["hit"], GM.previous_points(w, "neither", sub), S_MAX)))
    finally:
        set_case(pt, w, "both")


def test_kernel_selftest_refuses_bad_input(world):
    pt, _, w, feats = world
    f = {k: v[:, :4] for k, v in feats["pinhole"].items()}
    pixels = np.array([0, 1, 2, 3], np.uint32)
    rec = GW.queue_records(f, slice(0, 1))
    ok = lambda **kw: pt.ctx.selftest_guide_prev_queue(**dict(dict(pixels=pixels, records=rec, nsb=1, samples=1, first=True, last=True, groups=1), **kw))  # noqa: E731
    ok()
    bad_prim = rec.copy()
    bad_prim[2, 9] = 0x7FFFFFFF
    for kw in (dict(groups=0), dict(groups=65536), dict(samples=0), dict(nsb=2), dict(pixels=np.array([0, 1, 1, 3], np.uint32)), dict(records=bad_prim)):
        with pytest.raises(L.Rt3Error) as e:
            ok(**kw)
        assert e.value.code == L.E_INVALID, kw
    pt.ctx.set_prev_transforms(w["prev_transforms"][:-1])  # motion_tables' own refusal
    with pytest.raises(L.Rt3Error) as e:
        ok()
    assert e.value.code == L.E_STATE and "previous transforms" in pt.ctx.last_error()
    pt.ctx.set_prev_transforms(w["prev_transforms"])
    ok()


# ---------------------------------------------------------------------------------------------------------------- 2 the frame's image
@pytest.mark.parametrize("lens", sorted(LENSES))
def test_frame_image(world, lens):
    """S = 1 and 5; RT3_OPT_BATCH_SPP 0, 1 and 2: the same bits, the reference's; Light and the four guide images keep theirs"""
    pt, cam, w, feats = world
    f = feats[lens]
    pt.set_lens(*LENSES[lens])
    try:
        for S in (1, S_MAX):
            g = pt.make_gconst(cam, S, 3, frame=4, flags=FLAGS)
            want = want_image(w, "both", f, S)
            z = np.zeros(f["o"][:S].shape, F)
            position = rgd.accumulate(f["hit"][:S], f["o"][:S], f["d"][:S], f["t"][:S], z, z, z, S)["position"].reshape(H, W, 4)
            light0, guide0, _ = raw_frame(pt, g, motion=False)
            same(guide0["position"], position, f"{lens} S={S} position")
            for batch in (0, 1, 2):
                pt.ctx.set_option(L.OPT_BATCH_SPP, batch)
                light, guide, image = raw_frame(pt, g)
                same(image, want, f"{lens} S={S} batch={batch}")
                same(light, light0, f"{lens} S={S} batch={batch} Light")
                for k in rgd.KEYS:
                    same(guide[k], guide0[k], f"{lens} S={S} batch={batch} guide '{k}'")
            moved = (bits(want) != bits(position)).any(-1)
            print(f"{lens} S={S}: the image differs from the position image on {int(moved.sum())} of {int((want[..., 3] > 0).sum())} covered pixels")
            assert moved.sum() > 100 and np.array_equal(bits(want[..., 3]), bits(position[..., 3]))
        # nothing moved, nothing deformed: the position image
        set_case(pt, w, "neither")
        _, guide, image = raw_frame(pt, g)
        same(image, guide["position"], f"{lens}: nothing moved")
    finally:
        pt.ctx.set_option(L.OPT_BATCH_SPP, 0)
        set_case(pt, w, "both")


def test_frame_image_in_both_instance_modes_and_under_a_partition(world):
    _, cam, w, feats = world
    want = want_image(w, "both", feats["antialiased"], S_MAX)
    two = parity_pt(w, mode=1)
    try:
        two.set_lens(*LENSES["antialiased"])
        same(raw_frame(two, two.make_gconst(cam, S_MAX, 3, frame=4, flags=FLAGS))[2], want, "instance mode 1")
    finally:
        two.close()
    pattern = np.broadcast_to(SENTINEL, (H, W, 4)).copy()
    for r in range(2):
        part = parity_pt(w, rank=r, n_ranks=2)
        try:
            part.set_lens(*LENSES["antialiased"])
            part.rg.upload(guide_prev_position_image(part.rg), pattern)
            got = raw_frame(part, part.make_gconst(cam, S_MAX, 3, frame=4, flags=FLAGS))[2]
        finally:
            part.close()
        own = owned_mask(W, H, r, 2)
        assert own.any() and not own.all()
        assert np.array_equal(bits(got[own]), bits(want[own])), r
        assert np.array_equal(bits(got[~own]), bits(pattern[~own])), f"rank {r} wrote pixels of another rank"


# ---------------------------------------------------------------------------------------------------------------- 3 "temporal" reads it
class RawMotionPass(RawPass):
    """test_temporal_guide's raw pass with the guide motion input"""

    def __init__(self, window):
        super().__init__(window)
        self.image = guide_prev_position_image(self.pt.rg)

    def run_with(self, f, image, **params):
        self.upload(f)
        self.pt.ctx.set_temporal_params(**params) if params else self.pt.ctx.set_temporal_params()
        if image is not None:
            self.pt.rg.upload(self.image, image)
        self.pt.ctx.set_temporal_guide_motion_input(self.image if image is not None else 0)
        assert self.launch() == 0, self.pt.ctx.last_error()
        self.pt.ctx.set_temporal_guide_motion_input(0)
        return self.results()


def moved_image(f, seed):
    """the position image with a share of the texels displaced: by a few centimetres (the taps of other pixels), far away, and to NaN"""
    rng = np.random.default_rng(seed)
    Hh, Ww = f["light"].shape[:2]
    image = f["guide"]["position"].copy()
    kind = rng.integers(0, 10, (Hh, Ww))
    image[..., :3] += np.where((kind < 5)[..., None], rng.normal(0.0, 0.03, (Hh, Ww, 3)), 0.0).astype(F)
    image[kind == 5, :3] += F(40.0)
    image[kind == 6, 0] = np.nan
    image[..., 3] = rng.random((Hh, Ww)).astype(F)  # .w is not read
    return image


@pytest.mark.parametrize("window", ((1, 1), (32, 8), (33, 9), (67, 45)))
def test_temporal_with_the_input_on_caller_made_images(window):
    """over NaN-prefilled outputs; the all-unmoved input gives the bits of no input"""
    f = TW.edge_case_frame() if window == TW.WINDOW else TW.random_frame(window, seed=window[0])
    rp = RawMotionPass(window)
    try:
        image = moved_image(f, 5)
        for params in (dict(), dict(max_history=4, normal_cos=0.95, plane_tolerance=0.002), dict(flags=L.TEMPORAL_NO_DEMODULATION)):
            want = rgm.temporal(*TW.ref_args(f), image, **dict(rtg.DEFAULTS, **params))
            compare(rp.run_with(f, image, **params), want, f"{window} {params}")
        plain = rp.run_with(f, None)
        compare(plain, rtg.temporal(*TW.ref_args(f)), f"{window} no input")
        compare(rp.run_with(f, f["guide"]["position"]), plain, f"{window} the all-unmoved input")
        if window == TW.WINDOW:
            assert not np.array_equal(bits(want[1]), bits(rtg.temporal(*TW.ref_args(f), flags=L.TEMPORAL_NO_DEMODULATION)[1])), "the input is read"
    finally:
        rp.close()


def sequence(mode, lens, K=4, spp=2, denoise=True, check=True, feed=True, window=GM.WINDOW, world_at=dw.world, move=GM.CAMERA_MOVE, cam_d=GM.CAMERA,
             flags=FLAGS, bounces=3):
    """K frames of the moving and deforming world under a moving camera through PathTracer (update_vertices, set_instances,
    render(temporal=True)) with set_guide(True, temporal=True); with `check` every frame's fifth image, Out, History, Moments and
    `denoised` against the reference over the frame's own Light and guide images and the previous frame's.  Without `feed` the two calls
    are made with 0 whatever moved.  Returns per frame (Light, Out, History, Moments, denoised or Out, the fifth image or None, the guide)."""
    mesh, inst = world_at(0)
    pt = make_pt(mesh, window, instances=inst, mode=mode)
    calls = []
    set_out, set_in = pt.ctx.set_guide_motion_output, pt.ctx.set_temporal_guide_motion_input
    pt.ctx.set_guide_motion_output = lambda image=0: (calls.append(("out", image)), set_out(image if feed else 0))[1]
    pt.ctx.set_temporal_guide_motion_input = lambda image=0: (calls.append(("in", image)), set_in(image if feed else 0))[1]
    w, h = window
    px, py = window_pixels(w, h)
    frames, prev, prev_mesh, prev_inst = [], None, None, None
    try:
        pt.set_lens(*lens)
        pt.set_guide(True, temporal=True)
        for k in range(K):
            mesh, inst = world_at(k)
            if k:
                pt.update_vertices(mesh.vertices)
                pt.set_instances(inst)
            g = pt.make_gconst(camera(cam_d, window, k, move), spp, bounces, frame=k + 1, flags=flags)
            calls.clear()
            hd = pt.render(g, temporal=True, denoise=denoise)
            image_h = guide_prev_position_image(pt.rg)
            assert "motion" not in hd and not any(n.name == "motion" for n in pt.rg.nodes)
            # the two calls: the image after something moved or deformed, 0 on the first frame
            assert calls == [("in", image_h if k else 0), ("out", image_h if k else 0)], calls
            assert ("guide_motion" in hd) == bool(k) and pt.ctx.get_guide_motion_output() == (image_h if k and feed else 0)
            light, out, guide = pt.light(), pt.accumulated(), pt.guide()
            hist, mom = pt.history()
            image = pt.rg.download(image_h, (h, w, 4), F) if k else None
            if prev is None:
                prev = (as_orc(g), guide, zeros(h, w), zeros(h, w))
            if check:
                want_img = None
                if k:
                    f = GW.sample_features(pt, g, window, lens, px, py, spp)
                    R = rgm.previous_points(mesh, prev_mesh.vertices, inst, [m for _, _, m in prev_inst], *GM.prev_args(f))
                    want_img = rgm.accumulate_prev(f["hit"], R, spp).reshape(h, w, 4)
                    same(image, want_img, f"mode {mode} frame {k} the fifth image")
                    assert (bits(image) != bits(guide["position"])).any(-1).sum() > 100
                stages = {}
                want = rgm.temporal(as_orc(g), guide, light, *prev, want_img, stages=stages)
                compare((out, hist, mom), want, f"mode {mode} frame {k}")
                if denoise:
                    same(pt.denoised(), rtg.denoise(guide, out, moments=mom), f"mode {mode} frame {k} denoised")
                print(f"mode {mode} frame {k}: {int(stages['fg'].sum())} foreground pixels, N > 1 on {int((hist[..., 3] > 1).sum())}")
            prev, prev_mesh, prev_inst = (as_orc(g), guide, hist, mom), mesh, inst
            frames.append((light, out, hist, mom, pt.denoised() if denoise else out, image, guide))
        # a frame with nothing moved makes neither call non-zero
        calls.clear()
        hd = pt.render(pt.make_gconst(camera(cam_d, window, K, move), spp, bounces, frame=K + 1, flags=flags), temporal=True, denoise=denoise)
        assert calls == [("in", 0), ("out", 0)] and "guide_motion" not in hd and "motion" not in hd
    finally:
        pt.close()
    return frames


@pytest.mark.parametrize("lens", ("antialiased", "aperture"))
def test_frame_sequences_and_both_instance_modes(lens):
    """four frames at 2 spp, chained into the guided "denoise"; Out, History and Moments are equal between the instance modes"""
    a = sequence(0, LENSES[lens])
    b = sequence(1, LENSES[lens], check=False)
    for k, (fa, fb) in enumerate(zip(a, b)):
        for x, y, name in zip(fa[:5], fb[:5], ("Light", "Out", "History", "Moments", "denoised")):
            same(x, y, f"{lens} frame {k} {name}, instance mode 0 against 1")
    assert (a[-1][2][..., 3] > 2).any(), "history is kept"


# ---------------------------------------------------------------------------------------------------------------- 4 refusals
def test_refusals_change_nothing(world):
    pt, cam, w, feats = world
    ctx, rg = pt.ctx, pt.rg
    f4 = L.FORMAT_R32G32B32A32_SFLOAT
    pt.set_lens(*LENSES["antialiased"])
    g = pt.make_gconst(cam, 2, 2, frame=1, flags=FLAGS)
    light0, guide0, image0 = raw_frame(pt, g)
    imgs, image = guide_images(rg), guide_prev_position_image(rg)
    h = pt.handles
    trace = [h["gbuffer"], h["depth"], h["light"], h["prev"]]
    small = rg.image(ImageSize.XY(W - 3, H), f4, "small")
    buf = rg.buffer(W * H * 16, "a_buffer")
    try:
        assert ctx.get_guide_motion_output() == 0, "off by default"
        ctx.set_guide_motion_output(image)
        # set time: not a live RGBA32F image; nothing changes
        for bad in (buf, h["depth"], h["gbuffer"], 0x7FFFFFF0):
            with pytest.raises(L.Rt3Error) as e:
                ctx.set_guide_motion_output(bad)
            assert e.value.code == L.E_INVALID and ctx.get_guide_motion_output() == image, bad
        assert ctx.lib.rt3_camera_set_guide_motion_output(None, 0) == L.E_INVALID and ctx.lib.rt3_temporal_set_guide_motion_input(None, 0) == L.E_INVALID
        assert ctx.lib.rt3_camera_get_guide_motion_output(ctx.h, None) == L.E_INVALID

        def refused(code, word):
            rc = launch(pt, "refrence_mode", W, H, 1, g, trace)
            assert rc == code and word in ctx.last_error(), (rc, ctx.last_error())

        refused(L.E_STATE, "guide output")  # no four-image guide output
        ctx.set_guide_output(imgs)
        for bad, word in ((small, "guide motion output"), (imgs["position"], "four guide images"), (imgs["emission"], "four guide images"),
                          (h["light"], "'Light' or 'PrevLight'"), (h["prev"], "'Light' or 'PrevLight'")):
            ctx.set_guide_motion_output(bad)
            refused(L.E_INVALID, word)
        ctx.set_guide_motion_output(image)
        ctx.set_prev_transforms(w["prev_transforms"][:-1])
        refused(L.E_STATE, "previous transforms")
        ctx.set_prev_transforms(w["prev_transforms"])
        ctx.set_lens(None)
        refused(L.E_STATE, "lens")
        ctx.set_lens(aperture_radius=0.0, focus_distance=1.0, pixel_jitter=1.0)
        ctx.set_guide_output(None)
        ctx.set_guide_motion_output(0)
        assert ctx.get_guide_motion_output() == 0
        # the refusals changed nothing: the same frame has the same bits, and 0 restores the frame without the image
        light, guide, again = raw_frame(pt, g)
        same(light, light0, "Light after the refusals")
        same(again, image0, "the fifth image after the refusals")
        rg.upload(image, np.broadcast_to(SENTINEL, (H, W, 4)).copy())
        light, _, untouched = raw_frame(pt, g, motion=False)
        same(light, light0, "Light with the output off")
        assert np.array_equal(bits(untouched), bits(np.broadcast_to(SENTINEL, (H, W, 4)))), "0: the image is not written"
    finally:
        ctx.set_guide_output(None)
        ctx.set_guide_motion_output(0)
        ctx.set_prev_transforms(w["prev_transforms"])


def test_temporal_refusals_leave_the_context_usable():
    f = TW.edge_case_frame()
    rp = RawMotionPass(TW.WINDOW)
    ctx, rg = rp.pt.ctx, rp.pt.rg
    f4 = L.FORMAT_R32G32B32A32_SFLOAT
    try:
        image = moved_image(f, 5)
        first = rp.run_with(f, image)
        compare(first, rgm.temporal(*TW.ref_args(f), image), "before the refusals")

        def refused(code, word, handle, **kw):
            ctx.set_temporal_guide_motion_input(handle)
            rc = rp.launch(**kw)
            assert rc == code and word in ctx.last_error(), (handle, rc, ctx.last_error())

        small = rg.image(ImageSize.XY(W - 3, H), f4, "small")
        buf = rg.buffer(W * H * 16, "a_buffer")
        for bad in (0x7FFFFFF0, buf, rp.depth, rp.gb, small):
            refused(L.E_INVALID, "guide motion input", bad)
        for bad in (*rp.cur.values(), *rp.prev.values()):
            refused(L.E_INVALID, "eight guide images", bad)
        for name in ("accumulated", "history", "moments"):
            refused(L.E_INVALID, "'Out', 'History' or 'Moments'", rp.t[name])
        # without a guide input
        ctx.set_temporal_guide_input(None, None)
        refused(L.E_STATE, "no guide input", rp.image, set_input=False)
        # the pinhole motion input beside the guide input is still refused
        motion = rg.image(ImageSize.FullScreen, f4, "Motion")
        ctx.set_temporal_motion_input(motion)
        refused(L.E_STATE, "motion input", rp.image)
        ctx.set_temporal_motion_input(0)
        ctx.set_temporal_guide_motion_input(rp.image)
        assert rp.launch() == 0
        compare(rp.results(), first, "after the refusals")
        ctx.set_temporal_guide_motion_input(0)
        assert rp.launch() == 0
        compare(rp.results(), rtg.temporal(*TW.ref_args(f)), "0 restores the default")
    finally:
        rp.close()


# ---------------------------------------------------------------------------------------------------------------- 5 it helps
def test_it_helps_moved_blocks():
    """96 x 64, eight 1-spp antialiased frames of motion_worlds.moving_world, with the input and without it.  The protocol is section 4h's
    (tests/test_motion_cpu.py test_moved_instances_converge), which this world and its blocks' steps were made for: the Cornell camera
    drifting by QUALITY_MOVE a frame, four bounces, RT3_F_FACEFORWARD, the pass's default parameters.  On the foreground pixels whose
    previous point is not their own in the last frame: the mean history length is greater with the input, and the RMSE of `accumulated`
    against a 4096-spp frame of the last view is lower.  Only the direction is asserted; DESIGN.md section 7 has the measured values.
    (Under a camera that stands still the second comparison shows nothing and is not made: a face that slides in its own plane keeps a
    history without the input too -- of other points of the same evenly lit face -- and with the default alpha = 0.2 the blend weight
    max(alpha, 1 / N) is alpha from N = 5 on, so a longer history does not lower the variance further.  Measured so on the first try of
    this test, with the camera of motion_worlds.PARITY_CAMERA at rest: mean N 7.710 against 6.475, RMSE 0.29472 against 0.28296.)"""
    from raytracer3_amd import scenes
    from test_motion_cpu import QUALITY_MOVE

    window, K = (96, 64), 8
    lens = LENSES["antialiased"]
    cam_d, flags, bounces = scenes.CORNELL_CAMERA, L.F_FACEFORWARD, 4
    kw = dict(K=K, spp=1, denoise=False, check=False, window=window, world_at=mw.moving_world, move=QUALITY_MOVE, cam_d=cam_d, flags=flags,
              bounces=bounces)
    fed = sequence(0, lens, **kw)
    plain = sequence(0, lens, feed=False, **kw)
    same(fed[0][2], plain[0][2], "the first frame's History")
    mesh, inst = mw.moving_world(K - 1)
    pt = make_pt(mesh, window, instances=inst)
    try:
        pt.set_lens(*lens)
        pt.render(pt.make_gconst(camera(cam_d, window, K - 1, QUALITY_MOVE), 4096, bounces, frame=1000, flags=flags))
        ref = pt.light()
    finally:
        pt.close()
    image, guide = fed[-1][5], fed[-1][6]
    sel = rgd.foreground(guide)[0] & (bits(image[..., :3]) != bits(guide["position"][..., :3])).any(-1)
    assert sel.sum() > 100
    rm_se = lambda a: float(np.sqrt(np.mean(((a[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64))[sel]) ** 2)))  # noqa: E731
    n_fed, n_plain = float(fed[-1][2][..., 3][sel].mean()), float(plain[-1][2][..., 3][sel].mean())
    e_fed, e_plain = rm_se(fed[-1][1]), rm_se(plain[-1][1])
    print(f"moving blocks {window[0]} x {window[1]}, {K} frames of 1 spp, {int(sel.sum())} moved foreground pixels: mean N with the input {n_fed:.3f}, "
          f"without {n_plain:.3f}; RMSE against 4096 spp with the input {e_fed:.5f}, without {e_plain:.5f}")
    assert n_fed > n_plain
    assert e_fed < e_plain
