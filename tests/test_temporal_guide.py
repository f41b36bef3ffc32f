"""The sample-guided "temporal" pass on the MI355X (k_temporal_guide, rt3_temporal_set_guide_input): bit-for-bit
parity of Out, History and Moments with tests/ref_temporal_guide.py (the numpy float32 restatement that tests/test_temporal_guide_cpu.py
pins) on caller-made images with every edge case, on windows around the tile, and over frame sequences fed back into each other, where
the reference is given the guide images and the Light the GPU wrote; the chain temporal -> guided denoise; the NULL default; every
refusal; and the PathTracer surface."""
import ctypes as C
import math

import numpy as np
import pytest

import ref_guide as rgd
import ref_temporal_guide as rtg
import temporal_guide_worlds as TW
from raytracer3_amd import _lib as L
from raytracer3_amd import scenes
from raytracer3_amd.render_graph import ImageSize
from raytracer3_amd.renderer import Camera, guide_images, prev_guide_images, temporal_images
from support import as_orc, bits, camera, launch, same, tracer, zeros
from test_nee_emissive import make_pt

pytestmark = pytest.mark.gpu

F = np.float32
W, H = TW.WINDOW
NAMES = ("Out", "History", "Moments")
MOVE = ((0.02, 0.0, 0.01), (0.0, 0.0, 0.012))  # per frame: position, direction (a few pixels)
NON_DEFAULT = (dict(flags=L.TEMPORAL_NO_DEMODULATION, alpha=0.0, alpha_moments=0.0),
               dict(max_history=4, normal_cos=0.95, plane_tolerance=0.002))


def as_lib(og):
    """the library's GConst with the bytes of the oracle's"""
    g = L.GConst()
    C.memmove(C.byref(g), C.byref(og), 304)
    return g


# ---------------------------------------------------------------------------------------------------------------- the raw pass
class RawPass:
    """"temporal" with the guide input on caller-made images, through rt3_pass_launch"""

    def __init__(self, window):
        self.window = window
        self.pt = tracer(scenes.cornell(), window)  # (the pass reads no scene; any built context will do)
        rg = self.pt.rg
        full = ImageSize.FullScreen
        self.t = temporal_images(rg)
        self.gb = rg.image(full, L.FORMAT_R32G32B32A32_UINT, "gbuffer")
        self.depth = rg.image(full, L.FORMAT_R32_SFLOAT, "gbuffer_depth")
        self.light = rg.image(full, L.FORMAT_R32G32B32A32_SFLOAT, "Light")
        self.cur, self.prev = guide_images(rg), prev_guide_images(rg)
        t = self.t
        self.bindings = [self.gb, self.depth, self.light, t["prev_gbuffer"], t["prev_depth"], t["prev_history"], t["prev_moments"],
                         t["accumulated"], t["history"], t["moments"]]
        self.size = (math.ceil(window[0] / 8), math.ceil(window[1] / 8), 1)

    def close(self):
        self.pt.close()

    def upload(self, f):
        rg, (w, h) = self.pt.rg, self.window
        for k in TW.KEYS:
            rg.upload(self.cur[k], f["guide"][k])
            rg.upload(self.prev[k], f["prev_guide"][k] if k in f["prev_guide"] else zeros(h, w))
        rg.upload(self.light, f["light"])
        rg.upload(self.t["prev_history"], f["prev_history"])
        rg.upload(self.t["prev_moments"], f["prev_moments"])
        self.g = as_lib(f["g"])
        self.pt.ctx.set_prev_view(as_lib(f["prev_g"]))

    def launch(self, cur=None, prev=None, bindings=None, set_input=True):
        """the return code; the three written images are prefilled with NaN first"""
        rg, (w, h) = self.pt.rg, self.window
        nan = np.full((h, w, 4), np.nan, F)
        for k in ("accumulated", "history", "moments"):
            rg.upload(self.t[k], nan)
        if set_input:
            self.pt.ctx.set_temporal_guide_input(self.cur if cur is None else cur, self.prev if prev is None else prev)
        return launch(self.pt, "temporal", *self.size, self.g, self.bindings if bindings is None else bindings)

    def results(self):
        self.pt.ctx.wait()
        rg, (w, h) = self.pt.rg, self.window
        return tuple(rg.download(self.t[k], (h, w, 4), F) for k in ("accumulated", "history", "moments"))

    def run(self, f, **params):
        self.upload(f)
        self.pt.ctx.set_temporal_params(**params) if params else self.pt.ctx.set_temporal_params()
        assert self.launch() == 0, self.pt.ctx.last_error()
        return self.results()


def compare(got, want, what):
    for a, b, name in zip(got, want, NAMES):
        same(a, b, f"{what} {name}")


def test_pass_on_caller_made_images():
    """the two-quad guides of the CPU tests with every edge case in them -- non-foreground pixels and texels of all four kinds, NaN, Inf,
    huge and far positions, points behind the previous camera -- with Out, History and Moments prefilled with NaN; twice, for determinism"""
    f = TW.edge_case_frame()
    rp = RawPass(TW.WINDOW)
    try:
        for params in (dict(),) + NON_DEFAULT:
            stages = {}
            want = rtg.temporal(*TW.ref_args(f), stages=stages, **dict(rtg.DEFAULTS, **params))
            first = rp.run(f, **params)
            compare(first, want, f"edge cases {params}")
            again = rp.run(f, **params)
            for a, b in zip(first, again):
                assert np.array_equal(bits(a), bits(b)), "deterministic"
            if not params:
                print(f"edge cases: {int(stages['fg'].sum())} foreground pixels, history on {int(stages['has'].sum())}")
                assert stages["has"].sum() > 100 and (stages["fg"] & ~stages["has"]).any()
        # the G-buffer bindings are not read: whatever they hold changes no bit
        junk = np.random.default_rng(1).integers(0, 1 << 32, (H, W, 4), dtype=np.uint64).astype(np.uint32)
        for h in (rp.gb, rp.t["prev_gbuffer"]):
            rp.pt.rg.upload(h, junk)
        for h in (rp.depth, rp.t["prev_depth"]):
            rp.pt.rg.upload(h, np.full((H, W), np.nan, F))
        compare(rp.run(f), rtg.temporal(*TW.ref_args(f)), "edge cases over a junk G-buffer")
    finally:
        rp.close()


@pytest.mark.parametrize("window", ((1, 1), (31, 7), (32, 8), (33, 9), (97, 41)))
def test_windows_around_the_tile(window):
    f = TW.random_frame(window, seed=window[0])
    rp = RawPass(window)
    try:
        for params in (dict(), NON_DEFAULT[1]):
            compare(rp.run(f, **params), rtg.temporal(*TW.ref_args(f), **dict(rtg.DEFAULTS, **params)), f"{window} {params}")
    finally:
        rp.close()


# ---------------------------------------------------------------------------------------------------------------- frame sequences
def room_pt(window=TW.WINDOW):
    import guide_worlds as GW

    mesh, inst, cam_d = GW.open_material_room()
    return make_pt(mesh, window, instances=inst), cam_d, L.F_FACEFORWARD | L.F_SPECULAR, 3


def glass_pt(window=TW.WINDOW, roulette=True):
    import glass_worlds as GL
    import integrator_worlds as IW

    pt = make_pt(GL.glass_room(True), window, sky=IW.room_sky())
    if roulette:
        pt.set_roulette(1, 0.25)
    return pt, IW.ROOM_CAMERA, L.F_NEE_SKY | L.F_SPECULAR | L.F_FACEFORWARD, 6


def check_sequence(pt, gconsts, what, denoise=False, **params):
    """render the frames through refrence_mode (which writes the guide) -> temporal (-> denoise); after every frame Out, History and
    Moments must equal the reference applied to the frame's own Light and guide images and the previous frame's (GPU) guide, History
    and Moments.  Returns the last frame's images and, per frame, History.w."""
    pt.ctx.set_temporal_params(**params) if params else pt.ctx.set_temporal_params()
    pt.reset_history()
    w, h = pt.window
    prev, Ns = None, []
    for k, g in enumerate(gconsts):
        hd = pt.render(g, temporal=True, denoise=denoise)
        assert "motion" not in hd and len({*hd["guide"].values(), *hd["prev_guide"].values()}) == 8
        light, out, guide = pt.light(), pt.accumulated(), pt.guide()
        hist, mom = pt.history()
        if prev is None:  # zeroed history: no tap counts, whatever the previous guide images hold
            prev = (as_orc(g), guide, zeros(h, w), zeros(h, w))
        stages = {}
        want = rtg.temporal(as_orc(g), guide, light, *prev, stages=stages, **dict(rtg.DEFAULTS, **params))
        N = hist[..., 3]
        cover = guide["position"][..., 3]
        print(f"{what} frame {k}: {int(stages['fg'].sum())} foreground pixels, {int(((cover > 0) & (cover < 1)).sum())} partly covered, "
              f"N > 1 on {int((N > 1).sum())}, N max {N.max():.2f}")
        compare((out, hist, mom), want, f"{what} frame {k}")
        if denoise:
            same(pt.denoised(), rtg.denoise(guide, out, moments=mom), f"{what} frame {k} denoised")
        prev = (as_orc(g), guide, hist, mom)
        Ns.append(N)
    return dict(light=light, out=out, hist=hist, mom=mom, guide=guide, fg=stages["fg"], Ns=Ns)


def moving(pt, cam_d, flags, bounces, steps, spp=2, first_frame=1):
    return [pt.make_gconst(camera(cam_d, pt.window, s, MOVE), spp, bounces, frame=first_frame + k, flags=flags) for k, s in enumerate(steps)]


@pytest.mark.parametrize("scene", ("room antialiased", "room aperture", "glass room"))
def test_frame_sequences(scene):
    """five frames along a camera move at 2 spp, default and non-default parameters"""
    import glass_worlds as GL

    pt, cam_d, flags, bounces = glass_pt() if scene == "glass room" else room_pt()
    try:
        pt.set_lens(*{"room antialiased": (0.0, 1.0, 1.0), "room aperture": (0.06, 2.5, 1.0), "glass room": GL.ROOM_LENS}[scene])
        pt.set_guide(True, temporal=True)
        gs = moving(pt, cam_d, flags, bounces, range(5))
        r = check_sequence(pt, gs, scene)
        fg = r["fg"]
        assert fg.any() and (~fg).any(), "foreground and other pixels"
        assert (r["hist"][..., 3][fg] > 2).mean() > 0.5, "it did accumulate"
        assert not np.array_equal(bits(r["out"])[fg], bits(r["light"])[fg])
        assert np.array_equal(bits(r["out"][~fg]), bits(r["light"][~fg])) and not r["hist"][~fg].any() and not r["mom"][~fg].any()
        if scene == "glass room":
            assert pt.roulette_info()[1] > 0, "roulette ended paths"
        for params in NON_DEFAULT:
            r = check_sequence(pt, gs, f"{scene} {params}", **params)
            if "max_history" in params:
                assert r["hist"][..., 3].max() == 4
    finally:
        pt.close()


def test_camera_turned_away_and_back():
    """view A, A, then B (turned by 130 degrees: nothing it sees lay in A's window), then A again, then A: history is lost on the turn, lost
    again on the way back, and restarts"""
    pt, cam_d, flags, bounces = room_pt()
    try:
        pt.set_lens(0.0, 1.0, 1.0)
        pt.set_guide(True, temporal=True)
        d = np.asarray(cam_d["direction"], np.float64)
        a = math.radians(130.0)
        turned = (d[0] * math.cos(a) + d[2] * math.sin(a), d[1], -d[0] * math.sin(a) + d[2] * math.cos(a))
        dirs = (d, d, turned, d, d)
        gs = [pt.make_gconst(Camera(cam_d["position"], x, math.radians(cam_d["fov_deg"]), W / H), 2, bounces, frame=3 + k, flags=flags)
              for k, x in enumerate(dirs)]
        r = check_sequence(pt, gs, "turned away and back")
        fg = [(N > 0) for N in r["Ns"]]
        assert all(fg[k].any() for k in (0, 1, 3, 4))  # (B may look out of the opening)
        assert (r["Ns"][1][fg[1]] == 2).mean() > 0.5, "the static pair accumulated"
        assert np.all(r["Ns"][2][fg[2]] == 1), "turned away: every pixel starts over"
        assert np.all(r["Ns"][3][fg[3]] == 1), "turned back: the history is B's, and is lost"
        assert (r["Ns"][4][fg[4]] == 2).mean() > 0.5, "... and restarts"
    finally:
        pt.close()


def test_temporal_then_guided_denoise_with_the_variance_input():
    pt, cam_d, flags, bounces = room_pt()
    try:
        pt.set_lens(0.0, 1.0, 1.0)
        pt.set_guide(True, temporal=True)
        r = check_sequence(pt, moving(pt, cam_d, flags, bounces, range(6)), "temporal + guided denoise", denoise=True)
        fg = r["fg"]
        old = fg & (r["mom"][..., 3] >= 4)
        assert old.any() and (fg & ~old).any()
        den = pt.denoised()
        assert not np.array_equal(bits(den), bits(rgd.denoise(r["guide"], r["out"]))), "the variance input changed the result"
        assert np.array_equal(bits(den[~fg]), bits(r["out"][~fg]))
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- the default
def test_null_restores_the_gbuffer_pass():
    """after rt3_temporal_set_guide_input(images, images) and (NULL, NULL), "temporal" writes the bits it writes on a context that never
    made the call"""
    window = (64, 48)
    move = ((0.01, 0.0, 0.0), (0.0105, 0.0, 0.0))

    def frames(pt):
        got = []
        for s in range(3):
            pt.render(pt.make_gconst(camera(scenes.CORNELL_CAMERA, window, s, move), 1, 3, frame=2 + s, flags=L.F_FACEFORWARD), temporal=True)
            got.append((pt.accumulated(), *pt.history()))
        return got

    plain = tracer(scenes.cornell(), window)
    want = frames(plain)
    plain.close()
    pt = tracer(scenes.cornell(), window)
    try:
        pt.ctx.set_temporal_guide_input(guide_images(pt.rg), prev_guide_images(pt.rg))
        pt.ctx.set_temporal_guide_input(None, None)
        got = frames(pt)
    finally:
        pt.close()
    assert (want[-1][1][..., 3] > 1).any()
    for k, (a, b) in enumerate(zip(got, want)):
        compare(a, b, f"frame {k}")


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable():
    from raytracer3_amd.render_graph import ImageSize

    f = TW.edge_case_frame()
    rp = RawPass(TW.WINDOW)
    ctx, rg = rp.pt.ctx, rp.pt.rg
    f4 = L.FORMAT_R32G32B32A32_SFLOAT
    try:
        first = rp.run(f)
        compare(first, rtg.temporal(*TW.ref_args(f)), "before the refusals")
        cur, prev, t = rp.cur, rp.prev, rp.t

        def refused(code, word, **kw):
            rc = rp.launch(**kw)
            assert rc == code and word in ctx.last_error(), (kw, rc, ctx.last_error())

        # exactly one NULL: refused at the call, nothing changed
        gi = L.GuideImages(**cur)
        assert ctx.lib.rt3_temporal_set_guide_input(ctx.h, C.byref(gi), None) == L.E_INVALID and "NULL for both" in ctx.last_error()
        assert ctx.lib.rt3_temporal_set_guide_input(ctx.h, None, C.byref(gi)) == L.E_INVALID
        assert ctx.lib.rt3_temporal_set_guide_input(None, None, None) == L.E_INVALID
        with pytest.raises(L.Rt3Error):
            ctx.set_temporal_guide_input(cur, None)
        assert rp.launch(set_input=False) == 0
        compare(rp.results(), first, "after the one-NULL calls: still the guided pass")
        # at launch: a handle that names nothing, a buffer, another format, another size -- in either set
        small = rg.image(ImageSize.XY(W - 3, H), f4, "small")
        buf = rg.buffer(W * H * 16, "a_buffer")
        for key, bad in (("position", 0), ("normal", 0x7FFFFFF0), ("albedo", buf), ("emission", rp.depth), ("position", rp.gb), ("normal", small)):
            refused(L.E_INVALID, f"current image '{key}'", cur=dict(cur, **{key: bad}))
            refused(L.E_INVALID, f"previous image '{key}'", prev=dict(prev, **{key: bad}))
        # the eight are pairwise different
        refused(L.E_INVALID, "different images", cur=dict(cur, normal=cur["position"]))
        refused(L.E_INVALID, "different images", prev=dict(prev, emission=prev["albedo"]))
        refused(L.E_INVALID, "different images", prev=dict(prev, position=cur["position"]))
        refused(L.E_INVALID, "different images", cur=prev, prev=prev)
        # none is an image the pass writes
        for key, name in (("position", "accumulated"), ("normal", "history"), ("albedo", "moments")):
            refused(L.E_INVALID, "'Out', 'History' or 'Moments'", cur=dict(cur, **{key: t[name]}))
            refused(L.E_INVALID, "'Out', 'History' or 'Moments'", prev=dict(prev, **{key: t[name]}))
        # a motion input beside the guide input
        motion = rg.image(ImageSize.FullScreen, f4, "Motion")
        ctx.set_temporal_motion_input(motion)
        refused(L.E_STATE, "motion input")
        ctx.set_temporal_motion_input(0)
        # the previous view is still required
        ctx.set_prev_view(None)
        refused(L.E_STATE, "previous view")
        ctx.set_prev_view(as_lib(f["prev_g"]))
        # a tile partition with two ranks
        ctx.set_tile_partition(W, H, 1, 2)
        refused(L.E_STATE, "other ranks own")
        ctx.set_tile_partition(W, H, 0, 1)
        # the bindings are still validated
        refused(L.E_INVALID, "'gbuffer'", bindings=[rp.light] + rp.bindings[1:])
        refused(L.E_INVALID, "10 bindings", bindings=rp.bindings[:9])
        # ... and the context computes the same frame
        assert rp.launch() == 0
        compare(rp.results(), first, "after the refusals")
    finally:
        rp.close()


# ---------------------------------------------------------------------------------------------------------------- PathTracer
def rmse_over(a, ref, sel):
    return float(np.sqrt(np.mean(((a[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64))[sel]) ** 2)))


def test_pathtracer_static_camera_is_a_mean_of_k_samples():
    """set_guide(True, temporal=True) on the glass room under a static camera, alpha = 0, K = 8 frames of 1 spp at 96 x 64.  On pixels that
    are foreground in all frames N is K within ref_temporal_guide.history_length_bound (the CPU test's bound), and the RMSE of
    `accumulated` against a 4096-spp frame is below 0.5 of the last single frame's: the estimator is a mean of 8 independent samples
    there, so the expectation is 1 / sqrt(8) = 0.354.  Measured: 5762 such pixels, N == 8 exactly, ratio 0.349."""
    window, K = (96, 64), 8
    pt, cam_d, flags, bounces = glass_pt(window, roulette=False)
    try:
        assert pt.ctx.get_lens()[1], "a scene with glass has the per-sample pinhole on"
        pt.set_guide(True, temporal=True)
        cam = camera(cam_d, window)
        pt.render(pt.make_gconst(cam, 4096, bounces, frame=1000, flags=flags))
        ref = pt.light()
        pt.ctx.set_temporal_params(alpha=0.0, alpha_moments=0.0)
        pt.reset_history()
        always = np.ones((window[1], window[0]), bool)
        for k in range(K):
            h = pt.render(pt.make_gconst(cam, 1, bounces, frame=1 + k, flags=flags), temporal=True)
            assert "motion" not in h
            always &= rgd.foreground(pt.guide())[0]
        N = pt.history()[0][..., 3]
        worst = float(np.abs(N[always].astype(np.float64) - K).max())
        e_acc, e_one = rmse_over(pt.accumulated(), ref, always), rmse_over(pt.light(), ref, always)
        print(f"glass room {window[0]} x {window[1]}, K = {K}: {int(always.sum())} pixels foreground in all frames; max |N - K| = {worst:.3e} "
              f"(bound {rtg.history_length_bound(K):.3e}); RMSE against 4096 spp: accumulated {e_acc:.5f}, last frame {e_one:.5f}, ratio {e_acc / e_one:.3f}")
        assert always.sum() > 1000
        assert worst <= rtg.history_length_bound(K)
        assert e_acc < 0.5 * e_one
    finally:
        pt.close()


def test_pathtracer_guide_without_the_keyword_keeps_todays_temporal_frames():
    """set_guide(True) with the default temporal=False: temporal frames have the bits of a tracer whose guide is off, and no guide images"""
    window = (48, 32)
    pt, cam_d, flags, bounces = glass_pt(window)
    try:
        gs = moving(pt, cam_d, flags, bounces, range(3), spp=1)

        def frames(denoise):
            pt.reset_history()
            got = []
            for g in gs:
                h = pt.render(g, temporal=True, denoise=denoise)
                assert "guide" not in h and "prev_guide" not in h
                got.append((pt.accumulated(), *pt.history(), *([pt.denoised()] if denoise else [])))
            return got

        for denoise in (False, True):
            want = frames(denoise)
            pt.set_guide(True)
            got = frames(denoise)
            pt.set_guide(False)
            for k, (a, b) in enumerate(zip(got, want)):
                for x, y in zip(a, b):
                    assert np.array_equal(bits(x), bits(y)), (denoise, k)
        # several ranks cannot run the guided chain: the guide images are not gathered
        pt.set_guide(True, temporal=True)
        pt.n_ranks = 2
        with pytest.raises(ValueError):
            pt.denoise(gs[0], temporal=True)
        pt.n_ranks = 1
        # one rank: denoise(temporal=True) over the last render()'s Light and guide images
        pt.reset_history()
        prev = None
        for g in gs[:2]:
            pt.render(g)
            light, guide = pt.light(), pt.guide()
            pt.denoise(g, temporal=True)
            hist, mom = pt.history()
            if prev is None:
                prev = (as_orc(g), guide, zeros(window[1], window[0]), zeros(window[1], window[0]))
            want = rtg.temporal(as_orc(g), guide, light, *prev)
            compare((pt.accumulated(), hist, mom), want, "denoise(temporal=True)")
            same(pt.denoised(), rtg.denoise(guide, want[0], moments=mom), "denoise(temporal=True) denoised")
            prev = (as_orc(g), guide, hist, mom)
        assert (hist[..., 3] == 2).any()
    finally:
        pt.close()
