"""Guide images of a lens frame and the "denoise" pass guided by them, on the MI355X: k_lens_guide alone (self-test
op 39) and inside the frame against tests/ref_guide.py's accumulate, bit for bit, with the reference rebuilt from the camera function, a
closest-hit trace and hit_info (guide_worlds.sample_features); the frame's Light untouched by the guide output; the guided pass against
ref_guide.denoise, bit for bit; the modulation round trip; the contract of the three calls; and what the filter gains, measured."""
import math

import numpy as np
import pytest

import guide_worlds as GW
import ref_denoise as rd
import ref_guide as rg
from raytracer3_amd import _lib as L
from raytracer3_amd import scenes
from raytracer3_amd.render_graph import ImageSize
from raytracer3_amd.renderer import guide_images
from support import as_orc, bits, camera, launch
from test_nee_emissive import make_pt, owned_mask

pytestmark = pytest.mark.gpu

F = np.float32
W, H = GW.WINDOW
FLAGS = L.F_FACEFORWARD | L.F_SPECULAR
LENSES = {"pinhole": (0.0, 1.0, 0.0), "antialiased": (0.0, 1.0, 1.0), "aperture": (0.06, 2.5, 1.0)}
S_MAX = 5


def room_pt(window=GW.WINDOW, **kw):
    mesh, inst, cam_d = GW.open_material_room()
    pt = make_pt(mesh, window, instances=inst, **kw)
    return pt, camera(cam_d, window)


def window_pixels(w=W, h=H):
    py, px = (a.reshape(-1) for a in np.mgrid[0:h, 0:w])
    return px, py


def as_images(ref, w=W, h=H):
    return {k: ref[k].reshape(h, w, 4) for k in rg.KEYS}


def guide_frame(pt, cam, lens, S, bounces=3, frame=4, flags=FLAGS, denoise=False):
    """a lens frame with the guide on: (GConst, Light, the four guide images)"""
    pt.set_lens(*lens)
    pt.set_guide(True)
    g = pt.make_gconst(cam, S, bounces, frame=frame, flags=flags)
    pt.render(g, denoise=denoise)
    return g, pt.light(), pt.guide()


def same_images(got, want, what):
    for k in rg.KEYS:
        diff = (bits(got[k]) != bits(want[k])).any(-1)
        assert not diff.any(), f"{what}: '{k}' differs in {int(diff.sum())} pixels, first at {np.argwhere(diff)[:3].tolist()}"


@pytest.fixture(scope="module")
def room():
    """the opened material room at 67 x 45, one build, and per lens the rebuilt features of samples 0 .. 4 of every pixel of frame 4"""
    pt, cam = room_pt()
    g = pt.make_gconst(cam, S_MAX, 3, frame=4, flags=FLAGS)
    px, py = window_pixels()
    feats = {name: GW.sample_features(pt, g, GW.WINDOW, lens, px, py, S_MAX) for name, lens in LENSES.items()}
    yield pt, cam, feats
    pt.close()


# ---------------------------------------------------------------------------------------------------------------- 1 the kernel alone
@pytest.mark.parametrize("npix", (1, 63, 64, 65, 257, W * H))
def test_kernel_on_caller_made_queues(room, npix):
    """op 39 over the room's own hits: one, two and three batches (nsb 5; 2, 3; 1, 2, 2), one workgroup and three (the grid-stride loop);
    every intermediate state -- the running sums between batches -- and the end against the reference, bit for bit.  The library itself
    guards the words behind the queues and the images, and every pixel of the images' bounding box that is not listed."""
    pt, _, feats = room
    f = feats["antialiased"]
    rng = np.random.default_rng(npix)
    px, py = window_pixels()
    nh = f["hit"].sum(0)
    if npix == 1:
        pick = np.flatnonzero((nh > 0) & (nh < S_MAX))[:1]  # a mixed pixel
    elif npix == W * H:
        pick = np.arange(W * H)
    else:  # some of every class, in no order
        classes = [np.flatnonzero(nh == 0), np.flatnonzero(nh == S_MAX), np.flatnonzero((nh > 0) & (nh < S_MAX))]
        head = np.concatenate([c[:8] for c in classes])
        rest = np.setdiff1d(np.arange(W * H), head)
        pick = rng.permutation(np.concatenate([head, rng.choice(rest, npix - len(head), replace=False)]))
    assert len(pick) == npix
    sub = {k: v[:, pick] for k, v in f.items()}
    if npix > 1:
        n_hit = sub["hit"].sum(0)
        assert (n_hit == 0).any() and (n_hit == S_MAX).any() and ((n_hit > 0) & (n_hit < S_MAX)).any(), "all-miss, all-hit and mixed pixels"
    pixels = (px[pick] | (py[pick] << 16)).astype(np.uint32)
    garbage = rng.integers(0, 1 << 32, (npix, 16), dtype=np.uint64).astype(np.uint32)  # a first batch does not read what the images hold
    for plan in ((5,), (2, 3), (1, 2, 2)):
        for groups in (1, 3):
            state, words, s0 = None, garbage, 0
            for nsb in plan:
                sl = slice(s0, s0 + nsb)
                first, last = s0 == 0, s0 + nsb == S_MAX
                state = rg.accumulate(*GW.ref_args(sub, sl), S_MAX, state, first=first, last=last)
                words = pt.ctx.selftest_guide_queue(pixels, GW.queue_records(sub, sl), nsb, S_MAX, first, last, groups, prefill=words)
                want = np.concatenate([bits(state[k]) for k in rg.KEYS], -1)
                bad = (words != want).any(-1)
                assert not bad.any(), f"npix {npix} plan {plan} groups {groups} batch at {s0}: {int(bad.sum())} pixels differ, first {np.flatnonzero(bad)[:3].tolist()}"
                s0 += nsb


def test_kernel_selftest_refuses_bad_input(room):
    pt, _, feats = room
    f = {k: v[:, :4] for k, v in feats["pinhole"].items()}
    pixels = np.array([0, 1, 2, 3], np.uint32)
    rec = GW.queue_records(f, slice(0, 1))
    ok = lambda **kw: pt.ctx.selftest_guide_queue(**dict(dict(pixels=pixels, records=rec, nsb=1, samples=1, first=True, last=True, groups=1), **kw))  # noqa: E731
    ok()
    bad_prim = rec.copy()
    bad_prim[2, 9] = 0x7FFFFFFF
    for kw in (dict(groups=0), dict(groups=65536), dict(samples=0), dict(samples=(1 << 24) + 1), dict(nsb=2), dict(pixels=np.array([0, 1, 1, 3], np.uint32)),
               dict(records=bad_prim)):
        with pytest.raises(L.Rt3Error) as e:
            ok(**kw)
        assert e.value.code == L.E_INVALID, kw
    ok()


# ---------------------------------------------------------------------------------------------------------------- 2 the frame's images
@pytest.mark.parametrize("lens", sorted(LENSES))
def test_frame_guide_images(room, lens):
    """S = 1 and 5; RT3_OPT_BATCH_SPP 1, 2 and unset: the same bits, the reference's"""
    pt, cam, feats = room
    f = feats[lens]
    try:
        for S in (1, S_MAX):
            want = as_images(rg.accumulate(*GW.ref_args(f, slice(0, S)), S))
            for batch in (0, 1, 2):
                pt.ctx.set_option(L.OPT_BATCH_SPP, batch)
                g, _, got = guide_frame(pt, cam, LENSES[lens], S)
                same_images(got, want, f"{lens} S={S} batch={batch}")
            cover = want["position"][..., 3]
            print(f"{lens} S={S}: {int((cover == 1).sum())} covered pixels, {int((cover == 0).sum())} uncovered, {int(((cover > 0) & (cover < 1)).sum())} partly")
            assert (cover == 1).any() and (cover == 0).any()
            if lens == "pinhole" and S == 1:  # the words themselves
                hit = f["hit"][0].reshape(H, W)
                P = (f["o"][0] + f["d"][0] * f["t"][0][:, None]).reshape(H, W, 3)
                assert P.dtype == F and np.array_equal(bits(got["position"][hit][:, :3]), bits(P[hit]))
                for key, name in (("albedo", "albedo"), ("normal", "normal"), ("emission", "emissive")):
                    assert np.array_equal(bits(got[key][hit][:, :3]), bits(f[name][0].reshape(H, W, 3)[hit])), key
                assert np.all(got["albedo"][~hit][:, :3] == 1.0) and not got["position"][~hit].any()
    finally:
        pt.ctx.set_option(L.OPT_BATCH_SPP, 0)


def test_frame_guide_images_in_both_instance_modes_and_under_a_partition(room):
    pt, cam, feats = room
    lens = LENSES["antialiased"]
    want = as_images(rg.accumulate(*GW.ref_args(feats["antialiased"]), S_MAX))
    two, cam2 = room_pt(mode=1)
    try:
        same_images(guide_frame(two, cam2, lens, S_MAX)[2], want, "instance mode 1")
    finally:
        two.close()
    pattern = np.full((H, W, 4), -123.25, F)
    for r in range(2):
        part, camp = room_pt(rank=r, n_ranks=2)
        try:
            for h in guide_images(part.rg).values():
                part.rg.upload(h, pattern)
            got = guide_frame(part, camp, lens, S_MAX)[2]
        finally:
            part.close()
        own = owned_mask(W, H, r, 2)
        assert own.any() and not own.all()
        for k in rg.KEYS:
            assert np.array_equal(bits(got[k][own]), bits(want[k][own])), (r, k)
            assert np.array_equal(bits(got[k][~own]), bits(pattern[~own])), f"rank {r} wrote '{k}' pixels of another rank"


# ---------------------------------------------------------------------------------------------------------------- 3 Light is untouched
def light_with_and_without(pt, cam, S, bounces, flags):
    g = pt.make_gconst(cam, S, bounces, frame=6, flags=flags)
    pt.set_guide(False)
    pt.render(g)
    plain = pt.light()
    pt.set_guide(True)
    pt.render(g)
    assert pt.ctx.get_guide_output()[1] and pt.guide()["position"][..., 3].max() == 1.0
    return plain, pt.light()


def test_guide_output_does_not_perturb_light(room):
    pt, cam, _ = room
    pt.set_lens(*LENSES["aperture"])
    plain, guided = light_with_and_without(pt, cam, 4, 3, FLAGS)
    assert plain[..., :3].max() > 0.0 and np.array_equal(bits(plain), bits(guided))


def test_guide_output_does_not_perturb_a_glass_frame():
    import glass_worlds as GL
    import integrator_worlds as IW

    window = (48, 32)
    pt = make_pt(GL.glass_room(True), window, sky=IW.room_sky())
    try:
        pt.set_pane_shadows(True)
        pt.set_roulette(1, 0.25)
        pt.set_lens(*GL.ROOM_LENS)
        assert pt.ctx.pane_shadow_info() > 0
        plain, guided = light_with_and_without(pt, camera(IW.ROOM_CAMERA, window), 4, 6, L.F_NEE_SKY | L.F_SPECULAR | L.F_FACEFORWARD)
        assert pt.roulette_info()[1] > 0, "roulette ended paths"
    finally:
        pt.close()
    assert plain[..., :3].max() > 0.0 and np.array_equal(bits(plain), bits(guided))


# ---------------------------------------------------------------------------------------------------------------- 4 the guided pass
def check_guided_pass(pt, g, light, guide, what, **params):
    pt.ctx.set_denoise_params(**params) if params else pt.ctx.set_denoise_params()
    pt.render(g, denoise=True)
    assert np.array_equal(bits(pt.light()), bits(light))
    out = pt.denoised()
    want = rg.denoise(guide, light, **dict(rd.DEFAULTS, **params))
    diff = (bits(out) != bits(want)).any(-1)
    assert not diff.any(), f"{what} {params}: {int(diff.sum())} pixels differ, first at {np.argwhere(diff)[:3].tolist()}"
    return out


def test_guided_pass_against_the_reference(room):
    pt, cam, _ = room
    try:
        g, light, guide = guide_frame(pt, cam, LENSES["antialiased"], S_MAX, denoise=True)
        fg, _ = rg.foreground(guide)
        cover = guide["position"][..., 3]
        partly = (cover > 0) & (cover < 1)
        print(f"{int(fg.sum())} foreground pixels, {int(partly.sum())} partly covered, {int((cover == 0).sum())} uncovered")
        assert partly.sum() >= 20 and fg.any()
        for flags in (0, L.DENOISE_NO_DEMODULATION):
            for it in (0, 1, 3, 5):
                out = check_guided_pass(pt, g, light, guide, "room", iterations=it, flags=flags)
                assert np.array_equal(bits(out[~fg]), bits(light[~fg])), "partly covered and uncovered pixels are In, bit for bit"
                assert it == 0 or not np.array_equal(bits(out[fg]), bits(light[fg]))
        # the variance input: a caller-made Moments image overrides the 7 x 7 estimate where its w >= 4, as under the G-buffer guide
        rng = np.random.default_rng(2)
        mom = np.stack([rng.random((H, W)), rng.random((H, W)), rng.gamma(0.5, 0.2, (H, W)), rng.integers(0, 9, (H, W))], -1).astype(F)
        h = pt.handles
        mh = pt.rg.image(ImageSize.FullScreen, L.FORMAT_R32G32B32A32_SFLOAT, "Moments")
        pt.rg.upload(mh, mom)
        pt.ctx.set_denoise_params()
        pt.ctx.set_denoise_variance_input(mh)
        assert launch(pt, "denoise", math.ceil(W / 8), math.ceil(H / 8), 1, g, [h["gbuffer"], h["depth"], h["light"], h["denoised"]]) == 0
        with_var = pt.denoised()
        pt.ctx.set_denoise_variance_input(0)
        stages = {}
        want = rg.denoise(guide, light, moments=mom, stages=stages)
        assert np.array_equal(bits(with_var), bits(want))
        old = fg & (mom[..., 3] >= 4)
        assert old.any() and (fg & ~old).any() and np.array_equal(bits(stages["var0"][old]), bits(mom[..., 2][old]))
        assert not np.array_equal(bits(with_var), bits(rg.denoise(guide, light)))
    finally:
        pt.ctx.set_denoise_params()
        pt.ctx.set_denoise_variance_input(0)


@pytest.mark.parametrize("window", ((33, 9), (1, 40)))
def test_guided_pass_on_small_windows(window):
    pt, cam = room_pt(window)
    try:
        g, light, guide = guide_frame(pt, cam, LENSES["antialiased"], 3, denoise=True)
        for it in (1, 5):
            check_guided_pass(pt, g, light, guide, f"{window}", iterations=it)
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 5 albedo survives
def test_albedo_survives(room):
    """In = emission + 0.37 albedo from the downloaded guide comes back within ref_guide.constant_signal_bound (tests/test_guide_cpu.py)"""
    pt, cam, _ = room
    g, _, guide = guide_frame(pt, cam, LENSES["aperture"], S_MAX, denoise=True)
    fg, _ = rg.foreground(guide)
    k = F(0.37)
    alb, emi = guide["albedo"][..., :3], guide["emission"][..., :3]
    assert np.all(alb[fg] > rd.ALBEDO_FLOOR), "the room's albedo is above the floor: m = albedo"
    assert len(np.unique(alb[fg], axis=0)) > 3 and emi[fg].max() > 0.0
    light = np.concatenate([emi + k * alb, np.ones((H, W, 1), F)], -1).astype(F)
    h = pt.handles
    pt.rg.upload(h["light"], light)
    pt.ctx.set_denoise_params()
    assert launch(pt, "denoise", math.ceil(W / 8), math.ceil(H / 8), 1, g, [h["gbuffer"], h["depth"], h["light"], h["denoised"]]) == 0
    out = pt.denoised()
    err = np.abs(out[..., :3].astype(np.float64) - light[..., :3])
    bound = rg.constant_signal_bound(light, alb, float(k), rd.DEFAULTS["iterations"], fg)
    print(f"albedo round trip: worst |Out - In| {err[fg].max() / rg.U:.2f} units of 2^-24, worst share of the bound {np.max(err[fg] / bound[fg]):.3f}")
    assert np.all(err[fg] <= bound[fg])
    assert np.array_equal(bits(out[~fg]), bits(light[~fg]))


# ---------------------------------------------------------------------------------------------------------------- 6 contract
def test_contract():
    pt, cam = room_pt()
    ctx, rgr = pt.ctx, pt.rg
    f4 = L.FORMAT_R32G32B32A32_SFLOAT
    try:
        g = pt.make_gconst(cam, 2, 2, frame=1, flags=FLAGS)
        pt.set_lens(0.0, 1.0, 1.0)
        pt.render(g, denoise=True)  # guide off: the frame and the pass as they always were
        light0, den0 = pt.light(), pt.denoised()
        gb, depth = pt.gbuffer()
        assert np.array_equal(bits(den0), bits(rd.denoise(as_orc(g), gb, depth, light0))), "guide input NULL: the G-buffer pass, bit for bit"
        h = pt.handles
        imgs = guide_images(rgr)
        good = L.GuideImages(**imgs)
        assert ctx.get_guide_output()[1] is False and ctx.get_guide_output()[0].handles() == (0, 0, 0, 0), "off by default"
        ctx.set_guide_output(good)
        kept = ctx.get_guide_output()
        assert kept[0].handles() == good.handles() and kept[1] is True
        # set time: not a live RGBA32F image, two equal handles; nothing changes
        small = rgr.image(ImageSize.XY(W - 3, H), f4, "small")
        buf = rgr.buffer(W * H * 16, "a_buffer")
        for bad in (dict(imgs, normal=imgs["position"]), dict(imgs, albedo=h["depth"]), dict(imgs, emission=buf), dict(imgs, position=0),
                    dict(imgs, normal=0x7FFFFFF0)):
            with pytest.raises(L.Rt3Error) as e:
                ctx.set_guide_output(bad)
            assert e.value.code == L.E_INVALID, bad
            now = ctx.get_guide_output()
            assert now[0].handles() == good.handles() and now[1] is True
        X, Y = math.ceil(W / 8), math.ceil(H / 8)
        trace = [h["gbuffer"], h["depth"], h["light"], h["prev"]]
        filt = [h["gbuffer"], h["depth"], h["light"], h["denoised"]]
        before = pt.light()

        def refused(name, size, bindings, code, word):
            rc = launch(pt, name, *size, g, bindings)
            assert rc == code and word in ctx.last_error(), (name, rc, ctx.last_error())

        # launch time: wrong size, Light, PrevLight, too many samples, no lens
        for bad, word in ((dict(imgs, albedo=small), "albedo"), (dict(imgs, position=h["light"]), "Light"), (dict(imgs, emission=h["prev"]), "PrevLight")):
            ctx.set_guide_output(bad)
            refused("refrence_mode", (W, H, 1), trace, L.E_INVALID, word)
        ctx.set_guide_output(good)
        many = pt.make_gconst(cam, (1 << 24) + 1, 1, frame=1, flags=FLAGS)
        assert launch(pt, "refrence_mode", W, H, 1, many, trace) == L.E_INVALID and "2^24" in ctx.last_error()
        ctx.set_lens(None)
        refused("refrence_mode", (W, H, 1), trace, L.E_STATE, "lens")
        ctx.set_lens(aperture_radius=0.0, focus_distance=1.0, pixel_jitter=1.0)
        # "adaptive" while the output is set, even in coverage mode
        ctx.adaptive_set_coverage(True)
        mo = rgr.image(ImageSize.FullScreen, f4, "AdaptiveMoments")
        refused("adaptive", (W, H, 1), trace + [mo], L.E_STATE, "guide output")
        ctx.set_guide_output(None)
        assert launch(pt, "adaptive", W, H, 1, pt.make_gconst(cam, 4, 2, frame=1, flags=FLAGS), trace + [mo]) == 0
        ctx.adaptive_set_coverage(False)
        ctx.wait()
        # the guide input: checked at launch like the variance input
        for bad, word in ((dict(imgs, normal=small), "normal"), (dict(imgs, albedo=h["denoised"]), "Out"), (dict(imgs, position=buf), "position"),
                          (dict(imgs, emission=0), "emission"), (dict(imgs, albedo=h["depth"]), "albedo")):
            ctx.set_denoise_guide_input(bad)
            refused("denoise", (X, Y, 1), filt, L.E_INVALID, word)
        ctx.set_denoise_guide_input(good)
        ctx.set_tile_partition(W, H, 1, 2)
        refused("denoise", (X, Y, 1), filt, L.E_STATE, "other ranks own")
        ctx.set_tile_partition(W, H, 0, 1)
        assert ctx.lib.rt3_camera_set_guide_output(None, None) == L.E_INVALID and ctx.lib.rt3_denoise_set_guide_input(None, None) == L.E_INVALID
        # NULL restores today's behaviour: the refusals changed nothing, and the same frame has the same bits
        ctx.set_denoise_guide_input(None)
        assert ctx.get_guide_output()[1] is False and ctx.get_guide_output()[0].handles() == good.handles()
        pt.rg.upload(h["light"], before)
        pt.render(g, denoise=True)
        assert np.array_equal(bits(pt.light()), bits(light0)) and np.array_equal(bits(pt.denoised()), bits(den0))
        # PathTracer: several ranks cannot filter by the sample guide
        pt.set_guide(True)
        pt.n_ranks = 2
        with pytest.raises(ValueError):
            pt.denoise(g)
        pt.n_ranks = 1
        pt.render(g)
        pt.denoise(g)  # one rank: the guide images of the last render()
        assert np.array_equal(bits(pt.denoised()), bits(rg.denoise(pt.guide(), pt.light())))
        pt.set_guide(False)
        pt.render(g, denoise=True)
        assert np.array_equal(bits(pt.denoised()), bits(den0))
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 7 it helps
def rmse(a, ref):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)) ** 2)))


def measure(pt, cam, what, flags, bounces=8, spp=4, ref_spp=4096):
    ref = None
    g = pt.make_gconst(cam, ref_spp, bounces, frame=11, flags=flags)
    pt.set_guide(False)
    pt.render(g)
    ref = pt.light()
    g = pt.make_gconst(cam, spp, bounces, frame=3, flags=flags)
    pt.ctx.set_denoise_params()
    pt.render(g, denoise=True)
    raw, by_gbuffer = pt.light(), pt.denoised()
    pt.set_guide(True)
    pt.render(g, denoise=True)
    assert np.array_equal(bits(pt.light()), bits(raw))
    by_samples = pt.denoised()
    r = rmse(raw, ref), rmse(by_gbuffer, ref), rmse(by_samples, ref)
    fg, _ = rg.foreground(pt.guide())
    print(f"{what}: RMSE against {ref_spp} spp: raw {spp} spp {r[0]:.5f}, filtered by the pinhole G-buffer {r[1]:.5f}, by the sample guide {r[2]:.5f} "
          f"({100.0 * fg.mean():.1f} % of the pixels are foreground to the sample guide)")
    assert r[2] < r[0]
    return r


def test_it_helps_glass_cornell():
    window = (96, 64)
    pt = make_pt(scenes.glass_cornell(), window)
    try:
        measure(pt, camera(scenes.CORNELL_CAMERA, window), "glass_cornell 96 x 64, 8 bounces, per-sample pinhole", L.F_FACEFORWARD)
    finally:
        pt.close()


def test_it_helps_defocused_room():
    from test_lens import material_room_world

    window = (96, 64)
    mesh, inst, cam_d = material_room_world()
    pt = make_pt(mesh, window, instances=inst)
    try:
        pt.set_lens(*LENSES["aperture"])
        measure(pt, camera(cam_d, window), "material room 96 x 64, 8 bounces, aperture 0.06 focused at 2.5", FLAGS)
    finally:
        pt.close()
