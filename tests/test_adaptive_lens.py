"""Coverage mode of the "adaptive" pass on the GPU (rt3_adaptive_set_coverage): with a lens set the pass lists every
pixel of the rank and starts each sample from its own camera ray.

Pinned like the pinhole pass (tests/test_adaptive.py), with "foreground" read as "owned by the rank": a pixel that stopped after n samples
holds the bits "refrence_mode" with the same lens writes at samples = n, and the Moments of the run at one cap, fed to
tests/ref_adaptive.py, predict exactly which pixels go on in the run at the next cap.  The worlds are tests/adaptive_lens_worlds.py's;
every frame of a kind is rendered once per world and shared."""
import numpy as np
import pytest

import adaptive_lens_worlds as alw
import adaptive_worlds as aw
import glass_worlds as GW
import integrator_worlds as IW
import lens_worlds as LW
import orc
import ref_adaptive as ra
from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from support import bits, camera, tracer

pytestmark = pytest.mark.gpu

CAP, CAPS, MIN_SAMPLES, STEP = alw.CAP, alw.CAPS, alw.MIN_SAMPLES, alw.STEP
BACKGROUND = np.float32(L.BACKGROUND_DEPTH)


class LensWorld:
    """one context with a world of adaptive_lens_worlds, its lens set and coverage on; frames are rendered once per distinct request"""

    def __init__(self, world, mesh, sky, cam=None, lens=None, coverage=True, pane_shadows=False, roulette=None, **kw):
        self.world = world
        self.W, self.H = self.window = world["window"]
        self.pt = pt = tracer(mesh, self.window, sky=sky, bluenoise=assets.load_bluenoise(), **kw)
        if pane_shadows:
            pt.set_pane_shadows(True)
        if roulette is not None:
            pt.set_roulette(*roulette)
        pt.set_lens(*(lens if lens is not None else world["lens"]))
        pt.set_adaptive_coverage(coverage)
        self.cam = camera(cam if cam is not None else world["camera"], self.window)
        self.cache = {}

    def close(self):
        self.pt.close()

    def frame_args(self, flags=None, bounces=None, blend=1.0, frame=alw.FRAME):
        return (self.world["flags"] if flags is None else flags, self.world["bounces"] if bounces is None else bounces, blend, frame)

    def gconst(self, samples, flags, bounces, blend, frame):
        return self.pt.make_gconst(self.cam, samples=samples, bounces=bounces, frame=frame, blendfactor=blend, flags=flags)

    def fixed(self, samples, **frame):
        """Light of a "refrence_mode" frame with the world's lens"""
        key = ("fixed", samples, *self.frame_args(**frame))
        if key not in self.cache:
            self.pt.render(self.gconst(samples, *self.frame_args(**frame)))
            self.cache[key] = self.pt.light()
        return self.cache[key]

    def adaptive(self, cap=CAP, cached=True, flags=None, bounces=None, blend=1.0, frame=alw.FRAME, **kw):
        """(Light, Moments, (rounds, paths_traced, pixels_capped), depth) of an "adaptive" frame under alw.params(world, **kw)"""
        p = alw.params(self.world, **kw)
        args = self.frame_args(flags, bounces, blend, frame)
        key = ("adaptive", cap, *args, tuple(sorted(p.items())))
        if key not in self.cache or not cached:
            self.pt.render(self.gconst(cap, *args), adaptive=L.AdaptiveParams(**p))
            self.cache[key] = (self.pt.light(), self.pt.adaptive_moments(), self.pt.ctx.adaptive_info(), self.pt.gbuffer()[1])
        return self.cache[key]


def make_a(sky=None, **kw):
    return LensWorld(alw.A, scenes.cornell(), sky if sky is not None else aw.sky(), **kw)


def make_b(**kw):
    return LensWorld(alw.B, GW.glass_room(), IW.room_sky(), **kw)


@pytest.fixture(scope="module")
def world_a():
    w = make_a()
    yield w
    w.close()


@pytest.fixture(scope="module")
def world_b():
    w = make_b()
    yield w
    w.close()


@pytest.fixture(scope="module")
def worlds(world_a, world_b):
    return {"A": world_a, "B": world_b}


def owned_pixels(W, H, rank=0, n_ranks=1):
    xy = orc.tile_pixels(W, H, rank, n_ranks)
    o = np.zeros((H, W), bool)
    o[xy[:, 1], xy[:, 0]] = True
    return o


def counts_of(moments, owned):
    """the integer sample counts; no owned pixel has 0, every other pixel has"""
    n = moments[..., 2]
    assert np.array_equal(n, np.round(n)) and (n[~owned] == 0).all() and (n[owned] >= 1).all()
    return n.astype(np.int64)


def check_against_fixed(w, light, moments, owned, cap=CAP, **frame):
    """every owned pixel holds the bits of the fixed lens frame of its own count (at most six such frames); the other pixels' Moments are 0"""
    n = counts_of(moments, owned)
    distinct = sorted(set(n[owned].tolist()))
    assert set(distinct) <= set(CAPS), distinct
    for k in distinct:
        sel = owned & (n == k)
        fixed = w.fixed(k, **frame)
        differ = (bits(light)[sel] != bits(fixed)[sel]).any(-1)
        assert not differ.any(), f"{differ.sum()} of {sel.sum()} pixels with n = {k} differ"
    assert np.array_equal(moments[..., 3][owned], (n[owned] < cap).astype(np.float32))
    assert (bits(moments)[~owned] == 0).all()
    return n


def check_info(info, n, owned, cap=CAP):
    assert info[1] == n[owned].sum() and info[2] == (owned & (n == cap)).sum()


def everything(w):
    return np.ones((w.H, w.W), bool)


# ---------------------------------------------------------------------------------------------------------------- 1 coverage, closed form
RECT_FRAME = 3  # (the first frame number tried: a background pixel of row 16 goes past round 0 in it)


def test_partly_covered_pixels_are_sampled_on():
    """lens_worlds' emissive rectangle before a constant sky, one bounce, antialiased: a sample is Le inside the rectangle and the sky
    outside it.  A pixel whose box lies wholly inside or outside has constant samples and stops after round 0; only the pixels the outline
    crosses (columns 9 and 20, rows 5 and 16) can go on -- among them pixels of row 16, whose centres see the background (coverage 0.25:
    four samples agree with probability 0.75^4 + 0.25^4 = 0.32, so none of its ten pixels going on has probability 1e-5)."""
    world = dict(name="rect", window=LW.WINDOW, camera=LW.CAMERA, lens=(0.0, 1.0, 1.0), bounces=1, flags=0, threshold={0: 0.01})
    mesh, _ = LW.quad(LW.rect_corners(), LW.RECT_DEPTH)
    w = LensWorld(world, mesh, LW.constant_sky())
    try:
        light, moments, info, depth = w.adaptive(dilate=0, frame=RECT_FRAME)
        owned = everything(w)
        n = check_against_fixed(w, light, moments, owned, frame=RECT_FRAME)
        check_info(info, n, owned)
        x0, x1, y0, y1 = LW.RECT_PX
        cx0, cx1, cy0, cy1 = int(x0), int(x1), int(y0), int(y1)
        assert (cx0, cx1, cy0, cy1) == (9, 20, 5, 16)
        py, px = np.mgrid[0:w.H, 0:w.W]
        outline = (((px == cx0) | (px == cx1)) & (py >= cy0) & (py <= cy1)) | (((py == cy0) | (py == cy1)) & (px >= cx0) & (px <= cx1))
        went_on = n > MIN_SAMPLES
        assert went_on.any() and not (went_on & ~outline).any()
        assert (moments[..., 3][~outline] == 1).all() and (n[~outline] == MIN_SAMPLES).all()
        bg = depth == BACKGROUND
        assert (bg[cy1] & outline[cy1]).sum() == cx1 - cx0 + 1, "row 16: every centre is outside the rectangle"
        assert (went_on & bg).any(), "a pixel whose G-buffer depth is the background's is sampled past round 0"
        print(f"{went_on.sum()} of {outline.sum()} outline pixels went on, {(went_on & bg).sum()} of them background in the G-buffer; counts {np.unique(n)}")
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------------------------- 2 bit-exact against the fixed pass
@pytest.mark.parametrize("flags", [0, L.F_NEE_SKY | L.F_SPECULAR | L.F_BLUENOISE, L.F_NEE_EMISSIVE, aw.FLAGS],
                         ids=["flags0", "sky_specular_bluenoise", "nee_emissive", "fixture"])
def test_world_a_holds_the_fixed_frames_bits(world_a, flags):
    light, moments, info, depth = world_a.adaptive(flags=flags)
    owned = everything(world_a)
    assert 0 < (depth == BACKGROUND).sum() < depth.size
    n = check_against_fixed(world_a, light, moments, owned, flags=flags)
    check_info(info, n, owned)


def test_world_a_with_blendfactor(world_a):
    prev = np.random.default_rng(7).random((world_a.H, world_a.W, 4)).astype(np.float32)
    world_a.pt.load_prev(prev)
    light, moments, _, _ = world_a.adaptive(blend=0.25)
    n = check_against_fixed(world_a, light, moments, everything(world_a), blend=0.25)
    assert len(set(n.reshape(-1).tolist())) > 1
    assert np.array_equal(bits(moments), bits(world_a.adaptive()[1]))  # the moments do not know the blend
    assert not np.array_equal(bits(light), bits(world_a.adaptive()[0]))


def test_world_b_holds_the_fixed_frames_bits(world_b):
    light, moments, info, _ = world_b.adaptive()
    owned = everything(world_b)
    n = check_against_fixed(world_b, light, moments, owned)
    check_info(info, n, owned)
    assert len(np.unique(n)) > 1


def test_world_b_with_pane_shadows(world_b):
    w = make_b(pane_shadows=True)
    try:
        assert w.pt.ctx.pane_shadow_info() == 1
        light, moments, info, _ = w.adaptive()
        n = check_against_fixed(w, light, moments, everything(w))
        check_info(info, n, everything(w))
        assert len(np.unique(n)) > 1
        assert not np.array_equal(bits(light), bits(world_b.adaptive()[0])), "the pane's shadow rays change the frame"
    finally:
        w.close()


def test_world_b_with_roulette(world_b):
    w = make_b(roulette=(1, 1.0 / 16.0))
    try:
        light, moments, info, _ = w.adaptive()
        tested, ended = w.pt.roulette_info()
        assert 0 < ended < tested
        n = check_against_fixed(w, light, moments, everything(w))
        check_info(info, n, everything(w))
        assert not np.array_equal(bits(light), bits(world_b.adaptive()[0]))
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------------------------- 3 the decisions
def predicted_shares(w, threshold, dilate):
    """ref_adaptive.simulate over per-sample luminances rebuilt in float64 from "refrence_mode" lens frames of samples = 1 .. CAP: the
    shares of the pixels it has stop before the cap and reach it"""
    wts = np.array(ra.LUMA, np.float64)
    totals = np.stack([(w.fixed(k)[..., :3].astype(np.float64) * k) @ wts for k in range(1, CAP + 1)])
    y = np.diff(totals, axis=0, prepend=0.0)
    owned = everything(w)
    n = ra.simulate(y, owned, CAP, **alw.params(w.world, threshold=threshold, dilate=dilate))[0]
    return aw.shares(n, owned)


@pytest.mark.parametrize("name", ["A", "B"])
def test_thresholds_were_picked_on_predictions(worlds, name):
    w = worlds[name]
    for dilate in (0, 1):
        early, full = predicted_shares(w, w.world["threshold"][dilate], dilate)
        print(f"world {name}, dilate {dilate}, threshold {w.world['threshold'][dilate]}: predicted {early:.3f} early, {full:.3f} at the cap")
        assert early >= alw.PREDICTED_SHARE and full >= alw.PREDICTED_SHARE


@pytest.mark.parametrize("dilate", [0, 1])
@pytest.mark.parametrize("name", ["A", "B"])
def test_decisions_follow_the_reference(worlds, name, dilate):
    w = worlds[name]
    runs = [w.adaptive(cap=c, dilate=dilate) for c in CAPS]
    owned = everything(w)
    p = alw.params(w.world, dilate=dilate)
    for c, (_, m, info, _), (_, m_next, _, _) in zip(CAPS, runs, runs[1:]):
        n, n_next = counts_of(m, owned), counts_of(m_next, owned)
        stay, cnt = ra.next_active(m[..., 0], m[..., 1], n, owned & (n == c), owned, p["threshold"], p["dark"], dilate)
        grows = n_next > n
        assert np.array_equal(stay, grows), f"cap {c} -> {c + STEP}: {(stay != grows).sum()} pixels decided otherwise ({cnt})"
        assert (n_next[grows] == c + STEP).all()
        assert info[0] == c // STEP and info[2] == cnt["active"]
        frozen = ~grows  # a stopped pixel's state is frozen
        assert np.array_equal(bits(m[..., :3])[frozen], bits(m_next[..., :3])[frozen])
    early, full = aw.shares(counts_of(runs[-1][1], owned), owned)
    print(f"world {name}, dilate={dilate}: {early:.3f} of the pixels stop early, {full:.3f} reach the cap")
    assert early >= aw.MIN_SHARE and full >= aw.MIN_SHARE


# ---------------------------------------------------------------------------------------------------------------- 4 edges
def test_threshold_zero_is_the_fixed_frame(world_a):
    light, moments, info, _ = world_a.adaptive(threshold=0.0)
    W, H = world_a.window
    assert info == (CAP // STEP, CAP * W * H, W * H)
    assert (moments[..., 2] == CAP).all() and (moments[..., 3] == 0).all()
    assert np.array_equal(bits(light), bits(world_a.fixed(CAP)))


def test_a_frame_of_sky_alone():
    """the camera looks away from the box into a constant sky, one bounce: every sample of every pixel is the sky, round 0 is the only
    round, and -- unlike the pinhole pass, which lists no pixel here and leaves Light alone -- every pixel is written"""
    w = make_a(sky=LW.constant_sky(), cam=dict(position=(0.0, 1.0, 9.0), direction=(0.0, 0.0, 1.0), fov_deg=40.0))
    try:
        pt, (W, H) = w.pt, w.window
        _, _, _, depth = w.adaptive(flags=0, bounces=1)  # creates the images
        assert (depth == BACKGROUND).all()
        sentinel = (np.random.default_rng(3).random((H, W, 4)) + 2.0).astype(np.float32)  # in [2, 3): no sky value, no count of 4
        pt.rg.upload(pt.handles["light"], sentinel)
        pt.rg.upload(pt.handles["adaptive_moments"], sentinel)
        pt.ctx.stats_reset()
        light, moments, info, _ = w.adaptive(flags=0, bounces=1, cached=False)
        assert info == (1, MIN_SAMPLES * W * H, 0)
        assert pt.ctx.stats().extension_rays == W * H + MIN_SAMPLES * W * H  # the G-buffer's primary rays, then one camera ray per sample
        assert not (bits(light) == bits(sentinel)).all(-1).any() and not (bits(moments) == bits(sentinel)).any()
        assert np.allclose(light[..., :3], np.float32(LW.SKY_C), rtol=1e-5, atol=0) and (bits(light)[..., 3] == 0).all()
        assert (moments[..., 2] == MIN_SAMPLES).all() and (moments[..., 3] == 1).all()
        assert np.array_equal(bits(light), bits(w.fixed(MIN_SAMPLES, flags=0, bounces=1)))
    finally:
        w.close()


def test_batch_split_changes_nothing(world_a):
    light, moments, info, _ = world_a.adaptive()
    world_a.pt.ctx.set_option(L.OPT_BATCH_SPP, 1)
    try:
        light1, moments1, info1, _ = world_a.adaptive(cached=False)
    finally:
        world_a.pt.ctx.set_option(L.OPT_BATCH_SPP, 0)
    assert np.array_equal(bits(light1), bits(light)) and np.array_equal(bits(moments1), bits(moments)) and info1 == info


# ---------------------------------------------------------------------------------------------------------------- 5 partition
def test_tile_partition(world_a):
    W, H = world_a.window
    ranks = [make_a(rank=r, n_ranks=2) for r in range(2)]
    try:
        owned = [owned_pixels(W, H, r, 2) for r in range(2)]
        assert owned[0].any() and owned[1].any() and not (owned[0] & owned[1]).any() and (owned[0] | owned[1]).all()
        # dilate = 0: the result does not depend on the partition
        light, moments, info, _ = world_a.adaptive(dilate=0)
        total = 0
        for o, w in zip(owned, ranks):
            l, m, i, _ = w.adaptive(dilate=0)
            assert np.array_equal(bits(l)[o], bits(light)[o]) and np.array_equal(bits(m)[o], bits(moments)[o])
            assert (bits(m)[~o] == 0).all()  # a rank writes its own pixels only
            assert i[1] == counts_of(m, o)[o].sum()
            total += i[1]
        assert total == info[1]
        # dilate = 1: pixels of other ranks count as passing
        p = alw.params(alw.A, dilate=1)
        for o, w in zip(owned, ranks):
            for c in CAPS[:3]:
                m, m_next = w.adaptive(cap=c, dilate=1)[1], w.adaptive(cap=c + STEP, dilate=1)[1]
                n, n_next = counts_of(m, o), counts_of(m_next, o)
                stay, cnt = ra.next_active(m[..., 0], m[..., 1], n, o & (n == c), o, p["threshold"], p["dark"], 1)
                assert np.array_equal(stay, n_next > n), (c, cnt)
    finally:
        for w in ranks:
            w.close()


# ---------------------------------------------------------------------------------------------------------------- 6 instance modes
def test_two_level_instances_give_the_same_frame():
    mesh, inst = aw.instanced_world()
    world = dict(alw.A, camera=scenes.CORNELL_CAMERA, lens=(0.02, 4.4, 1.0), flags=L.F_NEE_EMISSIVE | L.F_FACEFORWARD,  # focused on the back wall
                 threshold=aw.THRESHOLD)
    frames = []
    for mode in (0, 1):
        w = LensWorld(world, mesh, aw.sky(), instances=inst, mode=mode)
        try:
            frames.append(w.adaptive())
        finally:
            w.close()
    (l0, m0, i0, d0), (l1, m1, i1, d1) = frames
    assert np.array_equal(bits(d0), bits(d1)) and np.array_equal(bits(l0), bits(l1)) and np.array_equal(bits(m0), bits(m1)) and i0 == i1
    assert len(np.unique(m0[..., 2])) > 1 and (m0[..., 2] >= MIN_SAMPLES).all()


# ---------------------------------------------------------------------------------------------------------------- 7 contract
def refused(w, cap=CAP, bounces=None, **kw):
    with pytest.raises(L.Rt3Error) as e:
        w.adaptive(cap=cap, bounces=bounces, cached=False, **kw)
    return e.value.code, str(e.value)


def test_contract_with_a_lens(world_a):
    pt, ctx = world_a.pt, world_a.pt.ctx
    W, H = world_a.window
    light, moments, info, _ = world_a.adaptive()
    assert ctx.adaptive_coverage() is True
    try:
        # the getter round-trips, and a refused value changes nothing
        ctx.adaptive_set_coverage(False)
        assert ctx.adaptive_coverage() is False
        ctx.adaptive_set_coverage(True)
        for bad in (2, -1):
            assert ctx.lib.rt3_adaptive_set_coverage(ctx.h, bad) == L.E_INVALID and "coverage" in ctx.last_error()
            assert ctx.adaptive_coverage() is True
        # a scene change leaves the mode
        pt.set_scene(scenes.cornell(), aw.sky(), assets.load_bluenoise())
        assert ctx.adaptive_coverage() is True
        # coverage off with a lens: refused, Light untouched, info zeroed
        ctx.adaptive_set_coverage(False)
        sentinel = np.random.default_rng(9).random((H, W, 4)).astype(np.float32)
        pt.rg.upload(pt.handles["light"], sentinel)
        code, text = refused(world_a)
        assert code == L.E_STATE and "lens" in text and "rt3_adaptive_set_coverage" in text
        assert np.array_equal(bits(pt.light()), bits(sentinel)) and ctx.adaptive_info() == (0, 0, 0)
        # render() does not switch it on
        assert ctx.adaptive_coverage() is False
        ctx.adaptive_set_coverage(True)
        # the lens rule, the cap as `samples`
        code, text = refused(world_a, cap=(1 << 26) + 1, bounces=4)
        assert code == L.E_INVALID and "2^31" in text and text.count("adaptive") >= 1
        assert np.array_equal(bits(pt.light()), bits(sentinel)) and ctx.adaptive_info() == (0, 0, 0)
        again = world_a.adaptive(cached=False)
        assert np.array_equal(bits(again[0]), bits(light)) and np.array_equal(bits(again[1]), bits(moments)) and again[2] == info
    finally:
        ctx.adaptive_set_coverage(True)


def test_contract_with_glass(world_b):
    pt, ctx = world_b.pt, world_b.pt.ctx
    try:
        # glass and a lens: the glass draws' RNG indices start at 2^30
        code, text = refused(world_b, cap=(1 << 25) + 1, bounces=4)
        assert code == L.E_INVALID and "2^30" in text and "adaptive" in text
        assert ctx.adaptive_info() == (0, 0, 0)
        # glass and no lens: coverage does not stand in for the lens
        pt.set_lens(None)
        assert ctx.adaptive_coverage() is True
        code, text = refused(world_b)
        assert code == L.E_STATE and "rt3_camera_set_lens" in text
        assert ctx.adaptive_info() == (0, 0, 0)
    finally:
        pt.set_lens(*alw.B["lens"])
    assert world_b.adaptive(cached=False)[2] == world_b.adaptive()[2]


def test_coverage_is_inert_without_a_lens():
    """no lens: the pinhole pass, whatever the mode says -- the same bits, background pixels untouched and unlisted"""
    w = make_a(coverage=False)
    try:
        w.pt.set_lens(None)
        off = w.adaptive(threshold=aw.THRESHOLD[1])
        w.pt.ctx.adaptive_set_coverage(True)
        on = w.adaptive(threshold=aw.THRESHOLD[1], cached=False)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((off[0], off[1], off[3]), (on[0], on[1], on[3]))) and off[2] == on[2]
        bg = off[3] == BACKGROUND
        assert bg.any() and (on[1][..., 2][bg] == 0).all() and len(np.unique(on[1][..., 2][~bg])) > 1
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------------------------- 8 fewer rays
def test_fewer_rays_than_the_fixed_frame(world_b):
    pt, ctx = world_b.pt, world_b.pt.ctx
    ctx.stats_reset()
    _, moments, info, _ = world_b.adaptive(cached=False)
    rays = ctx.stats().extension_rays
    assert info[1] == moments[..., 2].astype(np.int64).sum() < CAP * world_b.W * world_b.H
    ctx.stats_reset()
    pt.render(world_b.gconst(CAP, *world_b.frame_args()))
    assert rays < ctx.stats().extension_rays
