"""The "adaptive" pass on the GPU (include/rt3.h: rt3_adaptive_set_params).

The pass is pinned to the fixed pass: a pixel that stopped after n samples must hold the bits "refrence_mode" writes for it in a frame of
samples = n, and "refrence_mode" is pinned to the oracle elsewhere.  Its decisions are pinned to tests/ref_adaptive.py: the Moments of the
run at one cap, fed to the reference, predict exactly which pixels go on in the run at the next cap.  Frames are 67 x 45
(tests/adaptive_worlds.py); every frame of a kind is rendered once and shared."""
import ctypes as C

import numpy as np
import pytest

import adaptive_worlds as aw
import orc
import ref_adaptive as ra
from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from raytracer3_amd.renderer import Camera, PathTracer
from support import bits

pytestmark = pytest.mark.gpu

W, H, CAP = aw.W, aw.H, aw.CAP
CAPS = list(range(aw.MIN_SAMPLES, CAP + 1, aw.STEP))  # 4, 8, ..., 24
U = 2.0 ** -24  # unit roundoff of float32


def camera(cam=aw.CAMERA, window=(W, H)):
    return Camera(cam["position"], cam["direction"], aw.fov(cam), window[0] / window[1])


class World:
    """one context with the fixture's scene in a window (the fixture's 67 x 45 unless told otherwise); frames are rendered once per
    distinct request"""

    def __init__(self, mesh=None, cam=aw.CAMERA, rank=0, n_ranks=1, instances=None, instance_mode=0, window=(W, H)):
        self.pt = pt = PathTracer(tuple(window), rank=rank, n_ranks=n_ranks)
        if instance_mode:
            pt.ctx.set_option(L.OPT_INSTANCE_MODE, instance_mode)
        pt.set_scene(mesh if mesh is not None else scenes.cornell(), aw.sky(), assets.load_bluenoise())
        if instances is not None:
            pt.set_instances(instances)
        self.cam = camera(cam, window)
        self.cache = {}

    def close(self):
        self.pt.close()

    def gconst(self, samples, flags, bounces, blend, frame):
        return self.pt.make_gconst(self.cam, samples=samples, bounces=bounces, frame=frame, blendfactor=blend, flags=flags)

    def fixed(self, samples, flags=aw.FLAGS, bounces=aw.BOUNCES, blend=1.0, frame=aw.FRAME):
        """Light of a "refrence_mode" frame"""
        key = ("fixed", samples, flags, bounces, blend, frame)
        if key not in self.cache:
            self.pt.render(self.gconst(samples, flags, bounces, blend, frame))
            self.cache[key] = self.pt.light()
        return self.cache[key]

    def adaptive(self, cap=CAP, flags=aw.FLAGS, bounces=aw.BOUNCES, blend=1.0, frame=aw.FRAME, cached=True, **kw):
        """(Light, Moments, (rounds, paths_traced, pixels_capped), depth) of an "adaptive" frame under aw.params(**kw)"""
        p = aw.params(**kw)
        key = ("adaptive", cap, flags, bounces, blend, frame, tuple(sorted(p.items())))
        if key not in self.cache or not cached:
            self.pt.render(self.gconst(cap, flags, bounces, blend, frame), adaptive=L.AdaptiveParams(**p))
            self.cache[key] = (self.pt.light(), self.pt.adaptive_moments(), self.pt.ctx.adaptive_info(), self.pt.gbuffer()[1])
        return self.cache[key]


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def counts_of(moments, fg):
    n = moments[..., 2]
    assert np.array_equal(n, np.round(n)) and (n[~fg] == 0).all()
    return n.astype(np.int64)


def check_against_fixed(w, light, moments, fg, cap=CAP, **frame):
    """every foreground pixel holds the bits of the fixed frame of its own count; at most cap / step such frames"""
    n = counts_of(moments, fg)
    distinct = sorted(set(n[fg].tolist()))
    assert set(distinct) <= set(range(aw.MIN_SAMPLES, cap + 1, aw.STEP)), distinct
    for k in distinct:
        sel = fg & (n == k)
        fixed = w.fixed(k, **frame)
        assert np.array_equal(bits(light)[sel], bits(fixed)[sel]), f"{(bits(light)[sel] != bits(fixed)[sel]).any(-1).sum()} of {sel.sum()} pixels with n = {k} differ"
    assert np.array_equal(moments[..., 3][fg], (n[fg] < cap).astype(np.float32))
    assert (bits(moments)[~fg] == 0).all()
    return n


# ---- 1. bit-exact against the fixed pass
@pytest.mark.parametrize("flags", [0, L.F_NEE_SKY | L.F_SPECULAR | L.F_BLUENOISE, L.F_NEE_EMISSIVE, aw.FLAGS],
                         ids=["flags0", "sky_specular_bluenoise", "nee_emissive", "fixture"])
def test_bit_exact_against_fixed_frames(world, flags):
    light, moments, info, depth = world.adaptive(flags=flags)
    fg = depth != aw.BACKGROUND_DEPTH
    assert 0 < fg.sum() < fg.size
    n = check_against_fixed(world, light, moments, fg, flags=flags)
    assert info[1] == n[fg].sum() and info[2] == (fg & (n == CAP)).sum()


def test_bit_exact_with_blendfactor(world):
    prev = np.random.default_rng(7).random((H, W, 4)).astype(np.float32)
    world.pt.load_prev(prev)
    light, moments, _, depth = world.adaptive(blend=0.25)
    fg = depth != aw.BACKGROUND_DEPTH
    n = check_against_fixed(world, light, moments, fg, blend=0.25)
    assert len(set(n[fg].tolist())) > 1
    # and the moments do not know the blend
    assert np.array_equal(bits(moments), bits(world.adaptive()[1]))


# ---- 2. the decisions
def check_decisions(runs, caps, fg, p):
    """runs[k]: World.adaptive at cap caps[k] under the parameters p.  The Moments of the run at one cap, fed to the reference, say which
    pixels go on in the run at the next; a stopped pixel's state is frozen.  Returns the last run's counts."""
    dilate = p["dilate"]
    for c, (_, m, info, _), (_, m_next, _, _) in zip(caps, runs, runs[1:]):
        n, n_next = counts_of(m, fg), counts_of(m_next, fg)
        stay, cnt = ra.next_active(m[..., 0], m[..., 1], n, fg & (n == c), fg, p["threshold"], p["dark"], dilate)
        grows = n_next > n
        assert np.array_equal(stay, grows), f"cap {c} -> {c + aw.STEP}: {(stay != grows).sum()} pixels decided otherwise ({cnt})"
        assert (n_next[grows] == c + aw.STEP).all()
        assert info[0] == c // aw.STEP and info[2] == cnt["active"]
        frozen = fg & ~grows  # a stopped pixel's state is frozen
        assert np.array_equal(bits(m[..., :3])[frozen], bits(m_next[..., :3])[frozen])
    return counts_of(runs[-1][1], fg)


@pytest.mark.parametrize("dilate", [0, 1])
def test_decisions_follow_the_reference(world, dilate):
    runs = [world.adaptive(cap=c, dilate=dilate) for c in CAPS]
    fg = runs[0][3] != aw.BACKGROUND_DEPTH
    early, full = aw.shares(check_decisions(runs, CAPS, fg, aw.params(dilate=dilate)), fg)
    print(f"dilate={dilate}: {early:.3f} of the foreground stops early, {full:.3f} reaches the cap")
    assert early >= aw.MIN_SHARE and full >= aw.MIN_SHARE


# ---- 3. the moments
def test_moments_against_float64(world):
    """S1 and S2 of a 16 x 12 crop against sums rebuilt in float64 from the fixed frames of samples = 1 .. n.

    The bound (u = 2^-24, first order, samples >= 0).  c_k: the float32 colour sum after k samples, x_k the sample: c_k = fl(c_(k-1) + x_k),
    so |x_k - (c_k - c_(k-1))| <= u c_k.  The fixed frame of k samples holds m_k = fl(c_k / k), so k m_k = c_k (1 + e), |e| <= u, and the
    rebuilt sample x~_k = k m_k - (k - 1) m_(k-1) is within u (c_k + c_(k-1)) of c_k - c_(k-1): |x~_k - x_k| <= 3 u c_n per channel.
    With luminance weights w and Y = w . c_n: the rebuilt y~_k = w . x~_k is within 3 u Y of w . x_k; the kernel's y_k (three products,
    two sums) within 3 u (w . x_k).  So d_k = |y_k - y~_k| <= 3 u (w . x_k) + 3 u Y, and sum d_k <= (3 + 3 n) u Y.
    S1 is a float32 running sum of n terms: within (n - 1) u Y of sum y_k.  Together |S1 - sum y~_k| <= (4 n + 2) u Y.
    S2: fl(y_k^2) is within u y_k^2 of y_k^2, and |y_k^2 - y~_k^2| <= 2 y_k d_k <= 6 u y_k^2 + 6 u y_k Y; summed, with Q = sum y_k^2 and
    the running sum's (n - 1) u Q: |S2 - sum y~_k^2| <= ((n + 6) Q + 6 Y^2) u.  Both bounds get 1 % for the second-order terms."""
    _, moments, _, depth = world.adaptive()
    x0, y0 = 25, 16
    crop = (slice(y0, y0 + 12), slice(x0, x0 + 16))
    assert (depth[crop] != aw.BACKGROUND_DEPTH).all()
    wts = np.array(ra.LUMA, np.float64)
    totals = np.stack([(world.fixed(k)[crop][..., :3].astype(np.float64) * k) @ wts for k in range(1, CAP + 1)])  # sum of y~ up to k
    y = np.diff(totals, axis=0, prepend=0.0)
    sq = np.cumsum(y * y, axis=0)
    n = moments[crop][..., 2].astype(np.int64)
    assert len(np.unique(n)) > 1
    pick = lambda a: np.take_along_axis(a, (n - 1)[None], 0)[0]
    Y, Q = pick(totals), pick(sq)
    s1, s2 = moments[crop][..., 0].astype(np.float64), moments[crop][..., 1].astype(np.float64)
    b1 = 1.01 * (4 * n + 2) * U * Y
    b2 = 1.01 * ((n + 6) * Q + 6 * Y * Y) * U
    r1, r2 = np.abs(s1 - Y) / b1, np.abs(s2 - Q) / b2
    print(f"largest |S1 - ref| / bound = {r1.max():.3f}, largest |S2 - ref| / bound = {r2.max():.3f} over {n.size} pixels, n in {np.unique(n)}")
    assert (Y > 0).all() and r1.max() <= 1.0 and r2.max() <= 1.0


# ---- 4. compaction edges
def test_everything_stops_at_round_zero(world):
    """one bounce: every sample of a pixel is its own emission, the variance is 0 and round 0 is the only round"""
    light, moments, info, depth = world.adaptive(bounces=1, flags=0)
    fg = depth != aw.BACKGROUND_DEPTH
    n = counts_of(moments, fg)
    assert (n[fg] == aw.MIN_SAMPLES).all() and (moments[..., 3][fg] == 1).all()
    assert info == (1, aw.MIN_SAMPLES * int(fg.sum()), 0)
    fixed = world.fixed(aw.MIN_SAMPLES, flags=0, bounces=1)
    assert np.array_equal(bits(light)[fg], bits(fixed)[fg])


def test_threshold_zero_is_the_fixed_frame(world):
    light, moments, info, depth = world.adaptive(threshold=0.0)
    fg = depth != aw.BACKGROUND_DEPTH
    assert info == (CAP // aw.STEP, CAP * int(fg.sum()), int(fg.sum()))
    assert (counts_of(moments, fg)[fg] == CAP).all() and (moments[..., 3] == 0).all()
    assert np.array_equal(bits(light)[fg], bits(world.fixed(CAP))[fg])


def test_one_pixel_stays_active():
    mesh, cam = aw.one_pixel_world()
    w = World(mesh, cam)
    try:
        light, moments, info, depth = w.adaptive(cap=12, flags=0, bounces=2, frame=aw.ONE_PIXEL_FRAME, threshold=0.0, dilate=0)
        fg = depth != aw.BACKGROUND_DEPTH
        n = counts_of(moments, fg)
        assert info == (3, 4 * int(fg.sum()) + 8, 1)
        assert n[H // 2, W // 2] == 12 and (n[fg] == 4).sum() == fg.sum() - 1
        for k in (4, 12):
            sel = fg & (n == k)
            assert np.array_equal(bits(light)[sel], bits(w.fixed(k, flags=0, bounces=2, frame=aw.ONE_PIXEL_FRAME))[sel])
    finally:
        w.close()


def test_all_background_frame(world):
    away = World(cam=dict(position=(0.0, 1.0, 9.0), direction=(0.0, 0.0, 1.0), fov_deg=40.0))
    try:
        pt = away.pt
        light, moments, info, depth = away.adaptive()  # creates the images
        assert (depth == aw.BACKGROUND_DEPTH).all()
        sentinel = np.random.default_rng(3).random((H, W, 4)).astype(np.float32)
        pt.rg.upload(pt.handles["light"], sentinel)
        pt.rg.upload(pt.handles["adaptive_moments"], sentinel)
        pt.ctx.stats_reset()
        light, moments, info, _ = away.adaptive(cached=False)
        assert info == (0, 0, 0)
        assert np.array_equal(bits(light), bits(sentinel)) and (bits(moments) == 0).all()
        s = pt.ctx.stats()
        assert s.extension_rays == W * H and s.shadow_rays == 0  # the G-buffer's primary rays and nothing else
    finally:
        away.close()


# ---- 5. batch split
def test_batch_split_changes_nothing(world):
    light, moments, info, _ = world.adaptive()
    world.pt.ctx.set_option(L.OPT_BATCH_SPP, 1)
    try:
        light1, moments1, info1, _ = world.adaptive(cached=False)
    finally:
        world.pt.ctx.set_option(L.OPT_BATCH_SPP, 0)
    assert np.array_equal(bits(light1), bits(light)) and np.array_equal(bits(moments1), bits(moments)) and info1 == info


# ---- 6. partition
def test_tile_partition(world):
    ranks = [World(rank=r, n_ranks=2) for r in range(2)]
    try:
        owned = []
        for r in range(2):
            xy = orc.tile_pixels(W, H, r, 2)
            o = np.zeros((H, W), bool)
            o[xy[:, 1], xy[:, 0]] = True
            owned.append(o)
        assert owned[0].any() and owned[1].any() and not (owned[0] & owned[1]).any()
        # dilate = 0: the result does not depend on the partition
        light, moments, info, depth = world.adaptive(dilate=0)
        fg = depth != aw.BACKGROUND_DEPTH
        total = 0
        for o, w in zip(owned, ranks):
            l, m, i, _ = w.adaptive(dilate=0)
            assert np.array_equal(bits(l)[o & fg], bits(light)[o & fg]) and np.array_equal(bits(m)[o], bits(moments)[o])
            assert (bits(m)[~o] == 0).all()  # a rank writes its own pixels only
            total += i[1]
        assert total == info[1]
        # dilate = 1: pixels of other ranks count as passing
        p = aw.params(dilate=1)
        for o, w in zip(owned, ranks):
            for c in CAPS[:3]:
                m, m_next = w.adaptive(cap=c, dilate=1)[1], w.adaptive(cap=c + aw.STEP, dilate=1)[1]
                n, n_next = counts_of(m, fg & o), counts_of(m_next, fg & o)
                stay, cnt = ra.next_active(m[..., 0], m[..., 1], n, fg & o & (n == c), fg & o, p["threshold"], p["dark"], 1)
                assert np.array_equal(stay, n_next > n), (c, cnt)
    finally:
        for w in ranks:
            w.close()


# ---- 7. contract
def test_params_validation_leaves_them_unchanged(world):
    ctx = world.pt.ctx
    good = aw.params(threshold=0.2, dilate=0)
    before = world.adaptive(threshold=0.2, dilate=0)[1]
    nan, inf = float("nan"), float("inf")
    bad = [dict(min_samples=1), dict(min_samples=0), dict(step=0), dict(threshold=-0.5), dict(threshold=nan), dict(threshold=inf),
           dict(dark=0.0), dict(dark=-1.0), dict(dark=nan), dict(dark=inf), dict(dilate=2), dict(flags=1), dict(flags=0x80000000)]
    ctx.adaptive_set_params(L.AdaptiveParams(**good))
    for b in bad:
        fields = dict(min_samples=8, step=8, threshold=0.01, dark=0.5, dilate=1, flags=0)  # all of it differs from `good`
        fields.update(b)
        pr = L.AdaptiveParams(**fields)
        assert ctx.lib.rt3_adaptive_set_params(ctx.h, C.byref(pr)) == L.E_INVALID, b
        assert "adaptive params" in ctx.last_error()
    world.pt.render(world.gconst(CAP, aw.FLAGS, aw.BOUNCES, 1.0, aw.FRAME), adaptive=True)  # with the parameters the context holds
    assert np.array_equal(bits(world.pt.adaptive_moments()), bits(before))
    ctx.adaptive_set_params()  # the defaults: 16 samples first
    world.pt.render(world.gconst(CAP, aw.FLAGS, aw.BOUNCES, 1.0, aw.FRAME), adaptive=True)
    fg = world.pt.gbuffer()[1] != aw.BACKGROUND_DEPTH
    assert set(np.unique(world.pt.adaptive_moments()[..., 2][fg])) <= {16.0, 24.0}
    assert ctx.adaptive_info()[0] <= 2


def test_bindings_are_checked(world):
    pt, ctx = world.pt, world.pt.ctx
    world.adaptive()
    h = pt.handles
    g = world.gconst(CAP, aw.FLAGS, aw.BOUNCES, 1.0, aw.FRAME)
    good = [h["gbuffer"], h["depth"], h["light"], h["prev"], h["adaptive_moments"]]

    def launch(b, x=W, y=H):
        return ctx.pass_launch("adaptive", x, y, 1, g, b)

    err = ctx.last_error
    assert launch(good) == 0, err()
    assert launch(good[:4]) == L.E_INVALID and "5 bindings" in err()
    assert launch(good + [h["color"]]) == L.E_INVALID and "5 bindings" in err()
    assert launch(good, W + 1, H) == L.E_INVALID and "launch size" in err()
    assert launch(good[:4] + [h["depth"]]) == L.E_INVALID and "'Moments'" in err()  # R32F, not RGBA32F
    assert launch(good[:4] + [h["gbuffer"]]) == L.E_INVALID and "'Moments'" in err()
    for other in (2, 3):
        assert launch(good[:4] + [good[other]]) == L.E_INVALID and "different images" in err(), other
    assert launch(good) == 0, err()
    ctx.wait()


def test_fewer_rays_than_the_fixed_frame(world):
    pt, ctx = world.pt, world.pt.ctx
    ctx.stats_reset()
    _, moments, info, depth = world.adaptive(cached=False)
    rays = ctx.stats().extension_rays
    fg = depth != aw.BACKGROUND_DEPTH
    assert info[1] == counts_of(moments, fg)[fg].sum()
    ctx.stats_reset()
    pt.render(world.gconst(CAP, aw.FLAGS, aw.BOUNCES, 1.0, aw.FRAME))
    assert rays < ctx.stats().extension_rays


# ---- 8. two-level instances
def test_two_level_instances_give_the_same_frame():
    mesh, inst = aw.instanced_world()
    cam = scenes.CORNELL_CAMERA
    frames = []
    for mode in (0, 1):
        w = World(mesh, cam, instances=inst, instance_mode=mode)
        try:
            frames.append(w.adaptive(flags=L.F_NEE_EMISSIVE | L.F_FACEFORWARD))
        finally:
            w.close()
    (l0, m0, i0, d0), (l1, m1, i1, d1) = frames
    assert np.array_equal(bits(d0), bits(d1)) and np.array_equal(bits(l0), bits(l1)) and np.array_equal(bits(m0), bits(m1)) and i0 == i1
    assert len(np.unique(m0[..., 2])) > 1
