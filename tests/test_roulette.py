"""Russian roulette on the GPU (rt3_path_set_roulette): the rule and k_roulette's compaction against
tests/ref_roulette.py bit for bit, the furnace frame against the predictor, the open room against the float64 fixture, "off is the frame
without roulette" and invariance under batch size, instance mode, tile partition and window size, the coupled passes, and the contract of
the calls.

Bounds are derived: fp32 results carry one unit of 2^-24 per rounding of the longest chain; means of bounded samples are held within 5
sigma of the bounded deviation."""
import numpy as np
import pytest

import adaptive_worlds as aw
import combined_worlds as CW
import glass_worlds as GW
import integrator_worlds as IW
import ref_glass as RG
import ref_roulette as RR
from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from support import bits, camera
from test_adaptive import World, check_against_fixed
from test_glass import glass_pt, sky_bound
from test_integrator import furnace_pt
from test_integrator_cpu import LOW_CAP, check_against_fixture, fixture
from test_nee_emissive import frame, make_pt, owned_mask
from test_roulette_cpu import FLOOR, G, op33_rows, predict

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0**-24
FF = L.F_FACEFORWARD
FULL = L.F_NEE_SKY | L.F_BLUENOISE | L.F_FACEFORWARD | L.F_SPECULAR


@pytest.fixture(scope="module")
def ctx():
    """a context with a small world (the self-test ops read no context state)"""
    pt = make_pt(IW.open_room(), IW.WINDOW_ROOM)
    yield pt.ctx
    pt.close()


# ---------------------------------------------------------------------------------------------------------------- 3 the rule
def test_rule_bit_for_bit(ctx):
    total = 0
    for ms, T, u in op33_rows():
        rows = np.concatenate([bits(T), np.full((len(T), 1), F(ms).view(np.uint32)), bits(u)[:, None]], 1).astype(np.uint32)
        out = ctx.selftest(L.SELFTEST_ROULETTE, rows, 5)
        survived, Tn, qg = RR.rule(T, ms, u)
        assert np.array_equal(out[:, 0], survived.astype(np.uint32))
        assert np.array_equal(out[:, 1:4], bits(Tn)) and np.array_equal(out[:, 4], bits(qg))
        total += len(T)
        assert 0 < survived.sum() < len(T) or ms == 1.0
    assert total > 4000


# ---------------------------------------------------------------------------------------------------------------- 4 the compaction
QUEUE_N = (0, 1, 63, 64, 65, 511, 512, 513, 1537)
PATTERN = 0xA5000000


def queue(n, kind, npix, seed):
    """n records with distinct path ids: `kind` says what their throughputs make of them"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 11), np.uint32)
    rec[:, :7] = bits(rng.normal(size=(n, 7)).astype(F))
    rec[:, 3] = np.where(rng.random(n) < 0.3, F(3.4028234663852886e38).view(np.uint32), rec[:, 3])  # delta markers in the pdf slot
    rec[:, 7] = rng.permutation(npix * 64)[:n]
    T = {"everyone ends": np.zeros((n, 3)), "no one ends": 1.0 + rng.random((n, 3)), "mixture": rng.random((n, 3)) ** 2 * rng.choice([0.05, 0.5, 1.2], (n, 1))}[kind]
    if kind == "mixture" and n:
        T[rng.random(n) < 0.1] = 0.0
        T[rng.random(n) < 0.02] = np.nan
    rec[:, 8:] = bits(T.astype(F))
    return rec


@pytest.mark.parametrize("kind", ("everyone ends", "no one ends", "mixture"))
def test_compaction_against_the_reference(ctx, kind):
    npix, frame_no, B, b, s0 = 37, 5, 6, 2, 3
    pixels = (np.arange(npix) * 7 % 64 | ((np.arange(npix) * 5 % 48) << 16)).astype(np.uint32)
    for n in QUEUE_N:
        rec = queue(n, kind, npix, 100 + n)
        prefill = (PATTERN + np.arange(n * 11, dtype=np.uint32)).reshape(n, 11)
        count, tested, ended, dst = ctx.selftest_roulette_queue(frame_no, B, b, s0, FLOOR, pixels, rec, groups=2, prefill=prefill)
        want = RR.compact(rec, pixels, frame_no, B, b, s0, FLOOR)
        assert count == len(want) and (tested, ended) == (n, n - len(want)), (n, count, tested, ended, len(want))
        got = dst[:count]
        assert len(np.unique(got[:, 7])) == count, "no duplicates"
        assert np.array_equal(got[np.argsort(got[:, 7])], want[np.argsort(want[:, 7])]), n
        assert np.array_equal(dst[count:], prefill[count:]), "words beyond the count are untouched"
        if n >= 63:
            assert {"everyone ends": count == 0, "no one ends": count == n, "mixture": 0 < count < n}[kind]
    # inside a workgroup the order is kept: one workgroup's worth keeps the queue's order
    rec = queue(300, "mixture", npix, 9)
    count, _, _, dst = ctx.selftest_roulette_queue(frame_no, B, b, s0, FLOOR, pixels, rec, groups=1)
    assert np.array_equal(dst[:count], RR.compact(rec, pixels, frame_no, B, b, s0, FLOOR))


def test_selftest_queue_refuses_a_bad_header(ctx):
    rec = queue(4, "mixture", 3, 1)
    for kw in (dict(bounces=0), dict(bounces=65), dict(pixels=[]), dict(groups=0), dict(groups=65536)):
        args = dict(frame=0, bounces=4, bounce=1, s0=0, min_survival=FLOOR, pixels=[1, 2, 3], records=rec, groups=2)
        args.update(kw)
        with pytest.raises(L.Rt3Error) as e:
            ctx.selftest_roulette_queue(**args)
        assert e.value.code == L.E_INVALID


# ---------------------------------------------------------------------------------------------------------------- 5 the furnace
def roulette_tolerance(bounces, samples):
    """test_integrator_cpu.furnace_tolerance (one rounding per product and sum) and one more per bounce for the division by q_g"""
    return (3 * bounces + samples + 2) * U


@pytest.mark.parametrize("flags", (0, FF))
def test_furnace_frame_against_the_predictor(flags):
    S = 16
    pt, cam = furnace_pt("world")
    try:
        for B in (2, 4, 8):
            pt.set_roulette(None)
            pt.ctx.stats_reset()
            plain = frame(pt, cam, flags, S, B)
            rays_off = pt.ctx.stats().extension_rays
            assert pt.roulette_info() == (0, 0)
            gb = pt.gbuffer()[0]
            for start in (0, 1, 2):
                pt.set_roulette(start, FLOOR)
                pt.ctx.stats_reset()
                light = frame(pt, cam, flags, S, B).astype(np.float64)
                rays_on = pt.ctx.stats().extension_rays
                tested, ended = pt.roulette_info()
                want, nearest, p_tested, p_ended = predict(gb, B, S, start)
                near = nearest <= 4 * G
                assert near.mean() <= 0.01
                rel = light / want - 1.0
                tol = roulette_tolerance(B, S)
                high, low = (rel > tol).any(-1) & ~near, (rel < -tol).any(-1) & ~near
                print(f"furnace flags={flags} B={B} start={start}: {int(low.sum())} low, {int(high.sum())} high, {int(near.sum())} left out; ended {ended} of {tested} "
                      f"(predictor {p_ended} of {p_tested}); extension rays {rays_on} against {rays_off}")
                assert not high.any(), f"{int(high.sum())} pixels above the prediction, worst {rel[~near].max():+.3e}"
                assert low.mean() <= LOW_CAP
                if start < B - 1:
                    assert 0 < ended < tested <= p_tested and rays_on < rays_off and rays_off - rays_on >= ended
                    assert not np.array_equal(bits(light.astype(F)), bits(plain))
                else:  # nothing is tested: the frame without roulette
                    assert (tested, ended) == (0, 0) and rays_on == rays_off and np.array_equal(bits(light.astype(F)), bits(plain))
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 6 the open room
# What check_against_fixture's own condition (own standard error at most half the fixture's) needs: the case's 8 frames without roulette;
# with it 24 frames came to 0.28 of the fixture's error, so 8 would come to 0.28 sqrt(3) = 0.49 and 12 to 0.40
ROOM_FRAMES = 12


def test_open_room_against_the_fixture():
    name = "sky_b4"
    flags, bounces, specular, _, _, _ = IW.ROOM_CASES[name]
    assert flags & L.F_NEE_SKY
    pt = make_pt(IW.open_room(specular), IW.WINDOW_ROOM, sky=IW.room_sky())
    try:
        pt.set_roulette(1, FLOOR)
        cam = camera(IW.ROOM_CAMERA, IW.WINDOW_ROOM)
        frames = np.stack([frame(pt, cam, flags, IW.FRAME_SPP, bounces, index=k) for k in range(ROOM_FRAMES)])
        tested, ended = pt.roulette_info()
        assert 0 < ended < tested
        check_against_fixture(frames, pt.gbuffer()[1] != L.BACKGROUND_DEPTH, fixture(), name)
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 7 identity
def atrium_world():
    from raytracer3_amd.renderer import PathTracer

    pt = PathTracer((160, 90))
    pt.set_scene(scenes.atrium(0.3), scenes.sky(512, 256), assets.load_bluenoise())
    return pt, camera(scenes.ATRIUM_CAMERA, (160, 90)), L.F_NEE_SKY | L.F_BLUENOISE | L.F_FACEFORWARD, 8, 4, 3


def glass_world():
    pt = make_pt(GW.glass_room(True, 0.5), IW.WINDOW_ROOM, sky=IW.room_sky())
    pt.set_lens(0.05, 6.0, 1.0)
    return pt, camera(IW.ROOM_CAMERA, IW.WINDOW_ROOM), FULL | L.F_NEE_EMISSIVE, 4, 6, 0


def lens_lights_world():
    mesh, lens = CW.world("lens_lights_textures_cutout")
    pt = make_pt(mesh, CW.WINDOW, sky=CW.sky())
    pt.set_lens(*lens)
    return pt, camera(CW.CAMERA, CW.WINDOW), FULL | L.F_NEE_PUNCTUAL | L.F_NEE_EMISSIVE, 4, 3, 1


def light_of(pt, cam, flags, spp, bounces, index):
    pt.render(pt.make_gconst(cam, spp, bounces, frame=index, flags=flags))
    return pt.light()[..., :3].copy()


@pytest.mark.parametrize("world", (atrium_world, glass_world, lens_lights_world), ids=("atrium", "glass", "lens_lights"))
def test_off_is_the_frame_without_roulette(world):
    pt, cam, flags, spp, B, index = world()
    try:
        never = light_of(pt, cam, flags, spp, B, index)  # a context that never heard of roulette
        assert never.max() > 0.0 and pt.roulette_info() == (0, 0)
        for start in (B - 1, B, 1000):
            pt.set_roulette(start, FLOOR)
            assert np.array_equal(bits(light_of(pt, cam, flags, spp, B, index)), bits(never)), start
            assert pt.roulette_info() == (0, 0)
        pt.set_roulette(0, FLOOR)
        on = light_of(pt, cam, flags, spp, B, index)
        tested, ended = pt.roulette_info()
        assert 0 < ended < tested and not np.array_equal(bits(on), bits(never)) and np.isfinite(on).all()
        pt.set_roulette(None)
        assert np.array_equal(bits(light_of(pt, cam, flags, spp, B, index)), bits(never))
        assert pt.roulette_info() == (0, 0)
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 8 invariance
def glass_room_frame(window=IW.WINDOW_ROOM, setup=None, spp=5, **kw):
    pt = make_pt(GW.glass_room(True, 0.5), window, sky=IW.room_sky(), **kw)
    try:
        pt.set_lens(0.05, 6.0, 1.0)
        pt.set_roulette(1, FLOOR)
        if setup:
            setup(pt)
        out = light_of(pt, camera(IW.ROOM_CAMERA, window), FULL | L.F_NEE_EMISSIVE, spp, 6, 0)
        tested, ended = pt.roulette_info()
        assert 0 < ended < tested
        return out
    finally:
        pt.close()


def test_same_bits_for_every_batch_size_and_instance_mode():
    whole = glass_room_frame()
    assert whole.max() > 0.0
    for batch in (1, 3):
        assert np.array_equal(bits(whole), bits(glass_room_frame(setup=lambda pt: pt.ctx.set_option(L.OPT_BATCH_SPP, batch)))), batch
    assert np.array_equal(bits(whole), bits(glass_room_frame(mode=1)))


def test_two_ranks_stitch_to_one():
    W, H = window = (128, 48)
    whole = glass_room_frame(window)
    for r in range(2):
        part = glass_room_frame(window, rank=r, n_ranks=2)
        m = owned_mask(W, H, r, 2)
        assert m.any() and not m.all()
        assert np.array_equal(bits(part[m]), bits(whole[m]))


@pytest.mark.parametrize("window", ((1, 1), (7, 3), (33, 31)))
def test_windows_that_do_not_fill_their_last_workgroup(window):
    """5 samples of 1, 21 and 1023 pixels: 5, 105 and 5115 paths, none a multiple of the 512 of a workgroup.  From the G-buffer (no lens), in
    the open room, whose camera sees a surface in the window's centre: one batch and one batch per sample give the same bits"""
    def shot(batch):
        pt = make_pt(IW.open_room(), window, sky=IW.room_sky())
        try:
            pt.ctx.set_option(L.OPT_BATCH_SPP, batch)
            pt.set_roulette(0, FLOOR)
            out = frame(pt, camera(IW.ROOM_CAMERA, window), L.F_NEE_SKY | FF, 5, 6)
            return out, pt.roulette_info()
        finally:
            pt.close()
    (whole, info), (split, info1) = shot(0), shot(1)
    assert whole.shape[:2] == window[::-1] and np.isfinite(whole).all()
    assert info == info1
    if window != (1, 1):  # (the one pixel may see the background)
        assert whole.max() > 0.0 and 0 < info[1] < info[0]
    assert np.array_equal(bits(whole), bits(split))


# ---------------------------------------------------------------------------------------------------------------- 9 coupled passes
def test_adaptive_pixels_hold_the_fixed_frames_bits():
    """a pixel that stopped at n holds the bits "refrence_mode" writes at samples = n under the same roulette parameters.  (From vertex 0:
    under the fixture's flags the paths of this world, seen from outside, end at their second vertex.)"""
    w = World()
    try:
        w.pt.set_roulette(0, FLOOR)
        light, moments, info, depth = w.adaptive()
        tested, ended = w.pt.roulette_info()
        assert 0 < ended < tested
        fg = depth != aw.BACKGROUND_DEPTH
        check_against_fixed(w, light, moments, fg)
        w.pt.set_roulette(None)
        w.cache.clear()
        assert not np.array_equal(bits(w.fixed(aw.CAP)), bits(light))
    finally:
        w.close()


def test_thin_pane_keeps_its_closed_forms():
    """Roulette from vertex 0 on the thin pane under a constant sky (test_glass has the closed forms).  Untinted, every throughput is 1: no
    number is drawn, k_roulette copies every record, and a pixel off the wall is the sky as before -- the delta markers in the pdf slot
    survived the copy (a lost marker would weight the escaped ray's sky by MIS).  Tinted, B = 2: a transmitted ray survives with probability
    q_g = max c and then carries c / q_g <= 1, so a sample lies in [0, L], its standard deviation is at most L / 2, and a pane row's mean
    lies within 5 L / (2 sqrt(n S)) of mean_p(F'_p L + (1 - F'_p) c L)."""
    SKY = np.array(GW.SKY_L)
    wall, pane = GW.inside(GW.WALL_COLS, GW.PANE_ROWS), GW.inside(GW.PANE_COLS, GW.PANE_ROWS)
    pt = glass_pt(GW.pane_world())
    try:
        pt.set_roulette(0, FLOOR)
        for flags in (L.F_NEE_SKY, 0):
            pt.render(pt.make_gconst(camera(GW.CAMERA, GW.WINDOW), 4, 4, flags=flags))
            got = pt.light()[..., :3].astype(np.float64)
            tested, ended = pt.roulette_info()
            assert tested > 0 and np.abs(got[~wall] / SKY - 1.0).max() <= sky_bound(4)
    finally:
        pt.close()
    S, c = 1024, np.array(GW.TINT)
    pt = glass_pt(GW.pane_world(GW.TINT))
    try:
        pt.set_roulette(0, FLOOR)
        pt.render(pt.make_gconst(camera(GW.CAMERA, GW.WINDOW), S, 2, flags=L.F_NEE_SKY))
        got = pt.light()[..., :3].astype(np.float64)
        tested, ended = pt.roulette_info()
    finally:
        pt.close()
    assert 0 < ended < tested
    Ft = RG.thin_fresnel(RG.fresnel(-GW.pixel_dirs()[..., 2], GW.IOR))
    rows = np.flatnonzero(pane.any(1))
    assert len(rows) >= 30
    worst = 0.0
    for y in rows:
        m = pane[y]
        want = (Ft[y, m, None] * SKY + (1.0 - Ft[y, m, None]) * c * SKY).mean(0)
        band = 5.0 * SKY / (2.0 * np.sqrt(int(m.sum()) * S)) + sky_bound(S) * SKY
        dev = np.abs(got[y, m].mean(0) - want)
        worst = max(worst, float((dev / band).max()))
        assert np.all(dev <= band), (y, dev, band)
    print(f"tinted pane under roulette: worst deviation {worst:.2f} bands over {len(rows)} rows; ended {ended} of {tested}")


# ---------------------------------------------------------------------------------------------------------------- 10 the contract
def test_index_limit_holds_with_roulette_on_only():
    """samples * bounces * 8 one step over 2^30, on a window of one pixel: rendered with roulette off, refused with it on"""
    pt = make_pt(IW.open_room(), (1, 1), sky=IW.room_sky())
    try:
        big = pt.make_gconst(camera(IW.ROOM_CAMERA, (1, 1)), (1 << 21) + 1, 64, flags=0)
        pt.render(big)
        assert np.isfinite(pt.light()).all()
        pt.set_roulette(2, FLOOR)
        with pytest.raises(L.Rt3Error) as e:
            pt.render(big)
        assert e.value.code == L.E_INVALID and "2^30" in str(e.value)
        pt.render(pt.make_gconst(camera(IW.ROOM_CAMERA, (1, 1)), 1 << 21, 64, flags=0))  # at the limit: accepted
    finally:
        pt.close()


def state(c):
    p, on = c.get_roulette()
    return (p.start_bounce, p.min_survival, tuple(p.reserved), on)


def test_contract_of_the_calls():
    pt = make_pt(IW.open_room(), IW.WINDOW_ROOM, sky=IW.room_sky())
    try:
        c = pt.ctx
        cam = camera(IW.ROOM_CAMERA, IW.WINDOW_ROOM)
        assert state(c) == (2, 0.0625, (0, 0), False)
        c.set_roulette(L.RouletteParams(3, 0.25))
        assert state(c) == (3, 0.25, (0, 0), True)
        for what, bad in {"NaN": dict(min_survival=np.nan), "inf": dict(min_survival=np.inf), "below 2^-7": dict(min_survival=float(np.nextafter(F(2.0**-7), F(0)))),
                          "zero": dict(min_survival=0.0), "negative": dict(min_survival=-0.5), "above 1": dict(min_survival=float(np.nextafter(F(1), F(2)))),
                          "reserved 0": dict(reserved=(1, 0)), "reserved 1": dict(reserved=(0, 7))}.items():
            with pytest.raises(L.Rt3Error) as e:
                c.set_roulette(L.RouletteParams(**bad))
            assert e.value.code == L.E_INVALID and state(c) == (3, 0.25, (0, 0), True), what
        for edge in (2.0**-7, 1.0):  # the ends of the range are in it
            c.set_roulette(min_survival=edge)
            assert state(c) == (2, edge, (0, 0), True)
        c.set_roulette(None)  # off; the parameters last set stay readable
        assert state(c) == (2, 1.0, (0, 0), False)
        # the vertices' RNG indices may not reach the roulette draws': with roulette on only, and whatever start_bounce is
        big = pt.make_gconst(cam, (1 << 21) + 1, 64, flags=L.F_NEE_SKY)
        assert big.samples * big.bounces * 8 > 1 << 30
        g1 = pt.make_gconst(cam, 1, 1, flags=L.F_NEE_SKY)
        pt.render(g1)
        c.set_roulette(L.RouletteParams(1000, FLOOR))
        for adaptive in (None, True):
            with pytest.raises(L.Rt3Error) as e:
                pt.render(big, adaptive=adaptive)
            assert e.value.code == L.E_INVALID and "2^30" in str(e.value), adaptive
        # the counts are the last launch's: 0 / 0 after a frame with roulette off, after one with nothing to test, and after a refusal
        pt.set_roulette(0, FLOOR)
        frame(pt, cam, L.F_NEE_SKY | FF, 4, 4)
        tested, ended = pt.roulette_info()
        assert 0 < ended < tested
        pt.render(g1)
        assert pt.roulette_info() == (0, 0)
        frame(pt, cam, L.F_NEE_SKY | FF, 4, 4)
        assert pt.roulette_info() == (tested, ended)
        pt.set_roulette(None)
        frame(pt, cam, L.F_NEE_SKY | FF, 4, 4)
        assert pt.roulette_info() == (0, 0)
    finally:
        pt.close()
