"""Rough transmission on the GPU (rt3_scene_set_rough_transmission): the vertex rule against float64 inside derived
bounds, "nothing changes without it" bit for bit, the closed form of an index-matched rough slab, the whole integrator against the float64
fixture of tests/ref_frost.py, the blur of an edge behind a frosted pane, invariance under batch size, instance mode, tile partition and
window size, frosted panes under pane shadows, the contract of the three calls, and a ledger of the twelve k_shade_frost instances.

Bounds are derived: ref_frost.op38_reference for the rule; for frames one unit of 2^-24 per rounding of the longest chain."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import frost_worlds as FW
import glass_worlds as GW
import integrator_worlds as IW
import pane_worlds as PN
import ref_frost as RF
import ref_shading as R
from raytracer3_amd import _lib as L
from raytracer3_amd import assets
from raytracer3_amd.renderer import PathTracer
from support import bits, camera
from test_frost_cpu import fixture
from test_integrator_cpu import Z_MAX, check_against_fixture
from test_nee_emissive import owned_mask

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HERE = "tests/test_frost.py"
U = 2.0**-24
FULL = L.F_NEE_SKY | L.F_BLUENOISE | L.F_FACEFORWARD | L.F_SPECULAR
SKY = np.array(GW.SKY_L)


def frost_pt(mesh, window=GW.WINDOW, sky=GW.SKY_L, lens=GW.PINHOLE, *, on=True, panes=False, mode=0, options=(), rank=0, n_ranks=1, want_frosted=None):
    """a PathTracer over `mesh` with rough transmission `on` (and pane shadows `panes`) before the build, its lens set"""
    pt = PathTracer(window, rank=rank, n_ranks=n_ranks)
    pt.ctx.set_rough_transmission(on)
    pt.ctx.set_pane_shadows(panes)
    if sky is not None and not isinstance(sky, np.ndarray):
        sky = FW.constant_sky(sky)
    pt.set_scene(mesh, sky, assets.load_bluenoise(), options=[(L.OPT_INSTANCE_MODE, mode), *options])
    pt.set_lens(*lens)
    if want_frosted is not None:
        assert pt.ctx.rough_transmission_info() == want_frosted
    return pt


def frame(pt, flags, spp, bounces, window=GW.WINDOW, cam=GW.CAMERA, index=0, **kw):
    pt.render(pt.make_gconst(camera(cam, window), spp, bounces, frame=index, flags=flags), **kw)
    return pt.light()[..., :3].copy()


def one_frame(mesh, flags, spp, bounces, cam=GW.CAMERA, **kw):
    pt = frost_pt(mesh, **kw)
    try:
        return frame(pt, flags, spp, bounces, window=kw.get("window", GW.WINDOW), cam=cam)
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 1 the vertex rule
def test_frost_function_against_float64():
    """Self-test op 38 on ref_frost.op38_rows: direction, F and weight inside the per-row bounds that op38_reference derives (its docstring
    has the derivation), the event equal on every row that is not open; open rows stay at or under the 1 % cap.  Every output word also
    equals that of ref_frost.rule evaluated in numpy's float32, the same operations in the same order.  Rows with alpha = 0 are op 32's
    answers with weight 1, bit for bit."""
    rows = RF.op38_rows()
    ior, thin, d, n, alpha, u, u2, u3 = rows
    words = np.concatenate([bits(ior)[:, None], thin[:, None], bits(d), bits(n), bits(alpha)[:, None], bits(u)[:, None], bits(u2)[:, None], bits(u3)[:, None]], 1).astype(np.uint32)
    smooth = words[:256].copy()
    smooth[:, 8] = 0
    pt = frost_pt(GW.pane_world(), on=False)
    try:
        out = pt.ctx.selftest(L.SELFTEST_FROST, words, 6)
        out0 = pt.ctx.selftest(L.SELFTEST_FROST, smooth, 6)
        glass = pt.ctx.selftest(L.SELFTEST_GLASS, smooth[:, [0, 1, 2, 3, 4, 5, 6, 7, 9]], 5)
    finally:
        pt.close()
    assert np.array_equal(out0[:, :5], glass) and np.all(out0[:, 5] == bits(np.float32(1.0)))
    f = lambda c: np.ascontiguousarray(out[:, c]).view(np.float32).astype(np.float64)  # noqa: E731
    ev, direction, F, W = out[:, 0].astype(np.int64), f(slice(1, 4)), f(4), f(5)
    ref = RF.op38_reference(*rows)
    open_, ev_open = ref["open"], ref["ev_open"]
    print(f"op 38: {int(ev_open.sum())} of {len(u)} rows open ({ev_open.mean():.2%}; cap 1 %)")
    assert ev_open.mean() <= 0.01 and set(ev) <= {0, 1, 2}
    assert np.array_equal(ev[~ev_open], ref["event"][~ev_open])
    same = (ev == ref["event"]) & ~open_
    live = same & (ev != RF.INVALID)
    err_d = np.abs(direction - ref["dir"]).max(-1)
    err_F = np.abs(F - ref["F"])
    err_W = np.abs(W - ref["weight"])
    known = same & (F > 0) | (same & (ref["F"] == 0))
    model = RF.rule(np.float32, *rows)  # the device's operations in the device's order, in numpy's float32
    same_words = (np.array_equal(ev, model["event"]), int((bits(np.float32(direction)) != bits(model["dir"])).sum()),
                  int((bits(np.float32(F)) != bits(model["F"])).sum()), int((bits(np.float32(W)) != bits(model["weight"])).sum()))
    # the arithmetic contract (no contraction, IEEE division and square root): the device's words are the model's, which pins the rule to
    # the last bit wherever the derived bounds leave room
    assert same_words == (True, 0, 0, 0), same_words
    print(f"op 38 against the float32 model: events equal {same_words[0]}; words that differ: direction {same_words[1]}, F {same_words[2]}, weight {same_words[3]}")
    print(f"op 38: bounds in units of 2^-24, median / 99th percentile: direction {np.median(ref['d_dir'][same]) / U:.0f} / {np.percentile(ref['d_dir'][same], 99) / U:.0f}, "
          f"F {np.median(ref['dF'][same]) / U:.0f} / {np.percentile(ref['dF'][same], 99) / U:.0f}, weight {np.median(ref['dW'][live]) / U:.0f} / {np.percentile(ref['dW'][live], 99) / U:.0f}")
    print(f"op 38: worst error / bound: direction {np.max(err_d[same] / ref['d_dir'][same]):.4f} (worst error {err_d[same].max() / U:.0f} u), "
          f"F {np.max(err_F[known] / np.maximum(ref['dF'][known], U)):.4f} ({err_F[known].max() / U:.0f} u), "
          f"weight {np.max(err_W[live] / ref['dW'][live]):.4f} ({err_W[live].max() / U:.0f} u) over {int(same.sum())} rows")
    assert np.all(err_d[same] <= ref["d_dir"][same])
    assert np.all(err_F[known] <= ref["dF"][known] + U)
    assert np.all(err_W[live] <= ref["dW"][live])
    assert np.all(W[ev == RF.INVALID] == 0.0) and (ev == RF.INVALID).sum() > 100 and (ev == RF.REFLECT).sum() > 100
    # an index-matched solid surface: F = 0 exactly, the direction goes on, the weight is G1 of the incidence
    k = np.flatnonzero((ior == 1.0) & (thin == 0) & (ev == RF.TRANSMIT))
    ud = d[k].astype(np.float64) / np.linalg.norm(d[k].astype(np.float64), axis=1, keepdims=True)
    assert len(k) and np.all(F[k] == 0.0) and np.abs(direction[k] - ud).max() <= 64 * U


# ---------------------------------------------------------------------------------------------------------------- 2 nothing changes without it
def room_frame(mesh, window=IW.WINDOW_ROOM, flags=FULL | L.F_NEE_EMISSIVE, spp=4, bounces=6, setup=None, **kw):
    pt = frost_pt(mesh, window, sky=IW.room_sky(), lens=(0.05, 6.0, 1.0), **kw)
    try:
        if setup:
            setup(pt)
        return frame(pt, flags, spp, bounces, window=window, cam=IW.ROOM_CAMERA)
    finally:
        pt.close()


def test_mode_off_ignores_roughness_on_glass():
    """the glass room as glass_worlds builds it (roughness 0.4 on the pane, 0.3 on the block): with the mode off, or switched on and off
    again, nothing is classified and the frame is the parent's"""
    mesh = GW.glass_room(True, 0.5)
    never = room_frame(mesh, on=False, want_frosted=0)

    def on_and_off(pt):
        pt.set_rough_transmission(True)
        assert pt.ctx.rough_transmission_info() == 2
        pt.set_rough_transmission(False)
        assert pt.ctx.rough_transmission_info() == 0

    assert never.max() > 0 and np.array_equal(bits(never), bits(room_frame(mesh, on=False, setup=on_and_off)))


def test_mode_on_without_rough_glass_equals_mode_off():
    """every transmissive geometry at roughness 0: no frosted geometry, k_shade_glass as before"""
    mesh = FW.smooth(GW.glass_room(True, 0.5))
    off = room_frame(mesh, on=False, want_frosted=0)
    assert np.array_equal(bits(off), bits(room_frame(mesh, on=True, want_frosted=0)))


TEXTURED_LIGHTS = {"none": 0, "emitters": L.F_NEE_EMISSIVE, "emitters_point": L.F_NEE_EMISSIVE | L.F_NEE_PUNCTUAL}


@pytest.mark.parametrize("lights", sorted(TEXTURED_LIGHTS))
def test_a_smooth_vertex_inside_the_frost_kernels_keeps_its_bits(lights):
    """the block names a metallic-roughness texture whose roughness channel is 0 everywhere: the build classifies it as frosted, so
    k_shade_frost<EMIT, MAT = true, PUNCT, false> shades the frame, every glass vertex has alpha = 0, and the frame equals the one
    k_shade_glass<.., MAT = true, ..> shades with the mode off"""
    mesh = FW.textured_room()
    if lights == "emitters_point":
        mesh.lights = assets.lights_array([assets.make_light(assets.LIGHT_POINT, (6.0, 5.0, 4.0), position=(1.0, 2.5, 1.0))])
    flags = FULL | TEXTURED_LIGHTS[lights]
    off = room_frame(mesh, flags=flags, on=False, want_frosted=0)
    on = room_frame(mesh, flags=flags, on=True, want_frosted=1)
    assert off.max() > 0 and np.isfinite(off).all() and np.array_equal(bits(off), bits(on))


def test_classification_by_the_build():
    """rt3_rough_transmission_info over the room with a smooth pane and a block that is: at roughness factor 0 with a metallic-roughness
    texture (the texture alone: frosted); the same with the texture index at -1 while another geometry keeps the side table (not frosted);
    at factor 0.3 without any texture table (frosted); all of them with the mode off (none).  The roughness at a hit is factor x texel, so
    the block frosted by its texture alone has alpha 0 at every hit: its frame, shaded by k_shade_frost, is the mode-off frame bit for bit."""
    by_texture = FW.textured_room(factor=0.0, value=200)
    assert by_texture.geometries["roughness"][by_texture.names.index("block")] == 0.0
    off = room_frame(by_texture, on=False, want_frosted=0)
    on = room_frame(by_texture, on=True, want_frosted=1)
    assert off.max() > 0 and np.array_equal(bits(off), bits(on))
    for mesh, want in ((FW.textured_room(factor=0.0, value=200, texture=-1), 0), (FW.set_roughness(FW.smooth(GW.glass_room(True, 0.5)), block=0.3), 1),
                       (FW.frost_room(True, 0.5), 2)):
        for mode_on in (False, True):
            pt = frost_pt(mesh, IW.WINDOW_ROOM, sky=IW.room_sky(), on=mode_on)
            try:
                assert pt.ctx.rough_transmission_info() == (want if mode_on else 0)
            finally:
                pt.close()


# ---------------------------------------------------------------------------------------------------------------- 3 the closed form
def g1(cos, alpha):
    return R.smith_g1(alpha, cos)


def g1_squared_band(cos, alpha):
    """relative bound of the fp32 G1(cos, alpha^2)^2 of the two crossings of a slab: cos carries the frame's 15 u (ref_frost.op38_reference:
    Ewo) and a 16-bit octahedral normal's 2^-15 sin theta; G1's slope in cos is at most 2 / alpha; 8 roundings in G1; twice"""
    d_cos = 15 * U + 2.0**-15 * np.sqrt(1.0 - cos * cos) + 2.0**-31
    return 2.0 * ((2.0 / alpha) * d_cos / g1(cos, alpha) + 8 * U)


@pytest.mark.parametrize("tilt", (0.0, 35.0))
def test_index_matched_rough_slab_is_the_sky_times_g1_squared(tilt):
    """ior = 1, alpha 0.5, a constant sky, B = 3: F = 0, the direction never changes, each crossing weighs G1(cos theta, alpha^2), and the
    third vertex is the sky's: every sample of every pixel is SKY G1^2, theta between the pixel's ray and the slab's normal.  The band:
    g1_squared_band, then test_glass's sky_bound for the sky, the mean and the throughput, and the two products with G1.  It is narrow enough
    to tell G1^2 from G1 and from 1."""
    S, B, a = 4, 3, FW.SLAB_ALPHA
    mesh, normal = FW.matched_slab(tilt)
    got = one_frame(mesh, L.F_NEE_SKY, S, B, want_frosted=2).astype(np.float64)
    cos = -np.sum(GW.pixel_dirs() * normal, -1)
    G = g1(cos, a)
    want = SKY * (G * G)[..., None]
    rel = g1_squared_band(cos, a) + (S + 8 + 4) * U
    err = np.abs(got / want - 1.0).max(-1)
    print(f"rough slab tilted by {tilt}: worst error {np.max(err / rel):.3f} bounds; G1 from {G.min():.4f} to {G.max():.4f}")
    assert np.all(err <= rel)
    # (G1 -> 1 at normal incidence, where nothing can tell them apart: the pixels more than 5 degrees off the normal)
    off = cos < np.cos(np.radians(5.0))
    assert off.mean() > 0.3 and np.all(np.abs(1.0 / G - 1.0)[off] > 4.0 * rel[off]), "the band tells G1^2 from G1 and from 1"


# ---------------------------------------------------------------------------------------------------------------- 4 the fixture
def room_frames(name, mode=0):
    flags, bounces, specular, tau, _, _, frames, more = FW.ROOM_CASES[name]
    pt = frost_pt(FW.frost_room(specular, tau), IW.WINDOW_ROOM, sky=IW.room_sky(), lens=FW.ROOM_LENS, mode=mode, want_frosted=2)
    try:
        cam = camera(IW.ROOM_CAMERA, IW.WINDOW_ROOM)
        out = []
        for k in range(frames):
            pt.render(pt.make_gconst(cam, IW.FRAME_SPP, bounces, frame=k, flags=flags | more))
            out.append(pt.light()[..., :3].copy())
        return np.stack(out)
    finally:
        pt.close()


@pytest.mark.parametrize("name,mode", [("frost_b4", 0), ("frost_spec_b6", 0), ("frost_spec_b6", 1)])
def test_gpu_against_fixture(name, mode):
    W, H = IW.WINDOW_ROOM
    check_against_fixture(room_frames(name, mode), np.ones((H, W), bool), fixture(), name)


# ---------------------------------------------------------------------------------------------------------------- 5 the blur
def test_a_thin_frosted_pane_blurs_an_edge():
    """the emissive half-plane behind an index-matched thin pane: smooth (alpha 0) the pixel row across the edge is a step; at alpha 0.2
    it differs from that step by far more than the fixture's standard error, and matches ref_frost's row by the fixture's z-test"""
    S, B, K = 4096, 3, 2
    fx = fixture()
    row = FW.EDGE_ROW
    step = one_frame(FW.edge_world(0.0), 0, 4, B, sky=None, window=FW.EDGE_WINDOW, want_frosted=0)[row].astype(np.float64)
    assert len(np.unique(step[:, 0])) == 2 and step[0, 0] == 0.0 and step[-1, 0] > 0.0, "smooth: a step from black to the emitter"
    pt = frost_pt(FW.edge_world(FW.EDGE_ALPHA), FW.EDGE_WINDOW, sky=None, want_frosted=1)
    try:
        frames = np.stack([frame(pt, 0, S, B, window=FW.EDGE_WINDOW, index=k)[row] for k in range(K)]).astype(np.float64)
    finally:
        pt.close()
    got = frames.mean(0)
    ref, se = fx["edge_mean"], fx["edge_se"]
    # the same estimator on both sides (no light sampling in this world): K S samples have sqrt(spp / (K S)) of the fixture's noise
    assert K * S >= 4 * int(fx["edge_spp"].item()), "rendered to at most half the fixture's noise"
    lit = se > 0
    z = (got - ref)[lit] / se[lit]
    away = np.abs(step - got) / np.where(lit, se, np.inf)
    print(f"edge behind a frosted pane: max |z| {np.abs(z).max():.2f} over {int(lit.sum())} pixel-channels; {int((away > 10.0).any(-1).sum())} pixels of the row "
          f"are more than 10 standard errors from the smooth step, the furthest {away.max():.0f}")
    assert np.abs(z).max() < Z_MAX
    assert (away > 10.0).any(-1).sum() >= 8, "the blur is far outside the noise"


# ---------------------------------------------------------------------------------------------------------------- 6 plumbing
def test_same_bits_for_every_batch_size_and_instance_mode():
    mesh = FW.frost_room(True, 0.5)
    mesh.lights = assets.lights_array([assets.make_light(assets.LIGHT_POINT, (6.0, 5.0, 4.0), position=(1.0, 2.5, 1.0))])
    flags = FULL | L.F_NEE_EMISSIVE | L.F_NEE_PUNCTUAL  # k_shade_frost<true, false, true, false>
    whole = room_frame(mesh, flags=flags, want_frosted=2)
    assert whole.max() > 0.0
    assert np.array_equal(bits(whole), bits(room_frame(mesh, flags=flags, setup=lambda pt: pt.ctx.set_option(L.OPT_BATCH_SPP, 1))))
    assert np.array_equal(bits(whole), bits(room_frame(mesh, flags=flags, mode=1)))


def test_two_ranks_stitch_to_one():
    W, H = window = (128, 48)
    mesh = FW.frost_room(True, 0.5)
    whole = room_frame(mesh, window)
    for r in range(2):
        part = room_frame(mesh, window, rank=r, n_ranks=2)
        m = owned_mask(W, H, r, 2)
        assert m.any() and not m.all()
        assert np.array_equal(bits(part[m]), bits(whole[m]))


@pytest.mark.parametrize("window", ((60, 44), (8, 8)))
def test_windows_that_do_not_fill_their_last_block(window):
    """60 x 44 at 1 spp: five blocks of 512 paths and a part of one; 8 x 8: less than one block.  The index-matched rough slab: every
    pixel is SKY G1^2 inside the closed form's band (g1_squared_band and the sky's, the mean's and the throughput's roundings)"""
    S = 1
    mesh, normal = FW.matched_slab(35.0)
    got = one_frame(mesh, L.F_NEE_SKY, S, 3, window=window, want_frosted=2).astype(np.float64)
    cos = -np.sum(GW.pixel_dirs(window) * normal, -1)
    G = g1(cos, FW.SLAB_ALPHA)
    rel = g1_squared_band(cos, FW.SLAB_ALPHA) + (S + 8 + 4) * U
    assert got.shape[:2] == window[::-1] and np.all(np.abs(got / (SKY * (G * G)[..., None]) - 1.0).max(-1) <= rel)


# ---------------------------------------------------------------------------------------------------------------- 7 roulette, absorption
def test_roulette_decides_on_the_frosted_and_attenuated_throughput():
    """test_volume's index-matched absorbing slab, tilted by 35 degrees, at roughness 0.5, with roulette from vertex 1, floor 1/16, S = 16,
    B = 4.  Every sample of a pixel is one path: through the front face (T = G1), the internal segment (k_absorb: T = G1 exp(-sigma x) on
    arrival at the back face), through the back face (T = G1^2 exp(-sigma x)), whose extension ray k_roulette tests with q = max T,
    q_g = ceil(q 2^23) 2^-23 and u = ref_roulette.roulette_u(pixel, frame, sample, B, 1); the survivor escapes into the sky with T / q_g.
    So a pixel is k / S times SKY T / q, k the number of its samples with u < q, inside test_volume's band for the absorption plus
    g1_squared_band, the grid step of q_g and the division's and one more mean's roundings.  T is known to the band only: a pixel one of
    whose draws lies within the band of q is left out, under 2 % of them."""
    import ref_roulette as RR
    import volume_worlds as VW
    from test_volume import matched_band

    S, B, frame_no, a = 16, 4, 3, FW.SLAB_ALPHA
    mesh, n, _ = VW.slab_world(ior=1.0, tilt_deg=35.0)
    FW.set_roughness(mesh, slab_front=a, slab_back=a)
    absorbed, _, band = matched_band(mesh, n, S)
    cos = -np.sum(GW.pixel_dirs() * n, -1)
    G = g1(cos, a)
    want = absorbed * (G * G)[..., None]
    band = band + g1_squared_band(cos, a)[..., None] + 4.0 * U
    q = (want / SKY).max(-1)
    assert q.min() > 1.0 / 16.0 and q.max() < 1.0
    H, W = q.shape
    py, px = np.mgrid[0:H, 0:W]
    u = np.stack([RR.roulette_u(px.reshape(-1), py.reshape(-1), frame_no, s, B, 1).reshape(H, W) for s in range(S)]).astype(np.float64)
    margin = q * band.max(-1) + 2.0**-23
    open_ = (np.abs(u - q) <= margin).any(0)
    k = (u < q).sum(0)
    print(f"roulette on the frosted slab: {open_.mean():.2%} of the pixels open; survivors per pixel {k.min()} .. {k.max()} of {S}")
    assert open_.mean() < 0.02 and k.min() < S
    pt = frost_pt(mesh, want_frosted=2)
    try:
        assert pt.ctx.attenuation_info() == 2
        pt.set_roulette(1, 1.0 / 16.0)
        got = frame(pt, L.F_NEE_SKY, S, B, index=frame_no).astype(np.float64)
        tested, ended = pt.roulette_info()
    finally:
        pt.close()
    expect = (k / S)[..., None] * want / q[..., None]
    ok = ~open_ & (k > 0)
    assert np.all(np.abs(got[ok] / expect[ok] - 1.0) <= band[ok] + (2.0**-23 / q[ok])[..., None] + 4.0 * U)
    assert not got[~open_ & (k == 0)].any()
    assert ended >= int((S - k)[~open_].sum()) and tested > ended


# ---------------------------------------------------------------------------------------------------------------- 8 adaptive
def test_adaptive_coverage_pixels_hold_the_fixed_frames_bits():
    """ "adaptive" in coverage mode shares trace_batch: a pixel that stopped at n samples holds the bits of the fixed frost frame at
    samples = n"""
    mesh = FW.frost_room(True, 1.0)
    window, cap = (16, 16), 32
    pt = frost_pt(mesh, window, sky=IW.room_sky(), lens=FW.ROOM_LENS, want_frosted=2)
    try:
        pt.set_adaptive_coverage(True)
        g = pt.make_gconst(camera(IW.ROOM_CAMERA, window), cap, 4, frame=3, flags=FULL)
        pt.render(g, adaptive=True)
        light = pt.light()[..., :3].copy()
        counts = pt.sample_counts()
        assert counts.min() >= 1 and counts.max() <= cap
        checked = 0
        for n in np.unique(counts)[:3]:
            fixed = frame(pt, FULL, int(n), 4, window=window, cam=IW.ROOM_CAMERA, index=3)
            m = counts == n
            assert np.array_equal(bits(light[m]), bits(fixed[m])), int(n)
            checked += int(m.sum())
        assert checked > 0
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 9 pane shadows
PANE_CASES = [(textured, lights) for textured in (False, True) for lights in ("sky", "emitter", "directional")]


@pytest.mark.parametrize("textured,lights", PANE_CASES, ids=[f"{'mat' if t else 'plain'}-{l}" for t, l in PANE_CASES])
def test_a_frosted_pane_is_no_pane(textured, lights):
    """pane shadows on, a frosted and a clear thin-walled pane side by side above the floor: rt3_pane_shadow_info counts the clear one alone
    and k_shade_frost<EMIT, MAT, PUNCT, PANE = true> shades the frame.  Under the directional light (B = 2, no sky: direct light only) the
    floor in the frosted pane's shadow is exactly black, the floor under the clear pane carries the free frame times the pane's
    A = (1 - F') tint inside test_pane_shadows' bound, and beside both the frame is the free frame's, bit for bit.  With the sky or an
    emitter the frame is finite, lit, and the same bits at batch size 1."""
    from test_pane_shadows import crossing_bound

    mesh = FW.two_panes(textured, emitter=lights == "emitter")
    flags = {"sky": L.F_NEE_SKY, "emitter": L.F_NEE_EMISSIVE, "directional": L.F_NEE_PUNCTUAL}[lights]
    sky = GW.SKY_L if lights == "sky" else None
    pt = frost_pt(mesh, PN.WINDOW, sky=sky, lens=PN.PINHOLE, panes=True, want_frosted=1)
    try:
        assert pt.ctx.pane_shadow_info() == 1
        got = frame(pt, flags, 1 if lights == "directional" else 4, 2 if lights == "directional" else 3, window=PN.WINDOW, cam=PN.CAMERA)
        if lights != "directional":
            pt.ctx.set_option(L.OPT_BATCH_SPP, 1)
            again = frame(pt, flags, 4, 3, window=PN.WINDOW, cam=PN.CAMERA)
            assert np.isfinite(got).all() and got.max() > 0 and np.array_equal(bits(got), bits(again))
            return
    finally:
        pt.close()
    free = one_frame(FW.two_panes(textured, glass=False), flags, 1, 2, cam=PN.CAMERA, window=PN.WINDOW, sky=None, lens=PN.PINHOLE, panes=True, want_frosted=0)
    x = PN.floor_points(PN.WINDOW)
    w = PN.to_light(PN.LIGHTS["directional"], x)
    in_f, edge_f, _ = PN.crossing(FW.PANE_FROSTED, x, w)
    in_c, edge_c, _ = PN.crossing(FW.PANE_CLEAR, x, w)
    use = (edge_f >= PN.EDGE_MARGIN) & (edge_c >= PN.EDGE_MARGIN)
    got, free = got.reshape(-1, 3), free.reshape(-1, 3)
    shadow, lit, beside = use & in_f, use & in_c & ~in_f, use & ~in_f & ~in_c
    assert shadow.sum() > 100 and lit.sum() > 100 and beside.sum() > 100
    assert not got[shadow].any(), "a frosted pane occludes shadow rays"
    A = PN.pass_fraction(w[:, 1], PN.IOR)[:, None] * np.asarray(PN.TINT)
    want = free.astype(np.float64) * A
    bound = want * (1.01 * crossing_bound(w[:, 1], PN.IOR))[:, None]
    assert free[lit].min() > 0 and np.all(np.abs(got.astype(np.float64) - want)[lit] <= bound[lit])
    assert np.array_equal(bits(got[beside]), bits(free[beside]))


# ---------------------------------------------------------------------------------------------------------------- 10 the contract
def test_contract_of_the_three_calls():
    mesh, _ = FW.matched_slab(0.0)
    pt = PathTracer(GW.WINDOW)
    try:
        ctx = pt.ctx
        assert ctx.get_rough_transmission() is False
        with pytest.raises(L.Rt3Error) as e:
            ctx.rough_transmission_info()
        assert e.value.code == L.E_STATE
        pt.set_scene(mesh, FW.constant_sky(), assets.load_bluenoise())
        pt.set_lens(*GW.PINHOLE)
        assert ctx.rough_transmission_info() == 0
        off = frame(pt, L.F_NEE_SKY, 2, 3)
        for bad in (2, -1):
            with pytest.raises(L.Rt3Error) as e:
                ctx.set_rough_transmission(bad)
            assert e.value.code == L.E_INVALID and ctx.get_rough_transmission() is False
        assert np.array_equal(bits(frame(pt, L.F_NEE_SKY, 2, 3)), bits(off))  # a refusal changes nothing
        ctx.set_rough_transmission(False)  # no change: the structure stays usable
        assert np.array_equal(bits(frame(pt, L.F_NEE_SKY, 2, 3)), bits(off))
        ctx.set_rough_transmission(True)  # a change takes effect at the next build; until then the structure is unusable
        with pytest.raises(L.Rt3Error) as e:
            frame(pt, L.F_NEE_SKY, 2, 3)
        assert e.value.code == L.E_STATE
        ctx.build_accel()
        assert ctx.rough_transmission_info() == 2
        on = frame(pt, L.F_NEE_SKY, 2, 3)
        assert not np.array_equal(bits(on), bits(off)) and on.max() < off.max()
        # a refit keeps the classification, and so does an import of the structure's own tree
        ctx.update_vertices(mesh.vertices, 0)
        ctx.refit_accel()
        assert ctx.rough_transmission_info() == 2 and np.array_equal(bits(frame(pt, L.F_NEE_SKY, 2, 3)), bits(on))
        nodes, tris = ctx.accel_download()
        ctx.accel_import(nodes, tris)
        assert ctx.rough_transmission_info() == 2 and np.array_equal(bits(frame(pt, L.F_NEE_SKY, 2, 3)), bits(on))
        # the mode survives rt3_scene_set_geometry
        ctx.upload_mesh(mesh)
        assert ctx.get_rough_transmission() is True
        ctx.build_accel()
        assert ctx.rough_transmission_info() == 2
        # PathTracer.set_rough_transmission rebuilds when the mode changes
        pt.set_rough_transmission(False)
        assert ctx.rough_transmission_info() == 0 and np.array_equal(bits(frame(pt, L.F_NEE_SKY, 2, 3)), bits(off))
        pt.set_rough_transmission(True)
        assert ctx.rough_transmission_info() == 2 and np.array_equal(bits(frame(pt, L.F_NEE_SKY, 2, 3)), bits(on))
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 11 the ledger
_TEXTURED = f"{HERE}::test_a_smooth_vertex_inside_the_frost_kernels_keeps_its_bits"
_PANES = f"{HERE}::test_a_frosted_pane_is_no_pane"
# k_shade_frost<EMIT, MAT, PUNCT, PANE> -> (when launch_shade picks it, a test above that launches it)
LEDGER = {
    "k_shade_frost<false, false, false, false>": ("no light table", f"{HERE}::test_index_matched_rough_slab_is_the_sky_times_g1_squared"),
    "k_shade_frost<true, false, false, false>": ("emitters", f"{HERE}::test_gpu_against_fixture"),
    "k_shade_frost<true, false, true, false>": ("emitters and punctual lights", f"{HERE}::test_same_bits_for_every_batch_size_and_instance_mode"),
    "k_shade_frost<false, true, false, false>": ("material textures, no light table", _TEXTURED),
    "k_shade_frost<true, true, false, false>": ("material textures, emitters", _TEXTURED),
    "k_shade_frost<true, true, true, false>": ("material textures, emitters and punctual lights", _TEXTURED),
    "k_shade_frost<false, false, false, true>": ("panes, no light table", _PANES),
    "k_shade_frost<true, false, false, true>": ("panes, emitters", _PANES),
    "k_shade_frost<true, false, true, true>": ("panes, punctual lights", _PANES),
    "k_shade_frost<false, true, false, true>": ("panes, material textures, no light table", _PANES),
    "k_shade_frost<true, true, false, true>": ("panes, material textures, emitters", _PANES),
    "k_shade_frost<true, true, true, true>": ("panes, material textures, punctual lights", _PANES),
}


def library_instances():
    """the template instances of k_shade_frost in librt3.so's symbol table (their host stubs; names only)"""
    lib = ROOT / "raytracer3_amd" / "librt3.so"
    out = None
    for nm in ("nm", "/opt/rocm/llvm/bin/llvm-nm"):
        try:
            out = subprocess.run([nm, "-C", str(lib)], capture_output=True, text=True, check=True).stdout
            break
        except (OSError, subprocess.CalledProcessError):
            continue
    assert out is not None, "neither nm nor llvm-nm could read the library"
    return set(re.findall(r"__device_stub__(k_shade_frost<[^>]*>)\(", out))


def test_frost_instance_ledger():
    """fails when a k_shade_frost instance is added without an entry here, or an entry outlives its instance, or a credited test is gone"""
    have = library_instances()
    assert len(have) == 12, sorted(have)
    assert have == set(LEDGER), (sorted(have - set(LEDGER)), sorted(set(LEDGER) - have))
    text = (ROOT / HERE).read_text()
    for name, (conditions, credit) in LEDGER.items():
        path, _, test = credit.partition("::")
        assert conditions and path == HERE and re.search(rf"^def {re.escape(test)}\(", text, re.M), (name, credit)
