"""Pane shadows on the GPU (rt3_scene_set_pane_shadows): closed forms for punctual lights through panes, the same
expectation as without the mode against the float64 fixture of the glass tests, mode-off and no-pane equalities, invariance under batch
size, counting, instance mode, exit table and tile partition, windows that do not fill a block, the contract of the three calls, and a
ledger of the twenty new kernel instances.

The closed-form frames have B = 2: vertex 0 (the floor) takes the punctual light sample, vertex 1 can add nothing (no sky, no emission,
and RT3_F_NEE_PUNCTUAL samples lights at vertices 0 .. B - 2 only, so a B = 1 frame has no punctual light at all).  With one light its
selection probability is 1 and the per-sample pinhole sends every sample through the pixel centre: every sample of a pixel is one number.

The bound on A = transmission (1 - F'(cos_i)) tint, derived, one unit u = 2^-24 per fp32 rounding of the longest chain:
  * cos_i = |n.d| / |d|: the interpolated, twice normalised shading normal (10 roundings), the two dot products (3 each), the root and the
    quotient: under 18 u relative; cos_t = sqrt((cos_i^2 + ior^2 - 1) / ior^2): 5 more, halved by the root: under 16 u relative;
  * the numerators of r_s and r_p are differences of two terms whose magnitudes sum to at most 1 + ior = 2.5, each within 19 u relative:
    48 u absolute; the denominators are at least cos_i + ior cos_t >= ior sqrt(1 - 1 / ior^2) = 1.118 and within 20 u relative, so each
    of r_s, r_p (at most 1 in magnitude) is within 48 u / 1.118 + 21 u < 64 u; their squares within 129 u, F within 130 u;
  * F' = 2 F / (1 + F) has slope 2 / (1 + F)^2 <= 2: within 264 u with its own three roundings; 1 - F' one more: 265 u absolute;
  * the products with the transmission and the tint, and of the ray's contribution with A: 3 roundings.
  * the shading normal itself: the shading records hold vertex normals through the octahedral map at 16 bits per coordinate, a step of
    2^-15 in [-1, 1], so the decoded normal is within an angle of 2^-15 of the mesh's (tests/pane_worlds.py has (0, 1, 0)): cos_i moves by at
    most QUANT sin(theta_i), and 1 - F' by what float64 says it does over that interval (normal_quantisation below).
So a crossing multiplies the contribution by A (1 +- (265 u / (1 - F') + 3 u + that)); the errors of several crossings add (to first order;
the assert allows 1 % on top for the second).  With one sample the radiance slot and the frame's mean add nothing: 0 + x and x / 1 are exact."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import glass_worlds as GW
import integrator_worlds as IW
import lens_worlds as LW
import pane_worlds as PN
from raytracer3_amd import _lib as L
from raytracer3_amd import assets
from raytracer3_amd.renderer import PathTracer
from support import bits, camera, gamma
from test_glass_cpu import fixture as glass_fixture
from test_integrator_cpu import check_against_fixture
from test_nee_emissive import owned_mask

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HERE = "tests/test_pane_shadows.py"
U = 2.0**-24
P = L.F_NEE_PUNCTUAL
FULL = L.F_NEE_SKY | L.F_BLUENOISE | L.F_FACEFORWARD | L.F_SPECULAR


def pane_pt(mesh, on=True, window=PN.WINDOW, sky=None, lens=PN.PINHOLE, mode=0, options=(), rank=0, n_ranks=1):
    """a PathTracer over `mesh` with pane shadows `on` before the build, its lens set"""
    pt = PathTracer(window, rank=rank, n_ranks=n_ranks)
    pt.ctx.set_pane_shadows(on)
    pt.set_scene(mesh, sky, assets.load_bluenoise(), options=[(L.OPT_INSTANCE_MODE, mode), *options])
    pt.set_lens(*lens)
    return pt


def frame(pt, flags, spp, bounces, window=PN.WINDOW, cam=PN.CAMERA, index=0):
    pt.render(pt.make_gconst(camera(cam, window), spp, bounces, frame=index, flags=flags))
    return pt.light()[..., :3].copy()


def one_frame(mesh, flags, spp, bounces, *, on=True, cam=PN.CAMERA, want_panes=None, **kw):
    pt = pane_pt(mesh, on, **kw)
    try:
        if want_panes is not None:
            assert pt.ctx.pane_shadow_info() == want_panes
        return frame(pt, flags, spp, bounces, window=kw.get("window", PN.WINDOW), cam=cam)
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 4-6 closed forms
_FREE = {}


def free_frame(light, window=PN.WINDOW):
    """the frame of the floor under the light alone (no glass): computed once per light and window, never written to"""
    key = (light, window)
    if key not in _FREE:
        _FREE[key] = one_frame(PN.world("none", light), P, 1, 2, window=window, want_panes=0)
        _FREE[key].setflags(write=False)
    return _FREE[key]


QUANT = 2.0**-15  # the angle by which a 16-bit octahedral normal may differ from the one encoded


def normal_quantisation(cos_i, ior):
    """the largest relative change of 1 - F' when the normal turns by QUANT: cos_i moves by at most QUANT sin(theta_i) (+ QUANT^2 / 2)"""
    cos_i = np.asarray(cos_i, np.float64)
    step = QUANT * np.sqrt(np.maximum(0.0, 1.0 - cos_i * cos_i)) + 0.5 * QUANT * QUANT
    mid = PN.pass_fraction(cos_i, ior)
    lo, hi = PN.pass_fraction(np.maximum(cos_i - step, 0.0), ior), PN.pass_fraction(np.minimum(cos_i + step, 1.0), ior)
    return np.maximum(np.abs(lo - mid), np.abs(hi - mid)) / mid


def crossing_bound(cos_i, ior):
    """relative error of one crossing's A (module docstring)"""
    return 265.0 * U / PN.pass_fraction(cos_i, ior) + 3.0 * U + normal_quantisation(cos_i, ior)


def relative_bound(case, light, window=PN.WINDOW):
    """per pixel: the sum of crossing_bound over the panes crossed, 1 % added for the second order"""
    x = PN.floor_points(window)
    w = PN.to_light(PN.LIGHTS[light], x)
    total = np.zeros(len(x))
    for rect, mat in PN.case_quads(case):
        inside, _, _ = PN.crossing(rect, x, w)
        total += np.where(inside, crossing_bound(w[:, 1], mat.ior), 0.0)
    return 1.01 * total


def check_closed_form(case, light, want_panes, window=PN.WINDOW, mode=0):
    W, H = window
    factor, use, crossed = PN.closed_form(case, light, window)
    free = free_frame(light, window).reshape(-1, 3).astype(np.float64)
    got = one_frame(PN.world(case, light), P, 1, 2, window=window, want_panes=want_panes, mode=mode).reshape(-1, 3)
    assert use.mean() >= 0.9, "at most 10 % of the floor pixels touch a projected outline"
    want = free * factor
    bound = want * relative_bound(case, light, window)[:, None]
    err = np.abs(got.astype(np.float64) - want)
    attenuated = use & (crossed > 0)
    untouched = use & (factor == 1.0).all(-1)
    black = use & (factor == 0.0).all(-1)
    worst = float((err[attenuated] / bound[attenuated]).max()) if attenuated.any() else 0.0
    print(f"{case} / {light} {W}x{H}: {int(attenuated.sum())} pixels behind glass (worst error {worst:.3f} bounds), {int(untouched.sum())} beside it, "
          f"{int(black.sum())} black, {int((~use).sum())} left out")
    assert np.all(err[attenuated] <= bound[attenuated])
    assert np.array_equal(bits(got[untouched]), bits(free_frame(light, window).reshape(-1, 3)[untouched])), "beside the glass the frame is the frame without it"
    assert not got[black].any()
    return got, free, factor, use, crossed


def test_directional_light_through_a_pane():
    """Floor pixels inside the pane's projection are rho / pi E cos(theta) (1 - F'(theta)) c, outside rho / pi E cos(theta); with the mode
    off the pixels inside are exactly 0, which is the frame before pane shadows existed."""
    light = PN.LIGHTS["directional"]
    got, free, factor, use, crossed = check_closed_form("pane", "directional", 1)
    inside = use & (crossed == 1)
    assert inside.sum() > 300 and (use & (crossed == 0)).sum() > 300
    # the absolute level: rho / pi E cos(theta), the 34 roundings test_punctual_lights.closed_form_bound counts for a one-sample frame, and
    # the floor's quantised normal: cos(theta +- QUANT) / cos(theta) - 1 <= QUANT tan(theta) + QUANT^2
    d = np.asarray(light["direction"], np.float32).astype(np.float64)
    cos_theta = -d[1] / np.linalg.norm(d)
    level = np.asarray(PN.ALBEDO, np.float32).astype(np.float64) / np.pi * np.asarray(light["intensity"], np.float64) * cos_theta
    level_bound = gamma(34) + QUANT * np.sqrt(1.0 - cos_theta**2) / cos_theta + QUANT**2
    assert np.abs(free[use] / level - 1.0).max() <= level_bound
    A = PN.pass_fraction(cos_theta, PN.IOR) * np.asarray(PN.TINT)
    assert np.abs(got.astype(np.float64)[inside] / (level * A) - 1.0).max() <= level_bound + 1.01 * crossing_bound(cos_theta, PN.IOR)
    off = one_frame(PN.world("pane", "directional"), P, 1, 2, on=False, want_panes=0).reshape(-1, 3)
    assert not off[inside].any(), "with the mode off glass is a wall to shadow rays"
    outside = use & (crossed == 0)
    assert np.array_equal(bits(off[outside]), bits(got[outside]))


def test_point_light_above_a_pane():
    """cos_i varies per pixel (9 to 37 degrees).  The bound separates F' from F: what 1 - F instead of 1 - F' would give lies more than
    two bounds away at every pixel behind the pane."""
    got, free, factor, use, crossed = check_closed_form("pane", "point", 1)
    inside = use & (crossed == 1)
    assert inside.sum() > 300 and (use & (crossed == 0)).sum() > 300
    wrong = PN.closed_form("pane", "point", thin_slab=False)[0]
    rel = relative_bound("pane", "point")
    assert np.all(np.abs(wrong[inside] - factor[inside]) > 2.0 * (factor[inside] * rel[inside, None])), "the bound can tell F' from F"
    cos_i = PN.to_light(PN.LIGHTS["point"], PN.floor_points())[inside, 1]
    assert cos_i.min() < 0.82 and cos_i.max() > 0.98


@pytest.mark.parametrize("mode", (0, 1))
def test_two_stacked_panes_multiply(mode):
    """different tints, the upper one at transmission 0.5: pixels behind both get the product of the two A, behind one that one's.  In
    instance mode 1 the walk may meet the panes in the other order: one more rounding per extra crossing, which the 3 u per crossing hold."""
    got, free, factor, use, crossed = check_closed_form("stacked", "directional", 2, mode=mode)
    assert (use & (crossed == 2)).sum() > 200 and (use & (crossed == 1)).sum() > 50


def test_a_pane_that_is_also_a_cutout():
    """the alpha test comes first: the holes of the checker pass the full light, the rest A"""
    got, free, factor, use, crossed = check_closed_form("cutout", "directional", 1)
    behind = PN.crossing(PN.PANE, PN.floor_points(), PN.to_light(PN.LIGHTS["directional"], PN.floor_points()))[0]
    holes = use & behind & (crossed == 0)
    assert holes.sum() > 100 and (use & (crossed == 1)).sum() > 100
    assert np.array_equal(bits(got[holes]), bits(free_frame("directional").reshape(-1, 3)[holes]))


@pytest.mark.parametrize("case", ("solid", "normal_mapped"))
def test_glass_that_is_no_pane_still_occludes(case):
    """solid glass refracts, and a normal map would change the shading normal the walk would have to reproduce: neither is a pane, the floor
    below stays black and rt3_pane_shadow_info counts nothing"""
    got, free, factor, use, crossed = check_closed_form(case, "directional", 0)
    assert (use & (factor == 0.0).all(-1)).sum() > 300


def test_an_index_matched_untinted_pane_is_not_there():
    """ior 1, transmission 1, tint 1: F' = 0 and A = 1 exactly, so the frame is the frame without the pane, bit for bit"""
    got = one_frame(PN.world("index_matched", "point"), P, 1, 2, want_panes=1)
    assert got.any() and np.array_equal(bits(got), bits(free_frame("point")))


# ---------------------------------------------------------------------------------------------------------------- 8 the existing fixture
def room_frames(name, mode=0, on=True, roulette=None):
    flags, bounces, specular, tau, _, _, frames = GW.ROOM_CASES[name]
    pt = pane_pt(GW.glass_room(specular, tau), on, IW.WINDOW_ROOM, sky=IW.room_sky(), lens=GW.ROOM_LENS, mode=mode)
    try:
        assert pt.ctx.pane_shadow_info() == (1 if on else 0)
        if roulette is not None:
            pt.set_roulette(*roulette)
        cam = camera(IW.ROOM_CAMERA, IW.WINDOW_ROOM)
        out = []
        for k in range(frames):
            pt.render(pt.make_gconst(cam, IW.FRAME_SPP, bounces, frame=k, flags=flags))
            out.append(pt.light()[..., :3].copy())
        return np.stack(out)
    finally:
        pt.close()


@pytest.mark.parametrize("name,mode", (("glass_spec_b6", 0), ("glass_half_b4", 0), ("glass_half_b4", 1)))
def test_same_expectation_as_without_the_mode(name, mode):
    """glass_worlds.glass_room with the mode on against the fixture rendered by ref_glass, which knows nothing of pane shadows: sky light
    sampled through the room's pane plus the reweighted paths through it have the expectation of the paths alone"""
    W, H = IW.WINDOW_ROOM
    check_against_fixture(room_frames(name, mode), np.ones((H, W), bool), glass_fixture(), name)


def test_roulette_from_the_first_bounce_keeps_the_expectation():
    W, H = IW.WINDOW_ROOM
    check_against_fixture(room_frames("glass_half_b4", roulette=(0, 0.25)), np.ones((H, W), bool), glass_fixture(), "glass_half_b4")


# ---------------------------------------------------------------------------------------------------------------- 10 equalities
def observed(pt, flags=FULL | L.F_NEE_EMISSIVE, window=IW.WINDOW_ROOM):
    """what a frame leaves behind: `Light` as words, the structure's bytes, the ray counts"""
    pt.ctx.stats_reset()
    light = bits(frame(pt, flags, 4, 6, window=window, cam=IW.ROOM_CAMERA)).copy()
    s = pt.ctx.stats()
    nodes, tris = pt.ctx.accel_download()
    return light, nodes.copy(), tris.copy(), (s.extension_rays, s.shadow_rays)


def test_mode_on_without_panes_equals_mode_off():
    """solid glass only (the room's pane made solid): no pane, so on equals off -- frame, structure and ray counts; and off after on, rebuilt,
    equals never-on in the room WITH its pane"""
    mesh = GW.glass_room(True, 0.5)
    solid = GW.glass_room(True, 0.5)
    solid.transmission["thin_walled"] = 0
    seen = {}
    for on in (False, True):
        pt = pane_pt(solid, on, IW.WINDOW_ROOM, sky=IW.room_sky(), lens=(0.05, 6.0, 1.0))
        try:
            assert pt.ctx.pane_shadow_info() == 0 and pt.ctx.get_pane_shadows() == on
            seen[on] = observed(pt)
        finally:
            pt.close()
    for a, b in zip(seen[False], seen[True]):
        assert np.array_equal(a, b)
    pt = pane_pt(mesh, False, IW.WINDOW_ROOM, sky=IW.room_sky(), lens=(0.05, 6.0, 1.0))
    try:
        never = observed(pt)
        pt.set_pane_shadows(True)
        assert pt.ctx.pane_shadow_info() == 1
        with_panes = observed(pt)
        assert not np.array_equal(with_panes[0], never[0]) and not np.array_equal(with_panes[2], never[2])  # (the records carry the marks)
        assert np.array_equal(with_panes[1], never[1])  # the nodes do not
        pt.set_pane_shadows(False)
        assert pt.ctx.pane_shadow_info() == 0
        for a, b in zip(never, observed(pt)):
            assert np.array_equal(a, b)
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 11 partitions and options
def room_frame(window=IW.WINDOW_ROOM, flags=FULL | L.F_NEE_EMISSIVE, spp=4, setup=None, **kw):
    """glass_room: one pane and a solid block under sky and emitters -- a shadow ray crosses at most one pane"""
    pt = pane_pt(GW.glass_room(True, 0.5), True, window, sky=IW.room_sky(), lens=(0.05, 6.0, 1.0), **kw)
    try:
        assert pt.ctx.pane_shadow_info() == 1
        if setup:
            setup(pt)
        return frame(pt, flags, spp, 6, window=window, cam=IW.ROOM_CAMERA)
    finally:
        pt.close()


def test_same_bits_for_every_batch_size_option_and_instance_mode():
    whole = room_frame()
    assert whole.max() > 0.0
    assert np.array_equal(bits(whole), bits(room_frame(setup=lambda pt: pt.ctx.set_option(L.OPT_BATCH_SPP, 1))))
    assert np.array_equal(bits(whole), bits(room_frame(setup=lambda pt: pt.ctx.set_option(L.OPT_COUNT_TRAVERSAL, 1))))
    assert np.array_equal(bits(whole), bits(room_frame(options=[(L.OPT_SHADOW_EXIT_TABLE, 0)])))
    assert np.array_equal(bits(whole), bits(room_frame(mode=1)))
    assert np.array_equal(bits(whole), bits(room_frame(mode=1, setup=lambda pt: pt.ctx.set_option(L.OPT_COUNT_TRAVERSAL, 1))))


def test_two_ranks_stitch_to_one():
    W, H = window = (128, 48)
    whole = room_frame(window)
    for r in range(2):
        part = room_frame(window, rank=r, n_ranks=2)
        m = owned_mask(W, H, r, 2)
        assert m.any() and not m.all()
        assert np.array_equal(bits(part[m]), bits(whole[m]))


# ---------------------------------------------------------------------------------------------------------------- 12 small windows
@pytest.mark.parametrize("window", ((60, 44), (8, 8)))
def test_windows_that_do_not_fill_their_last_block(window):
    """60 x 44: 2640 paths, five blocks of 512 and a part of one; 8 x 8: 64 paths, less than one block.  The closed form of the first test.
    (An 8 x 8 window has few pixels, each large: the share beside an outline is not asserted there, only what the pixels show.)"""
    factor, use, crossed = PN.closed_form("pane", "directional", window)
    free = free_frame("directional", window).reshape(-1, 3).astype(np.float64)
    got = one_frame(PN.world("pane", "directional"), P, 1, 2, window=window, want_panes=1).reshape(-1, 3)
    bound = free * factor * relative_bound("pane", "directional", window)[:, None]
    assert (use & (crossed == 1)).any() and (use & (crossed == 0)).any()
    assert np.all(np.abs(got.astype(np.float64) - free * factor)[use] <= bound[use])
    assert got.shape[0] == window[0] * window[1]


# ---------------------------------------------------------------------------------------------------------------- 13 the contract
def test_contract_of_the_three_calls():
    mesh = PN.world("pane", "directional")
    pt = pane_pt(mesh, True)
    try:
        ctx = pt.ctx
        before = frame(pt, P, 1, 2)
        assert ctx.get_pane_shadows() is True and ctx.pane_shadow_info() == 1
        # refusals change nothing: the structure stays usable, the frame keeps its bits
        for bad in (2, -1, 7):
            with pytest.raises(L.Rt3Error) as e:
                ctx.set_pane_shadows(bad)
            assert e.value.code == L.E_INVALID
        assert ctx.get_pane_shadows() is True and np.array_equal(bits(frame(pt, P, 1, 2)), bits(before))
        # the same value again is no change
        ctx.set_pane_shadows(True)
        assert np.array_equal(bits(frame(pt, P, 1, 2)), bits(before))
        # a change takes effect at the next build; until then the structure is unusable
        ctx.set_pane_shadows(False)
        with pytest.raises(L.Rt3Error) as e:
            frame(pt, P, 1, 2)
        assert e.value.code == L.E_STATE
        with pytest.raises(L.Rt3Error) as e:
            ctx.pane_shadow_info()
        assert e.value.code == L.E_STATE
        ctx.build_accel()
        assert ctx.pane_shadow_info() == 0
        off = frame(pt, P, 1, 2)
        assert not np.array_equal(bits(off), bits(before))
        ctx.set_pane_shadows(True)
        ctx.build_accel()
        assert np.array_equal(bits(frame(pt, P, 1, 2)), bits(before))
        # the mode survives rt3_scene_set_geometry (which forgets the transmission table: upload_mesh sets it again)
        ctx.upload_mesh(mesh)
        assert ctx.get_pane_shadows() is True
        ctx.build_accel()
        assert ctx.pane_shadow_info() == 1 and np.array_equal(bits(frame(pt, P, 1, 2)), bits(before))
        # a refit keeps the marks
        ctx.update_vertices(mesh.vertices, 0)
        ctx.refit_accel()
        assert ctx.pane_shadow_info() == 1 and np.array_equal(bits(frame(pt, P, 1, 2)), bits(before))
        # an imported structure has no marks: refused while the built one has panes, accepted without
        nodes, tris = ctx.accel_download()
        with pytest.raises(L.Rt3Error) as e:
            ctx.accel_import(nodes, tris)
        assert e.value.code == L.E_UNSUPPORTED
        assert np.array_equal(bits(frame(pt, P, 1, 2)), bits(before))
        # panes need the default node layout; without a pane the mode asks nothing of it
        ctx.set_option(L.OPT_NODE_WIDTH, 2)
        with pytest.raises(L.Rt3Error) as e:
            ctx.build_accel()
        assert e.value.code == L.E_UNSUPPORTED and "rt3_scene_set_pane_shadows" in str(e.value)
        ctx.set_transmission([])
        ctx.build_accel()
        assert ctx.pane_shadow_info() == 0
        ctx.set_option(L.OPT_NODE_WIDTH, 4)
        ctx.set_transmission(mesh.transmission)
        ctx.build_accel()
        assert np.array_equal(bits(frame(pt, P, 1, 2)), bits(before))
    finally:
        pt.close()


def test_set_pane_shadows_rebuilds_like_set_scene():
    pt = PathTracer(PN.WINDOW)
    try:
        pt.set_pane_shadows(True)  # before a scene: only the mode
        pt.set_scene(PN.world("pane", "directional"), None, assets.load_bluenoise())
        assert pt.ctx.pane_shadow_info() == 1
        on = frame(pt, P, 1, 2)
        pt.set_pane_shadows(False)
        assert pt.ctx.pane_shadow_info() == 0
        off = frame(pt, P, 1, 2)
        assert on.sum() > off.sum() > 0.0
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 14 the ledger
SEALED = [(n_extra, textured, lights) for n_extra in (0, 253) for textured in (False, True) for lights in ("none", "emitters", "emitters_point")]


@pytest.mark.parametrize("n_extra,textured,lights", SEALED, ids=[f"{4 + n}geoms-{'mat' if t else 'plain'}-{l}" for n, t, l in SEALED])
def test_opaque_vertices_keep_their_bits(n_extra, textured, lights):
    """test_glass's sealed world with its sealed triangle a thin pane and the mode on: the frame is shaded by k_shade_pane<GLDS, EMIT, MAT,
    PUNCT> and its shadow rays walk k_shadow_pane, no path and no shadow ray reaches the pane, and the frame equals the one with
    transmission 0, which k_shade, k_shade_punct and k_shadow make, bit for bit."""
    mesh, k = GW.sealed_world(n_extra, textured, emissive=True)
    mesh.transmission["thin_walled"][k] = 1
    flags = FULL | {"none": 0, "emitters": L.F_NEE_EMISSIVE, "emitters_point": L.F_NEE_EMISSIVE | L.F_NEE_PUNCTUAL}[lights]
    if lights == "emitters_point":
        mesh.lights = assets.lights_array([assets.make_light(assets.LIGHT_POINT, GW.SEALED_LIGHT["intensity"], position=GW.SEALED_LIGHT["position"])])
    pt = pane_pt(mesh, True, GW.WINDOW, sky=LW.constant_sky(GW.SKY_L), lens=(0.0, 1.0, 1.0))
    try:
        assert pt.ctx.pane_shadow_info() == 1
        glassy = frame(pt, flags, 4, 3, window=GW.WINDOW, cam=GW.SEALED_CAMERA)
        t = mesh.transmission.copy()
        t["transmission"] = 0.0
        pt.ctx.set_transmission(t)
        pt.ctx.build_accel()
        assert pt.ctx.pane_shadow_info() == 0
        opaque = frame(pt, flags, 4, 3, window=GW.WINDOW, cam=GW.SEALED_CAMERA)
    finally:
        pt.close()
    assert np.isfinite(glassy).all() and (glassy > 0).mean() > 0.25
    assert np.array_equal(bits(glassy), bits(opaque))


_SEALED = f"{HERE}::test_opaque_vertices_keep_their_bits"
_ROOM = f"{HERE}::test_same_bits_for_every_batch_size_option_and_instance_mode"
_CLOSED = f"{HERE}::test_directional_light_through_a_pane"
# instance -> (when the launchers pick it, a test above that launches it)
LEDGER = {
    "k_shade_pane<true, false, false, false>": ("<= 256 geometries, no light table", f"{HERE}::test_same_expectation_as_without_the_mode"),
    "k_shade_pane<true, true, false, false>": ("<= 256 geometries, emitters", _ROOM),
    "k_shade_pane<true, true, false, true>": ("<= 256 geometries, emitters and punctual lights", _CLOSED),
    "k_shade_pane<true, false, true, false>": ("<= 256 geometries, material textures, no light table", _SEALED),
    "k_shade_pane<true, true, true, false>": ("<= 256 geometries, material textures, emitters", _SEALED),
    "k_shade_pane<true, true, true, true>": ("<= 256 geometries, material textures, emitters and punctual lights", _SEALED),
    "k_shade_pane<false, false, false, false>": ("> 256 geometries, no light table", _SEALED),
    "k_shade_pane<false, true, false, false>": ("> 256 geometries, emitters", _SEALED),
    "k_shade_pane<false, true, false, true>": ("> 256 geometries, emitters and punctual lights", _SEALED),
    "k_shade_pane<false, false, true, false>": ("> 256 geometries, material textures, no light table", _SEALED),
    "k_shade_pane<false, true, true, false>": ("> 256 geometries, material textures, emitters", _SEALED),
    "k_shade_pane<false, true, true, true>": ("> 256 geometries, material textures, emitters and punctual lights", _SEALED),
    "k_shadow_pane<false, 2, false>": ("one tree, the sky queue", _ROOM),
    "k_shadow_pane<false, 2, true>": ("one tree, the emitter and punctual queue", _CLOSED),
    "k_shadow_pane<true, 2, false>": ("one tree, counting, the sky queue", _ROOM),
    "k_shadow_pane<true, 2, true>": ("one tree, counting, the emitter and punctual queue", _ROOM),
    "k_shadow_pane<false, 4, false>": ("two-level, the sky queue", _ROOM),
    "k_shadow_pane<false, 4, true>": ("two-level, the emitter and punctual queue", f"{HERE}::test_two_stacked_panes_multiply"),
    "k_shadow_pane<true, 4, false>": ("two-level, counting, the sky queue", _ROOM),
    "k_shadow_pane<true, 4, true>": ("two-level, counting, the emitter and punctual queue", _ROOM),
}


def library_instances():
    """the template instances of the two pane kernels in librt3.so's symbol table (their host stubs; names only)"""
    lib = ROOT / "raytracer3_amd" / "librt3.so"
    out = None
    for nm in ("nm", "/opt/rocm/llvm/bin/llvm-nm"):
        try:
            out = subprocess.run([nm, "-C", str(lib)], capture_output=True, text=True, check=True).stdout
            break
        except (OSError, subprocess.CalledProcessError):
            continue
    assert out is not None, "neither nm nor llvm-nm could read the library"
    return set(re.findall(r"__device_stub__((?:k_shade_pane|k_shadow_pane)<[^>]*>)\(", out))


def test_pane_instance_ledger():
    """fails when an instance of k_shade_pane or k_shadow_pane is added without an entry here, or an entry outlives its instance, or a
    credited test is gone"""
    have = library_instances()
    assert len([n for n in have if n.startswith("k_shade_pane")]) == 12 and len([n for n in have if n.startswith("k_shadow_pane")]) == 8, sorted(have)
    assert have == set(LEDGER), (sorted(have - set(LEDGER)), sorted(set(LEDGER) - have))
    text = (ROOT / HERE).read_text()
    for name, (conditions, credit) in LEDGER.items():
        path, _, test = credit.partition("::")
        assert conditions and path == HERE and re.search(rf"^def {re.escape(test)}\(", text, re.M), (name, credit)


# ---------------------------------------------------------------------------------------------------------------- 7 a constant sky over a wide pane
def test_constant_sky_over_a_very_wide_pane():
    """RT3_F_NEE_SKY, B = 1: the floor vertex is the last, its sky light sample has weight 1 and crosses the pane, attenuated (k_shadow_pane's
    sky-queue instance).  Expectation per pixel rho L c K, K = 2 int (1 - F'(theta)) cos(theta) sin(theta) d theta in float64.  The finite
    pane (600 x 600 at height 3) is missed only by rays with cos(theta) < 3 / 297 from a floor point in view, which carry at most
    rho L (3 / 297)^2 = 1.02e-4 rho L unattenuated: added to the band.  The sample's variance follows from the sampler's definition
    (pane_worlds.wide_pane_moments: a constant sky's texel density is proportional to the sine of the row centre's polar angle), not
    from the frame; 2 % are added for the 16-bit alias thresholds and the fp32 row table.  A row's mean over its 64 pixels and S samples
    lies within 5 sigma / sqrt(64 S) of the expectation, plus (S + 48) u of rounding.  The band tells F' from F."""
    S, h = 4096, 32
    L_sky, rho, c = np.asarray(GW.SKY_L, np.float64), np.asarray(PN.ALBEDO, np.float32).astype(np.float64), np.asarray(PN.TINT, np.float32).astype(np.float64)
    K, M2 = PN.wide_pane_moments(h)
    K_wrong, _ = PN.wide_pane_moments(h, thin_slab=False)
    mu = rho * L_sky * c * K
    sigma = 1.02 * rho * L_sky * c * np.sqrt(M2 - K * K)
    got = one_frame(PN.wide_pane_world(), L.F_NEE_SKY, S, 1, sky=LW.constant_sky(GW.SKY_L, 64, h), want_panes=1).astype(np.float64)
    W, H = PN.WINDOW
    band = 5.0 * sigma / np.sqrt(W * S) + (S + 48) * U * mu + 1.1 * PN.WIDE_MISSED_COS**2 * rho * L_sky
    dev = np.abs(got.mean(1) - mu)
    print(f"wide pane: K = {K:.5f} (with F instead of F': {K_wrong:.5f}), sigma / mu = {(sigma / mu).max():.3f}, band / mu = {(band / mu).max():.4f}, "
          f"worst row deviation {(dev / band).max():.2f} bands, frame mean / mu = {(got.mean((0, 1)) / mu)}")
    assert np.all(dev <= band)
    assert np.all(np.abs(rho * L_sky * c * (K_wrong - K)) > 2.0 * band), "the band can tell F' from F"


# ---------------------------------------------------------------------------------------------------------------- 9 the window room
def window_frames(name, mode=0):
    from test_pane_shadows_cpu import fixture

    flags, bounces, specular, tau, emitter, lights, _, _, frames = PN.WINDOW_CASES[name]
    pt = pane_pt(PN.window_room(specular, tau, emitter, lights), True, IW.WINDOW_ROOM, sky=IW.room_sky(), lens=PN.ROOM_LENS, mode=mode)
    try:
        assert pt.ctx.pane_shadow_info() == 1
        cam = camera(PN.ROOM_CAMERA, IW.WINDOW_ROOM)
        out = []
        for k in range(frames):
            pt.render(pt.make_gconst(cam, IW.FRAME_SPP, bounces, frame=k, flags=flags))
            out.append(pt.light()[..., :3].copy())
        return np.stack(out), fixture()
    finally:
        pt.close()


@pytest.mark.parametrize("name,mode", (("window_sky_b4", 0), ("window_emit_spec_b6", 0), ("window_sun_b4", 0), ("window_sun_b4", 1)))
def test_window_room_against_the_float64_reference(name, mode):
    """A closed room lit only through the pane of its roof light, against tests/golden/pane_shadows_ref.npz (ref_pane_shadows.py, which samples
    lights its own way: only the expectation is shared).  `window_emit_spec_b6` -- transmission 0.5, an emissive quad outside, the layered
    BSDF -- is where the emitter weight reads the distance P2 carries: test_pane_shadows_cpu.test_a_wrong_distance_fails_the_fixture_case
    shows that this case rejects the last-segment distance."""
    W, H = IW.WINDOW_ROOM
    frames, fx = window_frames(name, mode)
    check_against_fixture(frames, np.ones((H, W), bool), fx, name)


# ---------------------------------------------------------------------------------------------------------------- more of 11, 12, 13
def test_instance_modes_differ_by_the_products_association_only():
    """several crossings per ray: the two-level walk may meet the panes in the other order, c A1 A2 against c A2 A1 -- each frame carries one
    rounding per extra crossing beyond the first, so the two differ by at most 2 (k - 1) u relative behind k panes, and not at all elsewhere"""
    _, _, crossed = PN.closed_form("stacked", "directional")
    a = one_frame(PN.world("stacked", "directional"), P, 1, 2, want_panes=2, mode=0).reshape(-1, 3).astype(np.float64)
    b = one_frame(PN.world("stacked", "directional"), P, 1, 2, want_panes=2, mode=1).reshape(-1, 3).astype(np.float64)
    extra = np.maximum(crossed - 1, 0)[:, None]
    assert (crossed == 2).sum() > 200 and np.all(np.abs(a - b) <= 2.0 * extra * U * np.abs(a))


def test_more_than_256_geometries_behind_a_pane():
    """the GLDS = false instances of k_shade_pane with a pane in the light's way: the directional closed form in a world padded with 255
    geometries under the floor (257 in all), where the glass entry and its pane bit come from the table in memory"""
    mesh = PN.world("pane", "directional", n_extra=255)
    assert len(mesh.geometries) == 257
    factor, use, crossed = PN.closed_form("pane", "directional")
    free = free_frame("directional").reshape(-1, 3).astype(np.float64)
    got = one_frame(mesh, P, 1, 2, want_panes=1).reshape(-1, 3)
    bound = free * factor * relative_bound("pane", "directional")[:, None]
    inside, outside = use & (crossed == 1), use & (crossed == 0)
    assert inside.sum() > 300 and np.all(np.abs(got.astype(np.float64) - free * factor)[inside] <= bound[inside])
    assert np.array_equal(bits(got[outside]), bits(free_frame("directional").reshape(-1, 3)[outside]))
    # and the frame is the unpadded world's, bit for bit
    assert np.array_equal(bits(got), bits(one_frame(PN.world("pane", "directional"), P, 1, 2, want_panes=1).reshape(-1, 3)))


def test_refit_keeps_the_marks_in_the_two_level_structure():
    mesh = PN.world("stacked", "directional")
    pt = pane_pt(mesh, True, mode=1)
    try:
        before = frame(pt, P, 1, 2)
        pt.ctx.update_vertices(mesh.vertices, 0)
        pt.ctx.refit_accel()
        assert pt.ctx.pane_shadow_info() == 2 and np.array_equal(bits(frame(pt, P, 1, 2)), bits(before))
        assert before.reshape(-1, 3)[PN.closed_form("stacked", "directional")[2] == 2].all()
    finally:
        pt.close()
