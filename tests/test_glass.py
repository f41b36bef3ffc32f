"""Glass on the GPU (rt3_scene_set_transmission): the glass function against float64, closed forms for the thin pane,
the tinted pane, the solid slab and the edge seen through a slab, "opaque vertices keep their bits" in all twelve k_shade_glass
configurations, the whole integrator against the float64 fixture, invariance under batch size, instance mode, tile partition and window
size, the contract of the new call, and a ledger of the twelve kernel instances.

Bounds are derived: fp32 results carry one unit of 2^-24 per rounding of the longest chain; a pixel of the flat worlds of glass_worlds is a
two-point variable (5 sigma of its bounded deviation, exact where only one value is possible)."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import glass_worlds as GW
import integrator_worlds as IW
import lens_worlds as LW
import ref_glass as RG
from raytracer3_amd import _lib as L
from raytracer3_amd import assets
from support import bits, camera
from test_glass_cpu import fixture, op32_reference, op32_rows
from test_integrator_cpu import check_against_fixture
from test_nee_emissive import make_pt, owned_mask

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HERE = "tests/test_glass.py"
U = 2.0**-24
FULL = L.F_NEE_SKY | L.F_BLUENOISE | L.F_FACEFORWARD | L.F_SPECULAR
SKY = np.array(GW.SKY_L)


def glass_pt(mesh, window=GW.WINDOW, sky=GW.SKY_L, lens=GW.PINHOLE, **kw):
    """a PathTracer over a glass world under a constant sky (or none), its lens set"""
    pt = make_pt(mesh, window, sky=None if sky is None else LW.constant_sky(sky), **kw)
    pt.set_lens(*lens)
    return pt


def frame(pt, flags, spp, bounces, window=GW.WINDOW, cam=GW.CAMERA, index=0):
    pt.render(pt.make_gconst(camera(cam, window), spp, bounces, frame=index, flags=flags))
    return pt.light()[..., :3].copy()


def one_frame(mesh, flags, spp, bounces, **kw):
    pt = glass_pt(mesh, **kw)
    try:
        return frame(pt, flags, spp, bounces, window=kw.get("window", GW.WINDOW))
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 1 the glass function
def test_glass_function_against_float64():
    """Self-test op 32 on the rows of test_glass_cpu.op32_rows: direction and F inside the rounding bounds that op32_reference derives
    (its docstring has the derivation), the event equal wherever u is further from F than F's bound.  Open rows are under 1 %
    (test_glass_cpu.test_op32_rows_leave_few_events_open checks that share without a GPU)."""
    ior, thin, d, n, u = op32_rows()
    rows = np.concatenate([bits(ior)[:, None], thin[:, None], bits(d), bits(n), bits(u)[:, None]], 1).astype(np.uint32)
    pt = glass_pt(GW.pane_world())
    try:
        out = pt.ctx.selftest(L.SELFTEST_GLASS, rows, 5)
    finally:
        pt.close()
    ev, direction, F = out[:, 0], np.ascontiguousarray(out[:, 1:4]).view(np.float32).astype(np.float64), np.ascontiguousarray(out[:, 4]).view(np.float32).astype(np.float64)
    tr, want, Fw, d_dir, dF, open_, ev_open = op32_reference(ior, thin, d, n, u)
    assert ev_open.mean() < 0.01
    err_F = np.abs(F - Fw)[~open_]
    print(f"op 32: worst |F - ref| / bound {np.max(err_F / np.maximum(dF[~open_], U)):.3f}; {int(ev_open.sum())} of {len(u)} rows open")
    assert np.all(err_F <= dF[~open_] + U * Fw[~open_])
    assert np.array_equal(ev[~ev_open], tr[~ev_open].astype(np.uint32)) and set(ev) <= {0, 1}
    same = (ev == tr) & ~open_
    err_d = np.abs(direction - want).max(-1)[same]
    print(f"op 32: worst |direction - ref| / bound {np.max(err_d / d_dir[same]):.3f} over {int(same.sum())} rows")
    assert np.all(err_d <= d_dir[same])
    # an index-matched surface is no surface: F = 0 exactly, and the unit direction goes on unchanged
    k = np.flatnonzero((ior == 1.0) & (thin == 0))
    ud = d[k].astype(np.float64) / np.linalg.norm(d[k].astype(np.float64), axis=1, keepdims=True)
    assert len(k) and np.all(F[k] == 0.0) and np.all(ev[k] == 1) and np.abs(direction[k] - ud).max() <= 4 * U


# ---------------------------------------------------------------------------------------------------------------- 2 the thin pane
def sky_bound(S):
    """three roundings for the bilinear blend of a constant, S + 1 for the mean of S samples, four for a throughput of 1 x 1"""
    return (S + 8) * U


@pytest.fixture(scope="module")
def pane_pt():
    pt = glass_pt(GW.pane_world())
    yield pt
    pt.close()


@pytest.mark.parametrize("bounces", (1, 2, 4))
def test_thin_pane_under_a_constant_sky_is_the_sky(pane_pt, bounces):
    """reflected or transmitted, with throughput 1, the path ends in the sky: every pixel off the diffuse wall is L.  B = 1 pins the last
    vertex's sky shadow ray (rule 4)."""
    S = 4
    got = frame(pane_pt, L.F_NEE_SKY, S, bounces)
    wall, pane = GW.inside(GW.WALL_COLS, GW.PANE_ROWS), GW.inside(GW.PANE_COLS, GW.PANE_ROWS)
    rel = np.abs(got[~wall].astype(np.float64) / SKY - 1.0)
    print(f"thin pane B={bounces}: worst relative error {rel.max() / U:.1f} units of 2^-24 (bound {S + 8}); pane pixels {int(pane.sum())}")
    assert pane.sum() > 500 and rel.max() <= sky_bound(S)
    assert got[GW.inside(GW.WALL_COLS, GW.PANE_ROWS, margin=1.0)].mean() > 0.05  # the wall is lit by the sky


@pytest.mark.parametrize("bounces", (2, 4))
def test_the_sky_shows_through_glass_without_sky_sampling(pane_pt, bounces):
    """rule 5: without RT3_F_NEE_SKY the pane shows the sky it stands in front of; the diffuse wall beside it, which sees nothing but
    sky, stays black; and a last glass vertex (B = 1) adds nothing"""
    S = 4
    got = frame(pane_pt, 0, S, bounces)
    wall, pane = GW.inside(GW.WALL_COLS, GW.PANE_ROWS), GW.inside(GW.PANE_COLS, GW.PANE_ROWS)
    assert np.abs(got[~wall].astype(np.float64) / SKY - 1.0).max() <= sky_bound(S)
    assert not got[wall].any()
    one = frame(pane_pt, 0, S, 1)
    assert not one[pane].any() and not one[wall].any() and np.abs(one[~wall & ~pane].astype(np.float64) / SKY - 1.0).max() <= sky_bound(S)


# ---------------------------------------------------------------------------------------------------------------- 3 the tinted pane
def test_tinted_pane_mixes_sky_and_tinted_sky_by_the_thin_slab_reflectance():
    """NEE_SKY, B = 2: a sample of a pane pixel is L (reflected, probability F') or c L (transmitted).  Per pixel row the mean over the
    row's n pane pixels and S samples has expectation mean_p(F'_p L + (1 - F'_p) c L); every sample lies in [c L, L], so its standard
    deviation is at most (L - c L) / 2 and the row mean lies within 5 (L - c L) / (2 sqrt(n S)) of it.  Derived, not measured.  The band
    is narrow enough to tell F' = 2 F / (1 + F) from F: the two expectations are more than two bands apart."""
    S = 1024
    c = np.array(GW.TINT)
    got = one_frame(GW.pane_world(GW.TINT), L.F_NEE_SKY, S, 2).astype(np.float64)
    pane = GW.inside(GW.PANE_COLS, GW.PANE_ROWS)
    F = RG.fresnel(-GW.pixel_dirs()[..., 2], GW.IOR)
    Ft = RG.thin_fresnel(F)
    rows = np.flatnonzero(pane.any(1))
    assert len(rows) >= 30
    worst = 0.0
    for y in rows:
        m = pane[y]
        n = int(m.sum())
        want = (Ft[y, m, None] * SKY + (1.0 - Ft[y, m, None]) * c * SKY).mean(0)
        wrong = (F[y, m, None] * SKY + (1.0 - F[y, m, None]) * c * SKY).mean(0)
        band = 5.0 * (SKY - c * SKY) / (2.0 * np.sqrt(n * S)) + sky_bound(S) * SKY
        dev = np.abs(got[y, m].mean(0) - want)
        worst = max(worst, float((dev / band).max()))
        assert np.all(dev <= band), (y, dev, band)
        assert np.all(np.abs(want - wrong) > 2.0 * band), "the band can tell F' from F"
    print(f"tinted pane: worst deviation {worst:.2f} bands over {len(rows)} rows")


# ---------------------------------------------------------------------------------------------------------------- 4 the slab furnace
def slab_furnace_bound(window, bounces, S):
    """A path through an untinted slab under a constant sky ends in the sky unless its last vertex, inside, turns it back: through the
    front (1 - R), turned back at each of the B - 1 vertices that follow (R each).  R at the largest incidence in view."""
    mesh, normal, _ = GW.slab_world()
    R = float(RG.fresnel(-np.sum(GW.pixel_dirs(window) * normal, -1), GW.IOR).max())
    return mesh, (1.0 - R) * R ** (bounces - 1) + sky_bound(S)


def test_solid_slab_furnace():
    S, B = 4, 8
    mesh, bound = slab_furnace_bound(GW.WINDOW, B, S)
    got = one_frame(mesh, L.F_NEE_SKY, S, B).astype(np.float64)
    rel = np.abs(got / SKY - 1.0)
    print(f"slab furnace B={B}: worst relative error {rel.max():.3e} (bound {bound:.3e})")
    assert rel.max() <= bound


# ---------------------------------------------------------------------------------------------------------------- 5 the edge through a slab
EDGE_PX = 30.3


@pytest.mark.parametrize("tilt", (0.0, 35.0))
def test_edge_seen_through_a_slab(tilt):
    """B = 4, no sky: the pixels that see the emissive half-plane through the slab are the ones the closed form of the displacement says
    (t sin(theta_i - theta_t) / cos(theta_t)); a lit pixel's samples are Le with probability p = (1 - R)^2 and 0 otherwise, so its mean
    lies within 5 sqrt(p (1 - p) / S) Le of p Le; dark pixels are exactly 0.  Pixels within 1e-3 m of the displaced edge are left out,
    at most 5 % of them (the share is the closed form's alone)."""
    S = 256
    mesh, normal, _ = GW.slab_world(tilt_deg=tilt, emitter_edge_px=EDGE_PX)
    dist, th_i = GW.edge_distance(normal, GW.IOR, EDGE_PX)
    near = np.abs(dist) < 1e-3
    assert near.mean() <= 0.05
    lit, dark = (dist >= 0.0) & ~near, (dist < 0.0) & ~near
    got = one_frame(mesh, 0, S, 4, sky=None).astype(np.float64)
    assert lit.sum() > 500 and dark.sum() > 500 and not got[dark].any()
    p = (1.0 - RG.fresnel(np.cos(th_i), GW.IOR)) ** 2
    band = 5.0 * np.sqrt(p * (1.0 - p) / S) + (S + 8) * U
    dev = np.abs(got / GW.LE - p[..., None]).max(-1)
    print(f"edge through a slab tilted by {tilt}: worst deviation {np.max(dev[lit] / band[lit]):.2f} bands over {int(lit.sum())} lit pixels")
    assert np.all(dev[lit] <= band[lit])


def test_an_index_matched_slab_is_not_there():
    """ior = 1: F = 0 and the direction is handed on unchanged, so the frame is the frame without the slab, bit for bit"""
    S = 16
    with_slab = one_frame(GW.slab_world(ior=1.0, tilt_deg=35.0, emitter_edge_px=EDGE_PX)[0], 0, S, 4, sky=None)
    without = one_frame(GW.slab_world(emitter_edge_px=EDGE_PX, with_slab=False)[0], 0, S, 4, sky=None)
    assert without.any() and not without.all() and np.array_equal(bits(with_slab), bits(without))


# ---------------------------------------------------------------------------------------------------------------- 6 opaque vertices
SEALED = [(n_extra, textured, lights) for n_extra in (0, 253) for textured in (False, True) for lights in ("none", "emitters", "emitters_point")]


@pytest.mark.parametrize("n_extra,textured,lights", SEALED, ids=[f"{4 + n}geoms-{'mat' if t else 'plain'}-{l}" for n, t, l in SEALED])
def test_opaque_vertices_keep_their_bits(n_extra, textured, lights):
    """The glass triangle is sealed inside an opaque box: no path reaches it, every vertex is opaque.  With transmission 1 on it the
    frame is shaded by k_shade_glass<GLDS, EMIT, MAT, PUNCT> -- 4 and 257 flattened geometries, with and without the material-texture
    table, without a light table, with emitters, with emitters and a point light -- and equals the frame with transmission 0, which
    k_shade and k_shade_punct shade, bit for bit: an opaque vertex in a glass scene draws what it draws without glass."""
    mesh, k = GW.sealed_world(n_extra, textured, emissive=True)  # (without RT3_F_NEE_EMISSIVE the block's light arrives by BSDF sampling alone)
    assert len(mesh.geometries) == 4 + n_extra
    flags = FULL | {"none": 0, "emitters": L.F_NEE_EMISSIVE, "emitters_point": L.F_NEE_EMISSIVE | L.F_NEE_PUNCTUAL}[lights]
    if lights == "emitters_point":
        mesh.lights = assets.lights_array([assets.make_light(assets.LIGHT_POINT, GW.SEALED_LIGHT["intensity"], position=GW.SEALED_LIGHT["position"])])
    pt = glass_pt(mesh, lens=(0.0, 1.0, 1.0))
    try:
        assert pt.ctx.get_lens()[1]
        glassy = frame(pt, flags, 4, 3, cam=GW.SEALED_CAMERA)
        if lights != "none":
            assert pt.ctx.light_info()[0] > 0
        t = mesh.transmission.copy()
        t["transmission"] = 0.0
        pt.ctx.set_transmission(t)
        pt.ctx.build_accel()
        opaque = frame(pt, flags, 4, 3, cam=GW.SEALED_CAMERA)
    finally:
        pt.close()
    assert np.isfinite(glassy).all() and (glassy > 0).mean() > 0.25  # (4 samples: where the block's light was found)
    assert np.array_equal(bits(glassy), bits(opaque))


# ---------------------------------------------------------------------------------------------------------------- 7 the fixture
def room_frames(name, mode=0, n_frames=None):
    flags, bounces, specular, tau, _, _, frames = GW.ROOM_CASES[name]
    pt = make_pt(GW.glass_room(specular, tau), IW.WINDOW_ROOM, sky=IW.room_sky(), mode=mode)
    try:
        pt.set_lens(*GW.ROOM_LENS)
        cam = camera(IW.ROOM_CAMERA, IW.WINDOW_ROOM)
        out = []
        for k in range(n_frames or frames):
            pt.render(pt.make_gconst(cam, IW.FRAME_SPP, bounces, frame=k, flags=flags))
            out.append(pt.light()[..., :3].copy())
        return np.stack(out)
    finally:
        pt.close()


@pytest.mark.parametrize("name", sorted(GW.ROOM_CASES))
def test_gpu_against_fixture(name):
    W, H = IW.WINDOW_ROOM
    check_against_fixture(room_frames(name), np.ones((H, W), bool), fixture(), name)


def test_gpu_against_fixture_two_level():
    W, H = IW.WINDOW_ROOM
    check_against_fixture(room_frames("glass_half_b4", mode=1), np.ones((H, W), bool), fixture(), "glass_half_b4")


# ---------------------------------------------------------------------------------------------------------------- 8 plumbing
def room_frame(window=IW.WINDOW_ROOM, flags=FULL | L.F_NEE_EMISSIVE, spp=4, setup=None, **kw):
    pt = make_pt(GW.glass_room(True, 0.5), window, sky=IW.room_sky(), **kw)
    try:
        pt.set_lens(0.05, 6.0, 1.0)
        if setup:
            setup(pt)
        return frame(pt, flags, spp, 6, window=window, cam=IW.ROOM_CAMERA)
    finally:
        pt.close()


def test_same_bits_for_every_batch_size_and_instance_mode():
    whole = room_frame()
    assert whole.max() > 0.0
    assert np.array_equal(bits(whole), bits(room_frame(setup=lambda pt: pt.ctx.set_option(L.OPT_BATCH_SPP, 1))))
    assert np.array_equal(bits(whole), bits(room_frame(mode=1)))


def test_two_ranks_stitch_to_one():
    W, H = window = (128, 48)
    whole = room_frame(window)
    for r in range(2):
        part = room_frame(window, rank=r, n_ranks=2)
        m = owned_mask(W, H, r, 2)
        assert m.any() and not m.all()
        assert np.array_equal(bits(part[m]), bits(whole[m]))


@pytest.mark.parametrize("window", ((60, 44), (8, 8)))
def test_windows_that_do_not_fill_their_last_block(window):
    """60 x 44 at 1 spp: 2640 paths, five blocks of 512 and a part of one; 8 x 8: 64 paths, less than one block.  The slab furnace: every
    pixel is the sky"""
    mesh, bound = slab_furnace_bound(window, 8, 1)
    got = one_frame(mesh, L.F_NEE_SKY, 1, 8, window=window).astype(np.float64)
    assert got.shape[:2] == window[::-1] and np.abs(got / SKY - 1.0).max() <= bound


BAD_TABLES = {
    "transmission above 1": dict(transmission=1.5), "negative transmission": dict(transmission=-0.25), "transmission NaN": dict(transmission=np.nan),
    "ior below 1": dict(ior=0.99), "ior inf": dict(ior=np.inf), "ior NaN": dict(ior=np.nan), "thin_walled 2": dict(thin_walled=2), "reserved": dict(reserved=1),
}


def test_contract_of_the_new_call():
    mesh = GW.pane_world(GW.TINT)
    pt = glass_pt(mesh)
    try:
        ctx = pt.ctx
        before = frame(pt, L.F_NEE_SKY, 4, 2)
        # refusals change nothing: the structure stays usable and the frame keeps its bits
        for what, bad in BAD_TABLES.items():
            t = mesh.transmission.copy()
            for key, value in bad.items():
                t[key][1] = value
            with pytest.raises(L.Rt3Error) as e:
                ctx.set_transmission(t)
            assert e.value.code == L.E_INVALID, what
        for n in (1, 3):
            with pytest.raises(L.Rt3Error) as e:
                ctx.set_transmission(assets.no_transmission(n))
            assert e.value.code == L.E_INVALID
        assert np.array_equal(bits(frame(pt, L.F_NEE_SKY, 4, 2)), bits(before))
        # an accepted table takes effect at the next build; until then the structure is unusable
        ctx.set_transmission(mesh.transmission)
        with pytest.raises(L.Rt3Error) as e:
            frame(pt, L.F_NEE_SKY, 4, 2)
        assert e.value.code == L.E_STATE
        ctx.build_accel()
        assert np.array_equal(bits(frame(pt, L.F_NEE_SKY, 4, 2)), bits(before))
        # a refit keeps the table
        ctx.update_vertices(mesh.vertices, 0)
        ctx.refit_accel()
        assert np.array_equal(bits(frame(pt, L.F_NEE_SKY, 4, 2)), bits(before))
        # the vertices' RNG indices may not reach the glass draws'
        with pytest.raises(L.Rt3Error) as e:
            frame(pt, L.F_NEE_SKY, (1 << 21) + 1, 64)
        assert e.value.code == L.E_INVALID and "2^30" in str(e.value)
        # without a lens the first vertex would come from the G-buffer, which has no room for a material class
        pt.set_lens(None)
        for adaptive in (None, True):
            with pytest.raises(L.Rt3Error) as e:
                pt.render(pt.make_gconst(camera(GW.CAMERA, GW.WINDOW), 4, 2, flags=L.F_NEE_SKY), adaptive=adaptive)
            assert e.value.code == L.E_STATE, adaptive
            if adaptive is None:
                assert "rt3_camera_set_lens" in str(e.value)
        # the G-buffer pass, which ran ahead of the refused one, sees the pane as the opaque surface its material describes
        assert (pt.gbuffer()[1][GW.inside(GW.PANE_COLS, GW.PANE_ROWS)] != L.BACKGROUND_DEPTH).all()
        # n = 0: no glass; rt3_scene_set_geometry resets the table too
        ctx.set_transmission([])
        ctx.build_accel()
        opaque = frame(pt, L.F_NEE_SKY, 4, 2)  # (no lens, no glass: the G-buffer's first vertex)
        ctx.set_transmission(mesh.transmission)
        ctx.upload_mesh(assets.Mesh(mesh.vertices, mesh.indices, mesh.geometries, mesh.prim_counts, list(mesh.names)))
        ctx.build_accel()
        assert np.array_equal(bits(frame(pt, L.F_NEE_SKY, 4, 2)), bits(opaque))
    finally:
        pt.close()


def lens_state(pt):
    p, on = pt.ctx.get_lens()
    return (p.aperture_radius, p.focus_distance, p.pixel_jitter, on)


def test_set_scene_switches_the_pinhole_on_for_glass():
    from raytracer3_amd.renderer import PathTracer

    glassy, plain = GW.pane_world(), GW.slab_world(emitter_edge_px=EDGE_PX, with_slab=False)[0]
    pt = PathTracer(GW.WINDOW)
    try:
        pt.set_scene(plain)
        assert not lens_state(pt)[3]
        pt.set_scene(glassy, LW.constant_sky(GW.SKY_L))
        assert lens_state(pt) == (0.0, 1.0, 0.0, True)
        assert np.abs(frame(pt, L.F_NEE_SKY, 2, 2)[GW.inside(GW.PANE_COLS, GW.PANE_ROWS)] / SKY - 1.0).max() <= sky_bound(2)
        pt.set_scene(plain)
        assert not lens_state(pt)[3]
        pt.set_lens(0.25, 3.0, 1.0)  # a lens the caller set wins, and stays
        pt.set_scene(glassy, LW.constant_sky(GW.SKY_L))
        assert lens_state(pt) == (0.25, 3.0, 1.0, True)
        pt.set_scene(plain)
        assert lens_state(pt) == (0.25, 3.0, 1.0, True)
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 9 the ledger
# instance -> (when launch_shade picks it, a test above that launches it).  test_opaque_vertices_keep_their_bits runs all twelve; the
# second credit, where there is one, is a test with a glass vertex in view.
_SEALED = f"{HERE}::test_opaque_vertices_keep_their_bits"
LEDGER = {
    "k_shade_glass<true, false, false, false>": ("<= 256 geometries, no light table", f"{HERE}::test_thin_pane_under_a_constant_sky_is_the_sky"),
    "k_shade_glass<true, true, false, false>": ("<= 256 geometries, emitters", _SEALED),
    "k_shade_glass<true, true, false, true>": ("<= 256 geometries, emitters and punctual lights", _SEALED),
    "k_shade_glass<true, false, true, false>": ("<= 256 geometries, material textures, no light table", _SEALED),
    "k_shade_glass<true, true, true, false>": ("<= 256 geometries, material textures, emitters", _SEALED),
    "k_shade_glass<true, true, true, true>": ("<= 256 geometries, material textures, emitters and punctual lights", _SEALED),
    "k_shade_glass<false, false, false, false>": ("> 256 geometries, no light table", _SEALED),
    "k_shade_glass<false, true, false, false>": ("> 256 geometries, emitters", _SEALED),
    "k_shade_glass<false, true, false, true>": ("> 256 geometries, emitters and punctual lights", _SEALED),
    "k_shade_glass<false, false, true, false>": ("> 256 geometries, material textures, no light table", _SEALED),
    "k_shade_glass<false, true, true, false>": ("> 256 geometries, material textures, emitters", _SEALED),
    "k_shade_glass<false, true, true, true>": ("> 256 geometries, material textures, emitters and punctual lights", _SEALED),
}
WITH_GLASS_IN_VIEW = {
    "k_shade_glass<true, false, false, false>": [f"{HERE}::test_tinted_pane_mixes_sky_and_tinted_sky_by_the_thin_slab_reflectance", f"{HERE}::test_solid_slab_furnace",
                                                 f"{HERE}::test_edge_seen_through_a_slab", f"{HERE}::test_gpu_against_fixture"],
    "k_shade_glass<true, true, false, false>": [f"{HERE}::test_same_bits_for_every_batch_size_and_instance_mode"],
}


def library_instances():
    """the template instances of k_shade_glass in librt3.so's symbol table (their host stubs; names only)"""
    lib = ROOT / "raytracer3_amd" / "librt3.so"
    out = None
    for nm in ("nm", "/opt/rocm/llvm/bin/llvm-nm"):
        try:
            out = subprocess.run([nm, "-C", str(lib)], capture_output=True, text=True, check=True).stdout
            break
        except (OSError, subprocess.CalledProcessError):
            continue
    assert out is not None, "neither nm nor llvm-nm could read the library"
    return set(re.findall(r"__device_stub__(k_shade_glass<[^>]*>)\(", out))


def test_glass_instance_ledger():
    """fails when a k_shade_glass instance is added without an entry here, or an entry outlives its instance, or a credited test is gone"""
    have = library_instances()
    assert len(have) == 12, sorted(have)
    assert have == set(LEDGER), (sorted(have - set(LEDGER)), sorted(set(LEDGER) - have))
    text = (ROOT / HERE).read_text()
    for name, (conditions, credit) in LEDGER.items():
        for c in [credit] + WITH_GLASS_IN_VIEW.get(name, []):
            path, _, test = c.partition("::")
            assert conditions and path == HERE and re.search(rf"^def {re.escape(test)}\(", text, re.M), (name, c)
