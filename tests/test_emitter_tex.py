"""Textured emitters ON the GPU (rt3_scene_set_textured_emitters): light sampling for geometry whose emission is a
factor times an emissive texture.  The pins: bit-exact no-ops, a constant map against the folded factor, the light side's lookup against
the hit side's (self-test ops 42 and 29), k_emit_tex against its float32 restatement (op 43), k_emit_tex_power against float64 inside a
derived bound and against its float32 restatement (op 44), a closed form under a striped light, the same expectation and a lower variance
than BSDF sampling alone on scenes.neon_room(), invariances, and refusals."""
import dataclasses
import math

import numpy as np
import pytest

import emitter_tex_worlds as EW
import ref_emitter_tex as R
import surface_worlds as SW
from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from raytracer3_amd.render_graph import Context
from raytracer3_amd.renderer import Camera
from support import bits, camera, tracer
from test_nee_emissive import FULL, block_z, frame, owned_mask, primary_points
from test_nee_emissive_cpu import CDF_TOTAL, masses

pytestmark = pytest.mark.gpu

F = np.float32
E = L.F_NEE_EMISSIVE
P = L.F_NEE_PUNCTUAL
WIN = (64, 48)


def make_pt(mesh, window=WIN, on=False, **kw):
    pt = tracer(mesh, window, bluenoise=assets.load_bluenoise(), **kw)
    pt.set_textured_emitters(on)
    return pt


def context(mesh, instances=None, mode=0, on=True):
    ctx = Context(0)
    ctx.set_option(L.OPT_INSTANCE_MODE, mode)
    ctx.upload_mesh(mesh)
    if instances:
        ctx.set_instances(instances)
    ctx.build_accel()
    ctx.set_textured_emitters(on)
    return ctx


def table_words(ctx, flags=E):
    rec, cdf, guide, prim, area, cells, shift = ctx.light_table(flags)
    return [bits(rec), cdf, guide, prim, bits(area), np.array([cells, shift])]


def same_table(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------- 1. no-ops
def unuploaded_cornell():
    """the panel names emissive texture 3 and no texture is uploaded: the hit side reads the factor"""
    return EW.with_emissive_texture(scenes.cornell(), "panel", [], index=3)


@pytest.mark.parametrize("name", ("cornell", "unuploaded"))
def test_mode_without_textured_emitter_changes_nothing(name):
    mesh = scenes.cornell() if name == "cornell" else unuploaded_cornell()
    pt = make_pt(mesh)
    try:
        cam = camera(scenes.CORNELL_CAMERA, WIN)
        got = []
        for on in (False, True):
            pt.set_textured_emitters(on)
            assert pt.ctx.get_textured_emitters() is on
            pt.ctx.stats_reset()
            img = frame(pt, cam, FULL | E, 64, 4, index=3)
            st = pt.ctx.stats()
            got.append((table_words(pt.ctx), img, (st.shadow_rays, st.extension_rays), st.emit_tex_launches, pt.ctx.light_emit_tex(E)))
    finally:
        pt.close()
    (t0, f0, r0, l0, s0), (t1, f1, r1, l1, s1) = got
    assert same_table(t0, t1) and np.array_equal(bits(f0), bits(f1)) and r0 == r1
    assert l0 == 0 and l1 == 0, "no k_emit_tex launch"
    assert len(s0[1]) == 0 and len(s1[1]) == 0, "no side array"
    assert f0.mean() > 0 and (len(t0[1]) > 0) == (name == "cornell")


# ---------------------------------------------------------------------------------------------------------------- 2. constant map
@pytest.fixture(scope="module")
def plain_cornell():
    """per instance mode: (table, {B: the FULL | E frame}) of scenes.cornell(), computed once and never modified"""
    out = {}
    cam = camera(scenes.CORNELL_CAMERA, WIN)
    for mode in (0, 1):
        pt = make_pt(scenes.cornell(), mode=mode)
        try:
            out[mode] = (table_words(pt.ctx), {B: frame(pt, cam, FULL | E, 16, B, index=5) for B in (1, 2, 4)})
        finally:
            pt.close()
    return out


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("size", (0, 1), ids=("1x1", "4x4"))
def test_constant_map_equals_the_folded_factor(plain_cornell, size, mode):
    want_table, want = plain_cornell[mode]
    pt = make_pt(EW.lit_cornell(EW.constant_maps()[size]), on=True, mode=mode)
    try:
        cam = camera(scenes.CORNELL_CAMERA, WIN)
        assert same_table(table_words(pt.ctx), want_table), "records, CDF, guide, prims and areas"
        uv, tex = pt.ctx.light_emit_tex(E)
        assert (tex == 0).all() and len(tex) == len(want_table[1])
        assert np.array_equal(pt.ctx.selftest_emit_mean(E), np.ones((len(tex), 3), F))
        for B in (1, 2, 4):
            pt.ctx.stats_reset()
            got = frame(pt, cam, FULL | E, 16, B, index=5)
            assert np.array_equal(bits(got), bits(want[B])), B
            assert pt.ctx.stats().emit_tex_launches == B - 1  # one per vertex that samples an emitter
        pt.set_textured_emitters(False)
        off = frame(pt, cam, FULL | E, 16, 4, index=5)
        assert len(pt.ctx.light_table(E)[1]) == 0  # the panel is left out again
    finally:
        pt.close()
    assert not np.array_equal(bits(off), bits(want[4])), "the mode really samples the textured panel"


# ---------------------------------------------------------------------------------------------------------------- 3. light side = hit side
def bary_grid():
    """(b1, b2): corners, edge points and interior points"""
    pts = [(0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5), (0.25, 0.75), (1 / 3, 1 / 3), (0.1, 0.2), (0.7, 0.05), (0.01, 0.98), (0.6, 0.3)]
    a = np.array(pts, F)
    return a[:, 0], a[:, 1]


@pytest.fixture(scope="module")
def soup_world():
    return EW.soup()


@pytest.mark.parametrize("mode", (0, 1))
def test_light_side_lookup_equals_hit_side(soup_world, mode):
    mesh, inst = soup_world
    ctx = context(mesh, inst, mode)
    try:
        rec, cdf, guide, prim, area, _, _ = ctx.light_table(E)
        uv, tex = ctx.light_emit_tex(E)
        b1, b2 = bary_grid()
        n, k = len(prim), len(b1)
        e = np.repeat(np.arange(n), k)
        B1, B2 = np.tile(b1, n), np.tile(b2, n)
        light = ctx.selftest_emit_radiance(E, e, B1, B2)
        hit = ctx.selftest(L.SELFTEST_HIT_INFO, SW.hit_rows(prim[e], B1, B2), 11)[:, 3:6]
    finally:
        ctx.close()
    want_uv, want_tex = EW.expected_side_array(mesh, inst, prim)
    g, _, _ = EW.entries(mesh, inst, prim)
    names = {mesh.names[x] for x in g}
    assert names == {"tex8", "tex53", "plain", "missing", "ladder"}, "the masked and the dark geometry stay out"
    assert np.array_equal(tex, want_tex) and np.array_equal(bits(uv), bits(want_uv)), "vertex order and texture index"
    assert (tex == 0).any() and (tex == 1).any() and (tex == -1).any()
    assert np.array_equal(bits(light), hit), "op 42 equals op 29's emissive bit for bit"
    # and both equal the float32 restatement
    le = rec[:, [7, 11, 15]]
    for i in np.flatnonzero(tex >= 0)[::5]:
        assert np.array_equal(bits(light[i * k:(i + 1) * k]), bits(R.radiance32(le[i], uv[i], mesh.textures[tex[i]], b1, b2))), i
    plain = np.flatnonzero(tex < 0)
    assert np.array_equal(bits(light.reshape(n, k, 3)[plain]), bits(np.repeat(le[plain, None, :], k, 1)))
    # the lookup varies from point to point (the three instances share their triangles' uvs, and so their texels)
    assert len(np.unique(bits(light[np.repeat(tex >= 0, k)]), axis=0)) > 0.9 * k * (tex >= 0).sum() / len(inst)


# ---------------------------------------------------------------------------------------------------------------- 4. the queue kernel
def queue_records(rng, n, npix, nsb):
    rec = np.zeros((n, 4), np.uint32)
    rec[:, :3] = rng.uniform(0.0, 4.0, (n, 3)).astype(F).view(np.uint32)
    rec[:, 3] = rng.integers(0, npix * nsb, n)
    if n > 2:
        rec[1, :3] = F([0.0, np.inf, -1.5]).view(np.uint32)
    return rec


@pytest.mark.parametrize("flags", (E, E | P), ids=("emitters", "with a punctual light"))
def test_queue_kernel_equals_its_float32_restatement(soup_world, flags):
    mesh, inst = soup_world
    rng = np.random.default_rng(77)
    ys, xs = np.mgrid[0:48:3, 0:64:5]  # a pixel list with gaps
    pixels = (xs.ravel() | (ys.ravel() << 16)).astype(np.uint32)
    npix, nsb = len(pixels), 4
    ctx = context(mesh, inst)
    try:
        if flags & P:
            ctx.set_lights(assets.lights_array([assets.make_light(L.LIGHT_POINT, (40.0, 30.0, 20.0), position=(0.0, 3.0, 0.0))]))
        _, cdf, _, prim, _, _, _ = ctx.light_table(flags)
        uv, tex = ctx.light_emit_tex(flags)
        seen = np.zeros(len(cdf), bool)
        # lengths: empty, one, around a wave, past one workgroup (256 threads), and past grid x block (2 x 256) with 2 workgroups
        for n, groups, dims, s0, count in ((0, 1, 8, 0, None), (1, 1, 8, 5, None), (63, 1, 8, 5, None), (64, 1, 2, 5, None), (65, 3, 8, 0, 40),
                                           (257, 4, 8, 9, None), (517, 2, 8, 5, None), (517, 2, 2, 1, 300)):
            rec = queue_records(rng, n, npix, nsb)
            got = ctx.selftest_emit_tex_queue(flags, 11, 4, 1, s0, dims, pixels, rec, groups, count)
            want, e = R.queue32(cdf, uv, tex, mesh.textures, 11, 4, 1, s0, dims, pixels, rec, count)
            assert np.array_equal(got, want), (n, groups, dims, s0, count)
            c = n if count is None else count
            assert np.array_equal(got[c:], rec[c:, :3]), "slots behind the count"
            keep = tex[e] < 0
            assert np.array_equal(got[:c][keep], rec[:c, :3][keep]), "rays of untextured or punctual picks"
            seen[e] = True
    finally:
        ctx.close()
    assert (tex[seen] >= 0).any() and (tex[seen] < 0).any()
    if flags & P:
        assert prim[-1] == L.MISS and tex[-1] == -1 and seen[-1], "the punctual light was picked, and left alone"


# ---------------------------------------------------------------------------------------------------------------- 5. masses
def moved_soup(mesh):
    v = mesh.vertices.copy()
    v[:, :3] = (v[:, :3].astype(np.float64) * [1.25, 0.75, 1.5] + [0.0, 0.125, 0.0]).astype(F)
    return v


def world_areas(mesh, inst, prim):
    _, k, idx = EW.entries(mesh, inst, prim)
    m = np.array([np.asarray(inst[i][2], np.float64) for i in k])
    p = np.einsum("nij,nvj->nvi", m[:, :3, :3], mesh.vertices[idx][:, :, :3].astype(np.float64)) + m[:, None, :3, 3]
    return 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)


def test_masses_against_float64_and_bit_equal_everywhere(soup_world):
    mesh, inst = soup_world
    runs = []
    for mode in (0, 1, 0):
        ctx = context(mesh, inst, mode)
        try:
            runs.append((table_words(ctx), bits(ctx.selftest_emit_mean(E)), ctx.light_masses(E)[2]))
            if len(runs) == 1:
                rec, _, _, prim, area, _, _ = ctx.light_table(E)
                uv, tex = ctx.light_emit_tex(E)
                mean = ctx.selftest_emit_mean(E)
        finally:
            ctx.close()
    for r in runs[1:]:
        assert same_table(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1]), "two runs and both instance modes: the same bits"
    # refit against a fresh build
    moved = moved_soup(mesh)
    for mode in (0, 1):
        ctx, fresh = context(mesh, inst, mode), context(with_moved(mesh, moved), inst, mode)
        try:
            ctx.update_vertices(moved)
            ctx.refit_accel()
            a, b = (table_words(ctx), bits(ctx.selftest_emit_mean(E))), (table_words(fresh), bits(fresh.selftest_emit_mean(E)))
        finally:
            ctx.close()
            fresh.close()
        assert same_table(a[0], b[0]) and np.array_equal(a[1], b[1]), mode
        assert not same_table(a[0], runs[0][0])
    # the mean: bit for bit the float32 restatement, and inside the derived bound of float64
    worst, Ls = 0.0, []
    mean64 = np.ones((len(tex), 3))
    for i in np.flatnonzero(tex >= 0):
        t = mesh.textures[tex[i]]
        (m32, Lq), (m64, _) = R.mean32(uv[i], t), R.mean64(uv[i], t)
        assert np.array_equal(bits(mean[i]), bits(m32)), (i, Lq)
        bound = R.mean_bound(Lq, float(np.abs(uv[i]).max()), max(t.shape[:2]))
        err = float(np.abs(mean[i].astype(np.float64) - m64).max())
        worst = max(worst, err / bound)
        assert err <= bound, (i, Lq, err, bound)
        mean64[i] = m64
        Ls.append(Lq)
    print(f"mean texel: worst error / bound {worst:.3f} over {len(Ls)} textured emitters, L from {min(Ls)} to {max(Ls)}; bound at L = 64: {R.mean_bound(64, 13.0, 8):.3e}")
    assert np.array_equal(mean[tex < 0], np.ones(((tex < 0).sum(), 3), F))
    g, _, _ = EW.entries(mesh, inst, prim)
    lad = np.flatnonzero((np.array(mesh.names)[g] == "ladder"))[:len(EW.LADDER_L)]
    assert [R.subdiv(uv[i], 8, 8) for i in lad] == list(EW.LADDER_L), "L = 1, 2, 63, 64 and the cap"
    # CDF units against the float64 table, test_table_matches_numpy_in_both_modes' allowance
    ref_area = world_areas(mesh, inst, prim)
    assert np.all(np.abs(area.astype(np.float64) / ref_area - 1.0) < 1e-5)
    le = rec[:, [7, 11, 15]].astype(np.float64)
    share = masses(ref_area * np.maximum((le * mean64) @ np.array(R.LUM), 0.0)).astype(np.float64)
    mass = runs[0][2].astype(np.float64)
    assert int(mass.sum()) == CDF_TOTAL
    assert np.all(np.abs(mass - share) <= 3.0 + 2e-5 * share), np.abs(mass - share).max()
    flat = masses(ref_area * np.maximum(le @ np.array(R.LUM), 0.0)).astype(np.float64)
    assert np.abs(mass - flat).max() > 1000, "the texture really steers the masses"


def with_moved(mesh, v):
    return dataclasses.replace(mesh, vertices=np.ascontiguousarray(v, F))


# ---------------------------------------------------------------------------------------------------------------- 6. closed form
def striped_integral(p, n):
    """the midpoint rule on an n x n grid over the unit square light at height 1, float64, for the floor points p (m, 3): the mean of
    profile cos cos' / (pi r^2) with cos = cos' = 1 / r (the light's area is 1).  128 points at a time: the grids are large."""
    c = (np.arange(n) + 0.5) / n - 0.5
    x, z = np.meshgrid(c, c, indexing="xy")
    prof = EW.profile(x + 0.5) / np.pi
    out = np.empty(len(p))
    for k in range(0, len(p), 128):
        q = p[k:k + 128]
        r2 = (x[None] - q[:, 0, None, None]) ** 2 + 1.0 + (z[None] - q[:, 2, None, None]) ** 2
        out[k:k + 128] = (prof[None] / (r2 * r2)).mean((1, 2))
    return out


def striped_want(p):
    """albedo x 12 e x the integral of profile cos cos' / (pi r^2) over the light by the midpoint rule in float64.  The grid is refined
    (doubled from 64) until the integral moves by less than 1e-5, relative, at every 8th floor point -- near and far ones, under the light
    and beside it -- and the last grid is then used for all of them."""
    probe, n = p[::8], 64
    prev = striped_integral(probe, n)
    while True:
        n *= 2
        assert n <= 2048
        val = striped_integral(probe, n)
        moved = np.abs(val / prev - 1.0).max()
        prev = val
        if moved < 1e-5:
            break
    print(f"midpoint rule: {n} x {n} cells, last refinement moved the integral by {moved:.2e}")
    return EW.ALBEDO * 12.0 * EW.EMISSION * striped_integral(p, n)


STRIPED_MEAN, STRIPED_WORST = 3e-3, 0.113


def test_floor_under_striped_light():
    """test_floor_under_square_light's floor, camera, 1024 spp and B = 2, the light carrying the 2 x 1 [255, 0] texture.  The mean threshold
    is that test's, 3e-3.  Its worst-pixel threshold, 0.08, is widened to 0.113 by the variance the stripe adds, inside what the mode-off
    frame of this scene (BSDF sampling alone, the estimator that was there before) shows a correct estimator needs here:
    a sample's value is proportional to the profile p at the sampled point, and int p^2 / (int p)^2 = (1/3) / (1/4) = 4/3, so where the
    uniform light's samples have relative deviation c, these have s^2 = (4/3) (c^2 + 1) - 1.  The worst of 3072 pixels' errors lies near
    3.6 deviations of a pixel's mean; 0.08 at 1024 spp therefore allows c = 0.08 x 32 / 3.6 = 0.71, which gives s = 1.00 and the
    threshold 0.08 x 1.00 / 0.71 = 0.113.
    Observed on an MI355X: mode on, mean +1.47e-04 and worst pixel 9.84e-02; mode off, mean -9.69e-04 and worst pixel 1.78 (DESIGN.md
    section 7)."""
    mesh = EW.floor_and_striped_light()
    pt = make_pt(mesh)
    try:
        cam = Camera((0.0, 0.9, 2.5), (0.0, -0.9, -2.5), math.radians(30.0), WIN[0] / WIN[1])
        g = pt.make_gconst(cam, 1024, 2, frame=3, flags=E | L.F_FACEFORWARD)
        out = {}
        for on in (False, True):
            pt.set_textured_emitters(on)
            pt.render(g)
            out[on] = pt.light()[..., :3].astype(np.float64)
        depth = pt.gbuffer()[1]
    finally:
        pt.close()
    hit = depth != L.BACKGROUND_DEPTH
    p = primary_points(g, depth)[hit]
    assert hit.sum() > 0.5 * hit.size and np.all(np.abs(p[:, 1]) < 1e-3), "every visible pixel is floor"
    want = striped_want(p)
    rel = {on: out[on][hit] / want[:, None] - 1.0 for on in out}
    for on in (False, True):
        print(f"textured emitters {'on' if on else 'off'}: mean relative error {rel[on].mean():+.2e}, worst pixel {np.abs(rel[on]).max():.2e}")
    assert abs(rel[True].mean()) < STRIPED_MEAN and abs(rel[False].mean()) < STRIPED_MEAN
    assert np.abs(rel[True]).max() < STRIPED_WORST < np.abs(rel[False]).max()


# ---------------------------------------------------------------------------------------------------------------- 7. neon_room
NEON_FLAGS = FULL | E
MIN_NEON_GAIN = 3.27  # RMSE(off) / RMSE(on) at 64 spp: 5.55 measured on an MI355X, asserted with half the gain (4.55 / 2) as margin


def neon_frames(pt, on, spp, indices):
    pt.set_textured_emitters(on)
    cam = camera(scenes.NEON_ROOM_CAMERA, WIN)
    return np.stack([frame(pt, cam, NEON_FLAGS, spp, 4, index=k) for k in indices]).astype(np.float64)


def test_neon_room_same_expectation_and_lower_variance():
    """test_same_expectation's protocol (K = 16 frames, 16 x 16 blocks, |z| < 4.5, a 3 % error must be visible) at 64 x 48 with 2048 spp:
    BSDF sampling alone is so noisy here that fewer samples could not see 3 %.  Then test_variance_is_lower's: RMSE at 64 spp against the
    16 384-spp mean of mode-off frames."""
    pt = make_pt(scenes.neon_room())
    try:
        K = 16
        on, off = neon_frames(pt, True, 2048, range(K)), neon_frames(pt, False, 2048, range(K))
        ref = neon_frames(pt, False, 512, range(1000, 1032)).mean(0)
        on64, off64 = neon_frames(pt, True, 64, [7])[0], neon_frames(pt, False, 64, [7])[0]
    finally:
        pt.close()
    z, z_scaled = block_z(on, off), block_z(on * 1.03, off)
    power = float(np.mean(np.abs(z_scaled) > 4.5))
    print(f"neon_room: max |z| {np.abs(z).max():.2f} over {z.size} block-channels; a 3 % error is rejected in {100 * power:.1f} % of them")
    assert on.mean() > 0 and np.abs(z).max() < 4.5
    assert np.abs(z_scaled).max() > 4.5, "the statistic must be able to see a 3 % bias"
    r_on, r_off = float(np.sqrt(np.mean((on64 - ref) ** 2))), float(np.sqrt(np.mean((off64 - ref) ** 2)))
    print(f"neon_room: RMSE at 64 spp against 16 384 spp (mode off): off {r_off:.4e}, on {r_on:.4e}, ratio {r_off / r_on:.2f}")
    assert r_on < r_off and r_off / r_on >= MIN_NEON_GAIN


# ---------------------------------------------------------------------------------------------------------------- 8. invariances
def test_batch_size_instance_mode_and_tile_partition_keep_the_bits():
    """(the stitch needs more than one 64 x 64 tile: 130 x 70 is six, still a frame of a few milliseconds)"""
    mesh = scenes.neon_room()
    cam = camera(scenes.NEON_ROOM_CAMERA, WIN)
    shots = {}
    for key, kw in (("whole", {}), ("batch 1", dict(options=[(L.OPT_BATCH_SPP, 1)])), ("mode 1", dict(mode=1))):
        pt = make_pt(mesh, on=True, **kw)
        try:
            pt.ctx.stats_reset()
            shots[key] = frame(pt, cam, NEON_FLAGS, 8, 4, index=2)
            shots[key + " launches"] = pt.ctx.stats().emit_tex_launches
        finally:
            pt.close()
    assert shots["whole"].mean() > 0 and shots["whole launches"] == 3 and shots["batch 1 launches"] == 24
    assert np.array_equal(bits(shots["batch 1"]), bits(shots["whole"])) and np.array_equal(bits(shots["mode 1"]), bits(shots["whole"]))
    big = (130, 70)
    cam = camera(scenes.NEON_ROOM_CAMERA, big)
    pt = make_pt(mesh, big, on=True)
    try:
        whole = frame(pt, cam, NEON_FLAGS, 8, 4, index=2)
    finally:
        pt.close()
    stitched = np.zeros_like(whole)
    for r in range(3):
        pt = make_pt(mesh, big, on=True, rank=r, n_ranks=3)
        try:
            part = frame(pt, cam, NEON_FLAGS, 8, 4, index=2)
        finally:
            pt.close()
        m = owned_mask(big[0], big[1], r, 3)
        stitched[m] = part[m]
    assert np.array_equal(bits(stitched), bits(whole))


def lamp_lit(mesh):
    """`mesh` (a Cornell box) with the all-255 4 x 4 map on its panel: the second path to the frame of `mesh` itself"""
    return EW.with_emissive_texture(mesh, "panel", [EW.constant_maps()[1]])


@pytest.mark.parametrize("feature", ("punctual", "panes", "roulette"))
def test_constant_map_equals_the_folded_factor_under_other_features(feature):
    """a frame that merely must equal a second path to it: with punctual lights in the union table (their picks untouched), through
    glass_cornell's pane with pane shadows, and with roulette"""
    base = scenes.glass_cornell() if feature == "panes" else scenes.cornell()
    flags = FULL | E | (P if feature == "punctual" else 0)
    got = []
    for mesh, on in ((base, False), (lamp_lit(base), True)):
        pt = make_pt(mesh, on=on)
        try:
            if feature == "punctual":
                pt.set_lights(assets.lights_array([assets.make_light(L.LIGHT_POINT, (3.0, 3.0, 2.0), position=(0.3, 1.2, 0.4)),
                                                   assets.make_light(L.LIGHT_SPOT, (9.0, 6.0, 6.0), position=(-0.5, 1.8, 0.5), direction=(0.2, -1.0, -0.1))]))
            if feature == "panes":
                pt.set_pane_shadows(True)
            if feature == "roulette":
                pt.set_roulette(1, 0.25)
            pt.ctx.stats_reset()
            img = frame(pt, camera(scenes.CORNELL_CAMERA, WIN), flags, 16, 6, index=4)
            got.append((img, pt.ctx.stats().emit_tex_launches, pt.ctx.light_masses(flags)[:2], pt.roulette_info()))
        finally:
            pt.close()
    (a, la, na, ra), (b, lb, nb, rb) = got
    assert np.array_equal(bits(a), bits(b)) and a.mean() > 0
    assert (la, lb) == (0, 5) and na == nb and ra == rb
    assert feature != "punctual" or na[1] == 2
    assert feature != "roulette" or ra[1] > 0


def test_adaptive_coverage_pixels_hold_the_fixed_frames_bits():
    """neon_room under a lens, "adaptive" in coverage mode with the mode on: a pixel that stopped at n samples holds the bits of the fixed
    n-sample frame"""
    pt = make_pt(scenes.neon_room(), on=True)
    try:
        pt.set_lens(0.02, 2.5, 1.0)
        pt.set_adaptive_coverage(True)
        cam = camera(scenes.NEON_ROOM_CAMERA, WIN)
        cap = 24
        pt.render(pt.make_gconst(cam, cap, 3, frame=6, flags=NEON_FLAGS), adaptive=L.AdaptiveParams(min_samples=4, step=4, threshold=0.5, dark=0.01, dilate=0, flags=0))
        light, n = pt.light(), pt.adaptive_moments()[..., 2].astype(np.int64)
        counts = sorted(set(n.ravel().tolist()))
        assert len(counts) > 1 and set(counts) <= set(range(4, cap + 1, 4)), counts
        for k in counts:
            pt.render(pt.make_gconst(cam, k, 3, frame=6, flags=NEON_FLAGS))
            fixed = pt.light()
            sel = n == k
            assert np.array_equal(bits(light)[sel], bits(fixed)[sel]), k
        assert pt.ctx.stats().emit_tex_launches > 0
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 9. refusals and state
def test_refusals_and_state(soup_world):
    mesh, inst = soup_world
    ctx = context(mesh, inst, on=False)
    try:
        lib, h = ctx.lib, ctx.h
        assert lib.rt3_scene_set_textured_emitters(h, 2) == L.E_INVALID and lib.rt3_scene_set_textured_emitters(h, -1) == L.E_INVALID
        assert lib.rt3_scene_set_textured_emitters(None, 1) == L.E_INVALID and lib.rt3_scene_get_textured_emitters(h, None) == L.E_INVALID
        assert ctx.get_textured_emitters() is False
        # mode off: no side array, and the ops that need one are refused
        off = table_words(ctx)
        assert len(ctx.light_emit_tex(E)[1]) == 0
        for call in (lambda: ctx.selftest_emit_mean(E), lambda: ctx.selftest_emit_radiance(E, [0], [0.1], [0.1])):
            with pytest.raises(L.Rt3Error) as err:
                call()
            assert err.value.code == L.E_STATE
        # toggling remakes the table and not the structure
        arena, info = ctx.stats().accel_arena_serial, ctx.accel_info()
        ctx.set_textured_emitters(True)
        on = table_words(ctx)
        assert not same_table(on, off) and len(on[1]) > len(off[1])
        assert ctx.stats().accel_arena_serial == arena and ctx.accel_info() == info
        ctx.trace_rays(np.zeros((8, 4), F))  # the structure is current
        n = len(on[1])
        with pytest.raises(L.Rt3Error) as err:
            ctx.selftest_emit_radiance(E, [n], [0.1], [0.1])
        assert err.value.code == L.E_INVALID
        with pytest.raises(L.Rt3Error) as err:
            ctx.selftest_emit_radiance(0, [0], [0.1], [0.1])  # no RT3_F_NEE_EMISSIVE
        assert err.value.code == L.E_INVALID
        rec = np.zeros((4, 4), np.uint32)
        for bad in (dict(bounces=0), dict(bounces=65), dict(bounce=4), dict(dims=0), dict(dims=9), dict(groups=0), dict(groups=70000), dict(count=5), dict(pixels=[])):
            kw = dict(frame=0, bounces=4, bounce=1, s0=0, dims=8, pixels=[0], records=rec, groups=1, count=None)
            kw.update(bad)
            with pytest.raises(L.Rt3Error) as err:
                ctx.selftest_emit_tex_queue(E, **kw)
            assert err.value.code == L.E_INVALID, bad
        # re-uploading a texture remakes the table: other texels, other masses
        mean = ctx.selftest_emit_mean(E)
        upload_textures(ctx, [255 - mesh.textures[0]])
        again = table_words(ctx)
        assert not np.array_equal(ctx.selftest_emit_mean(E), mean) and not np.array_equal(again[1], on[1])
        assert np.array_equal(again[3], on[3]) and ctx.stats().accel_arena_serial == arena
        ctx.set_textured_emitters(False)
        assert same_table(table_words(ctx), off)
    finally:
        ctx.close()


def upload_textures(ctx, textures):
    for i, t in enumerate(textures):
        t = np.ascontiguousarray(t, np.uint8)
        ctx.check(ctx.lib.rt3_scene_set_texture(ctx.h, i, t.ctypes.data, t.shape[1], t.shape[0]))
