"""The light sampler's selection table on the GPU, bit for bit.

(a) self-test op 40 -- the table's own quantise, scan, CDF and guide kernels and light_find, on caller-made powers -- against the float64 /
integer reference of tests/ref_light_table.py, from 1 to 2^20 + 1 lights; (b) the context's own table, records included, on worlds whose
fp32 arithmetic numpy reproduces (tests/light_table_worlds.py), in both instance modes, after a refit and with punctual lights; (c) one
frame: a panel cut into 8738 triangles of very different sizes lights the floor as the panel of two does.  No comparison in (a) or (b) has
a tolerance."""
import math
import time

import numpy as np
import pytest

import light_table_worlds as lw
import ref_light_table as rl
from raytracer3_amd import _lib as L
from raytracer3_amd.render_graph import Context
from raytracer3_amd.renderer import Camera
from support import bits, translate, with_vertices
from test_nee_emissive import ALBEDO, EMISSION, floor_and_light, make_pt, primary_points, rot
from test_nee_emissive_cpu import emitter_table, rect_form_factor

pytestmark = pytest.mark.gpu

E, P = L.F_NEE_EMISSIVE, L.F_NEE_PUNCTUAL
LARGE = ("uniform_2p19_1", "uniform_2p20_1")


@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------- (a) op 40
@pytest.mark.parametrize("name", list(rl.POWER_SETS))
def test_op40_equals_the_reference(ctx, name):
    power, area = rl.power_set(name)
    t = rl.LightTable(power, area)
    k = t.boundary_keys(7) if t.total else np.zeros(0, np.uint32)
    t0 = time.perf_counter()
    cells, shift, total, cdf, w, guide, found = ctx.selftest_light_table(power, area, k)
    dt = time.perf_counter() - t0
    print(f"{name}: n {t.n}, cells {cells}, shift {shift}, {len(k)} lookups, {int((t.mass == 0).sum())} entries without mass, op 40 took {dt:.2f} s")
    assert (cells, shift, total) == (t.cells, t.shift, t.total)
    assert total == (rl.CDF_TOTAL if power.any() else 0)
    assert np.array_equal(cdf, t.cdf), f"cdf differs first at {np.flatnonzero(cdf != t.cdf)[:3]}"
    assert np.array_equal(guide, t.guide), f"guide differs first at {np.flatnonzero(guide != t.guide)[:3]}"
    assert np.array_equal(bits(w), bits(t.w)), f"p_sel / area differs first at {np.flatnonzero(bits(w) != bits(t.w))[:3]}"
    want = t.find(k)
    assert np.array_equal(found, want), f"light_find differs first at k = {k[np.flatnonzero(found != want)[:3]]}"
    if t.total:
        assert np.all(t.mass[found] > 0), "an entry without mass is never found"
    if name in LARGE:
        assert cells == 1 << 20 and cells + 1 > 4096 * 256, "the guide kernel's threads make a second trip"


def test_op40_refuses_bad_input(ctx):
    one = np.ones(4, np.float32)
    bad = [(np.zeros(0, np.float32), np.zeros(0, np.float32), ()),  # n = 0
           (np.array([1.0, -1.0, 1.0, 1.0], np.float32), one, ()),
           (np.array([1.0, np.inf, 1.0, 1.0], np.float32), one, ()),
           (np.array([1.0, np.nan, 1.0, 1.0], np.float32), one, ()),
           (one, one, (0, 1 << 23)),  # k beyond the grid
           (np.zeros(4, np.float32), one, (0,))]  # nothing to look up
    for power, area, k in bad:
        with pytest.raises(L.Rt3Error) as e:
            ctx.selftest_light_table(power, area, k)
        assert e.value.code == L.E_INVALID
    assert ctx.selftest_light_table(np.array([0.0, -0.0, 2.0], np.float32), one[:3], (0, (1 << 23) - 1))[6].tolist() == [2, 2]


# ---------------------------------------------------------------------------------------------------------------- (b) the context's table
def reference(mesh, inst, lights=None):
    """the table of a dyadic world: (prim, records with p_sel / area in place, areas, ref_light_table.LightTable)"""
    prim, rec, area, power = lw.emitter_records(mesh, inst)
    if lights is not None:
        n = len(lights)
        tail = np.zeros((n, 16), np.float32)
        prim = np.concatenate([prim, np.full(n, lw.MISS, np.uint32)])
        area = np.concatenate([area, np.ones(n, np.float32)])
        power = np.concatenate([power, lw.punctual_powers(lights, mesh)])
        rec = np.concatenate([rec, tail])
    t = rl.LightTable(power, area)
    rec[:, 3] = t.w
    return prim, rec, area, t


def built(mesh, inst, mode):
    c = Context()
    c.set_option(L.OPT_INSTANCE_MODE, mode)
    c.upload_mesh(mesh)
    if inst:
        c.set_instances(inst)
    c.build_accel()
    return c


def assert_table(got, want, n_emit=None, what=""):
    """a Context.light_table answer against reference(): every word"""
    rec, cdf, guide, prim, area, cells, shift = got
    w_prim, w_rec, w_area, t = want
    n_emit = len(w_prim) if n_emit is None else n_emit
    assert len(cdf) == t.n and (cells, shift) == (t.cells, t.shift), what
    assert np.array_equal(prim, w_prim) and np.array_equal(bits(area), bits(w_area)), what
    assert np.array_equal(cdf, t.cdf), (what, np.flatnonzero(cdf != t.cdf)[:3])
    assert np.array_equal(guide, t.guide), (what, np.flatnonzero(guide != t.guide)[:3])
    for name, cols in (("A", slice(0, 3)), ("E1", slice(4, 7)), ("E2", slice(8, 11)), ("normal", slice(12, 15)), ("Le", [7, 11, 15])):
        a, b = bits(rec[:n_emit, cols]), bits(w_rec[:n_emit, cols])
        assert np.array_equal(a, b), (what, name, np.argwhere(a != b)[:3].tolist())
    assert np.array_equal(bits(rec[:, 3]), bits(w_rec[:, 3])), (what, "p_sel / area", np.flatnonzero(bits(rec[:, 3]) != bits(w_rec[:, 3]))[:3])


def same_bits(a, b):
    return all(np.array_equal(bits(x), bits(y)) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(lw.WORLDS))
def test_world_table_equals_the_reference(name):
    mesh, inst = lw.WORLDS[name]()
    want = reference(mesh, inst)
    t = want[3]
    assert np.array_equal(want[0], emitter_table(mesh, inst)[0]), "the emitters are the emissive flattened primitives, in order"
    got = []
    for mode in (0, 1):
        c = built(mesh, inst, mode)
        try:
            got.append(c.light_table(E))
            info, (d_prim, d_area, d_mass) = c.light_info(), c.light_download()
        finally:
            c.close()
        assert_table(got[-1], want, what=f"{name}, instance mode {mode}")
        assert info == (t.n, t.total) and t.total == rl.CDF_TOTAL
        assert np.array_equal(d_prim, want[0]) and np.array_equal(bits(d_area), bits(want[2])) and np.array_equal(d_mass, t.mass)
    assert same_bits(got[0], got[1]), "instance modes 0 and 1 give the same table bit for bit"
    rec = got[0][0]
    if name == "degenerate":
        assert rec[1, 12:15].tolist() == [0.0, 0.0, 1.0] and want[2][1] == 0.0 and t.mass[1] == 0 and rec[1, 3] == 0.0
        assert t.mass[0] > 0 and t.mass[2] > 0
    if name == "overflow":  # the scene calls accept such an emission: the light has no mass
        assert np.all(np.isinf(rec[1:3, 7])) and np.all(t.mass[1:3] == 0) and np.all(rec[1:3, 3] == 0.0) and t.mass[0] > 0 and t.mass[3] > 0
    if name == "instanced":  # entry 6: the first triangle of "red" under the mirror -- its normal points the other way
        assert rec[0, 12:15].tolist() == [0.0, 0.0, 1.0] and rec[6, 12:15].tolist() == [0.0, 0.0, -1.0]
        assert rec[6, 4:7].tolist() == [-1.0, 0.0, 0.0] and rec[6, 0:3].tolist() == [0.0, 2.0, 0.0]
    if name == "areas":
        assert sorted(np.log2(want[2]).tolist()) == list(range(-12, 1))
    if name == "many":
        assert len(np.unique(mesh.prim_counts[::2])) == 3 and t.n == int(mesh.prim_counts[::2].sum()) and len(mesh.geometries) == 600


@pytest.mark.parametrize("name,geometry,triangle", (("three", 1, 1), ("instanced", 2, 0)))
def test_world_table_after_refit(name, geometry, triangle):
    mesh, inst = lw.WORLDS[name]()
    rows, first = lw.doubled(mesh, geometry, triangle)
    v = mesh.vertices.copy()
    v[first:first + 3] = rows
    moved = with_vertices(mesh, v)
    want, before = reference(moved, inst), reference(mesh, inst)
    assert not np.array_equal(want[3].cdf, before[3].cdf) and np.array_equal(want[0], before[0])
    got = []
    for mode in (0, 1):
        c, fresh = built(mesh, inst, mode), built(moved, inst, mode)
        try:
            assert_table(c.light_table(E), before, what=f"{name} before the update, mode {mode}")
            c.update_vertices(rows, first)
            c.refit_accel()
            got += [c.light_table(E), fresh.light_table(E)]
        finally:
            c.close()
            fresh.close()
        assert_table(got[-2], want, what=f"{name} after the refit, mode {mode}")
        assert same_bits(got[-2], got[-1]), "a refit leaves the fresh build's table"
    assert same_bits(got[0], got[2])


@pytest.mark.parametrize("mode", (0, 1))
def test_mixed_table_of_emitters_and_punctual_lights(mode):
    mesh = lw.mixed()
    n_e, n_p = 3, len(mesh.lights)
    want = {E: reference(mesh, None), E | P: reference(mesh, None, mesh.lights)}
    w_p = rl.LightTable(lw.punctual_powers(mesh.lights, mesh), np.ones(n_p, np.float32))
    assert w_p.mass.min() > 0 and want[E | P][3].mass.min() > 0, "every entry has a mass the grid resolves"
    c = built(mesh, None, mode)
    try:
        answers = [(f, c.light_masses(f), c.light_table(f)) for f in (E, E | P, P, E)]
        none = c.light_table(0)
    finally:
        c.close()
    assert [a[1][:2] for a in answers] == [(n_e, 0), (n_e, n_p), (0, n_p), (n_e, 0)]
    assert none[5:] == (0, 0) and all(len(x) == 0 for x in none[:5])
    for f, (_, _, mass), table in answers:
        rec, cdf, guide, prim, area, cells, shift = table
        if f == P:
            assert np.array_equal(cdf, w_p.cdf) and np.array_equal(guide, w_p.guide) and (cells, shift) == (w_p.cells, w_p.shift)
            assert np.array_equal(bits(rec[:, 3]), bits(w_p.w))
        else:
            assert_table(table, want[f], n_emit=n_e, what=f"flags {f}")
        assert np.array_equal(mass, np.diff(cdf.astype(np.int64), prepend=0))
        tail = slice(len(cdf) - (n_p if f & P else 0), len(cdf))
        if f & P:  # a punctual entry: no primitive, area 1 -- its record's word is p_sel itself -- and the light's own words
            assert np.all(prim[tail] == lw.MISS) and np.all(area[tail] == 1.0)
            assert np.array_equal(bits(rec[tail, 3]), bits((mass[tail].astype(np.float64) / rl.CDF_TOTAL).astype(np.float32)))
            assert np.array_equal(bits(rec[tail, 0:3]), bits(mesh.lights["position"])) and np.array_equal(bits(rec[tail][:, [7, 11, 15]]), bits(mesh.lights["intensity"]))
    assert same_bits(answers[0][2], answers[3][2]) and np.array_equal(answers[0][1][2], answers[3][1][2]), "E asked first and last: the same bits"


def test_light_table_state_errors():
    mesh, _ = lw.three()
    c = Context()
    try:
        c.upload_mesh(mesh)
        with pytest.raises(L.Rt3Error) as e:
            c.light_table(E)
        assert e.value.code == L.E_STATE
        c.build_accel()
        assert len(c.light_table(E)[1]) == 3
        rows, first = lw.doubled(mesh, 1, 0)
        c.update_vertices(rows, first)
        with pytest.raises(L.Rt3Error) as e:
            c.light_table(E)
        assert e.value.code == L.E_STATE
        c.refit_accel()
        assert int(c.light_table(E)[1][-1]) == rl.CDF_TOTAL
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- (c) one frame
@pytest.mark.parametrize("placement", ("world", "instance_mode0", "instance_mode1"))
def test_tessellated_panel_is_the_panel(placement):
    """test_floor_under_square_light with the light cut into 8738 triangles whose areas span 2^12: emission is uniform, so selection by
    power is uniform over the panel and the estimator's expectation and per-sample distribution are the two-triangle panel's -- the same
    closed form, the same bounds"""
    W = (64, 48)
    obj = placement != "world"
    R = rot("y", 30.0)
    place = translate(0.0, 1.0, 0.0) @ R @ rot("x", 90.0)
    cam = Camera((0.0, 0.9, 2.5), (0.0, -0.9, -2.5), math.radians(30.0), W[0] / W[1])
    result = {}
    t0 = time.perf_counter()
    for what, mesh, n_light in (("tessellated", lw.tessellated_panel(obj, ALBEDO, EMISSION), 4), ("two triangles", floor_and_light(obj), 1)):
        inst = [(0, 1, np.eye(4)), (1, n_light, place)] if obj else None
        pt = make_pt(mesh, W, instances=inst, mode=1 if placement == "instance_mode1" else 0)
        try:
            g = pt.make_gconst(cam, 1024, 2, frame=3, flags=E | L.F_FACEFORWARD)
            pt.render(g)
            light = pt.light()[..., :3].astype(np.float64)
            depth = pt.gbuffer()[1]
            if what == "tessellated":
                rec, cdf, guide, prim, area, cells, shift = pt.ctx.light_table(E)
                assert len(cdf) == 8738 and cells == 16384 and area.max() / area.min() > 4095.0
        finally:
            pt.close()
        hit = depth != L.BACKGROUND_DEPTH
        p = primary_points(g, depth)[hit]
        assert hit.sum() > 0.5 * hit.size and np.all(np.abs(p[:, 1]) < 1e-3), "every visible pixel is floor"
        q = p @ R[:3, :3]  # into the light's frame (rotated about y)
        F = rect_form_factor(-0.5 - q[:, 0], 0.5 - q[:, 0], -0.5 - q[:, 2], 0.5 - q[:, 2], 1.0)
        rel = light[hit] / (ALBEDO * 12.0 * EMISSION * F)[:, None] - 1.0
        result[what] = (rel.mean(), np.abs(rel).max())
        print(f"{placement}, {what}: mean relative error {rel.mean():+.2e}, worst pixel {np.abs(rel).max():.2e}")
    print(f"{placement}: both frames took {time.perf_counter() - t0:.2f} s")
    mean, worst = result["tessellated"]
    assert abs(mean) < 3e-3
    assert worst < 0.08
