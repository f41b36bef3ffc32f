"""RT3_F_NEE_EMISSIVE on the GPU: next-event estimation to emissive triangles with MIS.

The flag must estimate the same integral as the frame without it, so it is pinned without the oracle: the emitter table against numpy (in
both instance modes, after a refit), bit-exact no-op cases (no emitters, B = 1), an analytic floor under a square light, the same
expectation as the flag-less estimator on two scenes (with the power of that test shown), a variance reduction, the tile partition, refit,
statistics and error codes."""
import math

import numpy as np
import pytest

from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from raytracer3_amd.assets import Material, MeshBuilder
from raytracer3_amd.render_graph import Context
from raytracer3_amd.renderer import Camera
from support import bits, camera, tracer, translate, with_vertices
from test_nee_emissive_cpu import CDF_TOTAL, emitter_table, rect_form_factor

pytestmark = pytest.mark.gpu

E = L.F_NEE_EMISSIVE
FULL = L.F_NEE_SKY | L.F_BLUENOISE | L.F_FACEFORWARD | L.F_SPECULAR
SPEC_FF = L.F_SPECULAR | L.F_FACEFORWARD


def make_pt(mesh, window, **kw):
    return tracer(mesh, window, bluenoise=assets.load_bluenoise(), **kw)


def frame(pt, cam, flags, spp, bounces, index=0):
    pt.render(pt.make_gconst(cam, spp, bounces, frame=index, flags=flags))
    light = pt.light()[..., :3].copy()
    light[pt.gbuffer()[1] == L.BACKGROUND_DEPTH] = 0.0  # (the pass leaves background pixels untouched)
    return light


def rot(axis, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    m = np.eye(4)
    i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def without_emission(mesh):
    g = mesh.geometries.copy()
    g["emission"] = 0.0
    return assets.Mesh(mesh.vertices, mesh.indices, g, mesh.prim_counts, list(mesh.names), list(mesh.textures))


def moved_light(mesh):
    """the Cornell panel 0.3 m down and 0.2 m sideways"""
    k = mesh.names.index("panel")
    g = mesh.geometries[k]
    idx = mesh.indices[int(g["index_offset"]):int(g["index_offset"]) + 3 * int(mesh.prim_counts[k])].astype(np.int64) + int(g["vertex_offset"])
    lo, hi = int(idx.min()), int(idx.max()) + 1
    v = mesh.vertices.copy()
    v[lo:hi, :3] = (v[lo:hi, :3].astype(np.float64) + [0.2, -0.3, 0.1]).astype(np.float32)
    return v, lo, hi


def twice_lit_cornell():
    mesh = scenes.cornell()
    k = mesh.names.index("panel")
    return mesh, [(0, len(mesh.geometries), np.eye(4)), (k, 1, translate(0.3, -0.5, 0.2) @ rot("y", 25.0) @ np.diag([0.5, 1.0, 0.8, 1.0]))]


TABLE_SCENES = {
    "cornell": lambda: (scenes.cornell(), None),
    "atrium": lambda: (scenes.atrium(0.2), None),
    "cornell_ref": lambda: (scenes.cornell_ref(), None),
    "cornell_twice": twice_lit_cornell,
}


def table(ctx):
    n, total = ctx.light_info()
    prim, area, mass = ctx.light_download()
    return n, total, prim, area, mass


# ---------------------------------------------------------------------------------------------------------------- (a) table
@pytest.mark.parametrize("name", sorted(TABLE_SCENES))
def test_table_matches_numpy_in_both_modes(name):
    mesh, inst = TABLE_SCENES[name]()
    ref_prim, ref_area, ref_mass = emitter_table(mesh, inst)
    got = []
    for mode in (0, 1):
        ctx = Context()
        try:
            ctx.set_option(L.OPT_INSTANCE_MODE, mode)
            ctx.upload_mesh(mesh)
            if inst:
                ctx.set_instances(inst)
            ctx.build_accel()
            n, total, prim, area, mass = table(ctx)
        finally:
            ctx.close()
        assert n == len(ref_prim) > 0
        assert total == CDF_TOTAL and int(mass.astype(np.int64).sum()) == total
        assert np.array_equal(prim, ref_prim), "emitters are exactly the emissive flattened primitives"
        assert np.all(np.abs(area.astype(np.float64) / ref_area - 1.0) < 1e-5)
        share = ref_mass.astype(np.float64)  # the reference's masses: floor of the fp64 cumulative power on 2^23 units
        assert np.all(np.abs(mass.astype(np.float64) - share) <= 3.0 + 2e-5 * share), np.abs(mass.astype(np.float64) - share).max()
        got.append((prim, bits(area), mass))
    for a, b in zip(*got):
        assert np.array_equal(a, b), "instance modes 0 and 1 give the same table bit for bit"


@pytest.mark.parametrize("mode", (0, 1))
def test_table_after_refit_equals_fresh_build(mode):
    mesh = scenes.cornell()
    v, lo, hi = moved_light(mesh)
    ctx = Context()
    fresh = Context()
    try:
        for c, m in ((ctx, mesh), (fresh, with_vertices(mesh, v))):
            c.set_option(L.OPT_INSTANCE_MODE, mode)
            c.upload_mesh(m)
            c.build_accel()
        ctx.update_vertices(v[lo:hi], lo)
        ctx.refit_accel()
        (n, total, prim, area, mass), (n2, total2, prim2, area2, mass2) = table(ctx), table(fresh)
    finally:
        ctx.close()
        fresh.close()
    assert (n, total) == (n2, total2)
    assert np.array_equal(prim, prim2) and np.array_equal(bits(area), bits(area2)) and np.array_equal(mass, mass2)


# ---------------------------------------------------------------------------------------------------------------- (b) no-op cases
@pytest.mark.parametrize("flags", (SPEC_FF, FULL))
def test_no_emitters_is_bit_identical(flags):
    W = (96, 64)
    pt = make_pt(without_emission(scenes.atrium(0.2)), W, sky=scenes.sky(256, 128))
    try:
        cam = camera(scenes.ATRIUM_CAMERA, W)
        assert pt.ctx.light_info()[1] == 0
        a, b = frame(pt, cam, flags, 8, 4), frame(pt, cam, flags | E, 8, 4)
    finally:
        pt.close()
    assert flags & L.F_NEE_SKY == 0 or a.mean() > 0  # (without sky NEE the sky is not seen at all: a black frame)
    assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("name", ("cornell", "atrium"))
@pytest.mark.parametrize("flags", (SPEC_FF, FULL))
def test_one_bounce_is_bit_identical(name, flags):
    W = (96, 64)
    mesh, cam, sky = (scenes.cornell(), scenes.CORNELL_CAMERA, None) if name == "cornell" else (scenes.atrium(0.2), scenes.ATRIUM_CAMERA, scenes.sky(256, 128))
    pt = make_pt(mesh, W, sky=sky)
    try:
        c = camera(cam, W)
        a, b = frame(pt, c, flags, 8, 1), frame(pt, c, flags | E, 8, 1)
    finally:
        pt.close()
    assert np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------- (c) analytic
ALBEDO = 0.64  # its square root, 0.8 = 204 / 255, survives the G-buffer's 8-bit sqrt encoding exactly
EMISSION = 1.0


def floor_and_light(light_in_object_space):
    mb = MeshBuilder()
    mb.add("floor", *scenes._grid([-3, 0, -3], [0, 0, 6], [6, 0, 0], 4, 4), Material((ALBEDO,) * 3))
    if light_in_object_space:  # a unit square in the xy plane, placed by an instance matrix
        mb.add("light", *scenes._grid([-0.5, -0.5, 0], [1, 0, 0], [0, 1, 0], 1, 1), Material((0.5,) * 3, emission=(EMISSION,) * 3))
    else:
        mb.add("light", *scenes._grid([-0.5, 1, -0.5], [1, 0, 0], [0, 0, 1], 1, 1), Material((0.5,) * 3, emission=(EMISSION,) * 3))
    return mb.build()


def primary_points(g, depth):
    H, W = depth.shape
    pinv = np.array(g.proj_inverse[:], np.float64).reshape(4, 4).T
    vinv = np.array(g.view_inverse[:], np.float64).reshape(4, 4).T
    py, px = np.mgrid[0:H, 0:W]
    dx, dy = (px + 0.5) / W * 2 - 1, -((py + 0.5) / H * 2 - 1)
    t = np.stack([dx, dy, np.ones_like(dx), np.ones_like(dx)], -1) @ pinv.T
    t = t[..., :3] / np.linalg.norm(t[..., :3], axis=-1, keepdims=True)
    d = t @ vinv[:3, :3].T
    return vinv[:3, 3] + depth[..., None].astype(np.float64) * d


@pytest.mark.parametrize("placement", ("world", "instance_mode0", "instance_mode1"))
def test_floor_under_square_light(placement):
    W = (64, 48)
    obj = placement != "world"
    mesh = floor_and_light(obj)
    R = rot("y", 30.0)
    inst = [(0, 1, np.eye(4)), (1, 1, translate(0.0, 1.0, 0.0) @ R @ rot("x", 90.0))] if obj else None
    pt = make_pt(mesh, W, instances=inst, mode=1 if placement == "instance_mode1" else 0)
    try:
        cam = Camera((0.0, 0.9, 2.5), (0.0, -0.9, -2.5), math.radians(30.0), W[0] / W[1])
        g = pt.make_gconst(cam, 1024, 2, frame=3, flags=E | L.F_FACEFORWARD)
        pt.render(g)
        light = pt.light()[..., :3].astype(np.float64)
        depth = pt.gbuffer()[1]
    finally:
        pt.close()
    hit = depth != L.BACKGROUND_DEPTH
    p = primary_points(g, depth)[hit]
    assert hit.sum() > 0.5 * hit.size and np.all(np.abs(p[:, 1]) < 1e-3), "every visible pixel is floor"
    q = p @ R[:3, :3]  # into the light's frame (rotated about y)
    F = rect_form_factor(-0.5 - q[:, 0], 0.5 - q[:, 0], -0.5 - q[:, 2], 0.5 - q[:, 2], 1.0)
    want = ALBEDO * 12.0 * EMISSION * F
    got = light[hit]
    rel = got / want[:, None] - 1.0
    print(f"{placement}: mean relative error {rel.mean():+.2e}, worst pixel {np.abs(rel).max():.2e}")
    assert abs(rel.mean()) < 3e-3
    assert np.abs(rel).max() < 0.08


# ---------------------------------------------------------------------------------------------------------------- (d) same expectation
def block_z(on, off):
    """per 16 x 16 block and channel: (mean difference) / (combined standard error over the K frames)"""
    def blocks(x):  # (K, H, W, 3) -> (K, H/16, W/16, 3) block means per frame
        K, H, W, C = x.shape
        return x.reshape(K, H // 16, 16, W // 16, 16, C).mean((2, 4))
    a, b = blocks(on), blocks(off)
    K = a.shape[0]
    se = np.sqrt(a.var(0, ddof=1) / K + b.var(0, ddof=1) / K)
    d = a.mean(0) - b.mean(0)
    return np.where(se > 0, d / np.where(se > 0, se, 1.0), np.where(d == 0, 0.0, np.inf))


@pytest.mark.parametrize("name", ("cornell", "atrium"))
@pytest.mark.parametrize("flags", (L.F_FACEFORWARD, FULL))
def test_same_expectation(name, flags):
    W = (256, 256)
    mesh, cam, sky = (scenes.cornell(), scenes.CORNELL_CAMERA, None) if name == "cornell" else (scenes.atrium(0.2), scenes.ATRIUM_CAMERA, scenes.sky(256, 128))
    pt = make_pt(mesh, W, sky=sky)
    try:
        c = camera(cam, W)
        K = 16
        on = np.stack([frame(pt, c, flags | E, 256, 4, index=k) for k in range(K)]).astype(np.float64)
        off = np.stack([frame(pt, c, flags, 256, 4, index=k) for k in range(K)]).astype(np.float64)
    finally:
        pt.close()
    z = block_z(on, off)
    z_scaled = block_z(on * 1.03, off)
    power = float(np.mean(np.abs(z_scaled) > 4.5))
    print(f"{name} flags={flags}: max |z| {np.abs(z).max():.2f} over {z.size} block-channels; a 3 % error is rejected in {100 * power:.1f} % of them")
    assert np.abs(z).max() < 4.5
    assert np.abs(z_scaled).max() > 4.5, "the statistic must be able to see a 3 % bias"


# ---------------------------------------------------------------------------------------------------------------- (e) variance
@pytest.mark.parametrize("name,min_gain", (("cornell", 2.0), ("atrium", 1.0)))
def test_variance_is_lower(name, min_gain):
    W = (128, 128)
    mesh, cam, sky = (scenes.cornell(), scenes.CORNELL_CAMERA, None) if name == "cornell" else (scenes.atrium(0.2), scenes.ATRIUM_CAMERA, scenes.sky(256, 128))
    pt = make_pt(mesh, W, sky=sky)
    try:
        c = camera(cam, W)
        ref = np.mean([frame(pt, c, FULL, 512, 4, index=1000 + k) for k in range(32)], axis=0, dtype=np.float64)  # 16 384 spp
        on, off = frame(pt, c, FULL | E, 64, 4, index=7), frame(pt, c, FULL, 64, 4, index=7)
    finally:
        pt.close()
    r_on, r_off = float(np.sqrt(np.mean((on - ref) ** 2))), float(np.sqrt(np.mean((off - ref) ** 2)))
    print(f"{name}: RMSE at 64 spp against 16 384 spp: without {r_off:.4e}, with NEE_EMISSIVE {r_on:.4e}, ratio {r_off / r_on:.2f}")
    assert r_off / r_on >= min_gain if min_gain > 1.0 else r_on < r_off


# ---------------------------------------------------------------------------------------------------------------- (f) tile partition
def owned_mask(W, H, rank, n_ranks):
    """rt3_set_tile_partition's ownership: 64 x 64 tiles in Z-order over the tile grid, tile i -> rank i % n_ranks"""
    def compact(x):
        x &= 0x55555555
        x = (x | (x >> 1)) & 0x33333333
        x = (x | (x >> 2)) & 0x0F0F0F0F
        x = (x | (x >> 4)) & 0x00FF00FF
        return (x | (x >> 8)) & 0x0000FFFF
    tw, th = (W + 63) // 64, (H + 63) // 64
    side = 1
    while side < tw or side < th:
        side *= 2
    mask, no = np.zeros((H, W), bool), 0
    for z in range(side * side):
        tx, ty = compact(z), compact(z >> 1)
        if tx >= tw or ty >= th:
            continue
        if no % n_ranks == rank:
            mask[ty * 64:(ty + 1) * 64, tx * 64:(tx + 1) * 64] = True
        no += 1
    return mask


def test_tile_partition_stitches_to_one_rank():
    W = (200, 130)
    mesh = scenes.cornell()
    c = camera(scenes.CORNELL_CAMERA, W)
    pt = make_pt(mesh, W)
    try:
        whole = frame(pt, c, FULL | E, 8, 4, index=2)
    finally:
        pt.close()
    stitched = np.zeros_like(whole)
    for r in range(3):
        pt = make_pt(mesh, W, rank=r, n_ranks=3)
        try:
            part = frame(pt, c, FULL | E, 8, 4, index=2)
        finally:
            pt.close()
        m = owned_mask(W[0], W[1], r, 3)
        stitched[m] = part[m]
    assert np.array_equal(bits(stitched), bits(whole))


# ---------------------------------------------------------------------------------------------------------------- (g) refit
def test_refit_frame_equals_fresh_build():
    W = (96, 64)
    mesh = scenes.cornell()
    v, lo, hi = moved_light(mesh)
    c = camera(scenes.CORNELL_CAMERA, W)
    pt = make_pt(mesh, W)
    try:
        before = frame(pt, c, FULL | E, 16, 4, index=5)
        pt.update_vertices(v[lo:hi], lo)
        after = frame(pt, c, FULL | E, 16, 4, index=5)
    finally:
        pt.close()
    pt = make_pt(with_vertices(mesh, v), W)
    try:
        fresh = frame(pt, c, FULL | E, 16, 4, index=5)
    finally:
        pt.close()
    assert not np.array_equal(bits(before), bits(after))
    assert np.array_equal(bits(after), bits(fresh))


# ---------------------------------------------------------------------------------------------------------------- (h) stats and errors
def test_shadow_rays_counted_without_sky():
    W = (64, 48)
    pt = make_pt(scenes.cornell(), W)
    try:
        c = camera(scenes.CORNELL_CAMERA, W)
        pt.ctx.stats_reset()
        frame(pt, c, L.F_FACEFORWARD, 4, 4)
        none = pt.ctx.stats().shadow_rays
        pt.ctx.stats_reset()
        frame(pt, c, L.F_FACEFORWARD | E, 4, 4)
        some = pt.ctx.stats().shadow_rays
    finally:
        pt.close()
    assert none == 0 and some > 0


def test_light_info_state_errors():
    mesh = scenes.cornell()
    ctx = Context()
    try:
        ctx.upload_mesh(mesh)
        with pytest.raises(L.Rt3Error) as e:
            ctx.light_info()
        assert e.value.code == L.E_STATE
        ctx.build_accel()
        assert ctx.light_info() == (int(mesh.prim_counts[mesh.names.index("panel")]), CDF_TOTAL)
        v, lo, hi = moved_light(mesh)
        ctx.update_vertices(v[lo:hi], lo)
        for call in (ctx.light_info, ctx.light_download):
            with pytest.raises(L.Rt3Error) as e:
                call()
            assert e.value.code == L.E_STATE
        ctx.refit_accel()
        assert ctx.light_info()[1] == CDF_TOTAL
    finally:
        ctx.close()
