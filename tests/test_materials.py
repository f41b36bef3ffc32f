"""Material textures ON the GPU: metallic-roughness, normal and emissive maps in hit_finish.  There is no oracle
for them (the reference samples base colour only), so the pin is the float64 reference of tests/ref_materials.py within its derived
bounds (self-test op 29, both instance modes), plus bit-exact cross-checks between kernels: refit against a fresh build, the G-buffer pass
against op 29, and k_shade's material variants against scenes whose textures fold into factors, against each other across the LDS table
limit, and against the plain kernels where no hit uses a map."""
import ctypes as C
import math

import numpy as np
import pytest

import material_worlds as MW
import orc
import ref_surface as R
import surface_worlds as SW
import test_materials_cpu as M
from raytracer3_amd import _lib as L
from raytracer3_amd import assets
from raytracer3_amd.render_graph import Context
from raytracer3_amd.renderer import Camera, PathTracer
from support import bits, constant

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, BOUNCES = 64, 48, 2, 4
FLAGS = L.F_NEE_SKY | L.F_BLUENOISE | L.F_SPECULAR
world = M.world  # the module-scoped fixture: the same world, hits and float64 reference


def context(mesh, instances, mode=0):
    ctx = Context(0)
    ctx.set_option(L.OPT_INSTANCE_MODE, mode)
    ctx.upload_mesh(mesh)
    if instances:
        ctx.set_instances(instances)
    ctx.build_accel()
    return ctx


# ------------------------------------------------------------------------------------------------ 1. op 29 against float64
@pytest.fixture(scope="module")
def words(world):
    mesh, instances, hits, _ = world
    out = []
    for mode in (0, 1):
        ctx = context(mesh, instances, mode)
        try:
            out.append(ctx.selftest(L.SELFTEST_HIT_INFO, SW.hit_rows(*hits), 11))
        finally:
            ctx.close()
    return out


def test_hit_info_is_the_same_in_both_instance_modes(words):
    assert np.array_equal(words[0], words[1])


def test_hit_info_matches_float64(words, world):
    M.check_world(world)
    mesh, instances, hits, ref = world
    got = words[0].view(F)
    # normals: unit length, within the bound everywhere (the base bound where no map applies), and the map is what was applied
    nrm = got[:, 6:9].astype(np.float64)
    ln = np.linalg.norm(nrm, axis=1)
    assert np.abs(ln - 1.0).max() < 8e-7
    err = R.angle(nrm / ln[:, None], ref.normal)
    ratio = err / ref.normal_bound
    print(f"normals: worst error / bound {ratio[ref.has_n].max():.3f} mapped, {ratio[~ref.has_n].max():.3f} unmapped, {ratio[ref.no_tangent].max():.3f} without tangent")
    bad = np.flatnonzero(ratio > 1.0)
    assert bad.size == 0, (bad[:8], hits[0][bad[:8]], err[bad[:8]], ref.normal_bound[bad[:8]])
    away = R.angle(nrm / ln[:, None], ref.unmapped_normal)[ref.has_n] > ref.normal_bound[ref.has_n]
    assert away.mean() >= 0.99
    # roughness and metalness
    e_r, e_m = np.abs(got[:, 9].astype(np.float64) - ref.roughness), np.abs(got[:, 10].astype(np.float64) - ref.metalness)
    t = ref.has_mr
    print(f"roughness: worst error / bound {(e_r[t] / ref.mr_bound[t]).max():.3f}; metalness: {(e_m[t] / ref.mr_bound[t]).max():.3f}")
    assert (e_r[t] <= ref.mr_bound[t]).all() and (e_m[t] <= ref.mr_bound[t]).all() and e_r[t].max() > 0
    assert np.array_equal(got[~t, 9], ref.roughness[~t].astype(F)) and np.array_equal(got[~t, 10], ref.metalness[~t].astype(F))  # copies
    # emissive: the lookup's bound where mapped, one rounding of e * 12 elsewhere
    e_e = np.abs(got[:, 3:6].astype(np.float64) - ref.emissive).max(1)
    print(f"emissive: worst error / bound {(e_e[ref.has_e] / ref.emissive_bound[ref.has_e]).max():.3f}")
    assert (e_e <= ref.emissive_bound).all() and (ref.emissive[ref.has_e] != 0).any() and e_e[ref.has_e].max() > 0
    # albedo: ref_surface's checks, unchanged
    base = ref.base
    tx = base.textured
    assert np.array_equal(got[~tx, 0:3], base.albedo[~tx].astype(F))
    e_a = np.abs(got[tx, 0:3].astype(np.float64) - base.albedo[tx]).max(1)
    print(f"albedo: worst error / bound {(e_a / base.albedo_bound[tx]).max():.3f}")
    assert (e_a <= base.albedo_bound[tx]).all()


# ------------------------------------------------------------------------------------------------ 2. refit
def test_refit_equals_a_fresh_build(world, words):
    mesh, instances, hits, _ = world
    rows = SW.hit_rows(*hits)
    new = MW.moved(mesh)
    for mode in (0, 1):
        ctx = context(mesh, instances, mode)
        try:
            ctx.update_vertices(new)
            ctx.refit_accel()
            refitted = ctx.selftest(L.SELFTEST_HIT_INFO, rows, 11)
        finally:
            ctx.close()
        fresh_mesh = MW.with_tables(mesh)
        fresh_mesh.vertices = new
        ctx = context(fresh_mesh, instances, mode)
        try:
            fresh = ctx.selftest(L.SELFTEST_HIT_INFO, rows, 11)
        finally:
            ctx.close()
        assert np.array_equal(refitted, fresh), mode
        changed = (refitted[:, 6:9] != words[0][:, 6:9]).any(1)
        assert changed.mean() > 0.5  # the tangent and shading records really were recomputed (a corner hit on vertex 1 keeps its normal)


# ------------------------------------------------------------------------------------------------ frames
@pytest.fixture(scope="module")
def env():
    """(sky, blue noise): shared, never modified"""
    from raytracer3_amd import scenes

    return scenes.sky(128, 64), assets.load_bluenoise()


class Gpu:
    def __init__(self, mesh, instances, env, mode=0):
        self.pt = PathTracer((W, H))
        ctx = self.pt.ctx
        ctx.set_option(L.OPT_INSTANCE_MODE, mode)
        ctx.upload_mesh(mesh)
        if instances:
            ctx.set_instances(instances)
        ctx.set_sky(env[0])
        ctx.set_bluenoise(env[1])
        ctx.build_accel()

    def gconst(self, camera, flags):
        cam = Camera(camera["position"], camera["direction"], math.radians(camera["fov_deg"]), W / H)
        return self.pt.make_gconst(cam, SPP, BOUNCES, frame=1, flags=flags)

    def frame(self, camera, flags=FLAGS):
        self.pt.render(self.gconst(camera, flags))
        return (self.pt.light(), *self.pt.gbuffer())

    def close(self):
        self.pt.close()


def frame_of(mesh, camera, env, flags=FLAGS, instances=None):
    gpu = Gpu(mesh, instances, env)
    try:
        return gpu.frame(camera, flags)
    finally:
        gpu.close()


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def mapped_room(rng, emissive):
    """(mesh with constant maps, the same mesh with the maps folded into its factors, camera)"""
    mesh, cam = MW.room()
    names = mesh.names
    sizes = [(1, 1), (5, 3), (64, 2), (7, 7), (2, 9), (3, 1), (16, 16), (1, 4)]
    textures, mr = [], {}
    for k, name in enumerate(["floor", "ceiling", "back", "left", "right", "box0", "box1", "front"]):
        textures.append(constant(rng.integers(0, 256, 4), *sizes[k]))
        mr[names.index(name)] = k
    em = {}
    if emissive:
        textures += [constant((255, 255, 255, 7), 3, 3), constant((0, 0, 0, 255), 4, 2)]
        em = {names.index("panel"): len(textures) - 2, names.index("box1"): len(textures) - 1}
    mapped = MW.with_tables(mesh, material_textures=MW.table(len(names), metallic_roughness_texture=mr, emissive_texture=em), textures=textures)
    g = mesh.geometries.copy()
    inv255 = F(1.0 / 255.0)
    for gi, t in mr.items():
        px = textures[t][0, 0]
        g["roughness"][gi] = F(g["roughness"][gi]) * (F(px[1]) * inv255)
        g["metallic_factor"][gi] = F(g["metallic_factor"][gi]) * (F(px[2]) * inv255)
    if emissive:
        g["emission"][names.index("box1")] = 0.0
    folded = MW.with_tables(mesh, geometries=g, textures=textures)
    return mapped, folded, cam


@pytest.mark.parametrize("flags, emissive", [(FLAGS, True), (FLAGS | L.F_NEE_EMISSIVE, False)], ids=["folded factors", "folded factors, emitter NEE"])
def test_constant_maps_equal_folded_factors(env, flags, emissive):
    mapped, folded, cam = mapped_room(np.random.default_rng(31), emissive)
    a, b = frame_of(mapped, cam, env, flags), frame_of(folded, cam, env, flags)
    assert same(a, b), int((bits(a[0]) != bits(b[0])).any(2).sum())
    removed = MW.with_tables(mapped, material_textures=assets.no_material_textures(len(mapped.geometries)))
    c = frame_of(removed, cam, env, flags)
    assert not np.array_equal(bits(a[0]), bits(c[0])) and not np.array_equal(a[1], c[1])
    assert a[0][..., :3].mean() > 0 and np.isfinite(a[0]).all() and (a[2] != L.BACKGROUND_DEPTH).all()
    if flags & L.F_NEE_EMISSIVE:
        d = frame_of(mapped, cam, env, FLAGS)
        assert not np.array_equal(bits(a[0]), bits(d[0]))  # and emitter NEE really ran


def normal_mapped_room(rng):
    mesh, cam = MW.room()
    names = mesh.names
    textures = MW.colour_textures(rng, [(8, 8), (5, 3)]) + MW.normal_textures(rng, [(16, 16), (7, 5), (1, 1)])
    nm = {names.index("floor"): 2, names.index("back"): 3, names.index("left"): 2, names.index("box0"): 4, names.index("box1"): 3}
    mr = {names.index("floor"): 0, names.index("right"): 1}
    t = MW.table(len(names), normal_texture=nm, metallic_roughness_texture=mr, normal_scale={names.index("floor"): 1.5, names.index("back"): 0.5})
    return MW.with_tables(mesh, material_textures=t, textures=textures), cam


@pytest.mark.parametrize("flags", [FLAGS, FLAGS | L.F_NEE_EMISSIVE], ids=["plain", "emitter NEE"])
def test_normal_maps_across_the_lds_table_limit(env, flags):
    """the same triangles behind 11 and behind 300 flattened geometries: k_shade<false, true, *, true> against k_shade<false, false, *, true>"""
    mesh, cam = normal_mapped_room(np.random.default_rng(32))
    small = frame_of(mesh, cam, env, flags)
    big_mesh, inst = MW.padded(mesh, 300)
    big = frame_of(big_mesh, cam, env, flags, inst)
    assert same(small, big), int((bits(small[0]) != bits(big[0])).any(2).sum())
    t = mesh.material_textures.copy()
    t["normal_texture"] = -1
    flat = frame_of(MW.with_tables(mesh, material_textures=t), cam, env, flags)
    assert not np.array_equal(small[1], flat[1]) and not np.array_equal(bits(small[0]), bits(flat[0]))
    assert small[0][..., :3].mean() > 0 and np.isfinite(small[0]).all()


def test_unmapped_hits_are_untouched_by_the_variant(env):
    """a closed room plus one quad outside it that carries all three maps: no path can reach the quad, so the frame of the material
    variant equals the frame of the plain kernels (the table cleared), G-buffer included"""
    rng = np.random.default_rng(33)
    room, cam = MW.room()
    mb = assets.MeshBuilder()
    from raytracer3_amd import scenes

    mb.add("outside", *scenes._grid([-1, 0, 10], [2, 0, 0], [0, 2, 0], 2, 2), assets.Material((0.5, 0.5, 0.5), 1.0, 1.0, (0.0, 0.0, 0.0)))
    q = mb.build()
    g = q.geometries.copy()
    g["index_offset"] += len(room.indices)
    g["vertex_offset"] += len(room.vertices)
    n = len(room.geometries)
    mesh = assets.Mesh(np.concatenate([room.vertices, q.vertices]), np.concatenate([room.indices, q.indices]), np.concatenate([room.geometries, g]),
                       np.concatenate([room.prim_counts, q.prim_counts]).astype(np.uint32), room.names + q.names,
                       MW.colour_textures(rng, [(8, 8), (4, 4)]) + MW.normal_textures(rng, [(8, 8)]),
                       material_textures=MW.table(n + 1, metallic_roughness_texture={n: 0}, emissive_texture={n: 1}, normal_texture={n: 2}))
    with_table = frame_of(mesh, cam, env)
    cleared = frame_of(MW.with_tables(mesh, material_textures=assets.no_material_textures(n + 1)), cam, env)
    assert same(with_table, cleared)
    assert with_table[0][..., :3].mean() > 0 and (with_table[2] != L.BACKGROUND_DEPTH).all()


# ------------------------------------------------------------------------------------------------ 3. G-buffer
def test_gbuffer_pass_equals_op_29(env):
    rng = np.random.default_rng(34)
    mesh, cam = normal_mapped_room(rng)
    names = mesh.names
    mesh.textures.append(constant((255, 128, 64, 255), 2, 2))
    mesh.material_textures["emissive_texture"][names.index("panel")] = len(mesh.textures) - 1
    gpu = Gpu(mesh, None, env)
    try:
        g = gpu.gconst(cam, FLAGS)
        _, gb, depth = gpu.frame(cam, FLAGS)
        og = orc.GConst()
        C.memmove(C.byref(og), C.byref(g), 304)
        ys, xs = np.mgrid[0:H, 0:W]
        t, u, v, prim, _ = gpu.pt.ctx.trace_rays(orc.primary_rays(og, xs.ravel(), ys.ravel()))
        hit = prim != L.MISS
        assert hit.all() and np.array_equal(bits(t), bits(depth.ravel()))
        surf = gpu.pt.ctx.selftest(L.SELFTEST_HIT_INFO, SW.hit_rows(prim, u, v), 11)
        packed = gpu.pt.ctx.selftest(4, surf, 4)
    finally:
        gpu.close()
    assert np.array_equal(packed, gb.reshape(-1, 4))
    assert len(np.unique(packed[:, 1])) > 200  # normal-mapped normals: far more distinct words than the room's six directions


# ------------------------------------------------------------------------------------------------ 5. emitter table
def test_emitter_table_leaves_out_emissive_textured_geometries():
    mesh, _ = MW.room()
    names = mesh.names
    panel, box1 = names.index("panel"), names.index("box1")
    mesh = MW.with_tables(mesh, material_textures=MW.table(len(names), emissive_texture={panel: 0}), textures=[constant((200, 200, 200, 255), 2, 2)])
    first = np.concatenate([[0], np.cumsum(mesh.prim_counts)[:-1]])
    ctx = context(mesh, None)
    try:
        prim, area, mass = ctx.light_download()
        assert np.array_equal(prim, first[box1] + np.arange(mesh.prim_counts[box1]))  # box1 only: the panel is left out
        ctx.set_material_textures([])
        ctx.build_accel()
        prim2 = ctx.light_download()[0]
        assert set(prim2.tolist()) == set((first[panel] + np.arange(mesh.prim_counts[panel])).tolist()) | set(prim.tolist())
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_and_state(world):
    mesh, instances, hits, ref = world
    pick = np.arange(0, len(hits[0]), len(hits[0]) // 64)[:64]  # spread over every geometry: mapped hits among them
    assert ref.has_mr[pick].any() and ref.has_n[pick].any() and ref.has_e[pick].any()
    rows = np.ascontiguousarray(SW.hit_rows(*hits)[pick])
    n = len(mesh.geometries)
    ctx = context(mesh, instances)
    try:
        want = ctx.selftest(L.SELFTEST_HIT_INFO, rows, 11)

        def call(table):
            t = np.ascontiguousarray(table, assets.MATERIAL_TEXTURES_DTYPE)
            return ctx.lib.rt3_scene_set_material_textures(ctx.h, t.ctypes.data, len(t))

        good = mesh.material_textures
        for bad in (good[:-1], np.concatenate([good, good[:1]])):
            assert call(bad) == L.E_INVALID  # a wrong n
        for column, value in (("normal_scale", np.nan), ("normal_scale", np.inf), ("metallic_roughness_texture", -2), ("normal_texture", -7), ("emissive_texture", -2)):
            bad = good.copy()
            bad[column][n // 2] = value
            assert call(bad) == L.E_INVALID, column
        assert ctx.lib.rt3_scene_set_material_textures(ctx.h, None, n) == L.E_INVALID
        assert np.array_equal(ctx.selftest(L.SELFTEST_HIT_INFO, rows, 11), want)  # nothing changed: the structure is still usable
        # a successful call leaves the structure unusable until a rebuild
        assert call(good) == L.RT3_OK
        out = np.zeros((len(rows), 11), np.uint32)
        assert ctx.lib.rt3_selftest_eval(ctx.h, L.SELFTEST_HIT_INFO, rows.ctypes.data, len(rows), out.ctypes.data) == L.E_STATE
        with pytest.raises(RuntimeError):
            ctx.trace_rays(np.zeros((8, 4), F))
        with pytest.raises(RuntimeError):
            ctx.refit_accel()
        ctx.build_accel()
        assert np.array_equal(ctx.selftest(L.SELFTEST_HIT_INFO, rows, 11), want)
        # rt3_scene_set_geometry clears the table: the same world without it
        g, pc = np.ascontiguousarray(mesh.geometries), np.ascontiguousarray(mesh.prim_counts, np.uint32)
        ctx.check(ctx.lib.rt3_scene_set_geometry(ctx.h, g.ctypes.data, pc.ctypes.data, n))
        ctx.build_accel()
        cleared = ctx.selftest(L.SELFTEST_HIT_INFO, rows, 11)
    finally:
        ctx.close()
    plain = context(MW.with_tables(mesh, material_textures=assets.no_material_textures(n)), instances)
    try:
        assert np.array_equal(cleared, plain.selftest(L.SELFTEST_HIT_INFO, rows, 11))
    finally:
        plain.close()
    assert not np.array_equal(cleared, want)


def test_frames_pass_launch_refuses_until_rebuilt(env):
    mesh, cam = normal_mapped_room(np.random.default_rng(35))
    gpu = Gpu(mesh, None, env)
    try:
        a = gpu.frame(cam)
        gpu.pt.ctx.set_material_textures(mesh.material_textures)
        with pytest.raises(RuntimeError):
            gpu.frame(cam)
        gpu.pt.ctx.build_accel()
        assert same(a, gpu.frame(cam))
    finally:
        gpu.close()
