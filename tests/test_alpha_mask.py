"""Alpha-masked cutout geometry on the GPU (glTF alphaMode MASK).

Masks are pinned without the oracle, through equivalences: a geometry that is transparent everywhere is the same scene as one without it, bit for
bit (hits, G-buffer, radiance with and without every estimator flag, probes, after a refit); a mask that lets everything through walks exactly
as the opaque structure does (same hits, same per-ray node and triangle counts); partial masks agree with a float64 brute force and with the
numpy fp32 restatement of the alpha test; two-level equals flattened; op 27 is the restatement bit for bit; the emitter table, the errors and
a glTF round trip."""
import math

import numpy as np
import pytest

from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from raytracer3_amd.assets import Material, MeshBuilder
from raytracer3_amd.render_graph import Context
import support
from support import bits
from test_alpha_mask_cpu import alpha_f32, tex_alpha_f32, tri_uvs

pytestmark = pytest.mark.gpu

FULL = L.F_NEE_SKY | L.F_BLUENOISE | L.F_SPECULAR | L.F_FACEFORWARD | L.F_NEE_EMISSIVE
WIN = (64, 48)


def merged(a, b, textures=None):
    """mesh a followed by the geometries of mesh b (b's vertices and indices appended: a's primitive and vertex ids stay)"""
    g = b.geometries.copy()
    g["index_offset"] += len(a.indices)
    g["vertex_offset"] += len(a.vertices)
    return assets.Mesh(np.ascontiguousarray(np.concatenate([a.vertices, b.vertices]), np.float32),
                       np.ascontiguousarray(np.concatenate([a.indices, b.indices]), np.uint32), np.concatenate([a.geometries, g]),
                       np.concatenate([a.prim_counts, b.prim_counts]).astype(np.uint32), a.names + b.names,
                       list(a.textures if textures is None else textures), np.concatenate([a.alpha_cutoffs, b.alpha_cutoffs]))


def panel(tex_index, cutoff, alpha=1.0):
    """a tilted 3 x 3 panel across the Cornell box, in front of both blocks"""
    mb = MeshBuilder()
    mb.add("mask", *scenes._grid([-0.9, 0.1, 0.2], [1.7, 0.1, 0.3], [0.1, 1.6, -0.4], 3, 3),
           Material((0.9, 0.9, 0.9), texture_offset=tex_index, alpha_cutoff=cutoff, alpha=alpha))
    return mb.build()


def texture(alpha_byte):
    yy, xx = np.mgrid[0:16, 0:16]
    return np.ascontiguousarray(np.stack([(xx * 15).astype(np.uint8), (yy * 15).astype(np.uint8), np.full(xx.shape, 90, np.uint8),
                                          np.full(xx.shape, alpha_byte, np.uint8)], -1))


def make_pt(mesh, mode, instances=None):
    return support.tracer(mesh, WIN, sky=scenes.sky(64, 32), bluenoise=assets.load_bluenoise(), instances=instances, mode=mode)


def camera():
    return support.camera(scenes.CORNELL_CAMERA, WIN)


def rays_for(mesh, n, seed):
    """(8, n) rays: primary-like rays from the camera region and random rays from inside the box"""
    rng = np.random.default_rng(seed)
    m = n // 2
    o1 = np.array(scenes.CORNELL_CAMERA["position"]) + rng.uniform(-0.3, 0.3, (m, 3))
    d1 = np.array([0.0, 0.0, -1.0]) + rng.uniform(-0.45, 0.45, (m, 3)) * [1, 1, 0]
    o2 = rng.uniform([-0.95, 0.05, -0.95], [0.95, 1.95, 2.5], (n - m, 3))
    d2 = rng.normal(size=(n - m, 3))
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((8, n), np.float32)
    r[0:3], r[3:6], r[6], r[7] = o.T, d.T, 0.0, 1e30
    return r


def observe(pt, rays, probes=True, counts=False):
    """everything the library computes for a scene: trace_rays closest / any, G-buffer, radiance at two flag sets, the probe atlas"""
    out = {}
    ctx = pt.ctx
    if counts:
        ctx.set_option(L.OPT_COUNT_TRAVERSAL, 1)
        t, u, v, p, cn, ct, _ = ctx.trace_rays(rays, counts=True)
        out["counts"] = (cn, ct)
        _, _, _, occ, an, at, _ = ctx.trace_rays(rays, any_hit=True, counts=True)
        out["any_counts"] = (an, at)
    else:
        t, u, v, p, _ = ctx.trace_rays(rays)
        _, _, _, occ, _ = ctx.trace_rays(rays, any_hit=True)
    out["closest"], out["any"] = (bits(t), bits(u), bits(v), p), occ
    cam = camera()
    for flags in (0, FULL):
        pt.render(pt.make_gconst(cam, 16, 4, frame=3, flags=flags))
        out[f"light{flags}"] = bits(pt.light())
    gb, depth = pt.gbuffer()
    out["gbuffer"], out["depth"] = gb, bits(depth)
    if counts:
        st = ctx.stats()
        out["stats"] = (st.nodes_visited, st.tris_tested, st.shadow_nodes_visited, st.shadow_tris_tested)
        ctx.set_option(L.OPT_COUNT_TRAVERSAL, 0)
    if probes:
        g = pt.make_gconst(cam, 1, 2, frame=1, flags=L.F_PROBE_RADIANCE)
        pt.render_probes(g)
        out["atlas"] = bits(pt.rg.download(pt.handles["atlas"], (WIN[1] // 16 * 8, WIN[0] // 16 * 8, 4), np.float32))
    return out


def assert_same(a, b, keys=None):
    for k in keys or a:
        x, y = a[k], b[k]
        if isinstance(x, tuple):
            for i, (xi, yi) in enumerate(zip(x, y)):
                assert np.array_equal(xi, yi), f"{k}[{i}]: {int(np.sum(np.asarray(xi) != np.asarray(yi)))} values differ"
        else:
            assert np.array_equal(x, y), f"{k}: {int(np.sum(np.asarray(x) != np.asarray(y)))} values differ"


def shifted_vertices(mesh):
    v = mesh.vertices.copy()
    k = mesh.names.index("tall")
    g = mesh.geometries[k]
    lo = int(g["vertex_offset"])
    hi = int(mesh.geometries["vertex_offset"][k + 1])
    v[lo:hi, :3] = (v[lo:hi, :3].astype(np.float64) + [0.1, 0.05, 0.15]).astype(np.float32)
    return v, lo, hi


# ------------------------------------------------------------------------------------------------ 1. transparent == absent
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("how", ["texture", "base_alpha"])
def test_transparent_geometry_is_absent(mode, how):
    base = scenes.cornell()
    if how == "texture":
        extra, tex = panel(0, 0.5), [texture(0)]
    else:
        extra, tex = panel(-1, 0.5, alpha=0.0), []
    masked = merged(base, extra, tex)  # the masked geometry and its vertices come last: the other primitive ids are the same in both scenes
    absent = assets.Mesh(base.vertices, base.indices, base.geometries, base.prim_counts, list(base.names), tex)
    rays = rays_for(base, 100_000, seed=11 + mode)
    pa, pb = make_pt(masked, mode), make_pt(absent, mode)
    try:
        assert_same(observe(pa, rays), observe(pb, rays))
        v, lo, hi = shifted_vertices(base)
        for pt in (pa, pb):
            pt.ctx.update_vertices(v[lo:hi], lo)
            pt.ctx.refit_accel()
        assert_same(observe(pa, rays, probes=False), observe(pb, rays, probes=False))
    finally:
        pa.close()
        pb.close()


# ------------------------------------------------------------------------------------------------ 2. opaque through the mask == unmasked
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cutoff", [0.5, 1.0])
def test_opaque_mask_walks_like_unmasked(mode, cutoff):
    base = scenes.cornell()
    opaque = merged(base, panel(0, 0.0), [texture(255)])
    masked = merged(base, panel(0, cutoff), [texture(255)])
    rays = rays_for(base, 60_000, seed=21)
    pa, pb = make_pt(masked, mode), make_pt(opaque, mode)
    try:
        assert_same(observe(pa, rays, probes=False, counts=True), observe(pb, rays, probes=False, counts=True))
    finally:
        pa.close()
        pb.close()


# ------------------------------------------------------------------------------------------------ 3. partial masks against brute force
def brute_f64(mesh, rays, cut_alpha):
    """float64 closest hit over every triangle with a float64 alpha test; also which rays are disputed (a candidate in front of the hit
    within 1e-4 of its cutoff or within the barycentric edge tolerance, or two candidates at nearly the same t)"""
    tri = mesh.triangle_positions().astype(np.float64)
    uvs, geo = tri_uvs(mesh)
    cut = mesh.alpha_cutoffs.astype(np.float64)[geo]
    base_a = mesh.geometries["base_color"][:, 3].astype(np.float64)[geo]
    from test_alpha_mask_cpu import tex_alpha_f64, texture_of
    o, d = rays[0:3].T.astype(np.float64), rays[3:6].T.astype(np.float64)
    n = o.shape[0]
    best_t, best_p = np.full(n, np.inf), np.full(n, L.MISS, np.uint32)
    disputed = np.zeros(n, bool)
    near_t = np.full(n, np.inf)
    A, E1, E2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    for k in range(len(tri)):
        p = np.cross(d, E2[k])
        det = p @ E1[k]
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            s = o - A[k]
            u = (s * p).sum(1) * inv
            q = np.cross(s, E1[k])
            v = (d * q).sum(1) * inv
            t = (q @ E2[k]) * inv
        w = 1.0 - u - v
        valid = np.isfinite(t) & (t > 0.0)
        inside = valid & (u >= 0) & (v >= 0) & (w >= 0)
        edge = valid & (np.minimum(np.minimum(u, v), w) > -1e-5) & (np.minimum(np.minimum(u, v), w) < 1e-5)
        alpha = np.ones(n)
        if cut[k] > 0:
            tu = uvs[k].astype(np.float64)
            uu, vv = tu[0, 0] * w + tu[1, 0] * u + tu[2, 0] * v, tu[0, 1] * w + tu[1, 1] * u + tu[2, 1] * v
            g = geo[k]
            alpha = base_a[k] * tex_alpha_f64(texture_of(mesh, g), uu, vv)
            edge |= valid & (np.abs(alpha - cut[k]) < 1e-4) & (np.minimum(np.minimum(u, v), w) > -1e-5)
        counts = inside & ((cut[k] <= 0) | (alpha >= cut[k]))
        # candidates that matter: in front of the hit found so far (disputes are settled after the loop against the final hit)
        near_t = np.where(edge, np.minimum(near_t, t), near_t)
        close = counts & np.isfinite(best_t) & (np.abs(t - best_t) < 1e-6 * np.maximum(1.0, best_t))
        disputed |= close
        better = counts & (t < best_t)
        best_t = np.where(better, t, best_t)
        best_p = np.where(better, k, best_p).astype(np.uint32)
    disputed |= near_t <= best_t * (1 + 1e-6) + 1e-9
    return best_t, best_p, disputed


def test_partial_masks_against_brute_force():
    mesh = scenes.cutout_cornell()
    rays = rays_for(mesh, 20_000, seed=31)
    bt, bp, disputed = brute_f64(mesh, rays, None)
    for mode in (0, 1):
        ctx = Context()
        try:
            ctx.set_option(L.OPT_INSTANCE_MODE, mode)
            ctx.upload_mesh(mesh)
            ctx.build_accel()
            t, u, v, p, _ = ctx.trace_rays(rays)
            _, _, _, occ, _ = ctx.trace_rays(rays, any_hit=True)
        finally:
            ctx.close()
        hit = p != L.MISS
        assert hit.mean() > 0.9
        # every returned hit of a masked geometry passes the fp32 alpha test at its own (prim, u, v)
        uvs, geo = tri_uvs(mesh)
        cut = mesh.alpha_cutoffs[geo]
        m = hit & (cut[np.where(hit, p, 0)] > 0)
        assert m.sum() > 500, "too few rays end on masked geometry for the test to mean anything"
        a = alpha_f32(mesh, p[m], u[m], v[m])
        assert (a >= cut[p[m]]).all(), f"mode {mode}: {int((a < cut[p[m]]).sum())} hits fail their own alpha test"
        ok = ~disputed
        assert disputed.mean() < 0.01, disputed.mean()
        same = (p == bp) & (~hit | (np.abs(t.astype(np.float64) - bt) <= 1e-4 * np.maximum(1.0, bt)))
        assert same[ok].all(), f"mode {mode}: {int((~same[ok]).sum())} undisputed rays differ from the float64 brute force"
        assert np.array_equal(occ != 0, hit), f"mode {mode}: occluded != (closest t < tmax) on {int(((occ != 0) != hit).sum())} rays"


# ------------------------------------------------------------------------------------------------ 4. two-level == flattened
def test_two_level_placements_equal_flattened():
    mesh = scenes.cutout_cornell()
    k0 = mesh.names.index("lattice")
    nk = len(mesh.geometries) - k0
    inst = [(0, k0, np.eye(4))]
    rng = np.random.default_rng(41)
    for i in range(16):
        m = np.eye(4)
        a = rng.uniform(0, 2 * math.pi)
        m[:3, :3] = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]) * rng.uniform(0.3, 0.7)
        m[:3, 3] = rng.uniform([-0.6, 0.1, -0.6], [0.6, 1.2, 1.5])
        inst.append((k0, nk, m))
    rays = rays_for(mesh, 60_000, seed=43)
    res = []
    for mode in (0, 1):
        ctx = Context()
        try:
            ctx.set_option(L.OPT_INSTANCE_MODE, mode)
            ctx.upload_mesh(mesh)
            ctx.set_instances(inst)
            ctx.build_accel()
            t, u, v, p, _ = ctx.trace_rays(rays)
            _, _, _, occ, _ = ctx.trace_rays(rays, any_hit=True)
            res.append((bits(t), bits(u), bits(v), p, occ))
        finally:
            ctx.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    assert (res[0][3] != L.MISS).mean() > 0.5


# ------------------------------------------------------------------------------------------------ 5. self-test op 27
def test_selftest_tex_alpha_bit_exact():
    mesh = scenes.cutout_cornell()
    ctx = Context()
    try:
        ctx.upload_mesh(mesh)
        rng = np.random.default_rng(51)
        n = 50_000
        idx = rng.choice([-1, 0, 1, 7], n).astype(np.int32)
        u, v = rng.uniform(-2, 3, n).astype(np.float32), rng.uniform(-2, 3, n).astype(np.float32)
        u[:64], v[:64] = np.float32(0.5) / 64 * np.arange(64), 1.0  # texel centres and edges
        inp = np.stack([idx.view(np.uint32), u.view(np.uint32), v.view(np.uint32)], 1)
        out = ctx.selftest(27, inp, 1, np.float32)[:, 0]
    finally:
        ctx.close()
    want = np.ones(n, np.float32)
    for t in (0, 1):
        s = idx == t
        want[s] = tex_alpha_f32(mesh.textures[t], u[s], v[s])
    assert np.array_equal(bits(out), bits(want))


# ------------------------------------------------------------------------------------------------ 6. emitter table
@pytest.mark.parametrize("mode", [0, 1])
def test_masked_emitter_left_out_of_table(mode):
    base = scenes.cornell()
    glow = panel(-1, 0.5, alpha=0.8)
    glow.geometries["emission"][0] = (2.0, 2.0, 2.0, 0.0)
    dark = panel(-1, 0.0)
    tables = []
    for mesh in (merged(base, glow), merged(base, dark)):
        ctx = Context()
        try:
            ctx.set_option(L.OPT_INSTANCE_MODE, mode)
            ctx.upload_mesh(mesh)
            ctx.build_accel()
            tables.append((ctx.light_info(), *ctx.light_download()))
        finally:
            ctx.close()
    (na, prim_a, area_a, mass_a), (nb, prim_b, area_b, mass_b) = tables
    assert na == nb and na[0] > 0
    assert np.array_equal(prim_a, prim_b) and np.array_equal(bits(area_a), bits(area_b)) and np.array_equal(mass_a, mass_b)
    assert prim_a.max() < base.n_triangles  # only the panel's emitters


# ------------------------------------------------------------------------------------------------ 7. errors
def test_errors():
    mesh = scenes.cutout_cornell()
    ng = len(mesh.geometries)
    ctx = Context()
    try:
        ctx.upload_mesh(mesh)
        ctx.build_accel()
        rays = rays_for(mesh, 2000, seed=61)
        before = ctx.trace_rays(rays)[:4]
        lib, h = ctx.lib, ctx.h
        for bad in ([np.nan] + [0.0] * (ng - 1), [-0.1] + [0.0] * (ng - 1), [1.5] + [0.0] * (ng - 1), [0.5] * (ng - 1)):
            c = np.ascontiguousarray(bad, np.float32)
            assert lib.rt3_scene_set_alpha_cutoffs(h, c.ctypes.data, len(c)) == L.E_INVALID
        after = ctx.trace_rays(rays)[:4]  # nothing changed: the structure is still current
        for a, b in zip(before, after):
            assert np.array_equal(bits(a), bits(b))
        # changed after a build: stale until a rebuild, refit refused
        ctx.set_alpha_cutoffs(np.zeros(ng, np.float32))
        assert lib.rt3_trace_rays(h, rays.ctypes.data, rays.shape[1], 0, *(np.zeros(rays.shape[1], np.float32).ctypes.data for _ in range(3)),
                                  np.zeros(rays.shape[1], np.uint32).ctypes.data, None, None, 1, None) == L.E_STATE
        assert lib.rt3_accel_refit(h, None) == L.E_STATE
        ctx.build_accel()
        t, u, v, p, _ = ctx.trace_rays(rays)
        ctx.set_alpha_cutoffs(mesh.alpha_cutoffs)
        ctx.build_accel()
        # import with masks: unsupported
        nodes = np.zeros((1, 16), np.uint32)
        tris = np.zeros((1, 12), np.uint32)
        assert lib.rt3_accel_import(h, nodes.ctypes.data, nodes.nbytes, tris.ctypes.data, tris.nbytes) == L.E_UNSUPPORTED
        # non-default layouts with a cutoff: unsupported at build
        for opt, val in ((L.OPT_NODE_WIDTH, 2), (L.OPT_NODE_QUANT, 0), (L.OPT_NODE_QUANT, 2)):
            ctx.set_option(opt, val)
            assert lib.rt3_accel_build(h, None) == L.E_UNSUPPORTED
            ctx.set_option(L.OPT_NODE_WIDTH, 4)
            ctx.set_option(L.OPT_NODE_QUANT, 1)
        ctx.build_accel()
    finally:
        ctx.close()


def test_pass_launch_stale_after_cutoff_change():
    mesh = scenes.cutout_cornell()
    pt = make_pt(mesh, 0)
    try:
        cam = camera()
        pt.render(pt.make_gconst(cam, 1, 2))
        pt.ctx.set_alpha_cutoffs(mesh.alpha_cutoffs)
        with pytest.raises(L.Rt3Error):
            pt.render(pt.make_gconst(cam, 1, 2))
        pt.ctx.build_accel()
        pt.render(pt.make_gconst(cam, 1, 2))
    finally:
        pt.close()


# ------------------------------------------------------------------------------------------------ 8. end to end through glTF
@pytest.mark.parametrize("mode", [0, 1])
def test_gltf_scene_renders_like_direct_upload(tmp_path, mode):
    mesh = scenes.cutout_cornell()
    p = tmp_path / "cut.glb"
    assets.write_glb(p, mesh)
    back = assets.load(p)
    out = []
    for m in (mesh, back):
        pt = make_pt(m, mode)
        try:
            pt.render(pt.make_gconst(camera(), 8, 3, frame=2, flags=FULL))
            out.append(bits(pt.light()))
        finally:
            pt.close()
    assert np.array_equal(out[0], out[1])
    # the masks do something: the opaque scene renders differently
    pt = make_pt(assets.Mesh(mesh.vertices, mesh.indices, mesh.geometries, mesh.prim_counts, list(mesh.names), list(mesh.textures)), mode)
    try:
        pt.render(pt.make_gconst(camera(), 8, 3, frame=2, flags=FULL))
        assert not np.array_equal(bits(pt.light()), out[0])
    finally:
        pt.close()
