"""Glass without a GPU: the Fresnel functions of tests/ref_glass.py against known answers, the glTF round trip of
KHR_materials_transmission / _ior / _volume through both loaders, the float64 glass tracer against closed forms on the small worlds of
tests/glass_worlds.py, and the fixture tests/golden/glass_ref.npz (size, contents, no generator drift)."""
import functools
import importlib.util
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import glass_worlds as GW
import integrator_worlds as IW
import lens_worlds as LW
import ref_glass as RG
import ref_pathtrace as RP
from raytracer3_amd import assets, scenes
from test_integrator_cpu import Z_MAX

GOLDEN = Path(__file__).resolve().parent / "golden" / "glass_ref.npz"
HOST = Path(__file__).resolve().parent.parent / "raytracer3_amd" / "host"
F_NEE_SKY = RP.F_NEE_SKY


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


# ---------------------------------------------------------------------------------------------------------------- Fresnel
def test_fresnel_at_normal_incidence():
    """((n - 1) / (n + 1))^2 = 0.04 at n = 1.5, from either side"""
    assert abs(float(RG.fresnel(1.0, 1.5)) - 0.04) < 1e-15 and abs(float(RG.fresnel(1.0, 1.0 / 1.5)) - 0.04) < 1e-15


def test_total_internal_reflection_beyond_the_critical_angle():
    crit = math.asin(1.0 / 1.5)
    th = np.array([crit + 1e-9, crit + 0.1, 1.5])
    assert np.array_equal(RG.fresnel(np.cos(th), 1.0 / 1.5), np.ones(3))
    below = RG.fresnel(np.cos(np.array([crit - 1e-6, crit - 0.1])), 1.0 / 1.5)
    assert np.all(below < 1.0) and below[0] > 0.98
    assert np.array_equal(RG.cos_transmitted(np.cos(th), 1.0 / 1.5), np.zeros(3))


def test_fresnel_is_the_same_from_both_sides_of_the_interface():
    th_i = np.linspace(0.0, 1.55, 200)
    th_t = np.arcsin(np.sin(th_i) / 1.5)
    assert np.abs(RG.fresnel(np.cos(th_i), 1.5) - RG.fresnel(np.cos(th_t), 1.0 / 1.5)).max() < 1e-13
    assert np.abs(RG.cos_transmitted(np.cos(th_i), 1.5) - np.cos(th_t)).max() < 1e-14


def test_thin_slab_reflectance_is_the_summed_series():
    """R' = F + sum over k >= 0 of (1 - F)^2 F^(2 k + 1): in at the front, an odd number of reflections inside, out at the front"""
    F = np.array([0.0, 0.04, 0.3, 0.9, 1.0 - 1e-9])
    k = np.arange(0, 200000)[:, None]
    series = F + ((1.0 - F) ** 2 * F ** (2 * k + 1)).sum(0)
    assert np.abs(RG.thin_fresnel(F) - series).max() < 1e-9
    assert float(RG.thin_fresnel(1.0)) == 1.0


def test_glass_event_directions():
    """reflection mirrors, refraction obeys Snell in the plane of incidence, thin walls pass straight through; both sides of a surface"""
    rng = np.random.default_rng(3)
    m = 2000
    d = rng.normal(size=(m, 3))
    n = rng.normal(size=(m, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    ud = d / np.linalg.norm(d, axis=1, keepdims=True)
    for thin in (False, True):
        tr, out, F = RG.glass_event(1.5, thin, d, n, np.full(m, 2.0))  # u above every F: transmit unless F = 1
        assert np.array_equal(tr, F < 2.0) and tr.all()
        tir = F >= 1.0
        assert np.abs(np.linalg.norm(out[~tir], axis=1) - 1.0).max() < 1e-12
        if thin:
            assert np.array_equal(out, ud) and not tir.any()
        else:
            c = np.sum(n * ud, -1)
            eta = np.where(c < 0, 1.5, 1 / 1.5)
            sin_i, sin_t = np.linalg.norm(np.cross(n, ud), axis=1), np.linalg.norm(np.cross(n, out), axis=1)
            assert np.abs(sin_i - eta * sin_t)[~tir].max() < 1e-12  # Snell
            assert np.all(np.sign(np.sum(n * out, -1))[~tir] == np.sign(c)[~tir])  # it goes on to the far side
            assert np.abs(np.sum(np.cross(n, ud) * out, -1))[~tir].max() < 1e-12  # and stays in the plane of incidence
            assert tir.any() and not tir[c < 0].any()
        tr, out, _ = RG.glass_event(1.5, thin, d, n, np.full(m, -1.0))  # u below every F: reflect
        assert not tr.any() and np.abs(out - (ud - 2.0 * np.sum(n * ud, -1)[:, None] * n)).max() < 1e-15


# ---------------------------------------------------------------------------------------------------------------- glTF
def glassy_mesh():
    mesh = scenes.glass_cornell()
    k = mesh.names.index("tall")
    mesh.transmission[k] = (0.25, 1.33, 0, 0)  # a partly transmissive solid with another index
    mesh.transmission[mesh.names.index("short")] = (0.0, 1.8, 1, 0)  # no glass, but an index of its own
    return mesh


def test_gltf_round_trip_keeps_the_transmission_table(tmp_path):
    import json
    import struct

    mesh = glassy_mesh()
    t = mesh.transmission
    assert t.dtype == assets.TRANSMISSION_DTYPE and (t["transmission"] == 1.0).sum() == 2 and set(t["thin_walled"]) == {0, 1}
    assets.write_glb(tmp_path / "g.glb", mesh)
    back = assets.load(tmp_path / "g.glb")
    assert back.transmission.dtype == assets.TRANSMISSION_DTYPE and back.transmission.tobytes() == t.tobytes()
    data = (tmp_path / "g.glb").read_bytes()
    doc = json.loads(data[20 : 20 + struct.unpack_from("<I", data, 12)[0]].decode())
    assert set(doc["extensionsUsed"]) == {"KHR_materials_transmission", "KHR_materials_ior", "KHR_materials_volume"}
    sphere, pane = (doc["materials"][mesh.names.index(n)]["extensions"] for n in ("glass_sphere", "glass_pane"))
    assert sphere["KHR_materials_transmission"] == {"transmissionFactor": 1.0} and sphere["KHR_materials_ior"] == {"ior": 1.5}
    assert sphere["KHR_materials_volume"] == {"thicknessFactor": 1.0} and "KHR_materials_volume" not in pane
    assert "extensions" not in doc["materials"][mesh.names.index("floor")]


def native_tool():
    subprocess.check_call(["make", "-C", str(HOST), "asset_tool"], stdout=subprocess.DEVNULL)
    return str(HOST / "asset_tool")


def test_native_loader_reads_the_same_table(tmp_path):
    mesh = glassy_mesh()
    assets.write_glb(tmp_path / "g.glb", mesh)
    subprocess.run([native_tool(), "glb", str(tmp_path / "g.glb"), str(tmp_path)], check=True, capture_output=True)
    got = np.fromfile(tmp_path / "transmission.bin", assets.TRANSMISSION_DTYPE)
    want = assets.load(tmp_path / "g.glb").transmission
    assert len(got) == len(mesh.geometries) and got.tobytes() == want.tobytes() == mesh.transmission.tobytes()


class CallLog:
    """stands in for librt3 under render_graph.Context.upload_mesh: every rt3_* call is recorded and succeeds"""

    def __init__(self):
        self.names = []

    def __getattr__(self, name):
        def call(*a):
            self.names.append(name)
            return 0
        return call


def uploaded_calls(mesh):
    from raytracer3_amd.render_graph import Context

    ctx = Context.__new__(Context)
    ctx.lib, ctx.h = CallLog(), None
    ctx.check = lambda rc: None
    Context.upload_mesh(ctx, mesh)
    return ctx.lib.names


def test_a_material_without_the_extensions_is_not_glass_and_makes_no_call(tmp_path):
    mesh = scenes.cornell()
    assets.write_glb(tmp_path / "c.glb", mesh)
    back = assets.load(tmp_path / "c.glb")
    t = back.transmission
    assert np.all(t["transmission"] == 0.0) and np.all(t["ior"] == np.float32(1.5)) and np.all(t["thin_walled"] == 1) and np.all(t["reserved"] == 0)
    assert t.tobytes() == assets.no_transmission(len(back.geometries)).tobytes()
    assert "rt3_scene_set_transmission" not in uploaded_calls(back)
    assert uploaded_calls(scenes.glass_cornell()).count("rt3_scene_set_transmission") == 1
    subprocess.run([native_tool(), "glb", str(tmp_path / "c.glb"), str(tmp_path)], check=True, capture_output=True)
    assert np.fromfile(tmp_path / "transmission.bin", assets.TRANSMISSION_DTYPE).tobytes() == t.tobytes()


def test_a_volume_without_thickness_is_thin_walled(tmp_path):
    import json
    import struct

    mesh = scenes.glass_cornell()
    assets.write_glb(tmp_path / "g.glb", mesh)
    data = (tmp_path / "g.glb").read_bytes()
    ln = struct.unpack_from("<I", data, 12)[0]
    doc = json.loads(data[20 : 20 + ln].decode())
    k = mesh.names.index("glass_sphere")
    doc["materials"][k]["extensions"]["KHR_materials_volume"]["thicknessFactor"] = 0.0
    doc["materials"][k]["extensions"]["KHR_materials_transmission"]["transmissionTexture"] = {"index": 0}  # ignored
    del doc["materials"][k]["extensions"]["KHR_materials_ior"]  # the default is 1.5
    js = json.dumps(doc, separators=(",", ":")).encode()
    js += b" " * ((-len(js)) % 4)
    rest = data[20 + ln :]
    (tmp_path / "t.glb").write_bytes(struct.pack("<4sII", b"glTF", 2, 20 + len(js) + len(rest)) + struct.pack("<I4s", len(js), b"JSON") + js + rest)
    back = assets.load(tmp_path / "t.glb")
    assert tuple(back.transmission[k]) == (1.0, 1.5, 1, 0)
    out = tmp_path / "dump"
    out.mkdir()
    subprocess.run([native_tool(), "glb", str(tmp_path / "t.glb"), str(out)], check=True, capture_output=True)
    assert np.fromfile(out / "transmission.bin", assets.TRANSMISSION_DTYPE).tobytes() == back.transmission.tobytes()


# ---------------------------------------------------------------------------------------------------------------- closed forms
def samples(mesh, flags, bounces, n, seed=1, sky=GW.SKY_L, window=GW.WINDOW):
    scene = RP.Scene(mesh, sky=None if sky is None else LW.constant_sky(sky))
    return RG.radiance_samples(scene, GW.CAMERA, window, flags, bounces, n, np.random.default_rng(seed), lens=GW.PINHOLE, glass=RG.table(mesh))


@pytest.mark.parametrize("bounces", (1, 2, 4))
def test_a_thin_untinted_pane_under_a_constant_sky_is_the_sky(bounces):
    """reflected or transmitted, the ray ends in the sky with throughput 1: every sample of every pane pixel is the sky, as is every
    pixel beside the pane; rule 4 at B = 1"""
    v = samples(GW.pane_world(), F_NEE_SKY, bounces, 8)
    wall = GW.inside(GW.WALL_COLS, GW.PANE_ROWS)
    assert np.abs(v[:, ~wall] - np.array(GW.SKY_L)).max() < 1e-12
    assert np.all(v[:, GW.inside(GW.WALL_COLS, GW.PANE_ROWS, margin=1.0)].mean(0) > 0.0)  # (the wall is lit by the sky)


def test_the_sky_shows_through_glass_without_sky_sampling():
    """rule 5: without NEE_SKY the pane still shows the sky, the diffuse wall beside it stays black; a last vertex adds nothing"""
    v = samples(GW.pane_world(), 0, 2, 8)
    wall, pane = GW.inside(GW.WALL_COLS, GW.PANE_ROWS), GW.inside(GW.PANE_COLS, GW.PANE_ROWS)
    assert np.abs(v[:, ~wall] - np.array(GW.SKY_L)).max() < 1e-12 and not v[:, wall].any() and pane.sum() > 500
    v1 = samples(GW.pane_world(), 0, 1, 2)
    assert not v1[:, pane].any() and np.abs(v1[:, ~wall & ~pane] - np.array(GW.SKY_L)).max() < 1e-12


def test_a_solid_slab_with_two_vertices_returns_R_plus_the_square_of_one_minus_R():
    """B = 2 under NEE_SKY: reflected at the front (R), or through the front and through the back ((1 - R)^2); a path turned back at
    the back face ends inside.  Every sample is the sky or nothing; the share per pixel within 5 sigma of the binomial."""
    n = 4096
    mesh, normal, _ = GW.slab_world()
    window = (8, 6)
    v = samples(mesh, F_NEE_SKY, 2, n, window=window)
    L = np.array(GW.SKY_L)
    assert np.all((np.abs(v - L).max(-1) < 1e-12) | (np.abs(v).max(-1) == 0.0))
    cos_i = -np.sum(GW.pixel_dirs(window) * normal, -1)
    R = RG.fresnel(cos_i, GW.IOR)
    p = R + (1.0 - R) ** 2
    share = (v[..., 1] > 0.5).mean(0)
    assert np.all(np.abs(share - p) < 5.0 * np.sqrt(p * (1.0 - p) / n)) and np.all(p < 0.97) and np.all(p > 0.9)


@pytest.mark.parametrize("tilt", (0.0, 35.0))
def test_an_edge_seen_through_a_slab_is_displaced_by_the_closed_form(tilt):
    """a slab of thickness t shifts a ray by t sin(theta_i - theta_t) / cos(theta_t) across its direction: the pixels that see the
    emissive half-plane are the ones the closed form says, their samples Le with probability (1 - R)^2 and 0 otherwise (B = 4)"""
    edge_px, n = 30.3, 256
    mesh, normal, _ = GW.slab_world(tilt_deg=tilt, emitter_edge_px=edge_px)
    dist, th_i = GW.edge_distance(normal, GW.IOR, edge_px)
    plain = GW.edge_distance(normal, 1.0, edge_px)[0]
    moved = (dist >= 0.0) != (plain >= 0.0)
    if tilt:  # 0.5 sin(35 - 22.5 deg) / cos(22.5 deg) = 0.117 at the centre, 1.7 pixels of 0.067 at the emitter's depth
        assert moved.sum() >= 48, "the displacement moves the edge by at least a pixel column"
    v = samples(mesh, 0, 4, n, sky=None)
    near = np.abs(dist) < 1e-3
    assert near.mean() <= 0.05
    lit, dark = (dist >= 0.0) & ~near, (dist < 0.0) & ~near
    assert not v[:, dark].any() and lit.sum() > 500 and dark.sum() > 500
    assert np.all((np.abs(v - GW.LE).max(-1) < 1e-12) | (np.abs(v).max(-1) == 0.0))
    R = RG.fresnel(np.cos(th_i), GW.IOR)
    p = (1.0 - R) ** 2
    share = (v[..., 0] > 0.0).mean(0)
    assert np.all(np.abs(share - p)[lit] < 5.0 * np.sqrt(p * (1.0 - p) / n)[lit])


def test_partial_transmission_mixes_the_two_lobes():
    """transmission 0.5 on a black, thin, untinted pane under a constant sky (NEE_SKY, B = 2): half the samples are the glass vertex's
    (the sky), the other half the black diffuse vertex's (nothing)"""
    mesh = GW.pane_world()
    k = mesh.names.index("pane")
    mesh.geometries["base_color"][k, :3] = 0.0
    mesh.transmission["transmission"][k] = 0.5
    n = 2048
    v = samples(mesh, F_NEE_SKY, 2, n, window=(16, 12))
    pane = GW.inside(  # (a coarser window over the same view)
    tuple(c / 4 for c in GW.PANE_COLS), tuple(r / 4 for r in GW.PANE_ROWS), (16, 12))
    share = (v[..., 1] > 0.0).mean(0)[pane]
    # a transmitted glass sample carries the tint, which is black here: only the reflected share F' of the glass half shows
    F = RG.thin_fresnel(RG.fresnel(-GW.pixel_dirs((16, 12))[..., 2], GW.IOR))[pane]
    p = 0.5 * F
    assert pane.sum() >= 20 and np.all(np.abs(share - p) < 5.0 * np.sqrt(p * (1.0 - p) / n))


# ---------------------------------------------------------------------------------------------------------------- fixture
def test_fixture_is_sized_and_arrays_only():
    fx = fixture()
    assert GOLDEN.stat().st_size < 64 * 1024
    for name, (_, _, _, _, spp, seed, _) in GW.ROOM_CASES.items():
        assert int(fx[f"{name}_spp"].item()) == spp and int(fx[f"{name}_seed"].item()) == seed
        assert fx[f"{name}_mean"].shape == fx[f"{name}_se"].shape == (2, 3, 3)
        assert np.all(fx[f"{name}_mean"] > 0) and np.all(fx[f"{name}_se"] > 0) and fx[f"{name}_cover"].all()
        # the fixture alone resolves 2 %: 0.02 x mean is beyond the band (by the margin the noise of the code under test may take)
        assert np.mean(0.02 * fx[f"{name}_mean"] > (Z_MAX + 1.0) * fx[f"{name}_se"]) >= 0.9


@pytest.mark.parametrize("name", sorted(GW.ROOM_CASES))
def test_generator_has_not_drifted(name):
    """the first CHUNK_SPP samples of each case, rendered again with the stored seed, give the stored prefix statistics"""
    spec = importlib.util.spec_from_file_location("gen_glass_ref", GOLDEN.parent / "gen_glass_ref.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fx = fixture()
    assert int(fx[f"{name}_seed"].item()) == GW.ROOM_CASES[name][5]
    bm, se = gen.render_prefix(name, RP.CHUNK_SPP)
    assert np.allclose(bm, fx[f"{name}_prefix_mean"], rtol=1e-9, atol=0.0)
    assert np.allclose(se, fx[f"{name}_prefix_se"], rtol=1e-9, atol=0.0)


def test_the_room_has_what_the_cases_are_about():
    mesh = GW.glass_room(False, 0.5)
    t = mesh.transmission
    assert sorted(np.flatnonzero(t["transmission"] > 0)) == sorted(mesh.names.index(n) for n in ("block", "pane"))
    assert t["thin_walled"][mesh.names.index("block")] == 0 and t["thin_walled"][mesh.names.index("pane")] == 1
    assert {c[3] for c in GW.ROOM_CASES.values()} == {1.0, 0.5}
    assert {(c[0], c[1]) for c in GW.ROOM_CASES.values()} >= {(0, 4), (IW.F_SPECULAR | IW.F_FACEFORWARD | IW.F_NEE_SKY, 6)}


# ---------------------------------------------------------------------------------------------------------------- self-test op 32
U24 = 2.0**-24


def op32_rows():
    """(ior, thin, d, n, u) as float32 / uint32 arrays: 512 random rows, then normal incidence from both sides, the critical angle of
    ior 1.5 from inside -+ 1e-3 rad, and thin-walled rows at those same angles"""
    f = np.float32
    rng = np.random.default_rng(32)
    m = 512
    n = rng.normal(size=(m, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = rng.normal(size=(m, 3)) * rng.uniform(0.25, 4.0, (m, 1))
    ior, thin = rng.uniform(1.0, 2.0, m), rng.integers(0, 2, m)
    u = rng.integers(0, 1 << 23, m) / float(1 << 23)
    nz, crit = np.array([0.0, 0.0, 1.0]), math.asin(1.0 / 1.5)
    special = [(1.5, 0, [0, 0, -1.0], nz, 0.5), (1.5, 0, [0, 0, 2.0], nz, 0.5), (1.5, 0, [0, 0, -1.0], nz, 0.01), (1.0, 0, [0.3, 0.1, -1.0], nz, 0.0)]
    for th in (crit - 1e-3, crit + 1e-3, 0.0, 1.2):
        for t in (0, 1):
            for uu in (0.03, 0.5, 0.999):
                special.append((1.5, t, [math.sin(th), 0.0, math.cos(th)], nz, uu))  # from inside: along +n
    ior = np.concatenate([ior, [s[0] for s in special]]).astype(f)
    thin = np.concatenate([thin, [s[1] for s in special]]).astype(np.uint32)
    d = np.concatenate([d, np.array([s[2] for s in special], np.float64)]).astype(f)
    n = np.concatenate([n, np.array([s[3] for s in special], np.float64)]).astype(f)
    u = np.concatenate([u, [s[4] for s in special]]).astype(f)
    return ior, thin, d, n, u


def op32_reference(ior, thin, d, n, u):
    """The float64 answers for the float32 rows and the rounding bounds of the device's fp32 evaluation (rt3_glass.hpp: glass_sample),
    derived, with e = 2^-24 per rounding, |n| = 1 and first-order propagation doubled to cover the second order:

      ud = d / sqrt(d.d): 3 e for the dot product of positive terms, 1.5 e through the root, 1 e for the division  -> 4 e per component
      c = n.ud: 3 products and 2 sums of magnitude <= 1 on operands off by 4 e                                    -> 7 e (absolute)
      eta^2: eta itself (1 e when it is 1 / ior), the square                                                      -> 3 e (relative)
      x = c^2 + (eta^2 - 1): 2 c 7 e + 1 e for c^2, 4 e eta^2 for the bracket, 1 e |x| for the sum;
      cos_t^2 = x / eta^2: + (3 + 1) e cos_t^2                        -> E2 = (15 e + 4 e eta^2) / eta^2 + 5 e cos_t^2 (absolute)
      cos_t = sqrt(cos_t^2): |sqrt(a + h) - sqrt(a)| <= |h| / sqrt(a) for |h| <= a                                -> Et = E2 / cos_t + e
      r = (a - b) / (a + b): |dr| <= 2 (b da + a db) / (a + b)^2 + 3 e; for r_s a = cos_i (da = 7 e), b = eta cos_t (db = eta Et + 2 e b);
                             for r_p a = eta cos_i (da = 7 e eta + 2 e a), b = cos_t (db = Et)
      F = (r_s^2 + r_p^2) / 2: |dF| <= |r_s| dr_s + |r_p| dr_p + (dr_s^2 + dr_p^2) / 2 + 3 e F;   thin: F' = 2 F / (1 + F), slope <= 2
      reflected: ud - (2 c) n: 4 e + 2 (7 e + e) + e                                                              -> 21 e per component
      refracted: ud / eta + k n, k = cos_i / eta - cos_t: dk = 9 e / eta + Et + e |k|                             -> 6 e / eta + dk + 3 e (1 / eta + |k|)
      thin, transmitted: ud itself                                                                                -> 4 e
    Rows whose cos_t^2 lies within 2 E2 of 0 have no determined branch (total internal reflection or not) and are `open`, as are, for the
    event alone, rows whose u lies within the bound of F.  Returns (transmit, direction, F, direction bound, F bound, open, event open)."""
    e = U24
    ior, d, n, u = (np.asarray(a, np.float64) for a in (ior, d, n, u))
    thin = np.asarray(thin) != 0
    tr, out, F = RG.glass_event(ior, thin, d, n, u)
    ud = d / np.linalg.norm(d, axis=1, keepdims=True)
    c = np.sum(n * ud, -1)
    cos_i = np.abs(c)
    eta = np.where(thin | (c < 0), ior, 1.0 / ior)
    ct2 = 1.0 - (1.0 - cos_i**2) / eta**2
    E2 = 2.0 * ((15 * e + 4 * e * eta**2) / eta**2 + 5 * e * np.abs(ct2))
    open_ = np.abs(ct2) <= 2.0 * E2
    tir = ct2 < 0
    ct = np.sqrt(np.where(tir | open_, 1.0, ct2))
    Et = E2 / ct + e

    def dr(a, b, da, db):
        return 2.0 * (2.0 * (b * da + a * db) / (a + b) ** 2 + 3 * e)

    rs, rp = (cos_i - eta * ct) / (cos_i + eta * ct), (eta * cos_i - ct) / (eta * cos_i + ct)
    drs = dr(cos_i, eta * ct, 7 * e, eta * Et + 2 * e * eta * ct)
    drp = dr(eta * cos_i, ct, 7 * e * eta + 2 * e * eta * cos_i, Et)
    F0 = 0.5 * (rs * rs + rp * rp)
    dF = np.abs(rs) * drs + np.abs(rp) * drp + 0.5 * (drs**2 + drp**2) + 3 * e * F0
    dF = np.where(thin, 2.0 * dF + 3 * e, dF)
    dF = np.where(tir, 0.0, dF)  # F = 1 exactly
    k = cos_i / eta - ct
    dk = 9 * e / eta + Et + e * np.abs(k)
    d_refr = 2.0 * (6 * e / eta + dk + 3 * e * (1.0 / eta + np.abs(k)))
    d_dir = np.where(tr, np.where(thin, 4 * e, d_refr), 21 * e)
    return tr, out, F, d_dir, dF, open_, open_ | (np.abs(u - F) <= dF)


def test_op32_rows_leave_few_events_open():
    """the reference alone: under 1 % of the rows are too close to a branch for an fp32 evaluation to be held to the event; the rows reach
    both events, both sides, both wall kinds and total internal reflection"""
    ior, thin, d, n, u = op32_rows()
    tr, out, F, d_dir, dF, open_, ev_open = op32_reference(ior, thin, d, n, u)
    assert ev_open.mean() < 0.01 and len(u) >= 512 + 20
    assert tr.sum() > 100 and (~tr).sum() > 50 and (F == 1.0).sum() > 10 and (thin != 0).sum() > 100
    assert d_dir.max() < 1e-3 and dF.max() < 1e-2 and np.median(dF) < 1e-5
