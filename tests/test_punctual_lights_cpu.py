"""Punctual lights without a GPU: the float64 reference of tests/ref_lights.py against known answers, the glTF
KHR_lights_punctual round trip of the Python loader, and the fixture tests/golden/punctual_ref.npz (size, contents, no generator drift)."""
import functools
import importlib.util
import math
from pathlib import Path

import numpy as np

import integrator_worlds as IW
import punctual_worlds as PW
import ref_lights as RL
import ref_pathtrace as RP
from raytracer3_amd import assets
from raytracer3_amd.assets import LIGHT_DIRECTIONAL, LIGHT_DTYPE, LIGHT_POINT, LIGHT_SPOT, make_light
from test_integrator_cpu import Z_MAX

GOLDEN = Path(__file__).resolve().parent / "golden" / "punctual_ref.npz"
UP = np.array([[0.0, 1.0, 0.0]])


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


# ---------------------------------------------------------------------------------------------------------------- known answers
def test_point_light_falls_off_with_the_inverse_square():
    l = make_light(LIGHT_POINT, (8.0, 4.0, 2.0), position=(0.0, 2.0, 0.0))
    E1, wl, d = RL.irradiance(l, [[0.0, 0.0, 0.0]], UP)
    assert np.allclose(E1, [[2.0, 1.0, 0.5]], rtol=1e-15) and np.allclose(wl, UP) and d[0] == 2.0
    E2, _, _ = RL.irradiance(l, [[0.0, -2.0, 0.0]], UP)
    assert np.allclose(E2, E1 / 4.0, rtol=1e-15)
    # oblique: cos = 2 / sqrt(8), d^2 = 8
    E3, _, _ = RL.irradiance(l, [[2.0, 0.0, 0.0]], UP)
    assert np.allclose(E3, np.array([[8.0, 4.0, 2.0]]) * (2.0 / math.sqrt(8.0)) / 8.0, rtol=1e-15)
    # below the horizon and at the light itself: nothing
    assert not RL.irradiance(l, [[0.0, 3.0, 0.0]], UP)[0].any()
    assert not RL.irradiance(l, [[0.0, 2.0, 0.0]], UP)[0].any()


def test_spot_cone_at_inner_outer_and_midway():
    inner, outer = 0.3, 0.7
    l = make_light(LIGHT_SPOT, (1.0, 1.0, 1.0), position=(0.0, 1.0, 0.0), direction=(0.0, -2.0, 0.0), inner_cone=inner, outer_cone=outer)
    ci, co = math.cos(float(np.float32(inner))), math.cos(float(np.float32(outer)))

    def cone_at(angle):  # the point below the light at that angle off the axis, one unit from it
        x = np.array([[math.sin(angle), 1.0 - math.cos(angle), 0.0]])
        return RL.light_sample(l, x)[2][0, 0]

    assert cone_at(0.0) == 1.0 and cone_at(0.5 * inner) == 1.0
    assert abs(cone_at(float(np.float32(inner))) - 1.0) < 1e-12
    assert cone_at(float(np.float32(outer)) + 1e-9) == 0.0 and cone_at(1.2) == 0.0
    mid = math.acos(0.5 * (ci + co))  # midway in the cosine: c = 1/2, cone = 1/4
    assert abs(cone_at(mid) - 0.25) < 1e-12


def test_range_window():
    l = make_light(LIGHT_POINT, (1.0, 1.0, 1.0), position=(0.0, 0.0, 0.0), range=4.0)
    k = lambda d: RL.light_sample(l, [[d, 0.0, 0.0]])[2][0, 0]
    assert k(4.0) == 0.0 and k(5.0) == 0.0
    assert abs(k(2.0) - (1.0 - 1.0 / 16.0)) < 1e-15 and abs(k(1e-3) - 1.0) < 1e-12
    unlimited = make_light(LIGHT_POINT, (1.0, 1.0, 1.0), position=(0.0, 0.0, 0.0), range=0.0)
    assert RL.light_sample(unlimited, [[1e4, 0.0, 0.0]])[2][0, 0] == 1.0


def test_directional_light():
    l = make_light(LIGHT_DIRECTIONAL, (3.0, 2.0, 1.0), direction=(0.0, -3.0, -4.0), range=1.0)  # (range means nothing here)
    E, wl, d = RL.irradiance(l, [[7.0, -2.0, 100.0]], UP)
    assert np.allclose(wl, [[0.0, 0.6, 0.8]]) and np.isinf(d[0])
    assert np.allclose(E, [[1.8, 1.2, 0.6]], rtol=1e-15)


def test_masses():
    ls = PW.lights(make_light(LIGHT_POINT, (1.0, 1.0, 1.0)), make_light(LIGHT_SPOT, (2.0, 0.0, 0.0), inner_cone=0.1, outer_cone=0.2),
                   make_light(LIGHT_DIRECTIONAL, (0.5, 0.5, 0.5)))
    p = RL.powers(ls, 9.0)
    assert np.allclose(p, [4.0, 4.0 * 2.0 * 0.299, 0.5 * 9.0], rtol=1e-15)
    m = RL.cdf_masses(p)
    assert m.sum() == RL.CDF_TOTAL and np.all(np.abs(m - p / p.sum() * RL.CDF_TOTAL) <= 1.0)
    assert not RL.cdf_masses([0.0, 0.0]).any()


def test_occlusion_segment():
    scene = RP.Scene(PW.floor_world(occluder=True))
    x = np.array([[0.2, 0.0, -0.3], [0.2, 0.0, -0.3], [2.0, 0.0, 2.0]])
    up = np.broadcast_to(UP, (3, 3)).copy()
    assert list(RL.occluded(scene, x, up, np.array([1.0, 0.7, 5.0]))) == [True, False, False]


# ---------------------------------------------------------------------------------------------------------------- glTF
def rotation(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    h = math.radians(deg) / 2.0
    return [float(a[0] * math.sin(h)), float(a[1] * math.sin(h)), float(a[2] * math.sin(h)), math.cos(h)]


def test_gltf_round_trip(tmp_path):
    mesh = PW.floor_world()
    mesh.lights = PW.lights(
        make_light(LIGHT_POINT, (3.0, 2.5, 0.25), position=(0.5, 1.5, -2.0), range=7.5),
        make_light(LIGHT_SPOT, (40.0, 10.0, 5.0), position=(-1.0, 3.0, 0.25), direction=(0.3, -2.0, 0.6), range=0.0, inner_cone=0.25, outer_cone=0.75),
        make_light(LIGHT_DIRECTIONAL, (1.5, 1.25, 1.0), direction=(-0.2, -1.0, 0.4)),
    )
    p = tmp_path / "lit.glb"
    assets.write_glb(p, mesh)
    back = assets.load(p)
    assert back.lights.dtype == LIGHT_DTYPE and len(back.lights) == 3
    for a, b in zip(mesh.lights, back.lights):
        assert int(a["type"]) == int(b["type"])
        assert np.array_equal(a["intensity"], b["intensity"]) and float(a["range"]) == float(b["range"])
        if int(a["type"]) != LIGHT_DIRECTIONAL:
            assert np.array_equal(a["position"], b["position"])
        if int(a["type"]) == LIGHT_SPOT:
            assert float(a["inner_cone"]) == float(b["inner_cone"]) and float(a["outer_cone"]) == float(b["outer_cone"])
        if int(a["type"]) != LIGHT_POINT:  # the file holds a unit quaternion: the direction comes back normalised, to fp32 rounding
            d = a["direction"].astype(np.float64)
            assert np.abs(b["direction"] - d / np.linalg.norm(d)).max() <= 2.0**-23
    assert np.array_equal(back.vertices, mesh.vertices)


def lit_glb(tmp_path):
    """a .glb with all three light types under one rotated, translated and (non-uniformly) scaled parent: (path, document, parent node,
    index of the parent)"""
    import json
    import struct

    mesh = PW.floor_world()
    p = tmp_path / "floor.glb"
    assets.write_glb(p, mesh)
    data = p.read_bytes()
    n_json = struct.unpack_from("<I", data, 12)[0]
    doc = json.loads(data[20:20 + n_json])
    rest = data[20 + n_json:]
    doc["extensionsUsed"] = ["KHR_lights_punctual"]
    doc["extensions"] = {"KHR_lights_punctual": {"lights": [
        {"type": "point", "color": [1.0, 0.5, 0.25], "intensity": 8.0, "range": 3.0},
        {"type": "spot", "intensity": 2.0},
        {"type": "directional", "color": [0.5, 0.5, 1.0], "intensity": 3.0},
    ]}}
    first = len(doc["nodes"])
    parent = {"translation": [1.0, 2.0, 3.0], "rotation": rotation((1.0, 2.0, -1.0), 40.0), "scale": [2.0, 0.5, 3.0], "children": [first + 1, first + 2, first + 3]}
    doc["nodes"] += [parent,
                     {"translation": [0.5, 0.0, -1.0], "extensions": {"KHR_lights_punctual": {"light": 0}}},
                     {"translation": [0.0, 1.0, 0.0], "rotation": rotation((0.0, 1.0, 0.0), 90.0), "extensions": {"KHR_lights_punctual": {"light": 1}}},
                     {"rotation": rotation((1.0, 0.0, 0.0), -60.0), "extensions": {"KHR_lights_punctual": {"light": 2}}}]
    doc["scenes"][0]["nodes"].append(first)
    js = json.dumps(doc).encode()
    js += b" " * ((-len(js)) % 4)
    q = tmp_path / "lit.glb"
    q.write_bytes(struct.pack("<4sII", b"glTF", 2, 12 + 8 + len(js) + len(rest)) + struct.pack("<I4s", len(js), b"JSON") + js + rest)
    return q, doc, parent, first


def test_gltf_lights_are_baked_through_their_nodes(tmp_path):
    """position M (0, 0, 0, 1), direction normalise(M3 (0, 0, -1)), intensity untouched by the node's scale; spot angles default to 0 and
    pi / 4"""
    q, doc, parent, first = lit_glb(tmp_path)
    back = assets.load(q)
    assert [int(t) for t in back.lights["type"]] == [LIGHT_POINT, LIGHT_SPOT, LIGHT_DIRECTIONAL]
    M = assets._node_matrix(parent)
    for k, l in enumerate(back.lights):
        m = M @ assets._node_matrix(doc["nodes"][first + 1 + k])
        d = m[:3, :3] @ [0.0, 0.0, -1.0]
        assert np.array_equal(l["position"], m[:3, 3].astype(np.float32))
        assert np.array_equal(l["direction"], (d / np.linalg.norm(d)).astype(np.float32))
    assert np.array_equal(back.lights["intensity"], np.array([[8.0, 4.0, 2.0], [2.0, 2.0, 2.0], [1.5, 1.5, 3.0]], np.float32))
    assert float(back.lights["range"][0]) == 3.0 and float(back.lights["range"][1]) == 0.0
    assert float(back.lights["inner_cone"][1]) == 0.0 and back.lights["outer_cone"][1] == np.float32(math.pi / 4)


def test_cpp_loader_reads_the_same_lights(tmp_path):
    """asset_tool glb dumps lights.bin: byte for byte the Python loader's records (built as tests/test_host_assets.py builds the tool)"""
    import os
    import subprocess

    host = Path(__file__).resolve().parent.parent / "raytracer3_amd" / "host"
    tool = os.environ.get("RT3_ASSET_TOOL")
    if not tool:
        subprocess.check_call(["make", "-C", str(host), "asset_tool"], stdout=subprocess.DEVNULL)
        tool = str(host / "asset_tool")
    q = lit_glb(tmp_path)[0]
    mesh = PW.floor_world()
    mesh.lights = PW.lights(make_light(LIGHT_SPOT, (40.0, 10.0, 5.0), position=(-1.0, 3.0, 0.25), direction=(0.3, -2.0, 0.6), range=9.0, inner_cone=0.25, outer_cone=0.75),
                            make_light(LIGHT_DIRECTIONAL, (1.5, 1.25, 1.0), direction=(0.0, 0.0, 1.0)), make_light(LIGHT_POINT, (3.0, 2.5, 0.25), position=(0.5, 1.5, -2.0)))
    w = tmp_path / "written.glb"
    assets.write_glb(w, mesh)
    for k, f in enumerate((q, w)):
        out = tmp_path / f"dump{k}"
        out.mkdir()
        r = subprocess.run([tool, "glb", str(f), str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        want = assets.load(f).lights
        assert len(want) == 3 and (out / "lights.bin").read_bytes() == want.tobytes()
    plain = tmp_path / "plain.glb"
    assets.write_glb(plain, PW.floor_world())
    out = tmp_path / "dump_plain"
    out.mkdir()
    assert subprocess.run([tool, "glb", str(plain), str(out)], capture_output=True).returncode == 0 and (out / "lights.bin").read_bytes() == b""


# ---------------------------------------------------------------------------------------------------------------- fixture
def test_world_condition():
    """no triangle nearer to a point or spot light than 1 % of its distance to any lit point (an upper bound: the scene's diagonal)"""
    for name in PW.CASES:
        mesh, _ = PW.room(name)
        scene = RP.Scene(mesh)
        pts = scene.p.reshape(-1, 3)
        for l in mesh.lights:
            if int(l["type"]) == LIGHT_DIRECTIONAL:
                continue
            P = l["position"].astype(np.float64)
            far = np.linalg.norm(pts - P, axis=1).max()
            # distance from P to every triangle's plane patch is at least the distance to its bounding sphere's surface; cheaper and
            # sufficient here: the distance to the nearest point of a dense sampling of every triangle
            s, t = np.meshgrid(np.linspace(0, 1, 33), np.linspace(0, 1, 33))
            keep = s + t <= 1.0
            grid = scene.v0[:, None] + s[keep][None, :, None] * scene.e1[:, None] + t[keep][None, :, None] * scene.e2[:, None]
            near = np.linalg.norm(grid - P, axis=-1).min()
            assert near - 0.2 > 0.01 * far, (name, near, far)  # (0.2: more than the sampling's spacing on these triangles' 8-unit edges / 32)


def test_fixture_is_sized_and_arrays_only():
    fx = fixture()
    assert GOLDEN.stat().st_size < 64 * 1024
    for name, (_, _, _, _, spp, seed, _) in PW.CASES.items():
        assert int(fx[f"{name}_spp"].item()) == spp and int(fx[f"{name}_seed"].item()) == seed
        assert fx[f"{name}_mean"].shape == fx[f"{name}_se"].shape == (2, 3, 3)
        assert np.all(fx[f"{name}_mean"] > 0) and np.all(fx[f"{name}_se"] > 0)
        # the fixture alone resolves 2 %: 0.02 x mean is beyond the band (by the margin the noise of the code under test may take)
        assert np.mean(0.02 * fx[f"{name}_mean"] > (Z_MAX + 1.0) * fx[f"{name}_se"]) >= 0.9


def test_generator_has_not_drifted():
    """the first CHUNK_SPP samples of one case, rendered again with the stored seed, give the stored prefix statistics"""
    spec = importlib.util.spec_from_file_location("gen_punctual_ref", GOLDEN.parent / "gen_punctual_ref.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fx = fixture()
    name = "point_b3"
    flags, bounces, _, _, _, _, _ = PW.CASES[name]
    scene, lights = gen.room_scene(name)
    mean, var = RL.render_lit(scene, lights, IW.ROOM_CAMERA, IW.WINDOW_ROOM, flags, bounces, RP.CHUNK_SPP, int(fx[f"{name}_seed"].item()))
    bm, se = RP.block_stats(mean, var, RP.CHUNK_SPP)
    assert np.allclose(bm, fx[f"{name}_prefix_mean"], rtol=1e-9, atol=0.0)
    assert np.allclose(se, fx[f"{name}_prefix_se"], rtol=1e-9, atol=0.0)


def test_lights_add_to_the_unlit_reference():
    """with no light the lit tracer is ref_pathtrace's, sample for sample; a light only adds"""
    mesh, _ = PW.room("point_b3")
    scene = RP.Scene(mesh)
    a = RP.radiance_samples(scene, IW.ROOM_CAMERA, IW.WINDOW_ROOM, RP.F_FACEFORWARD, 3, 2, np.random.default_rng(5))
    b = RL.radiance_samples_lit(scene, mesh.lights[:0], IW.ROOM_CAMERA, IW.WINDOW_ROOM, RP.F_FACEFORWARD, 3, 2, np.random.default_rng(5))
    c = RL.radiance_samples_lit(scene, mesh.lights, IW.ROOM_CAMERA, IW.WINDOW_ROOM, RP.F_FACEFORWARD, 3, 2, np.random.default_rng(5))
    assert np.allclose(a, b, rtol=1e-12, atol=0.0)
    assert np.all(c >= b - 1e-12) and c.sum() > 1.5 * b.sum()
