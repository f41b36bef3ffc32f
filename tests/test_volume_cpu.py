"""Absorbing glass without a GPU (rt3_scene_set_attenuation): the float64 reference (tests/ref_volume.py) against the two
closed forms of an absorbing slab, inside the bands the GPU tests use; the glTF round trip of attenuationColor / attenuationDistance
through both loaders; and the committed fixture against its generator."""
import importlib.util
import json
import math
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import glass_worlds as GW
import integrator_worlds as IW
import lens_worlds as LW
import ref_glass as RG
import ref_pathtrace as RP
import ref_volume as RV
import volume_worlds as VW
from raytracer3_amd import assets, scenes
from raytracer3_amd.assets import Material, MeshBuilder
from test_glass_cpu import native_tool, uploaded_calls
from test_integrator_cpu import Z_MAX

GOLDEN = Path(__file__).resolve().parent / "golden" / "volume_ref.npz"
SKY = np.array(VW.SKY_L)
F_NEE_SKY = RP.F_NEE_SKY


def fixture():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def samples(mesh, bounces, n, window, seed=1):
    scene = RP.Scene(mesh, sky=LW.constant_sky(VW.SKY_L))
    return RV.radiance_samples(scene, VW.CAMERA, window, F_NEE_SKY, bounces, n, np.random.default_rng(seed), lens=VW.PINHOLE,
                               glass=RG.table(mesh), sigma=VW.sigma_table(mesh))


# ---------------------------------------------------------------------------------------------------------------- 1 closed forms
@pytest.mark.parametrize("tilt", (0.0, 35.0))
def test_reference_meets_the_index_matched_slab(tilt):
    """closed form A: an index-matched slab neither reflects nor bends; every sample of a pixel is SKY exp(-sigma thickness / cos theta)"""
    mesh, n, centre = VW.slab_world(ior=1.0, tilt_deg=tilt)
    assert mesh.absorbing().sum() == 2
    on, near = VW.slab_outline_share(n, centre)
    assert on == 1.0 and near <= 0.10  # every pixel lies on the slab, none near its outline
    v = samples(mesh, 4, 2, VW.WINDOW)
    cos_i, t_front, t_back, _ = VW.slab_geometry(mesh, n)
    assert np.abs((t_back - t_front) * cos_i / VW.THICKNESS - 1.0).max() < 1e-4  # thickness / cos theta, up to the float32 vertices
    want = SKY * RV.slab_matched(VW.SLAB_SIGMA, t_back - t_front)
    assert np.abs(v / want - 1.0).max() < 1e-9
    dropped = SKY * RV.slab_matched(VW.SLAB_SIGMA, np.full_like(cos_i, VW.THICKNESS))
    assert np.abs(dropped / want - 1.0).max() > 1e-2  # the obliquity matters in this view


def test_reference_meets_the_absorbing_slab_with_inter_reflections():
    """closed form B at ior 1.5 in a coarse window: the mean over all pixels and samples within the GPU test's band of the summed series,
    and the band tells it from the series with one internal segment"""
    window, n_s, B = (8, 6), 2048, 8
    mesh, n, centre = VW.slab_world()
    v = samples(mesh, B, n_s, window)
    assert np.all(v >= 0.0) and np.all(v <= SKY + 1e-12)
    cos_i = VW.slab_geometry(mesh, n, window)[0]
    R, T = RV.slab_R_T(VW.SLAB_SIGMA, VW.THICKNESS, cos_i, GW.IOR)
    R1, T1 = RV.slab_R_T(VW.SLAB_SIGMA, VW.THICKNESS, cos_i, GW.IOR, single_segment=True)
    want, wrong = SKY * (R + T).mean((0, 1)), SKY * (R1 + T1).mean((0, 1))
    n_pix = window[0] * window[1]
    band = 5.0 * SKY / (2.0 * math.sqrt(n_pix * n_s)) + SKY * RV.slab_tail(VW.SLAB_SIGMA, VW.THICKNESS, cos_i, GW.IOR, B).max((0, 1))
    dev = np.abs(v.mean((0, 1, 2)) - want)
    assert np.all(dev <= band), (dev, band)
    assert np.all(np.abs(want - wrong) > 2.0 * band)


def test_the_rule_in_float64():
    T = np.array([[0.5, 0.25, 1.0]] * 3)
    sigma = np.array([[2.0, 0.0, 1.0], [2.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    n = np.array([[0.0, 0.0, 1.0]] * 3)
    d = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, -2.0], [0.0, 0.0, 2.0]])
    out, applied = RV.absorb(T, sigma, np.array([1.5, 1.5, 1.5]), n, d)
    assert applied.tolist() == [True, False, False]
    assert np.allclose(out[0], [0.5 * math.exp(-3.0), 0.25, math.exp(-1.5)], rtol=1e-15) and np.array_equal(out[1:], T[1:])


# ---------------------------------------------------------------------------------------------------------------- 2 the glb round trip
AMBER, GREEN = ((0.95, 0.55, 0.12), 0.25), ((0.35, 0.9, 0.45), 0.3)


def coloured_mesh():
    mb = MeshBuilder()
    quad = scenes._grid([0, 0, 0], [1, 0, 0], [0, 1, 0], 1, 1)
    mb.add("amber", *quad, Material(transmission=1.0, thin_walled=0, attenuation_color=AMBER[0], attenuation_distance=AMBER[1]))
    mb.add("green_pane", *quad, Material(transmission=1.0, thin_walled=1, attenuation_color=GREEN[0], attenuation_distance=GREEN[1]))
    mb.add("clear", *quad, Material(transmission=1.0, thin_walled=0))
    mb.add("black", *quad, Material(transmission=1.0, thin_walled=0, attenuation_color=(0.0, 1.0, 2.0), attenuation_distance=2.0))
    mb.add("opaque", *quad, Material(attenuation_color=GREEN[0], attenuation_distance=GREEN[1]))
    return mb.build()


def expected_sigma(color, distance):
    return np.array([-math.log(min(max(c, assets.FLT_MIN), 1.0)) / distance + 0.0 for c in color], np.float64).astype(np.float32)


def test_gltf_round_trip_keeps_the_sigmas(tmp_path):
    mesh = coloured_mesh()
    a = mesh.attenuation
    assert a.dtype == assets.ATTENUATION_DTYPE and a.dtype.itemsize == 16 and not a["reserved"].any()
    assert a["sigma"][0].tobytes() == expected_sigma(*AMBER).tobytes() and a["sigma"][1].tobytes() == expected_sigma(*GREEN).tobytes()
    assert not a["sigma"][2].any() and np.array_equal(a["sigma"][3], np.float32([-math.log(assets.FLT_MIN) / 2.0, 0.0, 0.0]))
    # a thin-walled or opaque material keeps its sigma in the table; the classification ignores it
    assert a["sigma"][1].all() and a["sigma"][4].all() and mesh.absorbing().tolist() == [True, False, False, True, False]
    assets.write_glb(tmp_path / "v.glb", mesh)
    back = assets.load(tmp_path / "v.glb")
    assert back.attenuation.tobytes() == a.tobytes() and back.transmission.tobytes() == mesh.transmission.tobytes()
    data = (tmp_path / "v.glb").read_bytes()
    doc = json.loads(data[20 : 20 + struct.unpack_from("<I", data, 12)[0]].decode())
    vol = [m.get("extensions", {}).get("KHR_materials_volume") for m in doc["materials"]]
    assert vol[0] == {"thicknessFactor": 1.0, "attenuationColor": list(AMBER[0]), "attenuationDistance": AMBER[1]}
    assert vol[1] == {"attenuationColor": list(GREEN[0]), "attenuationDistance": GREEN[1]}  # no thickness: thin-walled
    assert vol[2] == {"thicknessFactor": 1.0}  # the defaults stay implicit
    # the native loader, bit for bit
    subprocess.run([native_tool(), "glb", str(tmp_path / "v.glb"), str(tmp_path)], check=True, capture_output=True)
    assert np.fromfile(tmp_path / "attenuation.bin", assets.ATTENUATION_DTYPE).tobytes() == a.tobytes()
    # sigmas that did not come from a colour and a distance are written as a pair that reads back to the same bits
    mesh.attenuation_source = None
    mesh.attenuation["sigma"][2] = (7.25, 1e-3, 0.0)
    assets.write_glb(tmp_path / "w.glb", mesh)
    assert assets.load(tmp_path / "w.glb").attenuation.tobytes() == mesh.attenuation.tobytes()


def test_defaults_and_an_absent_extension_give_zero_and_make_no_call(tmp_path):
    for mesh in (scenes.cornell(), scenes.glass_cornell(), scenes.amber_cornell(absorb=False)):
        assets.write_glb(tmp_path / "c.glb", mesh)
        back = assets.load(tmp_path / "c.glb")
        assert back.attenuation.tobytes() == assets.no_attenuation(len(back.geometries)).tobytes() and not back.absorbing().any()
        assert b"attenuation" not in (tmp_path / "c.glb").read_bytes()
        assert "rt3_scene_set_attenuation" not in uploaded_calls(back)
        subprocess.run([native_tool(), "glb", str(tmp_path / "c.glb"), str(tmp_path)], check=True, capture_output=True)
        assert np.fromfile(tmp_path / "attenuation.bin", assets.ATTENUATION_DTYPE).tobytes() == back.attenuation.tobytes()
    amber = scenes.amber_cornell()
    assert amber.absorbing().sum() == 3 and uploaded_calls(amber).count("rt3_scene_set_attenuation") == 1
    big, small = amber.names.index("green_sphere_large"), amber.names.index("green_sphere_small")
    assert amber.attenuation[big].tobytes() == amber.attenuation[small].tobytes()  # the same glass at two sizes


def test_an_infinite_distance_is_no_absorption():
    assert not assets.attenuation_sigma((0.2, 0.3, 0.4), math.inf).any()
    assert np.array_equal(assets.attenuation_sigma((1.0, 1.0, 1.0), 0.5), np.zeros(3, np.float32))
    assert not np.signbit(assets.attenuation_sigma((1.0, 1.0, 1.0), 0.5)).any()
    with pytest.raises(ValueError):
        assets.attenuation_sigma((0.5, 0.5, 0.5), 0.0)


# ---------------------------------------------------------------------------------------------------------------- 3 the fixture
def test_fixture_is_sized_and_arrays_only():
    fx = fixture()
    assert GOLDEN.stat().st_size <= (GOLDEN.parent / "glass_ref.npz").stat().st_size
    for name, (_, _, _, _, spp, seed, _) in VW.ROOM_CASES.items():
        assert int(fx[f"{name}_spp"].item()) == spp and int(fx[f"{name}_seed"].item()) == seed
        assert fx[f"{name}_mean"].shape == fx[f"{name}_se"].shape == (2, 3, 3)
        assert np.all(fx[f"{name}_mean"] > 0) and np.all(fx[f"{name}_se"] > 0) and fx[f"{name}_cover"].all()
        assert np.mean(0.02 * fx[f"{name}_mean"] > (Z_MAX + 1.0) * fx[f"{name}_se"]) >= 0.9


@pytest.mark.parametrize("name", sorted(VW.ROOM_CASES))
def test_generator_reproduces_the_fixture(name):
    """the first CHUNK_SPP samples of each case, rendered again with the stored seed, give the stored prefix statistics"""
    spec = importlib.util.spec_from_file_location("gen_volume_ref", GOLDEN.parent / "gen_volume_ref.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fx = fixture()
    bm, se = gen.render_prefix(name, RP.CHUNK_SPP)
    assert np.allclose(bm, fx[f"{name}_prefix_mean"], rtol=1e-9, atol=0.0)
    assert np.allclose(se, fx[f"{name}_prefix_se"], rtol=1e-9, atol=0.0)


def test_the_room_absorbs_where_the_case_is_about_it():
    """the absorbing room differs from the glass room it extends: its block and ball are classified, its pane is not; and absorption
    changes the fixture's block means by many standard errors"""
    mesh = VW.absorbing_room()
    assert [mesh.names[k] for k in np.flatnonzero(mesh.absorbing())] == ["block", "ball"]
    name = "amber_b6"
    flags, bounces, specular, tau, _, seed, _ = VW.ROOM_CASES[name]
    clear = VW.absorbing_room(specular, tau, sigmas={})
    scene = RP.Scene(clear, sky=IW.room_sky())
    mean, var = RG.render(scene, IW.ROOM_CAMERA, IW.WINDOW_ROOM, flags, bounces, RP.CHUNK_SPP, seed, lens=VW.ROOM_LENS, glass=RG.table(clear))
    bm, se = RP.block_stats(mean, var, RP.CHUNK_SPP)
    fx = fixture()
    z = (bm - fx[f"{name}_prefix_mean"]) / np.hypot(se, fx[f"{name}_prefix_se"])
    assert np.abs(z).max() > 6.0
