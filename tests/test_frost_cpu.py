"""Rough transmission without a GPU: the float64 rule of tests/ref_frost.py against its limits and closed forms, the rows
and derived bounds of self-test op 38 (held against a float32 model of the device's arithmetic), the classification through the glTF round
trip, and the fixture tests/golden/frost_ref.npz (size, contents, no generator drift)."""
import functools
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

import frost_worlds as FW
import glass_worlds as GW
import ref_frost as RF
import ref_glass as RG
import ref_pathtrace as RP
import ref_shading as R
from raytracer3_amd import _lib as L
from raytracer3_amd import assets
from test_integrator_cpu import Z_MAX

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden" / "frost_ref.npz"
U24 = 2.0**-24


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@functools.lru_cache(maxsize=None)
def op38():
    rows = RF.op38_rows()
    return rows, RF.op38_reference(*rows)


def random_rows(m, seed):
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(m, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = rng.normal(size=(m, 3)) * rng.uniform(0.25, 4.0, (m, 1))
    return rng, d, n


# ---------------------------------------------------------------------------------------------------------------- self-test op 38
def test_op38_rows_leave_few_events_open():
    """the reference alone: under 1 % of the rows are too close to a branch for an fp32 evaluation to be held to the event (a condition, not
    a measurement); the rows reach all three events, both sides, both wall kinds, total internal reflection and every alpha"""
    (ior, thin, d, n, alpha, u, u2, u3), ref = op38()
    assert len(u) >= 8192 + 20 and ref["ev_open"].mean() < 0.01
    ev = ref["event"]
    assert (ev == RF.REFLECT).sum() > 500 and (ev == RF.TRANSMIT).sum() > 2000 and (ev == RF.INVALID).sum() > 200
    assert (ref["F"] == 1.0).sum() > 100 and (thin != 0).sum() > 2000 and set(alpha.tolist()) == {float(np.float32(a)) for a in RF.ALPHAS}
    # the bounds are not vacuous: in units of 2^-24 the well-conditioned half of the rows is held to a few hundred, nearly all to a few thousand
    closed = ~ref["open"]
    live = closed & (ev != RF.INVALID)
    assert np.all(np.isfinite(ref["d_dir"][closed]))
    assert np.median(ref["d_dir"][closed]) <= 400 * U24 and np.percentile(ref["d_dir"][closed], 99) <= 4000 * U24
    assert np.median(ref["dF"][closed]) <= 100 * U24 and np.percentile(ref["dF"][closed], 99) <= 4000 * U24
    assert np.median(ref["dW"][live]) <= 200 * U24 and np.percentile(ref["dW"][live], 99) <= 4000 * U24


def test_a_float32_model_of_the_rule_stays_inside_the_derived_bounds():
    """ref_frost.rule in float32 -- the device's operations in the device's order -- against the float64 answers: no closed row changes its
    event, and direction, F and weight stay inside op38_reference's per-row bounds"""
    rows, ref = op38()
    m32 = RF.rule(np.float32, *rows)
    closed = ~ref["ev_open"]
    assert np.array_equal(m32["event"][closed], ref["event"][closed])
    same = (m32["event"] == ref["event"]) & ~ref["open"]
    live = same & (ref["event"] != RF.INVALID)
    err_d = np.abs(m32["dir"].astype(np.float64) - ref["dir"]).max(-1)
    err_F = np.abs(m32["F"].astype(np.float64) - ref["F"])
    err_W = np.abs(m32["weight"].astype(np.float64) - ref["weight"])
    print(f"float32 model: {int((m32['event'] != ref['event']).sum())} of {len(closed)} rows change their event; worst error / bound: direction "
          f"{np.max(err_d[same] / ref['d_dir'][same]):.4f} ({err_d[same].max() / U24:.0f} u), F {np.max(err_F[same] / np.maximum(ref['dF'][same], U24)):.4f} "
          f"({err_F[same].max() / U24:.0f} u), weight {np.max(err_W[live] / ref['dW'][live]):.4f} ({err_W[live].max() / U24:.0f} u)")
    assert np.all(err_d[same] <= ref["d_dir"][same]) and np.all(err_F[same] <= ref["dF"][same] + U24) and np.all(err_W[live] <= ref["dW"][live])


# ---------------------------------------------------------------------------------------------------------------- the rule's limits
def test_the_rule_tends_to_the_smooth_event_as_alpha_goes_to_zero():
    rng, d, n = random_rows(4000, 5)
    ior, thin, u = rng.uniform(1.0, 2.0, len(d)), rng.integers(0, 2, len(d)), rng.random(len(d))
    tr, gdir, gF = RG.glass_event(ior, thin, d, n, u)
    ev, fdir, fF, w = RF.frost_event(ior, thin, d, n, 1e-7, u, rng.random(len(d)), rng.random(len(d)))
    ud = d / np.linalg.norm(d, axis=1, keepdims=True)
    # away from grazing incidence, the critical angle and u = F, where 1e-7 of roughness can still change the outcome
    c = np.abs(np.sum(n * ud, -1))
    eta = np.where((thin != 0) | (np.sum(n * ud, -1) < 0), ior, 1.0 / ior)
    safe = (c > 1e-2) & (np.abs(1.0 - (1.0 - c * c) / eta**2) > 1e-3) & (np.abs(u - gF) > 1e-4)
    assert safe.mean() > 0.9 and np.array_equal(ev[safe], tr[safe].astype(np.int64))
    assert np.abs(fdir - gdir)[safe].max() < 1e-4 and np.abs(fF - gF)[safe].max() < 1e-4 and np.abs(w[safe] - 1.0).max() < 1e-9
    # and alpha = 0 exactly is the smooth event itself
    ev0, dir0, F0, w0 = RF.frost_event(ior, thin, d, n, 0.0, u, 0.5, 0.5)
    assert np.array_equal(ev0, tr.astype(np.int64)) and np.array_equal(dir0, gdir) and np.array_equal(F0, gF) and np.all(w0 == 1.0)


@pytest.mark.parametrize("alpha", RF.ALPHAS)
def test_an_index_matched_solid_surface_keeps_the_direction_and_weighs_g1(alpha):
    """ior = 1: F = 0 at every micro-normal, t = -wo, so the direction is ud and the weight G1(cos, alpha^2) for every u2, u3"""
    rng, d, n = random_rows(2000, 7)
    ud = d / np.linalg.norm(d, axis=1, keepdims=True)
    cos = np.abs(np.sum(n * ud, -1))
    ev, out, F, w = RF.frost_event(1.0, 0, d, n, alpha, rng.random(len(d)), rng.random(len(d)), rng.random(len(d)))
    ok = cos > 1e-4
    assert np.all(F[ok] == 0.0) and np.all(ev[ok] == RF.TRANSMIT) and np.abs(out - ud)[ok].max() < 1e-12
    assert np.abs(w - R.smith_g1(alpha, cos))[ok].max() < 1e-9


@pytest.mark.parametrize("alpha", RF.ALPHAS)
@pytest.mark.parametrize("thin", (0, 1))
def test_the_mean_weight_never_exceeds_one(alpha, thin):
    """energy: at fixed (cos, alpha, ior) the mean over the draws of the weight (0 for an invalid sample) is at most 1 -- single scattering
    loses the invalid share and the masked part, and creates nothing"""
    rng = np.random.default_rng(11)
    m = 20000
    for cos in (0.05, 0.3, 0.7, 1.0):
        for side in (-1.0, 1.0):
            d = np.tile([np.sqrt(1.0 - cos * cos), 0.0, -side * cos], (m, 1))
            ev, _, _, w = RF.frost_event(1.5, thin, d, np.tile([0.0, 0.0, 1.0], (m, 1)), alpha, rng.random(m), rng.random(m), rng.random(m))
            assert np.all(w <= 1.0) and np.all(w[ev == RF.INVALID] == 0.0) and w.mean() <= 1.0


def test_the_invalid_share_grows_with_alpha():
    """the energy single scattering loses: about 1 % of the samples at alpha 0.05, about a fifth at alpha 1 (uniformly random directions,
    ior in [1, 2], both sides and wall kinds: the rows of op 38)"""
    (ior, thin, d, n, alpha, u, u2, u3), ref = op38()
    share = [float((ref["event"][alpha == np.float32(a)] == RF.INVALID).mean()) for a in RF.ALPHAS]
    print("invalid share by alpha:", dict(zip(RF.ALPHAS, np.round(share, 4))))
    assert share == sorted(share) and share[0] < 0.03 and 0.15 < share[-1] < 0.30


# ---------------------------------------------------------------------------------------------------------------- classification
def test_classification_survives_the_gltf_round_trip(tmp_path):
    """mode off: none; roughness 0 without a texture: none; a texture alone: frosted; what is frosted is what the loader gives back"""
    mesh = FW.textured_room()
    k = mesh.names.index("block")
    mesh.geometries["roughness"][k] = 0.0  # the texture alone
    FW.set_roughness(mesh, pane=0.0)
    assert not RF.frosted(mesh, on=False).any()
    assert np.flatnonzero(RF.frosted(mesh)).tolist() == [k]
    mesh.material_textures["metallic_roughness_texture"][k] = -1
    assert not RF.frosted(mesh).any()
    rough = FW.frost_room(True, 1.0)
    want = sorted(rough.names.index(n) for n in ("block", "pane"))
    assert np.flatnonzero(RF.frosted(rough)).tolist() == want
    assets.write_glb(tmp_path / "f.glb", rough)
    back = assets.load(tmp_path / "f.glb")
    assert np.flatnonzero(RF.frosted(back)).tolist() == want
    assert np.array_equal(back.geometries["roughness"], rough.geometries["roughness"]) and back.transmission.tobytes() == rough.transmission.tobytes()


def test_the_native_loader_reads_the_same_roughness(tmp_path):
    import subprocess

    from test_glass_cpu import native_tool

    rough = FW.frost_room(True, 1.0)
    assets.write_glb(tmp_path / "f.glb", rough)
    subprocess.run([native_tool(), "glb", str(tmp_path / "f.glb"), str(tmp_path)], check=True, capture_output=True)
    got_t = np.fromfile(tmp_path / "transmission.bin", assets.TRANSMISSION_DTYPE)
    got_g = np.fromfile(tmp_path / "geometries.bin", assets.GEOMETRY_DTYPE)
    assert got_t.tobytes() == rough.transmission.tobytes() and np.array_equal(got_g["roughness"], rough.geometries["roughness"])


def test_the_interface_is_declared_everywhere():
    header = (ROOT / "include" / "rt3.h").read_text()
    for name in ("rt3_scene_set_rough_transmission", "rt3_scene_get_rough_transmission", "rt3_rough_transmission_info"):
        assert name in L.EXPORTS and re.search(r"\bint " + name + r"\(", header)
    from raytracer3_amd import scenes
    from raytracer3_amd.render_graph import Context
    from raytracer3_amd.renderer import PathTracer

    assert all(hasattr(Context, n) for n in ("set_rough_transmission", "get_rough_transmission", "rough_transmission_info"))
    assert hasattr(PathTracer, "set_rough_transmission") and L.SELFTEST_FROST == 38
    mesh, clear = scenes.frosted_cornell(), scenes.glass_cornell()
    r = dict(zip(mesh.names, mesh.geometries["roughness"]))
    assert abs(r["glass_sphere"] - 0.3) < 1e-6 and abs(r["glass_pane"] - 0.15) < 1e-6 and mesh.transmission.tobytes() == clear.transmission.tobytes()
    assert "--rough-glass" in (ROOT / "tools" / "render.py").read_text() and (ROOT / "tools" / "time_frost.py").exists()


# ---------------------------------------------------------------------------------------------------------------- fixture
def test_fixture_is_sized_and_arrays_only():
    fx = fixture()
    assert GOLDEN.stat().st_size <= (GOLDEN.parent / "glass_ref.npz").stat().st_size
    for name, case in FW.ROOM_CASES.items():
        spp, seed = case[4], case[5]
        assert int(fx[f"{name}_spp"].item()) == spp and int(fx[f"{name}_seed"].item()) == seed
        assert fx[f"{name}_mean"].shape == fx[f"{name}_se"].shape == (2, 3, 3)
        assert np.all(fx[f"{name}_mean"] > 0) and np.all(fx[f"{name}_se"] > 0) and fx[f"{name}_cover"].all()
        # the fixture alone resolves 2 %: 0.02 x mean is beyond the band (by the margin the noise of the code under test may take)
        assert np.mean(0.02 * fx[f"{name}_mean"] > (Z_MAX + 1.0) * fx[f"{name}_se"]) >= 0.9
    assert fx["edge_mean"].shape == fx["edge_se"].shape == (FW.EDGE_WINDOW[0], 3)
    assert {c[1] for c in FW.ROOM_CASES.values()} == {4, 6}


def test_generator_has_not_drifted():
    """the first CHUNK_SPP samples of one case, rendered again with the stored seed, give the stored prefix statistics"""
    spec = importlib.util.spec_from_file_location("gen_frost_ref", GOLDEN.parent / "gen_frost_ref.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fx = fixture()
    name = gen.PREFIX_CASE
    bm, se = gen.render_prefix(name, RP.CHUNK_SPP)
    assert np.allclose(bm, fx[f"{name}_prefix_mean"], rtol=1e-9, atol=0.0) and np.allclose(se, fx[f"{name}_prefix_se"], rtol=1e-9, atol=0.0)


def test_the_room_has_what_the_cases_are_about():
    mesh = FW.frost_room(True, 1.0)
    r = dict(zip(mesh.names, mesh.geometries["roughness"]))
    assert abs(r["block"] - 0.3) < 1e-6 and abs(r["pane"] - 0.2) < 1e-6
    t = mesh.transmission
    assert t["thin_walled"][mesh.names.index("block")] == 0 and t["thin_walled"][mesh.names.index("pane")] == 1
    assert GW.glass_room(True, 1.0).transmission.tobytes() == t.tobytes()
