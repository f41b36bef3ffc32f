"""Fog without a GPU: the float64 restatement of the rule agrees with itself (the density integrates to 1 and the
inversion inverts it; the float32 segment equals the float64 one away from ties), the closed forms of tests/fog_worlds.py agree with the
quadrature of the integral, the reference estimator alone meets the quadrature within the tolerance tests/test_fog.py holds the GPU to, and
the interface is declared where the bindings expect it."""
import re
from pathlib import Path

import numpy as np
import pytest

import fog_worlds as FW
import ref_fog as RF
from raytracer3_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
N_REF = 256  # samples per pixel of the lamp and occluder frames, here and on the GPU


def op45_rows(n=6000, seed=11):
    """{o, d, t, lo, hi, sigma_a, sigma_s, u}: origins inside and outside a box, directions towards it, past it and along its faces (a
    component exactly 0, the origin on the face's plane or beside it), t inside the box, behind it and +inf, |d| from 0.5 to 2, sigma_t len
    from 0 (a tenth of the rows, and a quarter of the channels) over below the uniform threshold to thick (beyond 40)"""
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-2.0, 0.0, (n, 3))
    hi = lo + rng.uniform(0.5, 3.0, (n, 3))
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    o = c + e * rng.uniform(-3.0, 3.0, (n, 3))
    o[: n // 4] = (c + e * rng.uniform(-0.95, 0.95, (n, 3)))[: n // 4]  # inside
    target = c + e * rng.uniform(-1.4, 1.4, (n, 3))
    d = target - o
    d *= (rng.uniform(0.5, 2.0, n) / np.linalg.norm(d, axis=1))[:, None]
    graze = rng.random(n) < 0.15  # along a face: one component exactly 0, the origin on the face's plane, inside or outside the slab
    k = rng.integers(0, 3, n)
    rows_g = np.flatnonzero(graze)
    d[rows_g, k[rows_g]] = 0.0
    pick = rng.integers(0, 4, n)
    face = np.where(pick == 0, lo[np.arange(n), k], np.where(pick == 1, hi[np.arange(n), k], np.where(pick == 2, c[np.arange(n), k], hi[np.arange(n), k] + 0.25)))
    o[rows_g, k[rows_g]] = face[rows_g]
    t = rng.uniform(0.05, 8.0, n)
    t[rng.random(n) < 0.3] = np.inf
    a = 160.0 * rng.random((n, 3)) ** 2
    a[rng.random(n) < 0.1] *= 1e-9  # below the uniform threshold
    sig = a / np.maximum(np.linalg.norm(hi - lo, axis=1), 1e-3)[:, None]
    sig[rng.random((n, 3)) < 0.25] = 0.0
    sig[rng.random(n) < 0.1] = 0.0
    albedo = rng.random((n, 3))
    u = np.floor(rng.random(n) * 2.0**23) / 2.0**23
    return np.concatenate([o, d, t[:, None], lo, hi, sig * (1 - albedo), sig * albedo, u[:, None]], 1).astype(np.float32)


def test_rows_cover_the_cases():
    rows = op45_rows()
    ref = RF.rule_rows(rows)
    hit = ref["hit"]
    inside = np.all((rows[:, 0:3] >= rows[:, 7:10]) & (rows[:, 0:3] <= rows[:, 10:13]), 1)
    cut = hit & (ref["t1"] == rows[:, 6])
    graze = np.any(rows[:, 3:6] == 0, 1)
    assert 0.3 < hit.mean() < 0.9 and (inside & hit).sum() > 800 and (~inside & hit).sum() > 800 and (~hit).sum() > 500
    assert cut.sum() > 300 and (graze & hit).sum() > 100 and (graze & ~hit).sum() > 100
    assert (hit & (ref["a"].max(1) > 40)).sum() > 50 and (hit & (ref["ab"] > 20)).sum() > 50 and (hit & (ref["ab"] < RF.UNIFORM_BELOW)).sum() > 100 and (hit & (ref["ab"] == 0)).sum() > 50


def test_float32_segment_is_the_float64_one_away_from_ties():
    rows = op45_rows()
    o, d, t, lo, hi = rows[:, 0:3], rows[:, 3:6], rows[:, 6], rows[:, 7:10], rows[:, 10:13]
    h32, a32, b32 = RF.span32(o, d, t, lo, hi)
    h64, a64, b64 = RF.span(o, d, t, lo, hi)
    clear = h64 & (b64 - a64 > 1e-4 * (1.0 + np.abs(b64)))
    assert np.all(h32[clear]) and clear.sum() > 3000
    assert np.all(np.abs(a32[clear] - a64[clear]) <= 4 * RF.U * (1.0 + np.abs(a64[clear]) + np.abs(b64[clear])))
    assert np.all(np.abs(b32[clear] - b64[clear]) <= 4 * RF.U * (1.0 + np.abs(a64[clear]) + np.abs(b64[clear])))


def test_density_integrates_to_one_and_inverts():
    for sb, length in ((0.4, 3.0), (5.0, 2.0), (1e-9, 1.0), (40.0, 2.0)):
        u = (np.arange(4096) + 0.5) / 4096
        ds, pdf = RF.sample_distance(sb, length, u)
        assert np.all((ds >= 0) & (ds <= length))
        a = sb * length
        cdf = -np.expm1(-sb * ds) / -np.expm1(-a) if a >= RF.UNIFORM_BELOW else ds / length
        assert np.abs(cdf - u).max() < 1e-9
        r = (np.arange(200000) + 0.5) / 200000 * length
        dens = sb * np.exp(-sb * r) / -np.expm1(-a) if a >= RF.UNIFORM_BELOW else np.full_like(r, 1.0 / length)
        assert abs(dens.mean() * length - 1.0) < 1e-6


def test_phase_function_integrates_to_one():
    c = (np.arange(200000) + 0.5) / 100000 - 1.0
    for g in (0.0, 0.6, -0.8):
        assert abs(RF.phase(g, c).mean() * 2.0 * 2.0 * np.pi - 1.0) < 1e-6


def rays():
    d = FW.pixel_dirs().reshape(-1, 3)
    return np.asarray(FW.CAMERA["position"], np.float64), d


def test_closed_forms_agree_with_the_quadrature():
    o, d = rays()
    W, H = FW.WINDOW
    row = slice(FW.CENTRE_ROW * W, (FW.CENTRE_ROW + 1) * W)
    for g in (0.0, 0.6):
        _, med = FW.medium(g=g)
        q = RF.quadrature(o, d[row], np.inf, med, RF.Directional((0, -1, 0), FW.SUN_E), n=512)
        want, l, h = FW.shaft_centre_row(g)
        assert abs(h - 1.0) < 1e-12 and l.min() >= 2.0 and np.abs(q / want - 1.0).max() < 1e-5
    _, med = FW.medium()
    q = RF.quadrature(o, d[row], np.inf, med, RF.Directional((0, -1, 0), FW.SUN_E), FW.lit, n=4096)
    want, share = FW.shadowed_centre_row()
    assert (share == 0).sum() >= 4 and (share == 1).sum() >= 4 and ((share > 0.05) & (share < 0.95)).sum() >= 2
    assert np.abs(q - want).max() <= 2e-3 * want.max()
    assert np.all(np.isinf(FW.occluder_t_end()) | (FW.occluder_t_end() > 0))


# kind -> (camera, g, light, visibility): the frames tests/test_fog.py renders at N_REF samples
CASES = {
    "sun": (FW.CAMERA, 0.6, lambda: RF.Directional((0, -1, 0), FW.SUN_E), None),
    "lamp": (FW.TILTED_CAMERA, 0.0, lambda: RF.Point(FW.LAMP_P, FW.LAMP_I), None),
    "occluder": (FW.CAMERA, 0.0, lambda: RF.Directional((0, -1, 0), FW.SUN_E), FW.lit),
    "panel": (FW.TILTED_CAMERA, 0.3, lambda: RF.Panel(*FW.PANEL, 12.0 * np.asarray(FW.PANEL_EMISSION)), None),
}
N_QUAD = {"sun": 1024, "lamp": 1024, "occluder": 1024, "panel": 192}
_REFERENCE = {}


def reference(kind):
    """(quadrature (H W, 3), the float64 estimator's mean of N_REF samples, its standard error, edge (H W, 3): the quadrature's own error
    where the integrand jumps), computed once.  Only a ray that crosses the occluder's edge inside the slab has such a jump: the midpoint
    rule puts at most one of its N cells on the wrong side, an error of at most one cell's width len / N times the integrand there, which
    is at most e^(sigma_t len) < 4 times its mean q_lit / len over the ray: 4 q_lit / N, q_lit the quadrature without the occluder.
    The smooth part of every integrand carries the midpoint rule's own error, at most len^2 / (24 N^2) times the second derivative's
    share: with K = 12 for the relative rate of change per length of the ray (sigma_t len <= 1.2, the phase function's and the inverse
    square's variation over the ray a few units each), K^2 / (24 N^2) = 6 / N^2 of q: 6e-6 at N = 1024.  It matters only where the
    estimator is constant and its standard error 0 (the horizontal row under the sun).  Beside these two the tolerance is 6 standard
    errors alone."""
    if kind not in _REFERENCE:
        cam, g, make_light, visible = CASES[kind]
        o = np.asarray(cam["position"], np.float64)
        d = FW.pixel_dirs(cam=cam).reshape(-1, 3)
        _, med = FW.medium(g=g)
        light = make_light()
        q = RF.quadrature(o, d, np.inf, med, light, visible, n=N_QUAD[kind])
        mean, se = RF.estimator(o, d, np.inf, med, light, N_REF, np.random.default_rng(17), visible)
        edge = 6.0 / N_QUAD[kind] ** 2 * q
        if visible is not None:
            ok, t0, t1 = RF.span(o, d, np.inf, med[3], med[4])
            x0, x1 = o[0] + t0 * d[:, 0], o[0] + t1 * d[:, 0]
            crosses = ok & ((x0 - FW.EDGE_X) * (x1 - FW.EDGE_X) < 0)
            edge = edge + crosses[:, None] * 4.0 / N_QUAD[kind] * RF.quadrature(o, d, np.inf, med, light, None, n=256)
        _REFERENCE[kind] = (q, mean, se, edge)
    return _REFERENCE[kind]


def check_estimator(kind):
    """the reference estimator's mean of N_REF samples lies within 6 of its own standard errors of the quadrature, in every pixel"""
    q, mean, se, edge = reference(kind)
    ok = np.abs(mean - q) <= 6.0 * se + edge
    assert ok.all(), (int((~ok).sum()), float((np.abs(mean - q) / np.maximum(6.0 * se + edge, 1e-300)).max()))
    return q, se


def test_reference_estimator_meets_the_quadrature_under_the_lamp():
    """the tilted view: four rays in ten leave the slab through its bottom"""
    q, se = check_estimator("lamp")
    assert q.min(1).max() > 0 and np.median((se / np.maximum(q, 1e-300))[q > 0]) < 0.1
    d = FW.pixel_dirs(cam=FW.TILTED_CAMERA).reshape(-1, 3)
    ok, t0, t1 = RF.span(FW.TILTED_CAMERA["position"], d, np.inf, *FW.SLAB)
    y1 = FW.TILTED_CAMERA["position"][1] + t1 * d[:, 1]
    assert (ok & (np.abs(y1) < 1e-9)).mean() > 0.3


def test_reference_estimator_meets_the_quadrature_under_the_sun():
    check_estimator("sun")


def test_reference_estimator_meets_the_quadrature_under_the_occluder():
    q, _ = check_estimator("occluder")
    assert (q.max(1) == 0).sum() > 50 and (q.max(1) > 0).sum() > 500
    assert 10 < (reference("occluder")[3].max(1) > 1e-4 * q.max()).sum() < 400


def test_reference_estimator_meets_the_quadrature_under_the_panel():
    q, se = check_estimator("panel")
    assert (q.min(1) > 0).mean() > 0.8 and np.median((se / np.maximum(q, 1e-300))[q > 0]) < 0.1


@pytest.mark.parametrize("kind", ("sun", "lamp", "panel"))
def test_doubling_the_quadrature_moves_it_by_less_than_its_error_term(kind):
    """the 6 / N^2 of q that reference() allows for the midpoint rule: the rule's error falls by four when N doubles, so q_N - q_2N is three
    quarters of q_N's error and must lie inside the term (every eighth ray)"""
    cam, g, make_light, visible = CASES[kind]
    o = np.asarray(cam["position"], np.float64)
    d = FW.pixel_dirs(cam=cam).reshape(-1, 3)[::8]
    _, med = FW.medium(g=g)
    n = N_QUAD[kind]
    q1, q2 = (RF.quadrature(o, d, np.inf, med, make_light(), visible, n=k) for k in (n, 2 * n))
    assert q2.max() > 0 and np.all(np.abs(q1 - q2) <= 6.0 / n**2 * q2)


# ---------------------------------------------------------------------------------------------------------------- the fogged room's fixture
GOLDEN = ROOT / "tests" / "golden" / "fog_ref.npz"
Z_MAX = 4.5  # test_integrator_cpu's


def fixture():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def generator():
    import importlib.util

    spec = importlib.util.spec_from_file_location("gen_fog_ref", ROOT / "tests" / "golden" / "gen_fog_ref.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_fixture_is_sized_and_arrays_only():
    import ref_pane_shadows as RPS

    fx = fixture()
    assert GOLDEN.stat().st_size < 64 * 1024
    with np.load(GOLDEN, allow_pickle=False) as f:
        assert all(f[k].dtype.kind in "fib" for k in f.files)
    for name, case in FW.ROOM_CASES.items():
        assert int(fx[f"{name}_spp"].item()) == case[2] and int(fx[f"{name}_seed"].item()) == case[3]
        assert fx[f"{name}_mean"].shape == fx[f"{name}_se"].shape == (2, 3, 3) and fx[f"{name}_cover"].all()
        assert np.all(fx[f"{name}_mean"] > 0) and np.all(fx[f"{name}_se"] > 0)
        # the fixture alone resolves 2 % (test_integrator_cpu's criterion)
        assert np.mean(0.02 * fx[f"{name}_mean"] > (Z_MAX + 1.0) * fx[f"{name}_se"]) >= 0.9
    mesh = FW.fog_room()
    assert len(mesh.indices) // 3 <= 30 and RPS.pane_table(mesh).sum() == 1 and len(mesh.lights) == 2
    assert mesh.material_textures["emissive_texture"][mesh.names.index("lamp")] == 0 and (mesh.material_textures["emissive_texture"] >= 0).sum() == 1


def test_generator_has_not_drifted_and_the_fixture_sees_the_fog():
    """the first chunk of the case, rendered again with the stored seed, gives the stored prefix statistics; rendered without a medium, and
    with the medium's scattering turned into absorption (no in-scattered light), it lies many standard errors off: the fixture holds both
    the attenuation and the in-scatter"""
    import ref_pathtrace as RP

    gen, fx, name = generator(), fixture(), "fog_room_b5"
    mean, se = gen.render_prefix(name, RP.CHUNK_SPP)
    assert np.allclose(mean, fx[f"{name}_prefix_mean"], rtol=1e-12, atol=0) and np.allclose(se, fx[f"{name}_prefix_se"], rtol=1e-9, atol=0)
    st, ss, g, lo, hi = FW.room_medium()[1]
    clear, se_c = gen.render_prefix(name, RP.CHUNK_SPP, (0.0 * st, 0.0 * ss, g, lo, hi))
    dark, se_d = gen.render_prefix(name, RP.CHUNK_SPP, (st, 0.0 * ss, g, lo, hi))
    z_clear, z_dark = (clear - mean) / np.hypot(se, se_c), (mean - dark) / np.hypot(se, se_d)
    print(f"clear / fogged {np.round((clear / mean).reshape(-1), 2)}; fogged / absorbing only {np.round((mean / dark).reshape(-1), 2)}")
    assert z_clear.min() > 2 * Z_MAX and z_dark.min() > 2 * Z_MAX


def test_interface_is_declared():
    header = (ROOT / "include" / "rt3.h").read_text()
    for name in ("rt3_scene_set_medium", "rt3_scene_get_medium", "rt3_medium_info"):
        assert re.search(rf"\bint {name}\(", header) and name in L.EXPORTS
    assert L.SELFTEST_FOG == 45 and L.SELFTEST_FOG_QUEUE == 46
    m = L.Medium(0.1, (0.3, 0.2, 0.1), 0.5, (-1, -2, -3), (1, 2, 3))
    assert list(m.sigma_a) == [np.float32(0.1)] * 3 and abs(m.sigma_s[1] - 0.2) < 1e-7 and m.g == 0.5 and m.box_max[2] == 3.0
    src = (ROOT / "raytracer3_amd" / "csrc" / "rt3_fog.hpp").read_text()
    assert "kFogRngBase = 0x70000000u" in src
