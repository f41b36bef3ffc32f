"""tests/ref_lens.py against the closed forms the GPU tests of tests/test_lens.py use, with numpy's own random numbers, and the fixture
tests/golden/lens_ref.npz against its generator.  No GPU.

Every sample of the flat emitters of lens_worlds is 0 or Le, so a pixel mean over S samples is binomial: it lies within
5 Le sqrt(a (1 - a) / S) of a Le (a: the closed-form coverage) but for 6e-7 of the cases, and is exact where a is 0 or 1."""
import importlib.util
from pathlib import Path

import numpy as np

import integrator_worlds as IW
import lens_worlds as LW
import ref_lens as RL
import ref_pathtrace as RP
from test_integrator_cpu import Z_MAX

GOLDEN = Path(__file__).resolve().parent / "golden" / "lens_ref.npz"
PINV, VINV = RL.camera_matrices(LW.CAMERA, LW.WINDOW)


def band(a, S):
    return 5.0 * np.sqrt(a * (1.0 - a) / S)


def hit_share(mesh, lens, S, seed):
    """(H, W): the share of S camera samples per pixel that hit the mesh"""
    W, H = LW.WINDOW
    sc = RP.Scene(mesh)
    py, px = np.mgrid[0:H, 0:W]
    px, py = np.tile(px.reshape(-1), S), np.tile(py.reshape(-1), S)
    o, d, _, _ = RL.camera_sample(PINV, VINV, LW.WINDOW, lens, px, py, np.random.default_rng(seed).random((len(px), 4)))
    return (sc.trace(o, d)[0] >= 0).reshape(S, H, W).mean(0)


def test_camera_matrices_are_the_pinhole_of_ref_pathtrace():
    W, H = LW.WINDOW
    py, px = np.mgrid[0:H, 0:W]
    o, d, film, lens = RL.camera_sample(PINV, VINV, LW.WINDOW, (0.0, 1.0, 0.0), px.reshape(-1), py.reshape(-1), np.zeros((W * H, 4)))
    o0, d0 = RP.primary_rays(LW.CAMERA, LW.WINDOW)
    assert np.abs(o - o0).max() == 0.0 and np.abs(d - d0).max() < 1e-15
    assert np.array_equal(film, np.stack([px.reshape(-1) + 0.5, py.reshape(-1) + 0.5], -1)) and not lens.any()


def test_projection_inverts_the_scene_builder():
    c = LW.rect_corners()
    pts = LW.pixel_to_world(c[:, 0], c[:, 1], LW.RECT_DEPTH)
    assert np.abs(LW.project(PINV, VINV, pts) - c).max() < 1e-12


def test_lens_points_and_focus():
    rng = np.random.default_rng(3)
    n = 4096
    u = rng.random((n, 4))
    R_, F = 0.3, 4.0
    px, py = np.full(n, 7), np.full(n, 11)
    o, d, film, l = RL.camera_sample(PINV, VINV, LW.WINDOW, (R_, F, 0.0), px, py, u)
    assert np.all(np.hypot(l[:, 0], l[:, 1]) <= R_)
    assert np.abs(np.linalg.norm(d, axis=-1) - 1.0).max() < 1e-15
    # every ray passes through the one focus point
    P = RL.focus_point(PINV, VINV, LW.WINDOW, F, 7, 11)[0]
    w = P - o
    assert np.linalg.norm(w - np.sum(w * d, -1, keepdims=True) * d, axis=-1).max() < 1e-13
    # uniform in area: |l|^2 / R^2 is uniform on [0, 1]
    assert abs(np.mean(np.sum(l * l, -1) / R_**2) - 0.5) <= 5.0 * np.sqrt(1.0 / 12.0 / n)


def test_antialiasing_closed_form():
    S = 512
    for rot, jitter in ((0.0, 1.0), (25.0, 1.0), (0.0, 0.5)):
        corners = LW.rect_corners(rot_deg=rot)
        mesh, world = LW.quad(corners, LW.RECT_DEPTH)
        poly = LW.project(PINV, VINV, world)
        a = RL.polygon_coverage(poly, LW.WINDOW, jitter)
        if rot == 0.0:  # the two coverage functions agree on an axis-aligned rectangle
            box = RL.box_coverage(poly[:, 0].min(), poly[:, 0].max(), poly[:, 1].min(), poly[:, 1].max(), LW.WINDOW, jitter)
            assert np.abs(a - box).max() < 1e-12
        got = hit_share(mesh, (0.0, 1.0, jitter), S, seed=int(rot) + 7)
        assert np.all(np.abs(got - a) <= band(a, S) + 1e-12)
        assert np.all(got[a < 1e-12] == 0.0) and np.all(got[a > 1.0 - 1e-12] == 1.0)
        assert ((a > 0.01) & (a < 0.99)).sum() >= 20, "the rectangle has partly covered pixels"


def test_thin_lens_closed_form():
    W, H = LW.WINDOW
    S = 128
    for name, z in LW.HALF_PLANE_DEPTHS:
        mesh, world = LW.half_plane(z)
        e = LW.project(PINV, VINV, world)[0, 0]
        r = RL.coc_radius_px(LW.LENS_R, LW.LENS_F, z, LW.CAMERA["fov_deg"], H)
        a = RL.half_plane_columns(e, r, W)
        got = hit_share(mesh, (LW.LENS_R, LW.LENS_F, 1.0), S, seed=11).mean(0)  # the rows of a column pooled
        z_col = (got - a) / np.maximum(np.sqrt(a * (1.0 - a) / (S * H)), 1e-300)
        print(f"half-plane {name}: z = {z}, circle of confusion {r:.3f} px, edge at {e:.3f}; worst column {np.abs(z_col[(a > 0) & (a < 1)]).max():.2f} sigma")
        assert np.all(np.abs(got - a) <= band(a, S * H) + 1e-12)
        assert (r == 0.0) == (name == "sharp")
        # the blur keeps the flux: the frame's sum is the pinhole's
        assert abs(got.sum() - (W - e)) <= 5.0 * np.sqrt(np.sum(a * (1.0 - a)) / (S * H)) + 1e-12


def test_disk_edge_response_is_a_distribution():
    r = 2.5
    s = np.linspace(-4.0, 4.0, 1601)
    G = RL.disk_edge_G(s, r)
    dG = np.gradient(G, s)
    assert np.all(np.diff(G) >= -1e-15) and G[0] == 0.0 and G[-1] == s[-1]
    assert np.all(dG > -1e-9) and np.all(dG < 1.0 + 1e-9)
    # the derivative at the centre is half the disk
    assert abs(dG[800] - 0.5) < 1e-5


def test_textured_surface_without_textures_is_the_plain_tracer():
    """ref_lens.textured_surface (barycentrics from the hit point, primitive order, ref_materials' surfaces, the per-row layered BSDF) on
    the textured room with its material-texture table cleared: the same samples as the per-geometry constants give"""
    import material_worlds as MW
    from raytracer3_amd import assets

    mesh, cam = LW.material_room()
    mesh = MW.with_tables(mesh, material_textures=assets.no_material_textures(len(mesh.geometries)))
    sc = RP.Scene(mesh)
    pinv, vinv = RL.camera_matrices(cam, IW.WINDOW_ROOM)
    flags, bounces = LW.MATERIAL_CASES["lens_mat_b2"][:2]
    a = RL.radiance_samples(sc, pinv, vinv, IW.WINDOW_ROOM, LW.MATERIAL_LENS, flags, bounces + 1, 2, np.random.default_rng(9))
    b = RL.radiance_samples(sc, pinv, vinv, IW.WINDOW_ROOM, LW.MATERIAL_LENS, flags, bounces + 1, 2, np.random.default_rng(9), RL.textured_surface(mesh, sc))
    assert a.max() > 0.0 and np.abs(a - b).max() <= 1e-9 * a.max()


# ---------------------------------------------------------------------------------------------------------------- fixture
def fixture():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def test_fixture_is_sized_and_arrays_only():
    fx = fixture()
    assert GOLDEN.stat().st_size < 64 * 1024
    for name, (_, _, _, spp, seed, _) in {**LW.ROOM_CASES, **LW.MATERIAL_CASES}.items():
        assert int(fx[f"{name}_spp"].item()) == spp and int(fx[f"{name}_seed"].item()) == seed
        assert fx[f"{name}_mean"].shape == fx[f"{name}_se"].shape == (2, 3, 3)
        assert fx[f"{name}_cover"].all() and fx[f"{name}_cover"].shape == IW.WINDOW_ROOM[::-1]
        assert np.all(fx[f"{name}_mean"] > 0) and np.all(fx[f"{name}_se"] > 0)
        # the fixture alone resolves 2 %: 0.02 x mean is beyond the band (by the margin the noise of the code under test may take)
        assert np.mean(0.02 * fx[f"{name}_mean"] > (Z_MAX + 1.0) * fx[f"{name}_se"]) >= 0.9


def test_generator_has_not_drifted():
    """the first CHUNK_SPP samples of one case, rendered again with the stored seed, give the stored prefix statistics"""
    spec = importlib.util.spec_from_file_location("gen_lens_ref", GOLDEN.parent / "gen_lens_ref.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fx = fixture()
    name = "lens_sky_b4"
    bm, se = gen.render_prefix(name, RP.CHUNK_SPP)
    assert np.allclose(bm, fx[f"{name}_prefix_mean"], rtol=1e-9, atol=0.0)
    assert np.allclose(se, fx[f"{name}_prefix_se"], rtol=1e-9, atol=0.0)
