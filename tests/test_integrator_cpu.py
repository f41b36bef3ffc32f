"""The path tracer as a whole against two witnesses that share no code with it, with the CPU oracle as the backend;
tests/test_integrator.py runs the same checks on the GPU.

(a) Furnace: in a closed room where every surface has albedo rho and emission E, every path sample is
        L = E0 + rho0 E sum_{k=0}^{B-2} rho^k        (E0, rho0: the first vertex's G-buffer-quantised values)
    whatever the directions drawn.  A pixel either matches that within the rounding of its products and sums, or it lost a path through
    one of the two leaks of DESIGN.md section 10 and is LOW; none may be high, and the low share is capped.
(b) Open room: block means against tests/golden/integrator_ref.npz, rendered once by the float64 tracer of tests/ref_pathtrace.py
    (another estimator of the same integral: no light sampling, no MIS), within 4.5 of the fixture's standard errors.  The code under
    test is rendered so long that its own noise is at most half the fixture's, so it cannot widen the band; a frame scaled by 1.02 must
    fail the same band in 90 % of the block-channels, so the band can see a 2 % error."""
import functools
from pathlib import Path

import numpy as np
import pytest

import integrator_worlds as IW
import orc
import ref_pathtrace as RP
import ref_shading as R

GOLDEN = Path(__file__).resolve().parent / "golden" / "integrator_ref.npz"
FF = orc.F_FACEFORWARD
LOW_CAP = 0.01  # share of furnace pixels that may be low: a condition on the scene, not a tolerance (the oracle's worst is 0.36 %)
Z_MAX = 4.5
FURNACE_BS = ((1, 1), (2, 4), (4, 16), (5, 3), (8, 16))


# ---------------------------------------------------------------------------------------------------------------- shared with the GPU file
def first_vertex(gb):
    """(rho0, E0) per pixel from the G-buffer words, in the decoders' own fp32 arithmetic: (q / 255)^2 and RGB9E5"""
    w = gb[..., 0]
    q = np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], -1).astype(np.float32) / np.float32(255.0)
    return (q * q).astype(np.float64), R.rgb9e5_decode(gb[..., 3])


def furnace_radiance(gb, bounces):
    rho, E = np.asarray(IW.FURNACE_ALBEDO, np.float32).astype(np.float64), RP.EMISSION_SCALE * np.asarray(IW.FURNACE_EMISSION, np.float32).astype(np.float64)
    rho0, E0 = first_vertex(gb)
    return E0 + rho0 * E * sum((rho**k for k in range(bounces - 1)), np.zeros(3))


def furnace_tolerance(bounces, samples):
    """one rounding per product and per sum: 2 per bounce, one per sample added, the division and the first vertex"""
    return (2 * bounces + samples + 2) * 2.0**-24


def check_furnace(light, gb, covered, bounces, samples, label):
    """asserts the furnace conditions on one frame; returns the number of low pixels"""
    assert covered.all(), "the furnace camera sees a surface in every pixel"
    want = furnace_radiance(gb, bounces)
    rel = light.astype(np.float64) / want - 1.0
    tol = furnace_tolerance(bounces, samples)
    high = (rel > tol).any(-1)
    low = (rel < -tol).any(-1)
    exact = ~high & ~low
    worst = np.abs(rel[exact]).max() if exact.any() else 0.0
    ratio = light.astype(np.float64).mean((0, 1)) / want.mean((0, 1))
    print(f"furnace {label} B={bounces} S={samples}: {int(low.sum())} of {low.size} pixels low ({low.mean():.2%}), {int(high.sum())} high, "
          f"exact pixels within {worst:.2e} (bound {tol:.2e}), frame mean / closed form {ratio.min():.6f}")
    assert not high.any(), f"{int(high.sum())} pixels above the closed form, worst {rel.max():+.3e}"
    assert low.mean() <= LOW_CAP
    assert np.all(ratio >= 1.0 - LOW_CAP) and np.all(ratio <= 1.0 + tol)
    return int(low.sum())


def blocks(x, block=16):
    """(..., H, W, 3) -> block means (..., H / 16, W / 16, 3)"""
    *lead, H, W, C = x.shape
    return x.reshape(*lead, H // block, block, W // block, block, C).mean((-4, -2))


def check_against_fixture(frames, covered, fx, name):
    """frames: (K, H, W, 3) independent frames of the code under test, uncovered pixels 0; returns the largest |z|"""
    assert np.array_equal(covered, fx[f"{name}_cover"]), "same pixels covered"
    ref, se_ref = fx[f"{name}_mean"], fx[f"{name}_se"]
    frames = np.asarray(frames, np.float64)
    got = blocks(frames.mean(0))
    # the standard error of the code under test from its K frames: per pixel (K - 1 degrees of freedom each), summed over the block as
    # the fixture's is -- pixels are independent, their random streams are seeded per pixel and frame
    se_got = np.sqrt(blocks(frames.var(0, ddof=1) / len(frames)) / 16**2)
    z = (got - ref) / se_ref
    z_scaled = (1.02 * got - ref) / se_ref
    power = float(np.mean(np.abs(z_scaled) >= Z_MAX))
    print(f"{name}: max |z| {np.abs(z).max():.2f} over {z.size} block-channels; own standard error / fixture's at most {np.max(se_got / se_ref):.2f}; "
          f"relative means {np.abs(got.mean((0, 1)) / ref.mean((0, 1)) - 1.0).max():.1e}; a 2 % error is rejected in {power:.0%}")
    assert np.all(se_got <= 0.5 * se_ref), "the code under test must be rendered to at most half the fixture's noise"
    assert np.abs(z).max() < Z_MAX
    assert power >= 0.9
    return float(np.abs(z).max())


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


# ---------------------------------------------------------------------------------------------------------------- oracle backend
def oracle_gconst(cam, window, flags, bounces, samples, frame=0):
    g = orc.camera_gconst(cam["position"], cam["direction"], cam["fov_deg"], window[0], window[1])
    g.bounces, g.samples, g.blendfactor, g.frame = bounces, samples, 1.0, frame
    g.pad[0] = flags
    return g


def oracle_frame(osc, cam, window, flags, bounces, samples, frame=0):
    g = oracle_gconst(cam, window, flags, bounces, samples, frame)
    gb, depth = osc.gbuffer(g)
    light, _ = osc.reference_mode(g, gb, depth)
    covered = depth != orc.BACKGROUND_DEPTH
    light = light[..., :3].copy()
    light[~covered] = 0.0
    return light, gb, covered


@functools.lru_cache(maxsize=None)
def furnace_scene(scale):
    mesh, _, cam = IW.furnace(scale)
    return orc.Scene(mesh), cam


# ---------------------------------------------------------------------------------------------------------------- (a) furnace
@pytest.mark.parametrize("bounces,samples", FURNACE_BS)
@pytest.mark.parametrize("flags", (0, FF))
def test_furnace_closed_form(flags, bounces, samples):
    osc, cam = furnace_scene(10.0)
    light, gb, covered = oracle_frame(osc, cam, IW.WINDOW_FURNACE, flags, bounces, samples)
    low = check_furnace(light, gb, covered, bounces, samples, f"oracle flags={flags}")
    if bounces == 1:
        assert low == 0, "one vertex: no ray is traced, nothing can leak"


def test_furnace_scale_law():
    """far from the origin the room stays tight without FACEFORWARD; with it the fp32 hit point falls behind its surface often enough
    to darken the frame.  The direction is asserted, the share is printed."""
    osc, cam = furnace_scene(1000.0)
    want = None
    shares = {}
    for flags in (0, FF):
        light, gb, covered = oracle_frame(osc, cam, IW.WINDOW_FURNACE, flags, 8, 16)
        assert covered.all()
        want = furnace_radiance(gb, 8)
        rel = light.astype(np.float64) / want - 1.0
        tol = furnace_tolerance(8, 16)
        assert not (rel > tol).any(), "no pixel is high"
        shares[flags] = float((rel < -tol).any(-1).mean())
    print(f"furnace at scale 1000, B = 8, S = 16: low pixels without FACEFORWARD {shares[0]:.2%}, with it {shares[FF]:.2%}")
    assert shares[0] == 0.0
    assert shares[FF] > 0.0


@pytest.mark.parametrize("flags,bounces", ((0, 4), (RP.F_FACEFORWARD, 8)))
def test_reference_tracer_on_furnace(flags, bounces):
    """the reference's own sanity: every one of its samples is the closed form.  At scale 1000, where no vertex of these 16 samples per
    pixel comes within T_MIN of an edge (the reference has the T_MIN gap too: it is part of the scene's definition)."""
    mesh, _, cam = IW.furnace(1000.0)
    sc = RP.Scene(mesh)
    v = RP.radiance_samples(sc, cam, IW.WINDOW_FURNACE, flags, bounces, 16, np.random.default_rng(1))
    rho, E = sc.albedo[0], sc.emission[0]
    want = sc.emission0[0] + sc.albedo0[0] * E * sum((rho**k for k in range(bounces - 1)), np.zeros(3))
    assert np.abs(v / want - 1.0).max() < 1e-12
    # and its first-vertex quantisation is the one the G-buffer words decode to
    osc, _ = furnace_scene(1000.0)
    _, gb, _ = oracle_frame(osc, cam, IW.WINDOW_FURNACE, flags, 1, 1)
    rho0, E0 = first_vertex(gb)
    assert np.abs(rho0 / sc.albedo0[0] - 1.0).max() < 4 * R.EPS32 and np.array_equal(E0, np.broadcast_to(sc.emission0[0], E0.shape))


# ---------------------------------------------------------------------------------------------------------------- (b) fixture
def test_fixture_is_sized_and_arrays_only():
    fx = fixture()
    assert GOLDEN.stat().st_size < 64 * 1024
    for name, (_, _, _, spp, seed, _) in IW.ROOM_CASES.items():
        assert int(fx[f"{name}_spp"].item()) == spp and int(fx[f"{name}_seed"].item()) == seed
        assert fx[f"{name}_mean"].shape == fx[f"{name}_se"].shape == (2, 3, 3)
        assert np.all(fx[f"{name}_mean"] > 0) and np.all(fx[f"{name}_se"] > 0)
        # the fixture alone resolves 2 %: 0.02 x mean is beyond the band (by the margin the noise of the code under test may take)
        assert np.mean(0.02 * fx[f"{name}_mean"] > (Z_MAX + 1.0) * fx[f"{name}_se"]) >= 0.9


def test_generator_has_not_drifted():
    """the first CHUNK_SPP samples of one case, rendered again with the stored seed, give the stored prefix statistics"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("gen_integrator_ref", GOLDEN.parent / "gen_integrator_ref.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fx = fixture()
    name = "sky_b2"
    flags, bounces, specular, _, _, _ = IW.ROOM_CASES[name]
    mean, var = RP.render(gen.room_scene(specular), IW.ROOM_CAMERA, IW.WINDOW_ROOM, flags, bounces, RP.CHUNK_SPP, int(fx[f"{name}_seed"].item()))
    bm, se = RP.block_stats(mean, var, RP.CHUNK_SPP)
    assert np.allclose(bm, fx[f"{name}_prefix_mean"], rtol=1e-9, atol=0.0)
    assert np.allclose(se, fx[f"{name}_prefix_se"], rtol=1e-9, atol=0.0)


def test_sky_texels_are_the_ones_the_kernels_read():
    """the reference decodes its sky from ref_shading's RGB9E5 encoder; the oracle's texel words are the same"""
    sky = IW.room_sky()
    osc = orc.Scene(IW.open_room(), sky, None)
    words = osc.sky_tables(sky.shape[1], sky.shape[0])[1]
    want, ambiguous = R.rgb9e5_encode(sky.astype(np.float64).reshape(-1, 3))
    same = words.reshape(-1) == want
    assert np.all(same | ambiguous)
    assert np.abs(R.rgb9e5_decode(words.reshape(-1)) - R.rgb9e5_decode(want)).max() <= 2.0**-8 * sky.max()


@functools.lru_cache(maxsize=None)
def oracle_room_frames(name):
    flags, bounces, specular, _, _, n_frames = IW.ROOM_CASES[name]
    osc = orc.Scene(IW.open_room(specular), IW.room_sky(), None)
    out = [oracle_frame(osc, IW.ROOM_CAMERA, IW.WINDOW_ROOM, flags, bounces, IW.FRAME_SPP, frame=k) for k in range(n_frames)]
    return np.stack([o[0] for o in out]), out[0][2]


@pytest.mark.parametrize("name", sorted(IW.ROOM_CASES))
def test_oracle_against_fixture(name):
    frames, covered = oracle_room_frames(name)
    check_against_fixture(frames, covered, fixture(), name)
