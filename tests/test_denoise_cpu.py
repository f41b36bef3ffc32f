"""The "denoise" pass, CPU half: tests/ref_denoise.py -- the numpy float32 restatement the GPU pass must equal bit
for bit (tests/test_denoise.py) -- is pinned here by what a denoiser owes its user: it reduces the error of low-sample frames, it does
not bleed across geometric edges, it leaves background, alpha and (with 0 iterations) everything alone; and the Python frame graph
places the node where the header says."""
import ctypes as C
import math

import numpy as np
import pytest

import orc
import ref_denoise as rd
from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from raytracer3_amd.assets import MeshBuilder
from raytracer3_amd.render_graph import RenderGraph
from support import RecordingCtx, bits, gamma, quad, rmse_fg

U = 2.0 ** -24  # unit roundoff of float32
BG = np.float32(orc.BACKGROUND_DEPTH)


# ------------------------------------------------------------------------------------------------ 1. expn
EXPN_MAX_REL = 7.29e-6  # measured: max |expn(x) - exp(-x)| / exp(-x) over 2 000 001 evenly spaced float32 x in [0, 90] (at x = 89.91: the
#                         rounding of x * log2(e), ~6e-8 * 130 * ln 2, and above x = 87.3 the denormal grid); 9.9e-7 over [0, 20]


def test_expn_against_float64():
    x = np.linspace(0.0, 90.0, 2_000_001).astype(np.float32)
    got = rd.expn(x)
    assert got.dtype == np.float32
    want = np.exp(-x.astype(np.float64))
    rel = np.abs(got.astype(np.float64) - want) / want
    print(f"expn: max rel err over [0, 90] = {rel.max():.3e} at x = {x[rel.argmax()]:.4f}; over [0, 20] = {rel[x <= 20].max():.3e}")
    assert rel.max() < 2 * EXPN_MAX_REL
    assert rel[x <= 20].max() < 2 * 9.9e-7
    assert rd.expn(np.float32(0.0)) == np.float32(1.0)  # the centre tap's w_z and w_l are exactly 1
    assert np.all(np.diff(got.astype(np.float64)) <= got[:-1] * 4 * U)  # non-increasing up to the rounding of neighbouring arguments
    edge = rd.expn(np.array([88.0, 100.0, 103.0, 103.97, 104.0, 1e30, np.inf], np.float32))
    assert 0 < edge[1] < np.float32(1.1754944e-38) and edge[3] == np.float32(1.4012985e-45)  # denormal results, down to the smallest
    assert edge[0] > edge[1] > edge[2] >= edge[3] and edge[4] == 0 and edge[5] == 0 and edge[6] == 0  # 0 from x log2(e) >= 150 on


# ------------------------------------------------------------------------------------------------ 2. it denoises


def cornell_case():
    W = H = 128
    g = orc.camera_gconst(width=W, height=H, **scenes.CORNELL_CAMERA)
    g.bounces, g.blendfactor = 4, 1.0
    g.pad[0] = L.F_FACEFORWARD
    return orc.Scene(scenes.cornell()), g, 2048


def atrium_case():
    W, H = 192, 108
    g = orc.camera_gconst(width=W, height=H, **scenes.ATRIUM_CAMERA)
    g.bounces, g.blendfactor = 4, 1.0
    g.pad[0] = L.F_NEE_SKY | L.F_BLUENOISE | L.F_SPECULAR | L.F_FACEFORWARD  # 15: the default estimator with the layered BSDF
    return orc.Scene(scenes.atrium(0.25), scenes.sky(512, 256), assets.load_bluenoise()), g, 1024


@pytest.mark.parametrize("case", [cornell_case, atrium_case], ids=["cornell", "atrium"])
def test_filter_reduces_the_error_of_low_sample_frames(case):
    """Foreground RMSE of linear radiance against a converged oracle frame (another seed): filtered < unfiltered at 1, 4 and 16 spp, with 5
    and with 3 iterations.  Measured: cornell 1.346 -> 0.218 / 0.245, 0.671 -> 0.113 / 0.117, 0.339 -> 0.067 / 0.067."""
    osc, g, ref_spp = case()
    gb, depth = osc.gbuffer(g, threads=16)
    fg = depth != BG

    def render(spp, frame):
        g.samples, g.frame = spp, frame
        return osc.reference_mode(g, gb, depth, threads=16)[0]

    ref = render(ref_spp, 1000)
    for spp in (1, 4, 16):
        noisy = render(spp, 7)
        e0 = rmse_fg(noisy, ref, fg)
        for it in (5, 3):
            out = rd.denoise(g, gb, depth, noisy, iterations=it)
            e = rmse_fg(out, ref, fg)
            print(f"{case.__name__} {spp} spp: unfiltered {e0:.4f}, {it} iterations {e:.4f} ({e0 / e:.2f} x)")
            assert e < e0
            assert np.array_equal(bits(out)[~fg], bits(noisy)[~fg]) and np.array_equal(bits(out[..., 3]), bits(noisy[..., 3]))


# ------------------------------------------------------------------------------------------------ 3. it does not bleed


def synthetic(kind, W=96, H=80):
    """G-buffer and depth (the oracle's gbuffer pass) of two quads, and the surface id per pixel (0 = background, 1, 2)"""
    mb = MeshBuilder()
    if kind == "corner":  # a floor meeting a wall at a right angle
        quad(mb, "floor", [-1.6, 0, 2], [3.0, 0, 0], [0, 0, -4], (0.8, 0.2, 0.2))
        quad(mb, "wall", [-1.6, 0, -2], [3.0, 0, 0], [0, 1.8, 0], (0.2, 0.8, 0.2))
        cam = dict(position=(0.3, 1.2, 3.0), direction=(-0.05, -0.25, -1.0), fov_deg=50.0)
    else:  # two parallel quads at different depths, the near one covering part of the far one
        quad(mb, "far", [-4, -2, -2], [8, 0, 0], [0, 5, 0], (0.8, 0.2, 0.2))
        quad(mb, "near", [-0.6, 0.5, 0], [1.3, 0, 0], [0, 1.1, 0], (0.2, 0.8, 0.2))
        cam = dict(position=(0.1, 1.0, 3.0), direction=(0.02, 0.01, -1.0), fov_deg=50.0)
    g = orc.camera_gconst(width=W, height=H, **cam)
    g.pad[0] = L.F_FACEFORWARD
    gb, depth = orc.Scene(mb.build()).gbuffer(g)
    words = np.unique(gb[depth != BG][:, 0])
    assert len(words) == 2  # two albedo words = two surfaces
    ident = np.where(depth == BG, 0, np.where(gb[..., 0] == words[0], 1, 2))
    return g, gb, depth, ident


# One iteration computes c' = (sum_k w_k c_k) / (sum_k w_k) over N = 25 taps with non-negative weights: a product and at most N - 1
# additions per term of the numerator (gamma_N+1), N - 1 additions in the denominator (gamma_N-1), one division: with every c_k within d of
# a constant A, |c' - A| <= d + gamma_{2N+2} (|A| + d).  The variance estimate only moves the (non-negative) weights.
STEP_ROUNDING = gamma(2 * 25 + 2)


def constant_bound(a, iterations):
    d = 0.0
    for _ in range(iterations):
        d = d + STEP_ROUNDING * (abs(a) + d)
    return d


def frame_of(ident, values):
    H, W = ident.shape
    img = np.zeros((H, W, 4), np.float32)
    for k, v in values.items():
        img[ident == k] = v
    img[..., 3] = np.linspace(0, 1, H * W, dtype=np.float32).reshape(H, W)  # alpha: opaque data to carry over
    return img


def test_no_bleeding_across_a_normal_edge():
    """n_p . n_q is ~0 across the right angle (the 11:10:11 normals are a few 1e-4 off the axes), so seven squarings underflow the
    cross-edge weight to exactly 0: every pixel keeps its own constant to within the rounding of a weighted mean of equal values."""
    g, gb, depth, ident = synthetic("corner")
    assert (ident == 1).sum() > 1000 and (ident == 2).sum() > 1000 and (ident == 0).sum() > 100
    A, B = 3.0, 0.25
    img = frame_of(ident, {0: (9.0, 9.0, 9.0, 0), 1: (A, A, A, 0), 2: (B, B, B, 0)})
    for it in (1, 3, 5):
        out = rd.denoise(g, gb, depth, img, iterations=it, flags=rd.NO_DEMODULATION)
        for k, v in ((1, A), (2, B)):
            err = np.abs(out[ident == k][:, :3].astype(np.float64) - v).max()
            print(f"corner, {it} iterations, surface {k}: max |out - {v}| = {err:.3e} (bound {constant_bound(v, it):.3e})")
            assert err <= constant_bound(v, it)
        assert np.array_equal(bits(out)[ident == 0], bits(img)[ident == 0])


def test_no_bleeding_across_a_depth_edge():
    """Parallel surfaces: only w_z (and w_l) reject a tap across the silhouette.  With every pixel within d of its own constant, a pixel's
    new value is a weighted mean: |c' - A| <= d + rho (|B - A| + 2 d) + rounding, rho = (sum of its cross-edge weights) / (its centre
    weight) >= their share of the weight sum.  w_l <= 1 and the centre's w_l = w_z = 1 exactly, so rho is bounded from the geometry
    alone: sum_cross h w_n exp(-x_z) / (h_0 w_n(centre)), with exp widened by expn's measured error."""
    g, gb, depth, ident = synthetic("parallel")
    assert (ident == 1).sum() > 1000 and (ident == 2).sum() > 500
    A, B = 0.5, 4.0
    img = frame_of(ident, {0: (9.0, 9.0, 9.0, 0), 1: (A, A, A, 0), 2: (B, B, B, 0)})
    iterations = 5
    pr = rd.prepare(g, gb, depth, img, demodulate=False)
    T = rd._Taps(pr["P"], pr["n"], 2 << (iterations - 1), 7, np.float32(1.0) / np.float32(0.05))
    idp = T.pad(ident)
    d, D = 0.0, abs(B - A)
    for it in range(iterations):
        st = 1 << it
        cross = np.zeros(ident.shape)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                wn, xz = T.geo(dy * st, dx * st)
                w = float(rd.H5[dy + 2] * rd.H5[dx + 2]) * wn.astype(np.float64) * np.exp(-xz.astype(np.float64)) * (1 + 2 * EXPN_MAX_REL)
                other = (T.at(idp, dy * st, dx * st) != ident) & (T.at(idp, dy * st, dx * st) != 0)
                cross += np.where(other, w, 0.0)
        wn0, _ = T.geo(0, 0)
        fgm = ident != 0
        rho = float((cross[fgm] / (float(rd.H5[2] * rd.H5[2]) * wn0.astype(np.float64)[fgm])).max())
        d = d + rho * (D + 2 * d) + STEP_ROUNDING * (max(abs(A), abs(B)) + d)
        out = rd.denoise(g, gb, depth, img, iterations=it + 1, flags=rd.NO_DEMODULATION)
        err = max(np.abs(out[ident == k][:, :3].astype(np.float64) - v).max() for k, v in ((1, A), (2, B)))
        print(f"parallel, {it + 1} iterations: rho = {rho:.3e}, max |out - own constant| = {err:.3e} (bound {d:.3e})")
        assert rho < 1e-3  # the geometry of this test: the silhouette is steep, the bound is a small fraction of |B - A|
        assert err <= d


def test_a_constant_frame_stays_constant():
    for kind in ("corner", "parallel"):
        g, gb, depth, ident = synthetic(kind)
        A = 1.7
        img = frame_of(ident, {0: (A, A, A, 0), 1: (A, A, A, 0), 2: (A, A, A, 0)})
        out = rd.denoise(g, gb, depth, img, flags=rd.NO_DEMODULATION)
        err = np.abs(out[..., :3].astype(np.float64) - A).max()
        print(f"{kind}: constant frame, max |out - A| = {err:.3e} (bound {constant_bound(A, 5):.3e})")
        assert err <= constant_bound(A, 5)


# ------------------------------------------------------------------------------------------------ 4. pass-through, identity, odd windows
def test_background_alpha_identity_and_odd_windows():
    rng = np.random.default_rng(5)
    for W, H in ((61, 37), (33, 9), (7, 5)):  # no multiple of 8, of the kernels' 32 x 8 tile, and smaller than one tile / than the 7 x 7 window
        g = orc.camera_gconst(width=W, height=H, **scenes.ATRIUM_CAMERA)
        g.pad[0] = L.F_FACEFORWARD
        gb, depth = orc.Scene(scenes.atrium(0.2)).gbuffer(g)
        fg = depth != BG
        assert fg.any() and (~fg).any()
        img = rng.random((H, W, 4), dtype=np.float32) * 2
        img[~fg] = np.array([np.nan, np.inf, -1.0, 7.0], np.float32)  # k_accumulate leaves background Light unwritten: opaque data
        for it in (1, 5, 8):
            out = rd.denoise(g, gb, depth, img, iterations=it)
            assert out.shape == img.shape and out.dtype == np.float32
            assert np.array_equal(bits(out)[~fg], bits(img)[~fg])
            assert np.array_equal(bits(out[..., 3]), bits(img[..., 3]))
            assert np.isfinite(out[fg][:, :3]).all() and not np.array_equal(out[fg], img[fg])
        assert np.array_equal(bits(rd.denoise(g, gb, depth, img, iterations=0)), bits(img))


def test_demodulation_preserves_albedo_detail():
    """c = (In - e) / albedo is what the filter sees: a frame that is exactly albedo x constant irradiance (+ emission) comes back with
    its albedo edges intact, to rounding; without demodulation the same frame is blurred across them."""
    g, gb, depth, ident = synthetic("corner")
    alb, emi, _ = rd.unpack_gbuffer(gb)
    img = np.zeros(depth.shape + (4,), np.float32)
    img[..., :3] = emi + alb * np.float32(2.5)
    out = rd.denoise(g, gb, depth, img)
    fg = ident != 0
    rel = np.abs(out[fg][:, :3].astype(np.float64) - img[fg][:, :3]) / img[fg][:, :3]
    assert rel.max() <= constant_bound(1.0, 5) + 4 * U  # the division and the product of (de)modulation: 2 roundings each way


# ------------------------------------------------------------------------------------------------ 5. Python surface


def test_frame_graph_places_the_denoise_node():
    from raytracer3_amd.renderer import frame_nodes

    W, H = 250, 187
    ctx = RecordingCtx()
    rg = RenderGraph(ctx, (W, H))
    rg.begin_frame()
    h = frame_nodes(rg, L.GConst(), postprocess=True, denoise=True)
    rg.draw_frame(h["color"])
    assert [c[0] for c in ctx.calls] == ["gbuffer", "refrence_mode", "denoise", "postprocess"]
    dn, pp = ctx.calls[2], ctx.calls[3]
    assert dn[1] == (math.ceil(W / 8), math.ceil(H / 8), 1) == (32, 24, 1)
    assert dn[2] == [h["gbuffer"], h["depth"], h["light"], h["denoised"]]
    assert len(set(dn[2])) == 4 and pp[2] == [h["depth"], h["color"], h["denoised"]]  # the tone map reads the filtered image
    # without post-processing the filtered image is the frame's output
    ctx.calls.clear()
    rg.begin_frame()
    h = frame_nodes(rg, L.GConst(), postprocess=False, denoise=True)
    rg.draw_frame(h["denoised"])
    assert [c[0] for c in ctx.calls] == ["gbuffer", "refrence_mode", "denoise"]
    # default: today's graph
    ctx.calls.clear()
    rg.begin_frame()
    h = frame_nodes(rg, L.GConst())
    assert "denoised" not in h
    rg.draw_frame(h["color"])
    assert [c[0] for c in ctx.calls] == ["gbuffer", "refrence_mode", "postprocess"]
    assert ctx.calls[2][2] == [h["depth"], h["color"], h["light"]] and ctx.calls[2][1] == (32, 24, 1)


def test_params_struct_matches_the_header():
    p = L.DenoiseParams()
    assert C.sizeof(p) == 20
    assert (p.iterations, p.normal_squarings, p.flags) == (5, 7, 0) and p.sigma_z == np.float32(0.05) and p.sigma_l == 4.0
    assert rd.DEFAULTS == dict(iterations=5, normal_squarings=7, sigma_z=0.05, sigma_l=4.0, flags=0)
    assert L.DENOISE_NO_DEMODULATION == rd.NO_DEMODULATION == 1
    assert "rt3_denoise_set_params" in L.EXPORTS
