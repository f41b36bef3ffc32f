"""The sample-guided "temporal" pass, CPU half: tests/ref_temporal_guide.py -- the numpy float32 restatement the
GPU pass must equal bit for bit (tests/test_temporal_guide.py) -- is pinned here before a GPU sees the kernel: against an independently
written scalar loop, bit for bit; by what the pass owes its user on two-surface guides (no tap of the other surface counts); on what is
not foreground; on positions that must never become an index; and on the running mean under a static camera."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

import ref_guide as rgd
import ref_temporal_guide as rtg
import temporal_guide_worlds as TW
from raytracer3_amd import _lib as L
from raytracer3_amd.render_graph import RenderGraph
from support import RecordingCtx, bits, zeros

F = np.float32
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ 1. the scalar loop
def scalar_temporal(g, guide, light, prev_g, prev_guide, prev_history, prev_moments, alpha=0.2, alpha_moments=0.2, max_history=32,
                    normal_cos=0.9, plane_tolerance=0.01, flags=0):
    """steps 1 to 5 of the issue, one pixel at a time, in np.float32 scalars: written from the text, not from ref_temporal_guide.  An
    integer is made only from a float that passed the window test, and an image is indexed only by a pair that passed the index test."""
    H, W = light.shape[:2]
    alpha, alpha_m, max_h, ncos, ptol = F(alpha), F(alpha_moments), F(max_history), F(normal_cos), F(plane_tolerance)
    one, zero, half, floor_m = F(1), F(0), F(0.5), F(1.0 / 256.0)
    fmax = np.finfo(F).max
    out, hist, mom = np.empty((H, W, 4), F), np.empty((H, W, 4), F), np.empty((H, W, 4), F)

    def row(m, r, x, y, z, w):
        return ((F(m[r]) * x + F(m[4 + r]) * y) + F(m[8 + r]) * z) + F(m[12 + r]) * w

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    def record(images, y, x):
        """(foreground, unit normal) of a guide texel"""
        nx, ny, nz = images["normal"][y, x, :3]
        l2 = (nx * nx + ny * ny) + nz * nz
        if not (images["position"][y, x, 3] == one and l2 > zero and l2 <= fmax):
            return False, None
        s = one / np.sqrt(l2)
        return True, (nx * s, ny * s, nz * s)

    Wf, Hf = F(g.window_size[0]), F(g.window_size[1])
    eye = [F(g.view_inverse[12 + k]) for k in range(3)]
    for y in range(H):
        for x in range(W):
            In = light[y, x]
            fg, n = record(guide, y, x)
            if not fg:
                out[y, x], hist[y, x], mom[y, x] = In, 0, 0
                continue
            P = [F(v) for v in guide["position"][y, x, :3]]
            if flags & 1:
                m, e = [one] * 3, [zero] * 3
            else:
                m = [a if a > floor_m else floor_m for a in guide["albedo"][y, x, :3]]
                e = list(guide["emission"][y, x, :3])
            c = [(In[k] - e[k]) / m[k] for k in range(3)]
            lum = (F(0.2126) * c[0] + F(0.7152) * c[1]) + F(0.0722) * c[2]
            v = [row(prev_g.view, r, P[0], P[1], P[2], one) for r in range(4)]
            qx, qy, qw = (row(prev_g.proj, r, *v) for r in (0, 1, 3))
            ws, hs, ks = zero, [zero] * 4, [zero] * 2
            if qw > zero:
                sx = ((qx / qw) * half + half) * Wf - half
                sy = (-(qy / qw) * half + half) * Hf - half
                if sx > -one and sx < Wf and sy > -one and sy < Hf:
                    assert math.isfinite(sx) and math.isfinite(sy)
                    x0f, y0f = np.floor(sx), np.floor(sy)
                    fx, fy = sx - x0f, sy - y0f
                    x0, y0 = int(x0f), int(y0f)
                    assert -1 <= x0 <= W - 1 and -1 <= y0 <= H - 1
                    dE = [P[k] - eye[k] for k in range(3)]
                    tol = ptol * np.sqrt(dot(dE, dE))
                    for j in (0, 1):
                        ty = y0 + j
                        if ty < 0 or ty >= H:
                            continue
                        wy = fy if j else one - fy
                        for i in (0, 1):
                            tx = x0 + i
                            if tx < 0 or tx >= W:
                                continue
                            qfg, nq = record(prev_guide, ty, tx)
                            if not qfg:
                                continue
                            ph = prev_history[ty, tx]
                            if not ph[3] > zero:
                                continue
                            if not dot(n, nq) >= ncos:
                                continue
                            dP = [prev_guide["position"][ty, tx, k] - P[k] for k in range(3)]
                            if not abs(dot(n, dP)) <= tol:
                                continue
                            pm = prev_moments[ty, tx]
                            wt = (fx if i else one - fx) * wy
                            ws = ws + wt
                            hs = [hs[k] + wt * ph[k] for k in range(4)]
                            ks = [ks[k] + wt * pm[k] for k in range(2)]
            N, acc, mu1, mu2 = one, c, lum, lum * lum
            if ws > zero:
                hs = [h / ws for h in hs]
                ks = [k / ws for k in ks]
                n1 = hs[3] + one
                N = n1 if n1 < max_h else max_h
                inv = one / N
                ac = alpha if alpha > inv else inv
                am = alpha_m if alpha_m > inv else inv
                acc = [hs[k] + ac * (c[k] - hs[k]) for k in range(3)]
                mu1 = ks[0] + am * (lum - ks[0])
                mu2 = ks[1] + am * (mu2 - ks[1])
            d = mu2 - mu1 * mu1
            hist[y, x] = (*acc, N)
            mom[y, x] = (mu1, mu2, d if d > zero else zero, N)
            out[y, x] = (*[e[k] + acc[k] * m[k] for k in range(3)], In[3])
    return out, hist, mom


PARAMS = (dict(), dict(flags=rtg.NO_DEMODULATION), dict(alpha=0.0, alpha_moments=0.0, max_history=4), dict(normal_cos=0.95, plane_tolerance=0.002),
          dict(alpha=0.5, alpha_moments=0.1, max_history=7, normal_cos=0.5, plane_tolerance=0.1))


@pytest.mark.parametrize("window, seed", [((23, 17), 1), ((9, 14), 2), ((1, 1), 3)])
def test_vectorised_reference_equals_a_scalar_loop(window, seed):
    f = TW.random_frame(window, seed)
    counted = 0
    for params in PARAMS:
        stages = {}
        with np.errstate(all="ignore"):
            want = scalar_temporal(*TW.ref_args(f), **params)
        got = rtg.temporal(*TW.ref_args(f), stages=stages, **params)
        for a, b, name in zip(got, want, ("Out", "History", "Moments")):
            assert a.dtype == F and np.array_equal(bits(a), bits(b)), (window, params, name)
        counted += int(stages["has"].sum())
    assert counted > 0 or window == (1, 1), "taps did count"


def test_scalar_loop_on_the_edge_cases():
    """the same comparison on the frame that holds every edge case (the scalar loop asserts that nothing odd reaches an integer)"""
    f = TW.edge_case_frame((31, 22))
    with np.errstate(all="ignore"):
        want = scalar_temporal(*TW.ref_args(f))
    for a, b, name in zip(rtg.temporal(*TW.ref_args(f)), want, ("Out", "History", "Moments")):
        assert np.array_equal(bits(a), bits(b)), name


# ------------------------------------------------------------------------------------------------ 2. no tap of the other surface
@pytest.mark.parametrize("kind", ["corner", "parallel"])
def test_no_tap_of_the_other_surface_counts(kind):
    """Two surfaces with constant signals 0.25 and 37 (no demodulation), four frames under a sliding camera.  'corner': the surfaces meet at
    a right angle and only the normal test tells them apart (the plane tolerance is opened wide); 'parallel': they share a normal and only
    the plane test does (normal_cos = -1 lets every normal pass).  Every accumulated value stays within test_temporal_cpu's bound for a
    constant, which one tap of the other surface would break by orders of magnitude; and history is kept, not thrown away."""
    from test_temporal_cpu import constant_bound

    const = {0: 0.0, 1: 0.25, 2: 37.0}
    only = dict(plane_tolerance=1e6) if kind == "corner" else dict(normal_cos=-1.0)
    prev, n_frames = None, 4
    for step in range(n_frames):
        g, guide, ident = TW.two_quads(kind, step, (96, 80))
        H, W = ident.shape
        light = TW.constant_light(ident, const)
        if prev is None:
            prev = (g, guide, zeros(H, W), zeros(H, W))
        out, hist, mom = rtg.temporal(g, guide, light, *prev, flags=rtg.NO_DEMODULATION, **only)
        prev = (g, guide, hist, mom)
    N = hist[..., 3]
    for s in (1, 2):
        sel = ident == s
        err = np.abs(hist[..., :3][sel].astype(np.float64) - const[s]).max()
        bound = constant_bound(const[s], n_frames)
        print(f"{kind} surface {s}: max |c_acc - A| = {err:.3e}, bound {bound:.3e}; N > 1 on {100 * (N[sel] > 1).mean():.1f} %")
        assert err <= bound
        assert (N[sel] > 1).mean() > 0.5
        assert np.abs(out[..., :3][sel].astype(np.float64) - const[s]).max() <= bound
    assert not hist[ident == 0].any() and not mom[ident == 0].any()
    # ... and the test that was left on is the one that did it: with both opened wide the surfaces do mix
    g0, guide0, _ = TW.two_quads(kind, n_frames - 2, (96, 80))
    mixed = rtg.temporal(g, guide, light, g0, guide0, prev[2], prev[3], flags=rtg.NO_DEMODULATION, plane_tolerance=1e6, normal_cos=-1.0)[1]
    worst = max(np.abs(mixed[..., :3][ident == s].astype(np.float64) - const[s]).max() for s in (1, 2))
    assert worst > 1.0, "without either test a tap of the other surface counts"


# ------------------------------------------------------------------------------------------------ 3. what is not foreground
def test_non_foreground_pixels_and_texels():
    f = TW.edge_case_frame()
    stages = {}
    out, hist, mom = rtg.temporal(*TW.ref_args(f), stages=stages)
    light = f["light"]
    for kind, (ys, xs) in f["current_bad"].items():
        assert len(ys) and not stages["fg"][ys, xs].any(), kind
        assert np.array_equal(bits(out[ys, xs]), bits(light[ys, xs])), f"{kind}: copied bit for bit"
        assert not hist[ys, xs].any() and not mom[ys, xs].any(), kind
    bg = f["ident"] == 0
    assert bg.any() and np.array_equal(bits(out[bg]), bits(light[bg])) and not hist[bg].any()
    # previous texels that are not foreground carry weight exactly 0: whatever their History and Moments hold changes no bit
    fg_prev, _ = rgd.foreground(f["prev_guide"])
    for kind, mask in f["prev_bad"].items():
        assert mask.any() and not fg_prev[mask].any(), kind
    off = ~fg_prev
    poisoned = dict(f, prev_history=f["prev_history"].copy(), prev_moments=f["prev_moments"].copy())
    poisoned["prev_history"][off] = np.array([np.nan, np.inf, -1e30, 5.0], F)
    poisoned["prev_moments"][off] = np.nan
    for a, b in zip(rtg.temporal(*TW.ref_args(poisoned)), (out, hist, mom)):
        assert np.array_equal(bits(a), bits(b))
    # ... and they were in reach: foreground pixels reproject into each block
    x0, y0 = np.floor(stages["sx"]), np.floor(stages["sy"])
    H, W = off.shape
    for kind, mask in f["prev_bad"].items():
        ys, xs = np.nonzero(stages["valid"])
        cy, cx = np.clip(y0[ys, xs].astype(int), 0, H - 1), np.clip(x0[ys, xs].astype(int), 0, W - 1)
        assert mask[cy, cx].any(), f"no pixel reprojects into the '{kind}' block"
    # a texel with History.w == 0 is "no history" on a foreground texel too
    assert (stages["fg"] & ~stages["has"] & stages["valid"]).any()


# ------------------------------------------------------------------------------------------------ 4. nothing odd becomes an index
def test_odd_positions_never_reach_an_integer():
    f = TW.edge_case_frame()
    stages = {}
    with np.errstate(all="raise", under="ignore", over="ignore", invalid="ignore", divide="ignore"):
        out, hist, mom = rtg.temporal(*TW.ref_args(f), stages=stages)
    valid, sx, sy = stages["valid"], stages["sx"], stages["sy"]
    H, W = valid.shape
    # where the reprojection counts, the float position is finite and inside (-1, W) x (-1, H): floor gives -1 .. W - 1, every tap is index-tested
    assert np.all(np.isfinite(sx[valid]) & np.isfinite(sy[valid]))
    assert np.all((sx[valid] > -1) & (sx[valid] < W) & (sy[valid] > -1) & (sy[valid] < H))
    for name, where in f["odd_positions"].items():
        for y, x in where:
            assert stages["fg"][y, x], name
            if name != "far":  # (a far point in front of the camera may project inside; it then fails the plane test)
                assert not valid[y, x], name
            assert hist[y, x, 3] == 1 and mom[y, x, 3] == 1, f"{name}: no history"
            assert np.array_equal(bits(out[y, x, 3]), bits(f["light"][y, x, 3]))
    # the vectorised reference converts where(valid, floor, 0): no NaN, Inf or value beyond int32 is cast
    cast_x, cast_y = np.where(valid, np.floor(sx), F(0)), np.where(valid, np.floor(sy), F(0))
    assert np.all(np.abs(cast_x) <= W) and np.all(np.abs(cast_y) <= H)


# ------------------------------------------------------------------------------------------------ 5. the running mean
def test_static_camera_runs_the_mean():
    """Static camera, the same guide every frame, alpha = alpha_moments = 0, K = 8 frames whose In is emission + v_k albedo with one random
    v_k per frame: c_k = v_k at every pixel up to the demodulation's two roundings (3 u relative with In's own), N == K within
    ref_temporal_guide.history_length_bound and History.rgb is the mean of the c_k within running_mean_bound (both derived there)."""
    K = 8
    g, guide, ident = TW.two_quads("corner", 0)
    H, W = ident.shape
    fg, _ = rgd.foreground(guide)
    assert np.array_equal(fg, ident != 0) and fg.sum() > 500
    vals = (np.random.default_rng(5).random(K) * 3 + 0.1).astype(F)
    prev = (g, guide, zeros(H, W), zeros(H, W))
    cs = []
    for k, v in enumerate(vals):
        light = np.ones((H, W, 4), F)
        light[..., :3] = guide["emission"][..., :3] + v * guide["albedo"][..., :3]
        stages = {}
        out, hist, mom = rtg.temporal(g, guide, light, *prev, alpha=0.0, alpha_moments=0.0, max_history=K, stages=stages)
        cs.append(stages["c"][fg].astype(np.float64))
        assert np.all(np.abs(hist[..., 3][fg].astype(np.float64) - (k + 1)) <= rtg.history_length_bound(k + 1)), k
        prev = (g, guide, hist, mom)
    N = hist[..., 3][fg].astype(np.float64)
    scale = float(vals.max()) * (1 + 4 * U)
    spread = max(np.abs(c - float(v)).max() for c, v in zip(cs, vals))
    # In = fl(e + fl(v m)), c = fl(fl(In - e) / m): |c - v| <= 3 u |v| + u R, R = max |In| / m (ref_guide.constant_signal_bound's first lines)
    m = np.maximum(guide["albedo"][..., :3][fg].astype(np.float64), 1.0 / 256.0)
    R = float(((guide["emission"][..., :3][fg] + scale * m) / m).max())
    assert spread <= 1.01 * (3 * U * scale + U * R), "c_k is v_k up to the demodulation's roundings"
    mean = np.mean(cs, axis=0)
    err = np.abs(hist[..., :3][fg].astype(np.float64) - mean).max()
    # the c_k differ from pixel to pixel by `spread`: the taps' convex combination may move the mean by as much
    bound = rtg.running_mean_bound(K, scale) + spread
    print(f"K = {K}: max |N - K| = {np.abs(N - K).max():.3e} (bound {rtg.history_length_bound(K):.3e}), N == K exactly on {100 * (N == K).mean():.1f} %; "
          f"max |History - mean| = {err:.3e} (bound {bound:.3e})")
    assert np.all(np.abs(N - K) <= rtg.history_length_bound(K))
    assert err <= bound
    assert np.array_equal(bits(hist[..., 3]), bits(mom[..., 3]))


# ------------------------------------------------------------------------------------------------ 6. the Python surface
def test_frame_graph_declares_the_guide_as_context_state():
    from raytracer3_amd.renderer import frame_nodes

    W, H = 67, 45
    ctx = RecordingCtx()
    rg = RenderGraph(ctx, (W, H))
    rg.begin_frame()
    h = frame_nodes(rg, L.GConst(), postprocess=True, denoise=True, temporal=True, guide=True)
    assert sorted(h["guide"]) == sorted(h["prev_guide"]) == sorted(TW.KEYS)
    assert len({*h["guide"].values(), *h["prev_guide"].values()}) == 8
    nodes = {n.name: n for n in rg.nodes}
    state = lambda name, typ: [e.resource for e in nodes[name].edges if e.edge_type == typ]  # noqa: E731
    assert state("refrence_mode", "StateWrite") == list(h["guide"].values())
    assert state("temporal", "StateRead") == [*h["guide"].values(), *h["prev_guide"].values()]
    assert state("denoise", "StateRead") == list(h["guide"].values())
    rg.draw_frame(h["color"])
    assert [c[0] for c in ctx.calls] == ["gbuffer", "refrence_mode", "temporal", "denoise", "postprocess"]
    tp, dn = ctx.calls[2], ctx.calls[3]
    assert tp[2] == [h["gbuffer"], h["depth"], h["light"], h["prev_gbuffer"], h["prev_depth"], h["prev_history"], h["prev_moments"],
                     h["accumulated"], h["history"], h["moments"]], "ten bindings, the guide is none of them"
    assert dn[2] == [h["gbuffer"], h["depth"], h["accumulated"], h["denoised"]]
    # without `guide`: today's nodes, edge for edge
    ctx.calls.clear()
    rg.begin_frame()
    h = frame_nodes(rg, L.GConst(), postprocess=True, denoise=True, temporal=True)
    assert "guide" not in h and "prev_guide" not in h
    assert not any(e.edge_type.startswith("State") for n in rg.nodes for e in n.edges)
    # over a Light that is already there (PathTracer.denoise): the guide is imported
    rg.begin_frame()
    h = frame_nodes(rg, L.GConst(), False, True, True, trace=False, guide=True)
    rg.draw_frame(h["denoised"])


def test_export_and_header():
    assert "rt3_temporal_set_guide_input" in L.EXPORTS
    header = (Path(__file__).resolve().parent.parent / "include" / "rt3.h").read_text()
    assert re.search(r"\bint rt3_temporal_set_guide_input\(rt3_ctx \*ctx, const rt3_guide_images \*current, const rt3_guide_images \*previous\);", header)
    assert C.sizeof(L.GuideImages) == 16
