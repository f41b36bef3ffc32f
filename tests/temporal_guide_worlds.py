"""Caller-made guide images for the tests of the sample-guided "temporal" pass (tests/test_temporal_guide_cpu.py and
tests/test_temporal_guide.py).  Nothing here needs a GPU or a tracer: the two-quad guides come from the oracle's
G-buffer pass over the two-quad scenes of tests/test_temporal_cpu.py, the rest is written by hand."""
import numpy as np

import orc
import ref_denoise as rd
import ref_temporal as rt

F = np.float32
BG = F(orc.BACKGROUND_DEPTH)
KEYS = ("position", "normal", "albedo", "emission")
WINDOW = (67, 45)  # no multiple of the 32 x 8 tile, an odd row length


def two_quads(kind, step, window=WINDOW):
    """(GConst, guide, surface id per pixel) of test_temporal_cpu.synthetic(kind, step): 'corner' (told apart by the normal test) or
    'parallel' (by the plane test).  The guide is what a one-sample pinhole lens frame would write, but for the normal's length: the sum
    of several samples' normals is not a unit vector, so the normal is scaled by 0.83 and the pass has to normalise it."""
    from test_temporal_cpu import synthetic

    g, gb, depth, ident = synthetic(kind, step, *window)
    fg = depth != BG
    albedo, emission, n = rd.unpack_gbuffer(gb)
    H, W = depth.shape
    z = np.zeros((H, W, 1), F)
    f3 = fg[..., None]
    guide = dict(position=np.concatenate([np.where(f3, rt.positions(g, depth), F(0)), fg[..., None].astype(F)], -1).astype(F),
                 normal=np.concatenate([np.where(f3, n * F(0.83), F(0)), z], -1).astype(F),
                 albedo=np.concatenate([np.where(f3, albedo, F(1)), z], -1).astype(F),
                 emission=np.concatenate([np.where(f3, emission, F(0)), z], -1).astype(F))
    return g, guide, ident


def constant_light(ident, const):
    H, W = ident.shape
    light = np.zeros((H, W, 4), F)
    for s, v in const.items():
        light[ident == s, :3] = v
    light[..., 3] = 1.0
    return light


def random_history(rng, H, W, zero_share=0.2):
    """(PrevHistory, PrevMoments) with random contents; History.w = 0 (no history) on a share of the texels"""
    hist = rng.random((H, W, 4)).astype(F) * F(3)
    hist[..., 3] = rng.integers(1, 9, (H, W)).astype(F)
    hist[..., 3][rng.random((H, W)) < zero_share] = 0.0
    mom = rng.random((H, W, 4)).astype(F)
    mom[..., 3] = hist[..., 3]
    return hist, mom


# ---- what is not foreground, and what must not become an index
NOT_FOREGROUND = ("coverage", "zero normal", "nan normal", "inf normal")


def spoil(guide, ys, xs, kind):
    """make the texels (ys, xs) of `guide` non-foreground in the way `kind` names: coverage nextafter(1, 0), a zero normal, a NaN or an Inf
    normal component"""
    if kind == "coverage":
        guide["position"][ys, xs, 3] = np.nextafter(F(1), F(0))
    elif kind == "zero normal":
        guide["normal"][ys, xs, :3] = 0.0
    elif kind == "nan normal":
        guide["normal"][ys, xs, 1] = np.nan
    else:
        guide["normal"][ys, xs, 0] = np.inf


POSITIONS = (("nan", lambda P, eye, fwd: np.array([np.nan, P[1], P[2]], F)),
             ("inf", lambda P, eye, fwd: np.array([P[0], -np.inf, P[2]], F)),
             ("huge", lambda P, eye, fwd: np.array([F(3e38), F(-3e38), F(1e30)], F)),
             ("far", lambda P, eye, fwd: (P * F(1e12)).astype(F)),
             ("behind", lambda P, eye, fwd: (eye - fwd * F(2.5)).astype(F)),
             ("at the eye", lambda P, eye, fwd: eye.astype(F)))


def edge_case_frame(window=WINDOW, seed=7):
    """One launch's worth of caller-made images with every edge case of the pass in it: the 'corner' quads under a camera step, then
      current pixels of the four NOT_FOREGROUND kinds (rows 4 .. 7 of the foreground, columns spread over the window),
      previous texels of the same four kinds (a block each),
      current foreground pixels whose position.xyz is NaN, Inf, huge, far, behind the previous camera, or the previous eye itself.
    Returns a dict: g, guide, light, prev_g, prev_guide, prev_history, prev_moments and the masks `current_bad` {kind: (ys, xs)},
    `prev_bad` {kind: mask}, `odd_positions` {name: (y, x)}."""
    rng = np.random.default_rng(seed)
    prev_g, prev_guide, _ = two_quads("corner", 0, window)
    g, guide, ident = two_quads("corner", 1, window)
    W, H = window
    fg_y, fg_x = np.nonzero(ident)
    pick = rng.permutation(len(fg_y))
    current_bad, used = {}, 0
    for kind in NOT_FOREGROUND:
        sel = pick[used: used + 12]
        used += 12
        current_bad[kind] = (fg_y[sel], fg_x[sel])
        spoil(guide, fg_y[sel], fg_x[sel], kind)
    prev_bad = {}
    for k, kind in enumerate(NOT_FOREGROUND):
        mask = np.zeros((H, W), bool)
        y0, x0 = H // 2 + 2 + 4 * (k // 2), 6 + (W // 2) * (k % 2)
        mask[y0: y0 + 3, x0: x0 + 9] = True
        ys, xs = np.nonzero(mask)
        spoil(prev_guide, ys, xs, kind)
        prev_bad[kind] = mask
    eye = np.array([prev_g.view_inverse[12], prev_g.view_inverse[13], prev_g.view_inverse[14]], F)
    fwd = -np.array([prev_g.view_inverse[8], prev_g.view_inverse[9], prev_g.view_inverse[10]], F)  # the camera looks down its -z
    odd = {}
    for name, make in POSITIONS:
        for _ in range(3):
            i = pick[used]
            used += 1
            y, x = int(fg_y[i]), int(fg_x[i])
            guide["position"][y, x, :3] = make(guide["position"][y, x, :3].copy(), eye, fwd)
            odd.setdefault(name, []).append((y, x))
    light = (rng.random((H, W, 4)) * 2).astype(F)
    light[ident == 0] = np.array([np.nan, np.inf, -np.inf, -0.0], F)[rng.integers(0, 4, (int((ident == 0).sum()), 4))]  # passes through
    hist, mom = random_history(rng, H, W)
    return dict(g=g, guide=guide, light=light, prev_g=prev_g, prev_guide=prev_guide, prev_history=hist, prev_moments=mom, ident=ident,
                current_bad=current_bad, prev_bad=prev_bad, odd_positions=odd)


def random_frame(window, seed):
    """random guide images around a plane that both cameras see: positions jittered off the plane, normals jittered and of any length,
    coverage 1 on most texels, albedo on both sides of the 1/256 floor"""
    rng = np.random.default_rng(seed)
    W, H = window
    cam = dict(position=(0.2, 1.1, 3.0), direction=(-0.03, -0.2, -1.0), fov_deg=55.0)
    prev_g = orc.camera_gconst(width=W, height=H, **cam)
    g = orc.camera_gconst(width=W, height=H, **dict(cam, position=(0.26, 1.13, 2.97)))

    def guide_of(gc):
        ys, xs = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
        rays = orc.primary_rays(gc, xs.ravel(), ys.ravel())
        o, d = rays[0:3].T.reshape(H, W, 3), rays[3:6].T.reshape(H, W, 3)
        t = (F(-2.0) - o[..., 2]) / d[..., 2]  # the plane z = -2
        P = o + d * t[..., None] + (rng.standard_normal((H, W, 3)) * 0.004).astype(F)
        n = (np.array([0, 0, 1], F) + rng.standard_normal((H, W, 3)) * 0.25).astype(F) * rng.uniform(0.2, 3.0, (H, W, 1)).astype(F)
        cover = np.where(rng.random((H, W)) < 0.85, F(1), rng.random((H, W)).astype(F))
        return dict(position=np.concatenate([P, cover[..., None]], -1).astype(F), normal=np.concatenate([n, np.zeros((H, W, 1))], -1).astype(F),
                    albedo=np.concatenate([rng.random((H, W, 3)) ** 4, np.zeros((H, W, 1))], -1).astype(F),
                    emission=np.concatenate([rng.random((H, W, 3)) * 0.2, np.zeros((H, W, 1))], -1).astype(F))

    hist, mom = random_history(rng, H, W)
    return dict(g=g, guide=guide_of(g), light=(rng.random((H, W, 4)) * 2).astype(F), prev_g=prev_g, prev_guide=guide_of(prev_g), prev_history=hist,
                prev_moments=mom)


def ref_args(f):
    """the positional arguments of ref_temporal_guide.temporal from such a dict"""
    return f["g"], f["guide"], f["light"], f["prev_g"], f["prev_guide"], f["prev_history"], f["prev_moments"]
