"""numpy float32 restatement of the "temporal" pass: reprojected accumulation of the demodulated radiance and of
its luminance moments.  The GPU pass must equal `temporal()` bit for bit, so every line below is ONE rounded device operation on float32
arrays, in the device's order: `+ - * /` and `sqrt` only, min / max as selects, no fused multiply-add.  G-buffer unpacking and the primary
ray are the oracle's (ref_denoise.unpack_gbuffer, orc.primary_rays -- the latter with the previous GConst for the taps' positions); the
surface record (P, n, c, m, e) is ref_denoise.prepare(), the one the "denoise" pass uses.

Association order, chosen here and followed by the device: a matrix row times a vector is summed left to right,
((m0 x + m4 y) + m8 z) + m12 w, like primary_ray in rt3_camera.hpp; the four taps are accumulated rows outer (j), columns inner (i); a
tap's bilinear weight is w_x * w_y.  A tap that does not count is skipped by the device; here it adds +0, which leaves every bit of a sum
that started at +0 alone.  `floor` and the float -> int conversion are exact, and are applied only after the window test in float.
"""
from __future__ import annotations

import numpy as np

import orc
import ref_denoise as rd

F = np.float32
NO_DEMODULATION = 1  # rt3_temporal_params.flags: RT3_TEMPORAL_NO_DEMODULATION
DEFAULTS = dict(alpha=0.2, alpha_moments=0.2, max_history=32, normal_cos=0.9, plane_tolerance=0.01, flags=0)


def _mat_row(m, r, x, y, z, w):
    return ((F(m[r]) * x + F(m[4 + r]) * y) + F(m[8 + r]) * z) + F(m[12 + r]) * w


def positions(g, depth):
    """world position per pixel: o + d t with the oracle's primary ray under `g`"""
    H, W = depth.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    rays = orc.primary_rays(g, xs.ravel(), ys.ravel())
    o = rays[0:3].T.reshape(H, W, 3)
    d = rays[3:6].T.reshape(H, W, 3)
    return o + d * depth[..., None]


def reproject(g, prev_g, P):
    """(valid, sx, sy): the float position of world points P (H, W, 3) in the previous view, and whether it has one inside (-1, W) x (-1, H)"""
    W, H = F(g.window_size[0]), F(g.window_size[1])
    one = F(1.0)
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    v = [_mat_row(prev_g.view, r, x, y, z, one) for r in range(4)]
    qx, qy, qw = (_mat_row(prev_g.proj, r, v[0], v[1], v[2], v[3]) for r in (0, 1, 3))
    ndx, ndy = qx / qw, qy / qw
    sx = (ndx * F(0.5) + F(0.5)) * W - F(0.5)
    sy = (-ndy * F(0.5) + F(0.5)) * H - F(0.5)
    valid = (qw > F(0)) & (sx > F(-1)) & (sx < W) & (sy > F(-1)) & (sy < H)
    return valid, sx, sy


def temporal(g, gb, depth, light, prev_g, prev_gb, prev_depth, prev_history, prev_moments, alpha=0.2, alpha_moments=0.2, max_history=32,
             normal_cos=0.9, plane_tolerance=0.01, flags=0, stages=None):
    """(Out, History, Moments), each (H, W, 4) float32, of the "temporal" pass.  `stages` (a dict) receives intermediates."""
    light = np.ascontiguousarray(light, F)
    with np.errstate(all="ignore"):
        return _temporal(g, gb, depth, light, prev_g, prev_gb, np.asarray(prev_depth, F), np.asarray(prev_history, F), np.asarray(prev_moments, F),
                         F(alpha), F(alpha_moments), F(max_history), F(normal_cos), F(plane_tolerance), flags, stages)


def _temporal(g, gb, depth, light, prev_g, prev_gb, prev_depth, prev_history, prev_moments, alpha, alpha_m, max_history, normal_cos, plane_tol, flags,
              stages):
    H, W = depth.shape
    assert (prev_g.window_size[0], prev_g.window_size[1]) == (g.window_size[0], g.window_size[1]) == (W, H)
    BG = F(orc.BACKGROUND_DEPTH)
    pr = rd.prepare(g, gb, depth, light, demodulate=not (flags & NO_DEMODULATION))
    fg, P, n, c, m, e = pr["fg"], pr["P"], pr["n"], pr["c"], pr["m"], pr["e"]
    l = rd._lum(c)
    zero = np.zeros((H, W), F)
    # reprojection
    valid, sx, sy = reproject(g, prev_g, P)
    valid = valid & fg
    x0f, y0f = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0f, sy - y0f
    x0 = np.where(valid, x0f, F(0)).astype(np.int32)
    y0 = np.where(valid, y0f, F(0)).astype(np.int32)
    eye = np.array([g.view_inverse[12], g.view_inverse[13], g.view_inverse[14]], F)
    dE = P - eye
    tol = plane_tol * np.sqrt(rd._dot(dE, dE))
    # the previous frame's records
    _, _, prev_n = rd.unpack_gbuffer(prev_gb)
    prev_P = positions(prev_g, prev_depth)
    ws = zero.copy()
    hs = np.zeros((H, W, 4), F)
    ks = np.zeros((H, W, 2), F)
    for j in (0, 1):
        ty = y0 + j
        wy = fy if j else F(1.0) - fy
        for i in (0, 1):
            tx = x0 + i
            wx = fx if i else F(1.0) - fx
            inside = valid & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            cy, cx = np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)
            ph, pm = prev_history[cy, cx], prev_moments[cy, cx]
            dP = prev_P[cy, cx] - P
            counts = (inside & (prev_depth[cy, cx] != BG) & (ph[..., 3] > F(0)) & (rd._dot(n, prev_n[cy, cx]) >= normal_cos)
                      & (np.abs(rd._dot(n, dP)) <= tol))
            wt = wx * wy
            ws = ws + np.where(counts, wt, F(0))
            hs = hs + np.where(counts[..., None], wt[..., None] * ph, F(0))
            ks = ks + np.where(counts[..., None], wt[..., None] * pm[..., :2], F(0))
    has = ws > F(0)
    h = hs / ws[..., None]
    k = ks / ws[..., None]
    n1 = h[..., 3] + F(1.0)
    N = np.where(n1 < max_history, n1, max_history)
    inv = F(1.0) / N
    ac = np.where(alpha > inv, alpha, inv)
    am = np.where(alpha_m > inv, alpha_m, inv)
    ll = l * l
    c_hist = h[..., :3] + ac[..., None] * (c - h[..., :3])
    mu1_hist = k[..., 0] + am * (l - k[..., 0])
    mu2_hist = k[..., 1] + am * (ll - k[..., 1])
    N = np.where(has, N, F(1.0)).astype(F)
    c_acc = np.where(has[..., None], c_hist, c).astype(F)
    mu1 = np.where(has, mu1_hist, l).astype(F)
    mu2 = np.where(has, mu2_hist, ll).astype(F)
    d = mu2 - mu1 * mu1
    var = np.where(d > F(0), d, F(0))
    rgb = e + c_acc * m
    f3 = fg[..., None]
    history = np.where(f3, np.concatenate([c_acc, N[..., None]], -1), F(0)).astype(F)
    moments = np.where(f3, np.stack([mu1, mu2, var, N], -1), F(0)).astype(F)
    out = light.copy()
    out[..., :3] = np.where(f3, rgb, light[..., :3])
    if stages is not None:
        stages.update(valid=valid, sx=sx, sy=sy, ws=ws, has=has & fg, c=c, l=l, fg=fg)
    return out, history, moments


def denoise(g, gb, depth, light, moments=None, iterations=5, normal_squarings=7, sigma_z=0.05, sigma_l=4.0, flags=0, stages=None):
    """Out (H, W, 4) float32 of the "denoise" pass with the variance input (rt3_denoise_set_variance_input) set to `moments`, the Moments
    image {mu1, mu2, variance, N} of temporal(): the result of the 7 x 7 stage is replaced per foreground pixel by Moments.z where
    Moments.w >= 4.  The stages are those of ref_denoise.denoise, restated from its parts (prepare, the tap geometry, expn) line for line;
    with `moments` None this is that function, bit for bit (tests/test_temporal_cpu.py holds the two together)."""
    light = np.ascontiguousarray(light, F)
    if iterations == 0:
        return light.copy()
    with np.errstate(all="ignore"):
        return _denoise(g, gb, depth, light, moments, iterations, normal_squarings, F(sigma_z), F(sigma_l), flags, stages)


def _denoise(g, gb, depth, light, moments, iterations, squarings, sigma_z, sigma_l, flags, stages):
    H, W = depth.shape
    pr = rd.prepare(g, gb, depth, light, demodulate=not (flags & rd.NO_DEMODULATION))
    fg, c = pr["fg"], pr["c"]
    reach = max(3, 2 << (iterations - 1))
    T = rd._Taps(pr["P"], pr["n"], reach, squarings, F(1.0) / sigma_z)
    zero = np.zeros((H, W), F)
    # stage 2: spatial variance of the luminance over 7 x 7, weighted by w_n * w_z
    lp = T.pad(rd._lum(c))
    s0, s1, s2 = zero.copy(), zero.copy(), zero.copy()
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            wn, xz = T.geo(dy, dx)
            w = wn * rd.expn(xz)
            lq = T.at(lp, dy, dx)
            s0 = s0 + w
            s1 = s1 + w * lq
            s2 = s2 + w * (lq * lq)
    mu1 = s1 / s0
    d = s2 / s0 - mu1 * mu1
    var = np.where(fg, np.where(d > F(0), d, F(0)), zero)
    if stages is not None:
        stages["var_spatial"] = var.copy()
    if moments is not None:  # the temporal variance where the history is at least four frames long (SVGF's rule)
        var = np.where(fg & (moments[..., 3] >= F(4)), moments[..., 2].astype(F), var)
    if stages is not None:
        stages["var0"] = var.copy()
    ones = T.pad(np.ones((H, W), F))
    # stage 3: a-trous iterations
    for it in range(iterations):
        st = 1 << it
        vp, cp = T.pad(var), T.pad(c)
        gs, ks = zero.copy(), zero.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k = rd.K3[dy + 1] * rd.K3[dx + 1]
                gs = gs + k * T.at(vp, dy, dx)
                ks = ks + k * T.at(ones, dy, dx)
        gv = gs / ks
        inv_l = F(1.0) / (sigma_l * np.sqrt(gv) + rd.TINY_L)
        l = rd._lum(c)
        lp = T.pad(l)
        acc = np.zeros((H, W, 3), F)
        ws, vs = zero.copy(), zero.copy()
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                h = rd.H5[dy + 2] * rd.H5[dx + 2]
                wn, xz = T.geo(dy * st, dx * st)
                xl = np.abs(T.at(lp, dy * st, dx * st) - l) * inv_l
                w = (h * wn) * rd.expn(xz + xl)
                cq = T.at(cp, dy * st, dx * st)
                acc = acc + w[..., None] * cq
                ws = ws + w
                vs = vs + (w * w) * T.at(vp, dy * st, dx * st)
        c = np.where(fg[..., None], acc / ws[..., None], np.zeros((H, W, 3), F))
        var = np.where(fg, vs / (ws * ws), zero)
    # stage 4
    out = light.copy()
    rgb = pr["e"] + c * pr["m"]
    out[..., :3] = np.where(fg[..., None], rgb, light[..., :3])
    return out
