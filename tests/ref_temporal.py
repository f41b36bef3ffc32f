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


def gbuffer_records(g, gb, depth):
    """{fg, P, n} of a frame's G-buffer, as a tap reads them: foreground by the depth, the position through the frame's own camera"""
    _, _, n = rd.unpack_gbuffer(gb)
    return dict(fg=depth != F(orc.BACKGROUND_DEPTH), P=positions(g, depth), n=n)


def temporal(g, gb, depth, light, prev_g, prev_gb, prev_depth, prev_history, prev_moments, alpha=0.2, alpha_moments=0.2, max_history=32,
             normal_cos=0.9, plane_tolerance=0.01, flags=0, stages=None):
    """(Out, History, Moments), each (H, W, 4) float32, of the "temporal" pass.  `stages` (a dict) receives intermediates."""
    return _temporal(g, gb, depth, light, prev_g, prev_gb, prev_depth, prev_history, prev_moments, None, None, alpha, alpha_moments, max_history,
                     normal_cos, plane_tolerance, flags, stages)


def _temporal(g, gb, depth, light, prev_g, prev_gb, prev_depth, prev_history, prev_moments, R, known, alpha, alpha_moments, max_history, normal_cos,
              plane_tolerance, flags, stages):
    """the pass over the G-buffers of this frame and of the previous one; R, known: accumulate()'s (ref_motion.temporal sets them)"""
    light = np.ascontiguousarray(light, F)
    with np.errstate(all="ignore"):
        cur = rd.prepare(g, gb, depth, light, demodulate=not (flags & NO_DEMODULATION))
        prev = gbuffer_records(prev_g, prev_gb, np.asarray(prev_depth, F))
        return accumulate(g, prev_g, light, cur, prev, prev_history, prev_moments, alpha, alpha_moments, max_history, normal_cos, plane_tolerance,
                          stages, R, known)


def accumulate(g, prev_g, light, cur, prev, prev_history, prev_moments, alpha, alpha_moments, max_history, normal_cos, plane_tolerance, stages=None,
               R=None, known=None):
    """Steps 3 to 5 of the pass -- reprojection, the four taps, the blend -- for whichever source the records come from.  `cur`: this
    frame's record {fg, P, n, c, m, e} (ref_denoise.prepare's dict); `prev`: the previous frame's {fg, P, n}, which a tap reads.  `R` (H,
    W, 3): the points that are looked up in the previous frame instead of P, and `known` (H, W) bool: whether a pixel has one (the motion
    input); the tolerance, the normal and the record stay this frame's."""
    prev_history, prev_moments = np.asarray(prev_history, F), np.asarray(prev_moments, F)
    alpha, alpha_m, max_history, normal_cos, plane_tol = F(alpha), F(alpha_moments), F(max_history), F(normal_cos), F(plane_tolerance)
    H, W = light.shape[:2]
    assert (prev_g.window_size[0], prev_g.window_size[1]) == (g.window_size[0], g.window_size[1]) == (W, H)
    fg, P, n, c, m, e = cur["fg"], cur["P"], cur["n"], cur["c"], cur["m"], cur["e"]
    prev_fg, prev_P, prev_n = prev["fg"], prev["P"], prev["n"]
    l = rd._lum(c)
    zero = np.zeros((H, W), F)
    # step 3: reprojection
    if R is None:
        R = P
    valid, sx, sy = reproject(g, prev_g, R)
    valid = valid & fg
    if known is not None:
        valid = valid & known
    x0f, y0f = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0f, sy - y0f
    x0 = np.where(valid, x0f, F(0)).astype(np.int32)
    y0 = np.where(valid, y0f, F(0)).astype(np.int32)
    eye = np.array([g.view_inverse[12], g.view_inverse[13], g.view_inverse[14]], F)
    dE = P - eye
    tol = plane_tol * np.sqrt(rd._dot(dE, dE))
    # step 4: the four taps, rows outer
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
            dP = prev_P[cy, cx] - R
            counts = (inside & prev_fg[cy, cx] & (ph[..., 3] > F(0)) & (rd._dot(n, prev_n[cy, cx]) >= normal_cos)
                      & (np.abs(rd._dot(n, dP)) <= tol))
            wt = wx * wy
            ws = ws + np.where(counts, wt, F(0))
            hs = hs + np.where(counts[..., None], wt[..., None] * ph, F(0))
            ks = ks + np.where(counts[..., None], wt[..., None] * pm[..., :2], F(0))
    # step 5: the blend
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
    image {mu1, mu2, variance, N} of temporal(): ref_denoise.denoise_records over the G-buffer's records.  With `moments` None this is
    ref_denoise.denoise, bit for bit (tests/test_temporal_cpu.py holds the two together)."""
    return rd.denoise_records(lambda light, demodulate: rd.prepare(g, gb, depth, light, demodulate), light, moments, iterations, normal_squarings,
                              sigma_z, sigma_l, flags, stages)
