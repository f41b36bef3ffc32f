"""numpy float32 restatement of the "temporal" pass guided by the camera samples (k_temporal_guide): reprojected
accumulation whose surface records come from the guide images of this frame and of the previous one instead of the pinhole G-buffer.
The GPU pass must equal `temporal()` bit for bit, so every line below is ONE rounded device operation on float32 arrays, in the device's
order: `+ - * /` and `sqrt` only, min / max as selects, no fused multiply-add.

What is shared is imported, not restated: the foreground rule and the normalisation are ref_guide's (foreground, prepare_guide -- the
records of k_dn_prepare_guide), the matrix rows and the reprojection are ref_temporal's (_mat_row, reproject).  Steps 4 and 5 -- the four
taps, rows outer, and the blend -- follow ref_temporal._temporal line for line; what differs is where a tap's record comes from: the
previous guide is foreground at the tap by the same rule, its normal is normalised the same way, and its position is read, not
reconstructed through the previous camera.  A tap that does not count adds +0.  previous.albedo and previous.emission are not read.

denoise() is the guided "denoise" of ref_guide with the variance input: what follows a guided "temporal" in a frame.
"""
from __future__ import annotations

import numpy as np

import ref_denoise as rd
import ref_guide as rgd
import ref_temporal as rt

F = np.float32
NO_DEMODULATION = rt.NO_DEMODULATION
DEFAULTS = rt.DEFAULTS
KEYS = rgd.KEYS


def _images(guide, keys=KEYS):
    return {k: np.ascontiguousarray(guide[k], F) for k in keys}


def temporal(g, guide, light, prev_g, prev_guide, prev_history, prev_moments, alpha=0.2, alpha_moments=0.2, max_history=32, normal_cos=0.9,
             plane_tolerance=0.01, flags=0, stages=None):
    """(Out, History, Moments), each (H, W, 4) float32, of "temporal" with the guide input set to (`guide`, `prev_guide`): dicts
    {position, normal, albedo, emission} -> (H, W, 4) (`prev_guide` needs position and normal only).  `g`, `prev_g`: the GConst of this
    frame and of the previous one (view, proj, view_inverse, window_size are read).  `stages` (a dict) receives intermediates."""
    light = np.ascontiguousarray(light, F)
    with np.errstate(all="ignore"):
        return _temporal(g, _images(guide), light, prev_g, _images(prev_guide, ("position", "normal")), np.asarray(prev_history, F),
                         np.asarray(prev_moments, F), F(alpha), F(alpha_moments), F(max_history), F(normal_cos), F(plane_tolerance), flags, stages)


def _temporal(g, guide, light, prev_g, prev_guide, prev_history, prev_moments, alpha, alpha_m, max_history, normal_cos, plane_tol, flags, stages):
    H, W = light.shape[:2]
    assert (prev_g.window_size[0], prev_g.window_size[1]) == (g.window_size[0], g.window_size[1]) == (W, H)
    # steps 1 and 2: the record of k_dn_prepare_guide (P, n, c are zero off the foreground)
    pr = rgd.prepare_guide(guide, light, demodulate=not (flags & NO_DEMODULATION))
    fg, P, n, c, m, e = pr["fg"], pr["P"], pr["n"], pr["c"], pr["m"], pr["e"]
    l = rd._lum(c)
    zero = np.zeros((H, W), F)
    # step 3: reprojection
    valid, sx, sy = rt.reproject(g, prev_g, P)
    valid = valid & fg
    x0f, y0f = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0f, sy - y0f
    x0 = np.where(valid, x0f, F(0)).astype(np.int32)
    y0 = np.where(valid, y0f, F(0)).astype(np.int32)
    eye = np.array([g.view_inverse[12], g.view_inverse[13], g.view_inverse[14]], F)
    dE = P - eye
    tol = plane_tol * np.sqrt(rd._dot(dE, dE))
    # the previous frame's records
    prev_fg, prev_l2 = rgd.foreground(prev_guide)
    prev_inv = F(1.0) / np.sqrt(prev_l2)
    prev_n = prev_guide["normal"][..., :3] * prev_inv[..., None]
    prev_P = prev_guide["position"][..., :3]
    # step 4
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
            counts = (inside & prev_fg[cy, cx] & (ph[..., 3] > F(0)) & (rd._dot(n, prev_n[cy, cx]) >= normal_cos)
                      & (np.abs(rd._dot(n, dP)) <= tol))
            wt = wx * wy
            ws = ws + np.where(counts, wt, F(0))
            hs = hs + np.where(counts[..., None], wt[..., None] * ph, F(0))
            ks = ks + np.where(counts[..., None], wt[..., None] * pm[..., :2], F(0))
    # step 5
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
        stages.update(valid=valid, sx=sx, sy=sy, ws=ws, has=has & fg, c=c, l=l, fg=fg, prev_fg=prev_fg)
    return out, history, moments


def denoise(guide, light, moments=None, **params):
    """Out of "denoise" guided by `guide` with the variance input `moments` (the Moments of temporal()): ref_guide.denoise"""
    return rgd.denoise(guide, light, moments=moments, **params)


# ---- the running mean under a static camera and a constant guide (tests/test_temporal_guide_cpu.py, tests/test_temporal_guide.py)
U = 2.0 ** -24
GAMMA_8 = 8 * U / (1 - 8 * U)
GAMMA_11 = 11 * U / (1 - 11 * U)  # test_temporal_cpu.STEP_ROUNDING


def history_length_bound(K):
    """|N - K| allowed after K frames in which every foreground pixel keeps its history (static camera, the same guide every frame,
    max_history >= K).  Frame k computes hn = (sum_t w_t N_t) / (sum_t w_t) over at most four taps with weights >= 0: a product and at
    most three additions per term above, three additions below, one division -- gamma_8 relative to the largest N_t.  With every N_t
    within d_{k-1} of k - 1: |hn - (k - 1)| <= d_{k-1} + gamma_8 (k - 1 + d_{k-1}); n1 = hn + 1 rounds once: u k more; the select against
    max_history is exact.  So d_k <= d_{k-1} + 9 u k to first order, d_1 = 0 (no tap counts: N = 1 exactly), and
    d_K <= 9 u K (K + 1) / 2; times 1.01 for the terms of second order."""
    return 1.01 * 9 * U * K * (K + 1) / 2


def running_mean_bound(K, scale):
    """|History.rgb - mean(c_1 .. c_K)| allowed per channel after K such frames with alpha = 0, when c_k is the same value at every pixel
    of frame k and |c_k| <= scale.  Frame k computes c_acc = h + a (c_k - h), h = (sum_t w_t v_t) / (sum_t w_t), a = 1 / N.
      h: the taps hold values within d_{k-1} of the exact mean M_{k-1} of c_1 .. c_{k-1} (every pixel was fed the same values), so
      |h - M_{k-1}| <= d_{k-1} + gamma_8 scale (the weighted mean of history_length_bound);
      the blend: 1 / N, the difference, the product and the sum round once each, each relative to at most 2 scale or scale: with h's
      gamma_8 that is test_temporal_cpu's gamma_11 scale per launch (its STEP_ROUNDING, derived there the same way);
      a: N misses k by at most history_length_bound(k) <= 9 u k (k + 1) / 2, so 1 / N misses 1 / k by that over k^2, at most 9 u, and
      the product a (c_k - h) moves by at most 9 u 2 scale = 18 u scale.
    The error of frame k - 1 enters frame k with the factor 1 - a <= 1, so d_K <= K (gamma_11 + 18 u) scale; times 1.01 for the terms
    of second order."""
    return 1.01 * K * (GAMMA_11 + 18 * U) * scale
