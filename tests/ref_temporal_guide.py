"""numpy float32 restatement of the "temporal" pass guided by the camera samples (k_temporal<TemporalGuide>): reprojected
accumulation whose surface records come from the guide images of this frame and of the previous one instead of the pinhole G-buffer.
The GPU pass must equal `temporal()` bit for bit, so every line below is ONE rounded device operation on float32 arrays, in the device's
order: `+ - * /` and `sqrt` only, min / max as selects, no fused multiply-add.

What is shared is imported, not restated: the foreground rule, the normalisation and this frame's record are ref_guide's (foreground,
unit_normal, prepare_guide -- the records of k_dn_prepare<DnGuide>); the reprojection, the four taps and the blend are
ref_temporal.accumulate, the same lines that serve the G-buffer.  What differs is where a tap's record comes from: the previous guide is
foreground at the tap by the same rule, its normal is normalised the same way, and its position is read, not reconstructed through the
previous camera.  previous.albedo and previous.emission are not read.

denoise() is the guided "denoise" of ref_guide with the variance input: what follows a guided "temporal" in a frame.
"""
from __future__ import annotations

import numpy as np

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
    guide, prev_guide = _images(guide), _images(prev_guide, ("position", "normal"))
    with np.errstate(all="ignore"):
        # steps 1 and 2: this frame's record is prepare_guide's (P, n, c are zero off the foreground); a tap's comes from the previous guide
        cur = rgd.prepare_guide(guide, light, demodulate=not (flags & NO_DEMODULATION))
        prev_fg, prev_l2 = rgd.foreground(prev_guide)
        prev = dict(fg=prev_fg, P=prev_guide["position"][..., :3], n=rgd.unit_normal(prev_guide, prev_l2))
        out = rt.accumulate(g, prev_g, light, cur, prev, prev_history, prev_moments, alpha, alpha_moments, max_history, normal_cos, plane_tolerance,
                            stages)
    if stages is not None:
        stages["prev_fg"] = prev_fg
    return out


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
