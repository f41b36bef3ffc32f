"""numpy float32 restatement of the "denoise" pass: the edge-avoiding a-trous wavelet filter that librt3 runs on
the G-buffer.  The GPU pass must equal `denoise()` bit for bit, so every line below is ONE rounded device operation on float32 arrays, in
the device's order: `+ - * /` and `sqrt` only, min / max as selects, no fused multiply-add, taps accumulated rows outer (dy), columns
inner (dx).  G-buffer unpacking and the primary ray are the oracle's (orc_gbuffer_unpack, orc.primary_rays): not restated here.

Taps outside the window are skipped by the device; here they read a zero border (normal 0 -> weight exactly 0 -> the sums receive +0,
which leaves every bit of them alone).  Background pixels carry the same zero record, so they never contribute either.
"""
from __future__ import annotations

import numpy as np

import orc

F = np.float32
NO_DEMODULATION = 1  # rt3_denoise_params.flags: RT3_DENOISE_NO_DEMODULATION
DEFAULTS = dict(iterations=5, normal_squarings=7, sigma_z=0.05, sigma_l=4.0, flags=0)
H5 = [F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16)]  # B3 spline
K3 = [F(0.25), F(0.5), F(0.25)]
LUM = (F(0.2126), F(0.7152), F(0.0722))
TINY_R = F(1e-20)
TINY_L = F(1e-6)
ALBEDO_FLOOR = F(1.0 / 256.0)

# expn(x) = e^-x, x >= 0: t = x * log2(e) (one rounding); i = int(t + 1/2); f = t - i (exact, |f| <= 1/2); 2^-f by the degree-7 Taylor
# polynomial of exp(-f ln 2) in Horner form; scaled by 2^-i in two exact-power-of-two steps so that results below 2^-126 round once, as a
# denormal; 0 from t >= 150 on (2^-150 is the tie that rounds to 0), which +inf and NaN reach too.
LOG2E = F(1.4426950408889634)
EXPN_C = [F(c) for c in (1.0, -6.931471805599453e-01, 2.402265069591007e-01, -5.550410866482158e-02, 9.618129107628477e-03,
                         -1.3333558146428443e-03, 1.5403530393381608e-04, -1.5252733804059841e-05)]
EXPN_CUT = F(150.0)


def _exp2_neg_int(i):
    """2^-i for int32 i in [0, 126], by building the exponent bits"""
    return ((127 - i).astype(np.uint32) << np.uint32(23)).view(np.float32)


def expn(x):
    x = np.asarray(x, F)
    with np.errstate(over="ignore"):
        t = x * LOG2E
    live = t < EXPN_CUT
    tc = np.where(live, t, F(0))
    i = (tc + F(0.5)).astype(np.int32)
    f = tc - i.astype(F)
    p = np.full_like(f, EXPN_C[7])
    for k in range(6, -1, -1):
        p = p * f + EXPN_C[k]
    i0 = i >> 1
    r = (p * _exp2_neg_int(i0)) * _exp2_neg_int(i - i0)
    return np.where(live, r, F(0)).astype(F)


def unpack_gbuffer(gb):
    """(albedo, emission, normal) float32 (H, W, 3) by the oracle's gbuffer_unpack, one call per distinct G-buffer word"""
    H, W = gb.shape[:2]
    rows, inv = np.unique(gb.reshape(-1, 4), axis=0, return_inverse=True)
    rows = np.ascontiguousarray(rows, np.uint32)
    un = np.zeros((len(rows), 11), F)
    L = orc.lib()
    for k in range(len(rows)):
        L.orc_gbuffer_unpack(orc.ptr(rows[k:k + 1]), orc.ptr(un[k:k + 1]))
    un = un[inv.reshape(-1)].reshape(H, W, 11)
    return un[..., 0:3].copy(), un[..., 3:6].copy(), un[..., 6:9].copy()


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _lum(c):
    return (LUM[0] * c[..., 0] + LUM[1] * c[..., 1]) + LUM[2] * c[..., 2]


def prepare(g, gb, depth, light, demodulate=True):
    """stage 1: per-pixel records.  P, n (H, W, 3), c (H, W, 3), m, e (modulation), fg (H, W) bool; background records are all zero"""
    H, W = depth.shape
    fg = depth != F(orc.BACKGROUND_DEPTH)
    alb, emi, nrm = unpack_gbuffer(gb)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    rays = orc.primary_rays(g, xs.ravel(), ys.ravel())
    o = rays[0:3].T.reshape(H, W, 3)
    d = rays[3:6].T.reshape(H, W, 3)
    P = o + d * depth[..., None]
    if demodulate:
        m = np.where(alb > ALBEDO_FLOOR, alb, ALBEDO_FLOOR)
        e = emi
    else:
        m = np.ones((H, W, 3), F)
        e = np.zeros((H, W, 3), F)
    with np.errstate(all="ignore"):
        c = (light[..., :3] - e) / m
    z = np.zeros((H, W, 3), F)
    f3 = fg[..., None]
    return dict(P=np.where(f3, P, z), n=np.where(f3, nrm, z), c=np.where(f3, c, z), m=m, e=e, fg=fg)


class _Taps:
    """zero-bordered copies of the per-pixel images, and the geometric terms of the tap at (dy, dx): w_n, and the exponent x_z of
    w_z = expn(x_z)"""

    def __init__(self, P, n, reach, squarings, inv_sigma_z):
        self.H, self.W = P.shape[:2]
        self.R = reach
        self.P, self.n = P, n
        self.Pp, self.np_ = self.pad(P), self.pad(n)
        self.squarings, self.isz = squarings, F(inv_sigma_z)

    def pad(self, a):
        R = self.R
        return np.pad(a, [(R, R), (R, R)] + [(0, 0)] * (a.ndim - 2))

    def at(self, padded, dy, dx):
        R = self.R
        return padded[R + dy:R + dy + self.H, R + dx:R + dx + self.W]

    def geo(self, dy, dx):
        nq, Pq = self.at(self.np_, dy, dx), self.at(self.Pp, dy, dx)
        dn = _dot(self.n, nq)
        wn = np.where(dn > F(0), dn, F(0))
        for _ in range(self.squarings):
            wn = wn * wn
        dP = Pq - self.P
        r = np.sqrt(_dot(dP, dP))
        dd = np.abs(_dot(self.n, dP))
        return wn, (dd / (r + TINY_R)) * self.isz


def denoise(g, gb, depth, light, iterations=5, normal_squarings=7, sigma_z=0.05, sigma_l=4.0, flags=0, stages=None):
    """Out (H, W, 4) float32 of the "denoise" pass.  `stages` (a dict) receives the intermediate images for debugging."""
    return denoise_records(lambda light, demodulate: prepare(g, gb, depth, light, demodulate), light, None, iterations, normal_squarings, sigma_z,
                           sigma_l, flags, stages)


def denoise_records(prepare_fn, light, moments=None, iterations=5, normal_squarings=7, sigma_z=0.05, sigma_l=4.0, flags=0, stages=None):
    """The pass over the records of `prepare_fn(light, demodulate)` (prepare()'s dict, from whichever source: the G-buffer here, the guide
    images in ref_guide) and, with `moments`, the variance input (rt3_denoise_set_variance_input): the Moments image {mu1, mu2, variance,
    N} of ref_temporal.temporal(), whose z replaces the result of the 7 x 7 stage per foreground pixel where w >= 4."""
    light = np.ascontiguousarray(light, F)
    if iterations == 0:
        return light.copy()
    with np.errstate(all="ignore"):
        pr = prepare_fn(light, not (flags & NO_DEMODULATION))
        return _denoise(pr, light, moments, iterations, normal_squarings, F(sigma_z), F(sigma_l), stages)


def _denoise(pr, light, moments, iterations, squarings, sigma_z, sigma_l, stages):
    H, W = light.shape[:2]
    fg, c = pr["fg"], pr["c"]
    reach = max(3, 2 << (iterations - 1))
    T = _Taps(pr["P"], pr["n"], reach, squarings, F(1.0) / sigma_z)
    zero = np.zeros((H, W), F)
    # stage 2: spatial variance of the luminance over 7 x 7, weighted by w_n * w_z
    lp = T.pad(_lum(c))
    s0, s1, s2 = zero.copy(), zero.copy(), zero.copy()
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            wn, xz = T.geo(dy, dx)
            w = wn * expn(xz)
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
                k = K3[dy + 1] * K3[dx + 1]
                gs = gs + k * T.at(vp, dy, dx)
                ks = ks + k * T.at(ones, dy, dx)
        gv = gs / ks
        inv_l = F(1.0) / (sigma_l * np.sqrt(gv) + TINY_L)
        l = _lum(c)
        lp = T.pad(l)
        acc = np.zeros((H, W, 3), F)
        ws, vs = zero.copy(), zero.copy()
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                h = H5[dy + 2] * H5[dx + 2]
                wn, xz = T.geo(dy * st, dx * st)
                xl = np.abs(T.at(lp, dy * st, dx * st) - l) * inv_l
                w = (h * wn) * expn(xz + xl)  # w_z * w_l = e^-(x_z + x_l): one expn per tap
                cq = T.at(cp, dy * st, dx * st)
                acc = acc + w[..., None] * cq
                ws = ws + w
                vs = vs + (w * w) * T.at(vp, dy * st, dx * st)
        c = np.where(fg[..., None], acc / ws[..., None], np.zeros((H, W, 3), F))
        var = np.where(fg, vs / (ws * ws), zero)
        if stages is not None:
            stages[f"c{it}"], stages[f"var{it + 1}"] = c.copy(), var.copy()
    # stage 4
    out = light.copy()
    rgb = pr["e"] + c * pr["m"]
    out[..., :3] = np.where(fg[..., None], rgb, light[..., :3])
    return out
