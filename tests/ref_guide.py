"""numpy float32 restatement of the guide images of a lens frame and of the "denoise" pass guided by them.

accumulate() is k_lens_guide: per pixel the first-vertex features of the camera samples, summed in sample order, one rounding per written
operation, no fused multiply-add; between batches the images hold the running sums with the hit count in position.w, so the result does
not depend on how the samples are split.  prepare_guide() is k_dn_prepare<DnGuide>; denoise() hands it to
ref_denoise.denoise_records, which runs stages 2 to 4 over whichever records it is given -- the variance stage (with the variance
input), the a-trous iterations and the modulation are not restated here.  The GPU equals both bit for bit.
"""
from __future__ import annotations

import numpy as np

import ref_denoise as rd

F = np.float32
U = 2.0 ** -24
KEYS = ("position", "normal", "albedo", "emission")


def zero_state(npix):
    return {k: np.zeros((npix, 4), F) for k in KEYS}


def accumulate(hit, o, d, t, normal, albedo, emissive, samples, state=None, first=True, last=True):
    """One batch of k_lens_guide.  hit (nsb, npix) bool; o, d (nsb, npix, 3) the camera rays; t (nsb, npix) the hit distances; normal,
    albedo, emissive (nsb, npix, 3) hit_info's words for the hits (anything where `hit` is False); `samples` the frame's sample count S.
    `state`: the four images as the previous batch left them (read unless `first`).  Returns {position, normal, albedo, emission}, each
    (npix, 4) float32: the running sums, or with `last` the means."""
    hit = np.asarray(hit, bool)
    nsb, npix = hit.shape
    o, d, normal, albedo, emissive = (np.asarray(a, F).reshape(nsb, npix, 3) for a in (o, d, normal, albedo, emissive))
    t = np.asarray(t, F).reshape(nsb, npix)
    if first:
        state = zero_state(npix)
    sP, sN, sA, sE = (np.array(state[k], F) for k in KEYS)
    one = F(1.0)
    with np.errstate(all="ignore"):
        for s in range(nsb):
            h = hit[s]
            h3 = h[:, None]
            P = o[s] + d[s] * t[s][:, None]
            sP[:, :3] = np.where(h3, sP[:, :3] + P, sP[:, :3])
            sP[:, 3] = np.where(h, sP[:, 3] + one, sP[:, 3])
            sN[:, :3] = np.where(h3, sN[:, :3] + normal[s], sN[:, :3])
            sA[:, :3] = np.where(h3, sA[:, :3] + albedo[s], sA[:, :3] + one)
            sE[:, :3] = np.where(h3, sE[:, :3] + emissive[s], sE[:, :3])
        if last:
            fs = F(samples)
            nh = sP[:, 3].copy()
            some = nh > F(0)
            z = np.zeros((npix, 4), F)
            pos = np.concatenate([sP[:, :3] / nh[:, None], (nh / fs)[:, None]], -1)
            nrm = np.concatenate([sN[:, :3] / nh[:, None], np.zeros((npix, 1), F)], -1)
            sP = np.where(some[:, None], pos, z).astype(F)
            sN = np.where(some[:, None], nrm, z).astype(F)
            sA = np.concatenate([sA[:, :3] / fs, np.zeros((npix, 1), F)], -1).astype(F)
            sE = np.concatenate([sE[:, :3] / fs, np.zeros((npix, 1), F)], -1).astype(F)
    return dict(position=sP, normal=sN, albedo=sA, emission=sE)


def accumulate_split(hit, o, d, t, normal, albedo, emissive, batch):
    """the whole frame in batches of `batch` samples, as RT3_OPT_BATCH_SPP splits it"""
    S = len(hit)
    state = None
    for s0 in range(0, S, batch):
        sl = slice(s0, min(s0 + batch, S))
        state = accumulate(hit[sl], o[sl], d[sl], t[sl], normal[sl], albedo[sl], emissive[sl], S, state, first=s0 == 0, last=s0 + batch >= S)
    return state


def foreground(guide):
    """(fg, l2): every sample hit, and the summed normal has a finite, positive squared length"""
    N = guide["normal"]
    with np.errstate(all="ignore"):
        l2 = (N[..., 0] * N[..., 0] + N[..., 1] * N[..., 1]) + N[..., 2] * N[..., 2]
        fg = (guide["position"][..., 3] == F(1.0)) & (l2 > F(0)) & (l2 <= np.finfo(F).max)
    return fg, l2


def unit_normal(guide, l2):
    """normal.xyz * (1 / sqrt(l2)), the device header's normalize"""
    with np.errstate(all="ignore"):
        inv = F(1.0) / np.sqrt(l2)
        return guide["normal"][..., :3] * inv[..., None]


def prepare_guide(guide, light, demodulate=True):
    """k_dn_prepare<DnGuide>: the records of ref_denoise.prepare from the guide images (H, W, 4)"""
    H, W = light.shape[:2]
    fg, l2 = foreground(guide)
    with np.errstate(all="ignore"):
        n = unit_normal(guide, l2)
        if demodulate:
            alb = guide["albedo"][..., :3]
            m = np.where(alb > rd.ALBEDO_FLOOR, alb, rd.ALBEDO_FLOOR)
            e = guide["emission"][..., :3].copy()
        else:
            m = np.ones((H, W, 3), F)
            e = np.zeros((H, W, 3), F)
        c = (light[..., :3] - e) / m
    z = np.zeros((H, W, 3), F)
    f3 = fg[..., None]
    return dict(P=np.where(f3, guide["position"][..., :3], z), n=np.where(f3, n, z).astype(F), c=np.where(f3, c, z).astype(F), m=m, e=e, fg=fg)


def denoise(guide, light, moments=None, stages=None, **params):
    """Out (H, W, 4) float32 of "denoise" with the guide input set to `guide` ({position, normal, albedo, emission} -> (H, W, 4)) and,
    with `moments`, the variance input; `params` as ref_denoise.denoise's"""
    guide = {k: np.ascontiguousarray(guide[k], F) for k in KEYS}
    return rd.denoise_records(lambda light, demodulate: prepare_guide(guide, light, demodulate), light, moments, stages=stages, **params)


TAP_ROUNDINGS = 52  # a 5 x 5 weighted mean: 25 products and 24 sums above, 24 sums below, one division -- 74 operations, but a sum's error
#                     falls on the partial sum only: Higham's bound for the quotient of two 25-term sums is gamma_26 + gamma_25 + u <= 52 u


def constant_signal_bound(light, m, k, iterations, fg):
    """|Out - In| allowed per pixel and channel (H, W, 3), float64, for In = fl(e + fl(k m)) on foreground pixels.  First order in u = 2^-24:
      In = (e + k m (1 + d1)) (1 + d2), so x = In - e = k m (1 + d1) + d2 In;
      demodulate, two roundings: c = fl(fl(In - e) / m) = (x / m) (1 + d3) (1 + d4), so |c - k| <= 3 u |k| + u R, R = max |In| / m over
      the foreground (the subtraction cancels: the rounding of In counts by |In| / m, not by |k|);
      each iteration replaces c by a mean of such values with weights >= 0, computed with TAP_ROUNDINGS roundings: |c' - k| grows by
      TAP_ROUNDINGS u |k| per iteration (with iterations = 0 the pass copies In, and the bound is not used);
      modulate, two roundings, one of which stands against In's own: |Out - (e + c' m)| <= u |c' m| + u |Out|, |In - (e + k m)| <= u |k m| + u |In|.
    Sum: m (3 u |k| + u R + iterations TAP_ROUNDINGS u |k|) + 2 u |k| m + 2 u |In|, times 1.01 for the terms of second order."""
    a = np.abs(light[..., :3].astype(np.float64))
    m = m.astype(np.float64)
    R = float((a / m)[fg].max()) if fg.any() else 0.0
    E = 3 * U * abs(k) + U * R + iterations * TAP_ROUNDINGS * U * abs(k)
    return 1.01 * (m * E + 2 * U * abs(k) * m + 2 * U * a)
