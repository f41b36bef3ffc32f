"""Fog on the GPU (rt3_scene_set_medium): the rule against float64, k_fog_segment and k_fog_shadow on caller-made
queues, the closed forms of tests/fog_worlds.py, "nothing changes without it", invariance under batch size, instance mode and tile
partition, the adaptive pass in coverage mode, and the refusals.

Bounds are derived (ref_fog.rule_bounds and the docstrings here), in units of U = 2^-24; means of samples are held within 6 standard errors
of the float64 reference estimator's own sample variance (tests/test_fog_cpu.py holds that estimator to the same tolerance)."""
import math

import numpy as np
import pytest

import adaptive_lens_worlds as alw
import emitter_tex_worlds as EW
import fog_worlds as FW
import glass_worlds as GW
import integrator_worlds as IW
import lens_worlds as LW
import pane_worlds as PN
import ref_fog as RF
import ref_roulette as RR
import volume_worlds as VW
from raytracer3_amd import _lib as L
from raytracer3_amd.renderer import scene_medium
from support import bits, camera
from test_adaptive_lens import LensWorld, check_against_fixed, everything
from test_fog_cpu import CASES, N_REF, op45_rows, reference
from test_glass import frame, sky_bound
from test_integrator_cpu import check_against_fixture
from test_nee_emissive import make_pt, owned_mask
from test_pane_shadows import P, crossing_bound, free_frame, pane_pt, relative_bound

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0**-24
MISS = 0xFFFFFFFF
FOG_BASE = 0x70000000
SKY = np.array(FW.SKY)
FULL = L.F_NEE_SKY | L.F_BLUENOISE | L.F_FACEFORWARD | L.F_SPECULAR


def fog_pt(mesh=None, sky=FW.SKY, lights=None, window=FW.WINDOW, **kw):
    """a PathTracer over a fog world (nothing in view unless a mesh is given) under a constant sky or none, the pinhole lens set"""
    pt = make_pt(mesh if mesh is not None else FW.hidden_world(), window, sky=None if sky is None else LW.constant_sky(sky), **kw)
    pt.set_lens(*FW.PINHOLE)
    if lights is not None:
        pt.set_lights(lights)
    return pt


def shot(pt, flags, spp, bounces, index=0, window=FW.WINDOW, cam=FW.CAMERA):
    return frame(pt, flags, spp, bounces, window=window, cam=cam, index=index)


def f64(words):
    return np.ascontiguousarray(words).view(F).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- 1 the rule
def test_rule_against_float64():
    """self-test op 45 on test_fog_cpu.op45_rows: the empty / non-empty decision, t0 and t1 equal the float32 restatement bit for bit; s,
    the density and the transmittance lie within ref_fog.rule_bounds of float64 from the same inputs, row by row"""
    rows = op45_rows()
    pt = fog_pt()
    try:
        hit, out = pt.ctx.selftest_fog(rows)
    finally:
        pt.close()
    ref = RF.rule_rows(rows)
    bound = RF.rule_bounds(ref)
    want = ref["hit"]
    assert np.array_equal(hit, want) and not out[~want].any()
    assert np.array_equal(bits(out[want, 0]), bits(ref["t0"][want].astype(F))) and np.array_equal(bits(out[want, 1]), bits(ref["t1"][want].astype(F)))
    got = out.astype(np.float64)
    # rows where the device's a = sb len and the reference's may fall on different sides of the uniform threshold are left out: none expected
    near = np.abs(ref["ab"] - RF.UNIFORM_BELOW) <= 16 * U * RF.UNIFORM_BELOW
    sel = want & ~near
    assert near.sum() < 5
    # (a result below 2^-126 is rounded on the denormal grid: one spacing, 2^-149, absolute, beside the relative bound)
    r_tr = np.abs(got[:, 4:7] - ref["Tr"])[sel] / (bound["Tr"][sel] * ref["Tr"][sel] + 2.0**-149)
    r_s = np.abs(got[:, 2] - ref["s"])[sel] / np.maximum(bound["s"][sel], 1e-300)
    finite = np.isfinite(bound["pdf"][sel]) & (ref["pdf"][sel] > 1e-30)
    r_p = (np.abs(got[:, 3][sel] / np.where(finite, ref["pdf"][sel], 1.0) - 1.0) / np.where(finite, bound["pdf"][sel], 1.0))[finite]
    print(f"op 45: {int(sel.sum())} rows in the medium; worst error / bound: Tr {r_tr.max():.3f}, s {r_s.max():.3f}, pdf {r_p.max():.3f} ({int(finite.sum())} rows)")
    assert r_tr.max() <= 1.0 and r_s.max() <= 1.0 and r_p.max() <= 1.0 and finite.sum() > 0.9 * sel.sum()
    s_par = (got[:, 2] - ref["t0"])[sel] * ref["dl"][sel]
    assert np.all(s_par >= -bound["s"][sel] * ref["dl"][sel]) and np.all(s_par <= ref["length"][sel] * (1 + 16 * U) + bound["s"][sel] * ref["dl"][sel])


# ---------------------------------------------------------------------------------------------------------------- 2 the kernels on queues
QUEUE_BOX = ((-1.0, 0.0, -1.5), (1.5, 2.0, 1.0))
QUEUE_G = 0.4
QUEUE_SIGMA_A, QUEUE_SIGMA_S = (0.2, 0.05, 0.1), (0.5, 0.7, 0.3)
QUEUE_PIXELS = np.array([3 | 5 << 16, 17 | 2 << 16, 40 | 30 << 16, 0, 47 | 11 << 16, 9 | 9 << 16, 21 | 29 << 16], np.uint32)
QUEUE_FRAME, QUEUE_B, QUEUE_SEG, QUEUE_S0 = 5, 4, 2, 3


@pytest.fixture(scope="module")
def queue_pt():
    pt = fog_pt(lights=FW.sun())
    m, med = FW.medium(QUEUE_SIGMA_A, QUEUE_SIGMA_S, QUEUE_G, QUEUE_BOX)
    pt.set_medium(m)
    yield pt, med
    pt.close()


def segment_records(n, seed, box=None):
    """n records {o, d, t, prim, T, path id}: origins around and inside QUEUE_BOX, directions towards it or past it, |d| from 0.7 to 1.4, a
    third missed (t = +inf by the kernel's rule), a twentieth with throughput 0, path ids a permutation"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray((box or QUEUE_BOX)[0]), np.asarray((box or QUEUE_BOX)[1])
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    o = c + e * rng.uniform(-2.5, 2.5, (n, 3))
    d = c + e * rng.uniform(-1.3, 1.3, (n, 3)) - o
    d *= (rng.uniform(0.7, 1.4, n) / np.linalg.norm(d, axis=1))[:, None]
    t = rng.uniform(0.2, 6.0, n)
    miss = rng.random(n) < 0.33
    T = rng.uniform(0.1, 1.2, (n, 3))
    T[rng.random(n) < 0.05] = 0.0
    rec = np.zeros((n, 12), np.uint32)
    rec[:, 0:3], rec[:, 3:6], rec[:, 6], rec[:, 8:11] = bits(o.astype(F)), bits(d.astype(F)), bits(t.astype(F)), bits(T.astype(F))
    rec[:, 7] = np.where(miss, MISS, 0)
    rec[:, 11] = rng.permutation(n)
    return rec


def fog_u(pid, dim):
    """the fog draw `dim` of path `pid` of the queue tests"""
    xy = QUEUE_PIXELS[pid % len(QUEUE_PIXELS)]
    sample = QUEUE_S0 + pid // len(QUEUE_PIXELS)
    idx = FOG_BASE + (sample * QUEUE_B + QUEUE_SEG) * 8 + dim
    return RR.uniform_float(RR.rng_seed(xy & 0xFFFF, xy >> 16, QUEUE_FRAME), idx.astype(np.uint64)).astype(np.float64)


def exit_amplification(x, w, lo, hi):
    """how much the length of x + r w inside the box can change per unit of |dx|_inf: 1 / |w_k| of the exit face's axis (of every axis
    whose face lies within a thousandth of the exit)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        far = np.where(w > 0, (hi - x) / w, np.where(w < 0, (lo - x) / w, np.inf))
    tmin = far.min(1, keepdims=True)
    close = far <= tmin * (1 + 1e-3) + 1e-6
    return np.max(np.where(close, 1.0 / np.maximum(np.abs(w), 1e-30), 0.0), 1)


def check_segment_queue(pt, med, n, groups, seed, miss_radiance=False):
    """k_fog_segment through self-test op 46 against the float64 rule.

    Throughput: (4 + 7 a) U relative, the rule's transmittance (ref_fog.rule_bounds) and one product.  Counts: exact.  Queued rays, keyed by
    (queue, path id): the origin x = o + s d within |d| ds + 4 U (|o| + |s d|) per coordinate; the direction of the table's ray is the sun's,
    of the sky's ray the one self-test op 25 gives for the same two draws, bit for bit; the contribution within the sum of the density's
    bound, (3 + 7 sigma_t ds) U for the point's transmittance, (3 + 7 a_shadow) U for the shadow ray's, sigma_t dlen for the shadow length
    (dlen = |dx| times exit_amplification, plus 4 U len), and 40 U for the phase function (14 U) and the products, quotients and the
    light's own terms."""
    st, ss, g, lo, hi = med
    rec = segment_records(n, seed)
    flags = L.F_NEE_SKY | L.F_NEE_PUNCTUAL
    got = pt.ctx.selftest_fog_segment(rec, QUEUE_PIXELS, groups, flags, QUEUE_FRAME, QUEUE_B, QUEUE_SEG, QUEUE_S0, miss_radiance)
    o, d, T = f64(rec[:, 0:3]), f64(rec[:, 3:6]), f64(rec[:, 8:11])
    miss = rec[:, 7] == MISS
    t = np.where(miss, np.inf, f64(rec[:, 6]))
    pid = rec[:, 11].astype(np.int64)
    hit, t0, t1 = RF.span32(o.astype(F), d.astype(F), t.astype(F), lo.astype(F), hi.astype(F))
    t0, t1 = t0.astype(np.float64), t1.astype(np.float64)
    dl = np.linalg.norm(d, axis=1)
    length = np.where(hit, (t1 - t0) * dl, 0.0)
    # throughput
    a = st[None, :] * length[:, None]
    assert np.array_equal(got["T"][~hit], rec[~hit, 8:11]), "a record outside the medium keeps its bits"
    live = hit & (T.max(1) > 0)
    relT = np.abs(f64(got["T"])[live] / (T[live] * np.exp(-a[live])) - 1.0)
    assert np.all(relT <= (4.0 + 7.0 * a[live]) * U), float((relT / ((4.0 + 7.0 * a[live]) * U)).max())
    assert not f64(got["T"])[hit & ~live].any()
    # the radiance slots: only those of missed records in the medium, and only on request
    rad = f64(got["radiance"])
    changed = np.zeros(n, bool)
    if miss_radiance:
        changed[pid[hit & miss]] = True
        relR = np.abs(rad[pid[hit & miss], :3] / np.exp(-a[hit & miss]) - 1.0)
        assert np.all(relR <= (4.0 + 7.0 * a[hit & miss]) * U)
    assert np.all(rad[~changed] == np.array([1.0, 1.0, 1.0, 0.0]))
    # the point
    sb = st.sum() / 3.0
    u0 = fog_u(pid, 0)
    ds, pdf = RF.sample_distance(sb, np.where(live, length, 1.0), u0)
    ref = dict(L=sb * ds, ab=sb * np.where(live, length, 1.0), sb=np.full(n, sb), dl=dl, ds=ds, t0=t0, a=a)
    bnd = RF.rule_bounds(ref)
    s = t0 + ds / dl
    x = o + s[:, None] * d
    dx = dl * bnd["s"] + 4.0 * U * (np.abs(o).max(1) + np.abs(s) * np.abs(d).max(1))
    w = T * np.exp(-st[None, :] * ds[:, None]) * ss[None, :] / pdf[:, None]
    w_rel = bnd["pdf"] + (3.0 + 7.0 * st.max() * ds) * U
    # the two light samples
    sun_w = np.array([0.0, 1.0, 0.0])
    sky_rows = np.stack([fog_u(pid, 3), fog_u(pid, 4)], 1).astype(F)
    sky = pt.ctx.selftest(25, sky_rows, 9)
    sky_dir, sky_rad, sky_pdf = f64(sky[:, 0:3]), f64(sky[:, 3:6]), f64(sky[:, 6])
    expect = [live & (sky_pdf > 0), live]
    with np.errstate(divide="ignore", invalid="ignore"):
        le = [sky_rad / sky_pdf[:, None], np.broadcast_to(np.asarray(FW.SUN_E, np.float64), (n, 3))]
    wl = [sky_dir, np.broadcast_to(sun_w, (n, 3))]
    assert got["segments"] == int(hit.sum())
    total = 0
    for q in range(2):
        count = int(got["counts"][q])
        assert count == int(expect[q].sum()), (q, count, int(expect[q].sum()))
        total += count
        rays = got["queues"][q][:count]
        qpid = rays[:, 9].astype(np.int64)
        assert len(set(qpid.tolist())) == count and set(qpid.tolist()) == set(pid[expect[q]].tolist()), "one ray per path, the expected paths"
        row = np.empty(n, np.int64)
        row[pid] = np.arange(n)
        k = row[qpid]
        gx, gw, gc = f64(rays[:, 0:3]), f64(rays[:, 4:7]), np.stack([f64(rays[:, 3]), f64(rays[:, 7]), f64(rays[:, 8])], 1)
        assert np.all(np.abs(gx - x[k]) <= dx[k, None]), float((np.abs(gx - x[k]) / dx[k, None]).max())
        if q == 0:
            assert np.array_equal(rays[:, 4:7], sky[k, 0:3])
        else:
            assert np.all(gw == sun_w)
        assert np.all(f64(rays[:, 10]) == 100000.0)
        ls = RF.shadow_length(x[k], wl[q][k], np.inf, lo, hi)
        ph = RF.phase(g, np.sum(d[k] * wl[q][k], 1) / dl[k])
        want = w[k] * le[q][k] * ph[:, None] * np.exp(-st[None, :] * ls[:, None])
        dlen = dx[k] * exit_amplification(x[k], wl[q][k], lo, hi) + 4.0 * U * ls
        rel_b = w_rel[k] + (3.0 + 7.0 * st.max() * ls) * U + st.max() * dlen + 40.0 * U
        rel = np.abs(gc / want - 1.0)
        ratio = (rel / rel_b[:, None]).max() if count else 0.0
        print(f"op 46 n={n} groups={groups} queue {q}: {count} rays, worst contribution error / bound {ratio:.3f}")
        assert np.all(rel <= rel_b[:, None]), float(ratio)
    assert got["rays"] == total
    return int(hit.sum()), [int(got["counts"][0]), int(got["counts"][1])]


@pytest.mark.parametrize("n,groups", [(0, 1), (1, 1), (63, 1), (64, 2), (65, 1), (257, 2), (1500, 1), (1500, 3)])
def test_segment_kernel_on_a_queue(queue_pt, n, groups):
    """k_fog_segment (256 threads a workgroup): less than a wave, a wave and one lane more, a workgroup and one lane more, and 1500
    records over one workgroup (six passes of the grid-stride loop, the last partial) and over three (appends from several workgroups)"""
    pt, med = queue_pt
    check_segment_queue(pt, med, n, groups, seed=7 * n + groups)


def test_segment_queue_covers_every_kind_of_record_and_the_missed_radiance(queue_pt):
    pt, med = queue_pt
    segs, counts = check_segment_queue(pt, med, 1500, 2, seed=3, miss_radiance=True)
    assert 300 < segs < 1400 and min(counts) > 200 and counts[1] >= counts[0]


def test_medium_info_counts_a_frame(queue_pt):
    """rt3_medium_info after a frame: every camera ray of the slab world runs through the medium (W H S segments at one bounce), each with a
    sky ray and a sun ray"""
    pt, _ = queue_pt
    keep = pt.ctx.get_medium()[0]
    try:
        pt.set_medium(FW.medium()[0])
        shot(pt, L.F_NEE_SKY | L.F_NEE_PUNCTUAL, 2, 2)
        W, H = FW.WINDOW
        assert pt.medium_info() == (2 * W * H, 4 * W * H)
        pt.set_medium(None)
        shot(pt, L.F_NEE_SKY, 1, 2)
        assert pt.medium_info() == (0, 0)
    finally:
        pt.set_medium(keep)
        pt.set_lens(*FW.PINHOLE)


def shadow_records(n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(QUEUE_BOX[0]), np.asarray(QUEUE_BOX[1])
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    o = c + e * rng.uniform(-2.0, 2.0, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rec = np.zeros((n, 11), np.uint32)
    contrib = rng.uniform(0.01, 3.0, (n, 3)).astype(F)
    rec[:, 0:3], rec[:, 4:7] = bits(o.astype(F)), bits(d.astype(F))
    rec[:, 3], rec[:, 7], rec[:, 8] = bits(contrib[:, 0]), bits(contrib[:, 1]), bits(contrib[:, 2])
    rec[:, 9] = rng.permutation(n)
    rec[:, 10] = bits(rng.uniform(0.1, 4.0, n).astype(F))
    return rec, contrib


@pytest.mark.parametrize("with_tmax", (False, True))
@pytest.mark.parametrize("n,groups", [(0, 1), (1, 1), (63, 1), (64, 1), (65, 2), (257, 1), (1500, 2)])
def test_shadow_kernel_on_a_queue(queue_pt, n, groups, with_tmax):
    """k_fog_shadow through self-test op 46: every contribution within (4 + 7 a) U of float64 (the transmittance's bound and one product),
    a ray that does not meet the box keeps its bits; the queue with range ends stops at them, the one without runs to the box's exit"""
    pt, (st, ss, g, lo, hi) = queue_pt
    rec, contrib = shadow_records(n, 13 * n + groups)
    got = pt.ctx.selftest_fog_shadow(rec, groups, with_tmax)
    o, d = f64(rec[:, 0:3]), f64(rec[:, 4:7])
    tmax = f64(rec[:, 10]) if with_tmax else np.full(n, 100000.0)
    hit, t0, t1 = RF.span32(o.astype(F), d.astype(F), tmax.astype(F), lo.astype(F), hi.astype(F))
    length = np.where(hit, (t1.astype(np.float64) - t0) * np.linalg.norm(d, axis=1), 0.0)
    assert np.array_equal(got[~hit], bits(contrib)[~hit])
    a = st[None, :] * length[:, None]
    rel = np.abs(f64(got)[hit] / (contrib[hit].astype(np.float64) * np.exp(-a[hit])) - 1.0)
    assert np.all(rel <= (4.0 + 7.0 * a[hit]) * U)
    if n >= 257:
        assert hit.sum() > n // 5 and (~hit).sum() > n // 5


# ---------------------------------------------------------------------------------------------------------------- 3 closed forms
@pytest.mark.parametrize("nee", (True, False), ids=["sky_nee", "no_sky_nee"])
def test_absorbing_slab_dims_the_sky(nee):
    """sigma_s = 0, a constant sky, nothing in view, 1 spp: every pixel is SKY exp(-sigma_t chord), chord = 2 / |d.z| of its ray through the
    slab.  With sky NEE the escaped camera sample takes the sky in the first k_shade's miss branch, with the throughput k_fog_segment left;
    without it k_lens_miss has written the sky and k_fog_segment attenuates that radiance slot.
    Band, relative: sky_bound(S); the transmittance (3 + 7 a) U; the chord t1 - t0 of two quotients of magnitude 2 / |d.z| and 4 / |d.z|,
    each one rounding, and the difference: 4 U of the chord, 4 a U; the camera's fp32 direction, each component within 2 U, turns the ray
    by at most 4 U and changes 1 / cos by tan theta < 1 times that: 4 a U; two products.  sky_bound(S) + (6 + 16 a) U."""
    sigma = (0.3, 0.05, 0.6)
    m, (st, _, _, lo, hi) = FW.medium(sigma, 0.0)
    a = st[None, None, :] * FW.chords()[..., None]
    want = SKY * np.exp(-a)
    pt = fog_pt()
    try:
        pt.set_medium(m)
        got = shot(pt, L.F_NEE_SKY if nee else 0, 1, 1).astype(np.float64)
        assert pt.medium_info() == (FW.WINDOW[0] * FW.WINDOW[1], 0)
    finally:
        pt.close()
    band = sky_bound(1) + (6.0 + 16.0 * a) * U
    rel = np.abs(got / want - 1.0)
    print(f"absorbing slab nee={nee}: worst deviation {np.max(rel / band):.3f} bands; a up to {a.max():.2f}")
    assert a.max() > 1.0 and np.all(rel <= band)


@pytest.mark.parametrize("g", (0.0, 0.6))
def test_shaft_under_the_sun_is_constant_on_horizontal_rays(g):
    """A grey slab of medium, a black sky (none), the sun straight down, 1 spp.  On the horizontal rays of the centre row every point lies
    h = 1 below the slab's top and sees the sun at right angles, so with the exponential density the estimator is the constant
    sigma_s p_HG(0) E e^(-sigma_t h) (1 - e^(-sigma_t l)) / sigma_t whatever point is drawn.
    Band, relative, a = sigma_t l: the two exponentials of the weight share the device's ds and cancel analytically; each carries its
    product's rounding (U L absolute on the exponent, L <= a) and expf's 2 U, and sb = (3 sigma) / 3 differs from sigma_t by 2 U (2 U L on the
    exponent): 4 a U + 4 U; E 11 U, sb 3 U, the weight's three products and the quotient 4 U; the phase function 14 U; the sun's record and
    p_sel = 1 2 U; the shadow ray's transmittance (3 + 7 sigma_t h) U, with h known to 2 U (the point's y is o.y + s d.y, d.y < 2^-22 in fp32:
    sigma_t l 2^-22 more); three more products and the mean of one sample 5 U: (46 + 8 a + 7 sigma_t h) U, rounded up to (60 + 8 a + 7
    sigma_t h) U."""
    m, (st, *_rest) = FW.medium(g=g)
    want, l, h = FW.shaft_centre_row(g)
    pt = fog_pt(sky=None, lights=FW.sun())
    try:
        pt.set_medium(m)
        got = shot(pt, L.F_NEE_PUNCTUAL, 1, 2).astype(np.float64)
        again = shot(pt, L.F_NEE_PUNCTUAL, 1, 2, index=9).astype(np.float64)
    finally:
        pt.close()
    a = st[None, :] * l[:, None]
    band = (60.0 + 8.0 * a + 7.0 * st * h) * U + st * l[:, None] * 2.0**-22
    rel = np.abs(got[FW.CENTRE_ROW] / want - 1.0)
    print(f"shaft g={g}: worst deviation {np.max(rel / band):.3f} bands on the centre row ({rel.max() / U:.1f} U)")
    assert np.all(rel <= band) and np.all(np.abs(again[FW.CENTRE_ROW] / want - 1.0) <= band)
    assert g == 0.0 or not np.array_equal(got[0], again[0]), "off the centre row the estimator is not constant"


def check_mean_against_quadrature(got, kind):
    """6 standard errors of the float64 estimator's own mean (test_fog_cpu.reference), the quadrature's own error (6 / N^2 of q, and at
    the occluder's edge one cell of the rule: reference's docstring), and 64 U of q for the device's rounding (the shaft's band at its
    widest)"""
    q, _, se, edge = reference(kind)
    H, W = FW.WINDOW[1], FW.WINDOW[0]
    tol = 6.0 * se + edge + 64 * U * q
    err = np.abs(got.reshape(-1, 3) - q)
    worst = float((err / np.maximum(tol, 1e-300))[tol > 0].max())
    print(f"{kind}: worst deviation {worst:.3f} of the tolerance over {H * W} pixels; median relative standard error {np.median((se / np.maximum(q, 1e-30))[q > 0]):.3f}")
    assert np.all(err <= tol)
    return q


def n_ref_frame(kind, mesh=None, lights=None, flags=L.F_NEE_PUNCTUAL):
    cam, g, _, _ = CASES[kind]
    pt = fog_pt(mesh, sky=None, lights=lights)
    try:
        pt.set_medium(FW.medium(g=g)[0])
        return shot(pt, flags, N_REF, 2, cam=cam).astype(np.float64)
    finally:
        pt.close()


def test_shaft_off_the_horizontal_meets_the_quadrature():
    """the same frame at N_REF spp, g = 0.6, every row: the rays that climb or sink see the sun through a varying depth of medium and at a
    varying angle, and leave through the slab's top or bottom"""
    q = check_mean_against_quadrature(n_ref_frame("sun", lights=FW.sun()), "sun")
    assert q.reshape(FW.WINDOW[1], FW.WINDOW[0], 3)[0].mean() != q.reshape(FW.WINDOW[1], FW.WINDOW[0], 3)[FW.CENTRE_ROW].mean()


def test_lamp_above_the_slab_meets_the_quadrature():
    """a point light above the slab, seen by a camera tilted down into it (four rays in ten leave through the slab's bottom): inverse-square
    falloff, a slanted shadow ray that ends at the lamp; the mean of N_REF samples against the float64 quadrature of the integral"""
    check_mean_against_quadrature(n_ref_frame("lamp", lights=FW.lamp()), "lamp")


def test_emissive_panel_above_the_slab_meets_the_quadrature():
    """an emissive quad above the slab, out of view, sampled through the light table under RT3_F_NEE_EMISSIVE: the pick among its two
    triangles, the point, the two-sided cosine and p_sel / area dist^2 / |cos_l| against the float64 integral over the quad and the ray
    (ref_fog.Panel), g = 0.3, the tilted view"""
    check_mean_against_quadrature(n_ref_frame("panel", FW.panel_world(), flags=L.F_NEE_EMISSIVE), "panel")


def test_shadow_volume_under_an_occluder():
    """an occluder above the slab keeps the sun from x < EDGE_X: the in-scatter rays are traced.  Every pixel against the quadrature with
    the occluder's visibility; the centre row against the closed form whose limits the edge moves; the rays wholly in shadow are black"""
    got = n_ref_frame("occluder", FW.hidden_world(occluder=True), lights=FW.sun())
    q = check_mean_against_quadrature(got, "occluder")
    want, share = FW.shadowed_centre_row()
    row = got[FW.CENTRE_ROW]
    assert not row[share == 0].any() and (share == 0).sum() >= 4
    _, _, se, _ = reference("occluder")
    se = se.reshape(FW.WINDOW[1], FW.WINDOW[0], 3)[FW.CENTRE_ROW]
    assert np.all(np.abs(row - want) <= 6.0 * se + 64 * U * want), "against the closed form there is no quadrature error to allow for"
    unshadowed = FW.shaft_centre_row(0.0)[0]
    assert np.all(row[share < 0.5] < 0.75 * unshadowed[share < 0.5])


# ---------------------------------------------------------------------------------------------------------------- 4 bits that must not move
WORLDS = {
    "plain": lambda: (IW.open_room(), IW.ROOM_CAMERA, IW.WINDOW_ROOM, IW.room_sky()),
    "glass": lambda: (GW.glass_room(True, 0.5), IW.ROOM_CAMERA, IW.WINDOW_ROOM, IW.room_sky()),
    "emitter_nee": lambda: (GW.sealed_world(emissive=True)[0], GW.SEALED_CAMERA, GW.WINDOW, LW.constant_sky(GW.SKY_L)),
}


@pytest.mark.parametrize("world", sorted(WORLDS))
def test_nothing_changes_without_a_medium(world):
    """medium NULL, or every sigma 0: the frame without the call, bit for bit, and nothing is counted; a medium shows; NULL again restores"""
    mesh, cam, window, sky = WORLDS[world]()
    pt = make_pt(mesh, window, sky=sky)
    try:
        pt.set_lens(0.0, 1.0, 1.0)
        go = lambda: frame(pt, FULL | L.F_NEE_EMISSIVE, 2, 5, window=window, cam=cam)
        plain = go()
        assert plain.max() > 0.0 and pt.medium_info() == (0, 0)
        pt.set_medium(scene_medium(mesh, 0.0, 0.0, 0.3))
        assert pt.ctx.get_medium()[1] is False
        assert np.array_equal(bits(go()), bits(plain)) and pt.medium_info() == (0, 0)
        pt.set_medium(scene_medium(mesh, 0.2, 0.1, 0.3, margin=0.5))
        assert pt.ctx.get_medium()[1] is True
        fogged = go()
        assert not np.array_equal(bits(fogged), bits(plain)) and np.isfinite(fogged).all() and pt.medium_info()[0] > 0
        pt.set_medium(None)
        assert np.array_equal(bits(go()), bits(plain))
        assert pt.ctx.get_lens()[1], "the caller's lens stays"
    finally:
        pt.close()


def fogged_room(window=IW.WINDOW_ROOM, spp=2, setup=None, **kw):
    mesh = GW.glass_room(True, 0.5)
    pt = make_pt(mesh, window, sky=IW.room_sky(), **kw)
    try:
        pt.set_lens(0.05, 6.0, 1.0)
        pt.set_medium(scene_medium(mesh, (0.2, 0.15, 0.1), 0.05, 0.5, margin=0.25))
        if setup:
            setup(pt)
        return frame(pt, FULL | L.F_NEE_EMISSIVE, spp, 5, window=window, cam=IW.ROOM_CAMERA)
    finally:
        pt.close()


def test_same_bits_for_every_batch_size_and_instance_mode():
    whole = fogged_room()
    assert whole.max() > 0.0
    assert np.array_equal(bits(whole), bits(fogged_room(setup=lambda pt: pt.ctx.set_option(L.OPT_BATCH_SPP, 1))))
    assert np.array_equal(bits(whole), bits(fogged_room(mode=1)))


def test_two_ranks_stitch_to_one():
    W, H = window = (128, 32)
    whole = fogged_room(window)
    for r in range(2):
        part = fogged_room(window, rank=r, n_ranks=2)
        m = owned_mask(W, H, r, 2)
        assert m.any() and not m.all()
        assert np.array_equal(bits(part[m]), bits(whole[m]))


def test_adaptive_pixels_hold_the_fixed_frames_bits():
    """coverage mode over a fogged room (world B of adaptive_lens_worlds): a pixel that stopped at n holds the bits of the fixed fog frame
    at samples = n, and the fog shows in them"""
    mesh = VW.absorbing_room()
    w = LensWorld(alw.B, mesh, IW.room_sky())
    try:
        w.pt.ctx.set_medium(scene_medium(mesh, 0.2, 0.05, 0.3, margin=0.25))
        light, moments, info, _ = w.adaptive()
        n = check_against_fixed(w, light, moments, everything(w))
        assert len(set(n.reshape(-1).tolist())) > 1 and w.pt.medium_info()[0] > 0
        fogged = w.fixed(alw.MIN_SAMPLES)
        w.pt.ctx.set_medium(None)
        w.cache.clear()
        assert not np.array_equal(bits(w.fixed(alw.MIN_SAMPLES)), bits(fogged))
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------------------------- 5 refusals
BAD = {
    "negative sigma_a": dict(sigma_a=(0.1, -0.5, 0.1)), "sigma_s NaN": dict(sigma_s=(np.nan, 0.1, 0.1)), "sigma_a inf": dict(sigma_a=(0.1, 0.1, np.inf)),
    "g = 1": dict(g=1.0), "g = -1": dict(g=-1.0), "g NaN": dict(g=np.nan), "g inf": dict(g=np.inf),
    "box NaN": dict(box_min=(np.nan, 0.0, 0.0)), "box inf": dict(box_max=(1.0, np.inf, 1.0)), "empty box": dict(box_min=(0.0, 2.0, 0.0), box_max=(1.0, 2.0, 1.0)),
    "inverted box": dict(box_min=(3.0, 0.0, 0.0), box_max=(1.0, 2.0, 1.0)),
}


def test_refusals_leave_the_state_as_it_was():
    m, _ = FW.medium(g=0.25)
    pt = fog_pt(lights=FW.sun())
    try:
        ctx = pt.ctx
        ctx.set_medium(m)
        flags = L.F_NEE_SKY | L.F_NEE_PUNCTUAL
        before = shot(pt, flags, 2, 3)
        state = lambda: bytes(ctx.get_medium()[0])
        kept = state()
        for what, change in BAD.items():
            kw = dict(sigma_a=FW.SIGMA_A, sigma_s=FW.SIGMA_S, g=0.25, box_min=FW.SLAB[0], box_max=FW.SLAB[1])
            kw.update(change)
            with pytest.raises(L.Rt3Error) as e:
                ctx.set_medium(L.Medium(**kw))
            assert e.value.code == L.E_INVALID, what
            assert state() == kept and ctx.get_medium()[1], what
        assert np.array_equal(bits(shot(pt, flags, 2, 3)), bits(before))
        # the RNG range: samples * bounces * 8 may not pass 2^28
        with pytest.raises(L.Rt3Error) as e:
            shot(pt, flags, (1 << 23) + 1, 4)
        assert e.value.code == L.E_INVALID
        info = pt.medium_info()
        # no lens
        pt.set_lens(None)
        with pytest.raises(L.Rt3Error) as e:
            shot(pt, flags, 2, 3)
        assert e.value.code == L.E_STATE
        with pytest.raises(L.Rt3Error) as e:
            pt.render(pt.make_gconst(camera(FW.CAMERA, FW.WINDOW), 8, 3, flags=flags), adaptive=True)
        assert e.value.code == L.E_STATE
        # adaptive outside coverage mode, with the lens back
        pt.set_lens(*FW.PINHOLE)
        pt.set_adaptive_coverage(False)
        with pytest.raises(L.Rt3Error) as e:
            pt.render(pt.make_gconst(camera(FW.CAMERA, FW.WINDOW), 8, 3, flags=flags), adaptive=True)
        assert e.value.code == L.E_STATE
        assert state() == kept and pt.medium_info() == info
        assert np.array_equal(bits(shot(pt, flags, 2, 3)), bits(before))
    finally:
        pt.close()


def test_set_medium_switches_the_pinhole_on_and_off():
    pt = make_pt(FW.hidden_world(), FW.WINDOW, sky=LW.constant_sky(FW.SKY))
    try:
        assert not pt.ctx.get_lens()[1]
        pt.set_medium(FW.medium()[0])
        p, on = pt.ctx.get_lens()
        assert on and (p.aperture_radius, p.pixel_jitter) == (0.0, 0.0)
        assert shot(pt, L.F_NEE_SKY, 1, 2).max() > 0.0
        pt.set_medium(None)
        assert not pt.ctx.get_lens()[1]
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 6 emitters, textures, panes
def test_shaft_through_a_pane_under_pane_shadows():
    """the shaft world with a thin-walled pane over the slab and pane shadows on: every in-scatter ray meets the pane squarely on its way to
    the sun, so the centre row is the shaft's closed form times tau (1 - F'(1)) tint -- the in-scatter queues are walked by k_shadow_pane.
    Band: the shaft's, plus test_pane_shadows.crossing_bound for one crossing.  With the mode off the pane is a wall and the row is black."""
    m, (st, *_rest) = FW.medium()
    want, l, h = FW.shaft_centre_row(0.0)
    A = FW.CANOPY_TAU * PN.pass_fraction(1.0, FW.CANOPY_IOR) * np.asarray(FW.CANOPY_TINT)
    rows = {}
    for on in (True, False):
        pt = pane_pt(FW.hidden_world(canopy=True), on, window=FW.WINDOW, lens=FW.PINHOLE)
        try:
            assert pt.ctx.pane_shadow_info() == (1 if on else 0)
            pt.set_lights(FW.sun())
            pt.set_medium(m)
            rows[on] = shot(pt, L.F_NEE_PUNCTUAL, 1, 2).astype(np.float64)[FW.CENTRE_ROW]
        finally:
            pt.close()
    a = st[None, :] * l[:, None]
    band = (60.0 + 8.0 * a + 7.0 * st * h) * U + st * l[:, None] * 2.0**-22 + 1.01 * crossing_bound(1.0, FW.CANOPY_IOR)
    rel = np.abs(rows[True] / (want * A) - 1.0)
    print(f"shaft through a pane: worst deviation {np.max(rel / band):.3f} bands; A = {A}")
    assert np.all(rel <= band) and not rows[False].any()


@pytest.mark.parametrize("light", ("directional", "point"))
def test_lit_floor_under_a_pane_through_absorbing_fog(light):
    """pane_worlds' floor under a light and a pane, in a box of absorbing medium (sigma_s = 0) from the floor to y = 2, below the camera and
    the pane: the floor's light sample rides the emitter queue through k_fog_shadow (the point light's with its range end) and then through
    k_shadow_pane, the camera segment ends at a hit.  A pixel is the frame without glass and fog (test_pane_shadows.free_frame) times the
    pane's factor times exp(-sigma_t (c + s)), c = 2 |x - o| / o.y the camera ray's stretch below y = 2 and s = 2 / w_l.y the shadow ray's.
    Band, relative: test_pane_shadows.relative_bound for the pane; (3 + 7 a) U for each of the two transmittances; each stretch is a
    difference of two quotients of an fp32 ray (4 U of it, as for the slab before the sky) along a direction known to 4 U, which moves
    1 / cos by less than 2 x 4 U at these angles: 12 a U each; three products: (9 + 19 (a_c + a_s)) U."""
    sigma = np.array([0.3, 0.05, 0.6], np.float32)
    box = ((-10.0, 0.0, -10.0), (10.0, 2.0, 10.0))
    m, (st, *_rest) = FW.medium(tuple(sigma), 0.0, 0.0, box)
    x = PN.floor_points()
    o = np.asarray(PN.CAMERA["position"], np.float64)
    c = 2.0 * np.linalg.norm(x - o, axis=1) / o[1]
    w = PN.to_light(PN.LIGHTS[light], x)
    sh = 2.0 / w[:, 1]
    factor, use, crossed = PN.closed_form("pane", light)
    free = free_frame(light).reshape(-1, 3).astype(np.float64)
    pt = pane_pt(PN.world("pane", light))
    try:
        pt.set_medium(m)
        got = frame(pt, P, 1, 2, window=PN.WINDOW, cam=PN.CAMERA).reshape(-1, 3).astype(np.float64)
        segments, rays = pt.medium_info()
    finally:
        pt.close()
    W, H = PN.WINDOW
    assert rays == 0 and segments >= W * H
    ac, as_ = st[None, :] * c[:, None], st[None, :] * sh[:, None]
    want = free * factor * np.exp(-(ac + as_))
    bound = relative_bound("pane", light)[:, None] + (9.0 + 19.0 * (ac + as_)) * U
    lit = use & (want.min(1) > 0)
    rel = np.abs(got[lit] / want[lit] - 1.0)
    print(f"floor under a pane in fog, {light}: {int(lit.sum())} pixels, {int((lit & (crossed > 0)).sum())} behind the pane; worst deviation {np.max(rel / bound[lit]):.3f} bounds")
    assert (lit & (crossed > 0)).sum() > 300 and (lit & (crossed == 0)).sum() > 300 and (ac + as_).max() > 2.0
    assert np.all(rel <= bound[lit])


SOUP_BOX = ((-1.0, -1.0, -1.0), (13.0, 11.5, 1.5))


def test_segment_kernel_samples_emitters_and_their_textures():
    """k_fog_segment through self-test op 46 over emitter_tex_worlds.soup() (emitters with and without emissive textures, three instances)
    with textured emitters on: the light table's side of a ray against float64 from the table's own records (rt3_light_table).  Per
    record: k = floor(u5 2^23), the entry is the first with cdf > k; (b1, b2) = (u7 sqrt(u6), sqrt(u6) - b1) in fp32; the radiance Le (*)
    texel there by self-test op 42 (pinned to the hit side elsewhere); pe = A + b1 E1 + b2 E2, the direction, the two-sided cosine and
    p_sel / area dist^2 / |cos_l| in float64.  Counts exact; direction, range end and contribution within bounds that add, to
    check_segment_queue's, the point's uncertainty dx (the origin's, and 4 U of the record's coordinates) over the distance: 2 sqrt(3)
    dx / dist for each of 1 / dist^2 (twice), the cosine (over the cosine), the phase function (3 g / (1 - g)^2 < 4 times) and the shadow
    length (in units of sigma_t)."""
    mesh, instances = EW.soup()
    flags = L.F_NEE_EMISSIVE
    pt = make_pt(mesh, FW.WINDOW, instances=instances)
    try:
        pt.set_lens(*FW.PINHOLE)
        pt.set_textured_emitters(True)
        m, (st, ss, g, lo, hi) = FW.medium(QUEUE_SIGMA_A, QUEUE_SIGMA_S, QUEUE_G, SOUP_BOX)
        pt.set_medium(m)
        n = 1500
        rec = segment_records(n, 21, SOUP_BOX)
        got = pt.ctx.selftest_fog_segment(rec, QUEUE_PIXELS, 2, flags, QUEUE_FRAME, QUEUE_B, QUEUE_SEG, QUEUE_S0)
        table, cdf = pt.ctx.light_table(flags)[:2]
        _, tex = pt.ctx.light_emit_tex(flags)
        pid = rec[:, 11].astype(np.int64)
        k = np.floor(fog_u(pid, 5) * 2.0**23).astype(np.int64)
        e = np.searchsorted(cdf.astype(np.int64), k, side="right")
        su = np.sqrt(fog_u(pid, 6).astype(F))
        b1 = (fog_u(pid, 7).astype(F) * su).astype(F)
        b2 = (su - b1).astype(F)
        le_tex = pt.ctx.selftest_emit_radiance(flags, e, b1, b2).astype(np.float64)
    finally:
        pt.close()
    assert (tex[e] >= 0).sum() > 300 and (tex[e] < 0).sum() > 100 and len(set(e.tolist())) > 40
    o, d, T = f64(rec[:, 0:3]), f64(rec[:, 3:6]), f64(rec[:, 8:11])
    t = np.where(rec[:, 7] == MISS, np.inf, f64(rec[:, 6]))
    hit, t0, t1 = RF.span32(o.astype(F), d.astype(F), t.astype(F), lo.astype(F), hi.astype(F))
    t0, t1 = t0.astype(np.float64), t1.astype(np.float64)
    dl = np.linalg.norm(d, axis=1)
    live = hit & (T.max(1) > 0)
    length = np.where(live, (t1 - t0) * dl, 1.0)
    sb = st.sum() / 3.0
    ds, pdf = RF.sample_distance(sb, length, fog_u(pid, 0))
    bnd = RF.rule_bounds(dict(L=sb * ds, ab=sb * length, sb=np.full(n, sb), dl=dl, ds=ds, t0=t0, a=st[None, :] * length[:, None]))
    s = t0 + ds / dl
    x = o + s[:, None] * d
    r = table[e].astype(np.float64)
    A, pa, E1, E2, nrm = r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 8:11], r[:, 12:15]
    dx = dl * bnd["s"] + 4.0 * U * (np.abs(o).max(1) + np.abs(s) * np.abs(d).max(1)) + 4.0 * U * (np.abs(A).max(1) + np.abs(E1).max(1) + np.abs(E2).max(1))
    pe = A + b1.astype(np.float64)[:, None] * E1 + b2.astype(np.float64)[:, None] * E2
    wv = pe - x
    dist = np.linalg.norm(wv, axis=1)
    w1 = wv / dist[:, None]
    cle = np.abs(np.sum(nrm * w1, 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        le = le_tex / (pa * dist * dist / cle)[:, None]
    expect = live & (pa > 0) & (cle > 0) & (le.max(1) > 0)
    assert int(got["counts"][0]) == 0 and int(got["counts"][1]) == int(expect.sum()) and got["segments"] == int(hit.sum()) and got["rays"] == int(expect.sum())
    rays = got["queues"][1][: int(expect.sum())]
    qpid = rays[:, 9].astype(np.int64)
    assert set(qpid.tolist()) == set(pid[expect].tolist()) and len(set(qpid.tolist())) == len(qpid)
    row = np.empty(n, np.int64)
    row[pid] = np.arange(n)
    j = row[qpid]
    gx, gw, gc, gt = f64(rays[:, 0:3]), f64(rays[:, 4:7]), np.stack([f64(rays[:, 3]), f64(rays[:, 7]), f64(rays[:, 8])], 1), f64(rays[:, 10])
    turn = 2.0 * math.sqrt(3.0) * dx[j] / dist[j]
    assert np.all(np.abs(gx - x[j]) <= dx[j, None])
    assert np.all(np.abs(gw - w1[j]) <= (turn + 8.0 * U)[:, None])
    assert np.all(np.abs(gt - dist[j] * RF.EMIT_SHADOW_END) <= math.sqrt(3.0) * dx[j] + 8.0 * U * dist[j])
    ls = RF.shadow_length(x[j], w1[j], dist[j] * RF.EMIT_SHADOW_END, lo, hi)
    w = T[j] * np.exp(-st[None, :] * ds[j, None]) * ss[None, :] / pdf[j, None]
    want = w * le[j] * RF.phase(g, np.sum(d[j] * w1[j], 1) / dl[j])[:, None] * np.exp(-st[None, :] * ls[:, None])
    dlen = dx[j] * (exit_amplification(x[j], w1[j], lo, hi) + 2.0) + 8.0 * U * ls
    rel_b = (bnd["pdf"][j] + (3.0 + 7.0 * st.max() * ds[j]) * U + (3.0 + 7.0 * st.max() * ls) * U + st.max() * dlen + 48.0 * U
             + turn * (2.0 + 1.0 / cle[j] + 4.0))
    rel = np.abs(gc / np.where(want > 0, want, 1.0) - 1.0) * (want > 0)
    print(f"op 46 over the soup: {len(j)} emitter rays ({int((tex[e[j]] >= 0).sum())} textured), worst contribution error / bound {float((rel / rel_b[:, None]).max()):.3f}")
    assert np.all(rel <= rel_b[:, None]) and np.all((gc == 0) == (want == 0))


def test_set_scene_and_set_medium_share_the_pinhole():
    """the pinhole set_medium switches on passes to a scene with glass and ends with it; a medium that outlives a scene gets it back"""
    pt = make_pt(FW.hidden_world(), FW.WINDOW, sky=LW.constant_sky(FW.SKY))
    try:
        lens_on = lambda: pt.ctx.get_lens()[1]
        pt.set_medium(FW.medium()[0])
        assert lens_on()
        pt.set_scene(GW.pane_world(), LW.constant_sky(FW.SKY))
        pt.set_medium(None)
        assert lens_on(), "the glass needs it"
        pt.set_scene(FW.hidden_world(), LW.constant_sky(FW.SKY))
        assert not lens_on(), "nobody needs it"
        pt.set_medium(FW.medium()[0])
        pt.set_scene(GW.pane_world(), LW.constant_sky(FW.SKY))
        pt.set_scene(FW.hidden_world(), LW.constant_sky(FW.SKY))
        assert lens_on(), "the medium is still on"
        assert shot(pt, L.F_NEE_SKY, 1, 2).max() > 0.0
        pt.set_medium(None)
        assert not lens_on()
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 7 the fixture
def fogged_room_frames(name, mode=0):
    flags, bounces, _, _, frames = FW.ROOM_CASES[name]
    pt = pane_pt(FW.fog_room(), True, IW.WINDOW_ROOM, sky=IW.room_sky(), lens=PN.ROOM_LENS, mode=mode)
    try:
        assert pt.ctx.pane_shadow_info() == 1
        pt.set_textured_emitters(True)
        pt.set_medium(FW.room_medium()[0])
        cam = camera(PN.ROOM_CAMERA, IW.WINDOW_ROOM)
        pt.ctx.stats_reset()
        out = []
        for k in range(frames):
            pt.render(pt.make_gconst(cam, IW.FRAME_SPP, bounces, frame=k, flags=flags))
            out.append(pt.light()[..., :3].copy())
        segments, rays = pt.medium_info()
        assert pt.ctx.stats().emit_tex_launches == frames * (bounces - 1), "k_emit_tex runs in these frames, k_fog_shadow behind it"
        assert segments > 0 and rays > segments, "most segments queue more than one in-scatter ray"
        return np.stack(out)
    finally:
        pt.close()


@pytest.mark.parametrize("mode", (0, 1))
def test_fogged_room_against_the_float64_reference(mode):
    """A closed room lit only through the half-transmitting pane of its roof light -- by the sky, a sun, a point lamp and one textured
    emitter, pane shadows and textured emitters on -- in a box of medium, five bounces, against tests/golden/fog_ref.npz
    (ref_fog.room_radiance_samples, which samples lights its own way: only the expectation is shared), as test_pane_shadows meets its
    fixture: block means within 4.5 of the fixture's standard errors, the frames rendered to half its noise, a 2 % error rejected.
    Every sampler's in-scatter, k_fog_shadow on both shadow queues (behind k_emit_tex on the emitters'), and k_fog_segment on every later
    segment with surfaces in view meet in these frames; test_fog_cpu shows that the fixture lies many standard errors from the room
    without fog and from the room with absorption alone."""
    from test_fog_cpu import fixture

    W, H = IW.WINDOW_ROOM
    check_against_fixture(fogged_room_frames("fog_room_b5", mode), np.ones((H, W), bool), fixture(), "fog_room_b5")
