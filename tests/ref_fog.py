"""Float64 restatement of the fog rule (raytracer3_amd/csrc/rt3_fog.hpp): the segment of a ray inside the box, its
transmittance, the in-scatter point and its density, the phase function, the single-scattering integral along a ray by quadrature, and a
float64 estimator that draws points the way the kernels do (from numpy's generator, not the device's).  span32 restates the segment in
float32, operation for operation: the device's t0, t1 and its empty / non-empty decision equal it bit for bit."""
import math

import numpy as np

F = np.float32
U = 2.0**-24
UNIFORM_BELOW = 2.0**-23
BACKGROUND_DEPTH = 100000.0
EMIT_SHADOW_END = 1.0 - 2.0**-10
FLT_MAX = float(np.finfo(np.float32).max)


def _span(o, d, t, lo, hi, dtype):
    o, d, lo, hi = (np.asarray(a, dtype).reshape(-1, 3) for a in (o, d, lo, hi))
    n = 0 if min(len(o), len(d), len(lo)) == 0 else max(len(o), len(d), len(lo))
    o, d, lo, hi = (np.broadcast_to(a, (n, 3)) for a in (o, d, lo, hi))
    t0 = np.zeros(n, dtype)
    t1 = np.broadcast_to(np.asarray(t, dtype), (n,)).copy()
    ok = np.ones(n, bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k in range(3):
            zero = d[:, k] == 0
            ok &= ~zero | ((o[:, k] >= lo[:, k]) & (o[:, k] <= hi[:, k]))
            dk = np.where(zero, dtype(1), d[:, k])
            a, b = ((lo[:, k] - o[:, k]) / dk).astype(dtype), ((hi[:, k] - o[:, k]) / dk).astype(dtype)
            nr, fr = np.where(a < b, a, b), np.where(a > b, a, b)
            t0 = np.where(zero, t0, np.where(t0 > nr, t0, nr))
            t1 = np.where(zero, t1, np.where(t1 < fr, t1, fr))
        ok &= (t1 > t0) & (t1 <= FLT_MAX)
    return ok, t0.astype(dtype), t1.astype(dtype)


def span32(o, d, t, lo, hi):
    """(in medium (n,) bool, t0, t1 float32) of fog_span, in float32"""
    return _span(o, d, t, lo, hi, F)


def span(o, d, t, lo, hi):
    return _span(o, d, t, lo, hi, np.float64)


def transmittance(sigma_t, length):
    return np.exp(-np.asarray(sigma_t, np.float64) * np.asarray(length, np.float64)[..., None])


def sample_distance(sb, length, u):
    """(ds, pdf per unit length) of fog_sample_distance for u in [0, 1)"""
    sb, length, u = np.broadcast_arrays(np.asarray(sb, np.float64), np.asarray(length, np.float64), np.asarray(u, np.float64))
    a = sb * length
    with np.errstate(divide="ignore", invalid="ignore"):
        E = -np.expm1(-a)
        ds = np.minimum(-np.log1p(-(u * E)) / sb, length)
        pdf = sb * np.exp(-sb * ds) / E
        uni = ~(a >= UNIFORM_BELOW)
        ds = np.where(uni, u * length, ds)
        pdf = np.where(uni, 1.0 / length, pdf)
    return ds, pdf


def phase(g, c):
    den = 1.0 + g * g - 2.0 * g * np.asarray(c, np.float64)
    return (1.0 - g * g) / (4.0 * math.pi * den * np.sqrt(den))


def shadow_length(x, w, tmax, lo, hi):
    """length of x + r w, r in [0, tmax], inside the box (w unit)"""
    ok, t0, t1 = span(x, w, tmax, lo, hi)
    return np.where(ok, t1 - t0, 0.0)


# ---------------------------------------------------------------------------------------------------------------- op 45
def rule_rows(rows):
    """rows (n, 20) float32 {o, d, t, lo, hi, sigma_a, sigma_s, u} -> dict of what op 45 returns, in float64 from the same fp32 inputs
    (t0 and t1 from span32: they are exact), and the derived bounds (rule_bounds' docstring)"""
    r32 = np.asarray(rows, F).reshape(-1, 20)
    o, d, t, lo, hi = r32[:, 0:3], r32[:, 3:6], r32[:, 6], r32[:, 7:10], r32[:, 10:13]
    sigma_t = (r32[:, 13:16] + r32[:, 16:19]).astype(F).astype(np.float64)  # the fp32 sum rt3_scene_set_medium makes once
    u = r32[:, 19].astype(np.float64)
    hit, t0, t1 = span32(o, d, t, lo, hi)
    t0, t1 = t0.astype(np.float64), t1.astype(np.float64)
    dl = np.linalg.norm(d.astype(np.float64), axis=1)
    length = np.where(hit, (t1 - t0) * dl, 1.0)
    sb = sigma_t.sum(1) / 3.0
    sb_safe = np.where(sb > 0, sb, 1.0)
    ds, pdf = sample_distance(sb_safe, length, u)
    zero = ~(sb > 0)
    ds, pdf = np.where(zero, u * length, ds), np.where(zero, 1.0 / length, pdf)
    s = t0 + ds / dl
    Tr = transmittance(sigma_t, length)
    return dict(hit=hit, t0=t0, t1=t1, s=s, pdf=pdf, Tr=Tr, a=sigma_t * length[:, None], ab=sb * length, L=sb * ds, ds=ds, dl=dl, length=length, sb=sb)


def rule_bounds(ref):
    """Bounds of op 45 against rule_rows, U = 2^-24, derived and not measured.  t0 and t1 are exact inputs here.
      len = (t1 - t0) |d|: dot(d, d) has positive terms (3 U relative), the square root halves that and adds its own (2.5 U), the difference
        and the product round once each: 4.5 U, say 5 U relative.
      Tr.c = expf(-(sigma_t.c len)): the product rounds once, so the exponent a.c carries 6 a U absolute and the result 6 a U relative; expf is
        documented at 1 ulp = 2 U; second order in the third unit: (3 + 7 a) U relative.
      sb = (sum of three) / 3: 3 U.  ab = sb len: 9 U relative.  E = -expm1f(-ab): the argument's error moves E by 9 U ab e^-ab / E <= 9 U
        relative, expm1f 1 ulp: 11 U.  u E: 12 U.  w = 1 - u E.  L = -log1pf(-(u E)): the argument's error moves it by 12 U (1 - w) / w
        absolute, log1pf 1 ulp = 2 U L.  ds = L / sb: 4 U L more (sb, the division).  dL = (12 (1 - w) / w + 6 L) U absolute on L = sb ds.
        The clamp to len can only bring ds nearer: where it acts, ds is len, 5 U relative, i.e. 5 U ab on L.  Together dL + 5 ab U.
      s = t0 + ds / |d|: (dL + 5 ab U) / (sb |d|) + 6 U ds / |d| + 2 U |t0| absolute.
      pdf = sb expf(-(sb ds)) / E at the device's ds: the exponent carries the device's dL, the product's and sb's 4 U L; expf 2 U, sb 3 U, E
        11 U, product and quotient 2 U, one unit for the second order: dL + 5 ab U + (4 L + 19) U relative.
      Uniform branch (ab < 2^-23): ds = u len, pdf = 1 / len: 6 U relative each."""
    L, ab, sb, dl = ref["L"], ref["ab"], ref["sb"], ref["dl"]
    uni = ~(ab >= UNIFORM_BELOW)
    w = np.exp(-np.minimum(L, 700.0))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dL = (12.0 * (1.0 - w) / w + 6.0 * L + 5.0 * ab) * U
        s_abs = np.where(uni, 6.0 * U * ref["ds"] / dl, dL / (np.where(sb > 0, sb, 1.0) * dl) + 6.0 * U * ref["ds"] / dl) + 2.0 * U * np.abs(ref["t0"])
        pdf_rel = np.where(uni, 6.0 * U, dL + (4.0 * L + 19.0) * U)
    return dict(Tr=(3.0 + 7.0 * ref["a"]) * U, s=s_abs, pdf=pdf_rel)


# ---------------------------------------------------------------------------------------------------------------- lights and the integral
class Directional:
    def __init__(self, direction, E):
        self.w = -np.asarray(direction, np.float64) / np.linalg.norm(direction)  # towards the light
        self.E = np.asarray(E, np.float64)

    def samples(self, x, rng=None):
        """the light samples at the points x whose sum is the light's in-scattered radiance: tuples (w_l (n, 3), L_e / pdf_light (n, 3),
        tmax (n,)).  A punctual light has one; an area light one random point with `rng`, or a fixed grid of points without"""
        n = len(x)
        return [(np.broadcast_to(self.w, (n, 3)), np.broadcast_to(self.E, (n, 3)), np.full(n, BACKGROUND_DEPTH))]


class Point:
    def __init__(self, position, I):
        self.p, self.I = np.asarray(position, np.float64), np.asarray(I, np.float64)

    def samples(self, x, rng=None):
        v = self.p - x
        dist = np.linalg.norm(v, axis=1)
        return [(v / dist[:, None], self.I / (dist * dist)[:, None], dist * EMIT_SHADOW_END)]


class Panel:
    """a parallelogram emitter A + a E1 + b E2, a, b in [0, 1], radiance Le on both sides: the light table's two triangles of equal mass,
    each sampled uniformly, are one uniform density 1 / area on the whole; the solid-angle density is dist^2 / (area |cos_l|)"""

    def __init__(self, A, E1, E2, Le, grid=12):
        self.A, self.E1, self.E2, self.Le = (np.asarray(v, np.float64) for v in (A, E1, E2, Le))
        nrm = np.cross(self.E1, self.E2)
        self.area = float(np.linalg.norm(nrm))
        self.n = nrm / self.area
        self.grid = grid

    def _towards(self, x, a, b, weight):
        v = self.A + a[:, None] * self.E1 + b[:, None] * self.E2 - x
        dist = np.linalg.norm(v, axis=1)
        w = v / dist[:, None]
        cle = np.abs(w @ self.n)
        return w, self.Le * (weight * cle / (dist * dist))[:, None], dist * EMIT_SHADOW_END

    def samples(self, x, rng=None):
        n = len(x)
        if rng is not None:
            return [self._towards(x, rng.random(n), rng.random(n), self.area)]
        m = self.grid
        return [self._towards(x, np.full(n, (i + 0.5) / m), np.full(n, (j + 0.5) / m), self.area / (m * m)) for i in range(m) for j in range(m)]


def inscatter(x, d_unit, medium, light, visible=None, rng=None, factor=None):
    """sigma_s p_HG L_e Tr_shadow at the points x (n, 3) of rays with unit directions d_unit: the integrand without the ray's own Tr.
    factor(w_l): what else the shadow ray meets (a pane's attenuation), per channel"""
    sigma_t, sigma_s, g, lo, hi = medium
    val = 0.0
    for wl, le, tmax in light.samples(x, rng):
        ls = shadow_length(x, wl, tmax, lo, hi)
        term = np.asarray(sigma_s, np.float64) * phase(g, np.sum(d_unit * wl, 1))[:, None] * le * transmittance(sigma_t, ls)
        val = val + (term if factor is None else term * factor(wl))
    if visible is not None:
        val = val * visible(x)[:, None]
    return val


def quadrature(o, d_unit, t_end, medium, light, visible=None, n=2048):
    """the single-scattering radiance (rays, 3) along rays o + r d_unit, r in [0, t_end]: midpoint rule on the part inside the box"""
    sigma_t, _, _, lo, hi = medium
    o = np.broadcast_to(np.asarray(o, np.float64), d_unit.shape)
    ok, t0, t1 = span(o, d_unit, t_end, lo, hi)
    out = np.zeros((len(d_unit), 3))
    idx = np.flatnonzero(ok)
    h = (t1[idx] - t0[idx]) / n
    for k in range(n):
        r = (k + 0.5) * h
        x = o[idx] + (t0[idx] + r)[:, None] * d_unit[idx]
        out[idx] += inscatter(x, d_unit[idx], medium, light, visible) * transmittance(sigma_t, r) * h[:, None]
    return out


def estimator(o, d_unit, t_end, medium, light, N, rng, visible=None):
    """N samples per ray of the kernels' estimator in float64: (mean (rays, 3), standard error of the mean (rays, 3))"""
    sigma_t, _, _, lo, hi = medium
    o = np.broadcast_to(np.asarray(o, np.float64), d_unit.shape)
    ok, t0, t1 = span(o, d_unit, t_end, lo, hi)
    idx = np.flatnonzero(ok)
    s1, s2 = np.zeros((len(d_unit), 3)), np.zeros((len(d_unit), 3))
    length = t1[idx] - t0[idx]
    sb = float(np.mean(sigma_t))
    for _ in range(N):
        u = np.floor(rng.random(len(idx)) * 2.0**23) / 2.0**23
        ds, pdf = sample_distance(sb, length, u)
        x = o[idx] + (t0[idx] + ds)[:, None] * d_unit[idx]
        v = inscatter(x, d_unit[idx], medium, light, visible, rng) * transmittance(sigma_t, ds) / pdf[:, None]
        s1[idx] += v
        s2[idx] += v * v
    mean = s1 / N
    var = np.maximum(s2 / N - mean * mean, 0.0) * N / max(N - 1, 1)
    return mean, np.sqrt(var / N)


# ---------------------------------------------------------------------------------------------------------------- a fogged room
def room_radiance_samples(scene, camera, window, flags, bounces, n, rng, *, lens, medium, glass, panes, surface=None, lights=()):
    """n independent path samples per pixel of a scene with glass, panes and pane shadows inside a medium: (n, H, W, 3).

    ref_pane_shadows.radiance_samples' estimator (its camera, glass vertex, light samples through panes and weights P1 and P2; its
    functions are called) with the fog rule of this module at its three places: every traced segment attenuates the throughput over its
    stretch inside the box and draws one in-scatter point, lit by a sky sample, a point on an emitter and every punctual light, each
    through the panes and the medium on its way, weight 1; and every light sample of a surface is attenuated over its own stretch.
    Light sampling is ref_pane_shadows' own (luminance-proportional sky texels, emitter points uniform over the emissive area, every
    punctual light), not the kernels': only the expectation is shared.  An emitter's radiance at a sampled point is the surface's there,
    so an emissive texture shows on both sides of the weight."""
    import ref_combined as RC
    import ref_glass as RG
    import ref_lens as RLE
    import ref_lights as RL
    import ref_pane_shadows as RPS
    import ref_pathtrace as RP
    import ref_shading as R

    sigma_t, sigma_s, g_hg, lo, hi = medium
    sb = float(np.mean(sigma_t))
    scatter = bool(np.any(np.asarray(sigma_s) > 0))
    spec = bool(flags & RPS.F_SPECULAR)
    tau, ior, thin = glass
    W, H = window
    nee_sky = bool(flags & RPS.F_NEE_SKY) and scene.sky is not None
    sampler = RPS.SkySampler(scene.sky) if nee_sky else None
    e_idx, e_area, e_nrm = RPS.emitter_table(scene)
    nee_e = bool(flags & RPS.F_NEE_EMISSIVE) and len(e_idx) > 0
    p_area = 1.0 / e_area.sum() if nee_e else 0.0
    tri_is_emitter = np.zeros(len(scene.geom), bool)
    tri_is_emitter[e_idx] = True
    geo_n = np.cross(scene.e1, scene.e2)
    geo_n = geo_n / np.maximum(np.linalg.norm(geo_n, axis=1, keepdims=True), 1e-300)

    def sky(dirs):
        return R.sky_bilinear(scene.sky, *R.dir_to_equirect(dirs))

    def weight(pb, pl):
        return np.where(np.isinf(pb), 1.0, pb / (np.where(np.isinf(pb), 1.0, pb) + pl))

    def along(x, w, tmax):  # the medium's transmittance along the light sample x + r w, r in [0, tmax]
        return transmittance(sigma_t, shadow_length(x, w, tmax, lo, hi))

    def through(x, w, tmax, c):
        return RPS.through_panes(scene, surface, glass, panes, x, w, tmax, c)

    def emitter_points(x, k):
        pick = rng.choice(len(e_idx), size=k, p=e_area * p_area)
        su, u7 = np.sqrt(rng.random(k)), rng.random(k)
        et = e_idx[pick]
        pe = scene.v0[et] + scene.e1[et] * (u7 * su)[:, None] + scene.e2[et] * (su - u7 * su)[:, None]
        wv = pe - x
        dist = np.linalg.norm(wv, axis=1)
        wle = wv / np.maximum(dist, 1e-300)[:, None]
        cle = np.abs(np.sum(e_nrm[pick] * wle, -1))
        emi = RC._materials(scene, surface, et, pe, e_nrm[pick])[1]
        return wle, dist, cle, emi

    def fog_segment(L, T, paths, o, d, t_end):
        """the segments o + r d, r in [0, t_end], of the paths `paths`: T attenuated in place, the in-scattered light added to L"""
        ok, t0, t1 = span(o, d, t_end, lo, hi)
        q = np.nonzero(ok)[0]
        if not len(q):
            return
        length = t1[q] - t0[q]
        Tb = T[paths[q]].copy()
        T[paths[q]] = Tb * transmittance(sigma_t, length)
        if not scatter:
            return
        k = len(q)
        ds, pdf = sample_distance(sb, length, rng.random(k))
        xs = o[q] + (t0[q] + ds)[:, None] * d[q]
        w = Tb * transmittance(sigma_t, ds) * np.asarray(sigma_s) / pdf[:, None]
        if nee_sky:
            wl, pl = sampler.sample(rng, k)
            c = w * sky(wl) * (phase(g_hg, np.sum(d[q] * wl, -1)) / pl)[:, None] * along(xs, wl, np.inf)
            L[paths[q]] += through(xs, wl, np.full(k, np.inf), c)
        if nee_e:
            wle, dist, cle, emi = emitter_points(xs, k)
            use = (cle > 0.0) & (dist > 0.0)
            ps = p_area * dist * dist / np.maximum(cle, 1e-300)
            c = np.where(use[:, None], w * emi * (phase(g_hg, np.sum(d[q] * wle, -1)) / ps)[:, None] * along(xs, wle, dist), 0.0)
            L[paths[q]] += through(xs, wle, dist * RPS.SEGMENT_END, c)
        for light in lights:
            wp, dp, Ip, geo = RL.light_sample(light, xs)
            c = w * Ip * (phase(g_hg, np.sum(d[q] * wp, -1)) * geo)[:, None] * along(xs, wp, dp)
            L[paths[q]] += through(xs, wp, dp * RPS.SEGMENT_END, c)

    pinv, vinv = RLE.camera_matrices(camera, window)
    py, px = np.mgrid[0:H, 0:W]
    px, py = np.tile(px.reshape(-1), n), np.tile(py.reshape(-1), n)
    m = len(px)
    x, d, _, _ = RLE.camera_sample(pinv, vinv, window, lens, px, py, rng.random((m, 4)))
    L, T = np.zeros((m, 3)), np.ones((m, 3))
    chain = np.ones(m, bool)
    tri, t, nrm = scene.trace(x, d)
    out = tri < 0
    fog_segment(L, T, np.arange(m), x, d, np.where(out, np.inf, t))
    if scene.sky is not None and out.any():
        L[out] += T[out] * sky(d[out])
    live = np.nonzero(~out)[0]
    tri, nrm, d, tl = tri[live], nrm[live], d[live], t[live]
    x = x[live] + tl[:, None] * d
    pb, D = np.full(len(live), np.inf), np.zeros(len(live))
    for b in range(bounces):
        k = len(live)
        if k == 0:
            break
        last = b == bounces - 1
        alb, emi, nrm, rough, metal = RC._materials(scene, surface, tri, x, nrm)
        w_e = np.ones(k)
        if nee_e:
            dist = D + tl
            cle = np.abs(np.sum(geo_n[tri] * d, -1))
            ps = p_area * dist * dist / np.maximum(cle, 1e-300)
            w_e = np.where(tri_is_emitter[tri] & (cle > 0), weight(pb, ps), 1.0)
        L[live] += T[live] * emi * w_e[:, None]
        g = scene.geom[tri]
        is_glass = (tau[g] > 0.0) & ((tau[g] >= 1.0) | (rng.random(k) < tau[g]))
        nf = np.where(((np.sum(nrm * d, -1) > 0.0) & bool(flags & RPS.F_FACEFORWARD))[:, None], -nrm, nrm)
        b1, b2 = RP._frame(nf)
        wo = np.stack([-np.sum(d * b1, -1), -np.sum(d * b2, -1), -np.sum(d * nf, -1)], -1)
        op = ~is_glass

        def bsdf(q, w):
            if not spec:
                return alb[q] / np.pi
            wi_l = np.stack([np.sum(w * b1[q], -1), np.sum(w * b2[q], -1), np.sum(w * nf[q], -1)], -1)
            return RLE.layered_value(alb[q], rough[q], metal[q], wo[q], wi_l)

        if nee_sky:
            wl, pl = sampler.sample(rng, k)
            cs = np.sum(nf * wl, -1)
            q = np.nonzero(op & (cs > 0.0))[0]
            if len(q):
                den = pl[q] if last else pl[q] + cs[q] / np.pi
                c = T[live[q]] * bsdf(q, wl[q]) * sky(wl[q]) * (cs[q] / den)[:, None] * along(x[q], wl[q], np.inf)
                L[live[q]] += through(x[q], wl[q], np.full(len(q), np.inf), c)
        if nee_e and not last:
            wle, dist, cle, e_emi = emitter_points(x, k)
            cs = np.sum(nf * wle, -1)
            q = np.nonzero(op & (cs > 0.0) & (cle > 0.0) & (dist > 0.0))[0]
            if len(q):
                ps = p_area * dist[q] ** 2 / cle[q]
                c = T[live[q]] * bsdf(q, wle[q]) * e_emi[q] * (cs[q] / (ps + cs[q] / np.pi))[:, None] * along(x[q], wle[q], dist[q])
                L[live[q]] += through(x[q], wle[q], dist[q] * RPS.SEGMENT_END, c)
        if not last:
            for light in lights:
                wp, dp, Ip, geo = RL.light_sample(light, x)
                cs = np.sum(nf * wp, -1)
                q = np.nonzero(op & (cs > 0.0) & (geo > 0.0))[0]
                if len(q):
                    c = T[live[q]] * bsdf(q, wp[q]) * Ip[q] * (cs[q] * geo[q])[:, None] * along(x[q], wp[q], dp[q])
                    L[live[q]] += through(x[q], wp[q], dp[q] * RPS.SEGMENT_END, c)
        u0, u1 = rng.random(k), rng.random(k)
        r, phi = np.sqrt(u0), 2.0 * np.pi * u1
        wi = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u0)], -1)
        d_opaque = wi[:, :1] * b1 + wi[:, 1:2] * b2 + wi[:, 2:] * nf
        transmit, d_glass, _ = RG.glass_event(ior[g], thin[g], d, nrm, rng.random(k))
        straight = is_glass & transmit & panes[g]
        T[live] *= np.where(is_glass[:, None], np.where(transmit[:, None], alb, 1.0), np.pi * bsdf(np.arange(k), d_opaque))
        d = np.where(is_glass[:, None], d_glass, d_opaque)
        pb = np.where(straight, pb, np.where(is_glass, np.inf, wi[:, 2] / np.pi))
        D = np.where(straight, D + tl, 0.0)
        chain[live] &= is_glass
        if last:
            if nee_sky and is_glass.any():
                q = np.nonzero(is_glass)[0]
                c = T[live[q]] * sky(d[q]) * weight(pb[q], sampler.pdf(d[q]))[:, None] * along(x[q], d[q], np.inf)
                L[live[q]] += through(x[q], d[q], np.full(len(q), np.inf), c)
            break
        tri, tl, nrm = scene.trace(x, d)
        out = tri < 0
        fog_segment(L, T, live, x, d, np.where(out, np.inf, tl))
        if scene.sky is not None and out.any():
            if nee_sky:
                L[live[out]] += T[live[out]] * sky(d[out]) * weight(pb[out], sampler.pdf(d[out]))[:, None]
            else:
                sees = out & chain[live]
                L[live[sees]] += T[live[sees]] * sky(d[sees])
        keep = ~out
        live, tri, nrm, d, tl, pb, D = live[keep], tri[keep], nrm[keep], d[keep], tl[keep], pb[keep], D[keep]
        x = x[keep] + tl[:, None] * d
    return L.reshape(n, H, W, 3)


def room_chunk_sums(scene, camera, window, flags, bounces, seed, chunk, **features):
    """(sum, sum of squares) over the samples of chunk `chunk` (ref_pathtrace.CHUNK_SPP of them, from default_rng([seed, chunk]))"""
    import ref_pathtrace as RP

    v = room_radiance_samples(scene, camera, window, flags, bounces, RP.CHUNK_SPP, np.random.default_rng([seed, chunk]), **features)
    return v.sum(0), (v * v).sum(0)
