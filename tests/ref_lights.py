"""Float64 reference for the punctual lights of RT3_F_NEE_PUNCTUAL (test infrastructure).

Written from "the light is the next path vertex", not from k_shade: a point or spot light at P with radiant intensity I (W/sr) puts the
irradiance  I cos / d^2  on a surface point x, a directional light with irradiance E (W/m^2, measured across its direction) puts
E cos  there, and the surface sends  f x irradiance  towards the viewer.  A delta light is never found by a BSDF-sampled ray, so next-event
estimation is the whole of its contribution and there is no MIS weight.  Spot cone and range window are glTF KHR_lights_punctual's
recommended forms:

    cone   = clamp((cos_angle - cos_outer) / max(0.001, cos_inner - cos_outer), 0, 1)^2        (cos_angle between the axis and light -> x)
    window = clamp(1 - (d / range)^4, 0, 1)                                                   (range > 0; else 1)

Light records are assets.LIGHT_DTYPE rows; their fp32 values are taken as exact and everything else is float64.  Directions are normalised
here.  Selection masses restate include/rt3.h: 4 luminance(I) for a point or spot light (the cone is ignored), luminance(E) R^2 for a
directional one, luminance = (0.299, 0.587, 0.114) as for the emitter triangles."""
import numpy as np

import ref_pathtrace as RP
import ref_shading as R

POINT, SPOT, DIRECTIONAL = 0, 1, 2
F_NEE_SKY, F_SPECULAR, F_FACEFORWARD = RP.F_NEE_SKY, RP.F_SPECULAR, RP.F_FACEFORWARD
LUMA = np.array([0.299, 0.587, 0.114])
CDF_TOTAL = 1 << 23


def _f64(x):
    return np.asarray(x, np.float32).astype(np.float64)


def light_sample(light, x):
    """the light seen from the points x (m, 3): (wl (m, 3) unit direction to the light, distance (m,) -- inf for a directional light --,
    I' (m, 3) = I cone window, or E; geometric factor (m,) = 1 / d^2, or 1).  Where d = 0 everything is 0."""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    m = len(x)
    kind = int(light["type"])
    I = _f64(light["intensity"])
    if kind == DIRECTIONAL:
        axis = RP._unit(_f64(light["direction"]))
        return np.broadcast_to(-axis, (m, 3)).copy(), np.full(m, np.inf), np.broadcast_to(I, (m, 3)).copy(), np.ones(m)
    wv = _f64(light["position"]) - x
    d2 = np.sum(wv * wv, -1)
    ok = d2 > 0.0
    d = np.sqrt(np.where(ok, d2, 1.0))
    wl = wv / d[:, None]
    cone = np.ones(m)
    if kind == SPOT:
        axis = RP._unit(_f64(light["direction"]))
        ci, co = np.cos(float(_f64(light["inner_cone"]))), np.cos(float(_f64(light["outer_cone"])))
        cone = np.clip((np.sum(-wl * axis, -1) - co) / max(0.001, ci - co), 0.0, 1.0) ** 2
    rng = float(_f64(light["range"]))
    window = np.clip(1.0 - (d / rng) ** 4, 0.0, 1.0) if rng > 0.0 else np.ones(m)
    k = np.where(ok, cone * window, 0.0)
    return np.where(ok[:, None], wl, 0.0), np.where(ok, d, 0.0), I[None] * k[:, None], np.where(ok, 1.0 / np.where(ok, d2, 1.0), 0.0)


def cone_window_raw(light, x):
    """(c, w) before their clamps: c = (cos_angle - cos_outer) / max(0.001, cos_inner - cos_outer) and w = 1 - (d / range)^4, each 1 where
    the light has no such factor (I' = I clamp(c)^2 clamp(w)).  For tests that bound the effect of rounding next to a clamp."""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    c, w = np.ones(len(x)), np.ones(len(x))
    kind = int(light["type"])
    if kind == DIRECTIONAL:
        return c, w
    wv = _f64(light["position"]) - x
    d = np.sqrt(np.sum(wv * wv, -1))
    if kind == SPOT:
        axis = RP._unit(_f64(light["direction"]))
        ci, co = np.cos(float(_f64(light["inner_cone"]))), np.cos(float(_f64(light["outer_cone"])))
        c = (np.sum(-wv / np.maximum(d, 1e-300)[:, None] * axis, -1) - co) / max(0.001, ci - co)
    rng = float(_f64(light["range"]))
    if rng > 0.0:
        w = 1.0 - (d / rng) ** 4
    return c, w


def irradiance(light, x, n):
    """(E (m, 3), wl (m, 3), distance (m,)): what the unshadowed light puts on the surface points x with unit normals n; 0 below the horizon"""
    wl, dist, Ic, geo = light_sample(light, x)
    cs = np.sum(np.asarray(n, np.float64).reshape(-1, 3) * wl, -1)
    return Ic * (np.where(cs > 0.0, cs, 0.0) * geo)[:, None], wl, dist


def occluded(scene, x, wl, dist, chunk=16384):
    """(m,) bool: some triangle of the RP.Scene lies on the segment x + t wl, T_MIN < t < dist (Moeller-Trumbore over every triangle)"""
    x, wl, dist = np.asarray(x, np.float64), np.asarray(wl, np.float64), np.asarray(dist, np.float64)
    out = np.zeros(len(x), bool)
    for a in range(0, len(x), chunk):
        oo, dd = x[a:a + chunk, None, :], wl[a:a + chunk, None, :]
        pv = np.cross(dd, scene.e2[None])
        det = np.sum(scene.e1[None] * pv, -1)
        ok = det != 0.0
        inv = 1.0 / np.where(ok, det, 1.0)
        tv = oo - scene.v0[None]
        u = np.sum(tv * pv, -1) * inv
        qv = np.cross(tv, scene.e1[None])
        v = np.sum(dd * qv, -1) * inv
        tt = np.sum(scene.e2[None] * qv, -1) * inv
        ok &= (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0) & (tt > RP.T_MIN) & (tt < dist[a:a + chunk, None])
        out[a:a + chunk] = ok.any(1)
    return out


def powers(lights, radius2):
    """selection masses before normalisation (the emitters' unit, power / pi): 4 luminance(I), or luminance(E) R^2"""
    p = []
    for l in np.atleast_1d(lights):
        lum = float(np.sum(_f64(l["intensity"]) * LUMA))
        p.append(lum * radius2 if int(l["type"]) == DIRECTIONAL else 4.0 * lum)
    return np.array(p, np.float64)


def cdf_masses(power):
    """masses in CDF units of entries with the given powers: floor of the cumulative share of 2^23"""
    power = np.asarray(power, np.float64)
    if power.sum() <= 0.0:
        return np.zeros(len(power), np.int64)
    c = np.floor(np.cumsum(power) / power.sum() * CDF_TOTAL).astype(np.int64)
    c[-1] = CDF_TOTAL
    return np.diff(np.concatenate([[0], c]))


def radiance_samples_lit(scene, lights, cam, window, flags, bounces, n, rng):
    """RP.radiance_samples with one more term: at every vertex that is not the path's last, every light adds
    T f cos I' / d^2 (resp. T f cos E), deterministically, unless a triangle lies between the vertex and the light.
    n independent path samples per pixel: (n, H, W, 3); uncovered pixels are 0"""
    W, H = window
    o0, d0 = RP.primary_rays(cam, window)
    tri0, t0, n0 = scene.trace(o0, d0)
    cov = tri0 >= 0
    pix = np.tile(np.nonzero(cov)[0], n)
    m = len(pix)
    tri, nrm = np.tile(tri0[cov], n), np.tile(RP.gbuffer_normal(n0[cov]), (n, 1))
    d = np.tile(d0[cov], (n, 1))
    x = np.tile(o0[cov] + t0[cov, None] * d0[cov], (n, 1))
    L, T = np.zeros((m, 3)), np.ones((m, 3))
    live = np.arange(m)
    for b in range(bounces):
        first = b == 0
        g = scene.geom[tri]
        alb = (scene.albedo0 if first else scene.albedo)[g]
        L[live] += T[live] * (scene.emission0 if first else scene.emission)[g]
        if flags & F_FACEFORWARD:
            nrm = np.where((np.sum(nrm * d, -1) > 0.0)[:, None], -nrm, nrm)
        b1, b2 = RP._frame(nrm)
        wo = np.stack([-np.sum(d * b1, -1), -np.sum(d * b2, -1), -np.sum(d * nrm, -1)], -1)
        rough, metal = (scene.roughness0, scene.metalness0) if first else (scene.roughness, scene.metalness)

        def bsdf(wi):  # f (without the cosine) towards the tangent-frame directions wi
            if not flags & F_SPECULAR:
                return alb / np.pi
            f = np.zeros((len(live), 3))
            for k in np.unique(g):
                sel = g == k
                f[sel] = R.bsdf_eval(R.Material(alb[sel][0], rough[k], metal[k]), wo[sel], wi[sel])[0]
            return f

        if b < bounces - 1:  # the light is the next vertex: the path's last vertex has none
            for light in np.atleast_1d(lights):
                E, wl, dist = irradiance(light, x, nrm)
                lit = np.any(E > 0.0, -1)
                if lit.any():
                    lit[lit] = ~occluded(scene, x[lit], wl[lit], dist[lit])
                wi = np.stack([np.sum(wl * b1, -1), np.sum(wl * b2, -1), np.maximum(np.sum(wl * nrm, -1), 1e-300)], -1)
                L[live] += np.where(lit[:, None], T[live] * bsdf(wi) * E, 0.0)
        u0, u1 = rng.random(len(live)), rng.random(len(live))
        r, phi = np.sqrt(u0), 2.0 * np.pi * u1
        wi = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u0)], -1)
        T[live] *= np.pi * bsdf(wi)
        d = wi[:, :1] * b1 + wi[:, 1:2] * b2 + wi[:, 2:] * nrm
        if b == bounces - 1 and not (flags & F_NEE_SKY and scene.sky is not None):
            break
        tri, t, nrm = scene.trace(x, d)
        out = tri < 0
        if flags & F_NEE_SKY and scene.sky is not None and out.any():
            uu, vv = R.dir_to_equirect(d[out])
            L[live[out]] += T[live[out]] * R.sky_bilinear(scene.sky, uu, vv)
        keep = ~out
        live, tri, nrm, d = live[keep], tri[keep], nrm[keep], d[keep]
        x = x[keep] + t[keep, None] * d
        if len(live) == 0:
            break
    img = np.zeros((n, H * W, 3))
    img[np.repeat(np.arange(n), cov.sum()), pix] = L
    return img.reshape(n, H, W, 3)


def render_lit(scene, lights, cam, window, flags, bounces, spp, seed):
    """per-pixel (mean, variance) of `spp` per-sample values, as RP.render"""
    assert spp % RP.CHUNK_SPP == 0
    W, H = window
    s1, s2 = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    for c in range(spp // RP.CHUNK_SPP):
        v = radiance_samples_lit(scene, lights, cam, window, flags, bounces, RP.CHUNK_SPP, np.random.default_rng([seed, c]))
        s1 += v.sum(0)
        s2 += (v * v).sum(0)
    mean = s1 / spp
    return mean, np.maximum(s2 / spp - mean * mean, 0.0) * (spp / (spp - 1.0))


def gbuffer_words_normal(words):
    """the unit normal a G-buffer word holds (11-10-11 bit unorm, x in the low bits), decoded in float64"""
    w = np.asarray(words, np.uint32).reshape(-1).astype(np.int64)
    q = np.stack([(w & 2047) / 2047.0, ((w >> 11) & 1023) / 1023.0, (w >> 21) / 2047.0], -1)
    return RP._unit(q * 2.0 - 1.0)


def direct_light(scene, lights, cam, window, shadows=True, rays=None, gbuffer=None):
    """The closed form of a B = 2 frame without sky or emission: per pixel  f0 sum over the lights of the (shadowed) irradiance  at the
    float64 primary hit, f0 = G-buffer albedo / pi, with the G-buffer normal.  Returns (radiance (H, W, 3), covered (H, W), hit points
    (H W, 3), a function x -> radiance for the covered pixels' surface at other points x).  `rays` = (origins, directions) per pixel, row
    by row, replaces the ideal pinhole rays of `cam` (a direction need not be of unit length).  `gbuffer` = the frame's (H, W, 4) G-buffer
    words: the first vertex's normal and albedo are then decoded from them instead of being re-encoded here.  A normal component of
    exactly 0 sits on a rounding boundary of the 11-bit code, so which of the two neighbouring codes the frame holds is decided by the
    last bit of the normal the surface stage delivers; the estimator under test starts from the words, and so does its reference."""
    W, H = window
    o0, d0 = RP.primary_rays(cam, window) if rays is None else rays
    tri0, t0, n0 = scene.trace(o0, d0)
    cov = tri0 >= 0
    x = o0 + np.where(cov, t0, 0.0)[:, None] * d0
    nrm = RP.gbuffer_normal(n0)
    alb = scene.albedo0[scene.geom[np.where(cov, tri0, 0)]]
    if gbuffer is not None:
        gb = np.asarray(gbuffer, np.uint32).reshape(-1, 4)
        nrm = gbuffer_words_normal(gb[:, 1])
        c = np.stack([gb[:, 0] & 255, (gb[:, 0] >> 8) & 255, (gb[:, 0] >> 16) & 255], -1) / 255.0
        alb = c * c

    def at(points):
        out = np.zeros((len(points), 3))
        for light in np.atleast_1d(lights):
            E, wl, dist = irradiance(light, points, nrm)
            lit = np.any(E > 0.0, -1) & cov
            if shadows and lit.any():
                lit[lit] = ~occluded(scene, points[lit], wl[lit], dist[lit])
            out += np.where(lit[:, None], alb / np.pi * E, 0.0)
        return out

    return at(x).reshape(H, W, 3), cov.reshape(H, W), x, at
