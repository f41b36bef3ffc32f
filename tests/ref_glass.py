"""Float64 NumPy path tracer with glass (test infrastructure; DESIGN.md sections 2 and 4n): ref_combined's estimator with the transmissive
dielectric of rt3_scene_set_transmission, rules 1-5 of include/rt3.h restated from their definitions.

A scene without glass is ref_combined.radiance_samples itself (called, so the samples are its own).  With glass the loop is this module's,
built from the parents' functions: ref_lens.camera_sample for the camera (glass needs per-sample camera rays), ref_combined's surfaces
and closest hits, ref_pathtrace's tangent frame, ref_shading's BSDF and sky.

  1. lobe selection   a vertex on a geometry with transmission t > 0 is a glass vertex when its selection draw u < t (always at t = 1);
                      otherwise it is ref_combined's opaque vertex, from ref_combined's draws;
  2. glass vertex     glass_event below: exact Fresnel, mirror reflection with probability F, else transmission with throughput x albedo;
                      thin-walled surfaces transmit straight on with F' = 2 F / (1 + F);
  3. delta            a glass vertex adds no light sample (this estimator has none to drop: lights are not taken with glass);
  4. last vertex      the ray leaving vertex B adds sky under NEE_SKY, from a glass vertex as from any other;
  5. sky              without NEE_SKY a ray that escapes after nothing but glass vertices since the camera adds throughput x sky.

Random numbers per vertex, for every live path: the selection draw, ref_combined's two direction draws, the event draw."""
import numpy as np

import ref_combined as RC
import ref_lens as RLE
import ref_pathtrace as RP
import ref_shading as R

F_NEE_SKY, F_SPECULAR, F_FACEFORWARD = RP.F_NEE_SKY, RP.F_SPECULAR, RP.F_FACEFORWARD


# ---------------------------------------------------------------------------------------------------------------- the dielectric
def fresnel(cos_i, eta):
    """unpolarised Fresnel reflectance of a smooth interface met at cos_i >= 0 from the side where the relative index of the far medium
    is eta; 1 under total internal reflection"""
    cos_i, eta = np.broadcast_arrays(np.asarray(cos_i, np.float64), np.asarray(eta, np.float64))
    ct2 = 1.0 - (1.0 - cos_i * cos_i) / (eta * eta)
    tir = ct2 <= 0.0
    ct = np.sqrt(np.where(tir, 1.0, ct2))
    rs = (cos_i - eta * ct) / (cos_i + eta * ct)
    rp = (eta * cos_i - ct) / (eta * cos_i + ct)
    return np.where(tir, 1.0, 0.5 * (rs * rs + rp * rp))


def cos_transmitted(cos_i, eta):
    """cos of the refracted angle; 0 under total internal reflection"""
    ct2 = 1.0 - (1.0 - np.asarray(cos_i, np.float64) ** 2) / np.asarray(eta, np.float64) ** 2
    return np.sqrt(np.maximum(ct2, 0.0))


def thin_fresnel(F):
    """reflectance of a thin slab with both faces' inter-reflections summed: F + (1 - F)^2 F / (1 - F^2) = 2 F / (1 + F)"""
    F = np.asarray(F, np.float64)
    return 2.0 * F / (1.0 + F)


def glass_event(ior, thin, d, n, u):
    """(transmit (m,) bool, direction (m, 3) unit, reflection probability (m,)) of rays d (any length) at shading normals n (unit, not
    face-forwarded); ior, thin and u per row or scalars"""
    d = np.asarray(d, np.float64)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    n = np.asarray(n, np.float64)
    ior = np.broadcast_to(np.asarray(ior, np.float64), d.shape[:1])
    thin = np.broadcast_to(np.asarray(thin, bool), d.shape[:1])
    c = np.sum(n * d, -1)
    enter = c < 0.0
    cos_i = np.abs(c)
    eta = np.where(thin | enter, ior, 1.0 / ior)
    F = fresnel(cos_i, eta)
    F = np.where(thin, thin_fresnel(F), F)
    transmit = ~(np.asarray(u, np.float64) < F)
    n_in = np.where(enter[:, None], n, -n)  # the normal on the incoming side
    refl = d - 2.0 * c[:, None] * n
    refr = d / eta[:, None] + (cos_i / eta - cos_transmitted(cos_i, eta))[:, None] * n_in
    tdir = np.where(thin[:, None], d, refr)
    return transmit, np.where(transmit[:, None], tdir, refl), F


def table(mesh):
    """(transmission, ior, thin_walled) per geometry as float64 / bool arrays, from Mesh.transmission"""
    t = mesh.transmission
    return np.asarray(t["transmission"], np.float64), np.asarray(t["ior"], np.float64), np.asarray(t["thin_walled"]) != 0


# ---------------------------------------------------------------------------------------------------------------- the tracer
def radiance_samples(scene, camera, window, flags, bounces, n, rng, *, lens, glass=None, surface=None):
    """n independent path samples per pixel: (n, H, W, 3).  glass: table(mesh) or None; lens: (R, F, jitter), required with glass."""
    if glass is None or not np.any(glass[0] > 0.0):
        return RC.radiance_samples(scene, camera, window, flags, bounces, n, rng, lens=lens, surface=surface)
    assert lens is not None, "glass needs per-sample camera rays"
    tau, ior, thin = glass
    W, H = window
    nee_sky = bool(flags & F_NEE_SKY) and scene.sky is not None

    def sky(dirs):
        return R.sky_bilinear(scene.sky, *R.dir_to_equirect(dirs))

    pinv, vinv = RLE.camera_matrices(camera, window)
    py, px = np.mgrid[0:H, 0:W]
    px, py = np.tile(px.reshape(-1), n), np.tile(py.reshape(-1), n)
    m = len(px)
    x, d, _, _ = RLE.camera_sample(pinv, vinv, window, lens, px, py, rng.random((m, 4)))
    L, T = np.zeros((m, 3)), np.ones((m, 3))
    chain = np.ones(m, bool)  # nothing but glass since the camera
    tri, t, nrm = scene.trace(x, d)
    out = tri < 0
    if scene.sky is not None and out.any():  # an escaped camera sample sees the sky, with or without NEE_SKY
        L[out] += sky(d[out])
    live = np.nonzero(~out)[0]
    tri, nrm, d = tri[live], nrm[live], d[live]
    x = x[live] + t[live, None] * d
    for b in range(bounces):
        k = len(live)
        if k == 0:
            break
        alb, emi, nrm, rough, metal = RC._materials(scene, surface, tri, x, nrm)
        L[live] += T[live] * emi
        g = scene.geom[tri]
        us = rng.random(k)
        is_glass = (tau[g] > 0.0) & ((tau[g] >= 1.0) | (us < tau[g]))
        # the opaque vertex (ref_combined's, in its words)
        nf = np.where(((np.sum(nrm * d, -1) > 0.0) & bool(flags & F_FACEFORWARD))[:, None], -nrm, nrm)
        b1, b2 = RP._frame(nf)
        wo = np.stack([-np.sum(d * b1, -1), -np.sum(d * b2, -1), -np.sum(d * nf, -1)], -1)
        u0, u1 = rng.random(k), rng.random(k)
        r, phi = np.sqrt(u0), 2.0 * np.pi * u1
        wi = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u0)], -1)
        if not flags & F_SPECULAR:
            f = alb / np.pi
        elif surface is not None:
            f = RLE.layered_value(alb, rough, metal, wo, wi)
        else:
            f = np.zeros((k, 3))
            for q in np.unique(g):
                sel = g == q
                f[sel] = R.bsdf_eval(R.Material(alb[sel][0], rough[sel][0], metal[sel][0]), wo[sel], wi[sel])[0]
        d_opaque = wi[:, :1] * b1 + wi[:, 1:2] * b2 + wi[:, 2:] * nf
        # the glass vertex
        transmit, d_glass, _ = glass_event(ior[g], thin[g], d, nrm, rng.random(k))
        T[live] *= np.where(is_glass[:, None], np.where(transmit[:, None], alb, 1.0), np.pi * f)
        d = np.where(is_glass[:, None], d_glass, d_opaque)
        chain[live] &= is_glass
        if b == bounces - 1 and not nee_sky:
            break  # the ray leaving the last vertex can only add sky, and only under NEE_SKY
        tri, t, nrm = scene.trace(x, d)
        out = tri < 0
        if scene.sky is not None and out.any():
            sees = out & (nee_sky | chain[live])
            L[live[sees]] += T[live[sees]] * sky(d[sees])
        keep = ~out
        live, tri, nrm, d = live[keep], tri[keep], nrm[keep], d[keep]
        x = x[keep] + t[keep, None] * d
    return L.reshape(n, H, W, 3)


def chunk_sums(scene, camera, window, flags, bounces, seed, chunk, **features):
    """(sum, sum of squares) over the samples of chunk `chunk` (RP.CHUNK_SPP of them, from default_rng([seed, chunk])): (H, W, 3) each"""
    v = radiance_samples(scene, camera, window, flags, bounces, RP.CHUNK_SPP, np.random.default_rng([seed, chunk]), **features)
    return v.sum(0), (v * v).sum(0)


def render(scene, camera, window, flags, bounces, spp, seed, **features):
    """per-pixel (mean, variance) of `spp` per-sample values, spp a multiple of ref_pathtrace.CHUNK_SPP; (H, W, 3) each"""
    assert spp % RP.CHUNK_SPP == 0
    return RC.mean_var([chunk_sums(scene, camera, window, flags, bounces, seed, c, **features) for c in range(spp // RP.CHUNK_SPP)], spp)
