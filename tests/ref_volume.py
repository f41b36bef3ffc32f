"""Float64 NumPy path tracer with absorbing glass (test infrastructure; DESIGN.md sections 2 and 4s): ref_glass's estimator with the one rule
of rt3_scene_set_attenuation, restated from its definition, and the closed forms of an absorbing slab.

The rule: a path segment that arrives at a back face of an absorbing geometry (dot(shading normal, d) > 0) ran inside it; its throughput is
multiplied by exp(-sigma x), x the segment's length, per channel.  Camera segments are not attenuated.  A scene without an absorbing
geometry is ref_glass.radiance_samples itself (called, so the samples are its own); with one the loop is ref_glass's, word for word, with
the rule after each trace inside the loop, so that every random number is drawn as ref_glass draws it."""
import numpy as np

import ref_combined as RC
import ref_glass as RG
import ref_lens as RLE
import ref_pathtrace as RP
import ref_shading as R

F_NEE_SKY, F_SPECULAR, F_FACEFORWARD = RP.F_NEE_SKY, RP.F_SPECULAR, RP.F_FACEFORWARD


# ---------------------------------------------------------------------------------------------------------------- the rule
def absorb(T, sigma, x, n, d):
    """T (m, 3) after a segment of length x (m,) that ends at shading normal n with direction d, through sigma (m, 3): float64"""
    back = (np.sum(np.asarray(n, np.float64) * np.asarray(d, np.float64), -1) > 0.0) & np.any(np.asarray(sigma) > 0.0, -1)
    f = np.exp(-np.asarray(sigma, np.float64) * np.asarray(x, np.float64)[..., None])
    return np.where(back[..., None], np.asarray(T, np.float64) * f, T), back


# ---------------------------------------------------------------------------------------------------------------- closed forms
def slab_matched(sigma, segment):
    """transmittance of an index-matched absorbing slab crossed on a straight segment of length `segment` (thickness / cos theta for
    ideal faces): exp(-sigma segment) per channel, (..., 3)"""
    return np.exp(-np.asarray(sigma, np.float64) * np.asarray(segment, np.float64)[..., None])


def slab_R_T(sigma, thickness, cos_i, ior, single_segment=False):
    """(R, T) of an absorbing slab with every inter-reflection summed: with F the Fresnel reflectance of either face and
    a = exp(-sigma thickness / cos_t),  R = F + (1 - F)^2 F a^2 / (1 - F^2 a^2),  T = (1 - F)^2 a / (1 - F^2 a^2); (..., 3) each.
    single_segment: the wrong model that attenuates one internal segment only -- the a^2 terms at a = 1."""
    cos_i = np.asarray(cos_i, np.float64)
    F = RG.fresnel(cos_i, ior)[..., None]
    cos_t = RG.cos_transmitted(cos_i, ior)
    a = np.exp(-np.asarray(sigma, np.float64) * thickness / cos_t[..., None])
    a2 = np.ones_like(a) if single_segment else a * a
    return F + (1.0 - F) ** 2 * F * a2 / (1.0 - F * F * a2), (1.0 - F) ** 2 * a / (1.0 - F * F * a2)


def slab_tail(sigma, thickness, cos_i, ior, bounces):
    """what stopping at `bounces` vertices can cost a slab pixel at most, relative to the sky: (1 - F) (F a)^(B - 1)"""
    cos_i = np.asarray(cos_i, np.float64)
    F = RG.fresnel(cos_i, ior)[..., None]
    a = np.exp(-np.asarray(sigma, np.float64) * thickness / RG.cos_transmitted(cos_i, ior)[..., None])
    return (1.0 - F) * (F * a) ** (bounces - 1)


# ---------------------------------------------------------------------------------------------------------------- the tracer
def radiance_samples(scene, camera, window, flags, bounces, n, rng, *, lens, glass=None, sigma=None, surface=None):
    """n independent path samples per pixel: (n, H, W, 3).  glass: ref_glass.table(mesh); sigma: (g, 3) absorption coefficients per
    geometry, 0 where the geometry does not absorb (volume_worlds.sigma_table), or None."""
    if sigma is None or not np.any(np.asarray(sigma) > 0.0) or glass is None or not np.any(glass[0] > 0.0):
        return RG.radiance_samples(scene, camera, window, flags, bounces, n, rng, lens=lens, glass=glass, surface=surface)
    sigma = np.asarray(sigma, np.float64)
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
    chain = np.ones(m, bool)
    tri, t, nrm = scene.trace(x, d)  # the camera segment: not attenuated
    out = tri < 0
    if scene.sky is not None and out.any():
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
        transmit, d_glass, _ = RG.glass_event(ior[g], thin[g], d, nrm, rng.random(k))
        T[live] *= np.where(is_glass[:, None], np.where(transmit[:, None], alb, 1.0), np.pi * f)
        d = np.where(is_glass[:, None], d_glass, d_opaque)
        chain[live] &= is_glass
        if b == bounces - 1 and not nee_sky:
            break
        tri, t, nrm = scene.trace(x, d)
        out = tri < 0
        hit = np.nonzero(~out)[0]
        if len(hit):  # the rule: the segment that arrives at a back face of an absorbing geometry ran inside it
            seg = t[hit] * np.linalg.norm(d[hit], axis=-1)
            T[live[hit]] = absorb(T[live[hit]], sigma[scene.geom[tri[hit]]], seg, nrm[hit], d[hit])[0]
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
