"""Float64 NumPy path tracer with pane shadows (test infrastructure): ref_glass's scene, camera and glass vertex with
next-event estimation THROUGH thin-walled panes, rules P1 and P2 of section 4q restated from their definitions.

With `pane_shadows` off this is ref_glass.radiance_samples itself (called, so the samples are its own).  With it on the estimator is this
module's -- it is not ref_glass's estimator with a switch, because ref_glass takes no light samples at all (it follows BSDF samples and
adds what they find with weight 1); the two have the same expectation, which tests/test_pane_shadows_cpu.py checks:

  P1  a light sample's segment may cross panes (geometries with transmission > 0 that are thin-walled); each crossing multiplies its
      contribution by A = transmission (1 - F'(cos_i)) tint; anything else on the segment occludes;
  P2  a glass vertex on a pane that transmits hands on the pdf of the vertex that sampled the direction and the distance walked since;
      what the ray then finds -- the sky, an emitter -- is weighted pdf_b / (pdf_b + p_light) with p_light taken AT THAT VERTEX: for an
      emitter p_area D^2 / |cos_l| with D the whole distance back to it.  Reflection, and solid glass, reset both: weight 1.

Light sampling here is simple and valid, not the kernels': sky texels in proportion to luminance x solid angle (SkySampler), emitter points
uniform over the emissive area, every punctual light at every vertex that is not the last (ref_lights' deterministic term).  Balance
heuristic against the BSDF strategy, which is cosine sampling for every material, as in ref_glass: under F_SPECULAR the layered value
is evaluated, never sampled.  A vertex that is not the path's last takes
both samples and weights them against its BSDF sample; the last vertex takes the sky sample alone with weight 1, and a last GLASS vertex
sends its chosen direction out as that sample (ref_glass rule 4), through any further panes.  `wrong_distance` replaces D by the last
segment alone: the mistake P2's distance rule exists to avoid, for the test that shows the cases can see it."""
import numpy as np

import ref_combined as RC
import ref_glass as RG
import ref_lens as RLE
import ref_pathtrace as RP
import ref_lights as RL
import ref_shading as R

F_NEE_SKY, F_SPECULAR, F_FACEFORWARD, F_NEE_EMISSIVE = RP.F_NEE_SKY, RP.F_SPECULAR, RP.F_FACEFORWARD, 32


class SkySampler:
    """directions with density proportional to (luminance + 1e-3 of its mean) per texel x the texel's solid angle; the density of any direction"""

    def __init__(self, sky):
        sky = np.asarray(sky, np.float64)
        self.h, self.w = sky.shape[:2]
        lum = sky @ np.array([0.299, 0.587, 0.114])
        st = np.sin(np.pi * (np.arange(self.h) + 0.5) / self.h)
        p = (lum + 1e-3 * lum.mean() + 1e-12) * st[:, None]
        self.p = (p / p.sum()).reshape(-1)

    def pdf(self, d):
        u, v = R.dir_to_equirect(d)
        ix = np.minimum((u * self.w).astype(int), self.w - 1) % self.w
        iy = np.clip((v * self.h).astype(int), 0, self.h - 1)
        st = np.sqrt(np.maximum(1e-300, 1.0 - np.asarray(d)[..., 1] ** 2))
        return self.p[iy * self.w + ix] * (self.w * self.h) / (2.0 * np.pi * np.pi * st)

    def sample(self, rng, k):
        t = rng.choice(len(self.p), size=k, p=self.p)
        u, v = (t % self.w + rng.random(k)) / self.w, (t // self.w + rng.random(k)) / self.h
        phi, el = (u - 0.5) * 2.0 * np.pi, (0.5 - v) * np.pi  # dir_to_equirect's inverse
        d = np.stack([np.cos(el) * np.cos(phi), np.sin(el), np.cos(el) * np.sin(phi)], -1)
        return d, self.pdf(d)


SEGMENT_END = 1.0 - 1e-6  # a segment to a sampled emitter point ends just short of it


def pane_table(mesh):
    """(g,) bool: the geometries that are panes -- transmission > 0, thin-walled, no normal texture"""
    t = mesh.transmission
    mt = getattr(mesh, "material_textures", None)
    no_map = np.ones(len(t), bool) if mt is None or not len(mt) else np.asarray(mt["normal_texture"]) < 0
    return (np.asarray(t["transmission"]) > 0) & (np.asarray(t["thin_walled"]) != 0) & no_map


def attenuation(tau, ior, albedo, cos_i):
    """A of one crossing, (m, 3)"""
    return (tau * (1.0 - RG.thin_fresnel(RG.fresnel(cos_i, ior))))[:, None] * albedo


def through_panes(scene, surface, glass, panes, x, d, tmax, contrib):
    """contrib (m, 3) as it arrives at the end of the segments x + t d (d unit), 0 < t < tmax: multiplied by A at every pane crossed, 0
    where anything else lies on the way"""
    tau, ior, _ = glass
    x, left, out = np.array(x, np.float64), np.array(tmax, np.float64), np.array(contrib, np.float64)
    alive = out.any(-1)
    for _ in range(64):
        idx = np.nonzero(alive)[0]
        if not len(idx):
            break
        tri, t, nrm = scene.trace(x[idx], d[idx])
        hit = (tri >= 0) & (t < left[idx])
        alive[idx[~hit]] = False
        h, th, trih, nh = idx[hit], t[hit], tri[hit], nrm[hit]
        g = scene.geom[trih]
        ip = panes[g]
        out[h[~ip]] = 0.0
        alive[h[~ip]] = False
        p = h[ip]
        if len(p):
            xp = x[p] + th[ip, None] * d[p]
            alb, _, n, _, _ = RC._materials(scene, surface, trih[ip], xp, nh[ip])
            out[p] *= attenuation(tau[g[ip]], ior[g[ip]], alb, np.abs(np.sum(n * d[p], -1)))
            left[p] -= th[ip]
            x[p] = xp
            alive[p] = out[p].any(-1)
    return out


def emitter_table(scene):
    """(triangle indices, areas, unit geometric normals) of the emissive triangles"""
    nrm = np.cross(scene.e1, scene.e2)
    area = 0.5 * np.linalg.norm(nrm, axis=1)
    em = scene.emission[scene.geom].any(-1) & (area > 0)
    idx = np.nonzero(em)[0]
    return idx, area[idx], nrm[idx] / (2.0 * area[idx, None])


def radiance_samples(scene, camera, window, flags, bounces, n, rng, *, lens, glass=None, surface=None, pane_shadows=False, panes=None,
                     lights=(), wrong_distance=False):
    """n independent path samples per pixel: (n, H, W, 3).  glass: ref_glass.table(mesh); panes: pane_table(mesh)."""
    if not pane_shadows or glass is None or panes is None or not np.any(panes & (glass[0] > 0)):
        return RG.radiance_samples(scene, camera, window, flags & ~F_NEE_EMISSIVE, bounces, n, rng, lens=lens, glass=glass, surface=surface)
    spec = bool(flags & F_SPECULAR)
    tau, ior, thin = glass
    W, H = window
    nee_sky = bool(flags & F_NEE_SKY) and scene.sky is not None
    sampler = SkySampler(scene.sky) if nee_sky else None
    e_idx, e_area, e_nrm = emitter_table(scene)
    nee_e = bool(flags & F_NEE_EMISSIVE) and len(e_idx) > 0
    p_area = 1.0 / e_area.sum() if nee_e else 0.0
    tri_is_emitter = np.zeros(len(scene.geom), bool)
    tri_is_emitter[e_idx] = True
    geo_n = np.cross(scene.e1, scene.e2)
    geo_n = geo_n / np.maximum(np.linalg.norm(geo_n, axis=1, keepdims=True), 1e-300)

    def sky(dirs):
        return R.sky_bilinear(scene.sky, *R.dir_to_equirect(dirs))

    def weight(pb, pl):  # balance weight of a BSDF-sampled direction of density pb against a light sample of density pl; inf: a delta
        return np.where(np.isinf(pb), 1.0, pb / (np.where(np.isinf(pb), 1.0, pb) + pl))

    pinv, vinv = RLE.camera_matrices(camera, window)
    py, px = np.mgrid[0:H, 0:W]
    px, py = np.tile(px.reshape(-1), n), np.tile(py.reshape(-1), n)
    m = len(px)
    x, d, _, _ = RLE.camera_sample(pinv, vinv, window, lens, px, py, rng.random((m, 4)))
    L, T = np.zeros((m, 3)), np.ones((m, 3))
    chain = np.ones(m, bool)
    tri, t, nrm = scene.trace(x, d)
    out = tri < 0
    if scene.sky is not None and out.any():
        L[out] += sky(d[out])
    live = np.nonzero(~out)[0]
    tri, nrm, d, tl = tri[live], nrm[live], d[live], t[live]
    x = x[live] + tl[:, None] * d
    pb, D = np.full(len(live), np.inf), np.zeros(len(live))  # the pdf of the vertex that sampled the direction; the distance walked before this segment
    for b in range(bounces):
        k = len(live)
        if k == 0:
            break
        last = b == bounces - 1
        alb, emi, nrm, rough, metal = RC._materials(scene, surface, tri, x, nrm)
        w_e = np.ones(k)
        if nee_e:  # an emitter the sampling vertex also sampled directly (not from the camera or a delta vertex: pb = inf gives 1)
            dist = tl if wrong_distance else D + tl
            cle = np.abs(np.sum(geo_n[tri] * d, -1))
            ps = p_area * dist * dist / np.maximum(cle, 1e-300)
            w_e = np.where(tri_is_emitter[tri] & (cle > 0), weight(pb, ps), 1.0)
        L[live] += T[live] * emi * w_e[:, None]
        g = scene.geom[tri]
        is_glass = (tau[g] > 0.0) & ((tau[g] >= 1.0) | (rng.random(k) < tau[g]))
        nf = np.where(((np.sum(nrm * d, -1) > 0.0) & bool(flags & F_FACEFORWARD))[:, None], -nrm, nrm)
        b1, b2 = RP._frame(nf)
        wo = np.stack([-np.sum(d * b1, -1), -np.sum(d * b2, -1), -np.sum(d * nf, -1)], -1)
        op = ~is_glass

        def bsdf(q, w):  # the BSDF's value (without the cosine) of the rows q towards the world directions w
            if not spec:
                return alb[q] / np.pi
            wi_l = np.stack([np.sum(w * b1[q], -1), np.sum(w * b2[q], -1), np.sum(w * nf[q], -1)], -1)
            return RLE.layered_value(alb[q], rough[q], metal[q], wo[q], wi_l)

        # ---- light samples of the opaque vertices
        if nee_sky:
            wl, pl = sampler.sample(rng, k)
            cs = np.sum(nf * wl, -1)
            use = op & (cs > 0.0)
            if use.any():
                q = np.nonzero(use)[0]
                den = pl[q] if last else pl[q] + cs[q] / np.pi
                c = T[live[q]] * bsdf(q, wl[q]) * sky(wl[q]) * (cs[q] / den)[:, None]
                L[live[q]] += through_panes(scene, surface, glass, panes, x[q], wl[q], np.full(len(q), np.inf), c)
        if nee_e and not last:
            pick = rng.choice(len(e_idx), size=k, p=e_area * p_area)
            su, u7 = np.sqrt(rng.random(k)), rng.random(k)
            et = e_idx[pick]
            pe = scene.v0[et] + scene.e1[et] * (u7 * su)[:, None] + scene.e2[et] * (su - u7 * su)[:, None]
            wv = pe - x
            dist = np.linalg.norm(wv, axis=1)
            wle = wv / np.maximum(dist, 1e-300)[:, None]
            cs, cle = np.sum(nf * wle, -1), np.abs(np.sum(e_nrm[pick] * wle, -1))
            use = op & (cs > 0.0) & (cle > 0.0) & (dist > 0.0)
            if use.any():
                q = np.nonzero(use)[0]
                ps = p_area * dist[q] ** 2 / cle[q]
                c = T[live[q]] * bsdf(q, wle[q]) * scene.emission[scene.geom[et[q]]] * (cs[q] / (ps + cs[q] / np.pi))[:, None]
                L[live[q]] += through_panes(scene, surface, glass, panes, x[q], wle[q], dist[q] * SEGMENT_END, c)
        if not last:  # punctual lights: no BSDF counterpart, no weight
            for light in lights:
                wp, dp, Ip, geo = RL.light_sample(light, x)
                cs = np.sum(nf * wp, -1)
                use = op & (cs > 0.0) & (geo > 0.0)
                if use.any():
                    q = np.nonzero(use)[0]
                    c = T[live[q]] * bsdf(q, wp[q]) * Ip[q] * (cs[q] * geo[q])[:, None]
                    L[live[q]] += through_panes(scene, surface, glass, panes, x[q], wp[q], dp[q] * SEGMENT_END, c)
        # ---- the next direction
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
            if nee_sky and is_glass.any():  # the chosen direction goes out as the sky sample, through any further panes
                q = np.nonzero(is_glass)[0]
                c = T[live[q]] * sky(d[q]) * weight(pb[q], sampler.pdf(d[q]))[:, None]
                L[live[q]] += through_panes(scene, surface, glass, panes, x[q], d[q], np.full(len(q), np.inf), c)
            break
        tri, tl, nrm = scene.trace(x, d)
        out = tri < 0
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


def chunk_sums(scene, camera, window, flags, bounces, seed, chunk, **features):
    """(sum, sum of squares) over the samples of chunk `chunk` (RP.CHUNK_SPP of them, from default_rng([seed, chunk])): (H, W, 3) each"""
    v = radiance_samples(scene, camera, window, flags, bounces, RP.CHUNK_SPP, np.random.default_rng([seed, chunk]), **features)
    return v.sum(0), (v * v).sum(0)


def render(scene, camera, window, flags, bounces, spp, seed, **features):
    """per-pixel (mean, variance) of `spp` per-sample values, spp a multiple of ref_pathtrace.CHUNK_SPP; (H, W, 3) each"""
    assert spp % RP.CHUNK_SPP == 0
    return RC.mean_var([chunk_sums(scene, camera, window, flags, bounces, seed, c, **features) for c in range(spp // RP.CHUNK_SPP)], spp)
