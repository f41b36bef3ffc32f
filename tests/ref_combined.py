"""Float64 NumPy path tracer with every feature at once (test infrastructure): the per-sample camera of ref_lens,
the textured surfaces of ref_materials, the punctual lights of ref_lights and the alpha cutouts of DESIGN.md section 4e, in one loop.

Written from the rendering equation like ref_pathtrace, whose estimator it is: a path of B vertices, throughput x emission at each,
cosine-distributed directions about the shading normal, the sky for a ray that leaves the scene.  What it adds is what its three parents
add, each in the parent's own words (their functions are called, not copied):

  * camera    lens = None: the pixel centre's primary hit, whose first vertex carries the G-buffer's quantisation (ref_pathtrace).
              lens = (R, F, jitter): ref_lens.camera_sample per sample; no vertex is quantised, an escaped camera ray sees the sky.
  * surface   None: per-geometry constants and the interpolated vertex normal.  surface(tri, x, normal) -> (albedo, emission, normal,
              roughness, metalness) per hit, e.g. ref_lens.textured_surface; with the pinhole camera the first vertex is that surface
              after the G-buffer's quantisation.
  * lights    at every vertex but the path's last each light adds  T f ref_lights.irradiance  unless ref_lights.occluded.
  * cutouts   a Cutouts(mesh, scene): a hit whose alpha = base_color[3] x bilinear base-colour alpha is below its geometry's cutoff does
              not exist, for the closest hit (the next-closest counts) and for occlusion alike.  Both stay brute force: every masked
              triangle is intersected on its own (a one-triangle ref_pathtrace.Scene), judged by its own alpha, and the minimum taken.

Random numbers are drawn in the parents' order -- four per camera sample first (lens only), then two per live path and vertex -- so
with one feature set switched on the samples are the parent's own (tests/test_combined_cpu.py re-renders a prefix of each fixture)."""
import copy

import numpy as np

import ref_lens as RLE
import ref_lights as RLI
import ref_pathtrace as RP
import ref_shading as R
from test_alpha_mask_cpu import tex_alpha_f64, texture_of, tri_uvs

F_NEE_SKY, F_SPECULAR, F_FACEFORWARD = RP.F_NEE_SKY, RP.F_SPECULAR, RP.F_FACEFORWARD


# ---------------------------------------------------------------------------------------------------------------- cutouts
def _subscene(scene, idx):
    """the RP.Scene of the triangles idx alone (materials stay indexed by geometry)"""
    s = copy.copy(scene)
    for name in ("p", "n", "geom", "v0", "e1", "e2"):
        setattr(s, name, getattr(scene, name)[idx])
    return s


class Plain:
    """closest hit and occlusion of an RP.Scene without cutouts"""

    def __init__(self, scene):
        self.scene = scene

    def trace(self, o, d):
        return self.scene.trace(o, d)

    def occluded(self, x, wl, dist):
        return RLI.occluded(self.scene, x, wl, dist)


class Cutouts:
    """closest hit and occlusion of `scene` = RP.Scene(mesh) (no instances: triangles are the mesh's primitives in order) under the
    mesh's alpha cutoffs"""

    def __init__(self, mesh, scene):
        self.mesh, self.scene = mesh, scene
        self.cutoff = np.asarray(mesh.alpha_cutoffs, np.float32).astype(np.float64)
        self.base_alpha = np.asarray(mesh.geometries["base_color"][:, 3], np.float32).astype(np.float64)
        masked = self.cutoff[scene.geom] > 0.0
        self.opaque_idx = np.flatnonzero(~masked)
        self.opaque = _subscene(scene, self.opaque_idx)
        self.masked_idx = np.flatnonzero(masked)
        self.singles = [_subscene(scene, np.array([k])) for k in self.masked_idx]
        self.uv = tri_uvs(mesh)[0].astype(np.float64)

    def alpha(self, tri, x):
        """alpha at the points x of the triangles tri: barycentrics from the point, the vertex uvs blended by them"""
        sc = self.scene
        w, e1, e2 = x - sc.v0[tri], sc.e1[tri], sc.e2[tri]
        d11, d12, d22 = np.sum(e1 * e1, -1), np.sum(e1 * e2, -1), np.sum(e2 * e2, -1)
        w1, w2 = np.sum(w * e1, -1), np.sum(w * e2, -1)
        den = d11 * d22 - d12 * d12
        bu, bv = (d22 * w1 - d12 * w2) / den, (d11 * w2 - d12 * w1) / den
        t = self.uv[tri]
        u = t[:, 0, 0] * (1.0 - bu - bv) + t[:, 1, 0] * bu + t[:, 2, 0] * bv
        v = t[:, 0, 1] * (1.0 - bu - bv) + t[:, 1, 1] * bu + t[:, 2, 1] * bv
        out = np.ones(len(tri))
        g = sc.geom[tri]
        for k in np.unique(g):
            s = g == k
            out[s] = self.base_alpha[k] * tex_alpha_f64(texture_of(self.mesh, k), u[s], v[s])
        return out

    def _counts(self, k, single, o, d):
        """(counts (m,) bool, t, normal) of masked triangle k for the rays o + t d"""
        tri, t, nrm = single.trace(o, d)
        hit = tri >= 0
        if hit.any():
            a = self.alpha(np.full(int(hit.sum()), k), o[hit] + t[hit, None] * d[hit])
            hit[hit] = a >= self.cutoff[self.scene.geom[k]]
        return hit, t, nrm

    def trace(self, o, d):
        tri, t, nrm = self.opaque.trace(o, d)
        tri = np.where(tri >= 0, self.opaque_idx[np.maximum(tri, 0)], -1)
        for k, single in zip(self.masked_idx, self.singles):
            hit, tk, nk = self._counts(k, single, o, d)
            better = hit & (tk < t)
            tri, t, nrm = np.where(better, k, tri), np.where(better, tk, t), np.where(better[:, None], nk, nrm)
        return tri, t, nrm

    def occluded(self, x, wl, dist):
        out = RLI.occluded(self.opaque, x, wl, dist)
        for k, single in zip(self.masked_idx, self.singles):
            hit, tk, _ = self._counts(k, single, x, wl)
            out |= hit & (tk < dist)
        return out


# ---------------------------------------------------------------------------------------------------------------- surfaces
def _materials(scene, surface, tri, x, nrm):
    """(albedo, emission, shading normal, roughness, metalness), one row per hit"""
    g = scene.geom[tri]
    if surface is None:
        return scene.albedo[g], scene.emission[g], nrm, scene.roughness[g], scene.metalness[g]
    return surface(tri, x, nrm)


def gbuffer_quantise(alb, emi, nrm, rough, metal):
    """what survives the G-buffer (ref_pathtrace.Scene's first-vertex rule, per row): 8-bit sqrt(albedo), RGB9E5 emission, the
    11-10-11 bit normal, f16 sqrt(roughness) and metalness"""
    alb0 = (np.floor(np.sqrt(np.clip(alb, 0.0, 1.0)) * 255.0 + 0.5) / 255.0) ** 2
    emi0 = R.rgb9e5_decode(R.rgb9e5_encode(np.asarray(emi, np.float64).reshape(-1, 3))[0]).reshape(np.shape(emi))
    rough0 = np.sqrt(np.asarray(rough, np.float64)).astype(np.float16).astype(np.float64) ** 2
    metal0 = np.asarray(metal, np.float64).astype(np.float16).astype(np.float64)
    return alb0, emi0, RP.gbuffer_normal(nrm), rough0, metal0


# ---------------------------------------------------------------------------------------------------------------- the tracer
def radiance_samples(scene, camera, window, flags, bounces, n, rng, *, lens=None, lights=(), surface=None, cutouts=None):
    """n independent path samples per pixel: (n, H, W, 3).  scene: RP.Scene; camera: ref_pathtrace's camera dictionary.  Without a lens
    uncovered pixels are 0."""
    W, H = window
    world = cutouts if cutouts is not None else Plain(scene)
    lights = np.atleast_1d(lights) if len(lights) else ()
    nee_sky = bool(flags & F_NEE_SKY) and scene.sky is not None

    def sky(dirs):
        return R.sky_bilinear(scene.sky, *R.dir_to_equirect(dirs))

    if lens is None:
        o0, d0 = RP.primary_rays(camera, window)
        tri0, t0, n0 = world.trace(o0, d0)
        cov = tri0 >= 0
        x0 = o0[cov] + t0[cov, None] * d0[cov]
        first = gbuffer_quantise(*_materials(scene, surface, tri0[cov], x0, n0[cov]))  # once per pixel, then one copy per sample
        first = tuple(np.tile(a, (n,) + (1,) * (a.ndim - 1)) for a in first)
        pix = np.tile(np.nonzero(cov)[0], n)
        m = len(pix)
        tri, nrm, d, x = np.tile(tri0[cov], n), first[2], np.tile(d0[cov], (n, 1)), np.tile(x0, (n, 1))
        L, T = np.zeros((m, 3)), np.ones((m, 3))
        live = np.arange(m)
    else:
        pinv, vinv = RLE.camera_matrices(camera, window)
        py, px = np.mgrid[0:H, 0:W]
        px, py = np.tile(px.reshape(-1), n), np.tile(py.reshape(-1), n)
        m = len(px)
        x, d, _, _ = RLE.camera_sample(pinv, vinv, window, lens, px, py, rng.random((m, 4)))
        L, T = np.zeros((m, 3)), np.ones((m, 3))
        tri, t, nrm = world.trace(x, d)
        out = tri < 0
        if scene.sky is not None and out.any():  # an escaped camera sample sees the sky, with or without NEE_SKY
            L[out] += sky(d[out])
        live = np.nonzero(~out)[0]
        tri, nrm, d = tri[live], nrm[live], d[live]
        x = x[live] + t[live, None] * d
        first = None
    for b in range(bounces):
        if len(live) == 0:
            break
        alb, emi, nrm, rough, metal = first if (b == 0 and first is not None) else _materials(scene, surface, tri, x, nrm)
        L[live] += T[live] * emi
        if flags & F_FACEFORWARD:
            nrm = np.where((np.sum(nrm * d, -1) > 0.0)[:, None], -nrm, nrm)
        b1, b2 = RP._frame(nrm)
        wo = np.stack([-np.sum(d * b1, -1), -np.sum(d * b2, -1), -np.sum(d * nrm, -1)], -1)

        def bsdf(wi):  # f (without the cosine) towards the tangent-frame directions wi
            if not flags & F_SPECULAR:
                return alb / np.pi
            if surface is not None:
                return RLE.layered_value(alb, rough, metal, wo, wi)
            f, g = np.zeros((len(live), 3)), scene.geom[tri]  # constants per geometry: ref_shading's own evaluation, as the parents call it
            for k in np.unique(g):
                sel = g == k
                f[sel] = R.bsdf_eval(R.Material(alb[sel][0], rough[sel][0], metal[sel][0]), wo[sel], wi[sel])[0]
            return f

        if b < bounces - 1:  # the light is the next vertex: the path's last vertex has none
            for light in lights:
                E, wl, dist = RLI.irradiance(light, x, nrm)
                lit = np.any(E > 0.0, -1)
                if lit.any():
                    lit[lit] = ~world.occluded(x[lit], wl[lit], dist[lit])
                wi = np.stack([np.sum(wl * b1, -1), np.sum(wl * b2, -1), np.maximum(np.sum(wl * nrm, -1), 1e-300)], -1)
                L[live] += np.where(lit[:, None], T[live] * bsdf(wi) * E, 0.0)
        u0, u1 = rng.random(len(live)), rng.random(len(live))
        r, phi = np.sqrt(u0), 2.0 * np.pi * u1
        wi = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u0)], -1)
        T[live] *= np.pi * bsdf(wi)
        d = wi[:, :1] * b1 + wi[:, 1:2] * b2 + wi[:, 2:] * nrm
        if b == bounces - 1 and not nee_sky:
            break  # the ray leaving the last vertex can only add sky
        tri, t, nrm = world.trace(x, d)
        out = tri < 0
        if nee_sky and out.any():
            L[live[out]] += T[live[out]] * sky(d[out])
        keep = ~out
        live, tri, nrm, d = live[keep], tri[keep], nrm[keep], d[keep]
        x = x[keep] + t[keep, None] * d
    if lens is not None:
        return L.reshape(n, H, W, 3)
    img = np.zeros((n, H * W, 3))
    img[np.repeat(np.arange(n), cov.sum()), pix] = L
    return img.reshape(n, H, W, 3)


def coverage(scene, camera, window, lens=None, cutouts=None):
    """(H, W) bool: the pixels a frame writes -- all of them through a lens, else those whose centre ray hits something"""
    W, H = window
    if lens is not None:
        return np.ones((H, W), bool)
    world = cutouts if cutouts is not None else Plain(scene)
    return (world.trace(*RP.primary_rays(camera, window))[0] >= 0).reshape(H, W)


def chunk_sums(scene, camera, window, flags, bounces, seed, chunk, **features):
    """(sum, sum of squares) over the samples of chunk `chunk` (RP.CHUNK_SPP of them, from default_rng([seed, chunk])): (H, W, 3) each"""
    v = radiance_samples(scene, camera, window, flags, bounces, RP.CHUNK_SPP, np.random.default_rng([seed, chunk]), **features)
    return v.sum(0), (v * v).sum(0)


def mean_var(sums, spp):
    """per-pixel (mean, variance) from the chunks' sums, added in chunk order"""
    s1, s2 = np.zeros_like(sums[0][0]), np.zeros_like(sums[0][0])
    for a, b in sums:
        s1 += a
        s2 += b
    mean = s1 / spp
    return mean, np.maximum(s2 / spp - mean * mean, 0.0) * (spp / (spp - 1.0))


def render(scene, camera, window, flags, bounces, spp, seed, **features):
    """per-pixel (mean, variance) of `spp` per-sample values, spp a multiple of ref_pathtrace.CHUNK_SPP; (H, W, 3) each"""
    assert spp % RP.CHUNK_SPP == 0
    return mean_var([chunk_sums(scene, camera, window, flags, bounces, seed, c, **features) for c in range(spp // RP.CHUNK_SPP)], spp)
