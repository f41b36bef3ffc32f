"""Float64 NumPy path tracer (test infrastructure): a second witness for the integrator as a whole.

Written from the rendering equation  L(x, wo) = Le(x) + integral f(x, wo, wi) L(x', -wi) cos(theta_i) d wi,  not from the oracle's
refmode_body or the device's k_shade, so that an estimator error the two share (where emission is collected, throughput, the number of
path vertices, MIS weights) shows up against it.  It is the simplest estimator of the integral the kernels estimate:

  * a path has B vertices; the first is the pixel centre's primary hit;
  * every vertex adds throughput x emission (surfaces emit on both sides, EMISSION_SCALE x the material's emission);
  * the next direction is cosine-distributed about the shading normal (pdf cos / pi), so the throughput factor is f pi: the albedo
    without SPECULAR, ref_shading.bsdf_eval's layered value x pi with it;
  * a ray that leaves the scene adds throughput x sky radiance when NEE_SKY is set (without it the kernels never see the sky) and the
    path ends.  That also holds for the ray leaving vertex B: the kernels' light sample has weight 1 there, which is the same integral;
  * no light sampling, no MIS, no Russian roulette.

Scene conventions restated from their definitions: intersections are valid for t > T_MIN; the sky is the equirect map of ref_shading,
bilinear over the RGB9E5-decoded texels; the first vertex carries the G-buffer's quantisation (8-bit sqrt(albedo), 11-10-11 bit
normal, f16 sqrt(roughness) and metalness, RGB9E5 emission); FACEFORWARD flips a shading normal that faces away from the viewer, and
without the flag nothing is flipped.

Random numbers: numpy.random.default_rng([seed, chunk]) per chunk of CHUNK_SPP samples, so the first chunks of a long run are the
whole of a short one."""
import numpy as np

import ref_shading as R

F_NEE_SKY, F_SPECULAR, F_FACEFORWARD = 1, 4, 8
T_MIN = 1e-3
EMISSION_SCALE = 12.0
CHUNK_SPP = 64


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


class Scene:
    """triangles in world space (float64, from the fp32 vertices), vertex normals, one material per triangle"""

    def __init__(self, mesh, instances=None, sky=None):
        g = mesh.geometries
        P, N, G = [], [], []
        for first, count, m in instances or [(0, len(g), np.eye(4))]:
            m = _f32(m)
            nm = np.linalg.inv(m[:3, :3]).T  # normals transform by the inverse transpose
            for k in range(first, first + count):
                io, vo, cnt = int(g["index_offset"][k]), int(g["vertex_offset"][k]), int(mesh.prim_counts[k])
                idx = mesh.indices[io:io + 3 * cnt].astype(np.int64).reshape(-1, 3) + vo
                v = mesh.vertices[idx].astype(np.float64)  # (cnt, 3, 8)
                P.append(v[..., :3] @ m[:3, :3].T + m[:3, 3])
                N.append(_unit(v[..., 3:6] @ nm.T))
                G.append(np.full(cnt, k))
        self.p, self.n, self.geom = np.concatenate(P), np.concatenate(N), np.concatenate(G)
        self.v0, self.e1, self.e2 = self.p[:, 0], self.p[:, 1] - self.p[:, 0], self.p[:, 2] - self.p[:, 0]
        self.albedo = _f32(g["base_color"][:, :3])
        self.emission = EMISSION_SCALE * _f32(g["emission"][:, :3])
        self.roughness, self.metalness = _f32(g["roughness"]), _f32(g["metallic_factor"])
        # the first vertex's materials: what survives the G-buffer
        self.albedo0 = (np.floor(np.sqrt(np.clip(self.albedo, 0.0, 1.0)) * 255.0 + 0.5) / 255.0) ** 2
        self.emission0 = R.rgb9e5_decode(R.rgb9e5_encode(self.emission)[0])
        self.roughness0 = np.sqrt(self.roughness).astype(np.float16).astype(np.float64) ** 2
        self.metalness0 = self.metalness.astype(np.float16).astype(np.float64)
        self.sky = None if sky is None else R.rgb9e5_decode(R.rgb9e5_encode(np.asarray(sky, np.float64).reshape(-1, 3))[0]).reshape(np.shape(sky))

    def trace(self, o, d, chunk=32768):
        """closest hit with t > T_MIN by Moeller-Trumbore over every triangle: (triangle or -1, t, shading normal)"""
        n = len(o)
        tri, t, nrm = np.full(n, -1, np.int64), np.full(n, np.inf), np.zeros((n, 3))
        for a in range(0, n, chunk):
            oo, dd = o[a:a + chunk, None, :], d[a:a + chunk, None, :]
            pv = np.cross(dd, self.e2[None])
            det = np.sum(self.e1[None] * pv, -1)
            ok = det != 0.0
            inv = 1.0 / np.where(ok, det, 1.0)
            tv = oo - self.v0[None]
            u = np.sum(tv * pv, -1) * inv
            qv = np.cross(tv, self.e1[None])
            v = np.sum(dd * qv, -1) * inv
            tt = np.sum(self.e2[None] * qv, -1) * inv
            ok &= (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0) & (tt > T_MIN)
            tt = np.where(ok, tt, np.inf)
            k = np.argmin(tt, axis=1)
            r = np.arange(len(k))
            best = tt[r, k]
            hit = np.isfinite(best)
            bu, bv = u[r, k][:, None], v[r, k][:, None]
            nn = self.n[k, 0] * (1.0 - bu - bv) + self.n[k, 1] * bu + self.n[k, 2] * bv
            tri[a:a + chunk] = np.where(hit, k, -1)
            t[a:a + chunk] = best
            nrm[a:a + chunk] = _unit(np.where(hit[:, None], nn, [0.0, 0.0, 1.0]))
        return tri, t, nrm


def primary_rays(cam, window):
    """pinhole camera through the pixel centres: right-handed look-at with +y up, vertical field of view, row 0 on top"""
    W, H = window
    pos = _f32(cam["position"])
    f = _unit(_f32(cam["direction"]))
    s = _unit(np.cross(f, [0.0, 1.0, 0.0]))
    u = np.cross(s, f)
    th = np.tan(0.5 * np.deg2rad(cam["fov_deg"]))
    py, px = np.mgrid[0:H, 0:W]
    x = ((px + 0.5) / W * 2.0 - 1.0) * th * (W / H)
    y = -((py + 0.5) / H * 2.0 - 1.0) * th
    d = _unit(f + x[..., None] * s + y[..., None] * u).reshape(-1, 3)
    return np.broadcast_to(pos, d.shape).copy(), d


def gbuffer_normal(n):
    """the 11-10-11 bit unorm normal of the G-buffer, decoded and renormalised"""
    top = np.array([2047.0, 1023.0, 2047.0])
    q = np.floor(np.clip(n * 0.5 + 0.5, 0.0, 1.0) * top + 0.5)
    return _unit(q / top * 2.0 - 1.0)


def _frame(n):
    a = np.where((np.abs(n[:, 0]) > 0.9)[:, None], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0])
    b1 = _unit(np.cross(a, n))
    return b1, np.cross(n, b1)


def radiance_samples(scene, cam, window, flags, bounces, n, rng):
    """n independent path samples per pixel: (n, H, W, 3); uncovered pixels are 0"""
    W, H = window
    o0, d0 = primary_rays(cam, window)
    tri0, t0, n0 = scene.trace(o0, d0)
    cov = tri0 >= 0
    pix = np.tile(np.nonzero(cov)[0], n)
    m = len(pix)
    tri, nrm = np.tile(tri0[cov], n), np.tile(gbuffer_normal(n0[cov]), (n, 1))
    d = np.tile(d0[cov], (n, 1))
    x = np.tile(o0[cov] + t0[cov, None] * d0[cov], (n, 1))
    L, T = np.zeros((m, 3)), np.ones((m, 3))
    live = np.arange(m)  # indices into L / T of the paths still going; tri, nrm, d, x are per live path
    for b in range(bounces):
        first = b == 0
        g = scene.geom[tri]
        alb = (scene.albedo0 if first else scene.albedo)[g]
        L[live] += T[live] * (scene.emission0 if first else scene.emission)[g]
        if flags & F_FACEFORWARD:
            nrm = np.where((np.sum(nrm * d, -1) > 0.0)[:, None], -nrm, nrm)
        b1, b2 = _frame(nrm)
        u0, u1 = rng.random(len(live)), rng.random(len(live))
        r, phi = np.sqrt(u0), 2.0 * np.pi * u1
        wi = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u0)], -1)
        if flags & F_SPECULAR:
            wo = np.stack([-np.sum(d * b1, -1), -np.sum(d * b2, -1), -np.sum(d * nrm, -1)], -1)
            weight = np.zeros((len(live), 3))
            rough, metal = (scene.roughness0, scene.metalness0) if first else (scene.roughness, scene.metalness)
            for k in np.unique(g):
                sel = g == k
                mat = R.Material(alb[sel][0], rough[k], metal[k])
                weight[sel] = np.pi * R.bsdf_eval(mat, wo[sel], wi[sel])[0]
        else:
            weight = alb
        T[live] *= weight
        d = wi[:, :1] * b1 + wi[:, 1:2] * b2 + wi[:, 2:] * nrm
        if b == bounces - 1 and not (flags & F_NEE_SKY and scene.sky is not None):
            break  # the ray leaving the last vertex can only add sky
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


def coverage(scene, cam, window):
    W, H = window
    return (scene.trace(*primary_rays(cam, window))[0] >= 0).reshape(H, W)


def render(scene, cam, window, flags, bounces, spp, seed):
    """per-pixel (mean, variance) of `spp` per-sample values, spp a multiple of CHUNK_SPP; (H, W, 3) each"""
    assert spp % CHUNK_SPP == 0
    W, H = window
    s1, s2 = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    for c in range(spp // CHUNK_SPP):
        v = radiance_samples(scene, cam, window, flags, bounces, CHUNK_SPP, np.random.default_rng([seed, c]))
        s1 += v.sum(0)
        s2 += (v * v).sum(0)
    mean = s1 / spp
    return mean, np.maximum(s2 / spp - mean * mean, 0.0) * (spp / (spp - 1.0))


def block_stats(mean, var, spp, block=16):
    """(block means, their standard errors) per block x block tile and channel: pixels are independent, so the variance of a block mean
    is the sum of the pixel-mean variances over block^4"""
    H, W, C = mean.shape
    bm = mean.reshape(H // block, block, W // block, block, C).mean((1, 3))
    bv = (var / spp).reshape(H // block, block, W // block, block, C).sum((1, 3)) / block**4
    return bm, np.sqrt(bv)
