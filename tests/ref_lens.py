"""Float64 restatement of the per-sample camera ray and of a path whose every vertex is shaded alike (test
infrastructure).  Written from the definitions, not from lens_ray or k_lens_rays:

  * film point: (fx, fy) = (px + 1/2 + j (u0 - 1/2), py + 1/2 + j (u1 - 1/2)) in pixels, j the jitter width; in normalised device
    coordinates x = 2 fx / W - 1, y = -(2 fy / H - 1);
  * pinhole direction in view space: t = unit(xyz of proj_inverse (x, y, 1, 1));
  * focus point: Pv = t F / (-t.z), the point of that ray at view depth F;
  * lens point: l = R sqrt(u2) (cos 2 pi u3, sin 2 pi u3, 0), uniform on the disk of radius R;
  * the ray: origin view_inverse (l, 1), direction the rotation of view_inverse applied to unit(Pv - l).  With R = 0 the direction is t.

A lens path has B vertices, all of them shaded from the unquantised materials (there is no G-buffer in a lens frame); a camera ray that
escapes adds the sky's radiance whether or not NEE_SKY is set.  Everything else is ref_pathtrace's estimator."""
import numpy as np

import ref_pathtrace as RP
import ref_shading as R


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def camera_matrices(cam, window):
    """(proj_inverse, view_inverse) as 4 x 4 float64 matrices for ref_pathtrace's camera: right-handed look-at with +y up, vertical
    field of view.  proj_inverse maps (x, y, 1, 1) to a multiple of (x tan(fov / 2) W / H, y tan(fov / 2), -1)."""
    W, H = window
    pos = RP._f32(cam["position"])
    f = _unit(RP._f32(cam["direction"]))
    s = _unit(np.cross(f, [0.0, 1.0, 0.0]))
    u = np.cross(s, f)
    th = np.tan(0.5 * np.deg2rad(cam["fov_deg"]))
    vinv = np.eye(4)
    vinv[:3, 0], vinv[:3, 1], vinv[:3, 2], vinv[:3, 3] = s, u, -f, pos
    pinv = np.zeros((4, 4))
    pinv[0, 0], pinv[1, 1], pinv[2, 3], pinv[3, 2] = th * W / H, th, -1.0, 1.0
    return pinv, vinv


def gconst_matrices(g):
    """the same two matrices from a GConst block (column-major fp32), exactly"""
    return (np.array(g.proj_inverse[:], np.float32).astype(np.float64).reshape(4, 4).T,
            np.array(g.view_inverse[:], np.float32).astype(np.float64).reshape(4, 4).T)


def camera_sample(pinv, vinv, window, lens, px, py, u):
    """lens = (R, F, jitter); px, py (n,) pixel coordinates; u (n, 4) uniforms.  Returns o, d (world), film (n, 2) in pixels, lens
    point (n, 2) in view space."""
    W, H = window
    Rl, F, j = (float(x) for x in lens)
    px, py, u = np.asarray(px, np.float64), np.asarray(py, np.float64), np.asarray(u, np.float64)
    film = np.stack([px + 0.5 + j * (u[:, 0] - 0.5), py + 0.5 + j * (u[:, 1] - 0.5)], -1)
    x, y = 2.0 * film[:, 0] / W - 1.0, -(2.0 * film[:, 1] / H - 1.0)
    clip = np.stack([x, y, np.ones_like(x), np.ones_like(x)], -1)
    t = _unit((clip @ pinv.T)[:, :3])
    if Rl > 0.0:
        r, phi = Rl * np.sqrt(u[:, 2]), 2.0 * np.pi * u[:, 3]
        l = np.stack([r * np.cos(phi), r * np.sin(phi), np.zeros_like(r)], -1)
        dv = _unit(t * (F / -t[:, 2])[:, None] - l)
    else:
        l, dv = np.zeros_like(t), t
    o = l @ vinv[:3, :3].T + vinv[:3, 3]
    d = dv @ vinv[:3, :3].T
    return o, d, film, l[:, :2]


def focus_point(pinv, vinv, window, F, px, py):
    """world-space point the rays of pixel (px, py) share when the jitter is 0"""
    o, d, _, _ = camera_sample(pinv, vinv, window, (0.0, F, 0.0), np.atleast_1d(px), np.atleast_1d(py), np.zeros((np.size(px), 4)))
    depth = -(d @ vinv[:3, 2])  # view depth per unit of ray length
    return o + d * (F / depth)[:, None]


def layered_value(albedo, roughness, metalness, wo, wi):
    """ref_shading.bsdf_eval's value (rgb, without the cosine) with one material per row: f0 = lerp(0.04, albedo, metalness), diffuse
    albedo (1 - metalness), alpha = max(roughness, 0.05); GGX D, height-correlated Smith G2 and Schlick F are ref_shading's"""
    f0 = 0.04 + (albedo - 0.04) * metalness[:, None]
    da = albedo * (1.0 - metalness)[:, None]
    alpha = np.maximum(roughness, float(np.float32(0.05)))
    value = np.zeros_like(albedo)
    up, view = wi[:, 2] > 0, wo[:, 2] > R.COS_MIN
    value[up & ~view] = da[up & ~view] / np.pi
    m = up & view
    o, i = wo[m], wi[m]
    h = _unit(o + i)
    F = R.fresnel(f0[m], np.sum(i * h, -1))
    spec = R.smith_g2(alpha[m], o[:, 2], i[:, 2]) * R.ggx_d(alpha[m], h[:, 2]) / (4.0 * o[:, 2] * i[:, 2])
    value[m] = F * spec[:, None] + da[m] / np.pi * (1.0 - F)
    return value


def textured_surface(mesh, scene):
    """a `surface` for radiance_samples: the float64 surfaces of tests/ref_materials.py (material textures, base-colour textures) at the
    hits of `scene` = ref_pathtrace.Scene(mesh), whose triangles are the flattened primitives in order"""
    import ref_materials as RM

    def surface(tri, x, nrm):
        w, e1, e2 = x - scene.v0[tri], scene.e1[tri], scene.e2[tri]
        d11, d12, d22 = np.sum(e1 * e1, -1), np.sum(e1 * e2, -1), np.sum(e2 * e2, -1)
        w1, w2 = np.sum(w * e1, -1), np.sum(w * e2, -1)
        den = d11 * d22 - d12 * d12
        bu, bv = np.clip((d22 * w1 - d12 * w2) / den, 0.0, 1.0), np.clip((d11 * w2 - d12 * w1) / den, 0.0, 1.0)
        s = np.maximum(bu + bv, 1.0) * (1.0 + 1e-6)  # ref_materials takes fp32 barycentrics inside the triangle
        m = RM.reference(mesh, None, tri, bu / s, bv / s)
        return m.base.albedo, m.emissive, m.normal, np.asarray(m.roughness, np.float64), np.asarray(m.metalness, np.float64)

    return surface


def radiance_samples(scene, pinv, vinv, window, lens, flags, bounces, n, rng, surface=None):
    """n independent lens-path samples per pixel: (n, H, W, 3).  `surface(tri, x, normal)` -> (albedo, emission, shading normal,
    roughness, metalness) per hit replaces the scene's per-geometry constants and interpolated vertex normal (textured_surface)."""
    W, H = window
    py, px = np.mgrid[0:H, 0:W]
    px, py = np.tile(px.reshape(-1), n), np.tile(py.reshape(-1), n)
    m = len(px)
    x, d, _, _ = camera_sample(pinv, vinv, window, lens, px, py, rng.random((m, 4)))
    L, T = np.zeros((m, 3)), np.ones((m, 3))
    tri, t, nrm = scene.trace(x, d)
    out = tri < 0
    if scene.sky is not None and out.any():  # an escaped camera sample sees the sky, with or without NEE_SKY
        uu, vv = R.dir_to_equirect(d[out])
        L[out] += R.sky_bilinear(scene.sky, uu, vv)
    live = np.nonzero(~out)[0]
    tri, nrm, d = tri[live], nrm[live], d[live]
    x = x[live] + t[live, None] * d
    nee_sky = bool(flags & RP.F_NEE_SKY) and scene.sky is not None
    for b in range(bounces):
        if len(live) == 0:
            break
        g = scene.geom[tri]
        alb, emi = scene.albedo[g], scene.emission[g]
        if surface is not None:
            alb, emi, nrm, rough, metal = surface(tri, x, nrm)
        L[live] += T[live] * emi
        if flags & RP.F_FACEFORWARD:
            nrm = np.where((np.sum(nrm * d, -1) > 0.0)[:, None], -nrm, nrm)
        b1, b2 = RP._frame(nrm)
        u0, u1 = rng.random(len(live)), rng.random(len(live))
        r, phi = np.sqrt(u0), 2.0 * np.pi * u1
        wi = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u0)], -1)
        if flags & RP.F_SPECULAR:
            wo = np.stack([-np.sum(d * b1, -1), -np.sum(d * b2, -1), -np.sum(d * nrm, -1)], -1)
            weight = np.zeros((len(live), 3))
            if surface is not None:
                weight = np.pi * layered_value(alb, rough, metal, wo, wi)
            for k in np.unique(g) if surface is None else ():
                sel = g == k
                weight[sel] = np.pi * R.bsdf_eval(R.Material(scene.albedo[k], scene.roughness[k], scene.metalness[k]), wo[sel], wi[sel])[0]
        else:
            weight = alb
        T[live] *= weight
        d = wi[:, :1] * b1 + wi[:, 1:2] * b2 + wi[:, 2:] * nrm
        if b == bounces - 1 and not nee_sky:
            break  # the ray leaving the last vertex can only add sky
        tri, t, nrm = scene.trace(x, d)
        out = tri < 0
        if nee_sky and out.any():
            uu, vv = R.dir_to_equirect(d[out])
            L[live[out]] += T[live[out]] * R.sky_bilinear(scene.sky, uu, vv)
        keep = ~out
        live, tri, nrm, d = live[keep], tri[keep], nrm[keep], d[keep]
        x = x[keep] + t[keep, None] * d
    return L.reshape(n, H, W, 3)


def render(scene, pinv, vinv, window, lens, flags, bounces, spp, seed, surface=None):
    """per-pixel (mean, variance) of `spp` per-sample values, spp a multiple of ref_pathtrace.CHUNK_SPP; (H, W, 3) each"""
    assert spp % RP.CHUNK_SPP == 0
    W, H = window
    s1, s2 = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    for c in range(spp // RP.CHUNK_SPP):
        v = radiance_samples(scene, pinv, vinv, window, lens, flags, bounces, RP.CHUNK_SPP, np.random.default_rng([seed, c]), surface)
        s1 += v.sum(0)
        s2 += (v * v).sum(0)
    mean = s1 / spp
    return mean, np.maximum(s2 / spp - mean * mean, 0.0) * (spp / (spp - 1.0))


# ---------------------------------------------------------------------------------------------------------------- closed forms
def interval_overlap(lo, hi, a, b):
    """length of [lo, hi] n [a, b], elementwise"""
    return np.clip(np.minimum(hi, b) - np.maximum(lo, a), 0.0, None)


def box_coverage(x0, x1, y0, y1, window, jitter=1.0):
    """(H, W): the share of each pixel's jitter box (width `jitter`, centred in the pixel) inside the rectangle [x0, x1] x [y0, y1]
    given in pixel coordinates"""
    W, H = window
    cx, cy = np.arange(W) + 0.5, np.arange(H) + 0.5
    ox = interval_overlap(cx - 0.5 * jitter, cx + 0.5 * jitter, x0, x1) / jitter
    oy = interval_overlap(cy - 0.5 * jitter, cy + 0.5 * jitter, y0, y1) / jitter
    return oy[:, None] * ox[None, :]


def polygon_area(p):
    x, y = p[:, 0], p[:, 1]
    return 0.5 * abs(float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)))


def clip_polygon(p, a, b, c):
    """Sutherland-Hodgman: the part of the convex polygon p (k, 2) with a x + b y <= c"""
    out = []
    k = len(p)
    for i in range(k):
        s, e = p[i], p[(i + 1) % k]
        ds, de = a * s[0] + b * s[1] - c, a * e[0] + b * e[1] - c
        if ds <= 0.0:
            out.append(s)
        if (ds < 0.0 < de) or (de < 0.0 < ds):
            out.append(s + (e - s) * (ds / (ds - de)))
    return np.array(out).reshape(-1, 2)


def polygon_coverage(poly, window, jitter=1.0):
    """(H, W): the share of each pixel's jitter box inside the convex polygon (k, 2), pixel coordinates"""
    W, H = window
    cov = np.zeros((H, W))
    h = 0.5 * jitter
    for y in range(H):
        for x in range(W):
            q = np.asarray(poly, np.float64)
            for a, b, c in ((1, 0, x + 0.5 + h), (-1, 0, -(x + 0.5 - h)), (0, 1, y + 0.5 + h), (0, -1, -(y + 0.5 - h))):
                if len(q) >= 3:
                    q = clip_polygon(q, a, b, c)
            cov[y, x] = polygon_area(q) / jitter**2 if len(q) >= 3 else 0.0
    return cov


def disk_edge_G(s, r):
    """antiderivative of the edge response of a uniform disk of radius r (pixels): G' = the share of the disk centred at distance s
    inside the lit half-plane.  G = 0 for s <= -r, s for s >= r."""
    s = np.asarray(s, np.float64)
    if r <= 0.0:
        return np.maximum(s, 0.0)
    sc = np.clip(s, -r, r)
    q = np.sqrt(np.maximum(r * r - sc * sc, 0.0))
    mid = sc / 2.0 + (r * r * (sc * np.arcsin(sc / r) + q) - q**3 / 3.0) / (np.pi * r * r)
    return np.where(s <= -r, 0.0, np.where(s >= r, s, mid))


def half_plane_columns(e, r, W):
    """(W,): the share of pixel column x's samples that see the half-plane whose edge the pinhole shows at pixel coordinate e, under a
    circle of confusion of r pixels: the pixel box integrated exactly, G(x + 1 - e) - G(x - e) (kept in [0, 1] against the rounding of
    the difference)"""
    x = np.arange(W)
    return np.clip(disk_edge_G(x + 1.0 - e, r) - disk_edge_G(x - e, r), 0.0, 1.0)


def coc_radius_px(R_lens, F, z, fov_deg, H):
    """radius of the circle of confusion of a point at view depth z, in pixels"""
    return R_lens * abs(1.0 / F - 1.0 / z) * H / (2.0 * np.tan(0.5 * np.deg2rad(fov_deg)))
