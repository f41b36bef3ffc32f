"""Float64 NumPy restatement of the shading math (test infrastructure): the layered GGX + diffuse BSDF, its sampling
densities, the equirect sky maps and lookups, and RGB9E5.  Written from the definitions (Walter et al. 2007 GGX, Heitz 2014
height-correlated Smith, Heitz 2018 visible-normal sampling, Schlick Fresnel), not from the fp32 code, so that a formula error
shared by the device and the oracle shows up against it.  Inputs are the fp32 values the kernels see, widened to float64; the
branch thresholds (wo.z > 1e-5, Vh.z < 0.9999, ...) compare those same values, so both sides take the same branch."""
import numpy as np

EPS32 = 2.0**-24  # unit roundoff of fp32
LUM = np.array([0.299, 0.587, 0.114])
COS_MIN = float(np.float32(1e-5))  # the grazing-view threshold of bsdf_eval, as the fp32 constant


# ------------------------------------------------------------------------------------------------ layered BSDF
class Material:
    """albedo rgb, roughness, metalness -> f0, diffuse albedo, alpha, lobe-selection probability p_spec"""

    def __init__(self, albedo, roughness, metalness):
        a = np.asarray(albedo, np.float32).astype(np.float64)
        m = float(np.float32(metalness))
        self.f0 = 0.04 + (a - 0.04) * m
        self.da = a * (1.0 - m)
        self.alpha = max(float(np.float32(roughness)), float(np.float32(0.05)))
        ls, ld = float(LUM @ self.f0), float(LUM @ self.da)
        p = ls / (ls + ld) if ls + ld > 0 else 1.0
        self.p_spec = min(max(p, 0.1), 0.9) if ld > 0 else 1.0


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def ggx_d(alpha, cos_h):
    """GGX / Trowbridge-Reitz normal distribution D(h), per unit solid angle of h"""
    a2 = alpha * alpha
    c2 = cos_h * cos_h
    return np.where(cos_h > 0, a2 / (np.pi * (c2 * (a2 - 1.0) + 1.0) ** 2), 0.0)


def smith_lambda(alpha, cos_t):
    """Smith Lambda of GGX: (-1 + sqrt(1 + alpha^2 tan^2)) / 2"""
    c2 = cos_t * cos_t
    return 0.5 * (-1.0 + np.sqrt(1.0 + alpha * alpha * (1.0 - c2) / c2))


def smith_g1(alpha, cos_t):
    return 1.0 / (1.0 + smith_lambda(alpha, cos_t))


def smith_g2(alpha, cos_o, cos_i):
    """height-correlated masking-shadowing 1 / (1 + Lambda(o) + Lambda(i))"""
    return 1.0 / (1.0 + smith_lambda(alpha, cos_o) + smith_lambda(alpha, cos_i))


def fresnel(f0, cos_d):
    """Schlick with f90 = 1; f0 (..., 3), cos_d (...)"""
    return f0 + (1.0 - f0) * (np.clip(1.0 - cos_d, 0.0, None) ** 5)[..., None]


def vndf_pdf(alpha, wo, h):
    """density of visible normals (Heitz 2018 eq. 3) per unit solid angle of h: G1(wo) max(0, wo.h) D(h) / wo.z"""
    return smith_g1(alpha, wo[..., 2]) * np.clip(np.sum(wo * h, -1), 0.0, None) * ggx_d(alpha, h[..., 2]) / wo[..., 2]


def bsdf_eval(mat, wo, wi):
    """(value rgb without the cosine, mixture pdf in projected solid angle) for arrays of tangent-frame directions"""
    wo, wi = np.broadcast_arrays(np.asarray(wo, np.float64), np.asarray(wi, np.float64))
    shape = wo.shape[:-1]
    value, pdf = np.zeros(shape + (3,)), np.zeros(shape)
    up = wi[..., 2] > 0
    diffuse_only = up & ~(wo[..., 2] > COS_MIN)
    value[diffuse_only] = mat.da / np.pi
    pdf[diffuse_only] = 1.0 / np.pi
    m = up & (wo[..., 2] > COS_MIN)
    o, i = wo[m], wi[m]
    h = _unit(o + i)
    F = fresnel(mat.f0, np.sum(i * h, -1))
    D = ggx_d(mat.alpha, h[:, 2])
    spec = smith_g2(mat.alpha, o[:, 2], i[:, 2]) * D / (4.0 * o[:, 2] * i[:, 2])
    value[m] = F * spec[:, None] + mat.da / np.pi * (1.0 - F)
    # reflection Jacobian d(omega_h) / d(omega_i) = 1 / (4 wi.h); / wi.z turns solid angle into projected solid angle
    pdf_spec = vndf_pdf(mat.alpha, o, h) / (4.0 * np.sum(i * h, -1)) / i[:, 2]
    pdf[m] = mat.p_spec * pdf_spec + (1.0 - mat.p_spec) / np.pi
    return value, pdf


def bsdf_eval_rtol(mat, wo, wi, n_ops=64):
    """Relative error bound of the fp32 evaluation: n_ops roundings of EPS32 each, plus the amplification of the rounding
    error of the half vector's h.z by D (the peak of a low-roughness lobe: d ln D / d ln cos_h = 4 cos^2 (1 - a2) / denom) and
    of 1 - wi.h by the Fresnel power (d ln (1 - c)^5 / d ln c = 5 c / (1 - c), weighted by how much of F it is)."""
    wo, wi = np.broadcast_arrays(np.asarray(wo, np.float64), np.asarray(wi, np.float64))
    h = _unit(wo + wi)
    a2 = mat.alpha**2
    c2 = h[..., 2] ** 2
    kappa_d = 4.0 * c2 * (1.0 - a2) / (c2 * (a2 - 1.0) + 1.0)
    c = np.clip(np.sum(wi * h, -1), 0.0, 1.0)
    kappa_f = 5.0 * c * (1.0 - c) ** 4  # = |d (1-c)^5 / dc| * c: absolute in F <= 1
    return EPS32 * (n_ops + 4.0 * kappa_d + 8.0 * kappa_f)


def sample_vndf_as_written(alpha, wo, u0, u1):
    """The device's sample_vndf (brdf.slang:187-216) in float64, INCLUDING its tangent choice T1 = (1, 0, 0) when Vh.z >= 0.9999
    (brdf.slang:193).  Outside that band this is Heitz 2018's exact visible-normal sampler; inside it T1 is not orthogonal to Vh and
    the half vectors do not follow vndf_pdf ("VNDF frame band").  The branch is decided on the fp32 Vh.z, as on the
    device.  Returns (h, nz): the half vectors and the disk sample's height sqrt(1 - t1^2 - t2^2)."""
    wo = np.asarray(wo, np.float64)
    u0, u1 = np.asarray(u0, np.float64), np.asarray(u1, np.float64)
    Vh = _unit(np.array([alpha * wo[0], alpha * wo[1], wo[2]]))
    v32 = np.array([np.float32(alpha) * np.float32(wo[0]), np.float32(alpha) * np.float32(wo[1]), np.float32(wo[2])], np.float32)
    vh_z32 = float(v32[2] * (np.float32(1.0) / np.sqrt(np.float32(v32 @ v32))))
    if vh_z32 < float(np.float32(0.9999)):
        T1 = _unit(np.array([-Vh[1], Vh[0], 0.0]))
    else:
        T1 = np.array([1.0, 0.0, 0.0])
    T2 = np.cross(Vh, T1)
    r = np.sqrt(u0)
    t1, t2 = r * np.cos(2 * np.pi * u1), r * np.sin(2 * np.pi * u1)
    s = 0.5 * (1.0 + Vh[2])
    t2 = (1.0 - s) * np.sqrt(1.0 - t1 * t1) + s * t2
    nz = np.sqrt(np.clip(1.0 - t1 * t1 - t2 * t2, 0.0, None))
    Nh = t1[:, None] * T1 + t2[:, None] * T2 + nz[:, None] * Vh
    h = np.stack([alpha * Nh[:, 0], alpha * Nh[:, 1], np.clip(Nh[:, 2], 0.0, None)], -1)
    return _unit(h), nz


def ggx_h_grid(alpha, n_s=384, n_phi=384):
    """Gauss-Legendre nodes over the hemisphere of h in the coordinates of GGX's own CDF: s in [0, 1) with
    tan(theta_h) = alpha sqrt(s / (1 - s)), phi in [0, 2 pi).  There D(h) cos(theta_h) d omega_h = ds dphi / (2 pi), so any
    integrand divided by D cos is smooth across the specular peak, however narrow (s = 1 - q^2 with Gauss-Legendre in q, for the
    1 / sqrt(1 - s) growth at the horizon).  Returns h (n, 3) and weights w with
    sum w g(h) / (D(h) h.z) = integral of g d omega_h."""
    xs, ws = np.polynomial.legendre.leggauss(n_s)
    xp, wp = np.polynomial.legendre.leggauss(n_phi)
    # s = 1 - q^2: near the horizon (s -> 1) the integrands grow like 1 / h.z ~ 1 / sqrt(1 - s); ds = 2 q dq takes that out
    q = 0.5 * (xs + 1.0)
    s, w_s = 1.0 - q * q, ws * q
    phi, w_p = np.pi * (xp + 1.0), np.pi * wp
    t = alpha * np.sqrt(s / (1.0 - s))
    ct = 1.0 / np.sqrt(1.0 + t * t)
    st = t * ct
    S, P = np.meshgrid(np.arange(n_s), np.arange(n_phi), indexing="ij")
    h = np.stack([st[S] * np.cos(phi[P]), st[S] * np.sin(phi[P]), ct[S]], -1).reshape(-1, 3)
    w = (w_s[S] * w_p[P] / (2.0 * np.pi)).ravel()
    return h, w


def directional_albedo(mat, wo, n=384):
    """integral of f(wo, wi) cos(theta_i) d omega_i (rgb) in float64: the specular term over the half vector (d omega_i =
    4 (wo.h) d omega_h, GGX-CDF coordinates: resolves the peak at alpha = 0.05), the diffuse term over cosine-weighted wi."""
    wo = np.asarray(wo, np.float64)
    if not wo[2] > COS_MIN:
        return mat.da.copy()
    h, w = ggx_h_grid(mat.alpha, n, n)
    oh = h @ wo
    wi = 2.0 * oh[:, None] * h - wo
    ok = (oh > 0) & (wi[:, 2] > 0)
    h, w, oh, wi = h[ok], w[ok], oh[ok], wi[ok]
    F = fresnel(mat.f0, oh)
    # f_spec cos_i 4 (wo.h) / (D cos_h) = F G2 (wo.h) / (wo.z cos_h)
    g = smith_g2(mat.alpha, wo[2], wi[:, 2]) * oh / (wo[2] * h[:, 2])
    spec = (w * g) @ F
    # diffuse: cos d omega = pi * (d a d phi / 2 pi) with wi = (sqrt(a) cos phi, sqrt(a) sin phi, sqrt(1 - a))
    xa, wa = np.polynomial.legendre.leggauss(n)
    a, w_a = 0.5 * (xa + 1.0), 0.5 * wa
    phi, w_p = np.pi * (xa + 1.0), wa / 2.0
    A, P = np.meshgrid(a, phi, indexing="ij")
    W = np.outer(w_a, w_p).ravel()
    wi = np.stack([np.sqrt(A) * np.cos(P), np.sqrt(A) * np.sin(P), np.sqrt(1.0 - A)], -1).reshape(-1, 3)
    hd = _unit(wi + wo)
    Fd = fresnel(mat.f0, np.sum(wi * hd, -1))
    diff = mat.da * (W @ (1.0 - Fd))
    return spec + diff


def vndf_moments(alpha, wo, n=384):
    """(E[h], E[h h^T] diagonal) of the ideal visible-normal distribution, float64 quadrature"""
    h, w = ggx_h_grid(alpha, n, n)
    g = w * vndf_pdf(alpha, np.broadcast_to(wo, h.shape), h) / (ggx_d(alpha, h[:, 2]) * h[:, 2])
    return g @ h, g @ (h * h), g.sum()


def vndf_bin_probs(alpha, wo, n_s, n_phi, q=8):
    """probability of each (q, phi) bin, s = 1 - q^2 in the GGX-CDF coordinates of ggx_h_grid, under the ideal visible-normal
    distribution"""
    xq, wq = np.polynomial.legendre.leggauss(q)
    probs = np.zeros((n_s, n_phi))
    for i in range(n_s):
        qq = (i + 0.5 * (xq + 1.0)) / n_s
        s = 1.0 - qq * qq
        t = alpha * np.sqrt(s / (1.0 - s))
        ct = 1.0 / np.sqrt(1.0 + t * t)
        st = t * ct
        for j in range(n_phi):
            phi = 2 * np.pi * (j + 0.5 * (xq + 1.0)) / n_phi
            h = np.stack(np.broadcast_arrays((st[:, None] * np.cos(phi)), (st[:, None] * np.sin(phi)), ct[:, None]), -1).reshape(-1, 3)
            g = vndf_pdf(alpha, np.broadcast_to(wo, h.shape), h) / (ggx_d(alpha, h[:, 2]) * h[:, 2])
            ww = (np.outer(wq * 2 * qq, wq) * 0.25 / (n_s * n_phi)).ravel()  # ds dphi / (2 pi) = 2 q dq dphi / (2 pi) over the bin
            probs[i, j] = ww @ g
    return probs


def h_to_bins(alpha, h, n_s, n_phi):
    """bin indices of half vectors in vndf_bin_probs's (q, phi) coordinates"""
    t2 = (h[:, 0] ** 2 + h[:, 1] ** 2) / (alpha * alpha * h[:, 2] ** 2)
    q = np.sqrt(1.0 / (1.0 + t2))  # sqrt(1 - s)
    phi = np.mod(np.arctan2(h[:, 1], h[:, 0]), 2 * np.pi)
    return np.clip((q * n_s).astype(np.int64), 0, n_s - 1) * n_phi + np.clip((phi / (2 * np.pi) * n_phi).astype(np.int64), 0, n_phi - 1)


# ------------------------------------------------------------------------------------------------ equirect sky
def equirect_dir(u, v):
    """math.slang's equirect map: theta = pi v from +y, phi = 2 pi u; dir = (-cos phi sin theta, cos theta, -sin phi sin theta)"""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    st = np.sin(np.pi * v)
    return np.stack([-np.cos(2 * np.pi * u) * st, np.cos(np.pi * v), -np.sin(2 * np.pi * u) * st], -1)


def dir_to_equirect(d):
    """inverse of equirect_dir (math.slang:6-12): u = 0.5 + atan2(z, x) / 2 pi, v = 0.5 - asin(y) / pi"""
    d = np.asarray(d, np.float64)
    u = 0.5 + np.arctan2(d[..., 2], d[..., 0]) / (2 * np.pi)
    v = 0.5 - np.arcsin(np.clip(d[..., 1], -1.0, 1.0)) / np.pi
    return u, v


def equirect_jacobian(v):
    """d omega / (du dv) = 2 pi^2 sin(theta), theta = pi v"""
    return 2.0 * np.pi**2 * np.sin(np.pi * np.asarray(v, np.float64))


def sky_bilinear(rgb, u, v):
    """Skybox.SampleLevel(uv, 0): bilinear over texel centres, wrap in u, clamp in v; rgb (h, w, 3) float64"""
    H, W = rgb.shape[:2]
    x = np.asarray(u, np.float64) * W - 0.5
    y = np.asarray(v, np.float64) * H - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb = np.mod(x0, W), np.mod(x0 + 1, W)
    ya, yb = np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
    top = rgb[ya, xa] * (1 - fx) + rgb[ya, xb] * fx
    bot = rgb[yb, xa] * (1 - fx) + rgb[yb, xb] * fx
    return top * (1 - fy) + bot * fy


def sky_invert(cdf, alias, u0, u1):
    """The sampler's inversion in float64: row = first y with cdf[y] > u0, stretched linearly inside the row's CDF interval;
    inside the row, alias cell k = floor(u1 W) keeps column k when frac(u1 W) < Q = (q16 + 1) / 65536, else takes its alias, and
    the fraction is stretched back to [0, 1) as the position inside the texel.  The discrete choices (k, keep) compare fp32
    values as the device does; the continuous coordinates are float64.  Returns (x, y, u, v)."""
    H, W = alias.shape
    u0f, u1f = np.asarray(u0, np.float32), np.asarray(u1, np.float32)
    y = np.searchsorted(cdf.astype(np.float64), u0f.astype(np.float64), side="right")
    lo = np.where(y > 0, cdf[np.maximum(y - 1, 0)], 0.0).astype(np.float64)
    hi = cdf[y].astype(np.float64)
    dv = np.where(hi > lo, (u0f - lo) / np.where(hi > lo, hi - lo, 1.0), 0.5)
    sx = u1f * np.float32(W)  # fp32 product, as on the device: decides the cell
    k = np.minimum(sx.astype(np.int64), W - 1)
    xi = np.minimum(sx - k.astype(np.float32), np.float32(0.99999994)).astype(np.float64)
    e = alias[y, k]
    Q = ((e & 0xFFFF).astype(np.float64) + 1.0) / 65536.0
    keep = xi < Q
    x = np.where(keep, k, (e >> 16).astype(np.int64))
    du = np.minimum(np.where(keep, xi / Q, (xi - Q) / (1.0 - Q)), float(np.float32(0.99999994)))
    return x, y, (x + du) / W, (y + dv) / H


# ------------------------------------------------------------------------------------------------ RGB9E5
def rgb9e5_encode(c):
    """packing.slang:99-144 in exact arithmetic: clamp to [0, 511/512 2^16], shared exponent from the largest channel
    (floor(log2), at least -16), 9-bit mantissas rounded half up; a maximum that rounds to 512 moves to the next exponent.
    Returns (words, ambiguous): `ambiguous` marks rows where some channel's c / 2^(e-24) lies within 2^-14 of a rounding
    midpoint, where fp32's rounding of (c / denom + 0.5) may legitimately decide the other way."""
    c = np.clip(np.asarray(c, np.float64), 0.0, 511.0 / 512.0 * 65536.0)
    mx = c.max(-1)
    # floor(log2(max)) exactly (frexp); the device reads the fp32 exponent field, which is 0 (-> -127) for a subnormal maximum:
    # both are below -16 and clamp to it, so the definitions agree
    fl2 = np.where(mx >= 2.0**-126, np.frexp(np.where(mx > 0, mx, 1.0))[1] - 1, -127).astype(np.int64)
    exp = np.maximum(fl2, -16) + 1 + 15
    denom = np.exp2(exp - 24.0)
    ratio_max = mx / denom
    maxm = np.floor(ratio_max + 0.5)
    bump = maxm == 512
    denom = np.where(bump, denom * 2, denom)
    exp = np.where(bump, exp + 1, exp)
    r = c / denom[..., None]
    m = np.floor(r + 0.5).astype(np.int64)
    frac = r - np.floor(r)
    ambiguous = (np.abs(frac - 0.5) <= 2.0**-14).any(-1) | (np.abs(ratio_max - np.floor(ratio_max) - 0.5) <= 2.0**-14)
    words = (m[..., 0] << 23) | (m[..., 1] << 14) | (m[..., 2] << 5) | exp
    return words.astype(np.uint32), ambiguous


def rgb9e5_decode(w):
    w = np.asarray(w, np.uint32).astype(np.int64)
    scale = np.exp2((w & 31) - 24.0)
    return np.stack([(w >> 23) & 511, (w >> 14) & 511, (w >> 5) & 511], -1) * scale[..., None]
