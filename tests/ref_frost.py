"""Float64 NumPy restatement of rough transmission (test infrastructure) on top of tests/ref_glass.py: the vertex rule
of rt3_scene_set_rough_transmission (include/rt3.h), ref_glass's estimator with glass_event replaced on frosted geometry, and the answers and
rounding bounds of self-test op 38.

The rule (frost_event): frame about n_in = the shading normal on the incoming side, by the device's own tangent-frame construction (the
micro-normal's azimuth is counted in that frame, so any other frame is another sample); m = the opaque BSDF's sample_vndf as written,
with its tangent choice T1 = (1, 0, 0) from Vh.z >= 0.9999 on; Fresnel at cos_i = wo.m by ref_glass's expressions; reflection
2 cos_i m - wo, solid transmission -wo / eta + (cos_i / eta - cos_t) m, thin-walled transmission the reflection mirrored through the
macro-surface; a sample on the wrong side ends the path; weight G1(|wi.z|, alpha^2).  alpha = 0 is ref_glass.glass_event with weight 1.

`rule` evaluates the same text in the arithmetic of a dtype: float64 is the reference, float32 the model of the device's roundings that
tests/test_frost_cpu.py holds the derived bounds against."""
import numpy as np

import ref_combined as RC
import ref_glass as RG
import ref_lens as RLE
import ref_pathtrace as RP
import ref_shading as R

F_NEE_SKY, F_SPECULAR, F_FACEFORWARD = RP.F_NEE_SKY, RP.F_SPECULAR, RP.F_FACEFORWARD
MIN_COS = float(np.float32(1e-5))       # kFrostMinCos, as the fp32 constant
VNDF_BAND = float(np.float32(0.9999))   # sample_vndf's tangent switch
REFLECT, TRANSMIT, INVALID = 0, 1, 2
U24 = 2.0**-24


# ---------------------------------------------------------------------------------------------------------------- the rule
def _sincos_2pi(f, u):
    """float64: sin and cos of 2 pi u; float32: the device's quadrant split and Taylor polynomials (rt3_math.hpp)"""
    if f == np.float64:
        return np.sin(2.0 * np.pi * u), np.cos(2.0 * np.pi * u)
    x = u * f(4.0)
    q = x.astype(np.int32)
    r = x - q.astype(f)
    sw = r > f(0.5)
    r = np.where(sw, f(1.0) - r, r)
    a = r * f(1.57079632679489661923)
    a2 = a * a
    s = a * (f(1.0) + a2 * (f(-1.6666667163e-01) + a2 * (f(8.3333337680e-03) + a2 * (f(-1.9841270114e-04) + a2 * f(2.7557314297e-06)))))
    c = f(1.0) + a2 * (f(-0.5) + a2 * (f(4.1666667908e-02) + a2 * (f(-1.3888889225e-03) + a2 * (f(2.4801587642e-05) + a2 * f(-2.7557314297e-07)))))
    ss, cc = np.where(sw, c, s), np.where(sw, s, c)
    q = q & 3
    return np.select([q == 0, q == 1, q == 2], [ss, cc, -ss], -cc), np.select([q == 0, q == 1, q == 2], [cc, -ss, -cc], ss)


def _basis(f, n):
    """build_orthonormal_basis (rt3_math.hpp): (b1, b2) of rows n"""
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    neg = z < 0
    a = f(1.0) / np.where(neg, f(1.0) - z, f(1.0) + z)
    b = np.where(neg, x * y * a, -x * y * a)
    b1 = np.stack([f(1.0) - x * x * a, np.where(neg, -b, b), np.where(neg, x, -x)], -1)
    b2 = np.stack([b, np.where(neg, y * y * a - f(1.0), f(1.0) - y * y * a), -y], -1)
    return b1, b2


def _unit(v):
    return v * (v.dtype.type(1.0) / np.sqrt(np.sum(v * v, -1)))[:, None]


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def sample_vndf(f, alpha, wo, u0, u1):
    """rt3_bsdf.hpp: sample_vndf, rows; returns (m, the intermediate values the bounds of op38_reference are made of)"""
    Vh = _unit(np.stack([alpha * wo[:, 0], alpha * wo[:, 1], wo[:, 2]], -1))
    band = ~(Vh[:, 2] < f(VNDF_BAND))
    s = np.sqrt(Vh[:, 0] * Vh[:, 0] + Vh[:, 1] * Vh[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        T1 = np.stack([-Vh[:, 1], Vh[:, 0], np.zeros_like(s)], -1) * (f(1.0) / s)[:, None]
    T1 = np.where(band[:, None], np.array([1.0, 0.0, 0.0], f), T1)
    T2 = np.cross(Vh, T1).astype(f)
    r = np.sqrt(u0)
    sp, cp = _sincos_2pi(f, u1)
    t1, t2p, sv = r * cp, r * sp, f(0.5) * (f(1.0) + Vh[:, 2])
    root = np.sqrt(f(1.0) - t1 * t1)
    t2 = (f(1.0) - sv) * root + sv * t2p
    q = f(1.0) - t1 * t1 - t2 * t2
    nz = np.sqrt(np.maximum(f(0.0), q))
    Nh = t1[:, None] * T1 + t2[:, None] * T2 + nz[:, None] * Vh
    pre = np.stack([alpha * Nh[:, 0], alpha * Nh[:, 1], np.maximum(f(0.0), Nh[:, 2])], -1)
    return _unit(pre), dict(Vh=Vh, band=band, s=s, t1=t1, t2p=t2p, t2=t2, sv=sv, root=root, q=q, nz=nz, Nh=Nh, pre=pre)


def g1(f, c, a2):
    """g_smith_ggx1 (rt3_bsdf.hpp)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return f(2.0) / (f(1.0) + np.sqrt(f(1.0) + a2 * ((f(1.0) - c * c) / (c * c))))


def rule(f, ior, thin, d, n, alpha, u, u2, u3):
    """frost_sample (rt3_glass.hpp) for rows with alpha > 0, in the arithmetic of dtype f and the device's order of operations.  Returns a
    dict: event, dir (world), F, weight, and the intermediate values of the frame, the micro-normal and the event."""
    f = np.dtype(f).type
    ior, alpha, u, u2, u3 = (np.asarray(a, f) for a in (ior, alpha, u, u2, u3))
    d, n = np.asarray(d, f), np.asarray(n, f)
    thin = np.asarray(thin) != 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ud = d / np.sqrt(_dot(d, d))[:, None]
        enter = _dot(n, ud) < 0
        n_in = np.where(enter[:, None], n, -n)
        b1, b2 = _basis(f, n_in)
        wo = np.stack([-_dot(ud, b1), -_dot(ud, b2), -_dot(ud, n_in)], -1)
        frame_ok = wo[:, 2] > f(MIN_COS)
        m, mid = sample_vndf(f, alpha, wo, u2, u3)
        cos_i = _dot(wo, m)
        eta = np.where(thin | enter, ior, f(1.0) / ior)
        eta2 = eta * eta
        ct2 = (cos_i * cos_i + (eta2 - f(1.0))) / eta2
        tir = ~(ct2 > 0)
        ct = np.where(tir, f(0.0), np.sqrt(np.where(tir, f(1.0), ct2)))
        rs = (cos_i - eta * ct) / (cos_i + eta * ct)
        rp = (eta * cos_i - ct) / (eta * cos_i + ct)
        F = np.where(tir, f(1.0), f(0.5) * (rs * rs + rp * rp))
        F = np.where(thin, (f(2.0) * F) / (f(1.0) + F), F)
        refl = (f(2.0) * cos_i)[:, None] * m - wo
        k = cos_i / eta - ct
        refr = k[:, None] * m - wo / eta[:, None]
        reflect = u < F
        mirrored = refl * np.array([1.0, 1.0, -1.0], f)
        wi = np.where(reflect[:, None], refl, np.where(thin[:, None], mirrored, refr))
        # the tested height: the reflection's for reflection and the thin wall, minus the refracted direction's otherwise
        height = np.where(reflect | thin, refl[:, 2], -refr[:, 2])
        ok = frame_ok & (height > f(MIN_COS))
        world = wi[:, :1] * b1 + wi[:, 1:2] * b2 + wi[:, 2:] * n_in
        weight = g1(f, np.abs(wi[:, 2]), alpha * alpha)
    event = np.where(ok, np.where(reflect, REFLECT, TRANSMIT), INVALID)
    out = dict(event=event, dir=np.where(ok[:, None], world, ud), F=np.where(frame_ok, F, f(0.0)), weight=np.where(ok, weight, f(0.0)), ud=ud, wo=wo,
               frame_ok=frame_ok, m=m, cos_i=cos_i, eta=eta, ct2=ct2, tir=tir, ct=ct, rs=rs, rp=rp, F0=np.where(tir, f(1.0), f(0.5) * (rs * rs + rp * rp)),
               k=k, refl=refl, refr=refr, wi=wi, height=height, reflect=reflect, thin=thin)
    out.update(mid)
    return out


def frost_event(ior, thin, d, n, alpha, u, u2, u3):
    """(event (m,) int: 0 reflect / 1 transmit / 2 invalid, direction (m, 3), reflection probability (m,), weight (m,)) of rays d at
    shading normals n with roughness alpha; a row with alpha = 0 is ref_glass.glass_event with weight 1"""
    d = np.asarray(d, np.float64)
    k = len(d)
    ior, thin, alpha, u, u2, u3 = (np.broadcast_to(np.asarray(a), (k,)) for a in (ior, thin, alpha, u, u2, u3))
    alpha = np.asarray(alpha, np.float64)
    rough = alpha > 0.0
    tr, gdir, gF = RG.glass_event(ior, thin, d, n, u)
    if not rough.any():
        return tr.astype(np.int64), gdir, gF, np.ones(k)
    r = rule(np.float64, ior, thin, d, n, np.where(rough, alpha, 1.0), u, u2, u3)
    return (np.where(rough, r["event"], tr.astype(np.int64)), np.where(rough[:, None], r["dir"], gdir), np.where(rough, r["F"], gF),
            np.where(rough, r["weight"], 1.0))


def frosted(mesh, on=True):
    """the build's classification, per geometry: mode on, transmission > 0, and a roughness factor > 0 or a metallic-roughness texture"""
    tex = np.asarray(mesh.material_textures["metallic_roughness_texture"]) >= 0
    return bool(on) & (np.asarray(mesh.transmission["transmission"]) > 0) & ((np.asarray(mesh.geometries["roughness"]) > 0) | tex)


# ---------------------------------------------------------------------------------------------------------------- the tracer
def radiance_samples(scene, camera, window, flags, bounces, n, rng, *, lens, glass=None, frost=None, surface=None):
    """ref_glass.radiance_samples with the frost rule on the geometries of `frost` (bool per geometry; none: ref_glass itself, called).
    Random numbers per vertex, for every live path: ref_glass's four, then the micro-normal's two."""
    if glass is None or frost is None or not np.any(frost & (glass[0] > 0.0)):
        return RG.radiance_samples(scene, camera, window, flags, bounces, n, rng, lens=lens, glass=glass, surface=surface)
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
    tri, t, nrm = scene.trace(x, d)
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
        ue, u2, u3 = rng.random(k), rng.random(k), rng.random(k)
        alpha = np.where(frost[g], np.broadcast_to(rough, (k,)), 0.0)
        event, d_glass, _, weight = frost_event(ior[g], thin[g], d, nrm, alpha, ue, u2, u3)
        T[live] *= np.where(is_glass[:, None], np.where((event == TRANSMIT)[:, None], alb, 1.0) * weight[:, None], np.pi * f)
        d = np.where(is_glass[:, None], d_glass, d_opaque)
        chain[live] &= is_glass
        ended = is_glass & (event == INVALID)  # no extension ray and no last-vertex sky ray
        if b == bounces - 1 and not nee_sky:
            break
        if ended.any():
            keep = ~ended
            live, tri, nrm, d, x = live[keep], tri[keep], nrm[keep], d[keep], x[keep]
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
    v = radiance_samples(scene, camera, window, flags, bounces, RP.CHUNK_SPP, np.random.default_rng([seed, chunk]), **features)
    return v.sum(0), (v * v).sum(0)


def render(scene, camera, window, flags, bounces, spp, seed, **features):
    """per-pixel (mean, variance) of `spp` per-sample values, spp a multiple of ref_pathtrace.CHUNK_SPP; (H, W, 3) each"""
    assert spp % RP.CHUNK_SPP == 0
    return RC.mean_var([chunk_sums(scene, camera, window, flags, bounces, seed, c, **features) for c in range(spp // RP.CHUNK_SPP)], spp)


# ---------------------------------------------------------------------------------------------------------------- self-test op 38
ALPHAS = (0.05, 0.2, 0.5, 1.0)


def op38_rows(m=8192):
    """(ior, thin, d, n, alpha, u, u2, u3) as float32 / uint32 arrays: test_glass_cpu.op32_rows' recipe at m random rows plus its special
    rows, alpha drawn from ALPHAS, u2 and u3 uniform on the 2^-23 grid"""
    import math

    f = np.float32
    rng = np.random.default_rng(38)
    n = rng.normal(size=(m, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = rng.normal(size=(m, 3)) * rng.uniform(0.25, 4.0, (m, 1))
    ior, thin = rng.uniform(1.0, 2.0, m), rng.integers(0, 2, m)
    u = rng.integers(0, 1 << 23, m) / float(1 << 23)
    nz, crit = np.array([0.0, 0.0, 1.0]), math.asin(1.0 / 1.5)
    special = [(1.5, 0, [0, 0, -1.0], nz, 0.5), (1.5, 0, [0, 0, 2.0], nz, 0.5), (1.5, 0, [0, 0, -1.0], nz, 0.01), (1.0, 0, [0.3, 0.1, -1.0], nz, 0.0)]
    for th in (crit - 1e-3, crit + 1e-3, 0.0, 1.2):
        for t in (0, 1):
            for uu in (0.03, 0.5, 0.999):
                special.append((1.5, t, [math.sin(th), 0.0, math.cos(th)], nz, uu))
    ior = np.concatenate([ior, [s[0] for s in special]]).astype(f)
    thin = np.concatenate([thin, [s[1] for s in special]]).astype(np.uint32)
    d = np.concatenate([d, np.array([s[2] for s in special], np.float64)]).astype(f)
    n = np.concatenate([n, np.array([s[3] for s in special], np.float64)]).astype(f)
    u = np.concatenate([u, [s[4] for s in special]]).astype(f)
    k = len(u)
    alpha = np.asarray(ALPHAS, f)[rng.integers(0, len(ALPHAS), k)]
    u2 = (rng.integers(0, 1 << 23, k) / float(1 << 23)).astype(f)
    u3 = (rng.integers(0, 1 << 23, k) / float(1 << 23)).astype(f)
    return ior, thin, d, n, alpha, u, u2, u3


def op38_reference(ior, thin, d, n, alpha, u, u2, u3):
    """The float64 answers for the float32 rows (alpha > 0) and the rounding bounds of the device's fp32 evaluation (rt3_glass.hpp:
    frost_sample): e = 2^-24 per rounding, |n| = 1, first-order propagation.  Vectors carry bounds on the EUCLIDEAN NORM of their error (N..),
    scalars absolute bounds (E..); a unit vector's error is perpendicular to it to first order, which is where most of the tightness comes
    from.  Rows on which a first-order term exceeds 1/20 of the quantity it perturbs are `open`; on the others the second order is below
    1/20 of the first, and every final bound is the first order times 1.1.

      ud = d / sqrt(d.d): relative 4 e per component                                                              (op32_reference)
      b1, b2 (build_orthonormal_basis): a = 1 / (1 + |n.z|) 2 e; x y a relative 4 e of at most 1/2; 1 - x^2 a: 4 e + 1 e   5 e per entry
      wo.z = -(ud.n_in): n_in exact, sum |ud_i n_i| <= 1: (4 + 1) e, two sums 2 e                                 Ewz = 7 e
      wo.x, wo.y = -(ud.b): sum |ud_i| <= sqrt(3) times 5 e, sum |ud_i b_i| <= 1 times (4 + 1) e, two sums 2 e: 16 e each
                                                                                      Nwxy = 16 sqrt(2) e;  Nwo = sqrt(Nwxy^2 + Ewz^2)
      Vh = v / |v|, v = (alpha wo.x, alpha wo.y, wo.z): dv = (alpha dwo.xy, dwo.z); only its part across Vh counts, and of a z-error
          that is |Vh.xy|:                                                            NVh = (alpha Nwxy + Ewz |Vh.xy|) / |v| + 4 e
      T1 = (-Vh.y, Vh.x, 0) / |Vh.xy| (outside the band Vh.z >= 0.9999, where T1 = (1, 0, 0) exactly) is wo.xy turned by a right angle
          and normalised -- alpha and |v| cancel: it turns by wo.xy's error across its length      NT1 = Nwxy / |wo.xy| + 4 e
      T2 = Vh x T1                                                                    NT2 = NVh + NT1 + 5 e
          T2.z = |Vh.xy| (in the band -Vh.y), whatever T1's azimuth                   ET2z = NVh + 3 e
      r = sqrt(u2) e; sin, cos of 2 pi u3 by Horner polynomials 3 e; t1 = r cos, t2' = r sin              Et = 5 e
      sv = (1 + Vh.z) / 2                                                             Esv = NVh / 2 + e
      root = sqrt(a), a = 1 - t1^2: h = 2 |t1| Et + 2 e; |sqrt(a + h) - sqrt(a)| <= 0.6 h / sqrt(a) for h <= a / 2   Eroot = 0.6 h / root + e
      t2 = root + sv (t2' - root)                                                     Et2 = Esv |t2' - root| + (1 - sv) Eroot + sv Et + 3 e
      q = 1 - t1^2 - t2^2: Eq = 2 |t1| Et + 2 |t2| Et2 + 3 e;  nz = sqrt(max(0, q))   Enz = 0.6 Eq / nz + e
      Nh = t1 T1 + t2 T2 + nz Vh (T1.z = 0 exactly):   NNhxy = Et + |t1| NT1 + Et2 + |t2| NT2 + Enz |Vh.xy| + nz NVh + 4 e
                                                        ENhz = Et2 |T2.z| + |t2| ET2z + Enz Vh.z + nz NVh + 3 e
      m = p / |p|, p = (alpha Nh.x, alpha Nh.y, max(0, Nh.z)): as for Vh              Nm = (alpha NNhxy + ENhz |m.xy|) / |p| + 4 e
      cos_i = wo.m: dwo.m, and wo.dm with dm across m, so only wo's part across m counts, sin_i = sqrt(1 - cos_i^2)
                                                                                      Eci = Nwxy |m.xy| + Ewz m.z + sin_i Nm + 3 e
      cos_t^2, cos_t, r_s, r_p, F, F': op32_reference's lines with Eci in the place of its 7 e for c, without its doubling:
          E2 = (2 |cos_i| Eci + e + 4 e eta^2) / eta^2 + 5 e |cos_t^2|;  Ect = 0.6 E2 / cos_t + e;
          dr = 2 (b da + a db) / (a + b)^2 + 3 e;  dF = |r_s| dr_s + |r_p| dr_p + 3 e F;  thin: 2 dF + 3 e
      reflected r = (2 cos_i) m - wo                                                  Nr = 2 Eci + 2 |cos_i| Nm + Nwo + 3 e
                                                                                      Erz = 2 Eci m.z + 2 |cos_i| Nm |m.xy| + Ewz + 3 e
      refracted t = k m - wo / eta, k = cos_i / eta - cos_t:  Ek = (Eci + 2 e) / eta + Ect + e |k|
                                                                                      Nt = Ek + |k| Nm + (Nwo + 2 e) / eta + 2 e
                                                                                      Etz = Ek m.z + |k| Nm |m.xy| + (Ewz + 2 e) / eta + 2 e
      world = wi.x b1 + wi.y b2 + wi.z n_in: the frame is orthonormal, its five inexact entries 5 e each (norm sqrt(5) 5 e < 12 e), five
          roundings                                                                   Ndir = Nwi + 12 e |wi| + 5 e
      G1(c, a^2) = 2 / (1 + s), s = sqrt(1 + a^2 (1 - c^2) / c^2), c = |wi.z|: dG/dc = 2 a^2 / ((1 + s)^2 s c^3); eight roundings of
          values <= 1                                                                 EG = dG/dc Ewiz + 8 e

    A row is `open` -- no determined branch, or a first-order term above 1/20 of what it perturbs -- when Vh.z lies within 2 NVh of 0.9999,
    q < 20 Eq, 1 - t1^2 < 20 h, |cos_t^2| < 20 E2 (total internal reflection aside, where F = 1 exactly), |wo.xy| < 20 Nwxy outside the band,
    or |v| or |p| below 20 times the error of v or p; for the event alone also when u lies within dF of F, the frame's height wo.z within
    2 Ewz of 1e-5, or the tested height (r.z or -t.z) within twice its bound of 1e-5.
    Returns a dict: event, dir, F, weight, d_dir, dF, dW (bounds), open, ev_open."""
    e = U24
    r = rule(np.float64, ior, thin, d, n, alpha, u, u2, u3)
    a = np.asarray(alpha, np.float64)
    Ewz, Nwxy = 7 * e, 16 * np.sqrt(2.0) * e
    Nwo = np.hypot(Nwxy, Ewz)
    wo, Vh, m = r["wo"], r["Vh"], r["m"]
    wxy = np.hypot(wo[:, 0], wo[:, 1])
    lv = np.sqrt((a * wxy) ** 2 + wo[:, 2] ** 2)
    vhxy = np.hypot(Vh[:, 0], Vh[:, 1])
    band = r["band"]
    with np.errstate(divide="ignore", invalid="ignore"):
        NVh = (a * Nwxy + Ewz * vhxy) / lv + 4 * e
        NT1 = np.where(band, 0.0, Nwxy / wxy + 4 * e)
        NT2 = NVh + NT1 + 5 * e
        ET2z = NVh + 3 * e
        T2z = np.where(band, np.abs(Vh[:, 1]), vhxy)
        Et = 5 * e
        Esv = NVh / 2 + e
        t1, t2 = np.abs(r["t1"]), np.abs(r["t2"])
        h = 2 * t1 * Et + 2 * e
        Eroot = 0.6 * h / r["root"] + e
        Et2 = Esv * np.abs(r["t2p"] - r["root"]) + (1 - r["sv"]) * Eroot + r["sv"] * Et + 3 * e
        Eq = 2 * t1 * Et + 2 * t2 * Et2 + 3 * e
        Enz = 0.6 * Eq / r["nz"] + e
        NNhxy = Et + t1 * NT1 + Et2 + t2 * NT2 + Enz * vhxy + r["nz"] * NVh + 4 * e
        ENhz = Et2 * T2z + t2 * ET2z + Enz * Vh[:, 2] + r["nz"] * NVh + 3 * e
        lp = np.linalg.norm(r["pre"], axis=1)
        mxy, mz = np.hypot(m[:, 0], m[:, 1]), np.abs(m[:, 2])
        Nm = (a * NNhxy + ENhz * mxy) / lp + 4 * e
        ci, eta, ct2, ct, tir = np.abs(r["cos_i"]), r["eta"], r["ct2"], r["ct"], r["tir"]
        Eci = Nwxy * mxy + Ewz * mz + np.sqrt(np.maximum(0.0, 1.0 - ci * ci)) * Nm + 3 * e
        E2 = (2 * ci * Eci + e + 4 * e * eta**2) / eta**2 + 5 * e * np.abs(ct2)
        ctg = np.where(tir, 1.0, ct)
        Ect = np.where(tir, 0.0, 0.6 * E2 / ctg + e)

        def dr(x, y, dx, dy):
            return 2.0 * (y * dx + x * dy) / (x + y) ** 2 + 3 * e

        drs = dr(ci, eta * ctg, Eci, eta * Ect + 2 * e * eta * ctg)
        drp = dr(eta * ci, ctg, Eci * eta + 2 * e * eta * ci, Ect)
        dF = np.abs(r["rs"]) * drs + np.abs(r["rp"]) * drp + 3 * e * r["F0"]
        dF = np.where(r["thin"], 2.0 * dF + 3 * e, dF)
        dF = 1.1 * np.where(tir, 0.0, dF)
        Nr = 2 * Eci + 2 * ci * Nm + Nwo + 3 * e
        Erz = 2 * Eci * mz + 2 * ci * Nm * mxy + Ewz + 3 * e
        k = np.abs(r["k"])
        Ek = (Eci + 2 * e) / eta + Ect + e * k
        Nt = Ek + k * Nm + (Nwo + 2 * e) / eta + 2 * e
        Etz = Ek * mz + k * Nm * mxy + (Ewz + 2 * e) / eta + 2 * e
        solid_t = ~r["reflect"] & ~r["thin"]
        Nwi, Ewiz = np.where(solid_t, Nt, Nr), np.where(solid_t, Etz, Erz)
        wl = np.linalg.norm(r["wi"], axis=1)
        d_dir = 1.1 * (Nwi + 12 * e * wl + 5 * e)
        c = np.abs(r["wi"][:, 2])
        s = np.sqrt(1.0 + a * a * (1.0 - c * c) / (c * c))
        dW = 1.1 * (2 * a * a / ((1 + s) ** 2 * s * c**3) * Ewiz + 8 * e)
        Ev, Ep = a * Nwxy + Ewz, a * NNhxy + ENhz
        open_ = ((np.abs(Vh[:, 2] - VNDF_BAND) <= 2 * NVh) | (r["q"] < 20 * Eq) | (1 - t1 * t1 < 20 * h) | (~tir & (np.abs(ct2) < 20 * E2)) |
                 (tir & (np.abs(ct2) <= 2 * E2)) | (~band & (wxy < 20 * Nwxy)) | (lv < 20 * Ev) | (lp < 20 * Ep))
        open_ = open_ & r["frame_ok"]  # (a row whose frame is invalid ends before any of this)
        ev_open = open_ | (np.abs(wo[:, 2] - MIN_COS) <= 2 * Ewz) | (r["frame_ok"] & ((np.abs(np.asarray(u, np.float64) - r["F"]) <= dF) |
                                                                                     (np.abs(r["height"] - MIN_COS) <= 2 * Ewiz)))
    bad = ~np.isfinite(d_dir) | ~np.isfinite(dW) | ~np.isfinite(dF)
    return dict(event=r["event"], dir=r["dir"], F=r["F"], weight=r["weight"], d_dir=d_dir, dF=dF, dW=dW, open=open_ | (bad & r["frame_ok"]),
                ev_open=ev_open | (bad & r["frame_ok"]))
