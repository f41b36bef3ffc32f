"""Float64 NumPy restatement of the material-texture part of the surface stage (test infrastructure).  It extends
ref_surface.reference -- which stays the reference for albedo and for everything of a geometry without material textures -- with the
rule of include/rt3.h, and is written from that rule, not from the device code.

The rule
  All three lookups use the uv of ref_surface, the same texel coordinates (x = u W - 0.5, floor, indices mod W and H) and weights, at
  mip 0, and blend with lerp(a, b, f) = a + (b - a) f along x, then y.  In real arithmetic that is ref_surface's bilinear form.
  roughness = roughness_factor * G / 255, metalness = metallic_factor * B / 255.
  emissive  = (emission * 12) * EOTF(rgb).
  normal    per flattened primitive, from the fp32 positions and uvs as uploaded (object space): e1 = p1 - p0, e2 = p2 - p0,
            det = du1 dv2 - du2 dv1, T = normalise(e1 dv2 - e2 dv1) sign(det), h = sign(det) sign(dot(e1 x e2, n0 + n1 + n2)); det = 0:
            no tangent.  At a hit, n = the normalised blend of ref_surface (before the matrix): t = normalise(T - n (n.T)),
            b = h cross(n, t), c = 2 lerp(byte / 255) - 1, n' = normalise(s c.x t + s c.y b + c.z n); then normalise(M n') as before.
            No tangent, or a texture index outside the uploaded textures: n stays.

Tolerances (derived, not tuned).  d_tex below is ref_surface's albedo bound, 2^-23 (4 (max|u_i| W + max|v_i| H + 1) + 8): the error of a
bilinear lookup of values in [0, 1] times a factor <= 1, from the uv roundings (scaled by W, H; a weight enters twice) plus at most eight
fp32 roundings.
  roughness, metalness
            inherit d_tex unchanged: the values are in [0, 1] like a colour, the uv roundings are the same, and the arithmetic is
            byte * (1/255) (two roundings, where the colour table has one), two lerps of two roundings each (the other form has three)
            and the product with a factor in [0, 1]: seven roundings, within the eight counted.
  emissive  the same lookup (table, two lerps) times emission * 12, which carries one rounding more and is at most 12 max|emission|:
            d_tex * 12 max|emission| covers table + 4 + 1 + 1 = 7 roundings of values up to that size.
  normal    Three sources.  (1) n, before the matrix, is off by at most a_n = OCTA_STEP / L + 8 * 2^-23 (ref_surface's bound with kappa = 1,
            of which the blend and one normalisation are 8 roundings).  (2) T is stored octahedrally at 15 bits per coordinate: by
            ref_surface's argument with 32767 for 65535 it turns by at most sqrt(18) / 32767; its fp32 evaluation (edges, uv differences,
            two products, a difference without cancellation -- see the conditions -- and a normalisation) adds at most 16 roundings:
            a_T = sqrt(18) / 32767 + 16 * 2^-23.  The frame (t, b, n) is orthonormal and a function of n and of the azimuth of T about
            n only.  Tilting n by a_n inside the plane of n and T turns the frame by a_n; tilting it across that plane turns it by
            a_n / sin(theta), theta the angle between T and n (rotation vector -a_n (t + cot(theta) n)); moving T by a_T changes its
            azimuth by at most a_T / sin(theta).  Rotation vectors add, so the frame turns by at most (a_n + a_T) / sin(theta), and so
            does n' = frame * c', whatever the length of c' = (s c.x, s c.y, c.z).  (3) c' is off by at most
            d_c = 2 d_tex sqrt(2 s^2 + 1) (2 x - 1 doubles the lookup's error, s scales two components), which turns a vector of length
            |c'| by at most d_c / |c'|.  The fp32 evaluation of the projection (amplified by 1 / sin(theta)), the cross product, the
            three scaled sums (relative to |c'|) and the normalisation adds at most 24 / sin(theta) + 16 / min(|c'|, 1) roundings.
            The matrix multiplies all of it by kappa and adds ref_surface's 16 roundings:
                angle <= kappa ((a_n + a_T) / sin(theta) + d_c / |c'| + 2^-23 (24 / sin(theta) + 16 / min(|c'|, 1) + 16))
            (the first-order terms are of size 1e-3 at most, second order 1e-6 relative: covered by the rounding allowance).
            Where n stays, the bound is ref_surface's.

Conditions, asserted by `reference`: ref_surface's own (L >= 0.5, barycentrics, finite bounded uv -- for every texture a hit reads);
factors in [0, 1]; and for every normal-mapped hit sin(theta) >= 0.5, |c'| >= 0.5, |s| <= 2, no cancellation in the tangent
(|e1| |dv2| + |e2| |dv1| <= 2 |e1 dv2 - e2 dv1|, which orthogonal edges guarantee), a determinant that is exactly zero (both products
zero) or at least 2^-10 of |du1 dv2| + |du2 dv1|, and |dot(e1 x e2, sum n_i)| >= 0.1 |e1 x e2| |sum n_i| so that no rounding decides a
sign."""
import numpy as np

import ref_surface as R

TAN_STEP = np.sqrt(18.0) / 32767.0  # rad: the largest turn of a 2 x 15-bit octahedral tangent
EPS23 = R.EPS23


def linear_bilinear(tex, u, v, decode):
    """(n, 4) bilinear lookup of an (H, W, 4) uint8 texture at float64 (u, v), `decode` applied per byte; lerp along x, then y"""
    H, W = tex.shape[:2]
    val = decode(np.asarray(tex, np.uint8))
    x, y = u * W - 0.5, v * H - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb, ya, yb = np.mod(x0, W), np.mod(x0 + 1, W), np.mod(y0, H), np.mod(y0 + 1, H)
    top = val[ya, xa] + (val[ya, xb] - val[ya, xa]) * fx
    bot = val[yb, xa] + (val[yb, xb] - val[yb, xa]) * fx
    return top + (bot - top) * fy


def unorm(byte):
    return np.asarray(byte, np.float64) / 255.0


def tangents(p, uv, vn):
    """(T (n, 3), h (n,), valid (n,)) of triangles with positions p (n, 3, 3), uvs (n, 3, 2) and vertex normals vn (n, 3, 3), float64
    holding the uploaded fp32 values; asserts the conditions of the module docstring"""
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    du1, dv1 = uv[:, 1, 0] - uv[:, 0, 0], uv[:, 1, 1] - uv[:, 0, 1]
    du2, dv2 = uv[:, 2, 0] - uv[:, 0, 0], uv[:, 2, 1] - uv[:, 0, 1]
    a, b = du1 * dv2, du2 * dv1
    det = a - b
    valid = det != 0
    assert ((a[~valid] == 0) & (b[~valid] == 0)).all()  # "no tangent" only where fp32 sees an exact zero too
    assert (np.abs(det[valid]) >= 2.0**-10 * (np.abs(a) + np.abs(b))[valid]).all()
    r = e1 * dv2[:, None] - e2 * dv1[:, None]
    ln = np.linalg.norm(r, axis=1)
    assert (ln[valid] > 0).all()
    l1, l2 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)
    assert (l1 * np.abs(dv2) + l2 * np.abs(dv1) <= 2.0 * ln + 1e-300)[valid].all()
    T = np.where(valid[:, None], r / np.where(ln > 0, ln, 1.0)[:, None] * np.sign(det)[:, None], 0.0)
    gn, ns = np.cross(e1, e2), vn.sum(1)
    d = (gn * ns).sum(1)
    assert (np.abs(d) >= 0.1 * np.linalg.norm(gn, axis=1) * np.linalg.norm(ns, axis=1))[valid].all()
    return T, np.sign(det) * np.sign(d), valid


class Materials:
    """the float64 surfaces of a batch of hits under the material-texture rule, with the bounds of the module docstring per hit"""


def reference(mesh, instances, prim, bu, bv):
    """`base` = ref_surface.reference of the same hits (albedo, and everything where no material texture applies); the rest as named"""
    base = R.reference(mesh, instances, prim, bu, bv)
    geom, inst, first_prim, counts, mats = R.flatten(mesh, instances)
    prim = np.asarray(prim, np.int64)
    n_hits = len(prim)
    bu, bv = np.asarray(bu, np.float32).astype(np.float64), np.asarray(bv, np.float32).astype(np.float64)
    b = np.stack([1.0 - bu - bv, bu, bv], 1)
    entry = base.entry
    gi = geom[entry]
    g = mesh.geometries[gi]
    mt = mesh.material_textures[gi]
    io = g["index_offset"].astype(np.int64) + 3 * (prim - first_prim[entry])
    vi = g["vertex_offset"].astype(np.int64)[:, None] + np.stack([mesh.indices[io], mesh.indices[io + 1], mesh.indices[io + 2]], 1).astype(np.int64)
    vert = np.asarray(mesh.vertices, np.float32).astype(np.float64)[vi]  # (n, 3, 8)
    uv3 = vert[:, :, 6:8]
    u, v = (b * uv3[:, :, 0]).sum(1), (b * uv3[:, :, 1]).sum(1)
    textures = [np.asarray(t, np.uint8) for t in (getattr(mesh, "textures", None) or [])]

    def present(index):
        index = index.astype(np.int64)
        return (index >= 0) & (index < len(textures)), index

    def d_tex(k, image):
        H, W = image.shape[:2]
        assert np.isfinite(uv3[k]).all() and (np.abs(uv3[k, :, 0]) * W + np.abs(uv3[k, :, 1]) * H <= 2.0**12).all()
        return EPS23 * (4 * (np.abs(uv3[k, :, 0]).max(1) * W + np.abs(uv3[k, :, 1]).max(1) * H + 1) + 8)

    out = Materials()
    out.base = base
    # ---- roughness and metalness
    rf, mf = g["roughness"].astype(np.float64), g["metallic_factor"].astype(np.float64)
    out.roughness, out.metalness, out.mr_bound = rf.copy(), mf.copy(), np.zeros(n_hits)
    out.has_mr, mr = present(mt["metallic_roughness_texture"])
    assert ((rf >= 0) & (rf <= 1) & (mf >= 0) & (mf <= 1))[out.has_mr].all()
    for t in np.unique(mr[out.has_mr]):
        k = np.flatnonzero(out.has_mr & (mr == t))
        val = linear_bilinear(textures[t], u[k], v[k], unorm)
        out.roughness[k], out.metalness[k] = rf[k] * val[:, 1], mf[k] * val[:, 2]
        out.mr_bound[k] = d_tex(k, textures[t])
    # ---- emissive
    e12 = g["emission"][:, :3].astype(np.float64) * 12.0
    out.emissive, out.emissive_bound = e12.copy(), 2.0**-24 * np.abs(e12).max(1)
    out.has_e, em = present(mt["emissive_texture"])
    for t in np.unique(em[out.has_e]):
        k = np.flatnonzero(out.has_e & (em == t))
        out.emissive[k] = e12[k] * linear_bilinear(textures[t], u[k], v[k], R.srgb_eotf)[:, :3]
        out.emissive_bound[k] = d_tex(k, textures[t]) * np.abs(e12[k]).max(1)
    # ---- normal
    vn = vert[:, :, 3:6]
    vn = vn / np.linalg.norm(vn, axis=2, keepdims=True)
    blend = (b[:, :, None] * vn).sum(1)
    L = np.linalg.norm(blend, axis=1)
    n = blend / L[:, None]
    M = np.stack([m[:3, :3].astype(np.float64) for m in mats])[inst[entry]]
    sv = np.linalg.svd(M, compute_uv=False)
    kappa = sv[:, 0] / sv[:, -1]
    out.normal, out.normal_bound, out.unmapped_normal = base.normal.copy(), base.normal_bound.copy(), base.normal
    has_n, nt = present(mt["normal_texture"])
    T, h, valid = tangents(vert[:, :, 0:3], uv3, vert[:, :, 3:6])
    out.no_tangent = has_n & ~valid
    out.has_n = has_n & valid
    s = mt["normal_scale"].astype(np.float64)
    for t in np.unique(nt[out.has_n]):
        k = np.flatnonzero(out.has_n & (nt == t))
        c = 2.0 * linear_bilinear(textures[t], u[k], v[k], unorm)[:, :3] - 1.0
        nk, Tk, sk = n[k], T[k], s[k]
        proj = Tk - nk * (nk * Tk).sum(1, keepdims=True)
        sin_t = np.linalg.norm(proj, axis=1)
        tk = proj / sin_t[:, None]
        bk = h[k, None] * np.cross(nk, tk)
        cp = np.stack([sk * c[:, 0], sk * c[:, 1], c[:, 2]], 1)
        lc = np.linalg.norm(cp, axis=1)
        assert (sin_t >= 0.5).all() and (lc >= 0.5).all() and (np.abs(sk) <= 2.0).all(), (sin_t.min(), lc.min(), np.abs(sk).max())
        m = cp[:, 0:1] * tk + cp[:, 1:2] * bk + cp[:, 2:3] * nk
        m = np.einsum("nij,nj->ni", M[k], m / np.linalg.norm(m, axis=1, keepdims=True))
        out.normal[k] = m / np.linalg.norm(m, axis=1, keepdims=True)
        a_n, a_T = R.OCTA_STEP / L[k] + 8 * EPS23, TAN_STEP + 16 * EPS23
        d_c = 2.0 * d_tex(k, textures[t]) * np.sqrt(2.0 * sk * sk + 1.0)
        out.normal_bound[k] = kappa[k] * ((a_n + a_T) / sin_t + d_c / lc + EPS23 * (24.0 / sin_t + 16.0 / np.minimum(lc, 1.0) + 16.0))
    return out
