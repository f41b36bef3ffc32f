"""Float64 NumPy restatement of the surface stage (test infrastructure): what turns a hit (flattened primitive, bu, bv) into the
Surface a path vertex is shaded with -- hit_info of the device and of the oracle.  Written from the rule,
not from either fp32 implementation, and from the scene as it is uploaded: the mesh, the instance list and the textures.

The rule
  normal    n = normalise(b0 n0 + bu n1 + bv n2), b0 = 1 - bu - bv, over the triangle's three vertex normals, each normalised; under a
            non-identity instance n = normalise(M n) with M the upper 3 x 3 of the instance's fp32 matrix, as written (no inverse
            transpose).  Under the identity M n = n, so the reference needs no shortcut of its own.
  albedo    base_color[:3], times the texture colour when 0 <= texture index < number of textures: the IEC 61966-2-1 EOTF of each byte,
            bilinear at x = u W - 0.5, y = v H - 0.5 with (u, v) = b0 t0 + bu t1 + bv t2, texel indices mod W and mod H, mip 0.
  emissive  emission[:3] * 12;  roughness, metalness: copied.

Tolerances (derived, not tuned)
  normal    The implementations keep a vertex normal as a 2 x 16-bit octahedral word.  Rounding a coordinate of the [-1, 1]^2 octahedral
            square to 16 bits moves it by at most 1 / 65535; the unnormalised octahedral vector (x, y, 1 - |x| - |y|) therefore moves
            by at most sqrt(1 + 1 + 4) / 65535 in length (z moves by up to twice a coordinate step) and is at least 1 / sqrt(3) long,
            so the decoded direction turns by at most sqrt(6) sqrt(3) / 65535 = sqrt(18) / 65535 rad.  The blend b0 n0 + bu n1 + bv n2
            is a convex combination, so it moves by at most that much, and normalising a vector of length L = |sum b_i n_i| turns the
            error into an angle of at most (sqrt(18) / 65535) / L.  A linear map changes an angle by at most the ratio kappa of its
            extreme singular values.  fp32 evaluation (two normalisations, the blend, nine products) adds at most 16 roundings of
            2^-23 relative, amplified the same way:
                angle <= (sqrt(18) / 65535) kappa / L + 16 * 2^-23 kappa             (kappa = 1 under the identity)
  albedo    The lookup is continuous in (u, v): where the fp32 floor lands on the other side of a texel edge the weight of the texel
            that changed is the rounding error itself, so only rounding counts.  x = u W - 0.5 carries the rounding of the uv blend
            (three products, two sums of terms up to max_i |u_i|) scaled by W, of the product and of the difference: at most
            4 * 2^-24 (max|u_i| W + 1) absolute, and the same in y; a unit step of the weight fx or fy changes the result (values in
            [0, 1]) by at most 1, and a weight enters twice (top and bottom row).  The EOTF table, the three lerps and the product
            with base_color <= 1 add at most 8 roundings of 2^-23:
                |albedo - reference| <= 2^-23 (4 (max_i |u_i| W + max_i |v_i| H + 1) + 8)
            An untextured albedo is a copy and must be exact.
  emissive  one fp32 rounding of e * 12: |got - 12 e| <= 2^-24 * 12 |e|.  Roughness and metalness are copies: exact.

The bounds hold for inputs with L >= 0.5 (the vertex normals of a triangle within 60 degrees of a common direction), bu, bv >= 0,
bu + bv <= 1, finite uv and |u| W + |v| H <= 2^12 at every vertex; `reference` asserts these conditions on what it is given."""
import numpy as np

OCTA_STEP = np.sqrt(18.0) / 65535.0  # rad: the largest turn of a 2 x 16-bit octahedral normal
EPS23 = 2.0**-23
IDENTITY = np.eye(4, dtype=np.float32)


def flatten(mesh, instances):
    """The flattened world: one entry per (instance, geometry) pair, instance-major; no instances = everything once under the identity.
    Returns (geometry index, instance index, first flattened primitive, primitive count) per entry, and the instance matrices (fp32)."""
    if not instances:
        instances = [(0, len(mesh.geometries), IDENTITY)]
    geom, inst = [], []
    for i, (first, count, _) in enumerate(instances):
        assert first + count <= len(mesh.geometries)
        geom += list(range(first, first + count))
        inst += [i] * count
    geom, inst = np.array(geom, np.int64), np.array(inst, np.int64)
    counts = np.asarray(mesh.prim_counts, np.int64)[geom] if len(geom) else np.zeros(0, np.int64)
    first_prim = np.concatenate([[0], np.cumsum(counts)[:-1]]) if len(geom) else np.zeros(0, np.int64)
    mats = [np.asarray(m, np.float32).reshape(4, 4) for _, _, m in instances]
    return geom, inst, first_prim, counts, mats


def srgb_eotf(byte):
    """IEC 61966-2-1: the linear value of an sRGB-encoded byte"""
    c = np.asarray(byte, np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def texture_bilinear(tex, u, v):
    """(n, 3) linear colour of an (H, W, 4) uint8 sRGB texture at float64 (u, v): bilinear, repeat addressing, mip 0"""
    H, W = tex.shape[:2]
    lin = srgb_eotf(tex[..., :3])
    x, y = u * W - 0.5, v * H - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb, ya, yb = np.mod(x0, W), np.mod(x0 + 1, W), np.mod(y0, H), np.mod(y0 + 1, H)
    top = lin[ya, xa] * (1.0 - fx) + lin[ya, xb] * fx
    bot = lin[yb, xa] * (1.0 - fx) + lin[yb, xb] * fx
    return top * (1.0 - fy) + bot * fy


class Surfaces:
    """the float64 surfaces of a batch of hits, with the bounds of the module docstring per hit"""

    def __init__(self, n):
        self.albedo, self.emissive, self.normal = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
        self.roughness, self.metalness = np.zeros(n, np.float32), np.zeros(n, np.float32)
        self.normal_bound, self.albedo_bound = np.zeros(n), np.zeros(n)
        self.textured = np.zeros(n, bool)
        self.entry = np.zeros(n, np.int64)  # flattened geometry of each hit
        self.tex = np.full(n, -1, np.int64)  # the texture a hit reads, -1 for none
        self.uv = np.zeros((n, 2))  # and where


def reference(mesh, instances, prim, bu, bv):
    """Surfaces of the hits (flattened primitive ids, fp32 barycentrics) of the world `mesh` placed by `instances`"""
    geom, inst, first_prim, counts, mats = flatten(mesh, instances)
    prim = np.asarray(prim, np.int64)
    bu, bv = np.asarray(bu, np.float32).astype(np.float64), np.asarray(bv, np.float32).astype(np.float64)
    assert (prim >= 0).all() and (prim < counts.sum()).all()
    assert (bu >= 0).all() and (bv >= 0).all() and (bu + bv <= 1).all()
    b = np.stack([1.0 - bu - bv, bu, bv], 1)
    # the entry of a primitive: the last one that starts at or before it and is not empty
    live = np.flatnonzero(counts > 0)
    entry = live[np.searchsorted(first_prim[live], prim, side="right") - 1]
    local = prim - first_prim[entry]
    g = mesh.geometries[geom[entry]]
    io = g["index_offset"].astype(np.int64) + 3 * local
    vi = g["vertex_offset"].astype(np.int64)[:, None] + np.stack([mesh.indices[io], mesh.indices[io + 1], mesh.indices[io + 2]], 1).astype(np.int64)
    vert = np.asarray(mesh.vertices, np.float32).astype(np.float64)[vi]  # (n, 3, 8)
    out = Surfaces(len(prim))
    out.entry = entry
    # ---- normal
    vn = vert[:, :, 3:6]
    ln = np.linalg.norm(vn, axis=2, keepdims=True)
    assert (ln > 0).all()
    vn = vn / ln
    blend = (b[:, :, None] * vn).sum(1)
    L = np.linalg.norm(blend, axis=1)
    assert (L >= 0.5).all(), L.min()
    n = blend / L[:, None]
    M = np.stack([m[:3, :3].astype(np.float64) for m in mats])[inst[entry]]
    n = np.einsum("nij,nj->ni", M, n)
    out.normal = n / np.linalg.norm(n, axis=1, keepdims=True)
    sv = np.linalg.svd(M, compute_uv=False)
    kappa = sv[:, 0] / sv[:, -1]
    out.normal_bound = OCTA_STEP * kappa / L + 16 * EPS23 * kappa
    # ---- albedo
    out.albedo = g["base_color"][:, :3].astype(np.float64)
    tex = g["base_color_texture_index"].astype(np.int64)
    textures = list(getattr(mesh, "textures", None) or [])
    out.textured = (tex >= 0) & (tex < len(textures))
    uv = vert[:, :, 6:8]
    for t in np.unique(tex[out.textured]):
        k = np.flatnonzero(out.textured & (tex == t))
        image = np.asarray(textures[t], np.uint8)
        H, W = image.shape[:2]
        assert np.isfinite(uv[k]).all() and (np.abs(uv[k, :, 0]) * W + np.abs(uv[k, :, 1]) * H <= 2.0**12).all()
        u, v = (b[k] * uv[k, :, 0]).sum(1), (b[k] * uv[k, :, 1]).sum(1)
        out.albedo[k] = out.albedo[k] * texture_bilinear(image, u, v)
        out.tex[k], out.uv[k, 0], out.uv[k, 1] = t, u, v
        out.albedo_bound[k] = EPS23 * (4 * (np.abs(uv[k, :, 0]).max(1) * W + np.abs(uv[k, :, 1]).max(1) * H + 1) + 8)
    # ---- the rest
    out.emissive = g["emission"][:, :3].astype(np.float64) * 12.0
    out.roughness, out.metalness = g["roughness"].astype(np.float32), g["metallic_factor"].astype(np.float32)
    return out


def angle(a, b):
    """angle between unit vectors (rows), accurate near 0: 2 asin(|a - b| / 2)"""
    return 2.0 * np.arcsin(np.clip(np.linalg.norm(a - b, axis=1) / 2.0, 0.0, 1.0))
