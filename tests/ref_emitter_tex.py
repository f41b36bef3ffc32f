"""References for textured emitters: the emissive lookup of a point on an emitter, the quadrature of a textured
emitter's mean texel and the queue kernel k_emit_tex, each restated twice -- in float64 (the value meant) and in numpy float32 with the
device's operations in the device's order (the bits expected; the library is built without contraction, so every float32 numpy operation is
one device operation).  Test infrastructure only; tests/test_emitter_tex_cpu.py checks it against hand-worked answers."""
import numpy as np

import ref_roulette as RR
import ref_surface as RS

F = np.float32
MAX_L = 64
LUM = (0.299, 0.587, 0.114)


def lut32():
    """the device's sRGB table: the float64 EOTF of every byte, rounded once"""
    return RS.srgb_eotf(np.arange(256)).astype(F)


# ---------------------------------------------------------------------------------------------------------------- the lookup
def uv_at32(uv, b1, b2):
    """tri_uv_at(uv, 1 - b1 - b2, b1, b2) in float32: uv (..., 3, 2), b1 and b2 (...)"""
    uv, b1, b2 = np.asarray(uv, F), np.asarray(b1, F), np.asarray(b2, F)
    b0 = (F(1.0) - b1) - b2
    return ((uv[..., 0, 0] * b0 + uv[..., 1, 0] * b1) + uv[..., 2, 0] * b2).astype(F), ((uv[..., 0, 1] * b0 + uv[..., 1, 1] * b1) + uv[..., 2, 1] * b2).astype(F)


def uv_at64(uv, b1, b2):
    uv, b1, b2 = np.asarray(uv, np.float64), np.asarray(b1, np.float64), np.asarray(b2, np.float64)
    b0 = 1.0 - b1 - b2
    return uv[..., 0, 0] * b0 + uv[..., 1, 0] * b1 + uv[..., 2, 0] * b2, uv[..., 0, 1] * b0 + uv[..., 1, 1] * b1 + uv[..., 2, 1] * b2


def lookup32(tex, u, v):
    """tex_quad + quad_srgb in float32: (n, 3) of an (H, W, 4) uint8 texture at float32 (u, v)"""
    H, W = tex.shape[:2]
    u, v = np.asarray(u, F).reshape(-1), np.asarray(v, F).reshape(-1)
    lin = lut32()[tex[..., :3]]
    x, y = (u * F(W) - F(0.5)).astype(F), (v * F(H) - F(0.5)).astype(F)
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf).astype(F)[:, None], (y - yf).astype(F)[:, None]
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    xa, xb, ya, yb = np.mod(x0, W), np.mod(x0 + 1, W), np.mod(y0, H), np.mod(y0 + 1, H)
    lerp = lambda a, b, f: (a + ((b - a).astype(F) * f).astype(F)).astype(F)  # noqa: E731  lerp_ab
    return lerp(lerp(lin[ya, xa], lin[ya, xb], fx), lerp(lin[yb, xa], lin[yb, xb], fx), fy)


def lookup64(tex, u, v):
    return RS.texture_bilinear(tex, np.asarray(u, np.float64).reshape(-1), np.asarray(v, np.float64).reshape(-1))


def radiance32(le, uv, tex, b1, b2):
    """the emitter-side radiance Le (*) rgb at (b1, b2) in float32 (op 42): le (3,), uv (3, 2), b1 and b2 (n,)"""
    n = len(np.asarray(b1).reshape(-1))
    uu, vv = uv_at32(np.broadcast_to(np.asarray(uv, F), (n, 3, 2)), b1, b2)
    return (np.asarray(le, F)[None, :] * lookup32(tex, uu, vv)).astype(F)


def radiance64(le, uv, tex, b1, b2):
    n = len(np.asarray(b1).reshape(-1))
    uu, vv = uv_at64(np.broadcast_to(np.asarray(uv, np.float64), (n, 3, 2)), b1, b2)
    return np.asarray(le, np.float64)[None, :] * lookup64(tex, uu, vv)


# ---------------------------------------------------------------------------------------------------------------- the quadrature
def subdiv_of_edge(texels):
    """L for a longest edge of `texels` texels: clamp(ceil, 1, 64), 1 for a non-finite one"""
    t = F(texels)
    if not np.isfinite(t):
        return 1
    c = np.ceil(t)
    return 1 if not c >= 1 else int(min(c, MAX_L))


def subdiv(uv, W, H):
    """L of a triangle with vertex uvs uv (3, 2) on a W x H texture, float32 as the device measures it"""
    uv = np.asarray(uv, F)
    with np.errstate(invalid="ignore", over="ignore"):
        edge = lambda a, b: max(F(abs(F(uv[b, 0] - uv[a, 0])) * F(W)), F(abs(F(uv[b, 1] - uv[a, 1])) * F(H)))  # noqa: E731
        e = [edge(0, 1), edge(0, 2), edge(1, 2)]
    if not all(np.isfinite(x) for x in e):
        return 1
    return subdiv_of_edge(max(e))


def centroids(L):
    """(b1, b2) float32 of the L^2 centroids in the kernel's order k = a L + c"""
    k = np.arange(L * L)
    a, c = k // L, k % L
    up = a + c < L
    i, j, o = np.where(up, a, L - 1 - a), np.where(up, c, L - 1 - c), np.where(up, 1, 2)
    d = F(3 * L)
    return ((3 * i + o).astype(F) / d).astype(F), ((3 * j + o).astype(F) / d).astype(F)


def mean32(uv, tex):
    """k_emit_tex_power's mean texel, bit for bit: lane l of 64 adds centroids l, l + 64, ... in order, the lane sums meet in a butterfly"""
    H, W = tex.shape[:2]
    L = subdiv(uv, W, H)
    b1, b2 = centroids(L)
    val = radiance32((1.0, 1.0, 1.0), uv, tex, b1, b2)
    rows = -(-L * L // 64)
    pad = np.zeros((rows * 64, 3), F)
    pad[: L * L] = val
    pad = pad.reshape(rows, 64, 3)
    s = np.zeros((64, 3), F)
    for r in range(rows):
        live = (r * 64 + np.arange(64)) < L * L
        s[live] = (s[live] + pad[r][live]).astype(F)
    lane = np.arange(64)
    for w in (32, 16, 8, 4, 2, 1):
        s = (s + s[lane ^ w]).astype(F)
    return (s[0] / F(L * L)).astype(F), L


def mean64(uv, tex):
    H, W = tex.shape[:2]
    L = subdiv(uv, W, H)
    b1, b2 = centroids(L)  # the rule's own centroids (float32 quotients), evaluated in float64
    return radiance64((1.0, 1.0, 1.0), uv, tex, b1.astype(np.float64), b2.astype(np.float64)).mean(0), L


def mean_bound(L, uv_max, size_max):
    """|mean32 - mean64| per channel for texels in [0, 1], vertex uvs of magnitude <= uv_max (>= 1) and a texture of at most size_max texels
    a side; u = 2^-24.  One lookup: b0 = 1 - b1 - b2 carries 2 u; the uv is three products (<= uv_max each, one rounding each, plus b0's
    2 u uv_max) and two sums (<= 3 uv_max): at most 11 uv_max u, say 12.  The texel coordinate u W - 0.5 is then off by 12 uv_max W u plus the
    product's and the difference's rounding (<= uv_max W u each): 14 uv_max W u; x - floor(x) is exact.  A bilinear lookup of values in
    [0, 1] is continuous with slope <= 1 per texel in each direction (also across a texel border, where the two footprints agree), so both
    coordinates move it by <= 28 uv_max size_max u.  Each lerp a + (b - a) f of values in [0, 1] adds 3 roundings <= u; the two x lerps
    pass through the y lerp with weight <= 1: 6 u.  The table entry is rounded once: u.  So a lookup is off by (28 uv_max size_max + 7) u.
    A float32 sum of n = L^2 terms <= 1, in any order, is off by <= (n - 1) u n; after the division by n (one more u) the mean is off by
    (28 uv_max size_max + 7 + n) u.  (With the float32 texel coordinate given, this is the issue's rough (n + 8) u.)"""
    u = 2.0 ** -24
    return (28.0 * max(1.0, uv_max) * size_max + 7 + L * L) * u


def power64(area, le, mean):
    return float(area) * float(np.dot(np.asarray(le, np.float64) * np.asarray(mean, np.float64), LUM))


# ---------------------------------------------------------------------------------------------------------------- the queue kernel
def light_find(cdf, k):
    """the first entry with cdf > k"""
    return np.searchsorted(np.asarray(cdf, np.int64), np.asarray(k, np.int64), side="right")


def queue32(cdf, emit_uv, emit_tex, textures, frame, bounces, bounce, s0, dims, pixels, records, count=None):
    """k_emit_tex in float32 on the queue `records` (n, 4) of 32-bit words {contribution r, g, b, path id}: the contributions afterwards,
    (n, 3) uint32.  cdf: the table's; emit_uv (n_e, 3, 2) and emit_tex (n_e,): its side array; textures: the uploaded list."""
    rec = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 4)
    n = len(rec)
    count = n if count is None else count
    out = rec[:, :3].copy()
    pixels = np.asarray(pixels, np.uint32)
    npix = len(pixels)
    pid = rec[:count, 3].astype(np.int64)
    sib = pid // npix
    xy = pixels[pid - sib * npix].astype(np.uint64)
    seed = RR.rng_seed(xy & np.uint64(0xFFFF), xy >> np.uint64(16), frame)
    base = (((s0 + sib) * bounces + bounce) * dims).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    u5, u6, u7 = (RR.uniform_float(seed, (base + np.uint64(d)) & np.uint64(0xFFFFFFFF)) for d in (5, 6, 7))
    ke = (u5 * F(8388608.0)).astype(np.int64)
    e = light_find(cdf, ke)
    su = np.sqrt(u6).astype(F)
    b1 = (u7 * su).astype(F)
    b2 = (su - b1).astype(F)
    for t in np.unique(emit_tex[e]):
        if t < 0:
            continue
        m = np.flatnonzero(emit_tex[e] == t)
        uu, vv = uv_at32(emit_uv[e[m]], b1[m], b2[m])
        rgb = lookup32(textures[t], uu, vv)
        out[m] = (rec[m, :3].view(F) * rgb).astype(F).view(np.uint32)
    return out, e
