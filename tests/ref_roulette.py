"""The roulette rule of rt3_path_set_roulette restated in numpy float32, the random stream it draws from, a reference
for k_roulette's compaction, and a predictor of the furnace frame under roulette.  Shares no code with the library.

The rule, for the extension ray that sample s of a pixel emitted at vertex b with throughput T (float32):
    m = max(T) with NaN handed on; not (m > 0): ended, nothing drawn
    q = min(1, max(m, min_survival)); q >= 1: survives unchanged, nothing drawn
    q_g = ceil(q 2^23) 2^-23
    u = uniform_float(rng_seed(px, py, frame), 0x60000000 + s B + b); survives iff u < q_g, with T / q_g
Every operation is one IEEE float32 operation, so numpy float32 gives the device's bits."""
import numpy as np

F = np.float32
RNG_BASE = 0x60000000
GRID = 1 << 23


# ---------------------------------------------------------------------------------------------------------------- the random stream
def _u32(x):
    return np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)


def jenkins(a):
    a = _u32(a)
    a = _u32(_u32(a + np.uint64(0x7ED55D16)) + _u32(a << np.uint64(12)))
    a = _u32((a ^ np.uint64(0xC761C23C)) ^ (a >> np.uint64(19)))
    a = _u32(_u32(a + np.uint64(0x165667B1)) + _u32(a << np.uint64(5)))
    a = _u32(_u32(a + np.uint64(0xD3A2646C)) ^ _u32(a << np.uint64(9)))
    a = _u32(_u32(a + np.uint64(0xFD7046C5)) + _u32(a << np.uint64(3)))
    return _u32((a ^ np.uint64(0xB55A4F09)) ^ (a >> np.uint64(16)))


def _explode(x):
    x = _u32(x)
    for s, m in ((8, 0x00FF00FF), (4, 0x0F0F0F0F), (2, 0x33333333), (1, 0x55555555)):
        x = (x | (x << np.uint64(s))) & np.uint64(m)
    return x


def rng_seed(px, py, frame):
    return _u32(jenkins(_explode(px) | (_explode(py) << np.uint64(1))) + _u32(frame))


def _rotl(x, r):
    return _u32((x << np.uint64(r)) | (x >> np.uint64(32 - r)))


def murmur3(seed, index):
    k = _u32(_u32(index) * np.uint64(0xCC9E2D51))
    k = _u32(_rotl(k, 15) * np.uint64(0x1B873593))
    h = _u32(seed) ^ k
    h = _u32(_u32(_rotl(h, 13) * np.uint64(5)) + np.uint64(0xE6546B64))
    h ^= np.uint64(4)
    h ^= h >> np.uint64(16)
    h = _u32(h * np.uint64(0x85EBCA6B))
    h ^= h >> np.uint64(13)
    h = _u32(h * np.uint64(0xC2B2AE35))
    return h ^ (h >> np.uint64(16))


def uniform_float(seed, index):
    """k 2^-23 for the low 23 bits k of the hash: exactly the device's float"""
    return ((murmur3(seed, index) & np.uint64(GRID - 1)).astype(np.float64) / GRID).astype(F)


def roulette_u(px, py, frame, sample, bounces, bounce):
    return uniform_float(rng_seed(px, py, frame), _u32(RNG_BASE + _u32(sample) * np.uint64(bounces) + np.uint64(bounce)))


# ---------------------------------------------------------------------------------------------------------------- the rule
def survival(T, min_survival):
    """q_g per row of T (n, 3) float32: 0 where not (max(T) > 0), 1 where nothing is drawn"""
    T = np.asarray(T, F).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        m = np.maximum(np.maximum(T[:, 0], T[:, 1]), T[:, 2])  # np.maximum hands a NaN on
        alive = m > 0
        q = np.minimum(F(1.0), np.maximum(np.where(alive, m, F(1.0)), F(min_survival))).astype(F)
        qg = (np.ceil(q * F(GRID)).astype(F) * F(2.0**-23)).astype(F)
    return np.where(alive, np.where(q >= 1, F(1.0), qg), F(0.0)).astype(F)


def rule(T, min_survival, u):
    """(survived (n,) bool, T' (n, 3) float32, q_g (n,) float32) in float32, as self-test op 33 reports them: T' = T where q_g = 1, T / q_g
    for a survivor of a draw, zeros for an ended row"""
    T = np.asarray(T, F).reshape(-1, 3)
    u = np.asarray(u, F).reshape(-1)
    qg = survival(T, min_survival)
    with np.errstate(invalid="ignore"):
        drawn = (qg > 0) & (qg < 1)
        survived = (qg >= 1) | (drawn & (u < qg))
    with np.errstate(divide="ignore", invalid="ignore"):
        scaled = (T / np.where(drawn, qg, F(1.0))[:, None]).astype(F)
    out = np.where(survived[:, None], np.where(drawn[:, None], scaled, T), F(0.0)).astype(F)
    return survived, out, qg


def rule_float64(T, min_survival, u):
    """the rule from its definition, in float64 and exact integers: (survived, T / q_g, q_g); the witness of `rule`"""
    T = np.asarray(T, np.float64).reshape(-1, 3)
    survived, out, qgs = [], [], []
    for t, uu in zip(T, np.asarray(u, np.float64).reshape(-1)):
        m = np.nan if np.isnan(t).any() else t.max()
        if not m > 0:
            survived.append(False), out.append(np.zeros(3)), qgs.append(0.0)
            continue
        q = min(1.0, max(m, float(min_survival)))
        k = GRID if q >= 1 else -((-int(q * 2**60)) // 2**37)  # ceil(q 2^23) in integers: q 2^60 is an integer for q >= 2^-36
        qg = k / GRID
        ok = q >= 1 or int(uu * GRID) < k
        survived.append(ok), out.append(t / qg if ok else np.zeros(3)), qgs.append(qg)
    return np.array(survived), np.array(out), np.array(qgs)


# ---------------------------------------------------------------------------------------------------------------- the compaction
def compact(records, pixels, frame, bounces, bounce, s0, min_survival):
    """k_roulette on a queue of (n, 11) uint32 records {o xyz, pdf, d xyz, path id, T rgb}: the surviving records (their T divided, every other
    word untouched) in the queue's order.  path id = sample_in_batch * npix + pixel index."""
    rec = np.ascontiguousarray(records, np.uint32).reshape(-1, 11)
    pixels = np.asarray(pixels, np.uint32)
    pid = rec[:, 7].astype(np.uint64)
    sib, k = pid // len(pixels), (pid % len(pixels)).astype(np.int64)
    xy = pixels[k] if len(rec) else pixels[:0]
    u = roulette_u(xy & 0xFFFF, xy >> 16, frame, np.uint64(s0) + sib, bounces, bounce)
    survived, T, _ = rule(np.ascontiguousarray(rec[:, 8:11]).view(F), min_survival, u)
    out = rec.copy()
    out[:, 8:11] = np.ascontiguousarray(T).view(np.uint32)
    return out[survived]


# ---------------------------------------------------------------------------------------------------------------- the furnace under roulette
def furnace_predict(rho0, E0, rho, E, bounces, samples, start, min_survival, frame=0, on=True):
    """The frame of a furnace (every surface albedo rho and emission E; first vertex rho0, E0 per pixel from the G-buffer, (H, W, 3)) with
    the diffuse BRDF, whose value over pdf is the albedo: a sample is E0 + sum_k T_k E over the vertices k = 1 .. it reaches, with
    T_1 = rho0 and T_(k+1) = T_k rho, each T passed through the rule between its vertex's shading and the next trace.  The T chain and the
    decisions are the device's float32 operations; the sums are float64.
    Returns (pixel means (H, W, 3) float64, smallest |u - q_g| over each pixel's draws (inf without one), decisions tested, ended)."""
    H, W, _ = rho0.shape
    py, px = np.mgrid[0:H, 0:W]
    rho, E = np.asarray(rho, F), np.asarray(E, np.float64)
    total = np.zeros((H, W, 3))
    nearest = np.full((H, W), np.inf)
    tested = ended = 0
    for s in range(samples):
        value = np.array(E0, np.float64)
        T = np.asarray(rho0, F).copy()  # the extension ray of vertex 0 carries 1 x albedo0
        alive = np.ones((H, W), bool)
        for b in range(bounces - 1):  # the extension ray vertex b emitted
            if on and start <= b:
                u = roulette_u(px, py, frame, s, bounces, b).reshape(H, W)
                survived, Tn, qg = rule(T.reshape(-1, 3), min_survival, u.reshape(-1))
                survived, qg = survived.reshape(H, W), qg.reshape(H, W)
                drawn = alive & (qg > 0) & (qg < 1)
                nearest = np.where(drawn, np.minimum(nearest, np.abs(u.astype(np.float64) - qg.astype(np.float64))), nearest)
                tested += int(alive.sum())
                ended += int((alive & ~survived).sum())
                alive &= survived
                T = Tn.reshape(H, W, 3)
            value += np.where(alive[..., None], T.astype(np.float64) * E, 0.0)  # vertex b + 1 collects its emission
            T = (T * rho).astype(F)
        total += value
    return total / samples, nearest, tested, ended
