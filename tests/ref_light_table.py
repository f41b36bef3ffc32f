"""The light sampler's selection table in float64 and integers, written from the description of self-test op 40 in
include/rt3.h, for tests/test_light_table.py and tests/test_light_table_cpu.py.

Every float64 step is one IEEE operation or an exact scaling by a power of two, and every sum is an integer below 2^53, so this is what the
device computes bit for bit -- whatever the order of its scan and whether or not its compiler fuses a multiply with an add."""
import numpy as np

CDF_TOTAL = 1 << 23
WEIGHT_GRID = 1 << 24
MAX_GUIDE_CELLS = 1 << 20


class LightTable:
    """q (n,) int64 weights, cdf (n,) int64, mass (n,) int64, w (n,) float32 = p_sel / area, cells, shift, guide (cells + 1,) int64"""

    def __init__(self, power, area):
        power = np.asarray(power, np.float32).reshape(-1)
        area = np.asarray(area, np.float32).reshape(-1)
        n = len(power)
        assert n >= 1 and len(area) == n
        assert np.all(np.isfinite(power)) and np.all(power >= 0), "powers are non-negative and finite"
        p64 = power.astype(np.float64)
        pm = float(p64.max())
        if pm > 0.0:
            self.q = np.floor(p64 / pm * float(WEIGHT_GRID) + 0.5).astype(np.int64)
        else:
            self.q = np.zeros(n, np.int64)
        prefix = np.cumsum(self.q, dtype=np.int64)  # <= n 2^24 <= 2^48: exact
        Q = int(prefix[-1])
        if Q > 0:
            self.cdf = np.floor(prefix.astype(np.float64) / float(Q) * float(CDF_TOTAL)).astype(np.int64)
        else:
            self.cdf = np.zeros(n, np.int64)
        self.total = int(self.cdf[-1])
        self.mass = np.diff(self.cdf, prepend=0)
        p_sel = (self.mass.astype(np.float64) / CDF_TOTAL).astype(np.float32)  # mass <= 2^23: exact in fp32
        ok = (self.mass > 0) & (area > 0)
        with np.errstate(over="ignore"):  # a subnormal area may take the quotient to inf, on the device as here
            self.w = np.where(ok, p_sel / np.where(ok, area, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
        cells = 1
        while cells < n and cells < MAX_GUIDE_CELLS:
            cells <<= 1
        self.n, self.cells, self.shift = n, cells, 23 - (cells.bit_length() - 1)
        guide = np.searchsorted(self.cdf, np.arange(cells, dtype=np.int64) << self.shift, "right")
        self.guide = np.concatenate([guide, [n - 1]]).astype(np.int64)

    def find(self, k):
        """the entry that owns k in [0, 2^23): the first e with cdf[e] > k"""
        return np.searchsorted(self.cdf, np.asarray(k, np.int64), "right")

    def boundary_keys(self, seed, entries=None):
        """the values of k at which a lookup can go wrong: both sides of every CDF boundary (of the entries listed, default all with mass) and of
        every guide cell's start, both ends of the range, and 4096 random values"""
        e = np.flatnonzero(self.mass > 0) if entries is None else np.asarray(entries)
        e = e[self.mass[e] > 0]
        hi = self.cdf[e]
        c = np.arange(self.cells, dtype=np.int64) << self.shift
        rnd = np.random.default_rng(seed).integers(0, CDF_TOTAL, 4096)
        k = np.concatenate([hi - 1, hi, c, c - 1, [0, CDF_TOTAL - 1], rnd])
        return np.unique(k[(k >= 0) & (k < CDF_TOTAL)]).astype(np.uint32)


def light_table(power, area):
    """(q, cdf, w, cells, shift, guide, find) of the table over fp32 powers and areas"""
    t = LightTable(power, area)
    return t.q, t.cdf, t.w, t.cells, t.shift, t.guide, t.find


# ---------------------------------------------------------------------------------------------------------------- named power sets
def _areas(n, seed):
    """mixed areas: mostly ordinary, some 0, some subnormal, some huge"""
    rng = np.random.default_rng(seed)
    a = np.exp2(rng.uniform(-12.0, 4.0, n)).astype(np.float32)
    kind = rng.integers(0, 16, n)
    a[kind == 0] = 0.0
    a[kind == 1] = np.float32(1e-42)  # subnormal
    a[kind == 2] = np.float32(3e37)
    a[kind == 3] = 1.0
    return a


def _uniform(n):
    return np.ones(n, np.float32)


def _log_uniform(n, seed):
    return np.exp2(np.random.default_rng(seed).uniform(-20.0, 20.0, n)).astype(np.float32)


def _giant(n, at, rest):
    p = np.full(n, rest, np.float32)
    p[at] = 1.0
    return p


def _half_way(n):
    """ratios (j + 0.5) / 2^24 of the largest: every weight is a tie, rounded half up"""
    p = ((np.arange(n, dtype=np.float64) * 37 % 4093 + 0.5) / WEIGHT_GRID).astype(np.float32)  # j < 2^12: j + 0.5 is exact in fp32
    p[n // 2] = 1.0
    return p


def _geometric(n):
    return np.exp2(-(np.arange(n) % 24).astype(np.float64)).astype(np.float32)


def _sparse(n, seed):
    rng = np.random.default_rng(seed)
    p = np.zeros(n, np.float32)
    on = rng.random(n) < 1e-3
    on[rng.integers(0, n)] = True
    p[on] = np.exp2(rng.uniform(-3.0, 3.0, int(on.sum()))).astype(np.float32)
    return p


def _skewed(n, seed):
    return (np.random.default_rng(seed).random(n) ** 8).astype(np.float32)


POWER_SETS = {
    "one": lambda: _uniform(1),
    "two": lambda: np.array([3.0, 1.0], np.float32),
    "three": lambda: np.array([1.0, 2.0, 4.0], np.float32),  # cells = 4 > n
    "uniform_255": lambda: _uniform(255),
    "uniform_256": lambda: _uniform(256),
    "uniform_257": lambda: _uniform(257),
    "uniform_4097": lambda: _uniform(4097),
    "uniform_65537": lambda: _uniform(65537),  # several scan tiles
    "uniform_2p19_1": lambda: _uniform((1 << 19) + 1),  # cells = 2^20: the guide kernel's sentinel on a thread's second trip
    "uniform_2p20_1": lambda: _uniform((1 << 20) + 1),  # the cell cap: shift 3, masses 7 / 8
    "log_uniform_257": lambda: _log_uniform(257, 11),
    "log_uniform_4097": lambda: _log_uniform(4097, 12),
    "log_uniform_65537": lambda: _log_uniform(65537, 13),
    "giant_first": lambda: _giant(1000, 0, 2.0 ** -26),  # the rest round to weight 0
    "giant_middle": lambda: _giant(1000, 500, 2.0 ** -26),
    "giant_last": lambda: _giant(1000, 999, 2.0 ** -26),
    "giant_tie": lambda: _giant(1000, 500, 2.0 ** -25),  # exactly half a grid step: ties go up, to weight 1
    "half_way_4097": lambda: _half_way(4097),
    "geometric_4097": lambda: _geometric(4097),
    "sparse_4097": lambda: _sparse(4097, 21),  # one light in 1000 has power: runs of zero mass span many cells
    "sparse_65537": lambda: _sparse(65537, 22),
    "skewed_257": lambda: _skewed(257, 31),
    "all_zero": lambda: np.zeros(300, np.float32),
}


def power_set(name):
    """(power, area) float32 of a named set; the same arrays on every call"""
    p = POWER_SETS[name]()
    return p, _areas(len(p), 1000 + sorted(POWER_SETS).index(name))
