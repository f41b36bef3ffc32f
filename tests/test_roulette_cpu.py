"""Russian roulette (rt3_path_set_roulette) without a GPU: the float32 rule of tests/ref_roulette.py against its
definition in float64 and exact integers, the exactness of the estimator on uniform_float's grid, the random stream against the oracle's,
and the furnace predictor, which tests/test_roulette.py holds the GPU frame against, shown to be unbiased on its own.

Bounds are derived: a survivor's T / q_g is one IEEE division, so float32 and float64 differ by one unit of 2^-24; the predictor's mean is
the mean of bounded samples, held within 5 sigma of the bounded deviation."""
import ctypes as C
import functools
import re
from fractions import Fraction
from pathlib import Path

import numpy as np

import integrator_worlds as IW
import orc
import ref_pathtrace as RP
import ref_roulette as RR
from raytracer3_amd import _lib as L
from test_integrator_cpu import first_vertex, furnace_radiance, furnace_scene, oracle_frame

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
U = 2.0**-24
G = 2.0**-23  # one step of uniform_float's grid
FLOOR = 0.0625


def edge_rows():
    """(T, min_survival, u, what): the rows the issue names, u one grid step either side of q_g included"""
    rows = []
    for what, T in (("zero", (0, 0, 0)), ("negative zero", (-0.0, 0.0, -0.0)), ("negative", (-0.5, -0.25, -1.0)), ("one negative", (0.5, -0.25, 0.1)),
                    ("NaN first", (np.nan, 0.5, 0.5)), ("NaN second", (0.5, np.nan, 0.5)), ("NaN last", (0.5, 0.5, np.nan)), ("all NaN", (np.nan,) * 3),
                    ("m is the floor", (FLOOR, 0.01, 0.0)), ("m below the floor", (0.001, 0.0, 0.0005)), ("m one ulp above the floor", (np.nextafter(F(FLOOR), F(1)), 0, 0)),
                    ("m is 1", (1.0, 0.5, 0.25)), ("m above 1", (3.0, 0.5, 0.25)), ("m infinite", (np.inf, 1.0, 0.0)), ("m one ulp below 1", (np.nextafter(F(1), F(0)), 0.5, 0.5)),
                    ("m off the grid", (0.3, 0.2, 0.1)), ("m tiny off the grid", (0.1234567, 0.01, 0.0))):
        T = np.array(T, F)
        for ms in (FLOOR, 2.0**-7, 1.0, 0.3):
            qg = float(RR.survival(T[None], ms)[0])
            for u in {0.0, 1.0 - G, max(qg - G, 0.0), min(qg, 1.0 - G), min(qg + G, 1.0 - G), 0.5}:
                rows.append((T, ms, u, what))
    return rows


def random_rows(n, seed=7):
    rng = np.random.default_rng(seed)
    T = (rng.random((n, 3)) ** 3 * rng.choice([0.01, 0.3, 1.0, 2.0], (n, 1))).astype(F)
    T[rng.random(n) < 0.05] = 0.0
    ms = rng.choice(np.array([2.0**-7, FLOOR, 0.25, 1.0], F), n)
    u = (rng.integers(0, RR.GRID, n) / RR.GRID).astype(F)
    near = rng.random(n) < 0.2  # a fifth of the draws within two grid steps of q_g
    qg = np.array([RR.survival(T[i:i + 1], ms[i])[0] for i in range(n)])
    u[near] = np.clip(qg[near].astype(np.float64) + rng.integers(-2, 3, int(near.sum())) * G, 0.0, 1.0 - G).astype(F)
    return T, ms, u


def op33_rows():
    """the rows of GPU test 3 (edges, then random ones), grouped by min_survival: [(min_survival, T (n, 3), u (n,))]"""
    edges = edge_rows()
    T, ms, u = random_rows(4000)
    T = np.concatenate([np.array([e[0] for e in edges], F), T])
    ms = np.concatenate([np.array([e[1] for e in edges], F), ms])
    u = np.concatenate([np.array([e[2] for e in edges], F), u])
    return [(float(m), T[ms == m], u[ms == m]) for m in np.unique(ms)]


# ---------------------------------------------------------------------------------------------------------------- 1 the rule
def test_rule_float32_against_float64():
    for ms, T, u in op33_rows():
        s32, T32, q32 = RR.rule(T, ms, u)
        s64, T64, q64 = RR.rule_float64(T, float(F(ms)), u)
        assert np.array_equal(s32, s64)
        assert np.array_equal(q32.astype(np.float64), q64), "q_g is exact in float32: a multiple of 2^-23 in [2^-7, 1]"
        drawn = s64 & (q64 < 1)
        assert np.all(np.abs(T32[drawn].astype(np.float64) - T64[drawn]) <= U * np.abs(T64[drawn])), "one IEEE division"
        kept = s64 & (q64 >= 1)
        assert np.array_equal(T32[kept].view(np.uint32), T[kept].view(np.uint32)), "q_g = 1: the bits are carried"
        assert not T32[~s64].any()


def up(x):
    """the float32 value x, rounded up to uniform_float's grid"""
    return float(np.ceil(float(F(x)) * RR.GRID) / RR.GRID)


def test_edge_cases_by_name():
    seen = {}
    for T, ms, u, what in edge_rows():
        s, Tn, qg = RR.rule(T[None], ms, [u])
        seen.setdefault(what, []).append((bool(s[0]), float(qg[0]), ms, u, Tn[0]))
    for what in ("zero", "negative zero", "negative", "NaN first", "NaN second", "NaN last", "all NaN"):
        assert all(not s and qg == 0.0 for s, qg, *_ in seen[what]), what
    for s, qg, ms, u, _ in seen["one negative"]:  # the largest component decides
        assert qg == up(max(0.5, ms)) and s == (u < qg or qg == 1.0)
    for what in ("m is 1", "m above 1", "m infinite"):
        assert all(s and qg == 1.0 for s, qg, *_ in seen[what]), what
    # one ulp below 1 rounds up to q_g = 1: always survives, bits unchanged
    assert all(s and qg == 1.0 for s, qg, *_ in seen["m one ulp below 1"])
    # at the floor exactly: q_g is the floor, and a draw one step below survives, at q_g and above does not
    for s, qg, ms, u, _ in seen["m is the floor"]:
        assert qg == up(max(FLOOR, ms)) and (s == (u < qg) or qg == 1.0)
    for s, qg, ms, u, _ in seen["m below the floor"]:
        assert qg == up(ms) and (s == (u < qg) or qg == 1.0)
    for what in ("m off the grid", "m tiny off the grid", "m one ulp above the floor"):
        for s, qg, ms, u, _ in seen[what]:
            if qg < 1.0:
                assert (qg * RR.GRID) == int(qg * RR.GRID) and s == (u < qg)
    # both sides of q_g were tried
    assert {True, False} <= {s for s, qg, *_ in seen["m off the grid"] if qg < 1.0}


def test_estimator_is_exactly_unbiased_on_the_grid():
    """sum over all 2^23 values of u of [u < q_g] / q_g is 2^23 exactly; with q in q_g's place it is not, whenever q is off the grid"""
    u = np.arange(RR.GRID, dtype=np.float64) / RR.GRID
    off_grid = 0
    for m in (2.0**-7, FLOOR, 0.1, 0.3, 1.0 / 3.0, 0.5, 0.7071, float(np.nextafter(F(FLOOR), F(1))), float(np.nextafter(F(1), F(0))), 0.999):
        q = F(m)
        qg = float(RR.survival(np.array([[q, 0, 0]], F), 2.0**-7)[0])
        count = int(np.count_nonzero(u < qg))
        assert count == int(np.count_nonzero(u.astype(F) < q)), "u < q <=> u < q_g"
        assert Fraction(count) / Fraction(qg) == RR.GRID
        off_grid += Fraction(count) / Fraction(float(q)) != RR.GRID
    assert off_grid >= 4


def test_random_stream_is_the_oracles():
    lib = orc.lib()
    rng = np.random.default_rng(3)
    px, py, fr = rng.integers(0, 4096, 200), rng.integers(0, 4096, 200), rng.integers(0, 1 << 20, 200)
    idx = rng.integers(0, 1 << 32, 200)
    seed = RR.rng_seed(px, py, fr)
    got = RR.uniform_float(seed, idx)
    for k in range(200):
        s = lib.orc_rng_seed(int(px[k]), int(py[k]), int(fr[k]))
        assert s == int(seed[k]) and F(lib.orc_uniform_float(s, int(idx[k]))) == got[k]


def test_index_ranges_do_not_overlap():
    """at the largest samples * bounces the host accepts with roulette on (s B 8 = 2^30): vertices, glass, roulette, lens"""
    sb = (1 << 30) // 8
    ranges = [(0, sb * 8), (0x40000000, 0x40000000 + 2 * sb), (RR.RNG_BASE, RR.RNG_BASE + sb), (0x80000000, 1 << 32)]
    for (_, hi), (lo, _) in zip(ranges, ranges[1:]):
        assert hi <= lo
    assert RR.RNG_BASE == 0x60000000


# ---------------------------------------------------------------------------------------------------------------- 2 the predictor
@functools.lru_cache(maxsize=None)
def furnace_first_vertex(flags=0):
    osc, cam = furnace_scene(10.0)
    _, gb, covered = oracle_frame(osc, cam, IW.WINDOW_FURNACE, flags, 1, 1)
    assert covered.all()
    return gb


def predict(gb, bounces, samples, start, floor=FLOOR, frame=0, on=True):
    rho0, E0 = first_vertex(gb)
    rho = np.asarray(IW.FURNACE_ALBEDO, F)
    E = RP.EMISSION_SCALE * np.asarray(IW.FURNACE_EMISSION, F).astype(np.float64)
    return RR.furnace_predict(rho0.astype(F), E0, rho, E, bounces, samples, start, floor, frame, on)


def test_predictor_without_roulette_is_the_closed_form():
    gb = furnace_first_vertex()
    for B in (1, 2, 8):
        mean, nearest, tested, ended = predict(gb, B, 2, 0, on=False)
        assert tested == ended == 0 and np.isinf(nearest).all()
        assert np.abs(mean / furnace_radiance(gb, B) - 1.0).max() <= 2 * B * U  # the float32 products of the T chain


def test_predictor_is_unbiased():
    """B = 8, S = 16, start 1, floor 1/16 over the 64 x 48 window.  After the rule a throughput has no component above 1 (T / q with
    q >= max T, or T itself below 1), so vertex k adds at most E per channel and a sample lies in [0, E0 + (B - 1) E]: its standard
    deviation is at most half that range, and the mean of N = W H S independent samples lies within 5 (E0 + (B - 1) E) / (2 sqrt N) of
    its expectation, which for an unbiased rule is the mean of the closed form."""
    B, S = 8, 16
    gb = furnace_first_vertex()
    mean, nearest, tested, ended = predict(gb, B, S, 1)
    want = furnace_radiance(gb, B)
    _, E0 = first_vertex(gb)
    E = RP.EMISSION_SCALE * np.asarray(IW.FURNACE_EMISSION, np.float64)
    band = 5.0 * (E0.max((0, 1)) + (B - 1) * E) / (2.0 * np.sqrt(mean.shape[0] * mean.shape[1] * S))
    dev = np.abs(mean.mean((0, 1)) - want.mean((0, 1)))
    print(f"predictor B={B} S={S}: frame mean / closed form {mean.mean((0, 1)) / want.mean((0, 1))}, deviation / band {dev / band}; "
          f"{ended} of {tested} decisions ended; nearest |u - q_g| {nearest.min():.2e}")
    assert np.all(dev <= band)
    assert 0 < ended < tested
    assert (nearest <= 4 * G).mean() <= 0.01  # what the GPU test leaves out; expected: no pixel


# ---------------------------------------------------------------------------------------------------------------- 3 the surface without a GPU
def test_abi_is_declared_bound_and_built():
    header = (ROOT / "include" / "rt3.h").read_text()
    lib = L.load()
    for name in ("rt3_path_set_roulette", "rt3_path_get_roulette", "rt3_path_roulette_info"):
        assert name in L.EXPORTS and re.search(r"\bint " + name + r"\(", header) and hasattr(lib, name)
    assert C.sizeof(L.RouletteParams) == 16 and L.RouletteParams.min_survival.offset == 4 and L.RouletteParams.reserved.offset == 8
    p = L.RouletteParams()
    assert (p.start_bounce, p.min_survival, tuple(p.reserved)) == (2, 0.0625, (0, 0))
    assert (L.SELFTEST_ROULETTE, L.SELFTEST_ROULETTE_QUEUE) == (33, 34) and re.search(r"^ \*\s+33 the roulette rule", header, re.M) and re.search(r"^ \*\s+34 k_roulette", header, re.M)
    assert "rt3_roulette.o" in (ROOT / "raytracer3_amd" / "csrc" / "Makefile").read_text()
    assert f"kRouletteRngBase = 0x{RR.RNG_BASE:08X}u;" in (ROOT / "raytracer3_amd" / "csrc" / "rt3_roulette.hpp").read_text()
