"""The light table's reference (tests/ref_light_table.py) without a GPU: properties it did not assume -- the lookup realises the masses
exactly, never returns an entry without mass, stays inside the guide cells' brackets -- its agreement with the older numpy masses, and the
declaration and binding of self-test op 40 and rt3_light_table."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import ref_light_table as rl
from raytracer3_amd import _lib as L
from test_nee_emissive_cpu import masses

ROOT = Path(__file__).resolve().parent.parent
TABLES = ("skewed_257", "sparse_4097")


@pytest.fixture(scope="module", params=TABLES)
def table(request):
    p, a = rl.power_set(request.param)
    t = rl.LightTable(p, a)
    return p, a, t, t.find(np.arange(rl.CDF_TOTAL, dtype=np.int64))  # the lookup at every k there is


def test_histogram_of_find_is_the_mass(table):
    _, _, t, found = table
    assert found.min() >= 0 and found.max() < t.n
    assert np.array_equal(np.bincount(found, minlength=t.n), t.mass)


def test_cdf_ends_at_the_total(table):
    p, _, t, _ = table
    assert int(t.q.sum()) > 0 and t.total == int(t.cdf[-1]) == rl.CDF_TOTAL
    assert np.all(np.diff(t.cdf) >= 0) and int(t.mass.sum()) == rl.CDF_TOTAL
    assert np.all((t.q == 0) <= (t.mass == 0)), "no weight, no mass"
    for n in (1, 5, 300):  # and without any power there is no CDF
        z = rl.LightTable(np.zeros(n, np.float32), np.ones(n, np.float32))
        assert z.total == 0 and not z.cdf.any() and not z.w.any() and not z.q.any()


def test_find_never_returns_an_entry_without_mass(table):
    _, _, t, found = table
    assert (t.mass == 0).any(), "the table has such entries"
    assert np.all(t.mass[found] > 0)


def test_find_stays_between_its_cell_and_the_next(table):
    _, _, t, found = table
    c = np.arange(rl.CDF_TOTAL, dtype=np.int64) >> t.shift
    assert t.cells == 1 << (23 - t.shift) and t.cells >= t.n > t.cells // 2 and len(t.guide) == t.cells + 1
    assert np.all(t.guide[c] <= found) and np.all(found <= t.guide[c + 1])
    assert np.all(np.diff(t.guide) >= 0) and t.guide[-1] == t.n - 1


def test_masses_agree_with_the_older_reference(table):
    p, _, t, _ = table
    share = masses(p.astype(np.float64)).astype(np.float64)  # no 2^24 grid: test_table_matches_numpy_in_both_modes' tolerance
    err = np.abs(t.mass.astype(np.float64) - share)
    assert np.all(err <= 3.0 + 2e-5 * share), err.max()


def test_weights_and_quotients():
    p, a = rl.power_set("skewed_257")
    q, cdf, w, cells, shift, guide, find = rl.light_table(p, a)
    assert q.max() == rl.WEIGHT_GRID and (cells, shift) == (512, 14)
    assert np.array_equal(find([0, rl.CDF_TOTAL - 1]), [np.flatnonzero(cdf > 0)[0], np.flatnonzero(np.diff(cdf, prepend=0) > 0)[-1]])
    mass = np.diff(cdf, prepend=0)
    assert (a == 0).any() and ((a > 0) & (a < np.finfo(np.float32).tiny)).any(), "areas of every kind"
    assert w.dtype == np.float32 and np.all(w[(mass == 0) | (a == 0)] == 0) and np.all(w[(mass > 0) & (a > 0)] > 0)
    # ties go up: exactly half a grid step is weight 1, a quarter is 0
    assert rl.LightTable(*rl.power_set("giant_tie")).q.tolist().count(1) == 999
    assert rl.LightTable(*rl.power_set("giant_last")).q.sum() == rl.WEIGHT_GRID
    hp, ha = rl.power_set("half_way_4097")
    r = hp.astype(np.float64) * rl.WEIGHT_GRID
    tie = r != np.floor(r)
    assert tie.sum() == len(hp) - 1 and np.array_equal(rl.LightTable(hp, ha).q[tie], (r[tie] + 0.5).astype(np.int64))
    # the cap: 2^20 cells however many lights
    big = rl.LightTable(*rl.power_set("uniform_2p20_1"))
    assert (big.cells, big.shift) == (1 << 20, 3) and set(np.unique(big.mass)) == {7, 8}
    assert rl.LightTable(*rl.power_set("uniform_2p19_1")).cells == 1 << 20


def test_named_sets_reach_what_they_are_named_for():
    """the named sets reach what they are named for (the reference's own numbers)"""
    t = {n: rl.LightTable(*rl.power_set(n)) for n in ("three", "uniform_2p20_1", "giant_middle", "giant_tie", "sparse_65537", "all_zero")}
    assert t["three"].cells == 4 > t["three"].n
    assert (t["uniform_2p20_1"].shift, set(np.unique(t["uniform_2p20_1"].mass))) == (3, {7, 8})
    assert np.all(np.diff(t["uniform_2p20_1"].guide[:-1]) >= 1), "every cell of the capped table has a boundary"
    assert t["giant_middle"].mass.tolist().count(0) == 999 and t["giant_tie"].q.tolist().count(1) == 999
    s = t["sparse_65537"]
    lit = np.flatnonzero(s.mass > 0)
    assert np.diff(lit).max() > 1000 and np.all(np.isin(s.guide[:-1], lit)), "runs of zero mass that the guide cells step over"
    assert np.bincount(s.guide[:-1]).max() > 1000, "and lights that span many guide cells"
    assert t["all_zero"].total == 0


def test_boundary_keys_cover_what_they_claim():
    t = rl.LightTable(*rl.power_set("sparse_4097"))
    k = t.boundary_keys(5)
    assert k.dtype == np.uint32 and k.max() == rl.CDF_TOTAL - 1 and k.min() == 0 and len(np.unique(k)) == len(k)
    s = set(k.tolist())
    lit = np.flatnonzero(t.mass > 0)
    assert all(int(t.cdf[e]) - 1 in s for e in lit) and all(int(t.cdf[e]) in s for e in lit[:-1])
    assert all((c << t.shift) in s for c in range(t.cells)) and all((c << t.shift) - 1 in s for c in range(1, t.cells))
    few = t.boundary_keys(5, entries=lit[:2])
    assert len(few) < len(k) and int(t.cdf[lit[1]]) in set(few.tolist())


def test_header_declares_op_and_call():
    h = (ROOT / "include" / "rt3.h").read_text()
    assert re.search(r"^ \*\s+40 the selection part of the light table", h, re.M)
    assert re.search(r"int rt3_light_table\(rt3_ctx \*ctx, uint32_t flags, float \*rec[^,]*, uint32_t \*cdf, uint32_t \*guide, uint32_t \*prim, float \*area,\s+uint32_t \*cells, uint32_t \*shift\);", h)
    internal = (ROOT / "raytracer3_amd" / "csrc" / "rt3_internal.hpp").read_text()
    assert "kSelftestTableHeaderIn = 2, kSelftestTableHeader = 3;" in internal


def test_binding_exposes_op_and_call():
    assert L.SELFTEST_LIGHT_TABLE == 40
    assert "rt3_light_table" in L.EXPORTS
    lib = L.load()
    assert hasattr(lib, "rt3_light_table")
    assert lib.rt3_light_table.restype is C.c_int
    assert list(lib.rt3_light_table.argtypes) == [C.c_void_p, C.c_uint32] + [C.c_void_p] * 5 + [C.POINTER(C.c_uint32)] * 2
    assert lib.rt3_light_table(None, 0, None, None, None, None, None, None, None) == L.E_INVALID  # no context: refused, nothing touched
    from raytracer3_amd.render_graph import Context

    assert callable(Context.light_table) and callable(Context.selftest_light_table)
