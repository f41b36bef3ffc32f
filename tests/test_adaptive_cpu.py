"""The decisions of the "adaptive" pass without a GPU: known answers of tests/ref_adaptive.py's predicate, dilation and schedule, and the
condition the GPU tests' fixture has to meet, asserted on oracle frames alone."""
import numpy as np
import pytest

import adaptive_worlds as aw
import orc
import ref_adaptive as ra
from raytracer3_amd import scenes

F = np.float32


def moments(samples):
    """S1, S2 in float32 and in order, like the kernel"""
    s1, s2 = F(0), F(0)
    for y in np.asarray(samples, F):
        s1 = F(s1 + y)
        s2 = F(s2 + F(y * y))
    return s1, s2


def test_equal_samples_pass_at_two():
    s1, s2 = moments([0.37, 0.37])
    assert ra.passes(s1, s2, 2, 0.05, 0.01)
    assert ra.passes(s1, s2, 2, 0.0, 0.01)  # var == 0 passes any threshold, 0 included


def test_negative_variance_is_clamped():
    # three equal samples whose float32 sums round so that S2 - S1 * mean < 0: the clamp makes it a pass, not a NaN or a failure
    found = False
    for v in np.linspace(0.1, 0.9, 400, dtype=F):
        s1, s2 = moments([v] * 3)
        mean = F(s1 / F(3))
        if F(s2 - F(s1 * mean)) < 0:
            found = True
            assert ra.passes(s1, s2, 3, 0.0, 0.01)
    assert found, "no input of the sweep makes the float32 variance negative"
    assert ra.passes(F(1.0), F(0.25), 2, 0.0, 0.01)  # S2 below S1^2 / n outright


def test_threshold_zero_passes_only_without_variance():
    s1, s2 = moments([0.5, 0.5, 0.5, 0.5])
    assert ra.passes(s1, s2, 4, 0.0, 0.01)
    s1, s2 = moments([0.5, 0.5, 0.5, 0.75])
    assert not ra.passes(s1, s2, 4, 0.0, 0.01)
    assert ra.passes(s1, s2, 4, 10.0, 0.01)  # the same pixel under a generous threshold


def test_predicate_known_answer():
    # samples 1, 3: mean 2, var 2; rel = t (2 + dark); passes iff 2 <= 2 rel^2, i.e. rel >= 1
    s1, s2 = moments([1.0, 3.0])
    assert (s1, s2) == (F(4), F(10))
    assert ra.passes(s1, s2, 2, 0.5, 0.01)       # rel = 1.005
    assert not ra.passes(s1, s2, 2, 0.49, 0.01)  # rel = 0.985
    # dark keeps a black pixel with one bright sample from passing only through its low mean
    s1, s2 = moments([0.0, 0.0, 0.0, 0.02])
    assert not ra.passes(s1, s2, 4, 0.5, 1e-6)
    assert ra.passes(s1, s2, 4, 0.5, 0.1)


def test_dilation_and_background():
    H, W = 5, 6
    fg = np.ones((H, W), bool)
    fg[0, :] = False  # a background row
    n = np.full((H, W), 4)
    flat, noisy = moments([0.5] * 4), moments([0.0, 1.0, 0.0, 1.0])
    S1, S2 = np.full((H, W), flat[0], F), np.full((H, W), flat[1], F)
    S1[2, 2], S2[2, 2] = noisy  # one failing foreground pixel
    S1[0, 5], S2[0, 5] = noisy  # and a "failing" background pixel, which does not count
    stay, cnt = ra.next_active(S1, S2, n, fg, fg, 0.05, 0.01, 1)
    want = np.zeros((H, W), bool)
    want[1:4, 1:4] = True
    assert np.array_equal(stay, want) and cnt == dict(active=24, failed=1, staying=9)
    assert not stay[1, 4] and not stay[1, 5]  # next to the background pixel only
    stay0, cnt0 = ra.next_active(S1, S2, n, fg, fg, 0.05, 0.01, 0)
    assert stay0.sum() == 1 and stay0[2, 2] and cnt0["staying"] == 1
    # a stopped pixel never restarts, failing neighbour or not
    active = fg.copy()
    active[2, 3] = False
    stay, _ = ra.next_active(S1, S2, n, active, fg, 0.05, 0.01, 1)
    assert not stay[2, 3] and stay[2, 1]
    # at the window's edge the neighbourhood is clipped
    S1[:], S2[:] = flat
    S1[4, 0], S2[4, 0] = noisy
    stay, _ = ra.next_active(S1, S2, n, fg, fg, 0.05, 0.01, 1)
    assert stay.sum() == 4 and stay[3:5, 0:2].all()


def test_schedule():
    assert [ra.round_samples(n, 4, 4, 24) for n in (0, 4, 20)] == [4, 4, 4]
    assert ra.round_samples(0, 16, 16, 10) == 10  # a cap below min_samples: `samples` for every pixel
    assert ra.round_samples(16, 16, 16, 24) == 8  # the last round is cut at the cap
    y = np.zeros((10, 2, 2), F)
    n, _, _, rounds, paths, capped = ra.simulate(y, np.ones((2, 2), bool), 10)
    assert (n == 10).all() and rounds == 1 and paths == 40 and capped == 4
    y = np.random.default_rng(1).random((24, 3, 3)).astype(F)
    fg = np.ones((3, 3), bool)
    fg[0, 0] = False
    n, S1, _, rounds, paths, capped = ra.simulate(y, fg, 24, 4, 4, 0.0, 0.01, 0)  # threshold 0 on noise: nobody stops
    assert rounds == 6 and capped == 8 and paths == 8 * 24 and n[0, 0] == 0 and S1[0, 0] == 0


def oracle_samples(mesh, cam, bounces, cap, flags, frame, sky=None, window=(aw.W, aw.H)):
    """per-sample luminances (cap, H, W) rebuilt in float64 from the oracle's frames of samples = 1 .. cap (n mean_n - (n - 1) mean_(n-1)),
    and the foreground mask"""
    sc = orc.Scene(mesh, sky)
    g = orc.camera_gconst(cam["position"], cam["direction"], cam["fov_deg"], window[0], window[1])
    g.frame, g.bounces, g.blendfactor, g.samples = frame, bounces, 1.0, 1
    g.pad[0] = flags
    gb, depth = sc.gbuffer(g)
    prev, ys = np.zeros((window[1], window[0])), []
    for n in range(1, cap + 1):
        g.samples = n
        light, _ = sc.reference_mode(g, gb, depth)
        total = ra.luminance(light[..., :3]).astype(np.float64) * n
        ys.append(total - prev)
        prev = total
    return np.array(ys), depth != aw.BACKGROUND_DEPTH


@pytest.fixture(scope="module")
def fixture_samples():
    return oracle_samples(scenes.cornell(), aw.CAMERA, aw.BOUNCES, aw.CAP, aw.FLAGS, aw.FRAME, aw.sky())


@pytest.mark.parametrize("dilate", [0, 1])
def test_fixture_splits_both_ways(fixture_samples, dilate):
    """the condition test_adaptive.py relies on: under the fixture's threshold at least MIN_SHARE of the foreground pixels stop before
    the cap and at least MIN_SHARE reach it, and the window holds background too"""
    y, fg = fixture_samples
    assert 0.2 < fg.mean() < 0.8
    n, _, _, rounds, paths, capped = ra.simulate(y, fg, aw.CAP, **aw.params(dilate=dilate))
    early, full = aw.shares(n, fg)
    print(f"dilate={dilate} threshold={aw.THRESHOLD[dilate]}: {early:.3f} stop early, {full:.3f} reach the cap; counts "
          f"{dict(zip(*np.unique(n[fg], return_counts=True)))}")
    assert early >= aw.MIN_SHARE and full >= aw.MIN_SHARE
    assert rounds == aw.CAP // aw.STEP and paths == n[fg].sum() and capped == (fg & (n == aw.CAP)).sum()
    assert set(np.unique(n[fg])) <= set(range(aw.MIN_SAMPLES, aw.CAP + 1, aw.STEP)) and (n[~fg] == 0).all()


def test_one_pixel_world_on_the_oracle():
    """the construction of test_adaptive.py's one-active-pixel frame: under threshold 0 every foreground pixel but the centre one has
    constant samples, and the centre pixel's first four differ"""
    mesh, cam = aw.one_pixel_world()
    y, fg = oracle_samples(mesh, cam, 2, 12, 0, aw.ONE_PIXEL_FRAME)
    assert fg.sum() > 100 and not fg.all()
    n, _, _, rounds, _, capped = ra.simulate(y, fg, 12, **aw.params(threshold=0.0, dilate=0))
    assert capped == 1 and rounds == 3 and n[aw.H // 2, aw.W // 2] == 12
    assert (n[fg] == 4).sum() == fg.sum() - 1


# ---- the list compaction's reference (ref_adaptive.compact; tests/test_adaptive_compaction.py holds the kernels to it)
def loop_compact(records, mask, W, H, dilate):
    """ref_adaptive.compact as a plain loop over the list"""
    kept = []
    for xy, bn in records.tolist():
        x, y = xy & 0xFFFF, xy >> 16
        keep = mask[y][x] != 0
        if dilate:
            for yy in range(max(y - 1, 0), min(y + 2, H)):
                for xx in range(max(x - 1, 0), min(x + 2, W)):
                    keep = keep or mask[yy][xx] != 0
        kept.append(bool(keep))
    out = [r for r, k in zip(records.tolist(), kept) if k]
    offsets, total = [], 0
    for b in range(0, len(kept), ra.TILE):
        offsets.append(total)
        total += sum(kept[b:b + ra.TILE])
    return np.array(out, np.uint32).reshape(-1, 2), np.array(offsets, np.int64)


@pytest.mark.parametrize("window", aw.SMALL_WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
@pytest.mark.parametrize("dilate", [0, 1])
def test_compact_reference_against_a_plain_loop(window, dilate):
    W, H = window
    rec = aw.border_list(W, H)
    assert len(rec) == W * H - max(W - 2, 0) * max(H - 2, 0)
    some_kept, some_dropped = False, False
    for mask in aw.edge_masks(W, H):
        got, off = ra.compact(rec, mask, W, H, dilate)
        want, want_off = loop_compact(rec, mask.tolist(), W, H, dilate)
        assert np.array_equal(got, want) and np.array_equal(off, want_off), (window, dilate, mask)
        some_kept, some_dropped = some_kept or len(got) > 0, some_dropped or len(got) < len(rec)
    assert some_kept and some_dropped


def test_compact_reference_known_answers():
    # 5 x 4, the mask's one byte at (0, 2): with the 3 x 3 rule (4, 1) -- one byte in front of it in memory -- is not its neighbour
    rec = aw.border_list(5, 4)
    mask = np.zeros((4, 5), np.uint8)
    mask[2, 0] = 1
    xy = lambda r: sorted((int(v) & 0xFFFF, int(v) >> 16) for v in r[:, 0])
    assert xy(ra.compact(rec, mask, 5, 4, 0)[0]) == [(0, 2)]
    assert xy(ra.compact(rec, mask, 5, 4, 1)[0]) == [(0, 1), (0, 2), (0, 3), (1, 3)]  # (1, 1) and (1, 2) are interior: not listed
    # the offsets count per tile of the list, whatever the pixels are: 2 tiles and one entry, every second entry kept
    n = 2 * ra.TILE + 1
    rec = np.zeros((n, 2), np.uint32)
    rec[:, 0] = np.arange(n) % 2  # pixels (0, 0) and (1, 0) of a 2 x 1 window
    rec[:, 1] = np.arange(n)
    got, off = ra.compact(rec, np.array([[1, 0]], np.uint8), 2, 1, 0)
    assert np.array_equal(got[:, 1], np.arange(0, n, 2)) and off.tolist() == [0, ra.TILE // 2, ra.TILE]
    assert ra.compact(rec, np.array([[0, 1]], np.uint8), 2, 1, 1)[1].tolist() == [0, ra.TILE, 2 * ra.TILE]


@pytest.mark.parametrize("dilate", [0, 1])
def test_compact_agrees_with_next_active(dilate):
    """for a list of unique foreground pixels and mask = fail, what the compaction keeps is what next_active lets stay"""
    rng = np.random.default_rng(11 + dilate)
    W, H = 23, 17
    fg = rng.random((H, W)) < 0.7
    n = np.full((H, W), 4)
    y = rng.random((4, H, W)).astype(F) * (rng.random((H, W)) < 0.3)  # some pixels noisy, the rest constant 0
    S1, S2 = y.sum(0, dtype=F), (y * y).sum(0, dtype=F)
    active = fg.copy()
    stay, cnt = ra.next_active(S1, S2, n, active, fg, 0.05, 0.01, dilate)
    fail = active & ~ra.passes(S1, S2, n, 0.05, 0.01)
    assert 0 < cnt["failed"] < cnt["active"] and (not dilate or cnt["staying"] > cnt["failed"])
    ys, xs = np.nonzero(fg)
    order = rng.permutation(len(xs))
    rec = np.stack([(xs | (ys << 16))[order], rng.integers(0, 2 ** 32, len(xs))], 1).astype(np.uint32)
    got, _ = ra.compact(rec, fail.astype(np.uint8), W, H, dilate)
    kept = np.zeros((H, W), bool)
    kept[got[:, 0] >> 16, got[:, 0] & 0xFFFF] = True
    assert len(got) == cnt["staying"] and np.array_equal(kept, stay)


# ---- the big frame (aw.BIG_*): the condition test_adaptive_compaction.py relies on
def test_big_frame_crosses_the_scan_boundaries():
    """on the oracle: more foreground pixels than one chunk of the scan takes, both shares under both dilate settings, and both
    test-compactions read more than one wave's worth of blocks, the first more than one chunk's"""
    y, fg = oracle_samples(scenes.cornell(), aw.CAMERA, aw.BOUNCES, aw.BIG_CAP, aw.FLAGS, aw.FRAME, aw.sky(), (aw.BIG_W, aw.BIG_H))
    wave, chunk = aw.SCAN_WAVE * aw.COMPACT_TILE, aw.SCAN_CHUNK * aw.COMPACT_TILE
    print(f"foreground: {fg.sum()} of {fg.size} pixels = {-(-int(fg.sum()) // aw.COMPACT_TILE)} blocks")
    assert fg.sum() > chunk
    for dilate in (0, 1):
        n, _, _, rounds, paths, capped = ra.simulate(y, fg, aw.BIG_CAP, **aw.big_params(dilate))
        early, full = aw.shares(n, fg, aw.BIG_CAP)
        reads = [int(fg.sum()), int((fg & (n > aw.MIN_SAMPLES)).sum())]  # the lists the two test-compactions read
        print(f"dilate={dilate} threshold={aw.BIG_THRESHOLD[dilate]}: {early:.3f} stop early, {full:.3f} reach the cap; counts "
              f"{dict(zip(*np.unique(n[fg], return_counts=True)))}; the compactions read {reads}")
        assert early >= aw.MIN_SHARE and full >= aw.MIN_SHARE
        assert reads[0] > chunk and reads[1] > wave
        assert rounds == aw.BIG_CAP // aw.STEP and paths == n[fg].sum() and capped == (fg & (n == aw.BIG_CAP)).sum()


def test_compaction_selftest_is_declared():
    """op 35 is in the header and in the binding, and the tile the reference counts by is the kernels'"""
    import re
    from pathlib import Path

    from raytracer3_amd import _lib as L

    root = Path(__file__).resolve().parent.parent
    assert L.SELFTEST_ADAPTIVE_COMPACT == 35 and re.search(r"^ \*\s+35 the list compaction", (root / "include" / "rt3.h").read_text(), re.M)
    assert L.ADAPTIVE_TILE == ra.TILE == aw.COMPACT_TILE
    csrc = root / "raytracer3_amd" / "csrc"
    assert f"kAdaptiveTile = {ra.TILE};" in (csrc / "rt3_internal.hpp").read_text()
    kernels = (csrc / "rt3_adaptive.hip").read_text()
    assert "kAdTile == kAdaptiveTile" in kernels and f"kAdBlock = {aw.SCAN_CHUNK}, kAdWaves = kAdBlock / {aw.SCAN_WAVE};" in kernels
