"""The list compaction of the "adaptive" pass (rt3_adaptive.hip: k_ad_count, k_ad_scan, k_ad_scatter) past one
block, one wave and one chunk.

A block takes 2048 list entries; the one-workgroup scan takes 64 block counts per wave and 256 per chunk, with a carry between chunks.
The frames of test_adaptive.py and test_adaptive_lens.py are 67 x 45 and 64 x 48: two blocks, two live lanes of the scan.  Here

1. self-test op 35 (Context.selftest_adaptive_compact) runs the pass's own three launches, through its own scratch plan, on made-up
   lists and masks of up to 1 573 641 entries (769 blocks, four chunks) and is held to tests/ref_adaptive.compact: the count, every
   block offset, both destination lists and the caller's words behind them, all exactly (integers: there is no tolerance);
2. one whole frame at 1400 x 940 (adaptive_worlds.BIG_*: 545 222 foreground pixels, 267 blocks) is held to the fixed pass and to
   ref_adaptive.next_active like test_adaptive.py's small frames, with guards that it does cross the boundaries.

What the cases reach: lengths 1 .. 4096 the block boundary; 131 071 .. 131 073 the first block of a second wave; 524 287 .. 524 289 the
second chunk (carry, parity flip, the `i < n_blocks` tail in a later chunk); 1 048 577 and 1 573 641 a third and a fourth chunk."""
import numpy as np
import pytest

import adaptive_worlds as aw
import orc
import ref_adaptive as ra
from raytracer3_amd import _lib as L
from raytracer3_amd.render_graph import Context
from test_adaptive import World, check_against_fixed, check_decisions, counts_of

pytestmark = pytest.mark.gpu

TILE = aw.COMPACT_TILE
WAVE, CHUNK = aw.SCAN_WAVE * TILE, aw.SCAN_CHUNK * TILE  # list entries whose block counts fill one wave / one chunk of the scan
assert (TILE, WAVE, CHUNK) == (ra.TILE, 131072, 524288) and L.ADAPTIVE_TILE == TILE
SMALL_N = (1, 63, 64, 65, 2047, 2048, 2049, 4096)
LARGE_N = (WAVE - 1, WAVE, WAVE + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 3 * CHUNK + 777)
PREFILL = 0xC3000000
# the smallest of these windows that holds the list: odd sizes, no multiples of the 64 x 64 tiles of the list's order
WINDOWS = ((67, 62), (403, 327), (1029, 511), (1536, 683), (1536, 1025))


@pytest.fixture(scope="module")
def ctx():
    """a bare context: the op reads no context state"""
    c = Context()
    yield c
    c.close()


_lists = {}


def window_for(n):
    return next((w, h) for w, h in WINDOWS if w * h >= n)


def production_list(n, rank=0, n_ranks=1, window=None):
    """(W, H, records (n, 2)): the first n entries of the rank's pixel list of the window (Z-order inside 64 x 64 tiles), each with a random
    blue-noise word, so that a record that loses its partner shows"""
    W, H = window or window_for(n)
    key = (W, H, rank, n_ranks)
    if key not in _lists:
        xy = orc.tile_pixels(W, H, rank, n_ranks)
        rec = np.empty((len(xy), 2), np.uint32)
        rec[:, 0] = xy[:, 0] | (xy[:, 1] << 16)
        rec[:, 1] = np.random.default_rng(W * 7 + H + rank).integers(0, 2 ** 32, len(xy), dtype=np.uint32)
        rec.setflags(write=False)
        _lists[key] = rec
    rec = _lists[key]
    assert n is None or n <= len(rec)
    return W, H, rec[:n]


def wave_end_blocks(n):
    b = np.arange(n) // TILE
    return (b % aw.SCAN_WAVE == aw.SCAN_WAVE - 1) | (b % aw.SCAN_CHUNK == aw.SCAN_CHUNK - 1)


# name -> keep[i] per list entry.  The tile patterns make every block count 0 or 2048: "alternating" puts 2048 on the last lane of every
# wave and of every chunk of the scan and 0 on the first, "tiles_but_wave_ends" drops every 64th and every 256th block (the last lane has
# 0 under 63 lanes of 2048), "only_wave_ends" is its complement.
PATTERNS = {
    "none": lambda n, rng: np.zeros(n, bool),
    "all": lambda n, rng: np.ones(n, bool),
    "bernoulli_0.02": lambda n, rng: rng.random(n) < 0.02,
    "bernoulli_0.5": lambda n, rng: rng.random(n) < 0.5,
    "bernoulli_0.98": lambda n, rng: rng.random(n) < 0.98,
    "tiles_alternating": lambda n, rng: (np.arange(n) // TILE) % 2 == 1,
    "tiles_but_wave_ends": lambda n, rng: ~wave_end_blocks(n),
    "only_wave_ends": lambda n, rng: wave_end_blocks(n),
    "first": lambda n, rng: np.arange(n) == 0,
    "last": lambda n, rng: np.arange(n) == n - 1,
    "every_2048th": lambda n, rng: np.arange(n) % TILE == 0,
    "last_block": lambda n, rng: np.arange(n) // TILE == (n - 1) // TILE,
}


def mask_of(keep, rec, W, H, rng):
    """the window-space mask whose byte is non-zero exactly at the kept entries' pixels (any non-zero byte counts, not only 1)"""
    mask = np.zeros((H, W), np.uint8)
    xy = rec[keep, 0]
    mask[xy >> 16, xy & 0xFFFF] = rng.choice(np.array([1, 1, 1, 2, 0x80, 0xFF], np.uint8), len(xy))
    return mask


def check(ctx, W, H, dilate, mask, rec):
    """op 35 against the reference: count, block offsets, the kept entries in order in both lists, the caller's words behind them"""
    n = len(rec)
    pre_xy = PREFILL + np.arange(n, dtype=np.uint32)
    pre_bn = (PREFILL ^ 0x0F000000) + np.arange(2 * n, dtype=np.uint32).reshape(n, 2)
    count, off, xy, bn = ctx.selftest_adaptive_compact(W, H, dilate, mask, rec, pre_xy, pre_bn)
    want, want_off = ra.compact(rec, mask, W, H, dilate)
    what = f"n = {n}, window {W} x {H}, dilate {dilate}"
    assert count == len(want), f"{what}: count {count}, reference {len(want)}"
    assert len(off) == -(-n // TILE) and np.array_equal(off, want_off), f"{what}: block offsets differ first at block {np.flatnonzero(off != want_off)[:1]}"
    assert np.array_equal(bn[:count], want), f"{what}: {(bn[:count] != want).any(1).sum()} records of the destination differ"
    assert np.array_equal(xy[:count], want[:, 0]), f"{what}: the xy list is not the records' first words"
    assert np.array_equal(xy[count:], pre_xy[count:]) and np.array_equal(bn[count:], pre_bn[count:]), f"{what}: words behind the count changed"
    return count


def run_pattern(ctx, n, pattern, dilate):
    rng = np.random.default_rng([n, dilate, sorted(PATTERNS).index(pattern)])
    W, H, rec = production_list(n)
    keep = PATTERNS[pattern](n, rng)
    count = check(ctx, W, H, dilate, mask_of(keep, rec, W, H, rng), rec)
    if not dilate:
        assert count == keep.sum()  # the pattern is what was tested
    if pattern == "none":
        assert count == 0
    if pattern == "all":
        assert count == n


# ---- 1. the kernels against the reference
@pytest.mark.parametrize("dilate", [0, 1])
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_lengths_around_one_block(ctx, pattern, dilate):
    for n in SMALL_N:
        run_pattern(ctx, n, pattern, dilate)


@pytest.mark.parametrize("dilate", [0, 1])
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("n", LARGE_N)
def test_lengths_around_a_wave_and_a_chunk(ctx, n, pattern, dilate):
    run_pattern(ctx, n, pattern, dilate)


@pytest.mark.parametrize("n", SMALL_N[-1:] + LARGE_N)
def test_sparse_mask_with_halos(ctx, n):
    """0.001 of the window's pixels, listed or not, fail: with dilate each keeps its 3 x 3 neighbourhood, which crosses the 64 x 64 tiles of
    the list's order and so the blocks of the list; without, the bytes at unlisted pixels change nothing"""
    W, H, rec = production_list(n)
    mask = (np.random.default_rng(n).random((H, W)) < 0.001).astype(np.uint8)
    assert mask.any()
    plain, halo = check(ctx, W, H, 0, mask, rec), check(ctx, W, H, 1, mask, rec)
    assert plain < halo < n


@pytest.mark.parametrize("dilate", [0, 1])
def test_two_rank_list(ctx, dilate):
    """rank 1 of 2 lists every second tile: the listed pixels have unlisted neighbours, whose mask bytes count under the 3 x 3 rule"""
    W, H, rec = production_list(None, 1, 2, (403, 327))
    assert WAVE // 4 < len(rec) < W * H
    rng = np.random.default_rng(5)
    listed = np.zeros((H, W), bool)
    listed[rec[:, 0] >> 16, rec[:, 0] & 0xFFFF] = True
    for p in (0.001, 0.02):
        mask = (rng.random((H, W)) < p).astype(np.uint8)
        count = check(ctx, W, H, dilate, mask, rec)
        own = int((mask.astype(bool) & listed).sum())
        assert count > own if dilate else count == own
    mask = (~listed).astype(np.uint8)  # only the other rank's pixels: nothing without the 3 x 3 rule, the tiles' rims with it
    count = check(ctx, W, H, dilate, mask, rec)
    assert 0 < count < len(rec) if dilate else count == 0


@pytest.mark.parametrize("window", aw.SMALL_WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
def test_small_windows(ctx, window):
    """every edge and corner pixel listed, the mask just across each edge (adaptive_worlds.edge_masks)"""
    W, H = window
    rec = aw.border_list(W, H)
    for dilate in (0, 1):
        for mask in aw.edge_masks(W, H):
            check(ctx, W, H, dilate, mask, rec)


@pytest.mark.parametrize("window", [(1, 5000), (5000, 1)], ids=["1x5000", "5000x1"])
def test_one_pixel_wide_windows(ctx, window):
    W, H = window
    n = W * H
    rec = np.empty((n, 2), np.uint32)
    rec[:, 0] = np.arange(n) << 16 if W == 1 else np.arange(n)
    rec[:, 1] = np.random.default_rng(n).integers(0, 2 ** 32, n, dtype=np.uint32)
    rng = np.random.default_rng(W)
    flat = [np.arange(n) == 0, np.arange(n) == n - 1, np.arange(n) % TILE == TILE - 1, np.arange(n) % TILE == 0, rng.random(n) < 0.01,
            rng.random(n) < 0.5, np.ones(n, bool), np.zeros(n, bool)]
    for dilate in (0, 1):
        for m in flat:
            count = check(ctx, W, H, dilate, m.astype(np.uint8).reshape(H, W), rec)
            assert count >= m.sum() if dilate else count == m.sum()
        assert check(ctx, W, H, dilate, flat[0].reshape(H, W), rec) == 1 + dilate  # the neighbourhood is clipped at the window's end


# ---- 2. the contract
def test_bad_headers_are_refused():
    c = Context()
    try:
        def raw(W, H, dilate, n_header, n_call):
            inp, out = np.zeros(64, np.uint32), np.zeros(64, np.uint32)
            inp[:4] = W, H, dilate, n_header
            return c.lib.rt3_selftest_eval(c.h, L.SELFTEST_ADAPTIVE_COMPACT, inp.ctypes.data, n_call, out.ctypes.data)

        assert raw(3, 3, 1, 2, 2) == 0, c.last_error()  # two records at pixel (0, 0) fit the buffers
        big = (1 << 24) + 1
        for args in ((0, 3, 0, 2, 2), (3, 0, 0, 2, 2), (65536, 1, 0, 2, 2), (1, 65536, 0, 2, 2), (0xFFFFFFFF, 0xFFFFFFFF, 0, 2, 2), (3, 3, 2, 2, 2),
                     (3, 3, 0xFFFFFFFF, 2, 2), (3, 3, 0, 0, 0), (3, 3, 0, big, big), (3, 3, 0, 0xFFFFFFFF, 0xFFFFFFFF), (3, 3, 0, 2, 3)):
            assert raw(*args) == L.E_INVALID, args
            assert "adaptive compaction header" in c.last_error()
        # a list entry outside the window: x >= W, y >= H, in the first and in the last record
        W, H = 5, 4
        good = aw.border_list(W, H)
        mask = np.ones((H, W), np.uint8)
        for at, xy in ((0, W), (0, H << 16), (len(good) - 1, W | (H - 1) << 16), (len(good) - 1, 0xFFFF), (3, 0xFFFF0000)):
            rec = good.copy()
            rec[at, 0] = xy
            with pytest.raises(L.Rt3Error) as e:
                c.selftest_adaptive_compact(W, H, 1, mask, rec)
            assert e.value.code == L.E_INVALID and f"record {at} " in c.last_error()
        with pytest.raises(L.Rt3Error) as e:
            c.selftest_adaptive_compact(W, H, 2, mask, good)
        assert e.value.code == L.E_INVALID
        # and the context still works
        assert check(c, W, H, 1, mask, good) == len(good)
        _, _, rec = production_list(4096)
        check(c, 67, 62, 0, mask_of(np.arange(4096) % 3 == 0, rec, 67, 62, np.random.default_rng(0)), rec)
    finally:
        c.close()


# ---- 3. one whole frame whose lists cross the chunk boundary
BW, BH, BCAP = aw.BIG_W, aw.BIG_H, aw.BIG_CAP
BIG_CAPS = list(range(aw.MIN_SAMPLES, BCAP + 1, aw.STEP))  # 4, 8, 12


@pytest.fixture(scope="module")
def big():
    """the fixture's scene in the big window; World's cache renders every distinct frame once for the tests below"""
    w = World(window=(BW, BH))
    yield w
    w.close()


def big_runs(w, dilate):
    return [w.adaptive(cap=c, dilate=dilate, threshold=aw.BIG_THRESHOLD[dilate]) for c in BIG_CAPS]


@pytest.mark.parametrize("dilate", [0, 1])
def test_big_frame_bit_exact_against_fixed_frames(big, dilate):
    light, moments, info, depth = big_runs(big, dilate)[-1]
    fg = depth != aw.BACKGROUND_DEPTH
    n = check_against_fixed(big, light, moments, fg, cap=BCAP)
    assert info == (BCAP // aw.STEP, n[fg].sum(), (fg & (n == BCAP)).sum())


@pytest.mark.parametrize("dilate", [0, 1])
def test_big_frame_decisions_follow_the_reference(big, dilate):
    runs = big_runs(big, dilate)
    fg = runs[0][3] != aw.BACKGROUND_DEPTH
    n = check_decisions(runs, BIG_CAPS, fg, aw.big_params(dilate))
    # the guards: the frame does cross the boundaries.  info[2] of a run that ends at its cap is the length of its last list, which is
    # what the test-compaction of the next longer run reads
    early, full = aw.shares(n, fg, BCAP)
    reads = [runs[0][2][2], runs[1][2][2]]
    print(f"dilate={dilate}: foreground {fg.sum()} pixels = {-(-int(fg.sum()) // TILE)} blocks; {early:.3f} stop early, {full:.3f} reach the cap; "
          f"counts {dict(zip(*np.unique(n[fg], return_counts=True)))}; the compactions read {reads}")
    assert fg.sum() > CHUNK and BW * BH > 2 * CHUNK
    assert early >= aw.MIN_SHARE and full >= aw.MIN_SHARE
    assert reads[0] == fg.sum() and reads[0] > CHUNK and reads[1] > WAVE
    assert reads[1] == (fg & (counts_of(runs[1][1], fg) > aw.MIN_SAMPLES)).sum()
