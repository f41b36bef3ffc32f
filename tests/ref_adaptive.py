"""numpy float32 restatement of the "adaptive" pass's decisions (include/rt3.h, rt3_adaptive_set_params): the
convergence predicate in the header's operation order, the 3 x 3 dilation and the schedule.  Every float32 operation is one numpy
float32 operation, so the results are singly rounded like the kernels' (-ffp-contract=off, IEEE divide).

A state image is (H, W) arrays S1, S2 (float32) and n (integer); `fg` marks the foreground pixels of the rank's list (background,
out-of-window and foreign pixels count as passing) and `active` the pixels that have not stopped."""
import numpy as np

F = np.float32
LUMA = (F(0.299), F(0.587), F(0.114))  # math.slang:119-122, rt3_math.hpp luminance()


def luminance(rgb):
    """(c.x * 0.299 + c.y * 0.587) + c.z * 0.114 in float32, left to right"""
    c = np.asarray(rgb, F)
    return (c[..., 0] * LUMA[0] + c[..., 1] * LUMA[1]) + c[..., 2] * LUMA[2]


def passes(S1, S2, n, threshold, dark):
    """the predicate per pixel: mean = S1 / n; var = (S2 - S1 mean) / (n - 1), 0 if negative; rel = threshold (mean + dark);
    var <= (rel rel) n.  n >= 2."""
    S1, S2, nf = np.asarray(S1, F), np.asarray(S2, F), np.asarray(n).astype(F)
    with np.errstate(all="ignore"):
        mean = S1 / nf
        var = (S2 - S1 * mean) / (nf - F(1))
        var = np.where(var < F(0), F(0), var)
        rel = F(threshold) * (mean + F(dark))
        return var <= (rel * rel) * nf


def dilate3(fail):
    """a pixel is set when any pixel of its 3 x 3 neighbourhood inside the window is"""
    H, W = fail.shape
    p = np.zeros((H + 2, W + 2), bool)
    p[1:-1, 1:-1] = fail
    out = np.zeros((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + H, dx:dx + W]
    return out


def next_active(S1, S2, n, active, fg, threshold, dark, dilate):
    """After a round: the pixels that stay active, and the counts (active before, failed, staying).  A stopped pixel never restarts."""
    active = np.asarray(active, bool) & np.asarray(fg, bool)
    fail = active & ~passes(S1, S2, np.maximum(n, 2), threshold, dark)
    stay = active & (dilate3(fail) if dilate else fail)
    return stay, dict(active=int(active.sum()), failed=int(fail.sum()), staying=int(stay.sum()))


TILE = 2048  # list entries per block of the compaction (rt3_adaptive.hip: kAdTile)


def keeps(records, mask, W, H, dilate):
    """per record of a list ((n, 2) words {x | y << 16, blue-noise word}): does it stay -- its pixel's byte of the window-space mask (H, W)
    is non-zero or, with dilate, any byte of the 3 x 3 neighbourhood inside the window is"""
    m = np.asarray(mask).reshape(H, W) != 0
    if dilate:
        m = dilate3(m)
    xy = np.asarray(records, np.uint32).reshape(-1, 2)[:, 0]
    return m[(xy >> 16).astype(np.int64), (xy & 0xFFFF).astype(np.int64)]


def block_offsets(records, mask, W, H, dilate):
    """what the scan leaves: per TILE-entry tile of the list, the number of kept entries in front of it"""
    k = keeps(records, mask, W, H, dilate)
    per_tile = np.add.reduceat(k.astype(np.int64), np.arange(0, len(k), TILE)) if len(k) else np.zeros(0, np.int64)
    return np.cumsum(per_tile) - per_tile


def compact(records, mask, W, H, dilate):
    """The list after a compaction: (the kept records in the list's order, block_offsets(...)).  Integer work: exact."""
    records = np.asarray(records, np.uint32).reshape(-1, 2)
    return records[keeps(records, mask, W, H, dilate)], block_offsets(records, mask, W, H, dilate)


def round_samples(n, min_samples, step, cap):
    """the samples the round that starts at count n hands out"""
    return min(min_samples, cap) if n == 0 else min(step, cap - n)


def simulate(y, fg, cap, min_samples=16, step=16, threshold=0.05, dark=0.01, dilate=1, flags=0):
    """The whole loop over per-sample luminances y[k] ((cap, H, W), sample k of every pixel): returns n, S1, S2 (the Moments' first three
    channels), rounds, paths traced and pixels capped."""
    fg = np.asarray(fg, bool)
    H, W = fg.shape
    S1, S2, n = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), np.int64)
    active, done, rounds, paths = fg.copy(), 0, 0, 0
    while active.any():
        ns = round_samples(done, min_samples, step, cap)
        for k in range(done, done + ns):
            yk = np.asarray(y[k], F)
            S1 = np.where(active, S1 + yk, S1).astype(F)
            S2 = np.where(active, S2 + yk * yk, S2).astype(F)
        n = np.where(active, done + ns, n)
        done += ns
        rounds += 1
        paths += ns * int(active.sum())
        if done >= cap:
            break
        active, _ = next_active(S1, S2, n, active, fg, threshold, dark, dilate)
    capped = int((fg & (n == cap)).sum())
    return n, S1, S2, rounds, paths, capped
