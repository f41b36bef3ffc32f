"""The frames the "adaptive" tests share (test_adaptive_cpu.py on the oracle, test_adaptive.py on the GPU).

The fixture: scenes.cornell() seen from outside, in front of its front wall, under a small sky, 67 x 45 (no multiple of the 256-thread
block or of 64, two tiles of the partition): the window holds the wall in the middle and background around it.  Sky NEE with face-forward
normals lights the wall smoothly, so per-pixel variances spread and the counts take every value 4, 8, ..., 24.  min_samples = step = 4,
cap 24, three bounces.  THRESHOLD[dilate] is picked so that a good share of the foreground pixels stops before the cap and a good share
reaches it: test_adaptive_cpu.py asserts both shares (MIN_SHARE) on oracle frames, test_adaptive.py on the GPU frames.

The big frame (test_adaptive_compaction.py): the same scene, camera, flags, bounces and frame number at BIG_W x BIG_H = 1400 x 940, so
that the pass's list compaction (rt3_adaptive.hip: 2048 entries per block, a scan of 64 block counts per wave and 256 per chunk) crosses
the boundaries the 67 x 45 window's two blocks never reach.  The cap is BIG_CAP = 12 with min_samples = step = 4: three rounds, two
test-compactions.  BIG_THRESHOLD[dilate] was picked on the CPU oracle, not on what the pass does: per-sample luminances rebuilt from oracle
frames of samples = 1 .. 12 (test_adaptive_cpu.oracle_samples) and ref_adaptive.simulate over them.
    foreground: 545 222 of 1 316 000 pixels = 267 blocks (more than one chunk of 256); round 0 compacts the whole window, 643 blocks
    dilate 0, threshold 0.20: counts {4: 145 904, 8: 204 251, 12: 195 067}: 0.642 stop early, 0.358 reach the cap;
                              the test-compactions read 545 222 entries (267 blocks), then 399 318 (195 blocks: four waves of one chunk)
    dilate 1, threshold 0.25: counts {4: 611, 8: 192 978, 12: 351 633}: 0.355 stop early, 0.645 reach the cap;
                              the test-compactions read 545 222 entries, then 544 611 (266 blocks)
The shares do not depend on the resolution (268 x 180: 0.638 / 0.362 and 0.360 / 0.640), but they do on the cap: the small fixture's
thresholds (0.12 / 0.15 at cap 24) leave 0.12 and 0.00 stopping before cap 12.  test_adaptive_cpu.py repeats the computation and asserts
the shares (MIN_SHARE) and the list lengths; test_adaptive_compaction.py asserts them again on the GPU frames.  The GPU's counts are the
oracle's for dilate 0; for dilate 1 they are {4: 611, 8: 192 984, 12: 351 627}, six pixels of 545 222 stopping one round earlier: the
prediction's moments are float64 sums of samples rebuilt from frame means, the pass's are float32 running sums of the samples themselves
(test_adaptive.test_moments_against_float64 bounds the difference), and a pixel within that rounding of the threshold decides otherwise.
The pass's decisions are held exactly to ref_adaptive.next_active on its own moments."""
import math

import numpy as np

from raytracer3_amd import scenes
from raytracer3_amd.assets import Material, MeshBuilder

W, H = 67, 45
CAMERA = dict(position=(0.15, 1.05, 7.5), direction=(0.01, -0.005, -1.0), fov_deg=40.0)
BOUNCES, CAP, MIN_SAMPLES, STEP = 3, 24, 4, 4
THRESHOLD, DARK = {0: 0.12, 1: 0.15}, 0.01  # per dilate setting: the dilation keeps more pixels going
FLAGS = 1 | 8  # RT3_F_NEE_SKY | RT3_F_FACEFORWARD
SKY_SIZE = (64, 32)
ONE_PIXEL_FRAME = 1  # a frame number whose first four samples of the one-pixel world's centre pixel differ (asserted on the oracle)
MIN_SHARE = 0.15
FRAME = 3
BACKGROUND_DEPTH = np.float32(100000.0)
BIG_W, BIG_H, BIG_CAP = 1400, 940, 12
BIG_THRESHOLD = {0: 0.20, 1: 0.25}
COMPACT_TILE, SCAN_WAVE, SCAN_CHUNK = 2048, 64, 256  # entries per compaction block; block counts per wave and per chunk of the scan
SMALL_WINDOWS = [(1, 1), (1, 7), (7, 1), (3, 3), (5, 4)]  # (W, H): windows whose every pixel is at an edge or next to one


def big_params(dilate):
    """params() for the big frame"""
    return params(dilate=dilate, threshold=BIG_THRESHOLD[dilate])


def border_list(w, h, seed=0):
    """(n, 2) list records {x | y << 16, random word}: every edge and corner pixel of a w x h window, row-major"""
    y, x = np.mgrid[0:h, 0:w]
    edge = (x == 0) | (x == w - 1) | (y == 0) | (y == h - 1)
    rec = np.empty((int(edge.sum()), 2), np.uint32)
    rec[:, 0] = x[edge] | (y[edge] << 16)
    rec[:, 1] = np.random.default_rng(seed).integers(0, 2 ** 32, len(rec), dtype=np.uint32)
    return rec


def edge_masks(w, h):
    """Masks (h, w) of bytes that sit just across a listed pixel's edge: every single-pixel mask (the byte one step past the end of a row
    is the first of the next row: a 3 x 3 rule that wraps around keeps an edge pixel it should drop), the empty and the full mask, each
    row and each column alone, and non-zero bytes other than 1."""
    masks = [np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)]
    for i in range(w * h):
        m = np.zeros(w * h, np.uint8)
        m[i] = (1, 2, 0x80, 0xFF)[i % 4]
        masks.append(m.reshape(h, w))
    for r in range(h):
        m = np.zeros((h, w), np.uint8)
        m[r] = 1
        masks.append(m)
    for c in range(w):
        m = np.zeros((h, w), np.uint8)
        m[:, c] = 1
        masks.append(m)
    return masks


def params(**kw):
    """keyword arguments of Context.adaptive_set_params for the fixture"""
    p = dict(min_samples=MIN_SAMPLES, step=STEP, dark=DARK, dilate=1, flags=0)
    p.update(kw)
    p.setdefault("threshold", THRESHOLD[p["dilate"]])
    return p


def sky():
    return scenes.sky(*SKY_SIZE)


def shares(n, fg, cap=CAP):
    """(share of the foreground pixels that stopped before the cap, share that reached it)"""
    total = int(fg.sum())
    return float((fg & (n < cap)).sum()) / total, float((fg & (n == cap)).sum()) / total


def one_pixel_world():
    """Black surfaces (albedo 0: whatever a bounce finds is multiplied by 0) except one small grey quad on the camera's axis that covers
    the centre pixel of the odd-sized window and no other pixel's centre; an emitter behind the camera covers part of its hemisphere.
    With two bounces and the emissive-only estimator, that pixel's samples are albedo x (emission or 0); every other foreground pixel's
    are constant.  Returns (mesh, camera dict)."""
    black, grey = Material((0.0, 0.0, 0.0)), Material((0.8, 0.8, 0.8))
    lamp = Material((0.0, 0.0, 0.0), emission=(1.0, 0.9, 0.8))
    mb = MeshBuilder()
    grid = scenes._grid
    mb.add("wall", *grid([-0.61, -0.43, -3.0], [1.2, 0, 0], [0, 0.8, 0], 2, 2), black)        # part of the window: background around it
    # a pixel is 2 tan(20 deg) / 45 = 0.0162 wide at distance 1: the quad's half width is a quarter of that
    mb.add("speck", *grid([-0.003, -0.005, -1.0], [0.008, 0, 0], [0, 0.008, 0], 1, 1), grey)  # (its diagonal misses the axis)
    mb.add("lamp", *grid([0.0, -3.0, 0.5], [0, 6.0, 0], [3.0, 0, 0], 1, 1), lamp)           # behind the camera, over x > 0, facing -z
    return mb.build(), dict(position=(0.0, 0.0, 0.0), direction=(0.0, 0.0, -1.0), fov_deg=40.0)


def instanced_world():
    """the Cornell room under the identity and its tall block placed three more times (translations): (mesh, instances)"""
    room = scenes.cornell()
    t = room.names.index("tall")
    inst = [(0, len(room.names), np.eye(4, dtype=np.float32))]
    for dx, dz in ((0.9, 1.4), (0.2, 2.2), (1.1, 2.9)):
        m = np.eye(4, dtype=np.float32)
        m[0, 3], m[2, 3] = dx, dz
        inst.append((t, 1, m))
    return room, inst


def fov(cam):
    return math.radians(cam["fov_deg"])
