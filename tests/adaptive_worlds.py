"""The frames the "adaptive" tests share (test_adaptive_cpu.py on the oracle, test_adaptive.py on the GPU).

The fixture: scenes.cornell() seen from outside, in front of its front wall, under a small sky, 67 x 45 (no multiple of the 256-thread
block or of 64, two tiles of the partition): the window holds the wall in the middle and background around it.  Sky NEE with face-forward
normals lights the wall smoothly, so per-pixel variances spread and the counts take every value 4, 8, ..., 24.  min_samples = step = 4,
cap 24, three bounces.  THRESHOLD[dilate] is picked so that a good share of the foreground pixels stops before the cap and a good share
reaches it: test_adaptive_cpu.py asserts both shares (MIN_SHARE) on oracle frames, test_adaptive.py on the GPU frames."""
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
