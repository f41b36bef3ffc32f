"""Worlds of the guide-motion tests (tests/test_guide_motion_cpu.py and tests/test_guide_motion.py): the moving and
deforming world of tests/deform_worlds.py, imported, under the three lenses of tests/test_guide.py.  That world is open (no left and no
front wall), so camera rays escape; it has a cloth and bending blocks (deformed), a block that only moves, and a block whose previous
matrix is the identity.  Test infrastructure only.

cpu_samples() makes per-sample features without a GPU: camera rays from tests/ref_lens.py's camera function under seeded uniforms, cast to
float32, and the oracle's closest hits over the same instanced world.  They are not the GPU's samples (those come from
guide_worlds.sample_features), but they are samples of the same frame: what share of them is of which kind is a property of the world
and its camera."""
import copy

import numpy as np

import deform_worlds as dw
import orc
import ref_guide_motion as rgm
import ref_lens as RL

F = np.float32
WINDOW = (67, 45)  # guide_worlds.WINDOW: no multiple of the 32 x 8 tile, an odd row length
LENSES = {"pinhole": (0.0, 1.0, 0.0), "antialiased": (0.0, 1.0, 1.0), "aperture": (0.06, 2.5, 1.0)}  # tests/test_guide.py's
CAMERA = dw.CAMERA
CAMERA_MOVE = ((0.004, 0.0, 0.0), (0.004, 0.0, 0.0))  # per frame of a sequence (test_motion_cpu.QUALITY_MOVE)
S_MAX = 5


def parity():
    """deform_worlds.parity_world() as a dict: frame 1 against frame 0, `bend2`'s previous matrix the identity; `before` is the mesh a
    tracer is built with ahead of the snapshot and the vertex update"""
    mesh, prev_vertices, inst, prev = dw.parity_world()
    before = copy.copy(mesh)
    before.vertices = prev_vertices
    return dict(mesh=mesh, before=before, prev_vertices=prev_vertices, instances=inst, prev_transforms=prev)


CASES = ("both", "transforms", "snapshot", "neither")


def case_args(w, case):
    """(prev_vertices, prev_transforms) of the parity world with previous transforms only, a snapshot only, both, or neither"""
    return (w["prev_vertices"] if case in ("both", "snapshot") else None, w["prev_transforms"] if case in ("both", "transforms") else None)


def gconst(window, samples=S_MAX, frame=4, step=0):
    pos = np.asarray(CAMERA["position"], np.float64) + step * np.asarray(CAMERA_MOVE[0])
    dirn = np.asarray(CAMERA["direction"], np.float64) + step * np.asarray(CAMERA_MOVE[1])
    g = orc.camera_gconst(position=pos, direction=dirn, fov_deg=CAMERA["fov_deg"], width=window[0], height=window[1])
    g.bounces, g.samples, g.frame, g.blendfactor = 3, samples, frame, 1.0
    return g


def cpu_samples(mesh, instances, g, window, lens, S, seed=0):
    """dict of arrays with leading shape (S, npix), every pixel of the window in row-major order: hit, o, d, t, bu, bv, prim"""
    W, H = window
    py, px = (a.reshape(-1) for a in np.mgrid[0:H, 0:W])
    npix = W * H
    rng = np.random.default_rng(seed)
    pinv, vinv = RL.gconst_matrices(g)
    o, d, _, _ = RL.camera_sample(pinv, vinv, window, lens, np.tile(px, S), np.tile(py, S), rng.random((S * npix, 4)))
    o, d = o.astype(F), d.astype(F)
    rays = np.concatenate([o.T, d.T, np.full((1, S * npix), 1e-3, F), np.full((1, S * npix), orc.BACKGROUND_DEPTH, F)])
    t, bu, bv, prim = orc.Scene(mesh, instances=instances).trace_closest(rays)
    sh = lambda a: a.reshape(S, npix, *a.shape[1:])  # noqa: E731
    return dict(hit=sh(prim != np.uint32(orc.MISS)), o=sh(o), d=sh(d), t=sh(t), bu=sh(bu), bv=sh(bv), prim=sh(prim))


def prev_args(f, sl=slice(None)):
    """the sample arguments of ref_guide_motion.previous_points from a feature dict (cpu_samples' or guide_worlds.sample_features')"""
    return tuple(f[k][sl] for k in ("hit", "o", "d", "t", "bu", "bv", "prim"))


def previous_points(w, case, f, sl=slice(None)):
    pv, pm = case_args(w, case)
    return rgm.previous_points(w["mesh"], pv, w["instances"], pm, *prev_args(f, sl))


def kind_shares(w, f):
    """(shares of the samples that escaped, are unmoved, moved, deformed; the number of pixels that mix two kinds among their samples)"""
    kinds = rgm.sample_kinds(w["mesh"], w["prev_vertices"], w["instances"], w["prev_transforms"], f["hit"], f["prim"])
    shares = [float((kinds == k).mean()) for k in (rgm.ESCAPED, rgm.UNMOVED, rgm.MOVED, rgm.DEFORMED)]
    mixed = int(((kinds != kinds[0]).any(0)).sum())
    return shares, mixed
