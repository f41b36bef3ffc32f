"""Scenes and the rebuilt reference of the guide-image tests (tests/test_guide.py).

open_material_room(): the material-textured room of tests/test_lens.py placed without its back wall, so that camera rays escape through
the opening and the pixels along its outline are partly covered.  The mesh is that room's; only the instance list leaves the wall out.

sample_features(): what k_lens_guide sees at vertex 0, rebuilt from the library's own parts: the camera function (self-test op 31), a
closest-hit trace of those rays (ctx.trace_rays, the kernels of k_extend) and hit_info (self-test op 29)."""
import numpy as np

from raytracer3_amd import _lib as L
from support import bits

WINDOW = (67, 45)  # no multiple of the 32 x 8 tile, an odd row length


def open_material_room():
    """(mesh, instances, camera)"""
    from test_lens import material_room_world

    mesh, _, cam = material_room_world()
    back = mesh.names.index("back")
    eye = np.eye(4, dtype=np.float32)
    return mesh, [(0, back, eye), (back + 1, len(mesh.names) - back - 1, eye)], cam


def as_f32(words):
    return np.ascontiguousarray(words).view(np.float32)


def sample_features(pt, g, window, lens, px, py, S):
    """Samples 0 .. S-1 of the pixels (px, py) of the frame `g` under `lens`: a dict of arrays with leading shape (S, npix) -- hit, o, d,
    t, bu, bv, prim, normal, albedo, emissive (the last three op 29's words; zeros at a miss)"""
    from test_lens import op31

    npix = len(px)
    PX, PY, SM = np.tile(px, S), np.tile(py, S), np.repeat(np.arange(S), npix)
    o, d, _, _ = op31(pt.ctx, g, window, lens, PX, PY, SM, frame=g.frame)
    n = S * npix
    rays = np.concatenate([o.T, d.T, np.full((1, n), 1e-3, np.float32), np.full((1, n), L.BACKGROUND_DEPTH, np.float32)])
    t, bu, bv, prim, _ = pt.ctx.trace_rays(rays)
    hit = prim != L.MISS
    surf = np.zeros((n, 11), np.float32)
    if hit.any():
        rows = np.stack([prim[hit], bits(bu[hit]), bits(bv[hit])], -1).astype(np.uint32)
        surf[hit] = as_f32(pt.ctx.selftest(L.SELFTEST_HIT_INFO, rows, 11))
    sh = lambda a: a.reshape(S, npix, *a.shape[1:])  # noqa: E731
    return dict(hit=sh(hit), o=sh(o), d=sh(d), t=sh(t), bu=sh(bu), bv=sh(bv), prim=sh(prim), albedo=sh(surf[:, 0:3]), emissive=sh(surf[:, 3:6]),
                normal=sh(surf[:, 6:9]))


def ref_args(f, sl=slice(None)):
    """the arguments of ref_guide.accumulate from sample_features' dict (samples `sl`)"""
    return tuple(f[k][sl] for k in ("hit", "o", "d", "t", "normal", "albedo", "emissive"))


def queue_records(f, sl=slice(None)):
    """op 39's records {o xyz, d xyz, t, bu, bv, prim}, (n, 10) uint32, in path order"""
    o, d = bits(f["o"][sl]).reshape(-1, 3), bits(f["d"][sl]).reshape(-1, 3)
    cols = [bits(f[k][sl]).reshape(-1, 1) for k in ("t", "bu", "bv")]
    return np.concatenate([o, d, *cols, f["prim"][sl].reshape(-1, 1).astype(np.uint32)], -1)
