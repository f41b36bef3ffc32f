"""numpy float32 restatement of the "motion" pass and of the "temporal" pass with a motion input.  The GPU must equal
`motion()` and `temporal()` bit for bit, so every line below is ONE rounded device operation on float32 arrays in the device's order, no
fused multiply-add.  The primary ray is the oracle's (orc.primary_rays); the hits {t, u, v, prim} come from the oracle's closest-hit
traversal of the same instanced world (orc.Scene(mesh, instances=...).trace_closest), which tests/test_gpu_parity.py and
tests/test_instances_two_level.py pin the GPU's hits to.  The surface record, the reprojection and the tap loop are those of
ref_temporal / ref_denoise (ref_temporal.accumulate, which takes the looked-up points R and the `known` mask from here).

Texel kinds (Motion.w): 0 miss, 1 the hit instance did not move, 2 it moved.  "Moved" = the 12 stored floats of the instance's current
matrix (its 3 x 4 part) differ from the previous ones in some 32-bit word.  An exact-identity previous matrix (all 16 words) leaves the
object-space point as it is: the flattening's own rule for positions.
"""
from __future__ import annotations

import numpy as np

import orc
import ref_temporal as rt

F = np.float32
MISS, UNMOVED, MOVED = F(0.0), F(1.0), F(2.0)
EYE_WORDS = np.eye(4, dtype=F).view(np.uint32)


def primary_hits(scene, g):
    """(t, u, v, prim), each (H, W): the closest hits of `g`'s primary rays in the orc.Scene `scene`, row-major over the window"""
    W, H = int(g.window_size[0]), int(g.window_size[1])
    ys, xs = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    t, u, v, p = scene.trace_closest(orc.primary_rays(g, xs.ravel(), ys.ravel()))
    return t.reshape(H, W), u.reshape(H, W), v.reshape(H, W), p.reshape(H, W)


def flatten(mesh, instances):
    """per flattened geometry (instance-major, like rt3_accel_build): (instance, geometry, first primitive)"""
    if not instances:
        instances = [(0, len(mesh.geometries), np.eye(4, dtype=F))]
    rows, total = [], 0
    for i, (first, count, _) in enumerate(instances):
        for k in range(int(count)):
            rows.append((i, int(first) + k, total))
            total += int(mesh.prim_counts[int(first) + k])
    return instances, np.array(rows, np.int64).reshape(-1, 3), total


def moved_flags(instances, prev_transforms):
    """per instance: do the 3 x 4 words of the current and the previous matrix differ?"""
    if prev_transforms is None or len(prev_transforms) == 0:
        return np.zeros(len(instances), bool)
    assert len(prev_transforms) == len(instances)
    cur = np.stack([np.asarray(m, F)[:3] for _, _, m in instances]).view(np.uint32)
    prv = np.stack([np.asarray(m, F)[:3] for m in prev_transforms]).view(np.uint32)
    return (cur != prv).reshape(len(instances), -1).any(1)


def object_points(mesh, flat, prim, u, v):
    """the hit points in object space, (n, 3): p = (a w + b u) + c v with w = (1 - u) - v; a, b, c pair with (w, u, v) like hit_finish"""
    first = flat[:, 2]
    g = np.searchsorted(first, prim, side="right") - 1  # prim_geom
    geom = flat[g, 1]
    io = mesh.geometries["index_offset"][geom].astype(np.int64) + 3 * (prim - first[g])
    vo = mesh.geometries["vertex_offset"][geom].astype(np.int64)
    idx = np.asarray(mesh.indices, np.int64)
    pos = np.ascontiguousarray(mesh.vertices, F).reshape(-1, 8)[:, :3]
    a, b, c = (pos[vo + idx[io + k]] for k in range(3))
    u, v = u[:, None], v[:, None]
    w = (F(1.0) - u) - v
    return (a * w + b * u) + c * v, flat[g, 0]


def transform_point(m, p):
    """glam's transform_point3 as rt3_surface.hpp writes it: w_axis + (z_axis z + (y_axis y + x_axis x)); m (n, 4, 4) row-major, p (n, 3)"""
    x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    return m[:, :3, 3] + (m[:, :3, 2] * z + (m[:, :3, 1] * y + m[:, :3, 0] * x))


def motion(mesh, instances, prev_transforms, g, hits, stages=None):
    """the Motion image (H, W, 4) float32 for the hits (t, u, v, prim) of `g`'s primary rays"""
    t, u, v, prim = (np.asarray(a) for a in hits)
    H, W = t.shape
    instances, flat, _ = flatten(mesh, instances)
    moved_inst = moved_flags(instances, prev_transforms)
    out = np.zeros((H, W, 4), F)
    hit = prim != np.uint32(orc.MISS)
    with np.errstate(all="ignore"):
        P = rt.positions(g, np.where(hit, t, F(0)).astype(F))
        p, inst = object_points(mesh, flat, prim[hit].astype(np.int64), u[hit].astype(F), v[hit].astype(F))
        mv = moved_inst[inst]
        texel = np.concatenate([P[hit], np.full((int(hit.sum()), 1), UNMOVED, F)], 1)
        if mv.any():
            prv = np.stack([np.asarray(m, F) for m in prev_transforms])
            ident = (prv.view(np.uint32) == EYE_WORDS).reshape(len(prv), -1).all(1)
            pm, ii = p[mv], inst[mv]
            pp = np.where(ident[ii][:, None], pm, transform_point(prv[ii], pm)).astype(F)
            texel[mv] = np.concatenate([pp, np.full((len(pp), 1), MOVED, F)], 1)
    out[hit] = texel
    if stages is not None:
        obj = np.zeros((H, W, 3), F)
        obj[hit] = p
        ins = np.full((H, W), -1, np.int64)
        ins[hit] = inst
        stages.update(object_point=obj, instance=ins, hit=hit)
    return out


def temporal(g, gb, depth, light, prev_g, prev_gb, prev_depth, prev_history, prev_moments, motion=None, alpha=0.2, alpha_moments=0.2,
             max_history=32, normal_cos=0.9, plane_tolerance=0.01, flags=0, stages=None):
    """(Out, History, Moments) of the "temporal" pass with the motion input `motion` (H, W, 4): a foreground pixel whose texel has w < 1 has
    no history; otherwise the texel's xyz replaces P in the reprojection (step 3) and in dP = P_q - P' (step 4), while the tolerance, the
    normal and the surface record stay this frame's.  `motion` None is ref_temporal.temporal itself."""
    kw = dict(alpha=alpha, alpha_moments=alpha_moments, max_history=max_history, normal_cos=normal_cos, plane_tolerance=plane_tolerance, flags=flags)
    if motion is None:
        return rt.temporal(g, gb, depth, light, prev_g, prev_gb, prev_depth, prev_history, prev_moments, stages=stages, **kw)
    motion = np.asarray(motion, F)
    R = np.ascontiguousarray(motion[..., :3])  # where this surface point was one frame ago
    known = ~(motion[..., 3] < F(1.0))
    return rt._temporal(g, gb, depth, light, prev_g, prev_gb, prev_depth, prev_history, prev_moments, R, known, stages=stages, **kw)
