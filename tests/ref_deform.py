"""numpy float32 restatement of the "motion" pass with previous vertex positions.  The GPU must equal `motion()` and
`deformed_flags()` bit for bit, so every line that computes a texel is ONE rounded device operation on float32 arrays in the device's
order, no fused multiply-add.  Built from the parts of ref_motion (flatten, object_points, transform_point, moved_flags), which this module
imports and does not edit; the temporal side is ref_motion.temporal unchanged.

Texel kinds (Motion.w): 0 miss, 1 and 2 as in ref_motion, 3 the hit geometry is deformed.  A geometry is deformed when some vertex of its
span [vertex_offset + least index, vertex_offset + largest index] differs from the previous positions in one of its three position words,
compared as uint32; a vertex inside the span that no triangle of the geometry indexes counts too.  On a deformed geometry the texel is
M ((a' w + b' u) + c' v) over the triangle's PREVIOUS positions a', b', c', with M the instance's previous matrix when previous transforms
are set and its current matrix otherwise; an exact-identity M (all 16 words) leaves the point as it is.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import orc
import ref_motion as rm

F = np.float32
DEFORMED = F(3.0)


def positions(vertices):
    """(n, 3) float32 position words of an (n, 8) vertex array"""
    return np.ascontiguousarray(np.ascontiguousarray(vertices, F).reshape(-1, 8)[:, :3])


def spans(mesh):
    """per geometry (lo, hi), inclusive, in the vertex buffer; lo > hi for a geometry without triangles"""
    out = []
    idx = np.asarray(mesh.indices, np.int64)
    for g, cnt in zip(mesh.geometries, mesh.prim_counts):
        if int(cnt) == 0:
            out.append((1, 0))
            continue
        io, vo = int(g["index_offset"]), int(g["vertex_offset"])
        own = idx[io:io + 3 * int(cnt)]
        out.append((vo + int(own.min()), vo + int(own.max())))
    return out


def deformed_flags(mesh, prev_vertices):
    """per geometry of `mesh`: does a position word inside its span differ between mesh.vertices and prev_vertices?"""
    cur, prv = positions(mesh.vertices).view(np.uint32), positions(prev_vertices).view(np.uint32)
    assert cur.shape == prv.shape
    differs = (cur != prv).any(1)
    return np.array([bool(differs[lo:hi + 1].any()) if lo <= hi else False for lo, hi in spans(mesh)], bool)


def motion(mesh, prev_vertices, instances, prev_transforms, g, hits, stages=None):
    """the Motion image (H, W, 4) float32 for the hits (t, u, v, prim) of `g`'s primary rays; prev_vertices None = no snapshot"""
    out = rm.motion(mesh, instances, prev_transforms, g, hits, stages=stages)
    if prev_vertices is None:
        return out
    dflags = deformed_flags(mesh, prev_vertices)
    if stages is not None:
        stages.update(deformed=np.zeros(out.shape[:2], bool), geometry_flags=dflags)
    if not dflags.any():
        return out
    t, u, v, prim = (np.asarray(a) for a in hits)
    instances, flat, _ = rm.flatten(mesh, instances)
    hit = prim != np.uint32(orc.MISS)
    pr = prim[hit].astype(np.int64)
    fgeom = np.searchsorted(flat[:, 2], pr, side="right") - 1  # prim_geom
    df = dflags[flat[fgeom, 1]]
    before = SimpleNamespace(geometries=mesh.geometries, indices=mesh.indices, vertices=np.ascontiguousarray(prev_vertices, F).reshape(-1, 8))
    with np.errstate(all="ignore"):
        p, inst = rm.object_points(before, flat, pr[df], u[hit][df].astype(F), v[hit][df].astype(F))
        have_prev = prev_transforms is not None and len(prev_transforms) != 0
        mats = np.stack([np.asarray(m, F) for m in (prev_transforms if have_prev else [m for _, _, m in instances])])
        ident = (mats.view(np.uint32) == rm.EYE_WORDS).reshape(len(mats), -1).all(1)
        pp = np.where(ident[inst][:, None], p, rm.transform_point(mats[inst], p)).astype(F)
    texel = out[hit]
    texel[df] = np.concatenate([pp, np.full((len(pp), 1), DEFORMED, F)], 1)
    out[hit] = texel
    if stages is not None:
        mask = np.zeros(out.shape[:2], bool)
        mask[hit] = df
        prev_obj = np.zeros(out.shape[:2] + (3,), F)
        prev_obj[mask] = p
        stages.update(deformed=mask, prev_object_point=prev_obj)
    return out
