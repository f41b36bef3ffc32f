"""numpy float32 restatement of the fifth guide image of a lens frame -- the camera samples' mean previous position, k_lens_guide_prev -- and
of the "temporal" pass that looks it up (k_temporal<TemporalGuideMotion>).  The GPU must equal accumulate_prev() and
temporal() bit for bit, so every line that computes a value is ONE rounded device operation on float32 arrays in the device's order, no
fused multiply-add.

Composed by import, nothing restated: which instances moved (ref_motion.moved_flags) and which geometries are deformed
(ref_deform.deformed_flags), the object-space point (ref_motion.object_points, over the current vertices or over the snapshot's
ref_deform.positions) and the previous matrix on it (ref_motion.transform_point) are the "motion" pass's own parts; the sums run in the
order of ref_guide.accumulate, with the hit count in .w between batches; temporal() is ref_temporal_guide.temporal's body handed
R = image.xyz and an all-true `known` (a foreground pixel has every sample hit, so a point always exists).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import ref_deform as rdf
import ref_guide as rgd
import ref_motion as rm
import ref_temporal as rt
import ref_temporal_guide as rtg

F = np.float32
UNMOVED, MOVED, DEFORMED = 0, 1, 2  # the kind of a hit sample (sample_kinds); ESCAPED for a miss
ESCAPED = -1


def sample_kinds(mesh, prev_vertices, instances, prev_transforms, hit, prim):
    """per sample (the shape of `hit`) int: ESCAPED, UNMOVED, MOVED or DEFORMED -- the rule of the "motion" pass's slot table: a deformed
    geometry is DEFORMED whether or not its instance moved, otherwise a moved instance's is MOVED"""
    hit = np.asarray(hit, bool)
    instances, flat, _ = rm.flatten(mesh, instances)
    moved_inst = rm.moved_flags(instances, prev_transforms)
    dflags = rdf.deformed_flags(mesh, prev_vertices) if prev_vertices is not None else np.zeros(len(mesh.geometries), bool)
    kinds = np.full(hit.shape, ESCAPED, np.int64)
    pr = np.asarray(prim)[hit].astype(np.int64)
    fgeom = np.searchsorted(flat[:, 2], pr, side="right") - 1  # prim_geom
    kinds[hit] = np.where(dflags[flat[fgeom, 1]], DEFORMED, np.where(moved_inst[flat[fgeom, 0]], MOVED, UNMOVED))
    return kinds


def previous_points(mesh, prev_vertices, instances, prev_transforms, hit, o, d, t, bu, bv, prim):
    """R (nsb, npix, 3) float32: where each hit sample's surface point was one frame ago (anything where `hit` is False).
    prev_vertices None = no snapshot; prev_transforms None or empty = none set."""
    hit = np.asarray(hit, bool)
    o, d = np.asarray(o, F), np.asarray(d, F)
    t, bu, bv = (np.asarray(a, F) for a in (t, bu, bv))
    kinds = sample_kinds(mesh, prev_vertices, instances, prev_transforms, hit, prim)
    instances, flat, _ = rm.flatten(mesh, instances)
    have_prev = prev_transforms is not None and len(prev_transforms) != 0
    with np.errstate(all="ignore"):
        R = (o + d * t[..., None]).astype(F)  # unmoved: the addend of the guide's position sum
        for kind in (MOVED, DEFORMED):
            sel = kinds == kind
            if not sel.any():
                continue
            src = mesh
            if kind == DEFORMED:  # the same expression over the snapshot's records
                before = rdf.positions(prev_vertices)  # object_points reads the three position words of 8-word vertices
                src = SimpleNamespace(geometries=mesh.geometries, indices=mesh.indices, vertices=np.pad(before, ((0, 0), (0, 5))))
            p, inst = rm.object_points(src, flat, np.asarray(prim)[sel].astype(np.int64), bu[sel], bv[sel])
            # a moved instance has previous transforms; a deformed geometry without them is put under its current matrix
            mats = np.stack([np.asarray(m, F) for m in (prev_transforms if have_prev else [m for _, _, m in instances])])
            ident = (mats.view(np.uint32) == rm.EYE_WORDS).reshape(len(mats), -1).all(1)
            R[sel] = np.where(ident[inst][:, None], p, rm.transform_point(mats[inst], p)).astype(F)
    return R


def accumulate_prev(hit, R, samples, state=None, first=True, last=True):
    """One batch of k_lens_guide_prev.  hit (nsb, npix) bool; R (nsb, npix, 3) previous_points'; `samples` the frame's sample count S;
    `state` (npix, 4): the image as the previous batch left it (read unless `first`).  Returns (npix, 4) float32: {sum R, n_hit}, or with
    `last` {sum R / n_hit, n_hit / S} (all zero where nothing hit).  The loop is ref_guide.accumulate's, position image only."""
    hit = np.asarray(hit, bool)
    nsb, npix = hit.shape
    R = np.asarray(R, F).reshape(nsb, npix, 3)
    sR = np.zeros((npix, 4), F) if first else np.array(state, F)
    one = F(1.0)
    with np.errstate(all="ignore"):
        for s in range(nsb):
            h = hit[s]
            sR[:, :3] = np.where(h[:, None], sR[:, :3] + R[s], sR[:, :3])
            sR[:, 3] = np.where(h, sR[:, 3] + one, sR[:, 3])
        if last:
            nh = sR[:, 3].copy()
            mean = np.concatenate([sR[:, :3] / nh[:, None], (nh / F(samples))[:, None]], -1)
            sR = np.where((nh > F(0))[:, None], mean, np.zeros((npix, 4), F)).astype(F)
    return sR


def accumulate_prev_split(hit, R, batch):
    """the whole frame in batches of `batch` samples, as RT3_OPT_BATCH_SPP splits it"""
    S = len(hit)
    state = None
    for s0 in range(0, S, batch):
        sl = slice(s0, min(s0 + batch, S))
        state = accumulate_prev(hit[sl], R[sl], S, state, first=s0 == 0, last=s0 + batch >= S)
    return state


def temporal(g, guide, light, prev_g, prev_guide, prev_history, prev_moments, image, alpha=0.2, alpha_moments=0.2, max_history=32,
             normal_cos=0.9, plane_tolerance=0.01, flags=0, stages=None):
    """(Out, History, Moments) of the guided "temporal" with the guide motion input `image` (H, W, 4): ref_temporal_guide.temporal with
    image.xyz in P's place in the reprojection (step 3) and in dP = P_q - R (step 4); the tolerance, the normal and the record stay this
    frame's.  `image` None is ref_temporal_guide.temporal itself."""
    if image is None:
        return rtg.temporal(g, guide, light, prev_g, prev_guide, prev_history, prev_moments, alpha, alpha_moments, max_history, normal_cos,
                            plane_tolerance, flags, stages)
    light = np.ascontiguousarray(light, F)
    image = np.ascontiguousarray(image, F)
    guide, prev_guide = rtg._images(guide), rtg._images(prev_guide, ("position", "normal"))
    with np.errstate(all="ignore"):
        cur = rgd.prepare_guide(guide, light, demodulate=not (flags & rtg.NO_DEMODULATION))
        prev_fg, prev_l2 = rgd.foreground(prev_guide)
        prev = dict(fg=prev_fg, P=prev_guide["position"][..., :3], n=rgd.unit_normal(prev_guide, prev_l2))
        out = rt.accumulate(g, prev_g, light, cur, prev, prev_history, prev_moments, alpha, alpha_moments, max_history, normal_cos, plane_tolerance,
                            stages, R=np.ascontiguousarray(image[..., :3]), known=np.ones(light.shape[:2], bool))
    if stages is not None:
        stages["prev_fg"] = prev_fg
    return out
