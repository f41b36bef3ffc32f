"""numpy restatement of the skinning rule (raytracer3_amd/csrc/rt3_skin.hpp).  The GPU must equal `pose()` bit for bit,
so with dtype float32 every line that computes a value is ONE rounded device operation on float32 arrays in the device's order, no fused
multiply-add.  With dtype float64 the same lines evaluate the same rule almost exactly: what `rule_bounds` is checked against.

  morph   for t = 0 .. n_targets-1 with a_t != 0:  p = p + a_t * dP[t]   (n the same with dN, when there are normal deltas)
  blend   M = w_k0 * J[j_k0] for the first k0 with w_k0 != 0, then M = M + w_k * J[j_k] for every later k with w_k != 0, entry by entry;
          a row whose four weights are 0 keeps its morphed p and n as they are
  place   p' = ((M.x_axis p.x + M.y_axis p.y) + M.z_axis p.z) + M.w_axis;  n' = normalize(M3x3 n), normalize(a) = a * (1 / sqrt(dot(a, a)))
  uv      copied
  range   every |p'.k| <= 1e18, else the skin's flag

Matrices here are (4, 4) arrays that act on column vectors (M[r, c]), like the ones Context.set_instances takes.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

F = np.float32
U = 2.0 ** -24
RANGE = F(1.0e18)


def _cols(M, v):
    """(M[:, r, 2] * z + (M[:, r, 1] * y + M[:, r, 0] * x)) for r = 0, 1, 2: rt3_surface.hpp's transform_vector"""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([M[:, r, 2] * z + (M[:, r, 1] * y + M[:, r, 0] * x) for r in range(3)], 1)


def transform_point(M, p):
    return (M[:, :3, 3] + _cols(M, p)).astype(M.dtype)


def normalize(a):
    d = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]
    inv = a.dtype.type(1.0) / np.sqrt(d)
    return a * inv[:, None]


def blend(joints, weights, palette, dtype=F):
    """(M (n, 3, 4), any (n,) bool): the blend matrices and which rows have a weight != 0 (the others' M is 0 and unused)"""
    J = np.asarray(palette, F).reshape(-1, 4, 4)[:, :3, :].astype(dtype)
    j = np.asarray(joints, np.int64).reshape(-1, 4)
    w = np.asarray(weights, F).reshape(-1, 4).astype(dtype)
    M = np.zeros((len(j), 3, 4), dtype)
    some = np.zeros(len(j), bool)
    for k in range(4):
        nz = w[:, k] != 0
        term = w[:, k, None, None] * J[j[:, k]]
        first, later = nz & ~some, nz & some
        M[first] = term[first]
        M[later] = M[later] + term[later]
        some |= nz
    return M, some


def pose(rest, joints, weights, palette, target_dpos=None, target_dnrm=None, target_weights=None, dtype=F):
    """the (n, 8) rows k_skin_pose writes for the (n, 8) rest rows, in `dtype`"""
    rest = np.ascontiguousarray(rest, F).reshape(-1, 8)
    p, n = rest[:, 0:3].astype(dtype), rest[:, 3:6].astype(dtype)
    a = np.zeros(0, F) if target_weights is None else np.asarray(target_weights, F).reshape(-1)
    with np.errstate(all="ignore"):
        for t in range(len(a)):
            if a[t] != 0:
                at = dtype(a[t])
                p = p + at * np.asarray(target_dpos, F)[t].astype(dtype)
                if target_dnrm is not None:
                    n = n + at * np.asarray(target_dnrm, F)[t].astype(dtype)
        M, some = blend(joints, weights, palette, dtype)
        p = np.where(some[:, None], transform_point(M, p), p)
        n = np.where(some[:, None], normalize(_cols(M, n)), n)
    return np.ascontiguousarray(np.concatenate([p, n, rest[:, 6:8].astype(dtype)], 1), dtype)


def out_of_range(rows):
    """does a row set the range flag?  (n,) bool"""
    with np.errstate(invalid="ignore"):
        return ~(np.abs(np.asarray(rows)[:, :3]) <= RANGE).all(1)


def gamma(k):
    """Higham's gamma_k = k U / (1 - k U): the relative error k roundings in a row can make"""
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


def rule_bounds(rest, joints, weights, palette, target_dpos=None, target_dnrm=None, target_weights=None):
    """Absolute bounds (bp (n, 3), bn (n, 3)) of pose(float32) against the exact rule, U = 2^-24, derived and not measured.
      T = the row's targets with a_t != 0, K = its weights != 0.  Magnitudes, per component c: S_c = |p_c| + sum_t |a_t| |dP_t,c| bounds every
      partial sum of the morph; A_rc = sum_k |w_k| |J_k,rc| bounds every partial sum of the blend.
      morph: a delta term is rounded once as a product and once per later sum, at most T + 1 roundings; the rest position at most T.
      blend: a term w_k J_k,rc is rounded once as a product and once per later sum: at most K roundings.
      place: M_rc p_c is rounded once as a product and once in each of at most three sums: 4 roundings (3 for a vector, which has no w_axis).
      So every term of p'_r = sum_c M_rc p_c + M_r3 carries at most T + K + 5 roundings and |error| <= gamma(T + K + 5) B_r with
        B_r = sum_c A_rc S_c + A_r3; the vector v = M3x3 n has gamma(T + K + 4) Bn_r with Bn_r = sum_c A_rc Sn_c.
      normalize(v): dot(v, v) has positive terms, 3 U relative; the square root halves that and adds its own: 2.5 U; the reciprocal 3.5 U; the
        product 4.5 U; second order in the next unit: 5.5 U on a unit vector's components.  The error dv of v moves v / |v| by at most
        2 |dv| / |v| (Euclidean norms; true for any dv).  Where 2 |dv| is not below |v| the direction is not determined: the bound is inf.
      K = 0: p' = the morphed p, gamma(T + 1) S; n' = the morphed n, gamma(T + 1) Sn.
      A factor 1 + 2^-20 covers the float64 evaluation the test compares with."""
    rest = np.ascontiguousarray(rest, F).reshape(-1, 8).astype(np.float64)
    a = np.zeros(0) if target_weights is None else np.asarray(target_weights, F).reshape(-1).astype(np.float64)
    S, Sn = np.abs(rest[:, 0:3]), np.abs(rest[:, 3:6])
    T = int(np.count_nonzero(a))
    for t in range(len(a)):
        S = S + abs(a[t]) * np.abs(np.asarray(target_dpos, F)[t].astype(np.float64))
        if target_dnrm is not None:
            Sn = Sn + abs(a[t]) * np.abs(np.asarray(target_dnrm, F)[t].astype(np.float64))
    J = np.abs(np.asarray(palette, F).reshape(-1, 4, 4)[:, :3, :].astype(np.float64))
    j = np.asarray(joints, np.int64).reshape(-1, 4)
    w = np.abs(np.asarray(weights, F).reshape(-1, 4).astype(np.float64))
    A = sum(w[:, k, None, None] * J[j[:, k]] for k in range(4))
    K = np.count_nonzero(w, axis=1)
    B = np.einsum("nrc,nc->nr", A[:, :, :3], S) + A[:, :, 3]
    Bn = np.einsum("nrc,nc->nr", A[:, :, :3], Sn)
    bp = gamma(T + K + 5)[:, None] * B
    dv = gamma(T + K + 4)[:, None] * Bn
    with np.errstate(all="ignore"):
        M, _ = blend(joints, weights, palette, np.float64)
        morphed = pose(rest.astype(F), np.zeros_like(j), np.zeros_like(w), palette, target_dpos, target_dnrm, target_weights, dtype=np.float64)[:, 3:6]
        vlen = np.linalg.norm(_cols(M, morphed), axis=1)
        turn = 2.0 * np.linalg.norm(dv, axis=1) / vlen
        bn = np.where((turn < 1.0)[:, None], 5.5 * U + turn[:, None], np.inf) * np.ones((1, 3))
    zero = K == 0
    bp[zero] = gamma(T + 1) * S[zero]
    bn[zero] = gamma(T + 1) * Sn[zero]
    return bp * (1.0 + 2.0 ** -20), bn * (1.0 + 2.0 ** -20)
