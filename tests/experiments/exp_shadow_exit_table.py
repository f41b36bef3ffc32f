"""CPU experiment behind k_shadow's exit table ("The exit-table round"): oracle only, the any-hit walk in Python.

On the bench frame's shadow rays (scenes.atrium(detail), the bench sky, ATRIUM_CAMERA; vertex 0 = the primary hits, vertex 1 = the hits of a
cosine-weighted bounce from them; directions from orc_scene_sky_sample with uniform numbers; a ray is kept when the geometric normal faces the
direction and the pdf is positive) it prints
  * the occluded share and the steps (node visits + triangle tests) of occluded and unoccluded rays, the oracle's counts beside the walk's;
  * steps per ray under six child orders of the four-wide any-hit walk;
  * how often a per-lane "last occluder" cache would occlude the next ray of the same lane (rays in queue order, 64 lanes);
  * for R = 64 / 256 / 1024: how often the leaf found by an axis-aligned probe from the centre of the ray's exit cell on the root box occludes
    the ray, the probe depth, and the steps per ray of "table step + candidate leaf, then the walk if that fails".

usage: python tests/experiments/exp_shadow_exit_table.py [--detail 1.0] [--width 1920 --height 1080] [--walk-rays 2500] [--table-rays 200000]
The walk is scalar Python: --walk-rays bounds the rays it sees; the table statistics use the oracle's own traversal and take --table-rays."""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import orc  # noqa: E402
from raytracer3_amd import assets, scenes  # noqa: E402

F = np.float32
EMPTY = 0xFFFFFFFF


def pack(o, d, tmin, tmax):
    n = len(o)
    return np.ascontiguousarray(np.concatenate([np.asarray(o, F).T, np.asarray(d, F).T, np.full((1, n), tmin, F), np.full((1, n), tmax, F)]), F)


# ---------------------------------------------------------------------------------------------------------------- the tree, decoded
class Tree:
    def __init__(self, osc):
        self.nodes, self.tris = osc.nodes(), osc.tris()
        w = self.nodes
        self.org = w[:, :3].copy().view(F).astype(np.float64)
        self.step = np.stack([w[:, 3].copy().view(F), w[:, 14].copy().view(F), w[:, 15].copy().view(F)], 1).astype(np.float64)
        self.q = np.ascontiguousarray(w[:, 4:10]).view(np.uint8).reshape(-1, 4, 6).astype(np.float64)
        self.ref = w[:, 10:14]
        self.v = self.tris[:, :9].copy().view(F).reshape(-1, 3, 3).astype(np.float64)
        self.prim = self.tris[:, 9]
        live = (self.ref[0] != EMPTY)
        self.lo = (self.org[0] + self.q[0][live, :3] * self.step[0]).min(0).astype(F)
        self.hi = (self.org[0] + self.q[0][live, 3:] * self.step[0]).max(0).astype(F)
        self.leaf_of = {}
        for r in np.unique(self.ref[(self.ref != EMPTY) & ((self.ref & 0x80000000) != 0)]):
            first, cnt = int(r & 0x0FFFFFFF), int((r >> 28) & 7) + 1
            for j in range(cnt):
                self.leaf_of[int(self.prim[first + j])] = int(r)


def tri_hit(v, o, d, tmin, tmax):
    e1, e2 = v[1] - v[0], v[2] - v[0]
    p = np.cross(d, e2)
    det = e1 @ p
    if det == 0.0:
        return False
    s = o - v[0]
    u = (s @ p) / det
    qv = np.cross(s, e1)
    w = (d @ qv) / det
    t = (e2 @ qv) / det
    return u >= -1e-6 and w >= -1e-6 and u + w <= 1 + 1e-6 and tmin < t < tmax


def leaf_test(tree, ref, o, d, tmin, tmax):
    """(occluded, triangle tests) of one leaf: its triangles in order, stopping at the first that occludes"""
    first, cnt = ref & 0x0FFFFFFF, ((ref >> 28) & 7) + 1
    for j in range(cnt):
        if tri_hit(tree.v[first + j], o, d, tmin, tmax):
            return True, j + 1, int(tree.prim[first + j])
    return False, cnt, None


ORDERS = ("far-first", "farthest exit first", "longest chord first", "slot order", "near-first", "leaves first, then far")


def walk_any(tree, o, d, tmin, tmax, order="far-first"):
    """(occluded, node visits, triangle tests, occluding primitive) of the four-wide any-hit walk under a child order"""
    with np.errstate(divide="ignore"):
        inv = np.where(d != 0.0, 1.0 / d, np.copysign(1e30, d))
    stack, cur, nn, nt = [], 0, 0, 0
    while True:
        if cur & 0x80000000:
            hit, k, prim = leaf_test(tree, cur, o, d, tmin, tmax)
            nt += k
            if hit:
                return True, nn, nt, prim
        else:
            nn += 1
            lo = (tree.org[cur] + tree.q[cur][:, :3] * tree.step[cur] - o) * inv
            hi = (tree.org[cur] + tree.q[cur][:, 3:] * tree.step[cur] - o) * inv
            tn = np.maximum(np.minimum(lo, hi).max(1), tmin)
            tf = np.minimum(np.maximum(lo, hi).min(1), tmax)
            ent = [(k, tn[k], tf[k]) for k in range(4) if tree.ref[cur][k] != EMPTY and tn[k] <= tf[k]]
            if order == "far-first":
                ent.sort(key=lambda e: -e[1])
            elif order == "farthest exit first":
                ent.sort(key=lambda e: -e[2])
            elif order == "longest chord first":
                ent.sort(key=lambda e: -(e[2] - e[1]))
            elif order == "near-first":
                ent.sort(key=lambda e: e[1])
            elif order == "leaves first, then far":
                ent.sort(key=lambda e: (0 if tree.ref[cur][e[0]] & 0x80000000 else 1, -e[1]))
            for e in reversed(ent[1:]):
                stack.append(int(tree.ref[cur][e[0]]))
            if ent:
                cur = int(tree.ref[cur][ent[0][0]])
                continue
        if not stack:
            return False, nn, nt, None
        cur = stack.pop()


# ---------------------------------------------------------------------------------------------------------------- the bench frame's shadow rays
def geometric_normals(mesh, prim):
    t = mesh.triangle_positions().astype(np.float64)[prim]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)


def shadow_rays(osc, mesh, width, height, rng, vertex):
    # primary rays of a pinhole camera at ATRIUM_CAMERA (one through every pixel centre)
    cam_o = np.asarray(scenes.ATRIUM_CAMERA["position"], np.float64)
    fwd = np.asarray(scenes.ATRIUM_CAMERA["direction"], np.float64)
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    th = math.tan(math.radians(scenes.ATRIUM_CAMERA["fov_deg"]) / 2)
    x, y = np.meshgrid((np.arange(width) + 0.5) / width * 2 - 1, 1 - (np.arange(height) + 0.5) / height * 2)
    d0 = fwd + (x.ravel() * th * width / height)[:, None] * right + (y.ravel() * th)[:, None] * up
    d0 /= np.linalg.norm(d0, axis=1, keepdims=True)
    o = np.tile(cam_o, (len(d0), 1))
    t, u, v, p = osc.trace_closest(pack(np.tile(cam_o, (len(o), 1)), d0, 0.0, 1e30))
    keep = p != orc.MISS
    o, p, d0 = (cam_o + d0 * t[:, None])[keep], p[keep], d0[keep]
    n = geometric_normals(mesh, p)
    n[(n * d0).sum(1) > 0] *= -1  # towards the side the ray came from
    if vertex == 1:  # a cosine-weighted bounce, and its hit
        r1, r2 = rng.random(len(o)), rng.random(len(o))
        a = np.where(np.abs(n[:, :1]) < 0.9, [[1.0, 0, 0]], [[0, 1.0, 0]])
        tx = np.cross(n, a)
        tx /= np.linalg.norm(tx, axis=1, keepdims=True)
        ty = np.cross(n, tx)
        ph, sr = 2 * np.pi * r1, np.sqrt(r2)
        d1 = tx * (sr * np.cos(ph))[:, None] + ty * (sr * np.sin(ph))[:, None] + n * np.sqrt(1 - r2)[:, None]
        t, u, v, p = osc.trace_closest(pack(o + 1e-4 * n, d1, 0.0, 1e30))
        keep = p != orc.MISS
        o, p, d0 = (o + 1e-4 * n + d1 * t[:, None])[keep], p[keep], d1[keep]
        n = geometric_normals(mesh, p)
        n[(n * d0).sum(1) > 0] *= -1
    s = osc.sky_sample(rng.random((len(o), 2)))
    d = s[:, :3].copy().view(F).astype(np.float64)
    pdf = s[:, 6].copy().view(F)
    keep = ((n * d).sum(1) > 0) & (pdf > 0)
    return pack(o[keep] + 1e-4 * n[keep], d[keep], 0.0, 1e5)


# ---------------------------------------------------------------------------------------------------------------- the exit table
def exit_cells(rays, lo, hi, R):
    o, d = rays[:3].T.astype(F), rays[3:6].T.astype(F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = np.where(d != 0, F(1) / d, np.copysign(F(1e30), d)).astype(F)
        t = ((np.where(inv < 0, lo, hi) - o) * inv).astype(F)
        ax = np.argmin(t, 1)
        k = np.arange(len(t))
        ext = hi - lo
        scale = np.where(ext > 0, F(R) / np.where(ext > 0, ext, 1), 0).astype(F)
        c = np.nan_to_num(((o + t[k, ax][:, None] * d - lo) * scale).astype(F))
    iu = np.clip(c[k, (ax + 1) % 3], 0, R - 1).astype(np.int64)
    iv = np.clip(c[k, (ax + 2) % 3], 0, R - 1).astype(np.int64)
    return ((2 * ax + (inv[k, ax] >= 0)) * R + iv) * R + iu


def probe_rays(lo, hi, R):
    i = np.arange(6 * R * R)
    iu, iv, face = i % R, (i // R) % R, i // (R * R)
    ax, high = face >> 1, face & 1
    ext = (hi - lo).astype(F)
    pad = max(float(ext.max()) * 1e-3, float(np.abs(np.concatenate([lo, hi])).max()) * 1e-5, 1e-6)
    o, d, k = np.zeros((len(i), 3), F), np.zeros((len(i), 3), F), np.arange(len(i))
    au, av = (ax + 1) % 3, (ax + 2) % 3
    o[k, au] = lo[au] + (iu + F(0.5)) * (ext[au] / F(R))
    o[k, av] = lo[av] + (iv + F(0.5)) * (ext[av] / F(R))
    o[k, ax] = np.where(high, hi[ax] + pad, lo[ax] - pad)
    d[k, ax] = np.where(high, -1, 1)
    return pack(o, d, 0.0, 1e5), pad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--walk-rays", type=int, default=2500)
    ap.add_argument("--table-rays", type=int, default=200000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    mesh = scenes.atrium(a.detail)
    osc = orc.Scene(mesh, scenes.sky(2048, 1024), assets.load_bluenoise())
    tree = Tree(osc)
    print("root box", tree.lo, tree.hi, "nodes", osc.n_nodes, "triangles", osc.n_tris)
    for vertex in (0, 1):
        rays = shadow_rays(osc, mesh, a.width, a.height, rng, vertex)
        first = int(rng.integers(0, max(1, rays.shape[1] - a.table_rays + 1)))
        rays = rays[:, first : first + a.table_rays]  # a run of consecutive rays: the queue's order, which the cache experiment needs
        occ, nn, nt = osc.trace_any(rays, counts=True)
        occ = occ != 0
        print(f"\nvertex {vertex}: {rays.shape[1]} shadow rays, occluded {occ.mean():.3f}; oracle steps per ray {nn.mean():.2f} nodes + {nt.mean():.2f} triangles"
              f" (occluded {nn[occ].mean():.1f} + {nt[occ].mean():.2f}, unoccluded {nn[~occ].mean():.1f} + {nt[~occ].mean():.2f})")
        m = min(a.walk_rays, rays.shape[1])
        sub = rays[:, :m].astype(np.float64)
        last = [None] * 64
        cache_hits = 0
        for order in ORDERS:
            steps = 0
            for i in range(m):
                hit, wn, wt, prim = walk_any(tree, sub[:3, i], sub[3:6, i], sub[6, i], sub[7, i], order)
                steps += wn + wt
                if order == "far-first":
                    c = last[i % 64]
                    if c is not None and leaf_test(tree, tree.leaf_of[c], sub[:3, i], sub[3:6, i], sub[6, i], sub[7, i])[0]:
                        cache_hits += 1
                    if hit:
                        last[i % 64] = prim
            extra = f" (oracle on the same rays: {(nn[:m] + nt[:m]).mean():.2f})" if order == "far-first" else ""
            print(f"  order {order:>24}: {steps / m:6.2f} steps per ray{extra}")
        print(f"  last-occluder cache (64 lanes, queue order): the cached leaf occludes {cache_hits / m:.3f} of the rays")
        for R in (64, 256, 1024):
            pr, pad = probe_rays(tree.lo, tree.hi, R)
            pt, _, _, pp = osc.trace_closest(pr)
            cand = pp[exit_cells(rays, tree.lo, tree.hi, R)]
            ok = np.zeros(rays.shape[1], bool)
            tests = np.zeros(rays.shape[1])
            for i in np.flatnonzero(cand != orc.MISS)[: 20 * a.walk_rays]:
                ok[i], tests[i], _ = leaf_test(tree, tree.leaf_of[int(cand[i])], rays[:3, i].astype(np.float64), rays[3:6, i].astype(np.float64), rays[6, i], rays[7, i])
            seen = np.zeros(rays.shape[1], bool)
            seen[np.flatnonzero(cand != orc.MISS)[: 20 * a.walk_rays]] = True
            seen |= cand == orc.MISS
            steps = 1 + tests[seen] + np.where(ok[seen], 0, (nn + nt)[seen])
            print(f"  R {R:5d}: candidate occludes {ok[seen].mean():.3f} of all rays, {ok[seen & occ].mean():.3f} of the occluded; probe depth median"
                  f" {np.median(pt[pp != orc.MISS]) - pad:.3f}; steps per ray {(nn + nt)[seen].mean():.2f} -> {steps.mean():.2f}; table {6 * R * R * 4 / 1e6:.1f} MB")


if __name__ == "__main__":
    main()
