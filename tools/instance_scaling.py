"""Instance scaling: P placements of one ~50 k-triangle mesh under random rotations and translations, in both instance modes
(RT3_OPT_INSTANCE_MODE 0 = flatten, 1 = two-level).  Per (P, mode): accel_bytes; rt3_stats.accel_build_ms of a
second build with nothing changed (in mode 1 every bottom tree is cached by then) and of a build after one instance moved; k_extend Mrays/s
with nodes / triangles per ray on a primary batch and on a secondary batch (diffuse directions from the primary hits, the shape of a
bounce-1 batch).  Prints a markdown table (profiles/instances_two_level.md).

    python tools/instance_scaling.py [--placements 1 8 64 512] [--detail 0.45] [--res 512] [--repeat 10]
"""
from __future__ import annotations

import argparse
import math
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from raytracer3_amd import _lib as L  # noqa: E402
from raytracer3_amd import scenes  # noqa: E402
from raytracer3_amd.render_graph import Context  # noqa: E402


def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def world(mesh, P, seed=1):
    rng = np.random.default_rng(seed)
    side = 40.0 * P ** (1.0 / 3.0)
    inst = []
    for _ in range(P):
        m = np.eye(4)
        m[:3, :3] = rotation(rng)
        m[:3, 3] = rng.uniform(-side / 2, side / 2, 3) if P > 1 else 0.0
        inst.append((0, len(mesh.geometries), m.astype(np.float32)))
    return inst, side


def primary(res, side):
    eye = np.array([0.0, 0.0, -1.5 * side - 30.0])
    fov = 2.0 * math.atan((side / 2 + 20.0) / (1.5 * side + 30.0))
    ys, xs = np.mgrid[0:res, 0:res]
    px = ((xs.ravel() + 0.5) / res * 2 - 1) * math.tan(fov / 2)
    py = ((ys.ravel() + 0.5) / res * 2 - 1) * math.tan(fov / 2)
    d = np.stack([px, py, np.ones_like(px)])
    d /= np.linalg.norm(d, axis=0)
    n = d.shape[1]
    o = np.repeat(eye[:, None], n, 1)
    return np.ascontiguousarray(np.concatenate([o, d, np.zeros((1, n)), np.full((1, n), 1e5)]), np.float32)


def secondary(rays, t, p, seed=2):
    hit = p != L.MISS
    o = rays[:3, hit] + rays[3:6, hit] * t[hit]
    rng = np.random.default_rng(seed)
    d = rng.normal(size=o.shape)
    d /= np.linalg.norm(d, axis=0)
    back = -rays[3:6, hit]
    d = np.where((d * back).sum(0) < 0, -d, d)  # the hemisphere the primary ray came from
    n = o.shape[1]
    return np.ascontiguousarray(np.concatenate([o, d, np.full((1, n), 1e-3), np.full((1, n), 1e5)]), np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--placements", type=int, nargs="+", default=[1, 8, 64, 512])
    ap.add_argument("--detail", type=float, default=0.45)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=10)
    a = ap.parse_args()
    mesh = scenes.atrium(a.detail)
    print(f"mesh: scenes.atrium({a.detail}), {mesh.n_triangles} triangles; primary batch {a.res}x{a.res}; k_extend averaged over {a.repeat} launches\n")
    print("| P | mode | accel MiB | warm rebuild ms | move rebuild ms | primary Mrays/s | nodes/ray | tris/ray | secondary Mrays/s | nodes/ray | tris/ray |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for P in a.placements:
        inst, side = world(mesh, P)
        rays = primary(a.res, side)
        sec = None
        for mode in (0, 1):
            ctx = Context(0)
            try:
                ctx.upload_mesh(mesh)
                ctx.set_instances(inst)
                ctx.set_option(L.OPT_INSTANCE_MODE, mode)
                try:
                    ctx.build_accel()
                except L.Rt3Error as e:
                    print(f"| {P} | {mode} | {e} | | | | | | | | |")
                    continue
                ctx.stats_reset()
                ctx.build_accel()
                full_ms = ctx.stats().accel_build_ms
                moved = list(inst)
                m = moved[0][2].copy()
                m[:3, 3] += 1.0
                moved[0] = (moved[0][0], moved[0][1], m)
                ctx.set_instances(moved)
                ctx.stats_reset()
                ctx.build_accel()
                move_ms = ctx.stats().accel_build_ms
                ctx.set_instances(inst)
                ctx.build_accel()
                nbytes = ctx.accel_levels()[3]
                row = [f"{nbytes / 2**20:.2f}", f"{full_ms:.2f}", f"{move_ms:.2f}"]
                t, u, v, p, _ = ctx.trace_rays(rays)
                if sec is None:
                    sec = secondary(rays, t, p)
                for batch in (rays, sec):
                    n = batch.shape[1]
                    _, _, _, _, ms = ctx.trace_rays(batch, repeat=a.repeat)
                    ctx.set_option(L.OPT_COUNT_TRAVERSAL, 1)
                    _, _, _, _, cn, ct, _ = ctx.trace_rays(batch, counts=True)
                    ctx.set_option(L.OPT_COUNT_TRAVERSAL, 0)
                    row += [f"{n / ms / 1e3:.0f}", f"{cn.mean():.1f}", f"{ct.mean():.1f}"]
                print(f"| {P} | {mode} | " + " | ".join(row) + " |", flush=True)
            finally:
                ctx.close()


if __name__ == "__main__":
    main()
