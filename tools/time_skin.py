#!/usr/bin/env python3
"""What a skinned frame costs (the table of section 7 "Skinning"): the device path against the host path it replaces.

  python tools/time_skin.py [--details 1.0 1.9] [--joints 64] [--repeats 15] [--warmup 3] [--json time_skin.json]

Worlds: scenes.atrium(detail) with every vertex bound to one skin of --joints joints (four random influences per vertex, a palette of small
rotations and translations that changes from call to call), without targets and with four.
  (a) device     ctx.pose_skin + ctx.refit_accel                                                    host clock; the refit synchronises
  (b) host       a vectorised numpy float32 blend of the same rule + ctx.update_vertices + ctx.refit_accel, the path before skins existed;
      host, fed  the same with the blended vertices computed ahead: upload, synchronise and refit without the host arithmetic
  (c) kernel     k_skin_pose alone, by the HIP events of RT3_OPT_PROFILE (rt3_stats.other_ms over the launches), and the bytes per second it
                 achieves: rest + joints + weights + the record written, per vertex, + the deltas read, + the palette once; against 8 TB/s
Every figure is the median of --repeats runs after --warmup runs, with the least and the largest beside it.  (a) is compared with (b), never
with itself.  Needs the GPU: without one the context cannot be made and the tool fails."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PEAK_BYTES_PER_S = 8.0e12  # MI355X HBM3E


def host_blend(rest, joints, weights, palette, dpos, a):
    """the rule in vectorised float32 numpy, as a caller without skins would write it (sums over all four influences, zero weights included)"""
    p, n = rest[:, 0:3], rest[:, 3:6]
    for t in range(len(a)):
        if a[t] != 0:
            p = p + a[t] * dpos[t]
    J = palette[:, :3, :]
    M = weights[:, 0, None, None] * J[joints[:, 0]]
    for k in range(1, 4):
        M = M + weights[:, k, None, None] * J[joints[:, k]]
    pp = np.einsum("nrc,nc->nr", M[:, :, :3], p) + M[:, :, 3]
    nn = np.einsum("nrc,nc->nr", M[:, :, :3], n)
    nn = nn / np.sqrt(np.einsum("nr,nr->n", nn, nn))[:, None]
    return np.ascontiguousarray(np.concatenate([pp, nn, rest[:, 6:8]], 1), np.float32)


def palette_at(n_joints, k, rng):
    pal = np.tile(np.eye(4, dtype=np.float32), (n_joints, 1, 1))
    ang = 0.02 * (k + 1) * rng.uniform(-1, 1, n_joints)
    pal[:, 0, 0], pal[:, 0, 2], pal[:, 2, 0], pal[:, 2, 2] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang)
    pal[:, :3, 3] = 0.01 * rng.uniform(-1, 1, (n_joints, 3))
    return pal


def timed(fn, repeats, warmup):
    for k in range(warmup):
        fn(k)
    out = []
    for k in range(repeats):
        t0 = time.perf_counter()
        fn(warmup + k)
        out.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--details", type=float, nargs="+", default=[1.0, 1.9])
    ap.add_argument("--joints", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    from raytracer3_amd import _lib as L
    from raytracer3_amd import scenes
    from raytracer3_amd.render_graph import Context

    results = []
    for detail in args.details:
        mesh = scenes.atrium(detail)
        nv = len(mesh.vertices)
        for n_targets in (0, 4):
            rng = np.random.default_rng(17)
            joints = rng.integers(0, args.joints, (nv, 4)).astype(np.uint16)
            w = rng.uniform(0.05, 1.0, (nv, 4))
            weights = (w / w.sum(1, keepdims=True)).astype(np.float32)
            dpos = (0.002 * rng.uniform(-1, 1, (n_targets, nv, 3))).astype(np.float32) if n_targets else None
            a = rng.uniform(0.2, 1.0, n_targets).astype(np.float32)
            rest = np.ascontiguousarray(mesh.vertices, np.float32)
            pals = [palette_at(args.joints, k, rng) for k in range(args.repeats + args.warmup)]
            ctx = Context()
            ctx.upload_mesh(mesh)
            ctx.build_accel()
            skin = ctx.add_skin(0, joints, weights, args.joints, None, dpos)

            def device(k):
                ctx.pose_skin(skin, pals[k], a)
                ctx.refit_accel()

            def host(k):
                ctx.update_vertices(host_blend(rest, joints, weights, pals[k], dpos, a))
                ctx.refit_accel()

            fed = [host_blend(rest, joints, weights, p, dpos, a) for p in pals]

            def host_fed(k):
                ctx.update_vertices(fed[k])
                ctx.refit_accel()

            row = dict(detail=detail, vertices=nv, triangles=int(mesh.n_triangles), joints=args.joints, targets=n_targets,
                       device=timed(device, args.repeats, args.warmup), host=timed(host, args.repeats, args.warmup),
                       host_fed=timed(host_fed, args.repeats, args.warmup))
            # (c) the kernel alone: HIP events around every launch
            ctx.set_option(L.OPT_PROFILE, 1)
            kernel = []
            for k in range(args.warmup + args.repeats):
                ctx.wait()
                ctx.stats_reset()
                ctx.pose_skin(skin, pals[k], a)
                ctx.wait()
                if k >= args.warmup:
                    kernel.append(ctx.stats().other_ms)
            ctx.set_option(L.OPT_PROFILE, 0)
            ctx.refit_accel()
            moved = nv * (32 + 8 + 16 + 32) + n_targets * nv * 12 + args.joints * 48
            med = statistics.median(kernel)
            row["kernel"] = dict(median_ms=med, min_ms=min(kernel), max_ms=max(kernel), bytes=moved, bytes_per_s=moved / (med * 1e-3),
                                 share_of_peak=moved / (med * 1e-3) / PEAK_BYTES_PER_S)
            ctx.close()
            results.append(row)
            print(f"atrium({detail}) {nv} vertices, {args.joints} joints, {n_targets} targets:")
            for name in ("device", "host", "host_fed"):
                r = row[name]
                print(f"  {name:9s} {r['median_ms']:9.3f} ms  [{r['min_ms']:.3f}, {r['max_ms']:.3f}]")
            kr = row["kernel"]
            print(f"  kernel    {kr['median_ms']:9.4f} ms  [{kr['min_ms']:.4f}, {kr['max_ms']:.4f}]  {moved / 1e6:.1f} MB, {kr['bytes_per_s'] / 1e12:.2f} TB/s, "
                  f"{100 * kr['share_of_peak']:.0f} % of 8 TB/s (memory-bound)")
            print(f"  device / host = {row['device']['median_ms'] / row['host']['median_ms']:.3f}, device / host fed = {row['device']['median_ms'] / row['host_fed']['median_ms']:.3f}")
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(results, indent=1))


if __name__ == "__main__":
    main()
