#!/usr/bin/env python3
"""Refit against rebuild (DESIGN.md sections 4c and 7): what rt3_accel_refit costs next to rt3_accel_build, and what a refitted tree costs
the traversal as the vertices drift further from the ones the tree was built for.

For atrium(1.0) and atrium(1.9): the median of 10 builds and of 10 refits after warm-up (host clock around stream-synchronised calls); then,
for smooth wave displacements of 0 %, 0.5 %, 2 % and 10 % of the scene extent, the closest-hit and any-hit kernel time of rt3_trace_rays
(`kernel_ms`, 2^21 random rays, repeat 5) on the refitted tree and on a tree rebuilt over the same vertices."""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from raytracer3_amd import scenes  # noqa: E402
from raytracer3_amd.render_graph import Context  # noqa: E402

N_RAYS = 1 << 21


def wave(v0, amplitude):
    v = v0.copy()
    p = v[:, :3].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    ext = float((hi - lo).max())
    s = (p - lo) / ext
    d = np.stack([np.sin(2 * np.pi * (s[:, 1] + s[:, 2])), np.sin(2 * np.pi * (s[:, 0] - s[:, 2])), np.cos(2 * np.pi * (s[:, 0] + s[:, 1]))], 1)
    v[:, :3] = (p + amplitude * ext * d).astype(np.float32)
    return v


def rays_in(v, seed=0):
    rng = np.random.default_rng(seed)
    p = v[:, :3]
    lo, hi = p.min(0), p.max(0)
    o = rng.uniform(lo, hi, (N_RAYS, 3))
    d = rng.normal(size=(N_RAYS, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([o.T, d.T, np.zeros((1, N_RAYS)), np.full((1, N_RAYS), 1e30)]), np.float32)


def clock(ctx, fn, n=10, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        ctx.wait()
        t0 = time.perf_counter()
        fn()
        ctx.wait()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def main():
    print("| scene | triangles | build ms | refit ms | amplitude | closest refit / rebuilt ms | any refit / rebuilt ms |")
    print("|---|---|---|---|---|---|---|")
    for detail in (1.0, 1.9):
        mesh = scenes.atrium(detail)
        rf, rb = Context(0), Context(0)
        try:
            for c in (rf, rb):
                c.upload_mesh(mesh)
                c.build_accel()
            t_build = clock(rf, rf.build_accel)
            t_refit = clock(rf, rf.refit_accel)
            rays = rays_in(mesh.vertices)
            for amp in (0.0, 0.005, 0.02, 0.10):
                v = wave(mesh.vertices, amp)
                rf.update_vertices(v)
                rf.refit_accel()
                rb.update_vertices(v)
                rb.build_accel()
                ms = {}
                for name, c in (("refit", rf), ("rebuilt", rb)):
                    ms[name] = (c.trace_rays(rays, repeat=5)[-1], c.trace_rays(rays, any_hit=True, repeat=5)[-1])
                print(f"| atrium({detail}) | {mesh.n_triangles} | {t_build:.2f} | {t_refit:.2f} | {100 * amp:g} % | "
                      f"{ms['refit'][0]:.3f} / {ms['rebuilt'][0]:.3f} | {ms['refit'][1]:.3f} / {ms['rebuilt'][1]:.3f} |", flush=True)
                rf.update_vertices(mesh.vertices)  # every amplitude starts from the tree built on the undeformed scene
                rf.build_accel()
        finally:
            rf.close()
            rb.close()


if __name__ == "__main__":
    main()
