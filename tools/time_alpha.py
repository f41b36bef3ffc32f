#!/usr/bin/env python3
"""Cost of alpha-masked cutout geometry on scenes.cutout_cornell(): frame time and the k_extend / k_shadow time of one
frame (RT3_OPT_PROFILE), for three versions of the same scene:
  opaque       every cutoff 0 and the textures' alpha 255: the unmasked kernels (what the scene costs without masks)
  mask_opaque  the same textures, cutoffs as the scene has them: the MASK kernels, every alpha test passes (the walk is the opaque one's)
  masked       the scene as it is: the MASK kernels, cutaway regions let rays through
Prints one JSON line (medians of --frames timed frames after --warmup).

  python tools/time_alpha.py --size 1920x1080 --spp 16 --bounces 4 --out time_alpha.json
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer, default_camera

    W, H = (int(x) for x in args.size.split("x"))
    mesh = scenes.cutout_cornell()
    solid = [np.concatenate([t[..., :3], np.full(t.shape[:2] + (1,), 255, np.uint8)], -1) for t in mesh.textures]
    g1 = mesh.geometries.copy()
    g1["base_color"][:, 3] = 1.0
    variants = {
        "opaque": assets.Mesh(mesh.vertices, mesh.indices, g1, mesh.prim_counts, list(mesh.names), solid),
        "mask_opaque": assets.Mesh(mesh.vertices, mesh.indices, g1, mesh.prim_counts, list(mesh.names), solid, mesh.alpha_cutoffs),
        "masked": mesh,
    }
    cam = default_camera((W, H), scenes.CORNELL_CAMERA["position"], scenes.CORNELL_CAMERA["direction"], scenes.CORNELL_CAMERA["fov_deg"])
    result = {"scene": "cutout_cornell", "size": [W, H], "spp": args.spp, "bounces": args.bounces, "flags": DEFAULT_FLAGS}
    for name, m in variants.items():
        pt = PathTracer((W, H))
        pt.set_scene(m, scenes.sky(256, 128), assets.load_bluenoise())
        for k in range(args.warmup):
            pt.render(pt.make_gconst(cam, args.spp, args.bounces, frame=k, flags=DEFAULT_FLAGS))
        ms = []
        for k in range(args.frames):
            g = pt.make_gconst(cam, args.spp, args.bounces, frame=k, flags=DEFAULT_FLAGS)
            pt.ctx.wait()
            t0 = time.perf_counter()
            pt.render(g)  # waits for the frame
            ms.append((time.perf_counter() - t0) * 1e3)
        ext, sha = [], []
        pt.ctx.set_option(L.OPT_PROFILE, 1)
        for k in range(args.frames):
            pt.ctx.stats_reset()
            pt.render(pt.make_gconst(cam, args.spp, args.bounces, frame=k, flags=DEFAULT_FLAGS))
            st = pt.ctx.stats()
            ext.append(st.extend_ms)
            sha.append(st.shadow_ms)
        result[name] = {"frame_ms": round(statistics.median(ms), 3), "extend_ms": round(statistics.median(ext), 3),
                        "shadow_ms": round(statistics.median(sha), 3), "frame_ms_all": [round(x, 3) for x in ms]}
        pt.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
