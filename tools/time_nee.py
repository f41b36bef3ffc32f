#!/usr/bin/env python3
"""Cost and benefit of RT3_F_NEE_EMISSIVE (DESIGN.md sections 4d and 7) on the benchmark frame: the atrium from the bench camera, with and
without the flag on top of the default flags.  Prints one JSON line: ms per frame (median of --frames timed frames after --warmup), RMSE of
one frame against a flag-less reference of --ref-frames x --spp samples per pixel, and efficiency 1 / (RMSE^2 x time).

  python tools/time_nee.py --size 1920x1080 --spp 64 --bounces 4 --ref-frames 64 --out time_nee.json
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
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--ref-frames", type=int, default=64, help="reference: this many flag-less frames of --spp samples, averaged")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer, default_camera

    W, H = (int(x) for x in args.size.split("x"))
    pt = PathTracer((W, H))
    pt.set_scene(scenes.atrium(args.detail), scenes.sky(2048, 1024), assets.load_bluenoise())
    cam = default_camera((W, H), scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], scenes.ATRIUM_CAMERA["fov_deg"])

    def render(flags, index):
        pt.render(pt.make_gconst(cam, args.spp, args.bounces, frame=index, flags=flags))
        return pt.light()[..., :3].astype(np.float64)

    ref = np.zeros((H, W, 3))
    for k in range(args.ref_frames):
        ref += render(DEFAULT_FLAGS, 10_000 + k)
    ref /= args.ref_frames
    result = {"scene": "atrium", "detail": args.detail, "size": [W, H], "spp": args.spp, "bounces": args.bounces,
              "reference_spp": args.spp * args.ref_frames, "n_emitters": pt.ctx.light_info()[0]}
    for name, flags in (("default", DEFAULT_FLAGS), ("nee_emissive", DEFAULT_FLAGS | L.F_NEE_EMISSIVE)):
        for k in range(args.warmup):
            pt.render(pt.make_gconst(cam, args.spp, args.bounces, frame=k, flags=flags))
        ms = []
        for k in range(args.frames):
            g = pt.make_gconst(cam, args.spp, args.bounces, frame=k, flags=flags)
            pt.ctx.wait()
            t0 = time.perf_counter()
            pt.render(g)  # waits for the frame
            ms.append((time.perf_counter() - t0) * 1e3)
        rmse = float(np.sqrt(np.mean((render(flags, 1) - ref) ** 2)))
        t = statistics.median(ms)
        result[name] = {"flags": flags, "ms": round(t, 3), "ms_all": [round(x, 3) for x in ms], "rmse": rmse, "efficiency": 1.0 / (rmse * rmse * t * 1e-3)}
    result["efficiency_ratio"] = result["nee_emissive"]["efficiency"] / result["default"]["efficiency"]
    pt.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
