#!/usr/bin/env python3
"""Cost of RT3_F_NEE_PUNCTUAL (DESIGN.md sections 4k and 7) on the benchmark frame: the atrium from the bench camera with 0, 1 and 16
punctual lights, with and without RT3_F_NEE_EMISSIVE, on top of the default flags.  The six configurations are visited in turn, --rounds
times over, so that drift of the machine lands on all of them alike; each visit renders --warmup frames (the first remakes the light
table) and then times --frames frames (host clock around a waited frame).  Prints one JSON line: per configuration the median over all
its timed frames, the median of each round, and the shadow rays per frame (rt3_stats.shadow_rays: sky, emitter and light shadow rays).

  python tools/time_lights.py --size 1920x1080 --spp 64 --bounces 4 --out time_lights.json
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


def atrium_lights(n, seed=7):
    """n lights inside the atrium's bounds: point, spot and directional in turn, at seeded positions"""
    from raytracer3_amd.assets import LIGHT_DIRECTIONAL, LIGHT_POINT, LIGHT_SPOT, lights_array, make_light

    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        pos = rng.uniform((-6.0, 1.0, -6.0), (6.0, 5.0, 6.0))
        d = rng.normal(size=3)
        d[1] = -abs(d[1]) - 0.5
        kind = (LIGHT_POINT, LIGHT_SPOT, LIGHT_DIRECTIONAL)[k % 3]
        I = rng.uniform(0.5, 1.0, 3) * (1.0 if kind == LIGHT_DIRECTIONAL else 40.0)
        out.append(make_light(kind, I, pos, d, range=0.0 if k % 2 else 20.0, inner_cone=0.3, outer_cone=0.7))
    return lights_array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer, default_camera

    W, H = (int(x) for x in args.size.split("x"))
    pt = PathTracer((W, H))
    pt.set_scene(scenes.atrium(args.detail), scenes.sky(2048, 1024), assets.load_bluenoise())
    cam = default_camera((W, H), scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], scenes.ATRIUM_CAMERA["fov_deg"])
    result = {"scene": "atrium", "detail": args.detail, "size": [W, H], "spp": args.spp, "bounces": args.bounces, "rounds": args.rounds, "runs": []}
    configs = [(n, emissive) for n in (0, 1, 16) for emissive in (False, True)]
    runs = {cfg: {"lights": cfg[0], "nee_emissive": cfg[1], "ms_rounds": [], "ms_all": []} for cfg in configs}
    for _ in range(args.rounds):
        for n, emissive in configs:
            run = runs[n, emissive]
            pt.set_lights(atrium_lights(n) if n else None)
            flags = DEFAULT_FLAGS | L.F_NEE_PUNCTUAL | (L.F_NEE_EMISSIVE if emissive else 0)
            for k in range(args.warmup):
                pt.render(pt.make_gconst(cam, args.spp, args.bounces, frame=k, flags=flags))
            ms = []
            pt.ctx.stats_reset()
            for k in range(args.frames):
                g = pt.make_gconst(cam, args.spp, args.bounces, frame=k, flags=flags)
                pt.ctx.wait()
                t0 = time.perf_counter()
                pt.render(g)  # waits for the frame
                ms.append((time.perf_counter() - t0) * 1e3)
            ne, npu, _ = pt.ctx.light_masses(flags)
            run.update(flags=flags, table=[ne, npu], shadow_rays_per_frame=pt.ctx.stats().shadow_rays // args.frames, mean=float(pt.light()[..., :3].mean()))
            run["ms_rounds"].append(round(statistics.median(ms), 3))
            run["ms_all"] += [round(x, 3) for x in ms]
    for cfg in configs:
        runs[cfg]["ms"] = round(statistics.median(runs[cfg]["ms_all"]), 3)
        result["runs"].append(runs[cfg])
    pt.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
