#!/usr/bin/env python3
"""Cost of per-sample camera rays (rt3_camera_set_lens, DESIGN.md sections 4m and 7) on the benchmark frame: the atrium from the bench
camera under the default flags with the lens off, with antialiasing only ({0, -, 1}) and with an aperture.  A lens frame traces one more
k_extend launch per batch (the camera rays) and shades vertex 0 from the shading records instead of the G-buffer.  The three
configurations are visited in turn, --rounds times over, so that drift of the machine lands on all of them alike; each visit renders
--warmup frames and then times --frames frames (host clock around a waited frame).  Prints one JSON line: per configuration the median
over all its timed frames, the median of each round, the extension rays per frame (rt3_stats.extension_rays) and the frame's mean.

  python tools/time_lens.py --size 1920x1080 --spp 64 --bounces 4 --out time_lens.json
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--aperture", type=float, default=0.05)
    ap.add_argument("--focus", type=float, default=8.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer, default_camera

    W, H = (int(x) for x in args.size.split("x"))
    pt = PathTracer((W, H))
    pt.set_scene(scenes.atrium(args.detail), scenes.sky(2048, 1024), assets.load_bluenoise())
    cam = default_camera((W, H), scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], scenes.ATRIUM_CAMERA["fov_deg"])
    result = {"scene": "atrium", "detail": args.detail, "size": [W, H], "spp": args.spp, "bounces": args.bounces, "rounds": args.rounds, "runs": []}
    configs = {"off": None, "antialiasing": (0.0, 1.0, 1.0), "aperture": (args.aperture, args.focus, 1.0)}
    runs = {name: {"lens": name, "params": list(p) if p else None, "ms_rounds": [], "ms_all": []} for name, p in configs.items()}
    for _ in range(args.rounds):
        for name, p in configs.items():
            run = runs[name]
            if p is None:
                pt.set_lens(None)
            else:
                pt.set_lens(*p)
            for k in range(args.warmup):
                pt.render(pt.make_gconst(cam, args.spp, args.bounces, frame=k, flags=DEFAULT_FLAGS))
            ms = []
            pt.ctx.stats_reset()
            for k in range(args.frames):
                g = pt.make_gconst(cam, args.spp, args.bounces, frame=k, flags=DEFAULT_FLAGS)
                pt.ctx.wait()
                t0 = time.perf_counter()
                pt.render(g)  # waits for the frame
                ms.append((time.perf_counter() - t0) * 1e3)
            run.update(extension_rays_per_frame=pt.ctx.stats().extension_rays // args.frames, mean=float(pt.light()[..., :3].mean()))
            run["ms_rounds"].append(round(statistics.median(ms), 3))
            run["ms_all"] += [round(x, 3) for x in ms]
    pt.set_lens(None)
    for name in configs:
        runs[name]["ms"] = round(statistics.median(runs[name]["ms_all"]), 3)
        runs[name]["ms_min"], runs[name]["ms_max"] = min(runs[name]["ms_all"]), max(runs[name]["ms_all"])
        result["runs"].append(runs[name])
    pt.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
