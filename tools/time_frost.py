#!/usr/bin/env python3
"""Cost of rough transmission (rt3_scene_set_rough_transmission, DESIGN.md sections 4t and 7), from the Cornell camera through the per-sample
pinhole ({0, 1, 0}):
  (a) scenes.glass_cornell() -- no glass with roughness > 0 -- with the mode off and on: the same kernels launch, so the two times are one
      time within the spread (and the parent commit's, which has no mode: run the tool there too; it then times "off" alone);
  (b) scenes.frosted_cornell() with the mode off (clear glass, k_shade_glass) and on (frosted, k_shade_frost).
Each configuration has a context of its own; they are visited in turn, --rounds times over, so that drift of the machine lands on all
alike; each visit renders --warmup frames and then times --frames frames (host clock around a waited frame).  Prints one JSON line: per
configuration the median over all its timed frames, the median of each round, the smallest and largest frame, the frosted geometries of
the build, the extension rays per frame and the frame's mean.

  python tools/time_frost.py --size 1920x1080 --spp 64 --bounces 8 --frames 5 --rounds 3 --out time_frost.json
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
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer, default_camera

    W, H = (int(x) for x in args.size.split("x"))
    flags = DEFAULT_FLAGS | L.F_NEE_EMISSIVE  # the box is lit by its ceiling panel: sample it directly
    cam = default_camera((W, H), scenes.CORNELL_CAMERA["position"], scenes.CORNELL_CAMERA["direction"], scenes.CORNELL_CAMERA["fov_deg"])
    has_mode = hasattr(PathTracer, "set_rough_transmission")
    has_scene = hasattr(scenes, "frosted_cornell")
    configs = [("glass_off", "glass_cornell", False)]
    if has_mode:
        configs.append(("glass_on", "glass_cornell", True))
    if has_scene:
        configs.append(("frosted_off", "frosted_cornell", False))
        if has_mode:
            configs.append(("frosted_on", "frosted_cornell", True))
    tracers, frosted = {}, {}
    for name, scene, on in configs:
        pt = PathTracer((W, H))
        if has_mode:
            pt.set_rough_transmission(on)
        pt.set_scene(getattr(scenes, scene)(), None, assets.load_bluenoise())
        pt.set_lens(0.0, 1.0, 0.0)
        tracers[name] = pt
        frosted[name] = pt.ctx.rough_transmission_info() if has_mode else 0
    result = {"size": [W, H], "spp": args.spp, "bounces": args.bounces, "flags": flags, "rounds": args.rounds, "runs": []}
    runs = {name: {"config": name, "frosted_geometries": frosted[name], "ms_rounds": [], "ms_all": []} for name in tracers}
    for _ in range(args.rounds):
        for name, pt in tracers.items():
            run = runs[name]
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
            run.update(extension_rays_per_frame=pt.ctx.stats().extension_rays // args.frames, mean=float(pt.light()[..., :3].mean()))
            run["ms_rounds"].append(round(statistics.median(ms), 3))
            run["ms_all"] += [round(x, 3) for x in ms]
    for name, pt in tracers.items():
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
