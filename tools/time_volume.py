#!/usr/bin/env python3
"""Cost of absorbing glass (rt3_scene_set_attenuation, DESIGN.md sections 4s and 7): scenes.amber_cornell() from the Cornell camera through the
per-sample pinhole ({0, 1, 0}), against the same scene with every sigma 0 -- the same triangles, glass and lens, with no absorption
table and so no k_absorb launch.  Each configuration has a context of its own; the two are visited in turn, --rounds times over, so that
drift of the machine lands on both alike; each visit renders --warmup frames and then times --frames frames (host clock around a waited
frame).  A last visit with RT3_OPT_PROFILE on reads the per-category kernel times: k_absorb is the only launch of the category "other"
that one configuration has and the other lacks, so the difference of the two other_ms is its own time.  Prints one JSON line: per
configuration the median over all its timed frames with the smallest and largest, the median of each round, the extension rays per frame
and the frame's mean; and k_absorb's milliseconds per frame.

  python tools/time_volume.py --size 1920x1080 --spp 64 --bounces 8 --out time_volume.json
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
    tracers = {}
    for name in ("clear", "absorbing"):
        pt = PathTracer((W, H))
        pt.set_scene(scenes.amber_cornell(absorb=name == "absorbing"), None, assets.load_bluenoise())
        pt.set_lens(0.0, 1.0, 0.0)
        tracers[name] = pt
    result = {"scene": "amber_cornell", "size": [W, H], "spp": args.spp, "bounces": args.bounces, "flags": flags, "rounds": args.rounds, "runs": []}
    runs = {name: {"config": name, "absorbing_geometries": pt.ctx.attenuation_info(), "ms_rounds": [], "ms_all": []} for name, pt in tracers.items()}
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
    for name, pt in tracers.items():  # the kernels' own times, by category
        pt.ctx.set_option(L.OPT_PROFILE, 1)
        pt.render(pt.make_gconst(cam, args.spp, args.bounces, frame=0, flags=flags))
        pt.ctx.stats_reset()
        for k in range(args.frames):
            pt.render(pt.make_gconst(cam, args.spp, args.bounces, frame=k, flags=flags))
        st = pt.ctx.stats()
        runs[name]["kernel_ms_per_frame"] = {c: round(getattr(st, c + "_ms") / args.frames, 4) for c in ("extend", "shadow", "shade", "other")}
    for name, pt in tracers.items():
        runs[name]["ms"] = round(statistics.median(runs[name]["ms_all"]), 3)
        runs[name]["ms_min"], runs[name]["ms_max"] = min(runs[name]["ms_all"]), max(runs[name]["ms_all"])
        result["runs"].append(runs[name])
        pt.close()
    result["k_absorb_ms_per_frame"] = round(runs["absorbing"]["kernel_ms_per_frame"]["other"] - runs["clear"]["kernel_ms_per_frame"]["other"], 4)
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
