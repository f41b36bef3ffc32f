#!/usr/bin/env python3
"""Cost of the guide images of a lens frame and of the "denoise" pass guided by them (rt3_camera_set_guide_output,
rt3_denoise_set_guide_input; DESIGN.md sections 4u and 7): scenes.glass_cornell() from the Cornell camera through the per-sample pinhole,
tools/time_glass.py's frame.

 * the frame with the guide output off and on, at each --spp-list count.  Each configuration has a context of its own; the two are
   visited in turn, --rounds times over, so that drift of the machine lands on both alike; each visit renders --warmup frames and then
   times --frames frames (host clock around a waited frame).  Per configuration: the median over all its timed frames, its least and
   greatest, the median of each round.
 * k_lens_guide's own time: the difference of rt3_stats.other_ms per frame (RT3_OPT_PROFILE; the category of the streaming kernels
   between the traversal and shade launches) between the two configurations, median of --frames profiled frames each.
 * the pass alone, HIP events, guided by the G-buffer and by the guide images of the same frame: median of --repeats launches after
   --pass-warmup, with --iterations iterations.

  python tools/time_guide.py --size 1920x1080 --bounces 8 --out time_guide.json
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
    ap.add_argument("--spp-list", default="4,64")
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--pass-warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer, default_camera

    W, H = (int(x) for x in args.size.split("x"))
    flags = DEFAULT_FLAGS | L.F_NEE_EMISSIVE  # the box is lit by its ceiling panel: sample it directly
    cam = default_camera((W, H), scenes.CORNELL_CAMERA["position"], scenes.CORNELL_CAMERA["direction"], scenes.CORNELL_CAMERA["fov_deg"])
    tracers = {}
    for name in ("guide_off", "guide_on"):
        pt = PathTracer((W, H))
        pt.set_scene(scenes.glass_cornell(), None, assets.load_bluenoise())
        pt.set_lens(0.0, 1.0, 0.0)
        pt.set_guide(name == "guide_on")
        tracers[name] = pt
    result = {"scene": "glass_cornell", "size": [W, H], "bounces": args.bounces, "flags": flags, "rounds": args.rounds, "frames": []}
    for spp in (int(s) for s in args.spp_list.split(",")):
        runs = {name: {"config": name, "ms_rounds": [], "ms_all": []} for name in tracers}
        for _ in range(args.rounds):
            for name, pt in tracers.items():
                for k in range(args.warmup):
                    pt.render(pt.make_gconst(cam, spp, args.bounces, frame=k, flags=flags))
                ms = []
                for k in range(args.frames):
                    g = pt.make_gconst(cam, spp, args.bounces, frame=k, flags=flags)
                    pt.ctx.wait()
                    t0 = time.perf_counter()
                    pt.render(g)  # waits for the frame
                    ms.append((time.perf_counter() - t0) * 1e3)
                runs[name]["ms_rounds"].append(round(statistics.median(ms), 3))
                runs[name]["ms_all"] += [round(x, 3) for x in ms]
        row = {"spp": spp, "runs": []}
        for name, pt in tracers.items():
            r = runs[name]
            r["ms"], r["ms_min"], r["ms_max"] = round(statistics.median(r["ms_all"]), 3), min(r["ms_all"]), max(r["ms_all"])
            # the streaming kernels' share, HIP events: k_lens_guide is what the two configurations differ by
            pt.ctx.set_option(L.OPT_PROFILE, 1)
            other = []
            for k in range(args.frames):
                pt.ctx.stats_reset()
                pt.render(pt.make_gconst(cam, spp, args.bounces, frame=k, flags=flags))
                other.append(pt.ctx.stats().other_ms)
            pt.ctx.set_option(L.OPT_PROFILE, 0)
            r["other_ms"] = round(statistics.median(other), 4)
            row["runs"].append(r)
        row["k_lens_guide_ms"] = round(row["runs"][1]["other_ms"] - row["runs"][0]["other_ms"], 4)
        result["frames"].append(row)

    # ---- the pass alone, on the guided tracer's last frame
    pt = tracers["guide_on"]
    ctx = pt.ctx
    g = pt.make_gconst(cam, 4, args.bounces, frame=1, flags=flags)
    h = pt.render(g, denoise=True)
    b = [h["gbuffer"], h["depth"], h["light"], h["denoised"]]
    X, Y = -(-W // 8), -(-H // 8)
    ctx.set_denoise_params(iterations=args.iterations)
    ctx.set_option(L.OPT_PROFILE, 1)
    result["pass"] = {"iterations": args.iterations}
    for name, images in (("by_gbuffer", None), ("by_samples", h["guide"])):
        ctx.set_denoise_guide_input(images)
        for _ in range(args.pass_warmup):
            ctx.check(ctx.pass_launch("denoise", X, Y, 1, g, b))
        ms = []
        for _ in range(args.repeats):
            ctx.stats_reset()
            ctx.check(ctx.pass_launch("denoise", X, Y, 1, g, b))
            ms.append(ctx.stats().other_ms)  # synchronises
        result["pass"][name] = {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    ctx.set_option(L.OPT_PROFILE, 0)
    ctx.set_denoise_params()
    for pt in tracers.values():
        pt.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
