#!/usr/bin/env python3
"""Cost and worth of pane shadows (rt3_scene_set_pane_shadows, DESIGN.md sections 4q and 7).

Cost: scenes.glass_cornell() -- one thin pane, one solid sphere -- from the Cornell camera through the per-sample pinhole, with the mode off
and on.  Each configuration has a context of its own; they are visited in turn, --rounds times over, so that drift of the machine lands
on both alike; each visit renders --warmup frames and then times --frames frames (host clock around a waited frame).  A library without
the call (an older build, timed with this same script for the comparison with the parent) runs the "off" configuration only.

Worth (--worth): scenes.sunlit_room() under scenes.sky(), F_NEE_SKY alone (the sun left out: without pane shadows it does not exist, so
there is nothing to compare it with), at --worth-spp samples with the mode off and on, against a reference of --ref-spp samples rendered
with the mode OFF, which is independent of the new code.  Reports the RMSE of `Light`, the frame time and the efficiency
1 / (time x MSE) of each.

Prints one JSON line.

  python tools/time_pane_shadows.py --size 1920x1080 --spp 64 --bounces 8 --frames 5 --rounds 3 --worth --out time_pane_shadows.json
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
    ap.add_argument("--mode", type=int, default=0, help="RT3_OPT_INSTANCE_MODE of the cost frames: 0 one tree, 1 two-level")
    ap.add_argument("--worth", action="store_true")
    ap.add_argument("--worth-size", default="480x270")
    ap.add_argument("--worth-spp", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=16384)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer, default_camera

    has_mode = hasattr(PathTracer, "set_pane_shadows")
    W, H = (int(x) for x in args.size.split("x"))
    flags = DEFAULT_FLAGS | L.F_NEE_EMISSIVE  # the box is lit by its ceiling panel: sample it directly
    cam = default_camera((W, H), scenes.CORNELL_CAMERA["position"], scenes.CORNELL_CAMERA["direction"], scenes.CORNELL_CAMERA["fov_deg"])
    tracers = {}
    for name in ("off", "on") if has_mode else ("off",):
        pt = PathTracer((W, H))
        if has_mode:
            pt.set_pane_shadows(name == "on")
        pt.set_scene(scenes.glass_cornell(), None, assets.load_bluenoise(), options=[(L.OPT_INSTANCE_MODE, args.mode)])
        pt.set_lens(0.0, 1.0, 0.0)
        tracers[name] = pt
    result = {"scene": "glass_cornell", "instance_mode": args.mode, "size": [W, H], "spp": args.spp, "bounces": args.bounces, "flags": flags, "rounds": args.rounds, "runs": []}
    runs = {name: {"config": name, "ms_rounds": [], "ms_all": []} for name in tracers}
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
            s = pt.ctx.stats()
            run.update(shadow_rays_per_frame=s.shadow_rays // args.frames, mean=float(pt.light()[..., :3].mean()))
            run["ms_rounds"].append(round(statistics.median(ms), 3))
            run["ms_all"] += [round(x, 3) for x in ms]
    for name, pt in tracers.items():
        runs[name]["ms"] = round(statistics.median(runs[name]["ms_all"]), 3)
        runs[name]["ms_min"], runs[name]["ms_max"] = min(runs[name]["ms_all"]), max(runs[name]["ms_all"])
        result["runs"].append(runs[name])
        pt.close()

    if args.worth and has_mode:
        w, h = (int(x) for x in args.worth_size.split("x"))
        sky = scenes.sky(1024, 512)
        wflags = L.F_NEE_SKY | L.F_BLUENOISE | L.F_FACEFORWARD
        kw = scenes.SUNLIT_ROOM_CAMERA
        wcam = default_camera((w, h), kw["position"], kw["direction"], kw["fov_deg"])
        frames = {}
        worth = {"scene": "sunlit_room", "size": [w, h], "spp": args.worth_spp, "ref_spp": args.ref_spp, "bounces": args.bounces, "flags": wflags, "runs": []}
        for name in ("off", "on"):
            pt = PathTracer((w, h))
            pt.set_pane_shadows(name == "on")
            pt.set_scene(scenes.sunlit_room(), sky, assets.load_bluenoise())
            if name == "off":  # the reference: many samples, accumulated over frames of 1024 in float64
                acc, n = np.zeros((h, w, 3)), max(1, args.ref_spp // 1024)
                for k in range(n):
                    pt.render(pt.make_gconst(wcam, 1024, args.bounces, frame=1000 + k, flags=wflags))
                    acc += pt.light()[..., :3]
                frames["ref"] = acc / n
            ms = []
            for k in range(args.warmup + args.frames):
                g = pt.make_gconst(wcam, args.worth_spp, args.bounces, frame=k, flags=wflags)
                pt.ctx.wait()
                t0 = time.perf_counter()
                pt.render(g)
                if k >= args.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            frames[name] = pt.light()[..., :3].astype(np.float64)
            mse = float(((frames[name] - frames["ref"]) ** 2).mean())
            t = statistics.median(ms)
            worth["runs"].append({"config": name, "ms": round(t, 3), "rmse": mse**0.5, "efficiency": 1.0 / (t * 1e-3 * mse), "mean": float(frames[name].mean())})
            pt.close()
        worth["ref_mean"] = float(frames["ref"].mean())
        result["worth"] = worth
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
