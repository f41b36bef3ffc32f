#!/usr/bin/env python3
"""Cost and worth of Russian roulette (rt3_path_set_roulette, DESIGN.md sections 4o and 7): scenes.glass_cornell() through the per-sample
pinhole at B = 8, 16, 32 and the bench frame (the atrium under its sky) at B = 4, 8, each with roulette off and on (--start, --floor).
A case has one context; off and on are visited in turn, --rounds times over, so that drift of the machine lands on both alike; a visit
renders --warmup frames and then times --frames frames (host clock around a waited frame).  Per configuration: the median and the spread
of all its timed frames, the extension rays traced per frame (rt3_stats.extension_rays), the tested and ended rays, k_roulette's own time
(the rise of rt3_stats.other_ms in one profiled frame), and the mean squared error of one frame against the mean of --ref-frames frames
rendered WITHOUT roulette (other frame numbers; the reference's own noise, 1 / ref-frames of the off configuration's variance, is in both
figures alike), from which efficiency = 1 / (seconds x MSE).  Prints one JSON line.

  python tools/time_roulette.py --size 1920x1080 --spp 64 --out time_roulette.json
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
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--start", type=int, default=2)
    ap.add_argument("--floor", type=float, default=0.0625)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ref-frames", type=int, default=8)
    ap.add_argument("--cases", default="glass:8,glass:16,glass:32,bench:4,bench:8", help="scene:bounces, comma separated")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer, default_camera

    W, H = (int(x) for x in args.size.split("x"))
    result = {"size": [W, H], "spp": args.spp, "start_bounce": args.start, "min_survival": args.floor, "frames": args.frames * args.rounds, "cases": []}
    tracers = {}
    for case in args.cases.split(","):
        scene, B = case.split(":")
        B = int(B)
        if scene not in tracers:
            pt = PathTracer((W, H))
            if scene == "glass":  # set_scene switches the per-sample pinhole on
                pt.set_scene(scenes.glass_cornell(), None, assets.load_bluenoise())
                tracers[scene] = (pt, scenes.CORNELL_CAMERA, DEFAULT_FLAGS | L.F_NEE_EMISSIVE)
            else:
                pt.set_scene(scenes.atrium(1.0), scenes.sky(2048, 1024), assets.load_bluenoise())
                tracers[scene] = (pt, scenes.ATRIUM_CAMERA, DEFAULT_FLAGS)
        pt, cam_kw, flags = tracers[scene]
        cam = default_camera((W, H), cam_kw["position"], cam_kw["direction"], cam_kw["fov_deg"])

        def switch(on):
            pt.set_roulette(args.start if on else None, args.floor)

        def light(frame_no):
            pt.render(pt.make_gconst(cam, args.spp, B, frame=frame_no, flags=flags))
            return pt.light()[..., :3].astype(np.float64)

        switch(False)
        ref = sum(light(1000 + k) for k in range(args.ref_frames)) / args.ref_frames
        runs = {on: {"roulette": on, "ms_all": []} for on in (False, True)}
        for _ in range(args.rounds):
            for on, run in runs.items():
                switch(on)
                for k in range(args.warmup):
                    pt.render(pt.make_gconst(cam, args.spp, B, frame=k, flags=flags))
                pt.ctx.stats_reset()
                for k in range(args.frames):
                    g = pt.make_gconst(cam, args.spp, B, frame=k, flags=flags)
                    pt.ctx.wait()
                    t0 = time.perf_counter()
                    pt.render(g)  # waits for the frame
                    run["ms_all"].append(round((time.perf_counter() - t0) * 1e3, 3))
                tested, ended = pt.roulette_info()
                run.update(extension_rays_per_frame=pt.ctx.stats().extension_rays // args.frames, tested=tested, ended=ended)
        for on, run in runs.items():
            switch(on)
            run["mse"] = float(np.mean([np.mean((light(k) - ref) ** 2) for k in range(2)]))
            pt.ctx.set_option(L.OPT_PROFILE, 1)
            pt.ctx.stats_reset()
            light(0)
            st = pt.ctx.stats()
            run["profiled_ms"] = {"extend": st.extend_ms, "shadow": st.shadow_ms, "shade": st.shade_ms, "other": st.other_ms}
            pt.ctx.set_option(L.OPT_PROFILE, 0)
            run["ms"] = round(statistics.median(run["ms_all"]), 3)
            run["ms_min"], run["ms_max"] = min(run["ms_all"]), max(run["ms_all"])
            run["efficiency"] = 1.0 / (run["ms"] * 1e-3 * run["mse"]) if run["mse"] > 0 else None
        off, on = runs[False], runs[True]
        result["cases"].append({"scene": scene, "bounces": B, "off": off, "on": on, "k_roulette_ms": round(on["profiled_ms"]["other"] - off["profiled_ms"]["other"], 3),
                                "time_ratio": round(on["ms"] / off["ms"], 4), "efficiency_ratio": (on["efficiency"] / off["efficiency"]) if on["efficiency"] and off["efficiency"] else None})
        switch(False)
    for pt, _, _ in tracers.values():
        pt.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
