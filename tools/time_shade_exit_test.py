#!/usr/bin/env python3
"""Cost and worth of the exit test in the shade kernel (RT3_OPT_SHADE_EXIT_TEST, DESIGN.md sections 4r and 7): the bench frame (the atrium
under its sky) and the lit Cornell box (scenes.cornell() under the same sky, where nearly every sky shadow ray is occluded), each with the
option at 0 and at 1.  A case has one context; the two settings are visited in turn, --rounds times over, so that drift of the machine lands
on both alike; a visit renders --warmup frames and then times --frames frames (host clock around a waited frame).  Per setting: the median
and the spread of all its timed frames, the ray counts of one frame (which the option may not change), what that frame added to the exit
table's counters (tried, occluded: with the option at 1 the occluded rays are the ones that were never queued) and the per-category times of
one profiled frame (k_shade_defer_exit and k_light are in `shade`, k_shadow / k_shadow_exit in `shadow`); per case whether the two settings'
frames are the same bits.  Prints one JSON line.

  python tools/time_shade_exit_test.py --size 1920x1080 --spp 64 --out time_shade_exit_test.json
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
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="bench,cornell", help="comma separated: bench | cornell")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer, default_camera

    W, H = (int(x) for x in args.size.split("x"))
    sky, bn = scenes.sky(2048, 1024), assets.load_bluenoise()
    result = {"size": [W, H], "spp": args.spp, "bounces": args.bounces, "frames": args.frames * args.rounds, "cases": []}
    for case in args.cases.split(","):
        mesh, cam_kw = (scenes.atrium(1.0), scenes.ATRIUM_CAMERA) if case == "bench" else (scenes.cornell(), scenes.CORNELL_CAMERA)
        pt = PathTracer((W, H))
        pt.set_scene(mesh, sky, bn)
        cam = default_camera((W, H), cam_kw["position"], cam_kw["direction"], cam_kw["fov_deg"])

        def switch(opt):
            pt.ctx.set_option(L.OPT_SHADE_EXIT_TEST, opt)

        def gconst(frame_no):
            return pt.make_gconst(cam, args.spp, args.bounces, frame=frame_no, flags=DEFAULT_FLAGS)

        runs = {opt: {"shade_exit_test": opt, "ms_all": []} for opt in (0, 1)}
        for _ in range(args.rounds):
            for opt, run in runs.items():
                switch(opt)
                for k in range(args.warmup):
                    pt.render(gconst(k))
                for k in range(args.frames):
                    g = gconst(k)
                    pt.ctx.wait()
                    t0 = time.perf_counter()
                    pt.render(g)  # waits for the frame
                    run["ms_all"].append(round((time.perf_counter() - t0) * 1e3, 3))
        lights = {}
        for opt, run in runs.items():
            switch(opt)
            pt.ctx.set_option(L.OPT_PROFILE, 1)
            pt.ctx.stats_reset()
            _, tried0, occluded0, _ = pt.ctx.exit_table_info()
            pt.render(gconst(0))
            st = pt.ctx.stats()
            _, tried1, occluded1, in_use = pt.ctx.exit_table_info()
            run["profiled_ms"] = {"extend": st.extend_ms, "shadow": st.shadow_ms, "shade": st.shade_ms, "other": st.other_ms}
            run["extension_rays"], run["shadow_rays"] = int(st.extension_rays), int(st.shadow_rays)
            run["tried"], run["occluded_by_entry"], run["table_in_use"] = int(tried1 - tried0), int(occluded1 - occluded0), int(in_use)
            pt.ctx.set_option(L.OPT_PROFILE, 0)
            lights[opt] = pt.light()
            run["ms"] = round(statistics.median(run["ms_all"]), 3)
            run["ms_min"], run["ms_max"] = min(run["ms_all"]), max(run["ms_all"])
        p0, p1 = runs[0]["profiled_ms"], runs[1]["profiled_ms"]
        entry = {"scene": case, "off": runs[0], "on": runs[1], "time_ratio": round(runs[1]["ms"] / runs[0]["ms"], 4),
                 "shadow_ms_saved": round(p0["shadow"] - p1["shadow"], 3), "shade_ms_added": round(p1["shade"] - p0["shade"], 3),
                 "same_bits": bool(np.array_equal(lights[0].view(np.uint32), lights[1].view(np.uint32)))}
        result["cases"].append(entry)
        switch(1)
        pt.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
