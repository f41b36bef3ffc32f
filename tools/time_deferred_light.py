#!/usr/bin/env python3
"""Cost and worth of deferred sky light samples (RT3_OPT_DEFER_SKY_LIGHT, DESIGN.md sections 4p and 7): the bench frame (the atrium under its
sky) and the lit Cornell box (scenes.cornell() under the same sky, without and with emitter NEE), each with the option at 0 and at 1.  A
case has one context; the two settings are visited in turn, --rounds times over, so that drift of the machine lands on both alike; a visit
renders --warmup frames and then times --frames frames (host clock around a waited frame).  Per setting: the median and the spread of all
its timed frames, the ray counts of one frame (which the option may not change) and the per-category times of one profiled frame (k_light
is in `shade`); per case whether the two settings' frames are the same bits.
`survivor_share_estimate` (atrium only) is the unoccluded share of sky shadow rays made on the host the way
tests/experiments/exp_shadow_exit_table.py makes them (vertex 0 and vertex 1 of a pinhole frame, the oracle's sky sampler) and traced here
by rt3_trace_rays: an estimate of what k_light evaluates, not a count taken inside the kernels -- the library has no such counter.
Prints one JSON line.

  python tools/time_deferred_light.py --size 1920x1080 --spp 64 --out time_deferred_light.json
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


def survivor_share(pt, mesh, sky, size=(480, 270)):
    sys.path.insert(0, str(ROOT / "tests"))
    sys.path.insert(0, str(ROOT / "tests" / "experiments"))
    import exp_shadow_exit_table as exp
    import orc

    osc = orc.Scene(mesh, sky)
    rng = np.random.default_rng(7)
    out = {}
    for vertex in (0, 1):
        rays = exp.shadow_rays(osc, mesh, size[0], size[1], rng, vertex)
        occluded = pt.ctx.trace_rays(rays, any_hit=True)[3] != 0
        out[f"vertex_{vertex}"] = {"rays": int(rays.shape[1]), "unoccluded": round(float(1.0 - occluded.mean()), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="bench,cornell,cornell_emit", help="comma separated: bench | cornell | cornell_emit")
    ap.add_argument("--no-survivors", action="store_true", help="skip the host-made survivor estimate (it needs the oracle library)")
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
        flags = DEFAULT_FLAGS | (L.F_NEE_EMISSIVE if case == "cornell_emit" else 0)
        pt = PathTracer((W, H))
        pt.set_scene(mesh, sky, bn)
        cam = default_camera((W, H), cam_kw["position"], cam_kw["direction"], cam_kw["fov_deg"])

        def switch(opt):
            pt.ctx.set_option(L.OPT_DEFER_SKY_LIGHT, opt)

        def gconst(frame_no):
            return pt.make_gconst(cam, args.spp, args.bounces, frame=frame_no, flags=flags)

        runs = {opt: {"defer": opt, "ms_all": []} for opt in (0, 1)}
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
            pt.render(gconst(0))
            st = pt.ctx.stats()
            run["profiled_ms"] = {"extend": st.extend_ms, "shadow": st.shadow_ms, "shade": st.shade_ms, "other": st.other_ms}
            run["extension_rays"], run["shadow_rays"] = int(st.extension_rays), int(st.shadow_rays)
            pt.ctx.set_option(L.OPT_PROFILE, 0)
            lights[opt] = pt.light()
            run["ms"] = round(statistics.median(run["ms_all"]), 3)
            run["ms_min"], run["ms_max"] = min(run["ms_all"]), max(run["ms_all"])
        entry = {"scene": case, "off": runs[0], "on": runs[1], "time_ratio": round(runs[1]["ms"] / runs[0]["ms"], 4),
                 "shade_ms_saved": round(runs[0]["profiled_ms"]["shade"] - runs[1]["profiled_ms"]["shade"], 3),
                 "same_bits": bool(np.array_equal(lights[0].view(np.uint32), lights[1].view(np.uint32)))}
        if case == "bench" and not args.no_survivors:
            entry["survivor_share_estimate"] = survivor_share(pt, mesh, sky)
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
