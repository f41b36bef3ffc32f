#!/usr/bin/env python3
"""Cost of fog (rt3_scene_set_medium, DESIGN.md sections 4y and 7): scenes.sunlit_room() (pane shadows on, the sky and the sun sampled) and
scenes.glass_cornell() (the ceiling panel sampled), each through the per-sample pinhole ({0, 1, 0}), with a medium over the scene's bounds
against the same context state without one -- the same triangles, lens and flags, and no k_fog_segment / k_fog_shadow launch.  Each
configuration has a context of its own; the two are visited in turn, --rounds times over, so that drift of the machine lands on both
alike; each visit renders --warmup frames and then times --frames frames (host clock around a waited frame).  A last visit with
RT3_OPT_PROFILE on reads the per-category kernel times: the fog kernels are the only launches of the category "other" that one
configuration has and the other lacks, and the in-scatter walks the only further "shadow" launches, so the differences are their own
times.  To compare medium off with the parent commit, run this tool's "off" configuration there (--off-only works on a library without
the call).  Prints one JSON line: per scene and configuration the median over all timed frames with the smallest and largest, the median
of each round, the frame's mean, the medium's counts; and the fog kernels' milliseconds per frame.

  python tools/time_fog.py --size 1920x1080 --spp 64 --bounces 8 --frames 5 --rounds 3 --out time_fog.json

--shaft: the equal-time comparison on the shaft world instead (a slab of medium under a sun, nothing else in view): frames of --spp
samples with fog are timed, and the RMSE of one such frame against a 64 times longer one is reported beside the RMSE of the frame with
four times the samples, i.e. what the time buys."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def timed(pt, make, warmup, frames):
    for k in range(warmup):
        pt.render(make(k))
    ms = []
    for k in range(frames):
        g = make(k)
        pt.ctx.wait()
        t0 = time.perf_counter()
        pt.render(g)  # waits for the frame
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def shaft(args, W, H):
    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets
    from raytracer3_amd.assets import LIGHT_DIRECTIONAL, Material, MeshBuilder, lights_array, make_light
    from raytracer3_amd.renderer import PathTracer, default_camera

    mb = MeshBuilder()
    mb.add("floor", np.array([[-8.0, 0.0, -8.0], [8.0, 0.0, -8.0], [8.0, 0.0, 4.0], [-8.0, 0.0, 4.0]]), np.tile([0.0, 1.0, 0.0], (4, 1)), None,
           [[0, 2, 1], [0, 3, 2]], Material((0.5, 0.5, 0.5), 0.0, 1.0))
    mesh = mb.build()
    pt = PathTracer((W, H))
    pt.set_scene(mesh, None, assets.load_bluenoise())
    pt.set_lights(lights_array([make_light(LIGHT_DIRECTIONAL, (3.0, 2.5, 2.0), direction=(0.2, -1.0, 0.1))]))
    pt.set_medium(L.Medium(0.05, 0.25, 0.5, (-8.0, 0.0, -8.0), (8.0, 3.0, 4.0)))
    cam = default_camera((W, H), (0.5, 1.0, 3.0), (0.0, -0.1, -1.0), 50.0)
    flags = L.F_NEE_PUNCTUAL | L.F_FACEFORWARD
    out = {"world": "shaft", "size": [W, H], "bounces": args.bounces, "frames": []}
    pt.render(pt.make_gconst(cam, 64 * args.spp, args.bounces, frame=99, flags=flags))
    ref = pt.light()[..., :3].astype(np.float64)
    for spp in (args.spp, 4 * args.spp):
        ms = timed(pt, lambda k: pt.make_gconst(cam, spp, args.bounces, frame=k, flags=flags), args.warmup, args.frames)
        rmse = float(np.sqrt(np.mean((pt.light()[..., :3].astype(np.float64) - ref) ** 2)))
        out["frames"].append({"spp": spp, "ms": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "rmse": rmse})
    pt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sigma-s", type=float, default=0.15)
    ap.add_argument("--sigma-a", type=float, default=0.02)
    ap.add_argument("--g", type=float, default=0.3)
    ap.add_argument("--off-only", action="store_true", help="time the configuration without a medium alone (also on a library that lacks the call)")
    ap.add_argument("--shaft", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer, default_camera

    W, H = (int(x) for x in args.size.split("x"))
    if args.shaft:
        result = shaft(args, W, H)
    else:
        result = {"size": [W, H], "spp": args.spp, "bounces": args.bounces, "rounds": args.rounds, "sigma_s": args.sigma_s, "sigma_a": args.sigma_a, "g": args.g, "scenes": []}
        worlds = {
            "sunlit_room": (scenes.sunlit_room, scenes.SUNLIT_ROOM_CAMERA, DEFAULT_FLAGS | L.F_NEE_PUNCTUAL, True, lambda: scenes.sky(2048, 1024)),
            "glass_cornell": (scenes.glass_cornell, scenes.CORNELL_CAMERA, L.F_FACEFORWARD | L.F_SPECULAR | L.F_NEE_EMISSIVE, False, lambda: None),
        }
        for scene, (make_mesh, cam_kw, flags, panes, make_sky) in worlds.items():
            cam = default_camera((W, H), cam_kw["position"], cam_kw["direction"], cam_kw["fov_deg"])
            mesh = make_mesh()
            tracers = {}
            for name in ("off",) if args.off_only else ("off", "fog"):
                pt = PathTracer((W, H))
                pt.set_pane_shadows(panes)
                pt.set_scene(mesh, make_sky(), assets.load_bluenoise())
                pt.set_lens(0.0, 1.0, 0.0)
                if name == "fog":
                    from raytracer3_amd.renderer import scene_medium

                    pt.set_medium(scene_medium(mesh, args.sigma_s, args.sigma_a, args.g))
                tracers[name] = pt
            runs = {name: {"config": name, "ms_rounds": [], "ms_all": []} for name in tracers}
            def frames_of(pt):
                return lambda k: pt.make_gconst(cam, args.spp, args.bounces, frame=k, flags=flags)

            for _ in range(args.rounds):
                for name, pt in tracers.items():
                    ms = timed(pt, frames_of(pt), args.warmup, args.frames)
                    runs[name]["mean"] = float(pt.light()[..., :3].mean())
                    runs[name]["ms_rounds"].append(round(statistics.median(ms), 3))
                    runs[name]["ms_all"] += [round(x, 3) for x in ms]
            for name, pt in tracers.items():  # the kernels' own times, by category
                pt.ctx.set_option(L.OPT_PROFILE, 1)
                make = frames_of(pt)
                pt.render(make(0))
                pt.ctx.stats_reset()
                for k in range(args.frames):
                    pt.render(make(k))
                st = pt.ctx.stats()
                runs[name]["kernel_ms_per_frame"] = {c: round(getattr(st, c + "_ms") / args.frames, 4) for c in ("extend", "shadow", "shade", "other")}
                if name == "fog":
                    runs[name]["segments"], runs[name]["inscatter_rays"] = pt.medium_info()
                runs[name]["ms"] = round(statistics.median(runs[name]["ms_all"]), 3)
                runs[name]["ms_min"], runs[name]["ms_max"] = min(runs[name]["ms_all"]), max(runs[name]["ms_all"])
                pt.close()
            entry = {"scene": scene, "flags": flags, "runs": list(runs.values())}
            if "fog" in runs:
                k_on, k_off = runs["fog"]["kernel_ms_per_frame"], runs["off"]["kernel_ms_per_frame"]
                entry["fog_kernels_ms_per_frame"] = round(k_on["other"] - k_off["other"], 4)
                entry["inscatter_walks_ms_per_frame"] = round(k_on["shadow"] - k_off["shadow"], 4)
            result["scenes"].append(entry)
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
