#!/usr/bin/env python3
"""What the "adaptive" pass costs and buys in coverage mode (rt3_adaptive_set_coverage, DESIGN.md sections 4l and 7), on the two frames that
need it: scenes.glass_cornell() from the Cornell camera at --glass-bounces bounces (default flags + RT3_F_NEE_EMISSIVE, as
tools/time_glass.py), and the benchmark frame (the atrium from the bench camera, default flags, --bounces) -- both antialiased over the
pixel, lens {0, 1, 1}.  Per scene, three measurements; one JSON line in all:

  overhead    "adaptive" with threshold 0 (nobody stops: --spp / --step rounds on the full list) against "refrence_mode" with the same
              lens and sample count, the two visited in turn --rounds times, --frames timed frames a visit after --warmup: the price of
              the rounds, the moments and the once-per-round synchronisation.
  thresholds  for each --thresholds value at cap --cap: ms per frame, mean samples per pixel, the share of pixels at the cap, rounds,
              paths, and the RMSE of Light (every pixel, rgb) against one "refrence_mode" frame of --ref-spp samples with another frame
              number (an independent estimate) -- beside the same figures of the fixed frame of --cap samples.
  missing     the frame's mean radiance against the reference frame's: the pass is biased low (a pixel that stops
              early has not met its fireflies), and RMSE alone rewards that.

Times are the host clock around a waited frame (G-buffer pass included on both sides): the median, minimum and maximum over all timed
frames of a configuration (--rounds x --frames = 15 by default).

  python tools/time_adaptive_lens.py --out time_adaptive_lens.json
  python tools/time_adaptive_lens.py --scenes glass_cornell --size 640x360 --cap 64 --ref-spp 256     # a quick look
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
    ap.add_argument("--scenes", default="glass_cornell,atrium")
    ap.add_argument("--detail", type=float, default=1.0, help="tessellation of the atrium")
    ap.add_argument("--spp", type=int, default=64, help="the overhead comparison's sample count")
    ap.add_argument("--bounces", type=int, default=4, help="of the atrium frame")
    ap.add_argument("--glass-bounces", type=int, default=8)
    ap.add_argument("--cap", type=int, default=256)
    ap.add_argument("--thresholds", default="0.3,0.5")
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--step", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer, default_camera

    W, H = (int(x) for x in args.size.split("x"))
    result = {"size": [W, H], "lens": [0.0, 1.0, 1.0], "cap": args.cap, "min_samples": args.min_spp, "step": args.step, "ref_spp": args.ref_spp,
              "frames_per_config": args.rounds * args.frames, "scenes": []}
    for name in args.scenes.split(","):
        if name == "glass_cornell":
            mesh, sky, cam_kw, flags, bounces = scenes.glass_cornell(), None, scenes.CORNELL_CAMERA, DEFAULT_FLAGS | L.F_NEE_EMISSIVE, args.glass_bounces
        elif name == "atrium":
            mesh, sky, cam_kw, flags, bounces = scenes.atrium(args.detail), scenes.sky(2048, 1024), scenes.ATRIUM_CAMERA, DEFAULT_FLAGS, args.bounces
        else:
            ap.error(f"unknown scene {name}")
        pt = PathTracer((W, H))
        pt.set_scene(mesh, sky, assets.load_bluenoise())
        pt.set_lens(0.0, 1.0, 1.0)
        pt.set_adaptive_coverage(True)
        cam = default_camera((W, H), cam_kw["position"], cam_kw["direction"], cam_kw["fov_deg"])

        def visit(samples, adaptive=None):
            """the ms of --frames waited frames after --warmup (frame numbers 0, 1, ...; the last one's images stay)"""
            kw = {} if adaptive is None else {"adaptive": adaptive}
            ms = []
            for k in range(args.warmup + args.frames):
                g = pt.make_gconst(cam, samples, bounces, frame=max(0, k - args.warmup), flags=flags)
                pt.ctx.wait()
                t0 = time.perf_counter()
                pt.render(g, **kw)  # waits for the frame
                if k >= args.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            return ms

        def summary(ms_rounds):
            every = [x for r in ms_rounds for x in r]
            return {"ms": round(statistics.median(every), 3), "ms_min": round(min(every), 3), "ms_max": round(max(every), 3),
                    "ms_rounds": [round(statistics.median(r), 3) for r in ms_rounds]}

        def in_turn(configs):
            """{name: (samples, adaptive params or None)} visited in turn --rounds times -> {name: summary}"""
            got = {k: [] for k in configs}
            for _ in range(args.rounds):
                for k, (samples, adaptive) in configs.items():
                    got[k].append(visit(samples, adaptive))
            return {k: summary(v) for k, v in got.items()}

        scene = {"scene": name, "bounces": bounces, "flags": flags}
        # 1. nobody stops
        nobody = L.AdaptiveParams(min_samples=args.min_spp, step=args.step, threshold=0.0)
        scene["overhead"] = dict(in_turn({"fixed": (args.spp, None), "adaptive": (args.spp, nobody)}), spp=args.spp)
        scene["overhead"]["rounds_per_frame"] = pt.ctx.adaptive_info()[0]

        # 2. and 3. against an independent reference
        pt.render(pt.make_gconst(cam, args.ref_spp, bounces, frame=999, flags=flags))
        ref = pt.light()[..., :3].astype(np.float64)

        def quality():
            got = pt.light()[..., :3].astype(np.float64)
            return {"rmse": float(np.sqrt(np.mean((got - ref) ** 2))), "mean": float(got.mean())}

        configs = {"fixed": (args.cap, None)}
        for thr in (float(x) for x in args.thresholds.split(",")):
            configs[f"threshold_{thr:g}"] = (args.cap, L.AdaptiveParams(min_samples=args.min_spp, step=args.step, threshold=thr))
        rows = in_turn(configs)
        for k, (samples, adaptive) in configs.items():  # the figures of one more frame of each (frame number 0, as the timed ones' first)
            pt.render(pt.make_gconst(cam, samples, bounces, frame=0, flags=flags), **({} if adaptive is None else {"adaptive": adaptive}))
            rows[k].update(quality())
            if adaptive is not None:
                n = pt.sample_counts()
                rounds, paths, capped = pt.ctx.adaptive_info()
                rows[k].update(threshold=adaptive.threshold, mean_spp=float(n.mean()), capped_share=capped / float(W * H), rounds=rounds, paths=paths)
            else:
                rows[k].update(mean_spp=float(samples), paths=samples * W * H)
            rows[k]["missing_radiance"] = 1.0 - rows[k]["mean"] / float(ref.mean())
        scene["cap_rows"] = rows
        scene["ref_mean"] = float(ref.mean())
        result["scenes"].append(scene)
        pt.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
