#!/usr/bin/env python3
"""What the "adaptive" pass costs and buys (DESIGN.md sections 4l and 7) on the benchmark frame: the atrium from the bench camera, default
flags.  Three measurements, one JSON line:

  overhead   "adaptive" with threshold 0 (nobody stops: every round runs on the full list) against "refrence_mode" at the same spp, the
             two visited in turn --rounds times: the price of the rounds, the moments and the once-per-round synchronisation.
  thresholds for each --thresholds value at cap --cap: ms per frame, mean samples per foreground pixel, the share of pixels that reached
             the cap, rounds, the RMSE of Light (foreground, rgb) against one "refrence_mode" frame of --ref-spp samples rendered with
             another frame number (an independent estimate), and the frame's mean radiance beside the reference's: the pass is biased
             low, and RMSE alone rewards that where outliers dominate it.
  matched    the fixed sample counts of --ladder with their ms, RMSE and mean; per threshold the fixed spp whose RMSE equals the adaptive
             frame's (log-log interpolation along the ladder, its last segment extended up to 4 x the cap), and that frame rendered
             and timed.

Times are the host clock around a waited frame (G-buffer pass included on both sides), medians over --frames frames after --warmup.

  python tools/time_adaptive.py --out time_adaptive.json
  python tools/time_adaptive.py --fixed-only --package-root ../parent   # the fixed leg alone from another checkout (the parent commit)
"""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--spp", type=int, default=64, help="the overhead comparison's sample count")
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--cap", type=int, default=256)
    ap.add_argument("--thresholds", default="0.05,0.1,0.2,0.3,0.5")
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--step", type=int, default=16)
    ap.add_argument("--ladder", default="8,16,32,64,128,256")
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fixed-only", action="store_true", help="time refrence_mode at --spp and stop (works on a checkout without the pass)")
    ap.add_argument("--package-root", default=str(ROOT), help="the checkout to import raytracer3_amd from")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.package_root).resolve()))

    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer, default_camera

    W, H = (int(x) for x in args.size.split("x"))
    pt = PathTracer((W, H))
    pt.set_scene(scenes.atrium(args.detail), scenes.sky(2048, 1024), assets.load_bluenoise())
    cam = default_camera((W, H), scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], scenes.ATRIUM_CAMERA["fov_deg"])

    def timed(samples, adaptive=None, frames=args.frames, warmup=args.warmup):
        """median ms of `frames` waited frames (frame numbers 0, 1, ...; the last one's images stay)"""
        kw = {} if adaptive is None else {"adaptive": adaptive}
        ms = []
        for k in range(warmup + frames):
            g = pt.make_gconst(cam, samples, args.bounces, frame=max(0, k - warmup), flags=DEFAULT_FLAGS)
            pt.ctx.wait()
            t0 = time.perf_counter()
            pt.render(g, **kw)
            if k >= warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ms), 3), [round(x, 3) for x in ms]

    result = {"scene": "atrium", "detail": args.detail, "size": [W, H], "bounces": args.bounces, "package_root": args.package_root}
    if args.fixed_only:
        per_round = [timed(args.spp)[0] for _ in range(args.rounds)]
        result["fixed_only"] = {"spp": args.spp, "ms_rounds": per_round, "ms": round(statistics.median(per_round), 3)}
    else:
        nobody = L.AdaptiveParams(min_samples=args.min_spp, step=args.step, threshold=0.0)
        fixed_r, adapt_r = [], []
        for _ in range(args.rounds):
            fixed_r.append(timed(args.spp)[0])
            adapt_r.append(timed(args.spp, nobody)[0])
        rounds, paths, capped = pt.ctx.adaptive_info()
        result["overhead"] = {"spp": args.spp, "min_samples": args.min_spp, "step": args.step, "rounds_per_frame": rounds,
                              "fixed_ms_rounds": fixed_r, "adaptive_ms_rounds": adapt_r,
                              "fixed_ms": round(statistics.median(fixed_r), 3), "adaptive_ms": round(statistics.median(adapt_r), 3)}

        pt.render(pt.make_gconst(cam, args.ref_spp, args.bounces, frame=999, flags=DEFAULT_FLAGS))
        ref = pt.light()[..., :3].astype(np.float64)
        fg = pt.gbuffer()[1] != np.float32(L.BACKGROUND_DEPTH)

        def rmse():
            d = pt.light()[..., :3].astype(np.float64)[fg] - ref[fg]
            return float(np.sqrt(np.mean(d * d)))

        def mean():
            return float(pt.light()[..., :3].astype(np.float64)[fg].mean())

        ladder = []
        for spp in (int(x) for x in args.ladder.split(",")):
            ms, _ = timed(spp)
            ladder.append({"spp": spp, "ms": ms, "rmse": rmse(), "mean": mean()})
        result["ladder"] = ladder
        lx, ly = np.log([r["spp"] for r in ladder]), np.log([r["rmse"] for r in ladder])

        rows = []
        for thr in (float(x) for x in args.thresholds.split(",")):
            p = L.AdaptiveParams(min_samples=args.min_spp, step=args.step, threshold=thr)
            ms, _ = timed(args.cap, p)
            n = pt.sample_counts()
            rounds, paths, capped = pt.ctx.adaptive_info()
            row = {"threshold": thr, "cap": args.cap, "ms": ms, "rmse": rmse(), "mean": mean(), "mean_spp": float(n[fg].mean()), "rounds": rounds,
                   "capped_share": capped / max(1, int(fg.sum())), "paths": paths}
            # the fixed spp of the same RMSE: RMSE falls with spp, so interpolate spp as a function of log RMSE (np.interp wants rising x)
            lr = math.log(row["rmse"])
            if lr < ly[-1] and len(lx) > 1:  # better than the ladder's last frame: its last segment, extended
                match = min(float(np.exp(lx[-1] + (lr - ly[-1]) * (lx[-1] - lx[-2]) / (ly[-1] - ly[-2]))), 4.0 * args.cap)
            else:
                match = float(np.exp(np.interp(lr, ly[::-1], lx[::-1])))
            spp = max(1, round(match))
            fms, _ = timed(spp)
            row.update(matched_spp=match, matched_fixed={"spp": spp, "ms": fms, "rmse": rmse(), "mean": mean()})
            rows.append(row)
        result["thresholds"] = rows
        result["foreground_share"] = float(fg.mean())
        result["ref_spp"] = args.ref_spp
        result["ref_mean"] = float(ref[fg].mean())
    pt.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
