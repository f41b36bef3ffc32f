#!/usr/bin/env python3
"""Data sheet of the "denoise" pass (DESIGN.md sections 4f and 7) on the benchmark frame: the atrium from the bench camera, default flags.

 * HIP-event time of the pass alone (RT3_OPT_PROFILE brackets each of its launches; the sum over one pass) for 1..N iterations: median of
   --repeats launches after --warmup.  The increments are the single iterations (step 1, 2, 4, ...); the rest is prepare + variance + finish.
   Beside it the bytes the stages must move at least (every record read once and written once: prepare 36 + 48, variance 48 + 16, an
   iteration 48 + 16, finish 52 + 16 bytes per pixel), the time those bytes take at the 6.29 TB/s a float4 copy reaches on this GPU, and
   the fraction of that floor the pass reaches.
 * the frames it would be attached to: wall-clock ms of gbuffer + refrence_mode at each --spp-list count (median of --frames), their
   foreground RMSE of linear radiance against a converged render (--ref-frames x 64 spp), the same with the pass behind them, and the
   equal-time comparison: the unfiltered sample count that costs (k spp + denoise) milliseconds and its RMSE (both interpolated, log-log,
   in the measured table).

  python tools/time_denoise.py --size 1920x1080 --out time_denoise.json
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
sys.path.insert(0, str(ROOT))

COPY_TBPS = 6.29  # measured float4 copy rate of the MI355X (8.0 TB/s nominal)
FIXED_BYTES, ITERATION_BYTES = (36 + 48) + (48 + 16) + (52 + 16), 48 + 16  # per pixel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=5, help="time the pass for 1..this many iterations")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--spp-list", default="1,2,4,8,16,32")
    ap.add_argument("--ref-frames", type=int, default=32, help="converged reference: this many frames of 64 spp, averaged")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer, default_camera

    W, H = (int(x) for x in args.size.split("x"))
    pt = PathTracer((W, H))
    pt.set_scene(scenes.atrium(args.detail), scenes.sky(2048, 1024), assets.load_bluenoise())
    cam = default_camera((W, H), scenes.ATRIUM_CAMERA["position"], scenes.ATRIUM_CAMERA["direction"], scenes.ATRIUM_CAMERA["fov_deg"])
    ctx = pt.ctx

    def gconst(spp, frame):
        return pt.make_gconst(cam, spp, args.bounces, frame=frame, flags=DEFAULT_FLAGS)

    # ---- the pass alone, HIP events
    g = gconst(1, 1)
    h = pt.render(g, denoise=True)
    b = [h["gbuffer"], h["depth"], h["light"], h["denoised"]]
    X, Y = -(-W // 8), -(-H // 8)

    def launch():
        ctx.check(ctx.pass_launch("denoise", X, Y, 1, g, b))

    ctx.set_option(L.OPT_PROFILE, 1)
    pass_ms, rows = {}, []
    for n in range(1, args.iterations + 1):
        ctx.set_denoise_params(iterations=n)
        for _ in range(args.warmup):
            launch()
        ms = []
        for _ in range(args.repeats):
            ctx.stats_reset()
            launch()
            ms.append(ctx.stats().other_ms)  # synchronises
        pass_ms[n] = statistics.median(ms)
        floor_ms = (FIXED_BYTES + n * ITERATION_BYTES) * W * H / (COPY_TBPS * 1e12) * 1e3
        rows.append({"iterations": n, "ms": round(pass_ms[n], 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                     "added_by_last_iteration_ms": round(pass_ms[n] - pass_ms[n - 1], 4) if n > 1 else None,
                     "floor_bytes": (FIXED_BYTES + n * ITERATION_BYTES) * W * H, "floor_ms": round(floor_ms, 4), "fraction_of_floor": round(floor_ms / pass_ms[n], 4)})
    ctx.set_option(L.OPT_PROFILE, 0)
    ctx.set_denoise_params()
    result = {"scene": "atrium", "detail": args.detail, "size": [W, H], "bounces": args.bounces, "pass": rows}

    # ---- the frames it is attached to, and what it buys
    ref = np.zeros((H, W, 3))
    for k in range(args.ref_frames):
        pt.render(gconst(64, 10_000 + k))
        ref += pt.light()[..., :3].astype(np.float64)
    ref /= args.ref_frames
    fg = pt.gbuffer()[1] != np.float32(L.BACKGROUND_DEPTH)

    def rmse(img):
        return float(np.sqrt(((img[..., :3].astype(np.float64) - ref)[fg] ** 2).mean()))

    def frame_ms(spp, denoise):
        for k in range(2):
            pt.render(gconst(spp, k), denoise=denoise)
        ms = []
        for k in range(args.frames):
            gg = gconst(spp, k)
            ctx.wait()
            t0 = time.perf_counter()
            pt.render(gg, denoise=denoise)  # waits for the frame
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms)

    frames = []
    for spp in (int(s) for s in args.spp_list.split(",")):
        row = {"spp": spp, "ms": round(frame_ms(spp, False), 4), "ms_with_denoise": round(frame_ms(spp, True), 4)}
        pt.render(gconst(spp, 1), denoise=True)
        row["rmse"], row["rmse_denoised"] = rmse(pt.light()), rmse(pt.denoised())
        frames.append(row)
    ls, lt, le = (np.log([r[k] for r in frames]) for k in ("spp", "ms", "rmse"))
    lt = np.maximum.accumulate(lt)  # np.interp wants a non-decreasing abscissa (1 and 2 spp cost almost the same)
    for r in frames:  # the unfiltered sample count that costs the same milliseconds, and its error
        s = float(np.interp(math.log(r["ms_with_denoise"]), lt, ls))
        r["equal_time_spp"] = round(math.exp(s), 2)
        r["equal_time_rmse"] = float(math.exp(np.interp(s, ls, le)))
        r["beyond_table"] = bool(r["ms_with_denoise"] > frames[-1]["ms"])
    result["frames"] = frames
    result["reference_spp"] = 64 * args.ref_frames
    pt.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
