#!/usr/bin/env python3
"""Data sheet of the sample-guided "temporal" pass (DESIGN.md sections 4v and 7) on `scenes.glass_cornell()` from the Cornell camera,
through the per-sample pinhole a scene with glass switches on, default flags + RT3_F_NEE_EMISSIVE, 1 spp, the camera moving by the step
of tests/test_temporal_cpu.py's moving Cornell row (about 2 pixels a frame).

1. HIP-event time of the pass alone (RT3_OPT_PROFILE brackets its launch) at --size: median of --repeats launches after --warmup, of the
   guided launch (k_temporal<TemporalGuide>: rt3_temporal_set_guide_input) and of the G-buffer launch (k_temporal<TemporalGbuffer<false>>,
   the same kernel body over the other source of records) on the same frame, the same bindings and the same history; once reprojecting the
   previous frame under the camera move and once with zeroed history (no tap counts: the gathers stop at PrevHistory.w).  Per foreground
   pixel the guided launch reads 80 B of this frame and gathers up to 4 x 64 B where the G-buffer launch reads 36 B and gathers 4 x 52 B;
   both write 48 B.
2. What it buys at --small: K = --frames frames of 1 spp along the move; RMSE of linear radiance over all pixels against a --ref-spp frame
   of the last view, of the last single frame, of the guided "temporal" and of guided "temporal" + guided "denoise".

  python tools/time_temporal_guide.py --size 1920x1080 --out time_temporal_guide.json
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

MOVE = ((0.01, 0.0, 0.0), (0.0105, 0.0, 0.0))  # per frame: position, direction


def gconst_at(pt, window, step, spp, bounces, frame, flags):
    from raytracer3_amd import scenes
    from raytracer3_amd.renderer import default_camera

    kw = scenes.CORNELL_CAMERA
    pos = np.asarray(kw["position"], np.float64) + step * np.asarray(MOVE[0])
    dirn = np.asarray(kw["direction"], np.float64) + step * np.asarray(MOVE[1])
    return pt.make_gconst(default_camera(window, pos, dirn, kw["fov_deg"]), spp, bounces, frame=frame, flags=flags)


def rmse(a, ref):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)) ** 2)))


def pass_times(args, flags):
    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import PathTracer

    W, H = window = tuple(int(x) for x in args.size.split("x"))
    pt = PathTracer(window)
    pt.set_scene(scenes.glass_cornell(), None, assets.load_bluenoise())
    pt.set_guide(True, temporal=True)
    ctx = pt.ctx
    for k in range(2):
        g = gconst_at(pt, window, k, 1, args.bounces, k + 1, flags)
        h = pt.render(g, temporal=True)
    cur, prev = h["guide"], h["prev_guide"]  # (the names have traded places behind the frame; the handles are the frame's)
    cover = pt.guide()["position"][..., 3]
    n_hist = pt.history()[0][..., 3]
    b = [h["gbuffer"], h["depth"], h["light"], h["prev_gbuffer"], h["prev_depth"], h["prev_history"], h["prev_moments"],
         h["accumulated"], h["history"], h["moments"]]
    X, Y = -(-W // 8), -(-H // 8)

    def timed():
        for _ in range(args.warmup):
            ctx.check(ctx.pass_launch("temporal", X, Y, 1, g, b))
        ms = []
        for _ in range(args.repeats):
            ctx.stats_reset()
            ctx.check(ctx.pass_launch("temporal", X, Y, 1, g, b))
            ms.append(ctx.stats().other_ms)  # synchronises
        return ms

    ctx.set_option(L.OPT_PROFILE, 1)
    rows = []
    for case in ("reprojected", "no_history"):
        if case == "no_history":
            zero = np.zeros((H, W, 4), np.float32)
            pt.rg.upload(h["prev_history"], zero)
            pt.rg.upload(h["prev_moments"], zero)
        row = {"case": case}
        for kernel in ("guided", "gbuffer"):
            if kernel == "guided":
                ctx.set_temporal_guide_input(cur, prev)
            else:
                ctx.set_temporal_guide_input(None, None)
            ms = timed()
            row[kernel] = {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
        row["guided_over_gbuffer"] = round(row["guided"]["ms"] / row["gbuffer"]["ms"], 3)
        rows.append(row)
    ctx.set_option(L.OPT_PROFILE, 0)
    pt.close()
    return {"size": [W, H], "fully_covered_pixels": int((cover == 1).sum()), "pixels_with_history": int((n_hist > 1).sum()), "pass": rows}


def what_it_buys(args, flags):
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import PathTracer

    window = tuple(int(x) for x in args.small.split("x"))
    pt = PathTracer(window)
    pt.set_scene(scenes.glass_cornell(), None, assets.load_bluenoise())
    K = args.frames
    pt.render(gconst_at(pt, window, K - 1, args.ref_spp, args.bounces, 1000, flags))
    ref = pt.light()
    pt.set_guide(True, temporal=True)
    pt.ctx.set_denoise_params()
    pt.ctx.set_temporal_params()
    for k in range(K):
        pt.render(gconst_at(pt, window, k, 1, args.bounces, k + 1, flags), temporal=True, denoise=True)
    r = {"size": list(window), "frames": K, "ref_spp": args.ref_spp, "rmse_one_sample": round(rmse(pt.light(), ref), 5),
         "rmse_guided_temporal": round(rmse(pt.accumulated(), ref), 5), "rmse_guided_temporal_denoise": round(rmse(pt.denoised(), ref), 5),
         "share_with_history_of_4": round(float((pt.history()[0][..., 3] >= 4).mean()), 4)}
    pt.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--small", default="96x64")
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=31)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from raytracer3_amd import _lib as L
    from raytracer3_amd.renderer import DEFAULT_FLAGS

    flags = DEFAULT_FLAGS | L.F_NEE_EMISSIVE
    result = {"scene": "glass_cornell", "bounces": args.bounces, "time": pass_times(args, flags), "error": what_it_buys(args, flags)}
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
