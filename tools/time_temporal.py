#!/usr/bin/env python3
"""Data sheet of the "temporal" pass (DESIGN.md sections 4g and 7) on the benchmark frame: the atrium from the bench camera, default flags,
1 spp, the camera moving by the step of tests/test_temporal_cpu.py between the two frames.

HIP-event time of the pass alone (RT3_OPT_PROFILE brackets its launch): median of --repeats launches after --warmup, once reprojecting the
previous frame under the camera move and once with zeroed history (no tap counts: the gathers stop at PrevHistory.w).  Beside it the bytes
a launch must move at least -- per foreground pixel 36 read from this frame and 48 written, plus each previous record once (52: under a
small motion the four taps of neighbouring pixels are the same records) -- the time those bytes take at the 6.29 TB/s a float4 copy
reaches on this GPU, the fraction of that floor the pass reaches, and the rate at which it moves the gathered bytes as issued
(4 x 52 per pixel).

  python tools/time_temporal.py --size 1920x1080 --out time_temporal.json
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

COPY_TBPS = 6.29  # measured float4 copy rate of the MI355X (8.0 TB/s nominal)
FRAME_BYTES, PREV_BYTES = 36 + 48, 52  # per foreground pixel: this frame read + the three images written; one previous record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=31)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer, default_camera

    W, H = (int(x) for x in args.size.split("x"))
    pt = PathTracer((W, H))
    pt.set_scene(scenes.atrium(args.detail), scenes.sky(2048, 1024), assets.load_bluenoise())
    kw = scenes.ATRIUM_CAMERA
    ctx = pt.ctx
    gs = []
    for k in range(2):
        pos = np.asarray(kw["position"], np.float32) + np.float32(k) * np.array([0.02, 0.0, 0.01], np.float32)
        dirn = np.asarray(kw["direction"], np.float32) + np.float32(k) * np.array([0.0, 0.0, 0.012], np.float32)
        gs.append(pt.make_gconst(default_camera((W, H), pos, dirn, kw["fov_deg"]), 1, args.bounces, frame=k + 1, flags=DEFAULT_FLAGS))
        h = pt.render(gs[-1], temporal=True)
    g = gs[1]
    fg = int((pt.gbuffer()[1] != np.float32(L.BACKGROUND_DEPTH)).sum())
    n_hist = pt.history()[0][..., 3]
    b = [h["gbuffer"], h["depth"], h["light"], h["prev_gbuffer"], h["prev_depth"], h["prev_history"], h["prev_moments"],
         h["accumulated"], h["history"], h["moments"]]
    X, Y = -(-W // 8), -(-H // 8)

    def launch():
        ctx.check(ctx.pass_launch("temporal", X, Y, 1, g, b))

    def timed():
        for _ in range(args.warmup):
            launch()
        ms = []
        for _ in range(args.repeats):
            ctx.stats_reset()
            launch()
            ms.append(ctx.stats().other_ms)  # synchronises
        return ms

    ctx.set_option(L.OPT_PROFILE, 1)
    rows = []
    for what in ("reprojected", "no_history"):
        if what == "no_history":
            zero = np.zeros((H, W, 4), np.float32)
            pt.rg.upload(h["prev_history"], zero)
            pt.rg.upload(h["prev_moments"], zero)
        ms = timed()
        med = statistics.median(ms)
        floor_bytes = fg * (FRAME_BYTES + (PREV_BYTES if what == "reprojected" else 20)) + (W * H - fg) * (4 + 16 + 48)
        floor_ms = floor_bytes / (COPY_TBPS * 1e12) * 1e3
        issued = fg * (FRAME_BYTES + 4 * PREV_BYTES) + (W * H - fg) * (4 + 16 + 48)
        rows.append({"case": what, "ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "floor_bytes": floor_bytes,
                     "floor_ms": round(floor_ms, 4), "fraction_of_floor": round(floor_ms / med, 4),
                     "floor_tb_per_s": round(floor_bytes / (med * 1e-3) / 1e12, 3),
                     "issued_tb_per_s": round(issued / (med * 1e-3) / 1e12, 3) if what == "reprojected" else None})
    ctx.set_option(L.OPT_PROFILE, 0)
    result = {"scene": "atrium", "detail": args.detail, "size": [W, H], "foreground_pixels": fg,
              "pixels_with_history": int((n_hist > 1).sum()), "pass": rows}
    pt.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
