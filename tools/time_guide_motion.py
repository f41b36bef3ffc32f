#!/usr/bin/env python3
"""Data sheet of the guide's fifth image, the samples' mean previous position (DESIGN.md sections 4w and 7), on `scenes.glass_cornell()`
from the Cornell camera at --size, --bounces bounces, default flags + RT3_F_NEE_EMISSIVE, through the per-sample pinhole a scene with glass
switches on, with the short block placed as an instance of its own that moved by 2.5 cm since the previous frame.

1. The frame (gbuffer -> refrence_mode, wall clock around a waited draw) at 1 and 64 spp, medians of --frames frames after --warmup: the
   guide output on with the fifth image off, and with it on.  k_lens_guide_prev reads 48 B per sample beside the path tracer's own traffic
   and writes 16 B per pixel: the prediction is under 1 % of the frame at 64 spp.
2. The kernel alone: the HIP-event time of the launches RT3_OPT_PROFILE files under "other" (camera rays, guide kernels, accumulation), on
   minus off.
3. The "temporal" launch at 1 spp with the guide input, with and without the fifth image as its guide motion input (k_temporal<
   TemporalGuideMotion> against <TemporalGuide>: 16 B more read per foreground pixel).

`--tree PATH --off-only` runs part 1's "off" rows from another checkout (its package and its librt3.so), for the comparison with the
parent commit; that checkout needs none of this change.

  python tools/time_guide_motion.py --size 1920x1080 --out time_guide_motion.json
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def scene(moved=True):
    """(mesh, instances, previous transforms): everything under the identity but, with `moved`, the short block, 2.5 cm along x"""
    from raytracer3_amd import scenes

    mesh = scenes.glass_cornell()
    eye = np.eye(4, dtype=np.float32)
    block = eye.copy()
    block[0, 3] = 0.025 if moved else 0.0
    s = mesh.names.index("short")
    inst = [(0, s, eye), (s, 1, block), (s + 1, len(mesh.names) - s - 1, eye)]
    return mesh, inst, [eye, eye, eye]


def tracer(args, moved=True):
    from raytracer3_amd import assets
    from raytracer3_amd.renderer import PathTracer

    window = tuple(int(x) for x in args.size.split("x"))
    mesh, inst, prev = scene(moved)
    pt = PathTracer(window)
    pt.set_scene(mesh, None, assets.load_bluenoise(), instances=inst)
    return pt, window, prev


def gconst(pt, window, spp, bounces, frame, flags):
    from raytracer3_amd import scenes
    from raytracer3_amd.renderer import default_camera

    kw = scenes.CORNELL_CAMERA
    return pt.make_gconst(default_camera(window, kw["position"], kw["direction"], kw["fov_deg"]), spp, bounces, frame=frame, flags=flags)


def median_row(values):
    return {"ms": round(statistics.median(values), 4), "ms_min": round(min(values), 4), "ms_max": round(max(values), 4)}


def frame_times(args, flags):
    from raytracer3_amd import _lib as L
    from raytracer3_amd.renderer import guide_images

    pt, window, prev = tracer(args)
    ctx, rg = pt.ctx, pt.rg
    ctx.set_guide_output(guide_images(rg))
    image = 0
    if not args.off_only:
        from raytracer3_amd.renderer import guide_prev_position_image

        ctx.set_prev_transforms(prev)
        image = guide_prev_position_image(rg)
    rows = []
    for spp in (1, 64):
        row = {"spp": spp}
        for case in ("off",) if args.off_only else ("off", "on"):
            if not args.off_only:
                ctx.set_guide_motion_output(image if case == "on" else 0)
            wall, other = [], []
            for k in range(args.warmup + args.frames):
                h = pt.commands(gconst(pt, window, spp, args.bounces, k + 1, flags), postprocess=False, guide=True)
                ctx.set_option(L.OPT_PROFILE, 0)
                t0 = time.perf_counter()
                rg.draw_frame(h["light"], wait=True)
                if k >= args.warmup:
                    wall.append(1e3 * (time.perf_counter() - t0))
            ctx.set_option(L.OPT_PROFILE, 1)
            for k in range(args.frames):  # the same frames once more, with the launches bracketed by events
                h = pt.commands(gconst(pt, window, spp, args.bounces, args.warmup + k + 1, flags), postprocess=False, guide=True)
                ctx.stats_reset()
                rg.draw_frame(h["light"], wait=True)
                other.append(ctx.stats().other_ms)
            ctx.set_option(L.OPT_PROFILE, 0)
            row[case] = {"frame": median_row(wall), "other": median_row(other)}
        if not args.off_only:
            row["on_over_off"] = round(row["on"]["frame"]["ms"] / row["off"]["frame"]["ms"], 4)
            row["kernel_ms"] = round(row["on"]["other"]["ms"] - row["off"]["other"]["ms"], 4)
        rows.append(row)
    pt.close()
    return {"size": list(window), "frames": rows}


def temporal_times(args, flags):
    from raytracer3_amd import _lib as L

    pt, window, _ = tracer(args, moved=False)
    W, H = window
    ctx = pt.ctx
    pt.set_guide(True, temporal=True)
    for k in range(2):
        g = gconst(pt, window, 1, args.bounces, k + 1, flags)
        if k:
            pt.set_instances(scene()[1])  # the block moves between the two frames
        h = pt.render(g, temporal=True)
    assert "guide_motion" in h, "the second frame follows the moved block"
    b = [h["gbuffer"], h["depth"], h["light"], h["prev_gbuffer"], h["prev_depth"], h["prev_history"], h["prev_moments"],
         h["accumulated"], h["history"], h["moments"]]
    ctx.set_temporal_guide_input(h["guide"], h["prev_guide"])
    X, Y = -(-W // 8), -(-H // 8)
    ctx.set_option(L.OPT_PROFILE, 1)
    row = {}
    for case, image in (("with_input", h["guide_motion"]), ("without", 0)):
        ctx.set_temporal_guide_motion_input(image)
        ms = []
        for k in range(args.warmup + args.frames):
            ctx.stats_reset()
            ctx.check(ctx.pass_launch("temporal", X, Y, 1, g, b))
            if k >= args.warmup:
                ms.append(ctx.stats().other_ms)  # synchronises
        row[case] = median_row(ms)
    row["with_over_without"] = round(row["with_input"]["ms"] / row["without"]["ms"], 4)
    ctx.set_option(L.OPT_PROFILE, 0)
    pt.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--frames", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tree", default=None, help="run from this checkout's package and library instead of the tool's own")
    ap.add_argument("--off-only", action="store_true", help="only the frame with the fifth image off; makes none of the new calls")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.tree).resolve() if args.tree else ROOT))

    from raytracer3_amd import _lib as L
    from raytracer3_amd.renderer import DEFAULT_FLAGS

    flags = DEFAULT_FLAGS | L.F_NEE_EMISSIVE
    result = {"scene": "glass_cornell, the short block moved", "bounces": args.bounces, "tree": args.tree or ".", "frame": frame_times(args, flags)}
    if not args.off_only:
        result["temporal"] = temporal_times(args, flags)
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
