#!/usr/bin/env python3
"""Data sheet of the "motion" pass and of the motion input of "temporal" (DESIGN.md sections 4h and 7) on the benchmark frame: the atrium
from the bench camera, default flags, 1 spp, one more placement of a column standing in view that moves by 5 cm between the two frames
while the camera moves by the step of tests/test_temporal_cpu.py.

HIP-event times (RT3_OPT_PROFILE brackets every launch), median of --repeats launches after --warmup:
  "motion" beside "gbuffer" of the same frame -- both make the same primary trace (ray generation, k_extend) and differ in their last
  kernel -- with the trace and the rest apart;
  "temporal" with the motion input and without it (the kernel instance of the parent commit).
Beside the times the bytes each variant moves per pixel: the kernels of "motion" behind the trace read the 4-byte pixel word twice and the
16-byte hit record and write the 32-byte ray and the 16-byte texel (a moved pixel gathers up to 4 + 4 + 4 + 8 + 12 + 96 + 64 more from
small tables that its neighbours share); "temporal" reads 16 more with the input.

With --deform, after those rows (which stay as they are): the placed column's own mesh is bent through rt3_scene_update_vertices behind a
snapshot and four more rows are timed the same way -- the snapshot's full copy, its copy of the updated range, the
compare kernel over that range, and "motion" with the deformed mesh in view (both placements of the column follow).

  python tools/time_motion.py --size 1920x1080 --out time_motion.json
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

MOTION_BYTES = (4 + 32) + (4 + 16 + 16)  # per pixel, the pass's own kernels: k_raygen (pixel word, ray) + k_motion (pixel word, hit record, texel)
MOVED_GATHER_BYTES = 4 + 4 + 4 + 8 + 12 + 96 + 64  # prim_geom, slot, first_prim, the two offsets, indices, vertices, previous matrix
TEMPORAL_BYTES = 36 + 48 + 52       # tools/time_temporal.py: this frame, the three written images, one previous record
COLUMN = "col0_0"


def time_deform(args, ctx, pt, mesh, ci, passes, h, W, H):
    """the rows of --deform; leaves the column bent and the structure refitted"""
    first = int(mesh.geometries["vertex_offset"][ci])
    end = int(mesh.geometries["vertex_offset"][ci + 1]) if ci + 1 < len(mesh.geometries) else len(mesh.vertices)
    rest = np.ascontiguousarray(mesh.vertices[first:end], np.float32)
    bent = rest.copy()
    y = bent[:, 1] - bent[:, 1].min()
    bent[:, 0] += np.float32(0.02) * y * y  # 2 cm at one metre, growing with the height

    def timed(prepare, call):
        rows = []
        for k in range(args.warmup + args.repeats):
            prepare()
            ctx.stats_reset()
            call()
            rows.append(ctx.stats().other_ms)  # synchronises
        rows = rows[args.warmup:]
        return {"ms": round(statistics.median(rows), 4), "ms_min": round(min(rows), 4), "ms_max": round(max(rows), 4)}

    out = {"vertices": len(mesh.vertices), "updated_vertices": end - first}
    ctx.set_prev_transforms(None)
    out["snapshot_full"] = timed(ctx.forget_prev_vertices, ctx.snapshot_vertices)
    out["snapshot_dirty_range"] = timed(lambda: ctx.update_vertices(bent, first), ctx.snapshot_vertices)
    ctx.update_vertices(rest, first)
    ctx.snapshot_vertices()
    out["compare"] = timed(lambda: ctx.update_vertices(bent, first), lambda: ctx.deformed_geometries(len(mesh.geometries)))
    ctx.refit_accel()
    flags = ctx.deformed_geometries(len(mesh.geometries))
    assert flags.tolist() == [i == ci for i in range(len(flags))]
    out["motion_deformed"] = passes("motion", W, H, 1, [h["motion"]])
    M = pt.rg.download(h["motion"], (H, W, 4), np.float32)
    out["deformed_pixels"] = int((M[..., 3] == 3).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=31)
    ap.add_argument("--instance-mode", type=int, default=0)
    ap.add_argument("--deform", action="store_true", help="also time the snapshot, the compare kernel and \"motion\" on a deformed mesh")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.render_graph import ImageSize
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer, default_camera

    W, H = (int(x) for x in args.size.split("x"))
    mesh = scenes.atrium(args.detail)
    pt = PathTracer((W, H))
    pt.ctx.set_option(L.OPT_INSTANCE_MODE, args.instance_mode)
    pt.set_scene(mesh, scenes.sky(2048, 1024), assets.load_bluenoise())
    ctx = pt.ctx
    # one more placement of a column, standing 5 m in front of the camera; it moves by 5 cm a frame
    ci = mesh.names.index(COLUMN)
    first = int(np.sum(mesh.prim_counts[:ci]))
    base = mesh.triangle_positions()[first:first + int(mesh.prim_counts[ci])].reshape(-1, 3)
    foot = np.array([base[:, 0].mean(), base[:, 1].min(), base[:, 2].mean()])
    eye = np.eye(4, dtype=np.float32)

    def world(k):
        m = eye.copy()
        m[:3, 3] = np.array([-5.0 + 0.05 * k, 0.0, 0.6]) - foot
        return [(0, len(mesh.geometries), eye), (ci, 1, m)]

    kw = scenes.ATRIUM_CAMERA
    gs = []
    for k in range(2):
        pt.set_instances(world(k))
        pos = np.asarray(kw["position"], np.float32) + np.float32(k) * np.array([0.02, 0.0, 0.01], np.float32)
        dirn = np.asarray(kw["direction"], np.float32) + np.float32(k) * np.array([0.0, 0.0, 0.012], np.float32)
        gs.append(pt.make_gconst(default_camera((W, H), pos, dirn, kw["fov_deg"]), 1, args.bounces, frame=k + 1, flags=DEFAULT_FLAGS))
        h = pt.render(gs[-1], temporal=True)
    g = gs[1]
    M = pt.motion()  # the second frame had the node
    fg, moved = int((M[..., 3] > 0).sum()), int((M[..., 3] == 2).sum())
    n_hist = pt.history()[0][..., 3]
    n_moved = float(n_hist[M[..., 3] == 2].mean()) if moved else 0.0

    def passes(name, x, y, z, bindings):
        def launch():
            ctx.check(ctx.pass_launch(name, x, y, z, g, bindings))

        for _ in range(args.warmup):
            launch()
        rows = []
        for _ in range(args.repeats):
            ctx.stats_reset()
            launch()
            s = ctx.stats()  # synchronises
            rows.append((s.extend_ms + s.other_ms, s.extend_ms, s.other_ms))
        med = [statistics.median(r[i] for r in rows) for i in range(3)]
        return {"ms": round(med[0], 4), "trace_ms": round(med[1], 4), "rest_ms": round(med[2], 4),
                "ms_min": round(min(r[0] for r in rows), 4), "ms_max": round(max(r[0] for r in rows), 4)}

    ctx.set_option(L.OPT_PROFILE, 1)
    scratch_gb = pt.rg.image(ImageSize.FullScreen, L.FORMAT_R32G32B32A32_UINT, "timing_gbuffer")  # the frame's own G-buffer stays as it is
    scratch_depth = pt.rg.image(ImageSize.FullScreen, L.FORMAT_R32_SFLOAT, "timing_depth")
    out = {"gbuffer": passes("gbuffer", W, H, 1, [scratch_gb, scratch_depth]), "motion": passes("motion", W, H, 1, [h["motion"]])}
    ctx.set_prev_transforms(None)
    out["motion_nothing_moved"] = passes("motion", W, H, 1, [h["motion"]])
    ctx.set_prev_transforms([m for _, _, m in world(0)])
    ctx.check(ctx.pass_launch("motion", W, H, 1, g, [h["motion"]]))
    tb = [h[n] for n in ("gbuffer", "depth", "light", "prev_gbuffer", "prev_depth", "prev_history", "prev_moments", "accumulated", "history", "moments")]
    X, Y = -(-W // 8), -(-H // 8)
    out["temporal_with_motion_input"] = passes("temporal", X, Y, 1, tb)
    ctx.set_temporal_motion_input(0)
    out["temporal_without"] = passes("temporal", X, Y, 1, tb)
    deform = None
    if args.deform:
        deform = time_deform(args, ctx, pt, mesh, ci, passes, h, W, H)
    ctx.set_option(L.OPT_PROFILE, 0)
    npx = W * H
    for k, per_px in (("motion", MOTION_BYTES), ("motion_nothing_moved", MOTION_BYTES)):
        out[k]["bytes_per_pixel"] = per_px
        out[k]["kernel_tb_per_s"] = round(npx * per_px / (out[k]["rest_ms"] * 1e-3) / 1e12, 3)  # over k_raygen + k_motion, the pass's own kernels
    for k, per_px in (("temporal_with_motion_input", TEMPORAL_BYTES + 16), ("temporal_without", TEMPORAL_BYTES)):
        out[k]["bytes_per_foreground_pixel"] = per_px
        out[k]["tb_per_s"] = round(fg * per_px / (out[k]["ms"] * 1e-3) / 1e12, 3)
    result = {"scene": "atrium + one moved column", "detail": args.detail, "size": [W, H], "instance_mode": args.instance_mode,
              "foreground_pixels": fg, "moved_pixels": moved, "moved_gather_bytes": MOVED_GATHER_BYTES, "mean_history_on_moved_pixels": round(n_moved, 3),
              "pass": out}
    if deform:
        result["deform"] = deform
    pt.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
