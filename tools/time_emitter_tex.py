#!/usr/bin/env python3
"""Cost and gain of textured emitters (rt3_scene_set_textured_emitters, DESIGN.md sections 4x and 7).

Frames: material_cornell, neon_room and the benchmark frame (the atrium from the bench camera, which has no textured emitter: on must
equal off), each with the mode off and on under the full estimator + RT3_F_NEE_EMISSIVE.  The configurations are visited in turn, --rounds
times over, so that drift of the machine lands on all of them alike; each visit renders --warmup frames (the first remakes the light
table) and then times --frames frames (host clock around a waited frame).  Per configuration: the median, the smallest and the largest
of all its timed frames, k_emit_tex's launches per frame, and its own time -- the rise of rt3_stats.other_ms in one profiled frame over
the profiled mode-off frame (RT3_OPT_PROFILE; the category of the streaming kernels).
Table: the host time of remaking the light table (toggle the mode, read the masses back), median of --frames, with the mode on
(k_emit_prims + k_emit_tex_power + selection) and off (k_emit_prims + selection over the untextured emitters).
Quality: at --q-size, the mean squared error of a --spp frame against the mean of --ref-frames x --ref-spp mode-off frames, and the
efficiency 1 / (seconds x MSE), on against off.  Prints one JSON line.

  python tools/time_emitter_tex.py --size 1920x1080 --spp 64 --out time_emitter_tex.json
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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--q-size", default="96x64")
    ap.add_argument("--ref-spp", type=int, default=512)
    ap.add_argument("--ref-frames", type=int, default=8)
    ap.add_argument("--scenes", default="material_cornell,neon_room,atrium")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer, default_camera

    W, H = (int(x) for x in args.size.split("x"))
    QW, QH = (int(x) for x in args.q_size.split("x"))
    flags = DEFAULT_FLAGS | L.F_NEE_EMISSIVE
    worlds = {"material_cornell": (scenes.material_cornell, scenes.CORNELL_CAMERA, False), "neon_room": (scenes.neon_room, scenes.NEON_ROOM_CAMERA, False),
              "atrium": (scenes.atrium, scenes.ATRIUM_CAMERA, True)}
    result = {"size": [W, H], "spp": args.spp, "bounces": args.bounces, "flags": flags, "rounds": args.rounds, "frames_per_round": args.frames, "scenes": {}}
    for name in args.scenes.split(","):
        make, cam_kw, with_sky = worlds[name]
        mesh = make()
        sky = scenes.sky(2048, 1024) if with_sky else None
        pt = PathTracer((W, H))
        pt.set_scene(mesh, sky, assets.load_bluenoise())
        cam = default_camera((W, H), cam_kw["position"], cam_kw["direction"], cam_kw["fov_deg"])
        runs = {on: {"ms_all": [], "ms_rounds": []} for on in (False, True)}
        for _ in range(args.rounds):
            for on in (False, True):
                pt.set_textured_emitters(on)
                for k in range(args.warmup):
                    pt.render(pt.make_gconst(cam, args.spp, args.bounces, frame=k, flags=flags))
                ms = []
                pt.ctx.stats_reset()
                for k in range(args.frames):
                    g = pt.make_gconst(cam, args.spp, args.bounces, frame=k, flags=flags)
                    pt.ctx.wait()
                    t0 = time.perf_counter()
                    pt.render(g)  # waits for the frame
                    ms.append((time.perf_counter() - t0) * 1e3)
                st = pt.ctx.stats()
                runs[on].update(emit_tex_launches_per_frame=st.emit_tex_launches // args.frames, shadow_rays_per_frame=st.shadow_rays // args.frames,
                                table=list(pt.ctx.light_masses(flags)[:2]), textured=int((pt.ctx.light_emit_tex(flags)[1] >= 0).sum()), mean=float(pt.light()[..., :3].mean()))
                runs[on]["ms_rounds"].append(round(statistics.median(ms), 3))
                runs[on]["ms_all"] += [round(x, 3) for x in ms]
        # k_emit_tex alone: HIP events around every launch of the streaming category, one frame each
        pt.ctx.set_option(L.OPT_PROFILE, 1)
        other = {}
        for on in (False, True):
            pt.set_textured_emitters(on)
            pt.render(pt.make_gconst(cam, args.spp, args.bounces, frame=0, flags=flags))
            pt.ctx.stats_reset()
            pt.render(pt.make_gconst(cam, args.spp, args.bounces, frame=1, flags=flags))
            other[on] = pt.ctx.stats().other_ms
        pt.ctx.set_option(L.OPT_PROFILE, 0)
        # the table alone
        table_ms = {}
        for on in (False, True):
            ms = []
            for _ in range(args.frames + 1):
                pt.set_textured_emitters(not on)
                pt.ctx.light_masses(flags)
                pt.set_textured_emitters(on)
                pt.ctx.wait()
                t0 = time.perf_counter()
                pt.ctx.light_masses(flags)
                ms.append((time.perf_counter() - t0) * 1e3)
            table_ms[on] = round(statistics.median(ms[1:]), 4)
        pt.close()
        # quality at the small size
        pq = PathTracer((QW, QH))
        pq.set_scene(mesh, scenes.sky(256, 128) if with_sky else None, assets.load_bluenoise())
        camq = default_camera((QW, QH), cam_kw["position"], cam_kw["direction"], cam_kw["fov_deg"])

        def shot(on, spp, index):
            pq.set_textured_emitters(on)
            pq.ctx.wait()
            t0 = time.perf_counter()
            pq.render(pq.make_gconst(camq, spp, args.bounces, frame=index, flags=flags))
            return pq.light()[..., :3].astype(np.float64), time.perf_counter() - t0

        ref = np.mean([shot(False, args.ref_spp, 1000 + k)[0] for k in range(args.ref_frames)], axis=0)
        quality = {}
        for on in (False, True):
            shot(on, args.spp, 0)
            imgs = [shot(on, args.spp, 10 + k) for k in range(4)]
            mse = float(np.mean([np.mean((img - ref) ** 2) for img, _ in imgs]))
            sec = statistics.median(t for _, t in imgs)
            quality[on] = {"mse": mse, "seconds": sec, "efficiency": (1.0 / (sec * mse)) if mse > 0 else None}
        pq.close()
        entry = {}
        for on in (False, True):
            r = runs[on]
            entry["on" if on else "off"] = dict(r, ms=round(statistics.median(r["ms_all"]), 3), ms_min=min(r["ms_all"]), ms_max=max(r["ms_all"]),
                                                other_ms_profiled=round(other[on], 4), table_ms=table_ms[on], quality=quality[on])
        entry["k_emit_tex_ms_per_frame"] = round(other[True] - other[False], 4)
        entry["ref_spp"] = args.ref_spp * args.ref_frames
        result["scenes"][name] = entry
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
