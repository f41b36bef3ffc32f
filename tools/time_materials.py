#!/usr/bin/env python3
"""Cost of material textures on the bench frame (scenes.atrium under scenes.sky): frame time and the k_shade time of
one frame (RT3_OPT_PROFILE) for five versions of the same scene:
  none      no material-texture table: the plain k_shade instances (what the scene costs today)
  mr        a metallic-roughness map on every geometry
  normal    a normal map on every geometry (tangent records, the dependent gather)
  emissive  an emissive map on every geometry (a few geometries emit; the others multiply zero)
  all       the three maps on every geometry
The maps are 256 x 256 textures generated from a seed; uvs are the scene's own.  With --resources the tool also compiles rt3_shade.hip
with -Rpass-analysis=kernel-resource-usage (the library's own flags) and reports VGPRs, scratch and occupancy of every k_shade instance.
Prints one JSON line (medians of --frames timed frames after --warmup).

  python tools/time_materials.py --size 1920x1080 --spp 16 --bounces 4 --resources --out time_materials.json
"""
import argparse
import json
import re
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def shade_resources():
    """{k_shade<...>: {vgprs, scratch_bytes, waves_per_simd, lds_bytes}} from the compiler's resource remarks"""
    csrc = ROOT / "raytracer3_amd" / "csrc"
    flags = re.search(r"^FLAGS = (.*)$", (csrc / "Makefile").read_text(), re.M).group(1).replace("$(ARCH)", "gfx950").split()
    r = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", "rt3_shade.hip", "-o", "/dev/null"],
                       cwd=csrc, capture_output=True, text=True, check=True)
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            t = re.match(r"_ZN3rt37k_shadeI((?:Lb[01]E)+)E", m.group(1))
            cur = out.setdefault("k_shade<" + ", ".join("true" if b == "1" else "false" for b in re.findall(r"Lb([01])E", t.group(1))) + ">", {}) if t else None
        for key, name in (("VGPRs", "vgprs"), ("ScratchSize [bytes/lane]", "scratch_bytes"), ("Occupancy [waves/SIMD]", "waves_per_simd"), ("LDS Size [bytes/block]", "lds_bytes")):
            m = re.search(r"\s" + re.escape(key) + r": (\d+)", line)
            if m and cur is not None:
                cur[name] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer, default_camera

    W, H = (int(x) for x in args.size.split("x"))
    rng = np.random.default_rng(args.seed)
    mesh = scenes.atrium(args.detail)
    n, first = len(mesh.geometries), len(mesh.textures)
    maps = [np.ascontiguousarray(rng.integers(0, 256, (256, 256, 4), dtype=np.uint8)) for _ in range(3)]  # mr, normal, emissive
    maps[1][..., 2] = 192 + maps[1][..., 2] // 4
    columns = ("metallic_roughness_texture", "normal_texture", "emissive_texture")

    def variant(which):
        t = assets.no_material_textures(n)
        for k in which:
            t[columns[k]] = first + k
        return assets.Mesh(mesh.vertices, mesh.indices, mesh.geometries, mesh.prim_counts, list(mesh.names), list(mesh.textures) + maps, mesh.alpha_cutoffs, t)

    variants = {"none": variant(()), "mr": variant((0,)), "normal": variant((1,)), "emissive": variant((2,)), "all": variant((0, 1, 2))}
    c = scenes.ATRIUM_CAMERA
    cam = default_camera((W, H), c["position"], c["direction"], c["fov_deg"])
    result = {"scene": "atrium", "detail": args.detail, "size": [W, H], "spp": args.spp, "bounces": args.bounces, "flags": DEFAULT_FLAGS}
    sky, bn = scenes.sky(2048, 1024), assets.load_bluenoise()
    for name, m in variants.items():
        pt = PathTracer((W, H))
        pt.set_scene(m, sky, bn)
        for k in range(args.warmup):
            pt.render(pt.make_gconst(cam, args.spp, args.bounces, frame=k, flags=DEFAULT_FLAGS))
        ms = []
        for k in range(args.frames):
            g = pt.make_gconst(cam, args.spp, args.bounces, frame=k, flags=DEFAULT_FLAGS)
            pt.ctx.wait()
            t0 = time.perf_counter()
            pt.render(g)  # waits for the frame
            ms.append((time.perf_counter() - t0) * 1e3)
        shade = []
        pt.ctx.set_option(L.OPT_PROFILE, 1)
        for k in range(args.frames):
            pt.ctx.stats_reset()
            pt.render(pt.make_gconst(cam, args.spp, args.bounces, frame=k, flags=DEFAULT_FLAGS))
            shade.append(pt.ctx.stats().shade_ms)
        result[name] = {"frame_ms": round(statistics.median(ms), 3), "shade_ms": round(statistics.median(shade), 3), "frame_ms_all": [round(x, 3) for x in ms]}
        pt.close()
    if args.resources:
        result["k_shade_resources"] = shade_resources()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
