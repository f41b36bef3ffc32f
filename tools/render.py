#!/usr/bin/env python3
"""Render a scene to PNG through the three passes (gbuffer -> refrence_mode -> postprocess), optionally progressively
(BASELINE.json configs[4]: accumulation over passes with blendfactor = 1/(pass+1), RMSE-vs-spp curve against the final image).

  python tools/render.py --scene atrium --size 960x540 --spp 64 --passes 16 --out gpurun_out/atrium.png --curve gpurun_out/curve.json
  python tools/render.py --scene cornell_ref --size 1920x1080 --spp 64 --passes 64 --bounces 2 --flags 0 \
                         --compare resources/refrence_480x270.png --side-by-side profiles/r02_cornell_ref_side_by_side.png
                          (informational only: a 480x270 copy of the reference tree's resources/refrence.png, a Blender-Cycles render of
                          the box scenes.cornell_ref() rebuilds from the reference's processed asset; Cycles is not this estimator)
  python tools/render.py --scene atrium --size 1920x1080 --spp 1 --denoise --out atrium_1spp_denoised.png
                         (the a-trous filter of DESIGN.md section 4f between refrence_mode and postprocess; for low sample counts)
  python tools/render.py --scene atrium --size 1920x1080 --spp 1 --temporal 16 --denoise --out atrium_1spp_temporal.png
                         (16 frames of 1 spp along a small camera move through the "temporal" pass of DESIGN.md section 4g -- reprojected
                         accumulation -- and, with --denoise, the a-trous filter fed with its variance; the last frame is written)
  python tools/render.py --scene atrium --size 1920x1080 --spp 256 --adaptive 0.05 --spp-map atrium_spp.png --out atrium_adaptive.png
                         (the "adaptive" pass of DESIGN.md section 4l: --spp is the cap, pixels stop at a relative standard error of
                         0.05; --spp-map writes the sample counts as a grey PNG, white = the cap)
  python tools/render.py --scene atrium --size 1920x1080 --spp 256 --aa --aperture 0.05 --focus 8 --out atrium_dof.png
                         (per-sample camera rays, DESIGN.md section 4m: --aa antialiases over the pixel, --aperture / --focus add a thin lens)
  python tools/render.py --scene glass_cornell --size 1920x1080 --spp 256 --bounces 8 --adaptive 0.3 --spp-map glass_spp.png --out glass_adaptive.png
                         (--adaptive with --aa, --aperture or a scene with glass: the pass's coverage mode, every pixel sampled to the threshold)
  python tools/render.py --scene glass_cornell --size 1920x1080 --spp 4 --bounces 8 --denoise --guide --out glass_4spp_denoised.png
                         (--guide: the a-trous filter guided by the lens frame's own camera samples)
  python tools/render.py --scene glass_cornell --size 1920x1080 --spp 1 --bounces 8 --temporal 16 --denoise --guide --out glass_1spp_temporal.png
                         (--temporal with --guide: the "temporal" pass takes its surface records from the guide images too, section 4v)
  python tools/render.py --scene material_cornell --size 960x540 --spp 64 --flags 47 --textured-emitters --out material_cornell_nee.png
                         (flags 47 = the full estimator + RT3_F_NEE_EMISSIVE: the panel's lamps are sampled directly)
  python tools/render.py --scene skinned_arm --size 960x540 --spp 64 --time 1.0 --out arm_bent.png
                         (--time T [--animation N]: the scene's skins posed on the device at T seconds; a rigged --glb works too)
  python tools/render.py --glb resources/sponza_scene.glb --exr resources/skybox2.exr ...               (if the real assets are dropped in)
"""
import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="atrium", choices=["atrium", "cornell", "cornell_ref", "cutout_cornell", "material_cornell", "lit_room", "glass_cornell", "sunlit_room", "amber_cornell", "frosted_cornell", "neon_room", "skinned_arm"])
    ap.add_argument("--time", type=float, default=None, metavar="T",
                    help="pose the scene's skins at T seconds of --animation before rendering (PathTracer.pose, DESIGN.md section 4z); try --scene skinned_arm --time 1")
    ap.add_argument("--animation", type=int, default=0, metavar="N", help="with --time: which of the file's animations")
    ap.add_argument("--glb", default=None)
    ap.add_argument("--exr", default=None)
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--size", default="960x540")
    ap.add_argument("--spp", type=int, default=64, help="samples per pass")
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--flags", type=int, default=-1)
    ap.add_argument("--denoise", action="store_true", help="filter Light with the 'denoise' pass before the tone map (last pass only)")
    ap.add_argument("--denoise-iterations", type=int, default=5, help="a-trous iterations of --denoise (0..8)")
    ap.add_argument("--temporal", type=int, default=0, metavar="N",
                    help="render N frames of --spp along a small camera move through the 'temporal' pass and write the last one (replaces --passes)")
    ap.add_argument("--adaptive", type=float, default=None, metavar="THRESHOLD",
                    help="render with the 'adaptive' pass: --spp is the cap, a pixel stops at this relative standard error of its mean")
    ap.add_argument("--min-spp", type=int, default=16, help="with --adaptive: samples every pixel gets first")
    ap.add_argument("--step", type=int, default=16, help="with --adaptive: samples per later round")
    ap.add_argument("--spp-map", default=None, help="with --adaptive: write the per-pixel sample counts as a grey PNG here (white = the cap)")
    ap.add_argument("--aa", action="store_true", help="per-sample camera rays: every sample's film point is drawn from the whole pixel (DESIGN.md section 4m)")
    ap.add_argument("--aperture", type=float, default=0.0, metavar="R", help="thin lens of radius R (world units); implies per-sample camera rays")
    ap.add_argument("--focus", type=float, default=1.0, metavar="F", help="with --aperture: view depth of the plane of focus")
    ap.add_argument("--guide", action="store_true", help="with --denoise or --temporal and a lens (--aa, --aperture, a scene with glass): guide the filters by the "
                                                         "frame's own camera samples instead of the pinhole G-buffer (PathTracer.set_guide, DESIGN.md sections 4u, 4v)")
    ap.add_argument("--out", default="gpurun_out/render.png")
    ap.add_argument("--curve", default=None, help="write the RMSE-vs-spp convergence curve (JSON) here")
    ap.add_argument("--roulette", nargs="?", type=int, const=2, default=None, metavar="START",
                    help="Russian roulette on the extension rays from vertex START on (default 2), survival floor 1/16 (DESIGN.md section 4o)")
    ap.add_argument("--pane-shadows", action="store_true", help="sample lights through thin-walled glass (PathTracer.set_pane_shadows, DESIGN.md section 4q)")
    ap.add_argument("--textured-emitters", action="store_true",
                    help="sample emitters whose emission carries an emissive texture (PathTracer.set_textured_emitters, DESIGN.md section 4x); needs RT3_F_NEE_EMISSIVE (32) in --flags")
    ap.add_argument("--fog", type=float, default=None, metavar="SIGMA_S",
                    help="fog over the scene's bounds: scattering coefficient per world unit, single scattering (PathTracer.set_medium, DESIGN.md section 4y); "
                         "switches per-sample camera rays on; try --scene sunlit_room --pane-shadows --fog 0.15")
    ap.add_argument("--fog-absorb", type=float, default=0.0, metavar="A", help="with --fog: absorption coefficient per world unit")
    ap.add_argument("--fog-g", type=float, default=0.0, metavar="G", help="with --fog: Henyey-Greenstein asymmetry in (-1, 1); > 0 scatters forward")
    ap.add_argument("--rough-glass", action="store_true", help="frosted glass: rough transmission on glass with roughness > 0 (PathTracer.set_rough_transmission, DESIGN.md section 4t)")
    ap.add_argument("--compare", default=None, help="PNG to compare the tone-mapped result with (RMSE of 8-bit values / 255)")
    ap.add_argument("--side-by-side", default=None, help="with --compare: write [render | reference] at the reference's size here")
    ap.add_argument("--report", default=None, help="with --compare: write the numbers and the scene parameters as JSON here")
    args = ap.parse_args()

    from PIL import Image

    from raytracer3_amd import _lib as L
    from raytracer3_amd import assets, scenes
    from raytracer3_amd.renderer import DEFAULT_FLAGS, Camera, PathTracer, scene_medium

    W, H = (int(x) for x in args.size.split("x"))
    if args.glb:
        mesh, cam_kw = assets.GltfMeshLoader.load(args.glb), scenes.ATRIUM_CAMERA
    elif args.scene == "cornell":
        mesh, cam_kw = scenes.cornell(), scenes.CORNELL_CAMERA
    elif args.scene == "cutout_cornell":  # alpha-masked cutout geometry
        mesh, cam_kw = scenes.cutout_cornell(), scenes.CORNELL_CAMERA
    elif args.scene == "lit_room":  # point, spot and directional lights
        mesh, cam_kw = scenes.lit_room(), scenes.CORNELL_CAMERA
    elif args.scene == "material_cornell":  # metallic-roughness, normal and emissive maps
        mesh, cam_kw = scenes.material_cornell(), scenes.CORNELL_CAMERA
    elif args.scene == "glass_cornell":  # a solid glass sphere and a thin-walled pane; set_scene switches the pinhole lens on
        mesh, cam_kw = scenes.glass_cornell(), scenes.CORNELL_CAMERA
    elif args.scene == "frosted_cornell":  # glass_cornell with roughness 0.3 on the sphere and 0.15 on the pane; try --rough-glass
        mesh, cam_kw = scenes.frosted_cornell(), scenes.CORNELL_CAMERA
    elif args.scene == "amber_cornell":  # absorbing glass: an amber block and two green spheres of two sizes
        mesh, cam_kw = scenes.amber_cornell(), scenes.CORNELL_CAMERA
    elif args.scene == "sunlit_room":  # a closed room lit through one window by the sky and a sun; try --pane-shadows
        mesh, cam_kw = scenes.sunlit_room(), scenes.SUNLIT_ROOM_CAMERA
    elif args.scene == "neon_room":  # a room lit only by a sign whose emissive texture is mostly black; try --textured-emitters
        mesh, cam_kw = scenes.neon_room(), scenes.NEON_ROOM_CAMERA
    elif args.scene == "skinned_arm":  # a three-joint skinned tube with a morph target and a bend animation; try --time 1
        mesh, cam_kw = scenes.skinned_arm(), scenes.SKINNED_ARM_CAMERA
    elif args.scene == "cornell_ref":
        mesh, cam_kw = scenes.cornell_ref(), scenes.CORNELL_REF_CAMERA
    else:
        mesh, cam_kw = scenes.atrium(args.detail), scenes.ATRIUM_CAMERA
    sky = assets.read_exr(args.exr) if args.exr else (scenes.sky(2048, 1024) if args.scene in ("atrium", "sunlit_room") or args.glb else None)
    if sky is not None:  # rt3_scene_set_sky wants finite, non-negative radiance; HDR files carry inf / NaN / tiny negatives
        sky = np.clip(np.nan_to_num(sky, nan=0.0, posinf=65504.0, neginf=0.0), 0.0, 65504.0).astype(np.float32)
    flags = args.flags if args.flags >= 0 else (DEFAULT_FLAGS if sky is not None else L.F_FACEFORWARD | L.F_SPECULAR)
    if args.flags < 0 and len(getattr(mesh, "lights", ())):  # a scene with punctual lights is lit by them
        flags |= L.F_NEE_PUNCTUAL
    pt = PathTracer((W, H))
    pt.set_pane_shadows(args.pane_shadows)
    pt.set_rough_transmission(args.rough_glass)
    pt.set_textured_emitters(args.textured_emitters)
    pt.set_scene(mesh, sky, assets.load_bluenoise())
    if args.time is not None:
        if not mesh.skins:
            ap.error("--time poses skins: this scene has none (Mesh.skins)")
        pt.pose(args.time, args.animation)
    if args.denoise:
        pt.ctx.set_denoise_params(iterations=args.denoise_iterations)
    if args.aa or args.aperture > 0.0:
        if (args.temporal or args.denoise) and not args.guide:
            ap.error("--aa / --aperture do not combine with --temporal or --denoise unless --guide: those passes are guided by the pinhole G-buffer")
        pt.set_lens(args.aperture, args.focus, 1.0)
    if args.fog is not None:
        if args.temporal or args.denoise:
            ap.error("--fog does not combine with --temporal or --denoise: those passes do not see the medium")
        pt.set_medium(scene_medium(mesh, args.fog, args.fog_absorb, args.fog_g))
    if args.guide:
        if args.adaptive is not None:
            ap.error("--guide guides refrence_mode frames: it does not combine with --adaptive")
        if not pt.ctx.get_lens()[1]:
            ap.error("--guide needs per-sample camera rays: --aa, --aperture or a scene with glass")
        pt.set_guide(True, temporal=bool(args.temporal))
    if args.roulette is not None:
        pt.set_roulette(args.roulette)
    adaptive = None
    if args.adaptive is not None:
        if args.temporal:
            ap.error("--adaptive renders single frames: it does not combine with --temporal")
        adaptive = L.AdaptiveParams(min_samples=args.min_spp, step=args.step, threshold=args.adaptive)
        if pt.ctx.get_lens()[1]:  # --aa, --aperture or a scene with glass: every pixel is sampled to the threshold
            pt.set_adaptive_coverage(True)
    cam = Camera(cam_kw["position"], cam_kw["direction"], math.radians(cam_kw["fov_deg"]), W / H)
    history, t0 = [], time.perf_counter()
    for k in range(args.temporal):  # the camera slides and turns by a few pixels per frame; every frame reprojects the one before
        step = np.float32(k) * np.array([0.02, 0.0, 0.01], np.float32)
        moved = Camera(cam.position + step, cam.direction + np.float32(k) * np.array([0.0, 0.0, 0.012], np.float32), cam.fov, W / H)
        g = pt.make_gconst(moved, args.spp, args.bounces, frame=k + 1, flags=flags)
        last = k == args.temporal - 1
        pt.render(g, postprocess=last, denoise=args.denoise and last, temporal=True)
    for p in range(args.passes if not args.temporal else 0):
        g = pt.make_gconst(cam, args.spp, args.bounces, frame=p, blendfactor=1.0 / (p + 1), flags=flags)
        last = p == args.passes - 1
        pt.render(g, postprocess=last, denoise=args.denoise and last, adaptive=adaptive)
        if args.curve:
            history.append(pt.light()[..., :3].copy())
        if p != args.passes - 1:
            pt.copy_light_to_prev()
    dt = time.perf_counter() - t0
    st = pt.ctx.stats()
    color = pt.color()
    light = pt.light()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    img8 = (np.clip(color[..., :3], 0, 1) * 255 + 0.5).astype(np.uint8)
    Image.fromarray(img8).save(args.out)
    rays = st.extension_rays + st.shadow_rays
    print(f"{args.out}: {W}x{H} {args.temporal or args.passes} x {args.spp} spp, {rays / 1e6:.0f} Mrays in {dt:.2f} s ({rays / dt / 1e6:.0f} Mrays/s incl. host), mean radiance {light[..., :3].mean():.4f}")
    if args.roulette is not None:  # of the last pass
        tested, ended = pt.roulette_info()
        print(f"roulette from vertex {args.roulette}: {ended / 1e6:.2f} M of {tested / 1e6:.2f} M tested extension rays ended")
    if args.fog is not None:  # of the last pass
        segments, fog_rays = pt.medium_info()
        print(f"fog sigma_s {args.fog} sigma_a {args.fog_absorb} g {args.fog_g}: {segments / 1e6:.2f} M segments in the medium, {fog_rays / 1e6:.2f} M in-scatter shadow rays")
    if adaptive is not None:  # of the last pass
        n = pt.sample_counts()
        rounds, paths, capped = pt.ctx.adaptive_info()
        fgn = n[n > 0]  # (with a lens: every pixel)
        print(f"adaptive: threshold {args.adaptive}, cap {args.spp}: {rounds} rounds, {paths / 1e6:.1f} M paths, mean {fgn.mean() if fgn.size else 0:.1f} spp over "
              f"{fgn.size} {'pixels' if pt.ctx.get_lens()[1] else 'foreground pixels'}, {capped} at the cap")
        if args.spp_map:
            Path(args.spp_map).parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray((n.astype(np.float64) * (255.0 / max(1, args.spp)) + 0.5).astype(np.uint8)).save(args.spp_map)
    if args.curve:
        ref = history[-1].astype(np.float64)
        curve = [{"spp": (i + 1) * args.spp, "rmse_vs_final": float(np.sqrt(np.mean((h - ref) ** 2)))} for i, h in enumerate(history[:-1])]
        Path(args.curve).write_text(json.dumps({"size": [W, H], "spp_per_pass": args.spp, "passes": args.passes, "curve": curve}, indent=1))
        print("convergence:", ", ".join(f"{c['spp']}spp {c['rmse_vs_final']:.4f}" for c in curve[:: max(1, len(curve) // 8)]))
    if args.compare:
        refimg = Image.open(args.compare).convert("RGB")
        rw, rh = refimg.size
        if W % rw == 0 and H % rh == 0 and W // rw == H // rh:  # box-filter the render down to the reference's size
            k = W // rw
            mine = img8.reshape(rh, k, rw, k, 3).astype(np.float64).mean((1, 3)) / 255.0
            ref = np.array(refimg, np.float64) / 255
        else:
            mine, ref = img8 / 255.0, np.array(refimg.resize((W, H)), np.float64) / 255
        rmse = float(np.sqrt(np.mean((mine - ref) ** 2)))
        print(f"informational RMSE vs {args.compare} (8-bit, display referred, another renderer): {rmse:.4f}")
        if args.side_by_side:
            Image.fromarray(np.concatenate([(mine * 255 + 0.5).astype(np.uint8), (ref * 255 + 0.5).astype(np.uint8)], 1)).save(args.side_by_side)
        if args.report:
            Path(args.report).write_text(json.dumps({
                "scene": args.scene, "render": {"size": [W, H], "spp": args.spp * args.passes, "bounces": args.bounces, "flags": flags},
                "camera": {k: (list(v) if isinstance(v, tuple) else v) for k, v in cam_kw.items()},
                "light_emission": scenes.CORNELL_REF_EMISSION if args.scene == "cornell_ref" else None,
                "compare": args.compare, "compared_at": [int(mine.shape[1]), int(mine.shape[0])], "rmse_8bit": rmse,
                "note": "informational: the reference image is a Blender-Cycles render (100 spp, its own view transform); scene rebuilt from the "
                        "eight cubes / materials of the reference's processed box.glb, placements and emission fitted to the image"}, indent=1))
    pt.close()


if __name__ == "__main__":
    main()
