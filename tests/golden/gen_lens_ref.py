#!/usr/bin/env python3
"""Renders tests/golden/lens_ref.npz: the float64 lens tracer (tests/ref_lens.py) on integrator_worlds.open_room() through the thin lens
lens_worlds.ROOM_LENS, for every case of lens_worlds.ROOM_CASES, and on lens_worlds.material_room() (material textures, surfaces from
tests/ref_materials.py) for lens_worlds.MATERIAL_CASES.  Run from the repo root:  python tests/golden/gen_lens_ref.py [--jobs N]
Takes some minutes; the output is the same bytes on every run.

Per case `c` the file holds only arrays, named and shaped as tests/golden/integrator_ref.npz names them:
  c_mean, c_se        (2, 3, 3)  means of the 16 x 16 pixel blocks per channel and their standard errors
  c_cover             (32, 48)   all true: a lens frame writes every pixel
  c_seed, c_spp       scalars    the seed and the samples per pixel
  c_prefix_mean, _se  (2, 3, 3)  the same statistics of the first ref_pathtrace.CHUNK_SPP samples alone (the drift test re-renders them)"""
import argparse
import sys
from multiprocessing import Pool
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "golden"))
import integrator_worlds as IW  # noqa: E402
import lens_worlds as LW  # noqa: E402
import ref_lens as RL  # noqa: E402
import ref_pathtrace as RP  # noqa: E402
from gen_integrator_ref import room_scene, save  # noqa: E402

OUT = Path(__file__).resolve().parent / "lens_ref.npz"


CASES = {**LW.ROOM_CASES, **LW.MATERIAL_CASES}


def render_prefix(name, spp):
    """block means and standard errors of the first `spp` samples of one case"""
    flags, bounces, specular, _, seed, _ = CASES[name]
    if name in LW.MATERIAL_CASES:  # the textured room, every vertex from tests/ref_materials.py
        mesh, cam = LW.material_room()
        scene = RP.Scene(mesh, sky=LW.constant_sky(LW.MATERIAL_SKY_C))
        pinv, vinv = RL.camera_matrices(cam, IW.WINDOW_ROOM)
        mean, var = RL.render(scene, pinv, vinv, IW.WINDOW_ROOM, LW.MATERIAL_LENS, flags, bounces, spp, seed, RL.textured_surface(mesh, scene))
        return RP.block_stats(mean, var, spp)
    pinv, vinv = RL.camera_matrices(IW.ROOM_CAMERA, IW.WINDOW_ROOM)
    mean, var = RL.render(room_scene(specular), pinv, vinv, IW.WINDOW_ROOM, LW.ROOM_LENS, flags, bounces, spp, seed)
    return RP.block_stats(mean, var, spp)


def render_case(name):
    _, _, _, spp, seed, _ = CASES[name]
    out = {}
    for tag, n in (("prefix_", RP.CHUNK_SPP), ("", spp)):
        out[f"{name}_{tag}mean"], out[f"{name}_{tag}se"] = render_prefix(name, n)
    W, H = IW.WINDOW_ROOM
    out[f"{name}_cover"] = np.ones((H, W), bool)
    out[f"{name}_seed"], out[f"{name}_spp"] = np.array(seed, np.int64), np.array(spp, np.int64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=len(CASES))
    ap.add_argument("--out", default=str(OUT))
    a = ap.parse_args()
    with Pool(max(1, a.jobs)) as pool:
        parts = pool.map(render_case, list(CASES))
    arrays = {}
    for name, p in zip(CASES, parts):
        arrays.update(p)
        rel = p[f"{name}_se"] / np.maximum(p[f"{name}_mean"], 1e-30)
        print(f"{name}: {int(p[f'{name}_spp'])} spp, relative standard error per block-channel: median {np.median(rel):.3%}, max {rel.max():.3%}")
    save(a.out, arrays)


if __name__ == "__main__":
    main()
