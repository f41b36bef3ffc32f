#!/usr/bin/env python3
"""Renders tests/golden/punctual_ref.npz: the float64 reference tracer with punctual lights (tests/ref_lights.radiance_samples_lit) on the
lit rooms of tests/punctual_worlds.CASES.  Run from the repo root:  python tests/golden/gen_punctual_ref.py [--jobs N]
Takes some minutes; the output is the same bytes on every run.  The format is gen_integrator_ref.py's: per case `c`

  c_mean, c_se        (2, 3, 3)  means of the 16 x 16 pixel blocks per channel and their standard errors
  c_cover             (32, 48)   which pixels the primary rays hit
  c_seed, c_spp       scalars    the seed and the samples per pixel
  c_prefix_mean, _se  (2, 3, 3)  the same statistics of the first ref_pathtrace.CHUNK_SPP samples alone (the drift test re-renders them)"""
import argparse
import importlib.util
import sys
from multiprocessing import Pool
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import integrator_worlds as IW  # noqa: E402
import punctual_worlds as PW  # noqa: E402
import ref_lights as RL  # noqa: E402
import ref_pathtrace as RP  # noqa: E402

OUT = Path(__file__).resolve().parent / "punctual_ref.npz"


def room_scene(name):
    mesh, sky = PW.room(name)
    return RP.Scene(mesh, sky=sky), mesh.lights


def render_case(name, spp=None):
    """{array name: array} of one case; `spp` overrides the case's sample count (the drift test renders the prefix alone)"""
    flags, bounces, _, _, case_spp, seed, _ = PW.CASES[name]
    spp = spp or case_spp
    scene, lights = room_scene(name)
    out = {}
    for tag, n in (("prefix_", RP.CHUNK_SPP), ("", spp)):
        mean, var = RL.render_lit(scene, lights, IW.ROOM_CAMERA, IW.WINDOW_ROOM, flags, bounces, n, seed)
        out[f"{name}_{tag}mean"], out[f"{name}_{tag}se"] = RP.block_stats(mean, var, n)
    out[f"{name}_cover"] = RP.coverage(scene, IW.ROOM_CAMERA, IW.WINDOW_ROOM)
    out[f"{name}_seed"], out[f"{name}_spp"] = np.array(seed, np.int64), np.array(spp, np.int64)
    return out


def _save(path, arrays):  # gen_integrator_ref.save: an .npz without time stamps
    spec = importlib.util.spec_from_file_location("gen_integrator_ref", Path(__file__).resolve().parent / "gen_integrator_ref.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    gen.save(path, arrays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=len(PW.CASES))
    ap.add_argument("--out", default=str(OUT))
    a = ap.parse_args()
    with Pool(max(1, a.jobs)) as pool:
        parts = pool.map(render_case, list(PW.CASES))
    arrays = {}
    for name, p in zip(PW.CASES, parts):
        arrays.update(p)
        rel = p[f"{name}_se"] / np.maximum(p[f"{name}_mean"], 1e-30)
        print(f"{name}: {int(p[f'{name}_spp'])} spp, relative standard error per block-channel: median {np.median(rel):.3%}, max {rel.max():.3%}")
    _save(a.out, arrays)


if __name__ == "__main__":
    main()
