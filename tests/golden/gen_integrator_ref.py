#!/usr/bin/env python3
"""Renders tests/golden/integrator_ref.npz: the float64 reference tracer (tests/ref_pathtrace.py) on integrator_worlds.open_room()
for every case of integrator_worlds.ROOM_CASES.  Run from the repo root:  python tests/golden/gen_integrator_ref.py [--jobs N]
Takes some minutes; the output is the same bytes on every run.

Per case `c` the file holds only arrays:
  c_mean, c_se        (2, 3, 3)  means of the 16 x 16 pixel blocks per channel and their standard errors
  c_cover             (32, 48)   which pixels the primary rays hit
  c_seed, c_spp       scalars    the seed and the samples per pixel
  c_prefix_mean, _se  (2, 3, 3)  the same statistics of the first ref_pathtrace.CHUNK_SPP samples alone (the drift test re-renders them)"""
import argparse
import io
import sys
import zipfile
from multiprocessing import Pool
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import integrator_worlds as IW  # noqa: E402
import ref_pathtrace as RP  # noqa: E402

OUT = Path(__file__).resolve().parent / "integrator_ref.npz"


def room_scene(specular):
    return RP.Scene(IW.open_room(specular), sky=IW.room_sky())


def render_case(name, spp=None):
    """{array name: array} of one case; `spp` overrides the case's sample count (the drift test renders the prefix alone)"""
    flags, bounces, specular, case_spp, seed, _ = IW.ROOM_CASES[name]
    spp = spp or case_spp
    scene = room_scene(specular)
    out = {}
    for tag, n in (("prefix_", RP.CHUNK_SPP), ("", spp)):
        mean, var = RP.render(scene, IW.ROOM_CAMERA, IW.WINDOW_ROOM, flags, bounces, n, seed)
        out[f"{name}_{tag}mean"], out[f"{name}_{tag}se"] = RP.block_stats(mean, var, n)
    out[f"{name}_cover"] = RP.coverage(scene, IW.ROOM_CAMERA, IW.WINDOW_ROOM)
    out[f"{name}_seed"], out[f"{name}_spp"] = np.array(seed, np.int64), np.array(spp, np.int64)
    return out


def save(path, arrays):
    """an .npz without time stamps, so that the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=len(IW.ROOM_CASES))
    ap.add_argument("--out", default=str(OUT))
    a = ap.parse_args()
    with Pool(max(1, a.jobs)) as pool:
        parts = pool.map(render_case, list(IW.ROOM_CASES))
    arrays = {}
    for name, p in zip(IW.ROOM_CASES, parts):
        arrays.update(p)
        rel = p[f"{name}_se"] / np.maximum(p[f"{name}_mean"], 1e-30)
        print(f"{name}: {int(p[f'{name}_spp'])} spp, relative standard error per block-channel: median {np.median(rel):.3%}, max {rel.max():.3%}")
    save(a.out, arrays)


if __name__ == "__main__":
    main()
