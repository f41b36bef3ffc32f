#!/usr/bin/env python3
"""Renders tests/golden/combined_ref.npz: the composed float64 tracer (tests/ref_combined.py) on the cases of tests/combined_worlds.CASES.
Run from the repo root:  python tests/golden/gen_combined_ref.py [--jobs N]
Takes some minutes; the output is the same bytes on every run and for every N (a chunk of ref_pathtrace.CHUNK_SPP samples is one job; the
chunks' sums are added in chunk order).  The format is gen_punctual_ref.py's: per case `c`

  c_mean, c_se        (2, 3, 3)  means of the 16 x 16 pixel blocks per channel and their standard errors
  c_cover             (32, 48)   which pixels a frame writes (all of them through a lens)
  c_seed, c_spp       scalars    the seed and the samples per pixel
  c_prefix_mean, _se  (2, 3, 3)  the same statistics of the first ref_pathtrace.CHUNK_SPP samples alone (the drift test re-renders them)

--find-spp renders no file: per case it prints the smallest multiple of CHUNK_SPP at which the fixture alone meets the sizing condition
of tests/test_combined_cpu.py (0.02 x mean beyond (Z_MAX + 1) x se in 90 % of the block-channels), the number combined_worlds.CASES holds."""
import argparse
import functools
import sys
from multiprocessing import Pool
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "golden"))
import combined_worlds as CW  # noqa: E402
import ref_combined as RC  # noqa: E402
import ref_lens as RLE  # noqa: E402
import ref_pathtrace as RP  # noqa: E402
from gen_integrator_ref import save  # noqa: E402

OUT = Path(__file__).resolve().parent / "combined_ref.npz"
Z_MAX = 4.5  # test_integrator_cpu.Z_MAX


@functools.lru_cache(maxsize=None)
def case_scene(name):
    """(RP.Scene, the keyword features of ref_combined.radiance_samples) of a case"""
    mesh, lens = CW.world(name)
    scene = RP.Scene(mesh, sky=CW.sky())
    has = CW.CASES[name][2]
    features = dict(lens=lens, lights=mesh.lights)
    if has["textures"] or has["cutout"]:
        features["surface"] = RLE.textured_surface(mesh, scene)
    if has["cutout"]:
        features["cutouts"] = RC.Cutouts(mesh, scene)
    return scene, features


def chunk(job):
    name, c = job
    flags, bounces, _, _, _, seed, _ = CW.CASES[name]
    scene, features = case_scene(name)
    return RC.chunk_sums(scene, CW.CAMERA, CW.WINDOW, flags, bounces, seed, c, **features)


def stats(sums):
    n = len(sums) * RP.CHUNK_SPP
    return RP.block_stats(*RC.mean_var(sums, n), n)


def sized(mean, se, margin=1.0, share=0.9):
    return np.mean(0.02 * mean > (Z_MAX + margin) * se) >= share


def case_arrays(name, sums):
    _, _, _, _, spp, seed, _ = CW.CASES[name]
    scene, features = case_scene(name)
    out = {}
    out[f"{name}_prefix_mean"], out[f"{name}_prefix_se"] = stats(sums[:1])
    out[f"{name}_mean"], out[f"{name}_se"] = stats(sums)
    out[f"{name}_cover"] = RC.coverage(scene, CW.CAMERA, CW.WINDOW, features["lens"], features.get("cutouts"))
    out[f"{name}_seed"], out[f"{name}_spp"] = np.array(seed, np.int64), np.array(spp, np.int64)
    return out


def find_spp(pool, names, step, limit, margin, share):
    for name in names:
        sums = []
        while len(sums) * RP.CHUNK_SPP < limit:
            sums += pool.map(chunk, [(name, c) for c in range(len(sums), len(sums) + step)])
            ok = [k for k in range(len(sums) - step + 1, len(sums) + 1) if k > 1 and sized(*stats(sums[:k]), margin, share)]
            if ok:
                print(f"{name}: sized (margin {margin}, share {share}) at {ok[0] * RP.CHUNK_SPP} samples per pixel", flush=True)
                break
        else:
            print(f"{name}: not sized at {limit} samples per pixel", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=str(OUT))
    ap.add_argument("--find-spp", action="store_true")
    ap.add_argument("--cases", nargs="*", default=list(CW.CASES))
    ap.add_argument("--limit", type=int, default=16384)
    ap.add_argument("--margin", type=float, default=1.0, help="standard errors beyond Z_MAX that --find-spp asks for")
    ap.add_argument("--share", type=float, default=0.9, help="share of the block-channels that --find-spp asks the margin of")
    a = ap.parse_args()
    with Pool(max(1, a.jobs)) as pool:
        if a.find_spp:
            find_spp(pool, a.cases, max(1, a.jobs), a.limit, a.margin, a.share)
            return
        jobs = [(name, c) for name in CW.CASES for c in range(CW.CASES[name][4] // RP.CHUNK_SPP)]
        parts = pool.map(chunk, jobs, chunksize=1)
    arrays = {}
    for name in CW.CASES:
        assert CW.CASES[name][4] % RP.CHUNK_SPP == 0
        p = case_arrays(name, [s for (n, _), s in zip(jobs, parts) if n == name])
        arrays.update(p)
        rel = p[f"{name}_se"] / np.maximum(p[f"{name}_mean"], 1e-30)
        print(f"{name}: {int(p[f'{name}_spp'])} spp, relative standard error per block-channel: median {np.median(rel):.3%}, max {rel.max():.3%}; "
              f"sized: {bool(sized(p[f'{name}_mean'], p[f'{name}_se']))}")
    save(a.out, arrays)


if __name__ == "__main__":
    main()
