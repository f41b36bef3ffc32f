#!/usr/bin/env python3
"""Renders tests/golden/volume_ref.npz: the float64 tracer with absorbing glass (tests/ref_volume.py) on volume_worlds.absorbing_room() -- the
glass room of glass_worlds with an absorbing block and an absorbing sphere -- through the antialiased pinhole volume_worlds.ROOM_LENS, for
every case of volume_worlds.ROOM_CASES.  Run from the repo root:  python tests/golden/gen_volume_ref.py [--jobs N]
Takes some minutes; the output is the same bytes on every run.

Per case `c` the file holds only arrays, named and shaped as tests/golden/glass_ref.npz names them:
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
import ref_glass as RG  # noqa: E402
import ref_pathtrace as RP  # noqa: E402
import ref_volume as RV  # noqa: E402
import volume_worlds as VW  # noqa: E402
from gen_integrator_ref import save  # noqa: E402

OUT = Path(__file__).resolve().parent / "volume_ref.npz"


def _scene(name):
    flags, bounces, specular, tau, _, seed, _ = VW.ROOM_CASES[name]
    mesh = VW.absorbing_room(specular, tau)
    features = dict(lens=VW.ROOM_LENS, glass=RG.table(mesh), sigma=VW.sigma_table(mesh))
    return RP.Scene(mesh, sky=IW.room_sky()), flags, bounces, seed, features


def render_prefix(name, spp):
    """block means and standard errors of the first `spp` samples of one case"""
    scene, flags, bounces, seed, features = _scene(name)
    mean, var = RV.render(scene, IW.ROOM_CAMERA, IW.WINDOW_ROOM, flags, bounces, spp, seed, **features)
    return RP.block_stats(mean, var, spp)


def render_part(job):
    """(sum, sum of squares) of the chunks [c0, c1) of one case: the unit of work of the pool"""
    name, c0, c1 = job
    scene, flags, bounces, seed, features = _scene(name)
    return [RV.chunk_sums(scene, IW.ROOM_CAMERA, IW.WINDOW_ROOM, flags, bounces, seed, c, **features) for c in range(c0, c1)]


def main():
    import ref_combined as RC

    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=str(OUT))
    a = ap.parse_args()
    jobs = []
    for name, case in VW.ROOM_CASES.items():
        n_chunks = case[4] // RP.CHUNK_SPP
        assert case[4] % RP.CHUNK_SPP == 0
        step = 6
        jobs += [(name, c, min(c + step, n_chunks)) for c in range(0, n_chunks, step)]
    with Pool(max(1, a.jobs)) as pool:
        parts = pool.map(render_part, jobs)
    arrays = {}
    W, H = IW.WINDOW_ROOM
    for name, case in VW.ROOM_CASES.items():
        spp, seed = case[4], case[5]
        sums = [s for job, part in zip(jobs, parts) if job[0] == name for s in part]  # in chunk order, as ref_volume.render adds them
        for tag, n in (("prefix_", RP.CHUNK_SPP), ("", spp)):
            mean, var = RC.mean_var(sums[: n // RP.CHUNK_SPP], n)
            arrays[f"{name}_{tag}mean"], arrays[f"{name}_{tag}se"] = RP.block_stats(mean, var, n)
        arrays[f"{name}_cover"] = np.ones((H, W), bool)
        arrays[f"{name}_seed"], arrays[f"{name}_spp"] = np.array(seed, np.int64), np.array(spp, np.int64)
        rel = arrays[f"{name}_se"] / np.maximum(arrays[f"{name}_mean"], 1e-30)
        print(f"{name}: {spp} spp, relative standard error per block-channel: median {np.median(rel):.3%}, max {rel.max():.3%}")
    save(a.out, arrays)


if __name__ == "__main__":
    main()
