#!/usr/bin/env python3
"""Renders tests/golden/fog_ref.npz: the float64 tracer of a fogged room (tests/ref_fog.py: ref_pane_shadows' estimator with the fog rule
at its three places) on fog_worlds.fog_room() -- pane_worlds' closed room lit through the pane of its roof light by the sky, a sun, a
point lamp and one textured emitter, pane shadows on, in a box of medium that holds the room and the air above the pane -- through the
antialiased pinhole, for every case of fog_worlds.ROOM_CASES.  Run from the repo root:  python tests/golden/gen_fog_ref.py [--jobs N]
Takes a few minutes; the output is the same bytes on every run.  The arrays are named and shaped as tests/golden/glass_ref.npz names them."""
import argparse
import sys
from multiprocessing import Pool
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "golden"))
import fog_worlds as FW  # noqa: E402
import integrator_worlds as IW  # noqa: E402
import pane_worlds as PN  # noqa: E402
import ref_combined as RC  # noqa: E402
import ref_fog as RF  # noqa: E402
import ref_glass as RG  # noqa: E402
import ref_pane_shadows as RPS  # noqa: E402
import ref_pathtrace as RP  # noqa: E402
from gen_integrator_ref import save  # noqa: E402

OUT = Path(__file__).resolve().parent / "fog_ref.npz"


def chunks(name, c0, c1, medium=None):
    """(sum, sum of squares) of the chunks [c0, c1) of one case; `medium`: another medium than the room's (ref_fog's tuple)"""
    flags, bounces, _, seed, _ = FW.ROOM_CASES[name]
    mesh = FW.fog_room()
    scene = RP.Scene(mesh, sky=IW.room_sky())
    features = dict(lens=PN.ROOM_LENS, medium=medium if medium is not None else FW.room_medium()[1], glass=RG.table(mesh), panes=RPS.pane_table(mesh),
                    surface=FW.room_surface(mesh, scene), lights=list(mesh.lights))
    # (the reference takes every punctual light at every vertex: the flag belongs to the code under test)
    return [RF.room_chunk_sums(scene, PN.ROOM_CAMERA, IW.WINDOW_ROOM, flags & ~FW.F_NEE_PUNCTUAL, bounces, seed, c, **features) for c in range(c0, c1)]


def render_prefix(name, spp, medium=None):
    """block means and standard errors of the first `spp` samples of one case"""
    mean, var = RC.mean_var(chunks(name, 0, spp // RP.CHUNK_SPP, medium), spp)
    return RP.block_stats(mean, var, spp)


def render_part(job):
    return chunks(*job)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=str(OUT))
    a = ap.parse_args()
    jobs = []
    for name, case in FW.ROOM_CASES.items():
        n_chunks = case[2] // RP.CHUNK_SPP
        assert case[2] % RP.CHUNK_SPP == 0
        jobs += [(name, c, c + 1) for c in range(n_chunks)]
    with Pool(max(1, a.jobs)) as pool:
        parts = pool.map(render_part, jobs)
    arrays = {}
    W, H = IW.WINDOW_ROOM
    for name, case in FW.ROOM_CASES.items():
        spp, seed = case[2], case[3]
        sums = [s for job, part in zip(jobs, parts) if job[0] == name for s in part]
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
