#!/usr/bin/env python3
"""Renders tests/golden/frost_ref.npz: the float64 tracer with rough transmission (tests/ref_frost.py) on frost_worlds.frost_room() -- the
glass room with its block at roughness 0.3 and its pane at roughness 0.2 -- for every case of frost_worlds.ROOM_CASES, and the pixel row
across the emissive edge behind the frosted thin pane of frost_worlds.edge_world().
Run from the repo root:  python tests/golden/gen_frost_ref.py [--jobs N]
Takes some minutes; the output is the same bytes on every run.

Per room case `c` the arrays of tests/golden/glass_ref.npz: c_mean, c_se (2, 3, 3), c_cover (32, 48), c_seed, c_spp; c_prefix_mean, c_prefix_se for PREFIX_CASE.
The edge: edge_mean, edge_se (64, 3): the row's per-pixel means and their standard errors; edge_spp, edge_seed."""
import argparse
import sys
from multiprocessing import Pool
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "golden"))
import frost_worlds as FW  # noqa: E402
import glass_worlds as GW  # noqa: E402
import integrator_worlds as IW  # noqa: E402
import ref_combined as RC  # noqa: E402
import ref_frost as RF  # noqa: E402
import ref_glass as RG  # noqa: E402
import ref_pathtrace as RP  # noqa: E402
from gen_integrator_ref import save  # noqa: E402

OUT = Path(__file__).resolve().parent / "frost_ref.npz"
EDGE_SPP, EDGE_SEED, EDGE_BOUNCES = 1024, 383, 3
Z_MAX = 4.5  # test_integrator_cpu's
PREFIX_CASE = "frost_b4"  # the case whose first chunk the drift test renders again


def room_scene(name):
    flags, bounces, specular, tau = FW.ROOM_CASES[name][:4]
    mesh = FW.frost_room(specular, tau)
    return RP.Scene(mesh, sky=IW.room_sky()), dict(lens=FW.ROOM_LENS, glass=RG.table(mesh), frost=RF.frosted(mesh))


def render_prefix(name, spp):
    """block means and standard errors of the first `spp` samples of one case"""
    flags, bounces, _, _, _, seed = FW.ROOM_CASES[name][:6]
    scene, features = room_scene(name)
    mean, var = RF.render(scene, IW.ROOM_CAMERA, IW.WINDOW_ROOM, flags, bounces, spp, seed, **features)
    return RP.block_stats(mean, var, spp)


def edge_chunk(chunk):
    mesh = FW.edge_world(FW.EDGE_ALPHA)
    scene = RP.Scene(mesh)
    s1, s2 = RF.chunk_sums(scene, GW.CAMERA, FW.EDGE_WINDOW, 0, EDGE_BOUNCES, EDGE_SEED, chunk, lens=GW.PINHOLE, glass=RG.table(mesh), frost=RF.frosted(mesh))
    return s1[FW.EDGE_ROW], s2[FW.EDGE_ROW]


def edge_row(sums, spp):
    mean, var = RC.mean_var(sums, spp)
    return mean, np.sqrt(var / spp)


def render_part(job):
    name, c0, c1 = job
    if name == "edge":
        return [edge_chunk(c) for c in range(c0, c1)]
    flags, bounces, _, _, _, seed = FW.ROOM_CASES[name][:6]
    scene, features = room_scene(name)
    return [RF.chunk_sums(scene, IW.ROOM_CAMERA, IW.WINDOW_ROOM, flags, bounces, seed, c, **features) for c in range(c0, c1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=str(OUT))
    a = ap.parse_args()
    jobs = []
    for name, spp in [(n, c[4]) for n, c in FW.ROOM_CASES.items()] + [("edge", EDGE_SPP)]:
        assert spp % RP.CHUNK_SPP == 0
        n_chunks = spp // RP.CHUNK_SPP
        jobs += [(name, c, min(c + 4, n_chunks)) for c in range(0, n_chunks, 4)]
    with Pool(max(1, a.jobs)) as pool:
        parts = pool.map(render_part, jobs)
    arrays = {}
    W, H = IW.WINDOW_ROOM
    for name, case in FW.ROOM_CASES.items():
        spp, seed = case[4], case[5]
        sums = [s for job, part in zip(jobs, parts) if job[0] == name for s in part]
        for tag, n in (("prefix_", RP.CHUNK_SPP), ("", spp)) if name == PREFIX_CASE else (("", spp),):
            mean, var = RC.mean_var(sums[: n // RP.CHUNK_SPP], n)
            arrays[f"{name}_{tag}mean"], arrays[f"{name}_{tag}se"] = RP.block_stats(mean, var, n)
        arrays[f"{name}_cover"] = np.ones((H, W), bool)
        arrays[f"{name}_seed"], arrays[f"{name}_spp"] = np.array(seed, np.int64), np.array(spp, np.int64)
        rel = arrays[f"{name}_se"] / np.maximum(arrays[f"{name}_mean"], 1e-30)
        sized = float(np.mean(0.02 * arrays[f"{name}_mean"] > (Z_MAX + 1.0) * arrays[f"{name}_se"]))
        print(f"{name}: {spp} spp, relative standard error per block-channel: median {np.median(rel):.3%}, max {rel.max():.3%}; resolves 2 % in {sized:.0%}")
        assert sized >= 0.9, "the fixture must resolve 2 % in 90 % of its block-channels"
    sums = [s for job, part in zip(jobs, parts) if job[0] == "edge" for s in part]
    arrays["edge_mean"], arrays["edge_se"] = edge_row(sums, EDGE_SPP)
    arrays["edge_seed"], arrays["edge_spp"] = np.array(EDGE_SEED, np.int64), np.array(EDGE_SPP, np.int64)
    save(a.out, arrays)


if __name__ == "__main__":
    main()
