#!/usr/bin/env python3
"""Renders tests/golden/pane_shadows_ref.npz: the float64 tracer with pane shadows (tests/ref_pane_shadows.py, the mode on) on
pane_worlds.window_room() -- a closed room lit only through the pane of its roof light -- through the antialiased pinhole, for every case
of pane_worlds.WINDOW_CASES.  Run from the repo root:  python tests/golden/gen_pane_shadows_ref.py [--jobs N]
Takes some minutes; the output is the same bytes on every run.  The arrays are named and shaped as tests/golden/glass_ref.npz names them."""
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
import pane_worlds as PN  # noqa: E402
import ref_glass as RG  # noqa: E402
import ref_pane_shadows as RPS  # noqa: E402
import ref_pathtrace as RP  # noqa: E402
from gen_integrator_ref import save  # noqa: E402

OUT = Path(__file__).resolve().parent / "pane_shadows_ref.npz"


def chunks(name, c0, c1, **kw):
    """(sum, sum of squares) of the chunks [c0, c1) of one case"""
    mesh, flags, lights = PN.window_case(name)
    scene = RP.Scene(mesh, sky=IW.room_sky())
    case = PN.WINDOW_CASES[name]
    return [RPS.chunk_sums(scene, PN.ROOM_CAMERA, IW.WINDOW_ROOM, flags, case[1], case[7], c, lens=PN.ROOM_LENS, glass=RG.table(mesh), pane_shadows=True,
                           panes=RPS.pane_table(mesh), lights=lights, **kw) for c in range(c0, c1)]


def render_prefix(name, spp):
    """block means and standard errors of the first `spp` samples of one case"""
    import ref_combined as RC

    mean, var = RC.mean_var(chunks(name, 0, spp // RP.CHUNK_SPP), spp)
    return RP.block_stats(mean, var, spp)


def render_part(job):
    return chunks(*job)


def main():
    import ref_combined as RC

    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=str(OUT))
    a = ap.parse_args()
    jobs = []
    for name, case in PN.WINDOW_CASES.items():
        n_chunks = case[6] // RP.CHUNK_SPP
        assert case[6] % RP.CHUNK_SPP == 0
        jobs += [(name, c, min(c + 4, n_chunks)) for c in range(0, n_chunks, 4)]
    with Pool(max(1, a.jobs)) as pool:
        parts = pool.map(render_part, jobs)
    arrays = {}
    W, H = IW.WINDOW_ROOM
    for name, case in PN.WINDOW_CASES.items():
        spp, seed = case[6], case[7]
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
