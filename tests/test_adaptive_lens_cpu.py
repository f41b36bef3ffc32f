"""Coverage mode of the "adaptive" pass without a GPU (rt3_adaptive_set_coverage): the surface of the feature -- the
header, the library's exports, the binding, the host layers, the tools -- and the reference semantics the GPU tests rely on:
tests/ref_adaptive.py with every pixel foreground lists every pixel and leaves no count at 0."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

import adaptive_lens_worlds as alw
import ref_adaptive as ra
from raytracer3_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("rt3_adaptive_set_coverage", "rt3_adaptive_get_coverage")


def test_header_declares_and_library_exports():
    header = (ROOT / "include" / "rt3.h").read_text()
    assert re.search(r"int rt3_adaptive_set_coverage\(rt3_ctx \*ctx, int on\);", header)
    assert re.search(r"int rt3_adaptive_get_coverage\(rt3_ctx \*ctx, int \*on\);", header)
    lib = L.load()
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(lib, name)


def test_null_arguments_are_refused():
    lib = L.load()
    on = C.c_int(7)
    assert lib.rt3_adaptive_set_coverage(None, 1) == L.E_INVALID  # no context: refused, nothing touched
    assert lib.rt3_adaptive_get_coverage(None, C.byref(on)) == L.E_INVALID and on.value == 7
    assert lib.rt3_adaptive_get_coverage(None, None) == L.E_INVALID


def test_signature_table_names_both():
    lib = L.load()
    i32 = C.c_int
    assert lib.rt3_adaptive_set_coverage.restype is i32 and list(lib.rt3_adaptive_set_coverage.argtypes) == [C.c_void_p, i32]
    assert lib.rt3_adaptive_get_coverage.restype is i32 and list(lib.rt3_adaptive_get_coverage.argtypes) == [C.c_void_p, C.POINTER(i32)]


def test_host_layers_and_tools():
    from raytracer3_amd.render_graph import Context
    from raytracer3_amd.renderer import PathTracer

    assert callable(Context.adaptive_set_coverage) and callable(Context.adaptive_coverage)
    assert callable(PathTracer.set_adaptive_coverage)
    hpp = (ROOT / "raytracer3_amd" / "host" / "render_graph.hpp").read_text()
    assert all(name in hpp for name in NAMES)
    assert "set_adaptive_coverage" in (ROOT / "tools" / "render.py").read_text()
    assert (ROOT / "tools" / "time_adaptive_lens.py").exists()


def test_reference_with_every_pixel_foreground_lists_every_pixel():
    """what the GPU tests take from ref_adaptive: with fg all true round 0 lists the whole window (paths = min_samples x W x H after one
    round), no count stays 0, and a constant pixel stops at min_samples whatever its neighbours do without dilation"""
    W, H = alw.A["window"]
    rng = np.random.default_rng(5)
    # uniform noise around 0.5 whose amplitude grows with the column: the relative standard error of n samples is 0.58 a / sqrt(n), so
    # under threshold 0.1 the columns with a < 0.35 stop after four samples and those with a > 0.85 are still going after twenty
    y = (0.5 + np.linspace(0.0, 1.2, W) * (rng.random((alw.CAP, H, W)) - 0.5)).astype(np.float32)
    y[:, : H // 3] = 0.25  # constant samples: a background that is all sky
    fg = np.ones((H, W), bool)
    kw = dict(min_samples=alw.MIN_SAMPLES, step=alw.STEP, dark=alw.DARK)
    n, S1, S2, rounds, paths, capped = ra.simulate(y, fg, alw.CAP, threshold=0.1, dilate=0, **kw)
    assert (n >= alw.MIN_SAMPLES).all() and (n[: H // 3] == alw.MIN_SAMPLES).all() and paths == n.sum()
    assert 0 < capped < W * H and len(np.unique(n)) > 2
    # round 0 alone: every pixel, once
    n0, _, _, rounds0, paths0, capped0 = ra.simulate(y, fg, alw.MIN_SAMPLES, threshold=0.1, dilate=0, **kw)
    assert (n0 == alw.MIN_SAMPLES).all() and (rounds0, paths0, capped0) == (1, alw.MIN_SAMPLES * W * H, W * H)
    # threshold 0 on samples that differ: everyone reaches the cap
    n1, _, _, rounds1, paths1, capped1 = ra.simulate(rng.random((alw.CAP, H, W)).astype(np.float32), fg, alw.CAP, threshold=0.0, dilate=0, **kw)
    assert (n1 == alw.CAP).all() and (rounds1, paths1, capped1) == (alw.CAP // alw.STEP, alw.CAP * W * H, W * H)
    # the first decision is next_active's over the whole window
    stay, cnt = ra.next_active(S1 * 0, S2 * 0, np.full((H, W), alw.MIN_SAMPLES), fg, fg, 0.5, alw.DARK, 1)
    assert cnt["active"] == W * H and not stay.any()  # (S1 = S2 = 0: variance 0 passes)


def test_worlds_are_the_issues():
    assert alw.A["window"] == (67, 45) and alw.B["window"] == (64, 48) and alw.B["bounces"] == 4
    assert (alw.MIN_SAMPLES, alw.STEP, alw.CAP) == (4, 4, 24) and alw.CAPS == [4, 8, 12, 16, 20, 24]
    assert 67 * 45 > 2048 > 67 * 45 - 2048  # the list crosses exactly one boundary of the compaction's 2048-entry blocks
    for world in (alw.A, alw.B):
        for dilate in (0, 1):
            p = alw.params(world, dilate=dilate)
            assert p["threshold"] == world["threshold"][dilate] > 0 and p["min_samples"] == p["step"] == 4
            L.AdaptiveParams(**p)
