"""CPU-side checks of the refit interface (rt3_scene_update_vertices, rt3_accel_refit): the header declares it,
the ctypes binding lists and types it, the library exports it, and the Python layers wrap it."""
import inspect
import re
from pathlib import Path

from raytracer3_amd import _lib as L
from raytracer3_amd.render_graph import Context
from raytracer3_amd.renderer import PathTracer

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("rt3_scene_update_vertices", "rt3_accel_refit")


def test_header_declares_refit():
    header = (ROOT / "include" / "rt3.h").read_text()
    assert re.search(r"int rt3_scene_update_vertices\(rt3_ctx \*ctx, const float \*\w+, uint32_t first, uint32_t n\);", header)
    assert re.search(r"int rt3_accel_refit\(rt3_ctx \*ctx, uint32_t \*out_handle\);", header)
    for name in NAMES:
        assert name in L.EXPORTS, name


def test_library_exports_refit():
    lib = L.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.restype is not None and len(fn.argtypes) == {"rt3_scene_update_vertices": 4, "rt3_accel_refit": 2}[name]


def test_python_wrappers():
    assert list(inspect.signature(Context.update_vertices).parameters) == ["self", "vertices", "first"]
    assert inspect.signature(Context.update_vertices).parameters["first"].default == 0
    assert list(inspect.signature(Context.refit_accel).parameters) == ["self"]
    assert list(inspect.signature(PathTracer.update_vertices).parameters) == ["self", "vertices", "first"]
