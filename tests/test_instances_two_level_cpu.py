"""Instance mode 1 without a GPU: the option and rt3_accel_levels are declared by the C header, bound by _lib.py and exported by a built
librt3.so (the GPU behaviour is in test_instances_two_level.py)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from raytracer3_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "rt3.h").read_text()


def test_header_declares_instance_mode_and_levels():
    assert re.search(r"#define RT3_OPT_INSTANCE_MODE 14\b", HEADER)
    assert re.search(r"int rt3_accel_levels\(rt3_ctx \*ctx, uint32_t \*n_meshes, uint32_t \*n_meshes_built, uint32_t \*n_top_nodes, uint64_t \*accel_bytes\);", HEADER)


def test_python_binding_exposes_them():
    assert L.OPT_INSTANCE_MODE == 14
    assert "rt3_accel_levels" in L.EXPORTS  # __graft_entry__.build() checks every listed symbol
    from raytracer3_amd.render_graph import Context

    assert callable(getattr(Context, "accel_levels", None))


def test_built_library_exports_accel_levels():
    so = L.LIB_PATH
    if not so.exists():
        pytest.skip("librt3.so is not built")
    try:
        lib = C.CDLL(str(so))
    except OSError as e:  # the HIP runtime it links against is not loadable here
        pytest.skip(f"cannot load librt3.so: {e}")
    assert hasattr(lib, "rt3_accel_levels")
