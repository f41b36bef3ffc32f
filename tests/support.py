"""What the test modules share: bit views and comparisons, GConst conversion, a built PathTracer, cameras, raw pass launches, small meshes
and matrices, and a context that records launches.  Imported like `orc` and the `*_worlds` modules (conftest.py puts tests/ on sys.path)."""
import ctypes as C

import numpy as np

from raytracer3_amd import _lib as L
from raytracer3_amd import assets

F = np.float32
U = 2.0 ** -24  # unit roundoff of float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def as_orc(g):
    """the oracle's GConst with the bytes of the library's"""
    import orc

    o = orc.GConst()
    C.memmove(C.byref(o), C.byref(g), 304)
    return o


def same(got, want, what):
    diff = (bits(got) != bits(want)).reshape(got.shape[0], got.shape[1], -1).any(-1)
    assert not diff.any(), f"{what}: {int(diff.sum())} pixels differ, first at {np.argwhere(diff)[:3].tolist()}"


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): the relative error bound of n chained float32 roundings"""
    return n * U / (1 - n * U)


def rmse_fg(a, ref, fg):
    return float(np.sqrt((((a[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64))[fg]) ** 2).mean()))


def zeros(H, W):
    return np.zeros((H, W, 4), F)


# ---- the library through its Python surface
def tracer(mesh, window, *, sky=None, bluenoise=None, instances=None, mode=0, options=(), rank=0, n_ranks=1):
    """a PathTracer over `mesh`, built once, in instance mode `mode`"""
    from raytracer3_amd.renderer import PathTracer

    pt = PathTracer(window, rank=rank, n_ranks=n_ranks)
    pt.set_scene(mesh, sky, bluenoise, instances=instances, options=[(L.OPT_INSTANCE_MODE, mode), *options])
    return pt


def camera(kw, window, step=0, move=((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))):
    """the camera of a scenes.*_CAMERA dictionary, `step` times `move` = (position, direction) per step further on"""
    from raytracer3_amd.renderer import default_camera

    pos = np.asarray(kw["position"], np.float64) + step * np.asarray(move[0])
    dirn = np.asarray(kw["direction"], np.float64) + step * np.asarray(move[1])
    return default_camera(window, pos, dirn, kw["fov_deg"])


def launch(pt, name, x, y, z, g, bindings):
    return pt.ctx.pass_launch(name, x, y, z, g, bindings)


def err(pt):
    return pt.ctx.last_error()


class RecordingCtx:
    """stands in for render_graph.Context: records pass launches instead of running them"""

    def __init__(self):
        self.calls, self.n = [], 0
        self.lib, self.h = self, None

    def check(self, rc):
        assert rc == 0

    def rt3_image_create(self, h, w, hh, fmt, out):
        self.n += 1
        out._obj.value = (L.TAG_IMAGE << 30) | self.n
        return 0

    def pass_launch(self, name, x, y, z, gconst, bindings, entry="main"):
        self.calls.append((name, (x, y, z), list(bindings)))
        return 0

    def wait(self):
        pass


# ---- meshes, matrices, textures
def with_vertices(mesh, v):
    return assets.Mesh(np.ascontiguousarray(v, np.float32), mesh.indices, mesh.geometries, mesh.prim_counts, list(mesh.names), list(mesh.textures))


def soup_mesh(tri):
    """a mesh of world-space triangles (n, 3, 3)"""
    mb = assets.MeshBuilder()
    v = np.ascontiguousarray(tri, np.float32).reshape(-1, 3)
    mb.add("soup", v, np.tile([0, 0, 1], (len(v), 1)), None, np.arange(len(v), dtype=np.uint32).reshape(-1, 3), assets.Material())
    return mb.build()


def quad(mb, name, origin, du, dv, color):
    o, du, dv = (np.asarray(a, np.float64) for a in (origin, du, dv))
    pos = np.array([o, o + du, o + du + dv, o + dv])
    n = np.cross(du, dv)
    mb.add(name, pos, np.tile(n / np.linalg.norm(n), (4, 1)), np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64), [[0, 1, 2], [0, 2, 3]],
           assets.Material(color))


def translate(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def rotation(rng):
    """a uniformly random rotation matrix"""
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def constant(rgba, w=3, h=2):
    """a w x h RGBA8 texture of one colour"""
    return np.ascontiguousarray(np.tile(np.array(rgba, np.uint8), (h, w, 1)))
