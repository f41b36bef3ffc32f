"""The calls a PathTracer makes on its context, frame by frame, as a list that can be compared (tests/test_frame_trace_cpu.py).

A recording context stands in for render_graph.Context: every method PathTracer calls on it is recorded by name with its arguments
summarised (arrays as shape, dtype and crc32; structs as type and crc32), every image or buffer by the name it is first known under, and
every pass launch as (pass, entry, x, y, z, bindings), a binding written `name now @ name at creation` so that images that trade names
stay told apart.  Handle numbers are not recorded.  After every step of the script the tracer's handles are appended by name.

frame_trace.json was written once, from the commit before PathTracer's frame chain was unified, with
    python tests/golden/gen_frame_trace.py --explicit-set-scene tests/golden/frame_trace.json
(`--explicit-set-scene`: that commit's set_scene took no instances, so the step is spelt as the context calls its tests made).  The test
replays the script and compares; it does not write the file."""
import ctypes as C
import json
import sys
import types
import zlib
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from raytracer3_amd import _lib as L  # noqa: E402
from raytracer3_amd.assets import LIGHT_DTYPE  # noqa: E402
from raytracer3_amd.renderer import PathTracer  # noqa: E402

WINDOW = (48, 32)
HANDLE_BIT = 1 << 30


def crc(data):
    return zlib.crc32(bytes(data)) & 0xFFFFFFFF


class Recorder:
    """stands in for render_graph.Context (and for its `lib`, where the render graph goes to the library itself)"""

    def __init__(self):
        self.trace, self.dims, self.born, self.rg = [], {}, {}, None
        self.lib, self.h = self, None

    # ---- names for handles
    def sync(self):
        """resources created since the last event, by name (the graph names a resource after the library returned its handle)"""
        for name, handle in sorted(self.rg.named.items() if self.rg else ()):
            if handle not in self.born:
                self.born[handle] = name
                self.trace.append(["create", name, *self.dims[handle]])

    def name(self, handle):
        self.sync()
        now = sorted(n for n, h in self.rg.named.items() if h == handle)
        return f"{'|'.join(now) or '-'} @ {self.born[handle]}"

    def summary(self, a):
        if isinstance(a, (bool, str, float, type(None))):
            return a
        if isinstance(a, (int, np.integer)):
            return self.name(int(a)) if int(a) in self.dims else int(a)
        if isinstance(a, np.floating):
            return float(a)
        if isinstance(a, np.ndarray):
            return ["array", list(a.shape), str(a.dtype), crc(np.ascontiguousarray(a).tobytes())]
        if isinstance(a, C.Structure):
            return ["struct", type(a).__name__, crc(C.string_at(C.byref(a), C.sizeof(a)))]
        if isinstance(a, (list, tuple)):
            return [self.summary(x) for x in a]
        if hasattr(a, "vertices"):
            return ["mesh", self.summary(np.asarray(a.vertices)), self.summary(np.asarray(a.indices))]
        raise TypeError(type(a))

    def event(self, *what):
        self.sync()
        self.trace.append(list(what))

    # ---- the library calls of the render graph
    def check(self, rc):
        assert rc == 0

    def _new(self, out, *dims):
        out._obj.value = HANDLE_BIT | (len(self.dims) + 1)
        self.dims[out._obj.value] = dims
        return 0

    def rt3_image_create(self, h, w, hh, fmt, out):
        return self._new(out, "image", w, hh, fmt)

    def rt3_buffer_create(self, h, size, out):
        return self._new(out, "buffer", size)

    def rt3_resource_upload(self, h, handle, ptr, nbytes):
        self.event("upload", self.name(handle), nbytes, crc(C.string_at(ptr, nbytes)))
        return 0

    def rt3_resource_download(self, h, handle, ptr, nbytes):
        self.event("download", self.name(handle), nbytes)
        C.memset(ptr, 0, nbytes)
        return 0

    def rt3_pass_launch(self, h, path, entry, x, y, z, cst, size, b, nb):
        self.event("launch", path.decode(), entry.decode(), x, y, z, [self.name(b[i]) for i in range(nb)])
        return 0

    # ---- the context's methods
    def pass_launch(self, name, x, y, z, gconst, bindings, entry="main"):
        self.event("launch", name, entry, x, y, z, [self.name(b) for b in bindings])
        return 0

    def __getattr__(self, method):
        if method.startswith("_"):
            raise AttributeError(method)

        def call(*args, **kw):
            self.event(method, self.summary(args), {k: self.summary(v) for k, v in sorted(kw.items())})
            return 0

        return call


def gconst(frame, samples=2):
    g = L.GConst()
    g.proj[:] = [0.25 * (i + 1) for i in range(16)]
    g.view[:] = [0.5 * i - frame for i in range(16)]
    g.window_size[:] = WINDOW
    g.frame, g.samples, g.bounces, g.blendfactor = frame, samples, 3, 1.0
    return g


def mesh(seed, lights=0):
    rng = np.random.default_rng(seed)
    return types.SimpleNamespace(vertices=rng.random((12, 8)).astype(np.float32), indices=np.arange(12, dtype=np.uint32),
                                 lights=np.zeros(lights, LIGHT_DTYPE))


def matrix(x):
    m = np.eye(4, dtype=np.float32)
    m[0, 3] = x
    return m


def record(explicit_set_scene=False):
    """Run the script; returns the trace.  `explicit_set_scene`: spell set_scene(..., instances=, options=) as context calls."""
    trace = []

    def tracer(**kw):
        rec = Recorder()
        rec.trace = trace
        pt = PathTracer(WINDOW, ctx=rec, **kw)
        rec.rg = pt.rg
        return pt, rec

    def step(pt, rec, what, *args, **kw):
        rec.event("step", what, rec.summary(args), {k: rec.summary(v) for k, v in sorted(kw.items())})
        getattr(pt, what)(*args, **kw)
        rec.event("handles", sorted((k, rec.name(v)) for k, v in getattr(pt, "handles", {}).items()))

    sky, bn = np.full((4, 8, 3), 0.5, np.float32), np.arange(64, dtype=np.uint8).reshape(4, 4, 4)
    pt, rec = tracer()
    do = lambda what, *a, **kw: step(pt, rec, what, *a, **kw)  # noqa: E731
    do("set_scene", mesh(1), sky, bn)
    do("render", gconst(1), postprocess=True)
    do("render", gconst(2), postprocess=False)
    do("render", gconst(3), denoise=True)
    for f, dn in ((4, False), (5, False), (6, True), (7, True)):
        do("render", gconst(f), temporal=True, denoise=dn)
    do("render", gconst(8))
    do("reset_history")
    do("render", gconst(9), temporal=True)
    runs = [(0, 1, matrix(0.0)), (1, 1, matrix(1.0))]
    do("set_instances", runs)
    do("render", gconst(10), temporal=True)
    do("render", gconst(11), temporal=True, postprocess=True)
    do("set_instances", [runs[0], (1, 1, matrix(1.5))])
    do("render", gconst(12), temporal=True, denoise=True, postprocess=True)
    do("render", gconst(13), temporal=True)
    do("set_instances", [(0, 2, matrix(0.0))])
    do("render", gconst(14), temporal=True)
    do("update_vertices", mesh(2).vertices[:6], 3)
    do("update_vertices", mesh(3).vertices[:3])
    do("render", gconst(15), temporal=True)
    do("render", gconst(16), temporal=True)
    do("reset_history")
    do("update_vertices", mesh(2).vertices[:2], 1)
    do("render", gconst(40), temporal=True)
    do("update_vertices", mesh(3).vertices[:2], 1)
    do("render", gconst(41), temporal=True, denoise=True)
    do("render", gconst(17), adaptive=True)
    do("render", gconst(18), adaptive=L.AdaptiveParams(min_samples=4, step=2), postprocess=True)
    do("render", gconst(19), adaptive=False)
    do("set_lens", 0.05, 2.0, 0.5)
    do("render", gconst(20))
    do("set_lens", None)
    do("swap_light_prev")
    do("render", gconst(21))
    do("copy_light_to_prev")
    do("load_prev", np.full((WINDOW[1], WINDOW[0], 4), 0.25, np.float32))
    do("render", gconst(22), postprocess=True)
    do("light")
    do("gbuffer")
    do("set_scene", mesh(4))
    do("render", gconst(23), temporal=True)

    pt, rec = tracer()
    options = [(L.OPT_INSTANCE_MODE, 1), (L.OPT_LEAF_SIZE, 2)]
    if explicit_set_scene:
        rec.event("step", "set_scene", rec.summary((mesh(5, lights=1), sky, bn)), dict(instances=rec.summary(runs), options=rec.summary(options)))
        for opt, value in options:
            pt.ctx.set_option(opt, value)
        pt.ctx.upload_mesh(mesh(5, lights=1))
        pt.ctx.set_instances([(int(f), int(n), np.array(m, np.float32)) for f, n, m in runs])
        pt.ctx.set_sky(sky)
        pt.ctx.set_bluenoise(bn)
        pt.ctx.build_accel()
        rec.event("handles", [])
    else:
        do("set_scene", mesh(5, lights=1), sky, bn, instances=runs, options=options)
    do("render", gconst(24), temporal=True)
    do("render", gconst(25), temporal=True, denoise=True)

    pt, rec = tracer(rank=1, n_ranks=2)
    do("set_scene", mesh(6), sky)
    do("render", gconst(30))
    do("denoise", gconst(30))
    do("denoise", gconst(31), temporal=True)
    do("denoise", gconst(32), temporal=True)
    do("denoise", gconst(33), temporal=True, denoise=False)
    do("set_instances", runs)
    do("denoise", gconst(34), temporal=True)
    do("set_instances", [runs[0], (1, 1, matrix(2.0))])
    do("denoise", gconst(35), temporal=True)
    do("denoise", gconst(36), temporal=True, wait=False)
    do("render_probes", gconst(37))
    do("copy_atlas_to_prev")
    do("render_probes", gconst(38), wait=False)
    return json.loads(json.dumps(trace))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    Path(args[0]).write_text(json.dumps(record("--explicit-set-scene" in sys.argv), indent=0) + "\n")
