"""What rt3_pass_launch accepts and refuses, pass by pass, from one table of the ten passes: the launch shape, the binding count, every
binding's kind, size and format, the images that may not alias (and the ones that may), the context-state inputs of "denoise" and
"temporal", the tile partition and the unknown name.  Every refused launch is refused on the host, before anything is enqueued.

Cornell at 64 x 48: the probe grid (4 x 3) is more than one probe each way, the group dispatch (8 x 6) differs from the window, and the
probe atlas (32 x 24) differs from both."""
import math

import pytest

from raytracer3_amd import _lib as L
from raytracer3_amd import scenes

pytestmark = pytest.mark.gpu

W, H = 64, 48
X, Y = math.ceil(W / 8), math.ceil(H / 8)  # groups of a full-screen dispatch
PX, PY = W // 16, H // 16                  # probes
RAY_TRACING = ("gbuffer", "refrence_mode", "trace_probes", "motion")  # these ignore z

# name, the good (x, y, z), the good bindings as keys of World.h, the binding names as the errors quote them
PASSES = [
    ("gbuffer", (W, H, 1), ["gbuffer", "depth"], ["gbuffer", "gbuffer_depth"]),
    ("refrence_mode", (W, H, 1), ["gbuffer", "depth", "light", "prev"], ["gbuffer", "gbuffer_depth", "Light", "PrevLight"]),
    ("postprocess", (X, Y, 1), ["depth", "color", "light"], ["Depth", "Out", "In"]),
    ("structured_importance_sampling", (PX, PY, 1), ["gbuffer", "depth", "directions", "debug", "atlas"],
     ["gbuffer", "gbuffer_depth", "out", "debug", "probe_atlas"]),
    ("trace_probes", (8 * PX, 8 * PY, 1), ["gbuffer", "depth", "directions", "atlas", "prev_atlas"],
     ["gbuffer", "gbuffer_depth", "directions", "probe_atlas", "prev_probe_atlas"]),
    ("spherical_harmonic_conversion", (PX, PY, 1), ["sh", "atlas"], ["out", "probe_atlas"]),
    ("interpolate_probes", (X, Y, 1), ["gbuffer", "depth", "sh", "light"], ["gbuffer", "gbuffer_depth", "sh_coeficents", "Light"]),
    ("denoise", (X, Y, 1), ["gbuffer", "depth", "light", "denoised"], ["gbuffer", "gbuffer_depth", "In", "Out"]),
    ("temporal", (X, Y, 1),
     ["gbuffer", "depth", "light", "prev_gbuffer", "prev_depth", "prev_history", "prev_moments", "accumulated", "history", "moments"],
     ["gbuffer", "gbuffer_depth", "In", "PrevGbuffer", "PrevDepth", "PrevHistory", "PrevMoments", "Out", "History", "Moments"]),
    ("motion", (W, H, 1), ["motion"], ["Motion"]),
]
NAMES = [p[0] for p in PASSES]
BUFFER_SLOTS = {("spherical_harmonic_conversion", 0), ("interpolate_probes", 2)}
# (pass, position, the earlier position whose image is put there): launches refused with "different images" ...
ALIAS_REFUSED = ([("denoise", 3, 2), ("trace_probes", 4, 3), ("trace_probes", 3, 4)] +
                 [("temporal", i, j) for i in (7, 8, 9) for j in (2, 5, 6, 7, 8) if j < i])  # every earlier binding of the same format
# ... and the ones that are not refused
ALIAS_ACCEPTED = [("refrence_mode", 3, 2), ("postprocess", 1, 2)]


class World:
    def __init__(self):
        from raytracer3_amd.render_graph import ImageSize
        from raytracer3_amd.renderer import Camera, PathTracer, frame_nodes, motion_node, temporal_images

        cam = scenes.CORNELL_CAMERA
        self.pt = pt = PathTracer((W, H))
        pt.set_scene(scenes.cornell())
        self.g = g = pt.make_gconst(Camera(cam["position"], cam["direction"], math.radians(cam["fov_deg"]), W / H), 1, 2, frame=1,
                                    flags=L.F_FACEFORWARD)
        rg = pt.rg
        h = dict(pt.probe_commands(g))
        rg.begin_frame()
        h.update(frame_nodes(rg, g))
        h.update(temporal_images(rg))
        h["motion"] = motion_node(rg, g)[1]
        h["denoised"] = rg.image(ImageSize.FullScreen, L.FORMAT_R32G32B32A32_SFLOAT, "denoised")
        self.tiny = rg.image(ImageSize.XY(1, 1), L.FORMAT_R16_UINT, "tiny")  # the wrong size everywhere, the wrong format nearly everywhere
        self.buf48 = rg.buffer(48, "buf48")                                   # no image, and too short for the probe grid's coefficients
        self.h = h
        pt.render(g)  # a plain frame: the G-buffer, its depth and Light hold data
        pt.ctx.set_prev_view(g)

    def launch(self, name, xyz, bindings, ctx=None):
        ctx = ctx or self.pt.ctx
        return ctx.pass_launch(name, *xyz, self.g, bindings)

    def err(self, ctx=None):
        return (ctx or self.pt.ctx).last_error()

    def good(self, name):
        _, xyz, keys, _ = PASSES[NAMES.index(name)]
        return xyz, [self.h[k] for k in keys]


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.pt.close()


def swapped(bindings, i, handle):
    b = list(bindings)
    b[i] = handle
    return b


@pytest.mark.parametrize("name,xyz,keys,shown", PASSES, ids=NAMES)
def test_pass_contract(world, name, xyz, keys, shown):
    w, E = world, L.E_INVALID
    good = [w.h[k] for k in keys]
    x, y, z = xyz
    assert w.launch(name, xyz, good) == 0, w.err()
    assert w.pt.ctx.lib.rt3_frame_wait(w.pt.ctx.h) == 0
    # binding count
    count = f"{len(good)} binding" + ("s" if len(good) != 1 else "")
    assert w.launch(name, xyz, good[:-1]) == E and count in w.err() and name in w.err(), w.err()
    assert w.launch(name, xyz, good + [w.tiny]) == E and count in w.err() and name in w.err(), w.err()
    # launch shape
    assert w.launch(name, (x + 1, y, z), good) == E, w.err()
    if name in ("gbuffer", "refrence_mode", "motion"):
        assert "launch size" in w.err()
    if xyz == (X, Y, 1):
        assert "ceil(W/8)" in w.err()
    assert w.launch(name, (x, y, 2), good) == (0 if name in RAY_TRACING else E), w.err()
    # every binding: another size (and format), another kind, nothing
    for i, n in enumerate(shown):
        assert w.launch(name, xyz, swapped(good, i, w.tiny)) == E and f"'{n}'" in w.err(), (n, w.err())
        assert w.launch(name, xyz, swapped(good, i, w.buf48)) == E, n
        if (name, i) in BUFFER_SLOTS:
            assert "at least" in w.err(), (n, w.err())
        assert w.launch(name, xyz, swapped(good, i, 0)) == E, n
    # aliasing: what is refused, and what is not
    for p, i, j in ALIAS_REFUSED:
        if p == name:
            assert w.launch(name, xyz, swapped(good, i, good[j])) == E and "different images" in w.err(), (i, j, w.err())
    for p, i, j in ALIAS_ACCEPTED:
        if p == name:
            assert w.launch(name, xyz, swapped(good, i, good[j])) == 0, (i, j, w.err())
    assert w.launch(name, xyz, good) == 0, w.err()  # the refused launches left the context usable
    assert w.pt.ctx.lib.rt3_frame_wait(w.pt.ctx.h) == 0


def test_side_channel_inputs(world):
    """the variance input of "denoise" and the motion input of "temporal" are checked like bindings, and may not be an image the pass writes"""
    w, E, ctx = world, L.E_INVALID, world.pt.ctx
    xyz, good = w.good("denoise")
    try:
        for bad in (good[3], w.tiny):
            ctx.set_denoise_variance_input(bad)
            assert w.launch("denoise", xyz, good) == E, bad
        ctx.set_denoise_variance_input(w.h["moments"])
        assert w.launch("denoise", xyz, good) == 0, w.err()
    finally:
        ctx.set_denoise_variance_input(0)
    xyz, good = w.good("temporal")
    try:
        for bad in (good[7], good[8], good[9], w.tiny):
            ctx.set_temporal_motion_input(bad)
            assert w.launch("temporal", xyz, good) == E, bad
        ctx.set_temporal_motion_input(w.h["motion"])
        assert w.launch("temporal", xyz, good) == 0, w.err()
    finally:
        ctx.set_temporal_motion_input(0)
    ctx.wait()


def test_tile_partition(world):
    """only "denoise" and "temporal" need the whole window on one rank"""
    w, ctx = world, world.pt.ctx
    ctx.set_tile_partition(W, H, 0, 2)
    try:
        for name in ("denoise", "temporal"):
            assert w.launch(name, *w.good(name)) == L.E_STATE and "other ranks own" in w.err(), (name, w.err())
        assert w.launch("gbuffer", *w.good("gbuffer")) == 0, w.err()
    finally:
        ctx.set_tile_partition(W, H, 0, 1)
    ctx.wait()


def test_unknown_pass(world):
    from raytracer3_amd.render_graph import Context

    w = world
    xyz, good = w.good("gbuffer")
    assert w.launch("nonesuch", xyz, good) == L.E_INVALID
    assert "unknown pass" in w.err()
    listed = w.err().split("unknown pass", 1)[1]
    for name in NAMES:
        assert name in listed, (name, w.err())
    fresh = Context()  # no acceleration structure: the state is refused before the name is looked at
    assert w.launch("nonesuch", xyz, good, fresh) == L.E_STATE, w.err(fresh)
    fresh.close()
