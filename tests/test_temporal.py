"""The "temporal" pass on the MI355X: bit-for-bit parity of Out, History and Moments with tests/ref_temporal.py (the
numpy float32 restatement that tests/test_temporal_cpu.py pins) over sequences of frames fed back into each other, the chain
temporal -> denoise with the variance input, the documented errors, determinism, the multi-rank root path and the C++ example.  The input
frames come from the GPU passes themselves, which test_gpu_parity.py pins to the oracle."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

import orc
import ref_denoise as rd
import ref_temporal as rt
from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from support import as_orc, bits, camera, launch, same, tracer

pytestmark = pytest.mark.gpu
BG = np.float32(orc.BACKGROUND_DEPTH)
F = np.float32


CORNELL_MOVE = ((0.01, 0.0, 0.0), (0.0105, 0.0, 0.0))
ATRIUM_MOVE = ((0.02, 0.0, 0.01), (0.0, 0.0, 0.012))


def check_sequence(pt, gconsts, what, denoise=False, **params):
    """render the frames through gbuffer -> refrence_mode -> temporal (-> denoise); after every frame Out, History and Moments must equal
    the reference pass applied to the frame's own Light and the previous frame's (GPU) History and Moments.  Returns the last frame."""
    pt.ctx.set_temporal_params(**params) if params else pt.ctx.set_temporal_params()
    pt.reset_history()
    W, H = pt.window
    prev = None
    for k, g in enumerate(gconsts):
        pt.render(g, temporal=True, denoise=denoise)
        light, out = pt.light(), pt.accumulated()
        hist, mom = pt.history()
        gb, depth = pt.gbuffer()
        if prev is None:
            prev = (as_orc(g), gb, depth, np.zeros((H, W, 4), F), np.zeros((H, W, 4), F))
        want = rt.temporal(as_orc(g), gb, depth, light, *prev, **dict(rt.DEFAULTS, **params))
        fg = depth != BG
        N = hist[..., 3]
        print(f"{what} frame {k}: {W}x{H}, {int(fg.sum())} foreground pixels, N > 1 on {int((N > 1).sum())}, N max {N.max():.2f}")
        for got, ref, name in zip((out, hist, mom), want, ("Out", "History", "Moments")):
            same(got, ref, f"{what} frame {k} {name}")
        if denoise:
            same(pt.denoised(), rt.denoise(as_orc(g), gb, depth, out, moments=mom), f"{what} frame {k} denoised")
        prev = (as_orc(g), gb, depth, hist, mom)
    return dict(light=light, out=out, hist=hist, mom=mom, gb=gb, depth=depth)


def test_parity_cornell_static_moving_and_parameters():
    W = H = 128
    pt = tracer(scenes.cornell(), (W, H))

    def seq(steps, first_frame=1):
        return [pt.make_gconst(camera(scenes.CORNELL_CAMERA, (W, H), s, CORNELL_MOVE), 1, 4, frame=first_frame + k, flags=L.F_FACEFORWARD)
                for k, s in enumerate(steps)]

    r = check_sequence(pt, seq([0, 0, 0, 0]), "cornell static")
    fg = r["depth"] != BG
    assert (r["hist"][..., 3][fg] == 4).mean() > 0.95  # it did accumulate
    r = check_sequence(pt, seq([0, 1, 2, 3]), "cornell moving")
    assert (r["hist"][..., 3][fg] > 2).mean() > 0.5 and not np.array_equal(bits(r["out"])[fg], bits(r["light"])[fg])
    check_sequence(pt, seq([0, 1, 2], 5), "cornell, running mean", alpha=0.0, alpha_moments=0.0, max_history=2)
    check_sequence(pt, seq([0, 2, 4], 9), "cornell, other parameters", alpha=0.5, alpha_moments=0.1, max_history=7, normal_cos=0.5, plane_tolerance=0.1)
    check_sequence(pt, seq([0, 1, 2], 3), "cornell, strict tests", normal_cos=1.0, plane_tolerance=1e-4)
    check_sequence(pt, seq([0, 1, 2], 3), "cornell, demodulation off", flags=L.TEMPORAL_NO_DEMODULATION)
    pt.close()


def test_parity_atrium_sky_columns_and_odd_window():
    from raytracer3_amd.renderer import DEFAULT_FLAGS

    sky, bn = scenes.sky(512, 256), assets.load_bluenoise()
    for W, H in ((192, 108), (250, 187)):  # 250 x 187: no multiple of 8 nor of the kernel's tile
        pt = tracer(scenes.atrium(0.25), (W, H), sky=sky, bluenoise=bn)
        gs = [pt.make_gconst(camera(scenes.ATRIUM_CAMERA, (W, H), s, ATRIUM_MOVE), 1, 4, frame=5 + s, flags=DEFAULT_FLAGS) for s in range(4)]
        r = check_sequence(pt, gs, "atrium moving")
        fg = r["depth"] != BG
        assert (~fg).any() and np.array_equal(bits(r["out"])[~fg], bits(r["light"])[~fg])  # sky pixels pass through
        assert not r["hist"][~fg].any() and not r["mom"][~fg].any()
        assert np.array_equal(bits(r["out"][..., 3]), bits(r["light"][..., 3]))
        # through the tone map: postprocess reads the accumulated image
        pt.render(pt.make_gconst(camera(scenes.ATRIUM_CAMERA, (W, H), 4, ATRIUM_MOVE), 1, 4, frame=9, flags=DEFAULT_FLAGS), postprocess=True, temporal=True)
        g = pt.make_gconst(camera(scenes.ATRIUM_CAMERA, (W, H), 4, ATRIUM_MOVE), 1, 4, frame=9, flags=DEFAULT_FLAGS)
        want = orc.Scene(scenes.atrium(0.25), sky, bn).postprocess(as_orc(g), pt.gbuffer()[1], pt.accumulated())
        assert np.allclose(pt.color(), want, atol=2e-5, rtol=1e-4)
        pt.close()


def test_windows_around_the_tile_size():
    from raytracer3_amd.renderer import DEFAULT_FLAGS

    sky, bn = scenes.sky(128, 64), assets.load_bluenoise()
    for W, H in ((97, 41), (20, 6), (3, 9)):
        pt = tracer(scenes.atrium(0.25), (W, H), sky=sky, bluenoise=bn)
        gs = [pt.make_gconst(camera(scenes.ATRIUM_CAMERA, (W, H), s, ATRIUM_MOVE), 1, 3, frame=8 + s, flags=DEFAULT_FLAGS) for s in (0, 1, 3)]
        check_sequence(pt, gs, "odd window")
        check_sequence(pt, gs[:1] * 3, "odd window, static")
        pt.close()


def test_parity_textured_cornell():
    W, H = 160, 120
    pt = tracer(scenes.textured_cornell(), (W, H))
    gs = [pt.make_gconst(camera(scenes.CORNELL_CAMERA, (W, H), s, CORNELL_MOVE), 2, 3, frame=2 + s, flags=L.F_FACEFORWARD | L.F_SPECULAR) for s in range(3)]
    check_sequence(pt, gs, "textured cornell")
    pt.close()


def test_camera_turned_away():
    """the second view looks back past the first: for part of the frame the reprojection leaves the previous window or lies behind the
    previous camera (q.w <= 0); those pixels start over, the rest keep their history"""
    from raytracer3_amd.renderer import DEFAULT_FLAGS, Camera

    W, H = 192, 108
    sky, bn = scenes.sky(128, 64), assets.load_bluenoise()
    pt = tracer(scenes.atrium(0.25), (W, H), sky=sky, bluenoise=bn)
    kw = scenes.ATRIUM_CAMERA
    for what, dirs in (("turned 50 degrees", ((1.0, 0.1, 0.0), (0.64, 0.1, 0.77))), ("turned round", ((1.0, 0.1, 0.0), (-1.0, 0.1, 0.3), (1.0, 0.1, 0.0)))):
        gs = [pt.make_gconst(Camera(kw["position"], d, math.radians(kw["fov_deg"]), W / H), 1, 3, frame=4 + k, flags=DEFAULT_FLAGS) for k, d in enumerate(dirs)]
        r = check_sequence(pt, gs, what)
        fg = r["depth"] != BG
        valid, _, _ = rt.reproject(as_orc(gs[-1]), as_orc(gs[-2]), rt.positions(as_orc(gs[-1]), r["depth"]))
        print(f"{what}: reprojection valid on {int((valid & fg).sum())} of {int(fg.sum())} foreground pixels")
        assert (fg & ~valid).sum() > 0.3 * fg.sum() and np.all(r["hist"][..., 3][fg & ~valid] == 1)
        if what == "turned 50 degrees":
            assert (r["hist"][..., 3][fg & valid] == 2).any()
    pt.close()


def test_temporal_then_denoise_with_the_variance_input():
    from raytracer3_amd.renderer import DEFAULT_FLAGS

    W, H = 192, 108
    sky, bn = scenes.sky(512, 256), assets.load_bluenoise()
    pt = tracer(scenes.atrium(0.25), (W, H), sky=sky, bluenoise=bn)
    gs = [pt.make_gconst(camera(scenes.ATRIUM_CAMERA, (W, H), s, ATRIUM_MOVE), 1, 4, frame=1 + s, flags=DEFAULT_FLAGS) for s in range(6)]
    r = check_sequence(pt, gs, "atrium temporal + denoise", denoise=True)
    fg = r["depth"] != BG
    old = fg & (r["mom"][..., 3] >= 4)
    assert old.any() and (fg & ~old).any()
    den = pt.denoised()
    # the variance input is what changed the result, and without it the pass is the one it was
    plain = rd.denoise(as_orc(gs[-1]), r["gb"], r["depth"], r["out"])
    assert not np.array_equal(bits(den), bits(plain))
    h = pt.handles
    pt.ctx.set_denoise_variance_input(0)
    pt.ctx.check(launch(pt, "denoise", math.ceil(W / 8), math.ceil(H / 8), 1, gs[-1], [h["gbuffer"], h["depth"], h["accumulated"], h["denoised"]]))
    pt.ctx.wait()
    same(pt.denoised(), plain, "denoise, variance input unset")
    # render(denoise=True) without temporal clears the input too
    pt.ctx.set_denoise_variance_input(h["moments"])
    pt.render(gs[-1], denoise=True)
    same(pt.denoised(), rd.denoise(as_orc(gs[-1]), *pt.gbuffer(), pt.light()), "denoise alone after a temporal frame")
    pt.close()


def test_deterministic_and_outputs_prefilled_with_nan():
    W, H = 128, 96
    pt = tracer(scenes.cornell(), (W, H))
    gs = [pt.make_gconst(camera(scenes.CORNELL_CAMERA, (W, H), s, CORNELL_MOVE), 1, 4, frame=9 + s, flags=L.F_FACEFORWARD) for s in range(3)]
    a = check_sequence(pt, gs, "run 1")
    nan = np.full((H, W, 4), np.nan, F)
    for name in ("accumulated", "History", "Moments", "PrevHistory", "PrevMoments"):  # reset_history() must not depend on what they hold
        pt.rg.upload(pt.rg.named[name], nan)
    b = check_sequence(pt, gs, "run 2")
    for k in ("out", "hist", "mom"):
        assert np.array_equal(bits(a[k]), bits(b[k]))
    pt.close()


def test_errors_leave_the_context_usable():
    from raytracer3_amd.render_graph import ImageSize

    W, H = 100, 60
    pt = tracer(scenes.cornell(), (W, H))
    g0 = pt.make_gconst(camera(scenes.CORNELL_CAMERA, (W, H), 0, CORNELL_MOVE), 2, 3, frame=1, flags=L.F_FACEFORWARD)
    g = pt.make_gconst(camera(scenes.CORNELL_CAMERA, (W, H), 1, CORNELL_MOVE), 2, 3, frame=2, flags=L.F_FACEFORWARD)
    pt.render(g0, temporal=True)
    h = pt.render(g, temporal=True, denoise=True)
    first = (pt.accumulated(), *pt.history())
    lib, err = pt.ctx.lib, pt.ctx.last_error
    X, Y = math.ceil(W / 8), math.ceil(H / 8)
    names = ["gbuffer", "depth", "light", "prev_gbuffer", "prev_depth", "prev_history", "prev_moments", "accumulated", "history", "moments"]
    shown = ["gbuffer", "gbuffer_depth", "In", "PrevGbuffer", "PrevDepth", "PrevHistory", "PrevMoments", "Out", "History", "Moments"]
    good = [h[n] for n in names]

    def swapped(i, handle):
        b = list(good)
        b[i] = handle
        return b

    assert launch(pt, "temporal", X, Y, 1, g, good) == 0
    assert launch(pt, "temporal", X, Y, 1, g, good[:9]) == L.E_INVALID and "10 bindings" in err()
    assert launch(pt, "temporal", X, Y, 1, g, good + [h["denoised"]]) == L.E_INVALID and "10 bindings" in err()
    assert launch(pt, "temporal", W, H, 1, g, good) == L.E_INVALID and "ceil(W/8)" in err()
    assert launch(pt, "temporal", X, Y, 2, g, good) == L.E_INVALID
    small = pt.rg.image(ImageSize.XY(W - 4, H), L.FORMAT_R32G32B32A32_SFLOAT, "small")
    small_u = pt.rg.image(ImageSize.XY(W - 4, H), L.FORMAT_R32G32B32A32_UINT, "small_u")
    small_d = pt.rg.image(ImageSize.XY(W, H + 1), L.FORMAT_R32_SFLOAT, "small_d")
    buf = pt.rg.buffer(W * H * 16, "not_an_image")
    for i, n in enumerate(shown):  # every binding: another format, another size, no image
        wrong_format = h["depth"] if n not in ("gbuffer_depth", "PrevDepth") else h["light"]
        wrong_size = small_u if "buffer" in n.lower() and "depth" not in n.lower() else (small_d if "epth" in n else small)
        for bad in (wrong_format, wrong_size, buf, 0):
            assert launch(pt, "temporal", X, Y, 1, g, swapped(i, bad)) == L.E_INVALID and f"'{n}'" in err(), (n, bad)
    # the three written images differ from each other and from every image read
    for i, j in ((7, 8), (7, 9), (8, 9), (7, 2), (8, 5), (9, 6), (8, 2), (9, 5)):
        assert launch(pt, "temporal", X, Y, 1, g, swapped(i, good[j])) == L.E_INVALID and "different images" in err(), (i, j)
    # the previous view
    assert lib.rt3_temporal_set_prev_view(pt.ctx.h, C.byref(g0), 100) == L.E_INVALID and "304" in err()
    assert lib.rt3_temporal_set_prev_view(pt.ctx.h, None, 304) == L.E_INVALID
    assert lib.rt3_temporal_set_prev_view(None, None, 0) == L.E_INVALID
    assert launch(pt, "temporal", X, Y, 1, g, good) == 0  # ... refused calls left the view in place
    pt.ctx.set_prev_view(None)
    assert launch(pt, "temporal", X, Y, 1, g, good) == L.E_STATE and "previous view" in err()
    other = camera(scenes.CORNELL_CAMERA, (W, H)).gconst((W + 1, H))
    pt.ctx.set_prev_view(other)
    assert launch(pt, "temporal", X, Y, 1, g, good) == L.E_INVALID and "window_size" in err()
    pt.ctx.set_prev_view(g0)
    # parameters: refused values change nothing
    nanf, inf = float("nan"), float("inf")
    for kw in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=nanf), dict(alpha_moments=-1.0), dict(alpha_moments=2.0), dict(alpha_moments=nanf),
               dict(max_history=0), dict(max_history=65536), dict(normal_cos=1.5), dict(normal_cos=-1.5), dict(normal_cos=nanf),
               dict(plane_tolerance=0.0), dict(plane_tolerance=-1.0), dict(plane_tolerance=inf), dict(plane_tolerance=nanf), dict(flags=2)):
        p = L.TemporalParams(**kw)
        assert lib.rt3_temporal_set_params(pt.ctx.h, C.byref(p)) == L.E_INVALID and "temporal params" in err(), kw
    assert lib.rt3_temporal_set_params(None, None) == L.E_INVALID
    # the variance input of "denoise" is checked at launch
    dn = [h["gbuffer"], h["depth"], h["accumulated"], h["denoised"]]
    assert launch(pt, "denoise", X, Y, 1, g, dn) == 0
    for bad in (h["depth"], small, buf, 0x7FFFFFFF):
        pt.ctx.set_denoise_variance_input(bad)
        assert launch(pt, "denoise", X, Y, 1, g, dn) == L.E_INVALID and "variance input" in err(), bad
    pt.ctx.set_denoise_variance_input(h["denoised"])
    assert launch(pt, "denoise", X, Y, 1, g, dn) == L.E_INVALID and "must not be 'Out'" in err()
    assert lib.rt3_denoise_set_variance_input(None, 0) == L.E_INVALID
    pt.ctx.set_denoise_variance_input(h["moments"])
    assert launch(pt, "denoise", X, Y, 1, g, dn) == 0
    # a tile partition with more than one rank: a reprojected tap may belong to another rank
    pt.ctx.set_tile_partition(W, H, 1, 2)
    assert launch(pt, "temporal", X, Y, 1, g, good) == L.E_STATE and "other ranks own" in err()
    pt.ctx.set_tile_partition(W, H, 0, 1)
    assert launch(pt, "nonesuch", X, Y, 1, g, good) == L.E_INVALID and "temporal" in err()
    # ... and the context still computes the same frame, parameters untouched
    for n in ("accumulated", "history", "moments"):
        pt.rg.upload(h[n], np.full((H, W, 4), np.nan, F))
    assert launch(pt, "temporal", X, Y, 1, g, good) == 0
    pt.ctx.wait()
    for got, want in zip((pt.accumulated(), *pt.history()), first):
        assert np.array_equal(bits(got), bits(want))
    gs = [g0, g]
    check_sequence(pt, gs, "after the errors")
    pt.close()


def test_multi_rank_temporal_on_the_gather_root():
    """Three ranks on one GPU (the tiles travel through rt3_image_pack_tiles / rt3_gather_unpack, as in the denoise test).
    PathTracer.denoise(temporal=True) on the root -- partition off, G-buffer of the whole window, temporal and denoise on the gathered
    Light, partition back -- equals the single-rank frames bit for bit over two consecutive frames."""
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer

    mesh, sky, bn = scenes.atrium(0.25), scenes.sky(128, 64), assets.load_bluenoise()
    W, H, n, root = 200, 136, 3, 0
    solo = tracer(mesh, (W, H), sky=sky, bluenoise=bn)
    pts = [PathTracer((W, H), rank=r, n_ranks=n) for r in range(n)]
    for pt in pts:
        pt.set_scene(mesh, sky, bn)
    rootpt = pts[root]
    zero = np.zeros((H, W, 4), F)
    for k in range(2):
        g = solo.make_gconst(camera(scenes.ATRIUM_CAMERA, (W, H), k, ATRIUM_MOVE), 2, 3, frame=6 + k, flags=DEFAULT_FLAGS)
        solo.rg.upload(solo.commands(g)["light"], zero)  # k_accumulate leaves background pixels of Light unwritten: give them known bits
        solo.render(g, temporal=True, denoise=True)
        want = (solo.light(), solo.accumulated(), *solo.history(), solo.denoised())
        for pt in pts:
            pt.rg.upload(pt.commands(g)["light"], zero)
            pt.render(g)
        img = rootpt.handles["light"]
        off = rootpt.ctx.gather_layout(img, root, n)
        recv = rootpt.rg.buffer(off[-1] * 16, "recv")
        ptr, _ = rootpt.rg.device_ptr(recv)
        for r, pt in enumerate(pts):
            if r != root:
                pt.ctx.check(pt.ctx.lib.rt3_image_pack_tiles(pt.ctx.h, pt.handles["light"], r, n, C.c_void_p(ptr + off[r] * 16)))
                pt.ctx.wait()
        rootpt.ctx.gather_unpack(img, root, n, ptr)
        rootpt.denoise(g, temporal=True)
        got = (rootpt.light(), rootpt.accumulated(), *rootpt.history(), rootpt.denoised())
        for a, b, name in zip(got, want, ("Light", "Out", "History", "Moments", "denoised")):
            same(a, b, f"frame {k} {name}")
        if k:
            assert (want[2][..., 3] == 2).mean() > 0.5  # the second frame did reproject the first
        # the partition is back: the raw pass is refused again
        h = rootpt.handles
        b = [h[x] for x in ("gbuffer", "depth", "light", "prev_gbuffer", "prev_depth", "prev_history", "prev_moments", "accumulated", "history", "moments")]
        assert launch(rootpt, "temporal", math.ceil(W / 8), math.ceil(H / 8), 1, g, b) == L.E_STATE
    for pt in pts + [solo]:
        pt.close()


def test_cpp_host_renders_two_temporal_frames(tmp_path):
    """example_frame.cpp with the trailing word `temporal`: two frames through the C++ mirror's gbuffer -> refrence_mode -> temporal ->
    postprocess, the second from a moved camera; its accumulated image equals the reference chain on the two Lights"""
    import struct
    import subprocess

    from raytracer3_amd.renderer import Camera

    exe = Path(__file__).resolve().parent.parent / "raytracer3_amd" / "host" / "example_frame"
    if not exe.exists():
        subprocess.check_call(["make", "-C", str(exe.parent)])
    mesh, sky, bn = scenes.atrium(0.2), scenes.sky(256, 128), assets.load_bluenoise()
    W, H, spp, bounces, frame, flags = 96, 54, 2, 3, 9, 15
    cam = camera(scenes.ATRIUM_CAMERA, (W, H))
    scene = tmp_path / "scene.bin"
    with open(scene, "wb") as f:
        f.write(struct.pack("<8I", len(mesh.vertices), len(mesh.indices), len(mesh.geometries), sky.shape[1], sky.shape[0], bn.shape[1], bn.shape[0], 0))
        for arr in (mesh.vertices.astype("<f4"), mesh.indices.astype("<u4"), mesh.geometries, mesh.prim_counts.astype("<u4"), sky.astype("<f4"), bn):
            f.write(np.ascontiguousarray(arr).tobytes())
        f.write(np.array([*cam.position, *cam.direction, cam.fov, cam.aspect_ratio], "<f4").tobytes())
    out = tmp_path / "out.bin"
    subprocess.check_call([str(exe), str(scene), str(W), str(H), str(spp), str(bounces), str(flags), str(frame), str(out), "temporal"])
    light2, color, acc, light1 = np.fromfile(out, "<f4").reshape(4, H, W, 4)
    moved = Camera(cam.position, cam.direction, cam.fov, cam.aspect_ratio)  # the example adds its offset to the stored (unit) direction as it is
    moved.position = cam.position + np.array([0.02, 0.0, 0.01], F)
    moved.direction = cam.direction + np.array([0.0, 0.0, 0.012], F)
    gs = []
    for k, c in enumerate((cam, moved)):
        g = c.gconst((W, H))
        g.samples, g.bounces, g.frame, g.blendfactor = spp, bounces, frame + k, 1.0
        g.pad[0] = flags
        gs.append(as_orc(g))
    osc = orc.Scene(mesh, sky, bn)
    gb1, depth1 = osc.gbuffer(gs[0])
    gb2, depth2 = osc.gbuffer(gs[1])
    zero = np.zeros((H, W, 4), F)
    _, hist1, mom1 = rt.temporal(gs[0], gb1, depth1, light1, gs[0], gb1, depth1, zero, zero)
    want, hist2, _ = rt.temporal(gs[1], gb2, depth2, light2, gs[0], gb1, depth1, hist1, mom1)
    same(acc, want, "accumulated image of the second frame")
    assert (hist2[..., 3] == 2).mean() > 0.5
    assert np.allclose(color, osc.postprocess(gs[1], depth2, acc), atol=2e-5, rtol=1e-4)
