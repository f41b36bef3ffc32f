"""The "denoise" pass on the MI355X: bit-for-bit parity with tests/ref_denoise.py (the numpy float32 restatement
that tests/test_denoise_cpu.py pins), expn alone, the documented errors, determinism, and the multi-rank path.  The input frames come
from the GPU passes themselves, which test_gpu_parity.py pins to the oracle."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

import orc
import ref_denoise as rd
from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes
from support import as_orc, bits, camera, launch, tracer

pytestmark = pytest.mark.gpu
BG = np.float32(orc.BACKGROUND_DEPTH)


def check_parity(pt, g, what, **params):
    """render gbuffer -> refrence_mode -> denoise with `params`; Out must equal the reference filter of the frame's own Light"""
    pt.ctx.set_denoise_params(**params) if params else pt.ctx.set_denoise_params()
    pt.render(g, denoise=True)
    light, out = pt.light(), pt.denoised()
    gb, depth = pt.gbuffer()
    want = rd.denoise(as_orc(g), gb, depth, light, **dict(rd.DEFAULTS, **params))
    diff = bits(out) != bits(want)
    fg = depth != BG
    print(f"{what}: {pt.window[0]}x{pt.window[1]}, {int(fg.sum())} foreground pixels, {int(diff.any(-1).sum())} pixels differ")
    assert not diff.any(), f"{what}: {int(diff.any(-1).sum())} pixels differ, first at {np.argwhere(diff.any(-1))[:3].tolist()}"
    assert params.get("iterations", 5) == 0 or not np.array_equal(bits(out)[fg], bits(light)[fg])  # it did filter
    return light, out, gb, depth


def test_parity_cornell_iterations_and_parameters():
    W = H = 128
    pt = tracer(scenes.cornell(), (W, H))
    cam = camera(scenes.CORNELL_CAMERA, (W, H))
    for spp in (1, 16):
        g = pt.make_gconst(cam, spp, 4, frame=7, flags=L.F_FACEFORWARD)
        check_parity(pt, g, f"cornell {spp} spp")
    g = pt.make_gconst(cam, 1, 4, frame=3, flags=L.F_FACEFORWARD)
    for it in (1, 3, 5, 8):
        check_parity(pt, g, f"cornell 1 spp, {it} iterations", iterations=it)
    check_parity(pt, g, "cornell, demodulation off", flags=L.DENOISE_NO_DEMODULATION)
    check_parity(pt, g, "cornell, other parameters", iterations=4, normal_squarings=5, sigma_z=0.1, sigma_l=2.0)
    check_parity(pt, g, "cornell, no normal weight, wide sigmas", iterations=2, normal_squarings=0, sigma_z=3.0, sigma_l=50.0)
    # iterations = 0: a copy of In, bit for bit
    light, out, _, _ = check_parity(pt, g, "cornell, 0 iterations", iterations=0)
    assert np.array_equal(bits(out), bits(light))
    pt.close()


def test_parity_atrium_sky_columns_and_odd_window():
    from raytracer3_amd.renderer import DEFAULT_FLAGS

    sky, bn = scenes.sky(512, 256), assets.load_bluenoise()
    for W, H in ((192, 108), (250, 187)):  # 250 x 187: no multiple of 8 nor of the kernels' tile
        pt = tracer(scenes.atrium(0.25), (W, H), sky=sky, bluenoise=bn)
        g = pt.make_gconst(camera(scenes.ATRIUM_CAMERA, (W, H)), 1, 4, frame=5, flags=DEFAULT_FLAGS)
        light, out, gb, depth = check_parity(pt, g, "atrium 1 spp")
        fg = depth != BG
        assert (~fg).any() and np.array_equal(bits(out)[~fg], bits(light)[~fg])  # sky pixels pass through
        assert np.array_equal(bits(out[..., 3]), bits(light[..., 3]))
        # through the tone map: postprocess reads the filtered image
        pt.render(g, postprocess=True, denoise=True)
        col = pt.color()
        osc_col = orc.Scene(scenes.atrium(0.25), sky, bn).postprocess(as_orc(g), depth, out)
        assert np.allclose(col, osc_col, atol=2e-5, rtol=1e-4)
        pt.close()


def test_parity_textured_cornell():
    W, H = 160, 120
    pt = tracer(scenes.textured_cornell(), (W, H))
    g = pt.make_gconst(camera(scenes.CORNELL_CAMERA, (W, H)), 4, 3, frame=2, flags=L.F_FACEFORWARD | L.F_SPECULAR)
    check_parity(pt, g, "textured cornell 4 spp")
    check_parity(pt, g, "textured cornell 4 spp, 3 iterations", iterations=3)
    pt.close()


def test_expn_selftest_bit_exact():
    from raytracer3_amd.render_graph import Context

    rng = np.random.default_rng(11)
    x = np.concatenate([
        np.linspace(0.0, 110.0, 1_000_001).astype(np.float32),
        np.array([0.0, 1e-45, 1e-38, 1e-10, 87.0, 87.33655, 88.0, 95.0, 103.0, 103.9, 103.97, 103.972, 103.98, 104.0, 150.0, 1e10, 3.4e38, np.inf], np.float32),
        rng.integers(0, 0x7F800000, 200_000, dtype=np.uint32).view(np.float32),  # every magnitude of positive float32
    ])
    want = rd.expn(x)
    assert ((want > 0) & (want < np.float32(1.1754944e-38))).sum() > 1000  # denormal results are part of the comparison
    ctx = Context(0)
    got = ctx.selftest(L.SELFTEST_EXPN, bits(x).reshape(-1, 1), 1).reshape(-1)
    ctx.close()
    bad = np.flatnonzero(got != bits(want))
    assert bad.size == 0, f"{bad.size} of {x.size} differ, e.g. x = {x[bad[:4]].tolist()}"


def test_errors_leave_the_context_usable():
    from raytracer3_amd.render_graph import ImageSize

    W, H = 100, 60
    pt = tracer(scenes.cornell(), (W, H))
    g = pt.make_gconst(camera(scenes.CORNELL_CAMERA, (W, H)), 2, 3, frame=1, flags=L.F_FACEFORWARD)
    h = pt.commands(g, denoise=True)
    pt.rg.draw_frame(h["denoised"], wait=True)
    first = pt.denoised()
    lib, err = pt.ctx.lib, pt.ctx.last_error
    X, Y = math.ceil(W / 8), math.ceil(H / 8)
    good = [h["gbuffer"], h["depth"], h["light"], h["denoised"]]
    assert launch(pt, "denoise", X, Y, 1, g, good) == 0
    assert launch(pt, "denoise", X, Y, 1, g, [h["gbuffer"], h["depth"], h["light"], h["light"]]) == L.E_INVALID and "different images" in err()
    assert launch(pt, "denoise", X, Y, 1, g, good[:3]) == L.E_INVALID and "4 bindings" in err()
    assert launch(pt, "denoise", X, Y, 1, g, good + [h["prev"]]) == L.E_INVALID and "4 bindings" in err()
    assert launch(pt, "denoise", W, H, 1, g, good) == L.E_INVALID and "ceil(W/8)" in err()
    assert launch(pt, "denoise", X, Y, 2, g, good) == L.E_INVALID
    assert launch(pt, "denoise", X, Y, 1, g, [h["depth"], h["depth"], h["light"], h["denoised"]]) == L.E_INVALID and "'gbuffer'" in err()
    assert launch(pt, "denoise", X, Y, 1, g, [h["gbuffer"], h["gbuffer"], h["light"], h["denoised"]]) == L.E_INVALID and "'gbuffer_depth'" in err()
    assert launch(pt, "denoise", X, Y, 1, g, [h["gbuffer"], h["depth"], h["depth"], h["denoised"]]) == L.E_INVALID and "'In'" in err()
    small = pt.rg.image(ImageSize.XY(W - 4, H), L.FORMAT_R32G32B32A32_SFLOAT, "small")
    assert launch(pt, "denoise", X, Y, 1, g, [h["gbuffer"], h["depth"], h["light"], small]) == L.E_INVALID and "'Out'" in err()
    buf = pt.rg.buffer(W * H * 16, "not_an_image")
    assert launch(pt, "denoise", X, Y, 1, g, [h["gbuffer"], h["depth"], buf, h["denoised"]]) == L.E_INVALID
    # parameters: refused values change nothing
    for kw in (dict(iterations=9), dict(normal_squarings=17), dict(sigma_z=0.0), dict(sigma_z=-1.0), dict(sigma_l=float("nan")),
               dict(sigma_l=float("inf")), dict(sigma_z=float("nan")), dict(flags=2)):
        p = L.DenoiseParams(**kw)
        assert lib.rt3_denoise_set_params(pt.ctx.h, C.byref(p)) == L.E_INVALID and "denoise params" in err(), kw
    assert lib.rt3_denoise_set_params(None, None) == L.E_INVALID
    # a tile partition with more than one rank: a tap needs pixels other ranks own
    pt.ctx.set_tile_partition(W, H, 1, 2)
    assert launch(pt, "denoise", X, Y, 1, g, good) == L.E_STATE and "other ranks own" in err()
    pt.ctx.set_tile_partition(W, H, 0, 1)
    # ... and the context still renders the same frame, parameters untouched
    pt.rg.upload(h["denoised"], np.zeros((H, W, 4), np.float32))
    pt.rg.draw_frame(h["denoised"], wait=True)
    assert np.array_equal(bits(pt.denoised()), bits(first))
    check_parity(pt, g, "after the errors")
    pt.close()


def test_deterministic_and_scratch_reuse():
    """two runs give the same bits; a second, larger window on the same context grows the scratch and still matches the reference; a
    pre-existing garbage Out does not leak into the result"""
    W, H = 128, 96
    pt = tracer(scenes.cornell(), (W, H))
    g = pt.make_gconst(camera(scenes.CORNELL_CAMERA, (W, H)), 1, 4, frame=9, flags=L.F_FACEFORWARD)
    _, a, _, _ = check_parity(pt, g, "run 1")
    pt.rg.upload(pt.handles["denoised"], np.full((H, W, 4), np.nan, np.float32))
    _, b, _, _ = check_parity(pt, g, "run 2")
    assert np.array_equal(bits(a), bits(b))
    # the same context, other window sizes through the raw ABI (scratch grows, then is reused for the smaller one)
    from raytracer3_amd.render_graph import ImageSize
    for k, (w, h) in enumerate(((200, 150), (64, 40))):
        gg = camera(scenes.CORNELL_CAMERA, (w, h)).gconst((w, h))
        gg.samples, gg.bounces, gg.frame, gg.blendfactor = 1, 3, 4, 1.0
        gg.pad[0] = L.F_FACEFORWARD
        pt.ctx.set_tile_partition(w, h, 0, 1)
        img = {n: pt.rg.image(ImageSize.XY(w, h), f, f"{n}{k}") for n, f in (("gb", L.FORMAT_R32G32B32A32_UINT), ("depth", L.FORMAT_R32_SFLOAT),
               ("light", L.FORMAT_R32G32B32A32_SFLOAT), ("prev", L.FORMAT_R32G32B32A32_SFLOAT), ("out", L.FORMAT_R32G32B32A32_SFLOAT))}
        assert launch(pt, "gbuffer", w, h, 1, gg, [img["gb"], img["depth"]]) == 0
        assert launch(pt, "refrence_mode", w, h, 1, gg, [img["gb"], img["depth"], img["light"], img["prev"]]) == 0
        assert launch(pt, "denoise", math.ceil(w / 8), math.ceil(h / 8), 1, gg, [img["gb"], img["depth"], img["light"], img["out"]]) == 0
        pt.ctx.wait()
        gb, depth = pt.rg.download(img["gb"], (h, w, 4), np.uint32), pt.rg.download(img["depth"], (h, w), np.float32)
        light, out = pt.rg.download(img["light"], (h, w, 4), np.float32), pt.rg.download(img["out"], (h, w, 4), np.float32)
        assert np.array_equal(bits(out), bits(rd.denoise(as_orc(gg), gb, depth, light)))
    pt.close()


def test_windows_around_the_tile_size():
    """Steps 1 and 2 and the variance stage work from LDS tiles of 32 x 8 pixels plus a border, wider steps from cached loads: windows that
    are no multiple of the tile, smaller than one tile, and narrower than the 7 x 7 window must match the reference all the same (8 iterations: every path)."""
    from raytracer3_amd.renderer import DEFAULT_FLAGS

    sky, bn = scenes.sky(128, 64), assets.load_bluenoise()
    for W, H in ((97, 41), (20, 6), (33, 3), (3, 9)):
        pt = tracer(scenes.atrium(0.25), (W, H), sky=sky, bluenoise=bn)
        cam = camera(scenes.ATRIUM_CAMERA, (W, H))
        g = pt.make_gconst(cam, 1, 3, frame=8, flags=DEFAULT_FLAGS)
        check_parity(pt, g, "odd window", iterations=8)
        check_parity(pt, g, "odd window")
        pt.close()


def test_multi_rank_denoise_on_the_gather_root():
    """Three ranks on one GPU (RCCL cannot put three ranks on one device: the tiles travel through rt3_image_pack_tiles /
    rt3_gather_unpack at the offsets rt3_gather_layout reports, as in the probe test).  PathTracer.denoise() on the root -- partition off,
    G-buffer of the whole window, filter of the gathered Light -- equals the single-rank denoised frame bit for bit."""
    from raytracer3_amd.renderer import DEFAULT_FLAGS, PathTracer

    mesh, sky, bn = scenes.atrium(0.25), scenes.sky(128, 64), assets.load_bluenoise()
    W, H, n, root = 200, 136, 3, 0
    cam = camera(scenes.ATRIUM_CAMERA, (W, H))
    solo = tracer(mesh, (W, H), sky=sky, bluenoise=bn)
    g = solo.make_gconst(cam, 2, 3, frame=6, flags=DEFAULT_FLAGS)
    zero = np.zeros((H, W, 4), np.float32)
    solo.rg.upload(solo.commands(g)["light"], zero)  # k_accumulate leaves background pixels of Light unwritten: give them known bits
    solo.render(g, denoise=True)
    ref_light, ref = solo.light(), solo.denoised()
    pts = [PathTracer((W, H), rank=r, n_ranks=n) for r in range(n)]
    for pt in pts:
        pt.set_scene(mesh, sky, bn)
        pt.rg.upload(pt.commands(g)["light"], zero)
        pt.render(g)
    rootpt = pts[root]
    img = rootpt.handles["light"]
    off = rootpt.ctx.gather_layout(img, root, n)
    recv = rootpt.rg.buffer(off[-1] * 16, "recv")
    ptr, _ = rootpt.rg.device_ptr(recv)
    for r, pt in enumerate(pts):
        if r != root:
            pt.ctx.check(pt.ctx.lib.rt3_image_pack_tiles(pt.ctx.h, pt.handles["light"], r, n, C.c_void_p(ptr + off[r] * 16)))
            pt.ctx.wait()
    rootpt.ctx.gather_unpack(img, root, n, ptr)
    assert np.array_equal(bits(rootpt.light()), bits(ref_light))
    rootpt.denoise(g)
    assert np.array_equal(bits(rootpt.denoised()), bits(ref))
    # the partition is back: the raw pass is refused again, and the root still renders only its own tiles
    h = rootpt.handles
    assert launch(rootpt, "denoise", math.ceil(W / 8), math.ceil(H / 8), 1, g, [h["gbuffer"], h["depth"], h["light"], h["denoised"]]) == L.E_STATE
    rootpt.rg.upload(rootpt.commands(g)["light"], zero)
    rootpt.render(g)
    own = np.zeros((H, W), bool)
    xy = orc.tile_pixels(W, H, root, n)
    own[xy[:, 1], xy[:, 0]] = True
    assert np.array_equal(bits(rootpt.light()), bits(np.where(own[..., None], ref_light, zero)))
    # one rank is the plain case: denoise() filters the Light of the last render()
    solo.render(g)
    solo.denoise(g)
    assert np.array_equal(bits(solo.denoised()), bits(ref))
    for pt in pts + [solo]:
        pt.close()


def test_cpp_host_names_the_pass(tmp_path):
    """example_frame.cpp with the trailing word `denoise`: the C++ mirror's node chain gbuffer -> refrence_mode -> denoise -> postprocess"""
    import struct
    import subprocess

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
    subprocess.check_call([str(exe), str(scene), str(W), str(H), str(spp), str(bounces), str(flags), str(frame), str(out), "denoise"])
    light, color, denoised = np.fromfile(out, "<f4").reshape(3, H, W, 4)
    g = cam.gconst((W, H))
    g.samples, g.bounces, g.frame, g.blendfactor = spp, bounces, frame, 1.0
    g.pad[0] = flags
    osc = orc.Scene(mesh, sky, bn)
    gb, depth = osc.gbuffer(as_orc(g))
    want = rd.denoise(as_orc(g), gb, depth, light)
    assert np.array_equal(bits(denoised), bits(want))
    assert np.allclose(color, osc.postprocess(as_orc(g), depth, denoised), atol=2e-5, rtol=1e-4)
