"""The guide images of a lens frame and the "denoise" pass guided by them, without a GPU: tests/ref_guide.py, the
numpy float32 restatement that tests/test_guide.py holds the MI355X to, against a plain Python loop and a float64 sum; its invariance
under the batch size; the guided filter's end stages on a synthetic guide; and the Python surface (the frame's nodes, the bindings)."""
import numpy as np

import ref_guide as rg
from raytracer3_amd import _lib as L
from support import RecordingCtx, bits

F = np.float32
U = 2.0 ** -24


def samples(seed, S, npix, p_hit=0.7):
    rng = np.random.default_rng(seed)
    hit = rng.random((S, npix)) < p_hit
    hit[:, 0] = True   # an all-hit pixel,
    hit[:, 1] = False  # an all-miss pixel,
    hit[: S // 2, 2], hit[S // 2:, 2] = True, False  # and a mixed one whatever the draw
    o = rng.normal(size=(S, npix, 3)).astype(F)
    d = rng.normal(size=(S, npix, 3)).astype(F)
    t = rng.uniform(0.5, 30.0, (S, npix)).astype(F)
    n = rng.normal(size=(S, npix, 3)).astype(F)
    n /= np.linalg.norm(n, axis=-1, keepdims=True).astype(F)
    a = rng.random((S, npix, 3)).astype(F)
    e = (rng.random((S, npix, 3)) * (rng.random((S, npix, 1)) < 0.3) * 12.0).astype(F)
    bad = ~hit  # what a miss carries is never read
    for arr in (o, d, n, a, e):
        arr[bad] = np.nan
    t[bad] = np.nan
    return hit, o, d, t, n, a, e


def python_loop(hit, o, d, t, n, a, e):
    """the definition, one scalar float32 operation at a time"""
    S, npix = hit.shape
    out = rg.zero_state(npix)
    for i in range(npix):
        sP, sN, sA, sE, nh = [F(0)] * 3, [F(0)] * 3, [F(0)] * 3, [F(0)] * 3, F(0)
        for s in range(S):
            if hit[s, i]:
                for k in range(3):
                    sP[k] = F(sP[k] + F(o[s, i, k] + F(d[s, i, k] * t[s, i])))
                    sN[k] = F(sN[k] + n[s, i, k])
                    sA[k] = F(sA[k] + a[s, i, k])
                    sE[k] = F(sE[k] + e[s, i, k])
                nh = F(nh + F(1))
            else:
                for k in range(3):
                    sA[k] = F(sA[k] + F(1))
        fs = F(S)
        if nh > 0:
            out["position"][i] = [F(sP[0] / nh), F(sP[1] / nh), F(sP[2] / nh), F(nh / fs)]
            out["normal"][i] = [F(sN[0] / nh), F(sN[1] / nh), F(sN[2] / nh), F(0)]
        out["albedo"][i] = [F(sA[0] / fs), F(sA[1] / fs), F(sA[2] / fs), F(0)]
        out["emission"][i] = [F(sE[0] / fs), F(sE[1] / fs), F(sE[2] / fs), F(0)]
    return out


def test_accumulate_is_the_plain_loop_and_close_to_float64():
    S, npix = 13, 40
    data = samples(3, S, npix)
    got = rg.accumulate(*data, S)
    want = python_loop(*data)
    for k in rg.KEYS:
        assert got[k].dtype == F and np.array_equal(bits(got[k]), bits(want[k])), k
    hit, o, d, t, n, a, e = (x.astype(np.float64) if x.dtype != bool else x for x in data)
    h3 = hit[..., None]
    nh = hit.sum(0)
    assert (nh == S).any() and (nh == 0).any() and ((nh > 0) & (nh < S)).any()
    # S - 1 roundings of the running sum and one of the division: (S + 1) 2^-24 relative, of the sum of magnitudes where terms change sign;
    # a position term carries the two roundings of o + d t besides
    with np.errstate(all="ignore"):
        P = np.where(h3, o + d * t[..., None], 0.0)
        Pmag = np.where(h3, np.abs(o) + np.abs(d * t[..., None]), 0.0)
        some = nh > 0
        nhs = np.maximum(nh, 1)[:, None]
        checks = [
            (got["position"][:, :3], P.sum(0) / nhs, Pmag.sum(0) / nhs, S + 3),
            (got["normal"][:, :3], np.where(h3, n, 0.0).sum(0) / nhs, np.where(h3, np.abs(n), 0.0).sum(0) / nhs, S + 1),
            (got["albedo"][:, :3], np.where(h3, a, 1.0).sum(0) / S, np.where(h3, a, 1.0).sum(0) / S, S + 1),
            (got["emission"][:, :3], np.where(h3, e, 0.0).sum(0) / S, np.where(h3, e, 0.0).sum(0) / S, S + 1),
        ]
    for have, ref, mag, n_round in checks:
        err = np.abs(have.astype(np.float64) - ref)
        assert np.all(err <= n_round * U * mag + 1e-300)
    assert np.array_equal(got["position"][:, 3], (nh / S).astype(F)) and not got["position"][~some].any() and not got["normal"][~some].any()
    assert np.all(got["albedo"][nh == 0, :3] == 1.0), "an all-miss pixel has the sky's albedo 1"
    for k in ("normal", "albedo", "emission"):
        assert not got[k][:, 3].any()


def test_accumulate_does_not_depend_on_the_batch_size():
    S, npix = 7, 64
    data = samples(9, S, npix)
    whole = rg.accumulate(*data, S)
    for batch in (1, 3, S):
        part = rg.accumulate_split(*data, batch)
        for k in rg.KEYS:
            assert np.array_equal(bits(part[k]), bits(whole[k])), (batch, k)
    # between batches the images hold the sums, the count in position.w
    mid = rg.accumulate(*(x[:3] for x in data), S, first=True, last=False)
    assert np.array_equal(mid["position"][:, 3], data[0][:3].sum(0).astype(F))


def synthetic_guide(H=21, W=37, seed=5):
    """a floor and a wall under a random albedo and emission, with a band of partly covered pixels, a zero normal and a NaN normal"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(F)
    wall = xs > W * 0.6
    pos = np.where(wall[..., None], np.stack([np.full_like(xs, 10.0), ys * 0.1, xs * 0.1], -1), np.stack([xs * 0.1, np.zeros_like(xs), ys * 0.1], -1))
    nrm = np.where(wall[..., None], np.array([-0.9, 0.0, 0.1], F), np.array([0.02, 0.8, 0.0], F))  # means of unit normals: shorter than 1
    g = dict(position=np.concatenate([pos, np.ones((H, W, 1), F)], -1).astype(F), normal=np.concatenate([nrm, np.zeros((H, W, 1), F)], -1).astype(F),
             albedo=np.concatenate([rng.uniform(0.25, 1.0, (H, W, 3)), np.zeros((H, W, 1))], -1).astype(F),
             emission=np.concatenate([rng.uniform(0.0, 1.0, (H, W, 3)) * (rng.random((H, W, 1)) < 0.2), np.zeros((H, W, 1))], -1).astype(F))
    special = np.zeros((H, W), bool)
    g["position"][5, 4:30, 3] = 0.75  # partly covered
    g["position"][9, 7, 3] = 0.0
    g["normal"][12, 10, :3] = 0.0
    g["normal"][13, 20, 0] = np.nan
    g["normal"][14, 22, 1] = np.inf
    special[5, 4:30] = special[9, 7] = special[12, 10] = special[13, 20] = special[14, 22] = True
    return g, special


def test_guided_filter_end_stages():
    g, special = synthetic_guide()
    H, W = special.shape
    rng = np.random.default_rng(8)
    light = np.concatenate([rng.gamma(0.5, 1.0, (H, W, 3)), rng.random((H, W, 1))], -1).astype(F)
    fg, _ = rg.foreground(g)
    assert np.array_equal(fg, ~special)
    # iterations = 0 is a copy
    assert np.array_equal(bits(rg.denoise(g, light, iterations=0)), bits(light))
    for flags in (0, rg.rd.NO_DEMODULATION):
        out = rg.denoise(g, light, iterations=3, flags=flags)
        assert np.array_equal(bits(out[special]), bits(light[special])), "pixels that are not foreground are copied"
        assert np.array_equal(bits(out[..., 3]), bits(light[..., 3])), "alpha is copied"
        assert not np.array_equal(bits(out[fg]), bits(light[fg])), "it did filter"
        # ... and they weigh nothing as taps: other values there, NaN included, change no other pixel
        other = light.copy()
        other[special] = rng.gamma(2.0, 5.0, (int(special.sum()), 4)).astype(F)
        other[5, 10] = np.nan
        out2 = rg.denoise(g, other, iterations=3, flags=flags)
        assert np.array_equal(bits(out2[fg]), bits(out[fg]))
        assert np.array_equal(bits(out2[special]), bits(other[special]))


def test_constant_signal_comes_back():
    """In = e + k m: the demodulated signal is k everywhere but for rounding, whatever the weights; ref_guide.constant_signal_bound has the
    derivation.  The three roundings of the end stages alone (iterations' term left out) are printed beside the measured error."""
    g, special = synthetic_guide(seed=6)
    fg = ~special
    k = F(0.37)
    m = np.where(g["albedo"][..., :3] > rg.rd.ALBEDO_FLOOR, g["albedo"][..., :3], rg.rd.ALBEDO_FLOOR)
    light = np.concatenate([g["emission"][..., :3] + k * m, np.ones(special.shape + (1,), F)], -1).astype(F)
    for it in (1, 5):
        out = rg.denoise(g, light, iterations=it)
        err = np.abs(out[..., :3].astype(np.float64) - light[..., :3])[fg]
        bound = rg.constant_signal_bound(light, m, float(k), it, fg)[fg]
        ends = rg.constant_signal_bound(light, m, float(k), 0, fg)[fg]
        print(f"{it} iterations: worst |Out - In| {err.max() / U:.2f} units of 2^-24, worst share of the bound {np.max(err / bound):.3f} "
              f"(of the end stages' part alone {np.max(err / ends):.3f})")
        assert np.all(err <= bound)
    # the bound is a few units where the values are of order 1: it is no licence for a visible error
    assert rg.constant_signal_bound(light, m, float(k), 5, fg)[fg].max() <= 400 * U


def test_frame_nodes_declare_the_guide_as_context_state():
    """the four images are writes of the path-trace node and reads of "denoise", which order the frame, and are no bindings"""
    from raytracer3_amd.render_graph import RenderGraph
    from raytracer3_amd.renderer import frame_nodes, guide_images

    ctx = RecordingCtx()
    graph = RenderGraph(ctx, (16, 8))
    g = L.GConst()
    h = frame_nodes(graph, g, postprocess=True, denoise=True, guide=True)
    assert h["guide"] == guide_images(graph) and list(h["guide"]) == list(rg.KEYS) and len(set(h["guide"].values())) == 4
    graph.draw_frame(h["color"])
    names = [c[0] for c in ctx.calls]
    assert names == ["gbuffer", "refrence_mode", "denoise", "postprocess"]
    by = {c[0]: c[2] for c in ctx.calls}
    assert by["refrence_mode"] == [h["gbuffer"], h["depth"], h["light"], h["prev"]]
    assert by["denoise"] == [h["gbuffer"], h["depth"], h["light"], h["denoised"]]
    trace = next(n for n in graph.nodes if n.name == "refrence_mode")
    dn = next(n for n in graph.nodes if n.name == "denoise")
    assert [e.resource for e in trace.edges if e.edge_type == "StateWrite"] == list(h["guide"].values())
    assert [e.resource for e in dn.edges if e.edge_type == "StateRead"] == list(h["guide"].values())
    assert all(graph.nodes[e.origin].name == "refrence_mode" for e in dn.edges if e.edge_type == "StateRead")
    # over a Light that is already there (PathTracer.denoise) the guide is imported; without `guide` nothing changes
    graph.begin_frame()
    h2 = frame_nodes(graph, g, False, True, trace=False, gbuffer_node=False, guide=True)
    assert [e.origin for e in graph.nodes[-1].edges if e.edge_type == "StateRead"] == [None] * 4 and h2["guide"] == h["guide"]
    graph.begin_frame()
    h3 = frame_nodes(graph, g, True, True)
    assert "guide" not in h3 and not any(e.edge_type.startswith("State") for n in graph.nodes for e in n.edges)


def test_bindings_are_declared():
    for name in ("rt3_camera_set_guide_output", "rt3_camera_get_guide_output", "rt3_denoise_set_guide_input"):
        assert name in L.EXPORTS
    gi = L.GuideImages(1, 2, 3, 4)
    assert gi.handles() == (1, 2, 3, 4) and L.SELFTEST_GUIDE_QUEUE == 39
    import ctypes as C
    assert C.sizeof(L.GuideImages) == 16
