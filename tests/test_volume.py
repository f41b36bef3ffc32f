"""Absorbing glass on the GPU (rt3_scene_set_attenuation): the rule against float64, k_absorb on caller-made queues, the two
closed forms of an absorbing slab, "nothing changes without it", the whole integrator against the float64 fixture, invariance under batch
size, instance mode, tile partition and window size, roulette and the adaptive pass on top of it, and the contract of the new call.

Bounds are derived, in the docstrings of the tests that use them: fp32 results carry one unit of U = 2^-24 per rounding of the longest
chain; means of bounded samples are held within 5 sigma of the bounded deviation."""
import math

import numpy as np
import pytest

import adaptive_lens_worlds as alw
import glass_worlds as GW
import integrator_worlds as IW
import lens_worlds as LW
import ref_roulette as RR
import ref_volume as RV
import volume_worlds as VW
from raytracer3_amd import _lib as L
from raytracer3_amd import assets
from support import bits, camera
from test_adaptive_lens import LensWorld, check_against_fixed, everything
from test_glass import frame, glass_pt, sky_bound
from test_integrator_cpu import check_against_fixture
from test_nee_emissive import make_pt, owned_mask
from test_volume_cpu import fixture

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0**-24
FULL = L.F_NEE_SKY | L.F_BLUENOISE | L.F_FACEFORWARD | L.F_SPECULAR
SKY = np.array(VW.SKY_L)
MISS = 0xFFFFFFFF


def rule_bound(a):
    """Relative bound of T' = T expf(-(sigma x)), x = t sqrtf(dot(d, d)), against float64 from the same fp32 inputs, a = sigma x:
    on the way to the exponent the longest chain rounds five times (a product and a sum of dot(d, d) -- its three terms are positive, so
    each rounding is relative --, the square root, which halves what came before and adds its own, the product with t, the product with
    sigma): at most 5 half-ulps, U each, relative to a, i.e. an absolute 5 a U on the exponent and so a relative 5 a U (1 + 5 a U) < 6 a U
    on the result for a <= 80; expf is documented at 1 ulp = 2 U; the product with T rounds once, U; second-order terms fit in the fourth
    unit.  (4 + 6 a) U.  Derived, not measured."""
    return (4.0 + 6.0 * np.asarray(a, np.float64)) * U


@pytest.fixture(scope="module")
def ctx():
    """a context with a small world (op 36 reads no context state)"""
    pt = make_pt(IW.open_room(), IW.WINDOW_ROOM)
    yield pt.ctx
    pt.close()


# ---------------------------------------------------------------------------------------------------------------- 1 the rule
def op36_rows(n=6000, seed=5):
    """{T, sigma, t, d, n}: a = sigma x up to 80, |d| from 0.5 to 2, both signs of n.d (|cos| >= 0.05, so that float32 and float64 agree on
    the sign), a quarter of the channels and a tenth of the rows with sigma 0"""
    rng = np.random.default_rng(seed)
    T = rng.uniform(0.05, 1.5, (n, 3))
    d = rng.normal(size=(n, 3))
    d *= (rng.uniform(0.5, 2.0, n) / np.linalg.norm(d, axis=1))[:, None]
    nn = rng.normal(size=(n, 3))
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    t = rng.uniform(0.01, 10.0, n)
    a = 80.0 * rng.random((n, 3)) ** 3
    sigma = a / (t * np.linalg.norm(d, axis=1))[:, None]
    sigma[rng.random((n, 3)) < 0.25] = 0.0
    sigma[rng.random(n) < 0.1] = 0.0
    rows = np.concatenate([T, sigma, t[:, None], d, nn], 1).astype(F)
    cos = np.sum(rows[:, 10:13].astype(np.float64) * rows[:, 7:10], 1) / np.linalg.norm(rows[:, 7:10].astype(np.float64), axis=1)
    return rows[np.abs(cos) >= 0.05]


def test_rule_against_float64(ctx):
    """self-test op 36 within rule_bound of float64 from the same fp32 inputs; rows with n.d <= 0 or every sigma 0 keep their bits"""
    rows = op36_rows()
    got, applied = ctx.selftest_absorb(rows)
    r = rows.astype(np.float64)
    T, sigma, t, d, nn = r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7:10], r[:, 10:13]
    x = t * np.linalg.norm(d, axis=1)
    want, back = RV.absorb(T, sigma, x, nn, d)
    assert len(rows) > 4000 and 0.3 < back.mean() < 0.6 and (~back & (np.sum(nn * d, 1) > 0)).sum() > 100
    assert np.array_equal(applied, back)
    assert np.array_equal(bits(got[~back]), bits(rows[~back, 0:3]))
    a = sigma * x[:, None]
    assert a.max() > 70.0
    rel = np.abs(got.astype(np.float64) / want - 1.0)[back]
    ratio = rel / rule_bound(a[back])
    print(f"op 36: worst relative error / bound {ratio.max():.3f} over {int(back.sum())} rows (largest a {a.max():.1f}); worst in units of U {np.max(rel) / U:.1f}")
    assert np.all(ratio <= 1.0)
    keep = back[:, None] & (sigma == 0.0)  # a channel with sigma 0 keeps its bits in a row that is attenuated
    assert keep.sum() > 100 and np.array_equal(bits(got)[keep], bits(rows[:, 0:3])[keep])


# ---------------------------------------------------------------------------------------------------------------- 2 the kernel on a queue
QUEUE_N = (1, 63, 64, 65, 511, 512, 513, 1537)
CORNERS = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.5, 0.5), (0.5, 0.0), (0.0, 0.5), (0.25, 0.25), (1.0 / 3.0, 1.0 / 3.0)]


def queue(mesh, matrix, n, seed):
    """n records {d, t, u, v, prim, T} over the triangles of volume_worlds.bodies() -- misses, front-face and back-face hits on each of the
    three geometries, |d| from 0.5 to 2, barycentrics at corners, on edges and inside -- and per record its geometry, whether dot(n, d)
    > 0 for the shading normal (by a wide margin: every vertex normal of the triangle is within 50 degrees of +-d), and a = sigma x"""
    rng = np.random.default_rng(seed)
    tri_pos = mesh.triangle_positions().astype(np.float64)
    geom = np.repeat(np.arange(len(mesh.geometries)), mesh.prim_counts)
    M = np.eye(3) if matrix is None else np.asarray(matrix, np.float64)[:3, :3]
    prim = rng.integers(0, len(tri_pos), n)
    miss = rng.random(n) < 0.2
    fn = np.cross(tri_pos[prim, 1] - tri_pos[prim, 0], tri_pos[prim, 2] - tri_pos[prim, 0])
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    q = rng.normal(size=(n, 3))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    sign = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    d = (sign[:, None] * (fn + 0.2 * q)) @ M.T  # (object-space construction, taken to the world: the matrix keeps angles)
    d *= (rng.uniform(0.5, 2.0, n) / np.linalg.norm(d, axis=1))[:, None]
    uv = np.array(CORNERS)[rng.integers(0, len(CORNERS), n)]
    inner = rng.random(n) < 0.3
    uv[inner] = rng.dirichlet([1, 1, 1], int(inner.sum()))[:, :2]
    t = rng.uniform(0.05, 3.0, n)
    T = rng.uniform(0.1, 1.2, (n, 3))
    rec = np.zeros((n, 10), np.uint32)
    rec[:, 0:3], rec[:, 3], rec[:, 4:6], rec[:, 7:10] = bits(d.astype(F)), bits(t.astype(F)), bits(uv.astype(F)), bits(T.astype(F))
    rec[:, 6] = np.where(miss, MISS, prim)
    # every vertex normal of the triangle against d, in float64: all on one side, far from perpendicular
    for k in np.flatnonzero(~miss):
        g = mesh.geometries[geom[prim[k]]]
        io, vo = int(g["index_offset"]), int(g["vertex_offset"])
        local = prim[k] - int(np.concatenate([[0], np.cumsum(mesh.prim_counts)])[geom[prim[k]]])
        vn = mesh.vertices[mesh.indices[io + 3 * local : io + 3 * local + 3].astype(np.int64) + vo, 3:6].astype(np.float64) @ M.T
        c = (vn @ d[k]) / (np.linalg.norm(vn, axis=1) * np.linalg.norm(d[k]))
        assert np.all(sign[k] * c > 0.6), (k, c)
    back = ~miss & (sign > 0)
    x = bits(rec[:, 3]).view(F).astype(np.float64) * np.linalg.norm(np.ascontiguousarray(rec[:, 0:3]).view(F).astype(np.float64), axis=1)
    return rec, np.where(miss, -1, geom[prim]), back, x


def check_queue(ctx, mesh, matrix, n, groups, seed):
    rec, g, back, x = queue(mesh, matrix, n, seed)
    got = ctx.selftest_absorb_queue(rec, groups)  # (the call fails if a ray, a hit or a word behind the queue's end changed)
    amber = mesh.names.index("amber")
    changes = back & (g == amber)
    T = np.ascontiguousarray(rec[:, 7:10]).view(F)
    assert np.array_equal(got[~changes], bits(T)[~changes]), "only back-face hits on the absorbing box change"
    sigma = np.asarray(VW.BODY_SIGMA, np.float64)
    if changes.any():
        a = sigma[None, :] * x[changes, None]
        want = T[changes].astype(np.float64) * np.exp(-a)
        rel = np.abs(got[changes].view(F).astype(np.float64) / want - 1.0)
        assert np.all(rel <= rule_bound(a)), float((rel / rule_bound(a)).max())
        assert np.array_equal(got[changes][:, 1], bits(T)[changes][:, 1])  # sigma.g = 0
        assert np.all(got[changes][:, 0] != bits(T)[changes][:, 0])
    return int(changes.sum()), [int(((g == k) & back).sum()) for k in range(3)], [int(((g == k) & ~back).sum()) for k in range(3)], int((g < 0).sum())


@pytest.fixture(scope="module")
def bodies_pt():
    mesh = VW.bodies()
    pt = glass_pt(mesh)
    assert pt.ctx.attenuation_info() == 1
    yield pt, mesh
    pt.close()


@pytest.mark.parametrize("groups", (1, 2))
@pytest.mark.parametrize("n", QUEUE_N)
def test_absorb_kernel_on_a_queue(bodies_pt, n, groups):
    """k_absorb (256 threads a workgroup) through self-test op 37: one and two workgroups, so that the grid-stride loop runs up to seven
    times and its last pass is partial"""
    pt, mesh = bodies_pt
    check_queue(pt.ctx, mesh, None, n, groups, seed=100 * n + groups)


def test_absorb_queue_covers_every_kind_of_record(bodies_pt):
    pt, mesh = bodies_pt
    changed, backs, fronts, misses = check_queue(pt.ctx, mesh, None, 1537, 2, seed=9)
    assert changed > 100 and min(backs) > 20 and min(fronts) > 20 and misses > 100


@pytest.mark.parametrize("mode", (0, 1))
def test_absorb_queue_under_an_instance_matrix(mode):
    """the three bodies under a rotation, a uniform scale and a translation: the normal goes through the geometry's matrix; instance
    mode 1 reads the same flattened tables"""
    mesh, M = VW.bodies(), VW.bodies_matrix()
    pt = make_pt(mesh, VW.WINDOW, instances=[(0, 3, M)], mode=mode)
    try:
        assert pt.ctx.attenuation_info() == 1
        for n, groups in ((513, 1), (1537, 2)):
            assert check_queue(pt.ctx, mesh, M, n, groups, seed=n + mode)[0] > 20
    finally:
        pt.close()


def test_absorb_queue_needs_a_table_and_known_primitives(bodies_pt):
    pt, mesh = bodies_pt
    rec = queue(mesh, None, 4, 1)[0]
    rec[2, 6] = mesh.n_triangles
    with pytest.raises(L.Rt3Error) as e:
        pt.ctx.selftest_absorb_queue(rec, 1)
    assert e.value.code == L.E_INVALID
    clear = make_pt(GW.slab_world()[0], VW.WINDOW)
    try:
        with pytest.raises(L.Rt3Error) as e:
            clear.ctx.selftest_absorb_queue(queue(mesh, None, 4, 1)[0] * 0, 1)
        assert e.value.code == L.E_STATE
    finally:
        clear.close()


# ---------------------------------------------------------------------------------------------------------------- 3 closed form A
def one_frame(mesh, flags, spp, bounces, setup=None, **kw):
    pt = glass_pt(mesh, **kw)
    try:
        if setup:
            setup(pt)
        return frame(pt, flags, spp, bounces, window=kw.get("window", VW.WINDOW))
    finally:
        pt.close()


def matched_band(mesh, n, S, window=VW.WINDOW):
    """(expected frame, frame with 1 / cos theta dropped, relative band per pixel and channel) of the index-matched absorbing slab.

    A pixel is SKY T with T = exp(-sigma x), x the length of the one internal segment.  Relative bounds, added:
      sky_bound(S): the sky's blend, the mean of S equal samples, the throughput's products with 1;
      rule_bound(a), a = sigma x: the rule itself;
      sigma dx: x is measured between two fp32 hit points.  p1 = o + t1 d is rounded twice per coordinate (product, sum) at magnitudes
        up to C, the scene's largest coordinate among the hit points: |dp1| <= 2 sqrt(3) C U, which moves the distance to the back face
        along d by at most |dp1| / cos theta.  The two distances t1 (camera to front face, at most t_max) and t2 = x carry the triangle
        test's roundings, at most 16 half-ulps each: t1's moves p1 along d, t2's is x's own.  dx <= (2 sqrt(3) C + 16 (t_max + x)) U / cos_min;
      8 a U: the camera's and the transmitted direction are fp32 (each component within 2 U), which turns d by at most 4 U and changes
        1 / cos theta by tan theta times that, tan theta < 2 in these views."""
    cos_i, t_front, t_back, C = VW.slab_geometry(mesh, n, window)
    x = t_back - t_front
    sigma = np.asarray(VW.SLAB_SIGMA, np.float64)
    a = sigma * x[..., None]
    dx = (2.0 * math.sqrt(3.0) * C + 16.0 * (t_front.max() + x.max())) * U / cos_i.min()
    band = sky_bound(S) + rule_bound(a) + sigma * dx + 8.0 * a * U
    return SKY * np.exp(-a), SKY * np.exp(-sigma * VW.THICKNESS) * np.ones_like(a), band


@pytest.mark.parametrize("tilt", (0.0, 35.0))
def test_index_matched_absorbing_slab(tilt):
    """closed form A.  ior 1: no reflection, no bending, every sample of a pixel is the same path -- through the front face, one internal
    segment that arrives at the back face's back, out into the sky.  matched_band derives the band; it is narrow enough that the frame
    with 1 / cos theta dropped lies more than two bands away in at least 90 % of the pixels (all of them under the tilt; without it the
    few pixels around the axis meet the slab too squarely to tell).  The slab covers the window: no pixel lies off it or near its
    outline (volume_worlds.slab_outline_share, checked on the CPU too)."""
    S = 4
    mesh, n, centre = VW.slab_world(ior=1.0, tilt_deg=tilt)
    on, near = VW.slab_outline_share(n, centre)
    assert on == 1.0 and near <= 0.10
    want, dropped, band = matched_band(mesh, n, S)
    got = one_frame(mesh, L.F_NEE_SKY, S, 4).astype(np.float64)
    rel = np.abs(got / want - 1.0)
    print(f"matched slab tilt {tilt}: worst deviation {np.max(rel / band):.3f} bands, {rel.max() / U:.1f} U (bands {band.min() / U:.0f} .. {band.max() / U:.0f} U)")
    assert np.all(rel <= band)
    far = np.abs(dropped / want - 1.0) > 2.0 * band
    print(f"matched slab tilt {tilt}: 1 / cos dropped is more than two bands away in {far.mean():.1%} of the pixel-channels")
    assert far.mean() >= 0.9 and (tilt == 0.0 or far.all())


# ---------------------------------------------------------------------------------------------------------------- 4 closed form B
def test_absorbing_slab_with_inter_reflections():
    """closed form B, ior 1.5, B = 8, S = 1024, NEE_SKY under a constant sky: a sample is SKY times the path's throughput when the path
    leaves the slab on either side, 0 when it is still inside at its last vertex; summed over all numbers of internal segments a pixel's
    expectation is SKY (R + T), R = F + (1 - F)^2 F a^2 / (1 - F^2 a^2), T = (1 - F)^2 a / (1 - F^2 a^2), a = exp(-sigma thickness / cos
    theta_t).  Stopping at B vertices costs at most (1 - F) (F a)^(B - 1).  Every sample lies in [0, SKY], so the mean over a row's n
    pixels and S samples lies within 5 SKY / (2 sqrt(n S)) of its expectation, plus the tail, plus sky_bound(S).  The band tells the
    series from the one that attenuates a single internal segment (a^2 -> 1): the two are more than two bands apart in every row."""
    S, B = 1024, 8
    mesh, n, centre = VW.slab_world()
    got = one_frame(mesh, L.F_NEE_SKY, S, B).astype(np.float64)
    cos_i = VW.slab_geometry(mesh, n)[0]
    R, T = RV.slab_R_T(VW.SLAB_SIGMA, VW.THICKNESS, cos_i, GW.IOR)
    R1, T1 = RV.slab_R_T(VW.SLAB_SIGMA, VW.THICKNESS, cos_i, GW.IOR, single_segment=True)
    tail = RV.slab_tail(VW.SLAB_SIGMA, VW.THICKNESS, cos_i, GW.IOR, B)
    assert np.all(got >= 0.0) and np.all(got <= SKY * (1.0 + sky_bound(S)))
    worst = 0.0
    H, W = cos_i.shape
    for y in range(H):
        want, wrong = SKY * (R[y] + T[y]).mean(0), SKY * (R1[y] + T1[y]).mean(0)
        band = 5.0 * SKY / (2.0 * math.sqrt(W * S)) + SKY * tail[y].max(0) + sky_bound(S) * SKY
        dev = np.abs(got[y].mean(0) - want)
        worst = max(worst, float((dev / band).max()))
        assert np.all(dev <= band), (y, dev, band)
        assert np.all(np.abs(want - wrong) > 2.0 * band), (y, want, wrong, band)
    print(f"absorbing slab: worst deviation {worst:.2f} bands over {H} rows")


# ---------------------------------------------------------------------------------------------------------------- 5 nothing changes without it
def quiet_tables(mesh):
    """(every sigma 0, sigma > 0 on every geometry that is thin-walled or does not transmit)"""
    tr = mesh.transmission
    idle = assets.no_attenuation(len(mesh.geometries))
    idle["sigma"][(tr["transmission"] == 0) | (tr["thin_walled"] == 1)] = (2.0, 0.5, 1.0)
    assert idle["sigma"].any() and not (idle["sigma"].any(1) & (tr["transmission"] > 0) & (tr["thin_walled"] == 0)).any()
    return assets.no_attenuation(len(mesh.geometries)), idle


@pytest.mark.parametrize("world", ("glass_room", "sealed"))
def test_nothing_changes_without_an_absorbing_geometry(world):
    mesh, cam, window, sky = {"glass_room": (GW.glass_room(True, 0.5), IW.ROOM_CAMERA, IW.WINDOW_ROOM, IW.room_sky()),
                              "sealed": (GW.sealed_world(emissive=True)[0], GW.SEALED_CAMERA, GW.WINDOW, LW.constant_sky(GW.SKY_L))}[world]
    pt = make_pt(mesh, window, sky=sky)
    try:
        pt.set_lens(0.0, 1.0, 1.0)
        shot = lambda: frame(pt, FULL | L.F_NEE_EMISSIVE, 4, 5, window=window, cam=cam)
        plain = shot()
        assert pt.ctx.attenuation_info() == 0 and plain.max() > 0.0
        for table in quiet_tables(mesh):
            pt.ctx.set_attenuation(table)
            pt.ctx.build_accel()
            assert pt.ctx.attenuation_info() == 0
            assert np.array_equal(bits(shot()), bits(plain))
    finally:
        pt.close()


# ---------------------------------------------------------------------------------------------------------------- 6 the fixture
def room_frames(name, mode=0):
    flags, bounces, specular, tau, _, _, frames = VW.ROOM_CASES[name]
    pt = make_pt(VW.absorbing_room(specular, tau), IW.WINDOW_ROOM, sky=IW.room_sky(), mode=mode)
    try:
        assert pt.ctx.attenuation_info() == 2
        pt.set_lens(*VW.ROOM_LENS)
        cam = camera(IW.ROOM_CAMERA, IW.WINDOW_ROOM)
        out = []
        for k in range(frames):
            pt.render(pt.make_gconst(cam, IW.FRAME_SPP, bounces, frame=k, flags=flags))
            out.append(pt.light()[..., :3].copy())
        return np.stack(out)
    finally:
        pt.close()


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("name", sorted(VW.ROOM_CASES))
def test_gpu_against_fixture(name, mode):
    W, H = IW.WINDOW_ROOM
    check_against_fixture(room_frames(name, mode), np.ones((H, W), bool), fixture(), name)


# ---------------------------------------------------------------------------------------------------------------- 7 plumbing
def room_frame(window=IW.WINDOW_ROOM, flags=FULL | L.F_NEE_EMISSIVE, spp=4, setup=None, **kw):
    pt = make_pt(VW.absorbing_room(True, 0.5), window, sky=IW.room_sky(), **kw)
    try:
        pt.set_lens(0.05, 6.0, 1.0)
        if setup:
            setup(pt)
        return frame(pt, flags, spp, 6, window=window, cam=IW.ROOM_CAMERA)
    finally:
        pt.close()


def test_same_bits_for_every_batch_size_and_instance_mode():
    whole = room_frame()
    assert whole.max() > 0.0
    assert np.array_equal(bits(whole), bits(room_frame(setup=lambda pt: pt.ctx.set_option(L.OPT_BATCH_SPP, 1))))
    assert np.array_equal(bits(whole), bits(room_frame(mode=1)))

    def clear(pt):
        pt.ctx.set_attenuation([])
        pt.ctx.build_accel()
    assert not np.array_equal(bits(whole), bits(room_frame(setup=clear))), "the room's absorption shows"


def test_two_ranks_stitch_to_one():
    W, H = window = (128, 48)
    whole = room_frame(window)
    for r in range(2):
        part = room_frame(window, rank=r, n_ranks=2)
        m = owned_mask(W, H, r, 2)
        assert m.any() and not m.all()
        assert np.array_equal(bits(part[m]), bits(whole[m]))


@pytest.mark.parametrize("window", ((60, 44), (8, 8)))
def test_windows_that_do_not_fill_their_last_block(window):
    """60 x 44 at 1 spp: 2640 paths, ten workgroups of k_absorb and a part of one; 8 x 8: 64 paths, a quarter of one.  The room keeps its
    bits from one batch size to the other, and the index-matched slab meets its closed form"""
    assert np.array_equal(bits(room_frame(window, spp=2)), bits(room_frame(window, spp=2, setup=lambda pt: pt.ctx.set_option(L.OPT_BATCH_SPP, 1))))
    mesh, n, _ = VW.slab_world(ior=1.0, tilt_deg=35.0)
    want, _, band = matched_band(mesh, n, 1, window)
    got = one_frame(mesh, L.F_NEE_SKY, 1, 4, window=window).astype(np.float64)
    assert got.shape[:2] == window[::-1] and np.all(np.abs(got / want - 1.0) <= band)


# ---------------------------------------------------------------------------------------------------------------- 8 roulette, adaptive
def test_roulette_decides_on_the_attenuated_throughput():
    """The index-matched slab with roulette from vertex 0, floor 1/16, S = 16, B = 4.  A sample's path: vertex 0 on the front face
    (T = 1: survives undrawn), the internal segment, vertex 1 on the back face with T = exp(-sigma x) as k_absorb left it, whose
    extension ray k_roulette tests with q = max T = T.r (above the floor), q_g = ceil(q 2^23) 2^-23, and u = ref_roulette.roulette_u(pixel,
    frame, sample, B, 1): the survivor escapes into the sky with T / q_g.  So a pixel is k / S times SKY T / q_g, k the number of its
    samples with u < q_g -- inside the band of closed form A plus the division's and one more mean's roundings (4 U).  T.r is known to
    the band only, so a pixel one of whose draws lies within the band of q is left out: under 2 % of them."""
    S, B, frame_no = 16, 4, 3
    mesh, n, _ = VW.slab_world(ior=1.0, tilt_deg=35.0)
    want, _, band = matched_band(mesh, n, S)
    T = want / SKY
    q = T[..., 0]
    assert q.min() > 1.0 / 16.0 and q.max() < 1.0
    H, W = q.shape
    py, px = np.mgrid[0:H, 0:W]
    u = np.stack([RR.roulette_u(px.reshape(-1), py.reshape(-1), frame_no, s, B, 1).reshape(H, W) for s in range(S)]).astype(np.float64)
    margin = q * band[..., 0] + 2.0**-23
    open_ = (np.abs(u - q) <= margin).any(0)
    k = (u < q).sum(0)
    print(f"roulette on the slab: {open_.mean():.2%} of the pixels open; survivors per pixel {k.min()} .. {k.max()} of {S}")
    assert open_.mean() < 0.02 and k.min() < S
    pt = glass_pt(mesh)
    try:
        pt.set_roulette(0, 1.0 / 16.0)
        got = frame(pt, L.F_NEE_SKY, S, B, index=frame_no).astype(np.float64)
        tested, ended = pt.roulette_info()
    finally:
        pt.close()
    expect = (k / S)[..., None] * want / q[..., None]
    ok = ~open_ & (k > 0)
    assert np.all(np.abs(got[ok] / expect[ok] - 1.0) <= band[ok] + 4.0 * U)
    assert not got[~open_ & (k == 0)].any()
    assert ended >= int((S - k)[~open_].sum()) and tested > ended


def test_adaptive_pixels_hold_the_fixed_frames_bits():
    """coverage mode over the absorbing room (world B of adaptive_lens_worlds with the room's absorption): a pixel that stopped at n holds
    the bits of the fixed frame at samples = n, and the absorption shows in them"""
    w = LensWorld(alw.B, VW.absorbing_room(), IW.room_sky())
    try:
        assert w.pt.ctx.attenuation_info() == 2
        light, moments, info, _ = w.adaptive()
        n = check_against_fixed(w, light, moments, everything(w))
        assert len(set(n.reshape(-1).tolist())) > 1
        w.pt.ctx.set_attenuation([])
        w.pt.ctx.build_accel()
        w.cache.clear()
        assert not np.array_equal(bits(w.fixed(alw.MIN_SAMPLES)), bits(light)) and w.pt.ctx.attenuation_info() == 0
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------------------------- 9 the contract
BAD_TABLES = {"negative sigma": (0, -0.5), "sigma NaN": (1, np.nan), "sigma inf": (2, np.inf), "reserved": ("reserved", 1)}


def test_contract_of_the_new_call():
    mesh, n, _ = VW.slab_world(ior=1.0)
    pt = glass_pt(mesh)
    try:
        ctx = pt.ctx
        shot = lambda: frame(pt, L.F_NEE_SKY, 4, 4)
        before = shot()
        assert ctx.attenuation_info() == 2
        # refusals change nothing: the structure stays usable and the frame keeps its bits
        for what, (key, value) in BAD_TABLES.items():
            t = mesh.attenuation.copy()
            if key == "reserved":
                t["reserved"][1] = value
            else:
                t["sigma"][1, key] = value
            with pytest.raises(L.Rt3Error) as e:
                ctx.set_attenuation(t)
            assert e.value.code == L.E_INVALID, what
        for k in (1, 3):
            with pytest.raises(L.Rt3Error) as e:
                ctx.set_attenuation(assets.no_attenuation(k))
            assert e.value.code == L.E_INVALID
        assert np.array_equal(bits(shot()), bits(before)) and ctx.attenuation_info() == 2
        # an accepted table takes effect at the next build; until then the structure is unusable
        ctx.set_attenuation(mesh.attenuation)
        with pytest.raises(L.Rt3Error) as e:
            shot()
        assert e.value.code == L.E_STATE
        with pytest.raises(L.Rt3Error) as e:
            ctx.attenuation_info()
        assert e.value.code == L.E_STATE
        ctx.build_accel()
        assert np.array_equal(bits(shot()), bits(before))
        # a refit keeps the table
        ctx.update_vertices(mesh.vertices, 0)
        ctx.refit_accel()
        assert ctx.attenuation_info() == 2 and np.array_equal(bits(shot()), bits(before))
        # n = 0 clears: the slab is clear glass, index-matched, and shows the sky
        ctx.set_attenuation([])
        ctx.build_accel()
        clear = shot()
        assert ctx.attenuation_info() == 0 and np.abs(clear.astype(np.float64) / SKY - 1.0).max() <= sky_bound(4)
        # rt3_scene_set_geometry resets the table too
        ctx.set_attenuation(mesh.attenuation)
        ctx.upload_mesh(assets.Mesh(mesh.vertices, mesh.indices, mesh.geometries, mesh.prim_counts, list(mesh.names), transmission=mesh.transmission))
        ctx.build_accel()
        assert ctx.attenuation_info() == 0 and np.array_equal(bits(shot()), bits(clear))
        # and a mesh with the table brings it back through upload_mesh
        ctx.upload_mesh(mesh)
        ctx.build_accel()
        assert ctx.attenuation_info() == 2 and np.array_equal(bits(shot()), bits(before))
    finally:
        pt.close()


def test_the_scene_function_absorbs():
    from raytracer3_amd import scenes
    from raytracer3_amd.renderer import PathTracer

    pt = PathTracer((64, 48))
    try:
        pt.set_scene(scenes.amber_cornell())
        assert pt.ctx.attenuation_info() == 3 and pt.ctx.get_lens()[1]
        amber = frame(pt, L.F_NEE_EMISSIVE | L.F_FACEFORWARD, 8, 6, cam=scenes.CORNELL_CAMERA)
        pt.set_scene(scenes.amber_cornell(absorb=False))
        assert pt.ctx.attenuation_info() == 0
        clear = frame(pt, L.F_NEE_EMISSIVE | L.F_FACEFORWARD, 8, 6, cam=scenes.CORNELL_CAMERA)
        assert np.isfinite(amber).all() and amber.mean() < clear.mean() and np.all(amber <= clear * (1.0 + 16 * U))
    finally:
        pt.close()
