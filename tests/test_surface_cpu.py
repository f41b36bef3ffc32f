"""The surface stage (hit_info) against its float64 restatement (tests/ref_surface.py), on a world built to reach its edges
(tests/surface_worlds.py): first and last triangles of geometries of different sizes, textures of 1 x 1, 1 x 7, 3 x 5, 64 x 64 and 257 x 2
texels, uvs on texel centres, edges and the seam, negative and several periods out, and instances under the identity, a rotation, a
non-uniform scale and a mirror.  The frame tests compare the device with the oracle, which shares its author; these checks compare the rule
both implement with float64, within the two derived bounds of ref_surface.  They take a backend (the oracle here; the device, compared with
the oracle bit for bit first, in test_surface.py).

Also here, on the CPU: the premise of the table-size tests of test_shade_tables.py -- placing a geometry of zero triangles changes no
pixel of the oracle's frame, wherever the empty entry sits in the flattened table."""
import numpy as np
import pytest

import orc
import ref_surface as R
import surface_worlds as SW
from raytracer3_amd import assets, scenes


class Oracle:
    name = "oracle"

    def __init__(self, mesh, instances):
        self.scene = orc.Scene(mesh, instances=instances, build=False)

    def hit_info(self, prim, bu, bv):
        return self.scene.hit_info(prim, bu, bv)


@pytest.fixture(scope="module")
def world():
    """(mesh, instances, (prim, bu, bv), float64 reference): made once, never modified"""
    mesh, instances = SW.surface_world()
    hits = SW.surface_hits(mesh, instances)
    return mesh, instances, hits, R.reference(mesh, instances, *hits)


@pytest.fixture(scope="module")
def backend(world):
    return Oracle(world[0], world[1])


# ------------------------------------------------------------------------------------------------ checks (shared with the GPU suite)
def check_world_reaches_the_edges(world):
    """the inputs cover what the module docstring says (so that a change of the generator cannot hollow the checks out)"""
    mesh, instances, (prim, bu, bv), ref = world
    geom, inst, first, counts, mats = R.flatten(mesh, instances)
    assert len(set(counts.tolist())) >= 7 and counts.max() <= 400
    assert set(first.tolist()) <= set(prim.tolist()) and set((first + counts - 1).tolist()) <= set(prim.tolist())  # first and last triangles
    n_tex = len(mesh.textures)
    tex = mesh.geometries["base_color_texture_index"]
    assert set(range(n_tex)) <= set(tex.tolist()) and -1 in tex and (tex >= n_tex).any()
    assert [(t.shape[1], t.shape[0]) for t in mesh.textures] == SW.TEXTURE_SIZES
    assert ref.textured.any() and (~ref.textured).any()
    identity = np.array([np.array_equal(m, R.IDENTITY) for m in mats])
    dets = np.array([np.linalg.det(m[:3, :3].astype(np.float64)) for m in mats])
    assert identity.any() and (dets < 0).any() and (np.abs(np.abs(dets[~identity]) - 1) < 1e-5).any()
    assert sorted(geom.tolist()).count(2) >= 3  # one geometry under several matrices
    uv = mesh.vertices[:, 6:8]
    assert (uv == 0).any() and (uv == 1).any() and (uv < 0).any() and (np.abs(uv) > 2).any() and np.signbit(uv[uv == 0]).any()
    corners = (bu.astype(np.float64) + bv == 1) | ((bu == 0) & (bv == 0))
    assert corners.any() and ((bu == 0.5) | (bv == 0.5)).any() and (~corners & (bu > 0) & (bv > 0)).sum() > 1000
    # the seam: in every texture wider than a texel, a hit whose left texel is the last column (x1 wraps to 0) inside [0, 1) and one outside
    for k, (w, h) in enumerate(SW.TEXTURE_SIZES):
        x0 = np.floor(ref.uv[ref.tex == k, 0] * w - 0.5)
        assert len(x0) and (w == 1 or ((x0 == w - 1).any() and (x0 == -1).any() and (np.mod(x0, w) == w - 1).sum() > 10)), (w, h)
    assert (mesh.geometries["emission"][:, :3] != 0).any(1).sum() >= 2


def check_normals(backend, world):
    """angle to the float64 normal within (sqrt(18) / 65535) kappa / L + 16 * 2^-23 kappa; unit length; returns the worst error / bound"""
    mesh, instances, hits, ref = world
    got = backend.hit_info(*hits)[:, 6:9].astype(np.float64)
    ln = np.linalg.norm(got, axis=1)
    assert np.abs(ln - 1.0).max() < 4e-7 * 2, np.abs(ln - 1.0).max()  # normalize in fp32: a few roundings of 2^-24
    err = R.angle(got / ln[:, None], ref.normal)
    ratio = err / ref.normal_bound
    bad = np.flatnonzero(ratio > 1.0)
    assert bad.size == 0, (bad[:8], hits[0][bad[:8]], err[bad[:8]], ref.normal_bound[bad[:8]])
    assert ratio.max() > 0.05  # the comparison saw the 16-bit quantisation, i.e. both sides really computed
    return float(ratio.max())


def check_albedo(backend, world):
    """textured albedo within 2^-23 (4 (max|u| W + max|v| H + 1) + 8) of float64, untextured albedo exact; returns the worst error / bound"""
    mesh, instances, hits, ref = world
    got = backend.hit_info(*hits)[:, 0:3]
    t = ref.textured
    assert np.array_equal(got[~t], ref.albedo[~t].astype(np.float32))  # a copy of base_color (float64 here holds the fp32 values)
    err = np.abs(got[t].astype(np.float64) - ref.albedo[t]).max(1)
    assert ref.albedo_bound[t].max() <= 2e-3
    ratio = err / ref.albedo_bound[t]
    bad = np.flatnonzero(ratio > 1.0)
    assert bad.size == 0, (bad[:8], hits[0][t][bad[:8]], err[bad[:8]], ref.albedo_bound[t][bad[:8]])
    assert ratio.max() > 0.0
    return float(ratio.max()), {f"{w}x{h}": float(err[ref.tex[t] == k].max()) for k, (w, h) in enumerate(SW.TEXTURE_SIZES)}


def check_material(backend, world):
    """emissive = emission * 12 within one fp32 rounding; roughness and metalness are copies"""
    mesh, instances, hits, ref = world
    got = backend.hit_info(*hits)
    assert (np.abs(got[:, 3:6].astype(np.float64) - ref.emissive) <= 2.0**-24 * np.abs(ref.emissive)).all()
    assert (ref.emissive != 0).any() and (ref.emissive == 0).all(1).any()
    assert np.array_equal(got[:, 9], ref.roughness) and np.array_equal(got[:, 10], ref.metalness)
    assert len(np.unique(got[:, 9])) == len(mesh.geometries)  # every material distinct: a neighbour's row would show


# ------------------------------------------------------------------------------------------------ the oracle
def test_world_reaches_the_edges(world):
    check_world_reaches_the_edges(world)


def test_normals_match_float64(backend, world):
    print(f"hit_info normals ({backend.name}): worst error / bound {check_normals(backend, world):.3f}")


def test_albedo_matches_float64(backend, world):
    worst, by_size = check_albedo(backend, world)
    print(f"hit_info albedo ({backend.name}): worst error / bound {worst:.3f}; worst error by texture size {by_size}")


def test_material_fields_match(backend, world):
    check_material(backend, world)


def test_octahedral_step_bound():
    """the first term of the normal bound on its own: 200 000 random normals through the oracle's 16-bit round trip turn by less than
    sqrt(18) / 65535 rad"""
    L = orc.lib()
    rng = np.random.default_rng(4)
    n = rng.normal(size=(200_000, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    out = np.zeros_like(n)
    for i in range(len(n)):
        L.orc_octa_decode16(L.orc_octa_encode16(n[i].ctypes.data), out[i].ctypes.data)
    a = n.astype(np.float64)
    b = out.astype(np.float64)
    err = R.angle(a / np.linalg.norm(a, axis=1, keepdims=True), b / np.linalg.norm(b, axis=1, keepdims=True))
    assert 0.5 * R.OCTA_STEP < err.max() <= R.OCTA_STEP, err.max()


# ------------------------------------------------------------------------------------------------ premise of test_shade_tables.py
def oracle_frame(mesh, instances, camera, sky, bn, flags, W=64, H=48, spp=4, bounces=3):
    osc = orc.Scene(mesh, sky, bn, instances=instances)
    g = orc.camera_gconst(camera["position"], camera["direction"], camera["fov_deg"], W, H)
    g.bounces, g.samples, g.blendfactor, g.frame = bounces, spp, 1.0, 1
    g.pad[0] = flags
    gb, depth = osc.gbuffer(g)
    light, _ = osc.reference_mode(g, gb, depth)
    return light, gb, depth


@pytest.mark.parametrize("at", [None, 100], ids=["appended", "in the middle"])
def test_empty_geometry_leaves_the_oracles_frame_unchanged(at):
    """one zero-triangle geometry placed, last or in the middle of the instance list (every later table index shifts by one): the
    flattened table grows by one entry and no word of the frame or the G-buffer changes"""
    mesh, inst, cam = SW.many_geometries(256)
    sky, bn = scenes.sky(128, 64), assets.load_bluenoise()
    flags = orc.F_NEE_SKY | orc.F_BLUENOISE | orc.F_SPECULAR | orc.F_FACEFORWARD
    base = oracle_frame(mesh, inst, cam, sky, bn, flags)
    mesh1, inst1 = SW.with_empty_geometry(mesh, inst, at)
    assert len(R.flatten(mesh1, inst1)[0]) == len(R.flatten(mesh, inst)[0]) + 1 == 257
    if at is not None:
        assert R.flatten(mesh1, inst1)[0][at] == 256 and R.flatten(mesh1, inst1)[3][at] == 0
    plus = oracle_frame(mesh1, inst1, cam, sky, bn, flags)
    for a, b in zip(base, plus):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    light, _, depth = base
    assert light[..., :3].mean() > 0 and (depth != orc.BACKGROUND_DEPTH).mean() > 0.6
