"""Material textures on the CPU: the float64 reference of tests/ref_materials.py checks itself against cases whose
answer is known; glTF carries the four fields through a write -> read round trip; the C++ loader reads the same table as the Python loader;
and the world of tests/material_worlds.py meets the conditions the reference's bounds need and reaches the cases it is meant to reach."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import material_worlds as MW
import ref_materials as RM
import ref_surface as R
from raytracer3_amd import assets, scenes
from raytracer3_amd.assets import Material, MeshBuilder
from support import constant

F = np.float32
HOST = Path(__file__).resolve().parent.parent / "raytracer3_amd" / "host"


@pytest.fixture(scope="module")
def world():
    """(mesh, instances, (prim, bu, bv), float64 reference): made once, never modified"""
    mesh, instances = MW.material_world()
    hits = MW.material_hits(mesh, instances)
    return mesh, instances, hits, RM.reference(mesh, instances, *hits)


def one_triangle(uv, normal=(0.0, 0.0, 1.0), textures=(), **material):
    """the triangle (0,0,0) (1,0,0) (0,1,0) (geometric normal +z) with the given uvs, one vertex normal and material fields"""
    mb = MeshBuilder()
    mb.add("t", [[0, 0, 0], [1, 0, 0], [0, 1, 0]], [normal] * 3, uv, [[0, 1, 2]], Material((0.5, 0.5, 0.5), 0.75, 0.5, (0.5, 0.25, 1.0), **material))
    mesh = mb.build()
    mesh.textures = [np.ascontiguousarray(t, np.uint8) for t in textures]
    return mesh


HITS = (np.zeros(5, np.uint32), np.array([0.0, 1.0, 0.0, 0.25, 0.3], F), np.array([0.0, 0.0, 1.0, 0.25, 0.6], F))
UV = [[0.1, 0.2], [1.7, -0.4], [-2.3, 0.9]]


# ------------------------------------------------------------------------------------------------ the reference against known answers
def test_constant_textures_fold_into_the_factors():
    mesh = one_triangle(UV, textures=[constant((9, 77, 200, 3)), constant((255, 255, 255, 0)), constant((0, 0, 0, 255))],
                        metallic_roughness_texture=0, emissive_texture=1)
    ref = RM.reference(mesh, [], *HITS)
    assert np.allclose(ref.roughness, 0.5 * 77 / 255, rtol=1e-15) and np.allclose(ref.metalness, 0.75 * 200 / 255, rtol=1e-15)
    assert np.allclose(ref.emissive, np.array([0.5, 0.25, 1.0]) * 12.0, rtol=1e-15)  # EOTF(255) = 1
    mesh.material_textures["emissive_texture"][0] = 2
    assert (RM.reference(mesh, [], *HITS).emissive == 0).all()
    plain = RM.reference(one_triangle(UV), [], *HITS)
    assert (plain.roughness == 0.5).all() and (plain.metalness == 0.75).all() and not plain.has_mr.any() and not plain.has_n.any()
    assert np.array_equal(plain.normal, plain.unmapped_normal)


@pytest.mark.parametrize("scale", [1.0, 0.5, 2.0])
def test_a_flat_texel_leaves_the_normal_and_a_tilted_one_tilts_it_by_the_expected_angle(scale):
    """(128, 128, 255): c = (1/255, 1/255, 1), a tilt of atan(s sqrt(2) / 255); (255, 128, 255): c = (1, 1/255, 1), towards +T"""
    flat = one_triangle([[0, 0], [1, 0], [0, 1]], textures=[constant((128, 128, 255, 255))], normal_texture=0, normal_scale=scale)
    ref = RM.reference(flat, [], *HITS)
    assert ref.has_n.all()
    assert np.allclose(R.angle(ref.normal, ref.unmapped_normal), math.atan(scale * math.sqrt(2.0) / 255.0), rtol=1e-12)
    steep = one_triangle([[0, 0], [1, 0], [0, 1]], textures=[constant((255, 128, 255, 255))], normal_texture=0, normal_scale=scale)
    n = RM.reference(steep, [], *HITS).normal
    want = np.array([scale, scale / 255.0, 1.0])  # u runs along +x, v along +y, h = +1: T = +x, b = +y
    assert np.allclose(n, want / np.linalg.norm(want), rtol=1e-12)


def test_handedness_flips_with_mirrored_uvs_and_with_normals_opposed_to_the_winding():
    tex = [constant((128, 255, 255, 255))]  # c = (~0, 1, 1): the tilt goes along the bitangent
    kw = dict(textures=tex, normal_texture=0, normal_scale=1.0)
    plain = RM.reference(one_triangle([[0, 0], [1, 0], [0, 1]], **kw), [], *HITS).normal
    mirrored = RM.reference(one_triangle([[0, 0], [-1, 0], [0, 1]], **kw), [], *HITS).normal  # u mirrored: T = -x, det < 0, h = -1
    opposed = RM.reference(one_triangle([[0, 0], [1, 0], [0, 1]], normal=(0.0, 0.0, -1.0), **kw), [], *HITS).normal
    assert (plain[:, 1] > 0.6).all() and (plain[:, 2] > 0.6).all()  # b = +y
    # mirrored u: T = -x and h = -1, so b = -cross(z, -x) = +y still: the map's v axis did not move; its u axis did
    assert (mirrored[:, 1] > 0.6).all() and np.allclose(mirrored[:, 0], -plain[:, 0], atol=1e-15)
    # normals against the winding: n = -z, T = +x, h = -1: b = -cross(-z, x) = +y; the result leans along +y, below the triangle
    assert (opposed[:, 1] > 0.6).all() and (opposed[:, 2] < -0.6).all()
    degenerate = RM.reference(one_triangle([[0.5, 0.5]] * 3, **kw), [], *HITS)
    assert degenerate.no_tangent.all() and not degenerate.has_n.any() and np.array_equal(degenerate.normal, degenerate.unmapped_normal)


def test_the_reference_refuses_inputs_outside_its_conditions():
    tex = [constant((128, 128, 100, 255))]  # B below 128: the mapped vector may be shorter than 0.5
    with pytest.raises(AssertionError):
        RM.reference(one_triangle([[0, 0], [1, 0], [0, 1]], textures=[constant((128, 128, 128, 255))], normal_texture=0, normal_scale=0.1), [], *HITS)
    with pytest.raises(AssertionError):
        RM.reference(one_triangle([[0, 0], [1, 0], [0, 1]], textures=tex, normal_texture=0, normal_scale=3.0), [], *HITS)
    with pytest.raises(AssertionError):  # a nearly cancelling uv determinant
        RM.reference(one_triangle([[0, 0], [1, 1], [2, 2.0000002]], textures=[constant((128, 128, 255, 255))], normal_texture=0), [], *HITS)


# ------------------------------------------------------------------------------------------------ glTF
def test_gltf_round_trip_keeps_the_material_textures(tmp_path):
    mesh = scenes.material_cornell()
    t = mesh.material_textures
    assert (t["metallic_roughness_texture"] >= 0).any() and (t["normal_texture"] >= 0).any() and (t["emissive_texture"] >= 0).any()
    assert (t["normal_scale"] != 1.0).any() and (t["normal_texture"] < 0).any()
    assets.write_glb(tmp_path / "m.glb", mesh)
    back = assets.load(tmp_path / "m.glb")
    assert back.material_textures.dtype == assets.MATERIAL_TEXTURES_DTYPE and back.material_textures.tobytes() == t.tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(back.textures, mesh.textures)) and len(back.textures) == 3
    assert back.geometries.tobytes() == mesh.geometries.tobytes()


def test_a_texture_on_another_uv_set_counts_as_absent(tmp_path):
    import json
    import struct

    mesh = scenes.material_cornell()
    assets.write_glb(tmp_path / "m.glb", mesh)
    data = (tmp_path / "m.glb").read_bytes()
    ln = struct.unpack_from("<I", data, 12)[0]
    doc = json.loads(data[20 : 20 + ln].decode())
    for m in doc["materials"]:
        if "normalTexture" in m:
            m["normalTexture"]["texCoord"] = 1
    js = json.dumps(doc, separators=(",", ":")).encode()
    js += b" " * ((-len(js)) % 4)
    rest = data[20 + ln :]
    (tmp_path / "n.glb").write_bytes(struct.pack("<4sII", b"glTF", 2, 20 + len(js) + len(rest)) + struct.pack("<I4s", len(js), b"JSON") + js + rest)
    back = assets.load(tmp_path / "n.glb")
    assert (back.material_textures["normal_texture"] == -1).all() and (back.material_textures["normal_scale"] != 1.0).any()
    assert np.array_equal(back.material_textures["metallic_roughness_texture"], mesh.material_textures["metallic_roughness_texture"])
    tool = native_tool()
    out = tmp_path / "dump"
    out.mkdir()
    subprocess.run([tool, "glb", str(tmp_path / "n.glb"), str(out)], check=True, capture_output=True)
    assert np.fromfile(out / "material_textures.bin", assets.MATERIAL_TEXTURES_DTYPE).tobytes() == back.material_textures.tobytes()


def native_tool():
    subprocess.check_call(["make", "-C", str(HOST), "asset_tool"], stdout=subprocess.DEVNULL)
    return str(HOST / "asset_tool")


def test_native_loader_reads_the_same_table(tmp_path):
    mesh = scenes.material_cornell()
    assets.write_glb(tmp_path / "m.glb", mesh)
    subprocess.run([native_tool(), "glb", str(tmp_path / "m.glb"), str(tmp_path)], check=True, capture_output=True)
    got = np.fromfile(tmp_path / "material_textures.bin", assets.MATERIAL_TEXTURES_DTYPE)
    want = assets.load(tmp_path / "m.glb").material_textures
    assert len(got) == len(mesh.geometries) and got.tobytes() == want.tobytes() == mesh.material_textures.tobytes()


# ------------------------------------------------------------------------------------------------ the world
def check_world(world):
    """the world reaches what the module docstring of material_worlds says (the reference itself has asserted its conditions)"""
    mesh, instances, (prim, bu, bv), ref = world
    t = mesh.material_textures
    n_tex = len(mesh.textures)
    combos = {(int(a >= 0), int(b >= 0), int(c >= 0)) for a, b, c in zip(t["metallic_roughness_texture"], t["normal_texture"], t["emissive_texture"])}
    assert len(combos) == 8
    for column in ("metallic_roughness_texture", "normal_texture", "emissive_texture"):
        used = {(mesh.textures[k].shape[1], mesh.textures[k].shape[0]) for k in t[column] if 0 <= k < n_tex}
        assert {(1, 1), (257, 2)} <= used and len(used) >= 4, (column, used)
        assert (t[column] >= n_tex).any()  # an index past the uploaded textures
    assert all((mesh.textures[k][..., 2] >= 192).all() for k in t["normal_texture"] if 0 <= k < n_tex)
    assert ((t["normal_scale"] >= 0.25) & (t["normal_scale"] <= 2.0)).all()
    assert ref.has_mr.sum() > 1000 and ref.has_n.sum() > 1000 and ref.has_e.sum() > 1000 and ref.no_tangent.sum() >= 10
    assert (~ref.has_mr & ~ref.has_n & ~ref.has_e).sum() > 500
    geom, inst, first, counts, mats = R.flatten(mesh, instances)
    dets = np.array([np.linalg.det(m[:3, :3].astype(np.float64)) for m in mats])
    sv = [np.linalg.svd(m[:3, :3].astype(np.float64), compute_uv=False) for m in mats]
    assert (dets < 0).any() and max(s[0] / s[-1] for s in sv) > 5 and any(np.array_equal(m, R.IDENTITY) for m in mats)
    assert set(first.tolist()) <= set(prim.tolist()) and set((first + counts - 1).tolist()) <= set(prim.tolist())
    # mirrored uvs and normals opposed to the winding both occur among the normal-mapped triangles
    v = mesh.vertices.reshape(-1, 3, 8).astype(np.float64)
    det = (v[:, 1, 6] - v[:, 0, 6]) * (v[:, 2, 7] - v[:, 0, 7]) - (v[:, 2, 6] - v[:, 0, 6]) * (v[:, 1, 7] - v[:, 0, 7])
    facing = (np.cross(v[:, 1, :3] - v[:, 0, :3], v[:, 2, :3] - v[:, 0, :3]) * v[:, :, 3:6].sum(1)).sum(1)
    assert (det > 0).sum() > 50 and (det < 0).sum() > 50 and (facing > 0).sum() > 50 and (facing < 0).sum() > 50
    # discrimination: on at least 99 % of the normal-mapped hits the un-mapped normal lies outside the bound
    away = R.angle(ref.unmapped_normal[ref.has_n], ref.normal[ref.has_n]) > ref.normal_bound[ref.has_n]
    assert away.mean() >= 0.99, away.mean()
    # the bounds stay small against what they bound: kappa 10, a 257-texel axis at |u| <= 5 (d_tex 6.2e-4), |s| <= 2, |c'| >= 0.5
    assert ref.normal_bound.max() < 0.1 and np.median(ref.normal_bound[ref.has_n]) < 5e-3 and ref.mr_bound.max() <= 2e-3


def test_world_meets_the_conditions_and_reaches_the_cases(world):
    check_world(world)


def test_the_tilt_is_rarely_small():
    """the premise of the discrimination condition: with uniform random texels (B >= 192) and scales in [0.25, 2] the tilt is below
    1e-2 rad on under 0.3 % of 2 M samples"""
    rng = np.random.default_rng(5)
    n = 2_000_000
    c = 2.0 * rng.integers(0, 256, (n, 3)) / 255.0 - 1.0
    c[:, 2] = 2.0 * rng.integers(192, 256, n) / 255.0 - 1.0
    s = rng.uniform(0.25, 2.0, n)
    tilt = np.arctan2(s * np.hypot(c[:, 0], c[:, 1]), c[:, 2])
    assert (tilt < 1e-2).mean() < 0.003
