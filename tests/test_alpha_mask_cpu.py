"""Alpha-masked cutout geometry (glTF alphaMode MASK) without a GPU: the glTF round trip of alphaMode / alphaCutoff /
baseColorFactor[3], the C++ loader against the Python one, and the numpy fp32 restatement of the device's tex_alpha (rt3_surface.hpp) that
the GPU tests pin bit for bit, checked here against float64."""
import json
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from raytracer3_amd import assets, scenes
from raytracer3_amd.assets import Material, MeshBuilder

ROOT = Path(__file__).resolve().parent.parent
TOOL = ROOT / "raytracer3_amd" / "host" / "asset_tool"

F = np.float32


# ------------------------------------------------------------------------------------------------ restatements of the device functions
def tex_alpha_f32(tex, u, v):
    """tex_alpha (rt3_surface.hpp) in fp32: texture_sample's texel coordinates, weights and association on byte * (1 / 255); tex (h, w, 4)
    uint8 or None (no texture: 1)"""
    u, v = np.asarray(u, F), np.asarray(v, F)
    if tex is None:
        return np.ones(np.broadcast(u, v).shape, F)
    H, W = tex.shape[:2]
    x, y = u * F(W) - F(0.5), v * F(H) - F(0.5)
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = x - xf, y - yf
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    x1, y1 = np.mod(x0 + 1, W), np.mod(y0 + 1, H)
    x0, y0 = np.mod(x0, W), np.mod(y0, H)
    a = tex[..., 3].astype(F) * (F(1.0) / F(255.0))
    one = F(1.0)
    top = a[y0, x0] * (one - fx) + a[y0, x1] * fx
    bot = a[y1, x0] * (one - fx) + a[y1, x1] * fx
    return (top * (one - fy) + bot * fy).astype(F)


def tex_alpha_f64(tex, u, v):
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    if tex is None:
        return np.ones(np.broadcast(u, v).shape)
    H, W = tex.shape[:2]
    x, y = u * W - 0.5, v * H - 0.5
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = x - xf, y - yf
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    x1, y1 = np.mod(x0 + 1, W), np.mod(y0 + 1, H)
    x0, y0 = np.mod(x0, W), np.mod(y0, H)
    a = tex[..., 3].astype(np.float64) / 255.0
    return (a[y0, x0] * (1 - fx) + a[y0, x1] * fx) * (1 - fy) + (a[y1, x0] * (1 - fx) + a[y1, x1] * fx) * fy


def texture_of(mesh, g):
    t = int(mesh.geometries["base_color_texture_index"][g])
    return mesh.textures[t] if 0 <= t < len(mesh.textures) else None


def tri_uvs(mesh):
    """(n_tris, 3, 2) float32 vertex uvs in global primitive order (the device's tri_uv) and (n_tris,) geometry of each primitive"""
    uv, geo = [], []
    for k, (g, cnt) in enumerate(zip(mesh.geometries, mesh.prim_counts)):
        io, vo = int(g["index_offset"]), int(g["vertex_offset"])
        idx = mesh.indices[io:io + 3 * int(cnt)].astype(np.int64) + vo
        uv.append(mesh.vertices[idx, 6:8].reshape(-1, 3, 2))
        geo.append(np.full(int(cnt), k, np.int64))
    return np.concatenate(uv).astype(F), np.concatenate(geo)


def alpha_f32(mesh, prim, bu, bv):
    """alpha = base_color[3] * tex_alpha at the uv hit_finish interpolates (b0 = 1 - u - v), fp32, per (prim, u, v)"""
    uvs, geo = tri_uvs(mesh)
    prim = np.asarray(prim, np.int64)
    bu, bv = np.asarray(bu, F), np.asarray(bv, F)
    b0 = F(1.0) - bu - bv
    t = uvs[prim]
    uu = t[:, 0, 0] * b0 + t[:, 1, 0] * bu + t[:, 2, 0] * bv
    vv = t[:, 0, 1] * b0 + t[:, 1, 1] * bu + t[:, 2, 1] * bv
    out = np.ones(len(prim), F)
    for g in np.unique(geo[prim]):
        s = geo[prim] == g
        out[s] = F(mesh.geometries["base_color"][g][3]) * tex_alpha_f32(texture_of(mesh, g), uu[s], vv[s])
    return out


# ------------------------------------------------------------------------------------------------ tests
def test_tex_alpha_fp32_matches_float64():
    mesh = scenes.cutout_cornell()
    rng = np.random.default_rng(5)
    for tex in mesh.textures:
        u, v = rng.uniform(-2.0, 3.0, 20000).astype(F), rng.uniform(-2.0, 3.0, 20000).astype(F)
        a32, a64 = tex_alpha_f32(tex, u, v), tex_alpha_f64(tex, u.astype(np.float64), v.astype(np.float64))
        # the fp32 texel coordinate u W - 0.5 carries one rounding of |x|'s ulp; the weights move by that much, alpha by at most as much
        x, y = np.abs(u * F(tex.shape[1])) + 1.0, np.abs(v * F(tex.shape[0])) + 1.0
        tol = (np.spacing(x.astype(F)) + np.spacing(y.astype(F))).astype(np.float64) + 8 * 2.0 ** -24
        assert (np.abs(a32 - a64) <= tol).all(), float(np.max(np.abs(a32 - a64) - tol))
        assert a32.min() >= 0.0 and a32.max() <= 1.0


def test_opaque_texture_gives_alpha_one():
    """an all-255 alpha channel is exactly 1 everywhere: such a geometry passes every cutoff in (0, 1], 1 included"""
    rng = np.random.default_rng(3)
    tex = np.full((7, 5, 4), 255, np.uint8)
    a = tex_alpha_f32(tex, rng.uniform(-4, 4, 50000), rng.uniform(-4, 4, 50000))
    assert (a == F(1.0)).all()


def _glb_doc(path):
    data = Path(path).read_bytes()
    ln, _ = struct.unpack_from("<I4s", data, 12)
    return json.loads(data[20:20 + ln].decode())


def _rewrite_materials(src, dst, edit):
    """the .glb at src with its materials passed through edit(list) (JSON chunk rewritten, binary chunk kept)"""
    data = Path(src).read_bytes()
    ln, _ = struct.unpack_from("<I4s", data, 12)
    doc = json.loads(data[20:20 + ln].decode())
    edit(doc["materials"])
    js = json.dumps(doc, separators=(",", ":")).encode()
    js += b" " * ((-len(js)) % 4)
    rest = data[20 + ln:]
    Path(dst).write_bytes(struct.pack("<4sII", b"glTF", 2, 12 + 8 + len(js) + len(rest)) + struct.pack("<I4s", len(js), b"JSON") + js + rest)


def test_gltf_round_trip_of_alpha_mode(tmp_path):
    mesh = scenes.cutout_cornell()
    p = tmp_path / "cut.glb"
    assets.write_glb(p, mesh)
    mats = _glb_doc(p)["materials"]
    for g, c in enumerate(mesh.alpha_cutoffs):
        if c > 0:
            assert mats[g]["alphaMode"] == "MASK" and np.float32(mats[g]["alphaCutoff"]) == c
        else:
            assert "alphaMode" not in mats[g]
    back = assets.load(p)
    assert np.array_equal(back.alpha_cutoffs, mesh.alpha_cutoffs)
    assert back.geometries.tobytes() == mesh.geometries.tobytes()  # base_color[3] (the veil's 0.6) included
    assert back.geometries["base_color"][mesh.names.index("veil")][3] == np.float32(0.6)

    def edit(ms):  # MASK without a cutoff -> 0.5; OPAQUE / BLEND -> 0 (BLEND is not supported and draws opaque)
        ms[0]["alphaMode"] = "MASK"
        ms[1]["alphaMode"], ms[1]["alphaCutoff"] = "OPAQUE", 0.7
        ms[2]["alphaMode"] = "BLEND"
        ms[3]["pbrMetallicRoughness"]["baseColorFactor"] = [0.5, 0.5, 0.5, 0.25]
    q = tmp_path / "edited.glb"
    _rewrite_materials(p, q, edit)
    e = assets.load(q)
    assert e.alpha_cutoffs[0] == np.float32(0.5) and e.alpha_cutoffs[1] == 0.0 and e.alpha_cutoffs[2] == 0.0
    assert e.geometries["base_color"][3][3] == np.float32(0.25)
    assert np.array_equal(e.alpha_cutoffs[4:], mesh.alpha_cutoffs[4:])


def test_material_sets_mesh_cutoffs():
    mb = MeshBuilder()
    quad = ([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], [[0, 0, 1]] * 4, [[0, 0], [1, 0], [1, 1], [0, 1]], [[0, 1, 2], [0, 2, 3]])
    mb.add("a", *quad, Material())
    mb.add("b", *quad, Material(alpha_cutoff=0.25, alpha=0.5))
    m = mb.build()
    assert m.alpha_cutoffs.dtype == np.float32 and list(m.alpha_cutoffs) == [0.0, 0.25]
    assert list(m.geometries["base_color"][:, 3]) == [1.0, 0.5]
    assert list(assets.Mesh(m.vertices, m.indices, m.geometries, m.prim_counts).alpha_cutoffs) == [0.0, 0.0]  # default: opaque


def test_host_loader_matches_python(tmp_path):
    if not TOOL.exists():
        try:
            subprocess.check_call(["make", "-C", str(TOOL.parent), "asset_tool"], stdout=subprocess.DEVNULL)
        except (OSError, subprocess.CalledProcessError):
            pytest.skip("asset_tool is not built")
    mesh = scenes.cutout_cornell()
    p = tmp_path / "cut.glb"
    assets.write_glb(p, mesh)

    def edit(ms):
        ms[0]["alphaMode"] = "MASK"  # the default cutoff
        ms[2]["alphaMode"] = "BLEND"
    q = tmp_path / "edited.glb"
    _rewrite_materials(p, q, edit)
    for f in (p, q):
        out = tmp_path / (f.stem + "_dump")
        out.mkdir()
        r = subprocess.run([str(TOOL), "glb", str(f), str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        py = assets.load(f)
        assert (out / "alpha_cutoffs.bin").read_bytes() == py.alpha_cutoffs.tobytes()
        assert (out / "geometries.bin").read_bytes() == py.geometries.tobytes()
