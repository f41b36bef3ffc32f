"""Asset IO for the path tracer: binary glTF (.glb) meshes, scanline EXR skies, the blue-noise PNG.

Mirrors the *shape* of the reference loader API (`GltfMeshLoader` -> `MeshTransformer` -> `Mesh{vertices, indices,
materials}`, /root/reference/src/assets/mod.rs:118-133,179-286) without its limitations: every mesh x primitive x node
transform is loaded (the reference reads only the first primitive of the first mesh, assets/mod.rs:221), roughness is
read from the roughness factor (the reference decodes it from the metallic bytes, :88,110), and indices stay u32
(the reference's `indices: Vec<u8>` are meshlet-local and unusable for ray tracing).  Meshlet building and the bincode
cache are raster-/bevy-specific and out of scope.

`Vertex` layout == assets/mod.rs:127-133: p[3] n[3] t[2], 32 bytes, interleaved float32.
`GeometryInfo` layout == shaders/include/datatypes.slang:11-19 padded to 64 bytes (include/rt3.h: rt3_geometry_info).
"""
from __future__ import annotations

import json
import math
import struct
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

GEOMETRY_DTYPE = np.dtype(
    [
        ("base_color", "<f4", (4,)),
        ("base_color_texture_index", "<i4"),
        ("metallic_factor", "<f4"),
        ("index_offset", "<u4"),
        ("vertex_offset", "<u4"),
        ("emission", "<f4", (4,)),
        ("roughness", "<f4"),
        ("_pad", "<u4", (3,)),
    ]
)
assert GEOMETRY_DTYPE.itemsize == 64
# rt3_material_textures (include/rt3.h): texture indices into Mesh.textures, -1 = none
MATERIAL_TEXTURES_DTYPE = np.dtype(
    [("metallic_roughness_texture", "<i4"), ("normal_texture", "<i4"), ("emissive_texture", "<i4"), ("normal_scale", "<f4")]
)
assert MATERIAL_TEXTURES_DTYPE.itemsize == 16
# rt3_transmission (include/rt3.h): glass per geometry
TRANSMISSION_DTYPE = np.dtype([("transmission", "<f4"), ("ior", "<f4"), ("thin_walled", "<u4"), ("reserved", "<u4")])
assert TRANSMISSION_DTYPE.itemsize == 16
# rt3_attenuation (include/rt3.h): absorption coefficients of solid glass per geometry
ATTENUATION_DTYPE = np.dtype([("sigma", "<f4", (3,)), ("reserved", "<u4")])
assert ATTENUATION_DTYPE.itemsize == 16
FLT_MIN = 1.1754943508222875e-38  # the smallest normal float32: the floor of an attenuation colour's component
# rt3_punctual_light (include/rt3.h): a point, spot or directional light of KHR_lights_punctual, in world space
LIGHT_POINT, LIGHT_SPOT, LIGHT_DIRECTIONAL = 0, 1, 2
LIGHT_DTYPE = np.dtype(
    [
        ("type", "<u4"),
        ("range", "<f4"),  # <= 0: unlimited
        ("inner_cone", "<f4"),
        ("outer_cone", "<f4"),
        ("position", "<f4", (3,)),
        ("_pad0", "<f4"),
        ("direction", "<f4", (3,)),  # the way the light shines
        ("_pad1", "<f4"),
        ("intensity", "<f4", (3,)),  # colour x intensity: W/sr (point, spot), W/m^2 (directional)
        ("_pad2", "<f4"),
    ]
)
assert LIGHT_DTYPE.itemsize == 64


def make_light(type, intensity, position=(0, 0, 0), direction=(0, 0, -1), range=0.0, inner_cone=0.0, outer_cone=math.pi / 4):
    """one LIGHT_DTYPE record"""
    l = np.zeros((), LIGHT_DTYPE)
    l["type"], l["range"], l["inner_cone"], l["outer_cone"] = type, range, inner_cone, outer_cone
    l["position"], l["direction"], l["intensity"] = position, direction, intensity
    return l


def lights_array(records) -> np.ndarray:
    """(l,) LIGHT_DTYPE from a sequence of make_light records"""
    out = np.zeros(len(records), LIGHT_DTYPE)
    for k, r in enumerate(records):
        out[k] = r
    return out


def no_material_textures(n: int) -> np.ndarray:
    """n entries of MATERIAL_TEXTURES_DTYPE that name no texture (normal_scale 1)"""
    t = np.zeros(n, MATERIAL_TEXTURES_DTYPE)
    t["metallic_roughness_texture"] = t["normal_texture"] = t["emissive_texture"] = -1
    t["normal_scale"] = 1.0
    return t


def no_transmission(n: int) -> np.ndarray:
    """n entries of TRANSMISSION_DTYPE without glass: what a glTF material without the transmission, ior and volume extensions is
    (transmission 0, ior 1.5, thin-walled)"""
    t = np.zeros(n, TRANSMISSION_DTYPE)
    t["ior"], t["thin_walled"] = 1.5, 1
    return t


def attenuation_sigma(color, distance) -> np.ndarray:
    """(3,) float32 absorption coefficients of KHR_materials_volume's attenuationColor / attenuationDistance:
    sigma = -ln(max(c, FLT_MIN)) / distance, in float64, rounded once to float32; an infinite distance gives 0.  (A component above 1 would
    amplify: it counts as 1.)"""
    c = np.minimum(np.maximum(np.asarray(color, np.float64).reshape(3), FLT_MIN), 1.0)
    d = float(distance)
    if not d > 0.0:
        raise ValueError("attenuationDistance must be > 0")
    if math.isinf(d):
        return np.zeros(3, np.float32)
    # (math.log: the C library's, as host/assets.hpp calls it; + 0.0: no negative zero)
    return np.array([-math.log(float(x)) / d + 0.0 for x in c], np.float64).astype(np.float32)


def no_attenuation(n: int) -> np.ndarray:
    """n entries of ATTENUATION_DTYPE that absorb nothing: what a glTF material without attenuationColor / attenuationDistance is"""
    return np.zeros(n, ATTENUATION_DTYPE)


@dataclass
class Material:
    """assets/mod.rs:52-59 (f16 fields there; plain floats here) + emission (datatypes.slang:17)."""

    color: tuple = (0.8, 0.8, 0.8)
    metalic_factor: float = 0.0
    roughness_factor: float = 1.0
    emission: tuple = (0.0, 0.0, 0.0)
    texture_offset: int = -1
    alpha_cutoff: float = 0.0  # glTF alphaMode MASK: alphaCutoff (0 = opaque)
    alpha: float = 1.0  # baseColorFactor[3] -> GeometryInfo.base_color[3]
    # material textures: indices into Mesh.textures, -1 = none
    metallic_roughness_texture: int = -1  # G = roughness, B = metalness, linear
    normal_texture: int = -1  # tangent-space normal map, linear
    emissive_texture: int = -1  # sRGB-encoded colour
    normal_scale: float = 1.0  # glTF normalTexture.scale
    # glass: KHR_materials_transmission, _ior, _volume
    transmission: float = 0.0  # transmissionFactor
    ior: float = 1.5
    thin_walled: int = 1  # 0 = solid: the material has a volume (thicknessFactor > 0)
    # absorbing glass: KHR_materials_volume's attenuationColor / attenuationDistance (attenuation_sigma)
    attenuation_color: tuple = (1.0, 1.0, 1.0)
    attenuation_distance: float = math.inf


SKIN_MAX_TARGETS, SKIN_MAX_JOINTS = 8, 65536  # RT3_SKIN_MAX_TARGETS; joint indices are uint16


@dataclass
class Skin:
    """One skinned and / or morphed primitive (rt3_skin_desc): the vertex range it owns and what a pose needs.  The rest
    records are in bind space: the accessors' own values, without the mesh node's matrix, as glTF prescribes for a skinned mesh.  A morphed
    primitive without a glTF skin is bound with weight 1 to one joint, its own node, under an identity inverse bind matrix."""

    first_vertex: int
    rest: np.ndarray  # (n, 8) float32  p n t
    joints: np.ndarray  # (n, 4) uint16, indices into joint_nodes
    weights: np.ndarray  # (n, 4) float32
    joint_nodes: list  # indices into Rig.nodes
    inverse_bind: np.ndarray  # (n_joints, 4, 4) float32, acting on column vectors
    target_dpos: np.ndarray = None  # (n_targets, n, 3) float32; None -> no targets
    target_dnrm: np.ndarray = None  # same shape, or None: normals are not morphed
    default_weights: np.ndarray = None  # (n_targets,) float32: the mesh's (or its node's) `weights`
    geometry: int = -1  # the geometry of Mesh.geometries it deforms

    def __post_init__(self):
        self.rest = np.ascontiguousarray(self.rest, np.float32).reshape(-1, 8)
        n = len(self.rest)
        self.joints = np.ascontiguousarray(self.joints, np.uint16).reshape(n, 4)
        self.weights = np.ascontiguousarray(self.weights, np.float32).reshape(n, 4)
        self.inverse_bind = np.ascontiguousarray(self.inverse_bind, np.float32).reshape(len(self.joint_nodes), 4, 4)
        self.target_dpos = np.zeros((0, n, 3), np.float32) if self.target_dpos is None else np.ascontiguousarray(self.target_dpos, np.float32).reshape(-1, n, 3)
        if self.target_dnrm is not None:
            self.target_dnrm = np.ascontiguousarray(self.target_dnrm, np.float32).reshape(len(self.target_dpos), n, 3)
        nt = len(self.target_dpos)
        self.default_weights = np.zeros(nt, np.float32) if self.default_weights is None else np.ascontiguousarray(self.default_weights, np.float32).reshape(nt)


@dataclass
class Rig:
    """The node hierarchy and the animations the skins are posed from.  nodes: dicts with glTF's own keys (`translation`, `rotation` xyzw,
    `scale`, or `matrix` as 16 column-major floats; `name`) plus `parent` (-1: a root).  animations: dicts {name, channels}, a channel being
    {path: translation | rotation | scale | weights, node (or, for weights, skin: the index into Mesh.skins), interpolation: LINEAR | STEP,
    times (k,) float32, values (k, components) float32}."""

    nodes: list = field(default_factory=list)
    animations: list = field(default_factory=list)


def _sample_channel(ch, t):
    """the channel's value at time t (clamped to its key range), float64"""
    times = np.asarray(ch["times"], np.float64)
    vals = np.asarray(ch["values"], np.float64).reshape(len(times), -1)
    rot = ch["path"] == "rotation"

    def unit(q):
        return q / np.linalg.norm(q) if rot else q

    if t <= times[0]:
        return unit(vals[0])
    if t >= times[-1]:
        return unit(vals[-1])
    i = int(np.searchsorted(times, t, side="right")) - 1
    if ch.get("interpolation", "LINEAR") == "STEP" or times[i + 1] == times[i]:
        return unit(vals[i])
    u = (t - times[i]) / (times[i + 1] - times[i])
    a, b = vals[i], vals[i + 1]
    if not rot:
        return a + (b - a) * u
    d = float(np.dot(a, b))
    if d < 0.0:  # the shorter arc
        b, d = -b, -d
    d = min(d / (np.linalg.norm(a) * np.linalg.norm(b)), 1.0)
    theta = math.acos(d)
    if theta < 1e-6:
        return unit(a + (b - a) * u)
    return unit((math.sin((1.0 - u) * theta) * a + math.sin(u * theta) * b) / math.sin(theta))


@dataclass
class Mesh:
    """Flattened scene: global vertex / index buffers + one GeometryInfo per primitive (world/mod.rs:103-125)."""

    vertices: np.ndarray  # (n, 8) float32  p n t
    indices: np.ndarray  # (m,) uint32, relative to each geometry's vertex_offset
    geometries: np.ndarray  # (g,) GEOMETRY_DTYPE
    prim_counts: np.ndarray  # (g,) uint32
    names: list = field(default_factory=list)
    textures: list = field(default_factory=list)  # base-colour textures: (h, w, 4) uint8, sRGB-encoded colour
    alpha_cutoffs: np.ndarray = None  # (g,) float32 alpha cutoff per geometry (rt3_scene_set_alpha_cutoffs); None -> zeros (all opaque)
    material_textures: np.ndarray = None  # (g,) MATERIAL_TEXTURES_DTYPE (rt3_scene_set_material_textures); None -> no texture anywhere
    lights: np.ndarray = None  # (l,) LIGHT_DTYPE punctual lights (rt3_scene_set_lights); None -> none
    transmission: np.ndarray = None  # (g,) TRANSMISSION_DTYPE glass (rt3_scene_set_transmission); None -> no glass anywhere
    # (g,) ATTENUATION_DTYPE sigma per geometry (rt3_scene_set_attenuation); None -> zeros.  A thin-walled or opaque
    # geometry keeps what its material said; only solid glass absorbs (absorbing()).
    attenuation: np.ndarray = None
    # (g, 4) float64 {attenuationColor rgb, attenuationDistance} the sigmas were made from, for write_glb; None -> derived from the sigmas
    attenuation_source: np.ndarray = None
    # skinned and / or morphed primitives: one Skin each, in vertex order; `rig` holds the nodes and animations they
    # are posed from.  `vertices` stays the static load whatever these say.
    skins: list = field(default_factory=list)
    rig: "Rig" = None

    def pose(self, t, animation=0):
        """per skin (palette (n_joints, 4, 4) float32, target weights (n_targets,) float32) at time `t` of animation `animation`: palette
        entry k = G(joint_k, t) . IBM_k, with G the joint's global matrix through the node hierarchy, evaluated in float64 and rounded once.
        Translation and scale are interpolated linearly, rotations along the shorter arc (slerp) and normalised, STEP holds the earlier key;
        `t` is clamped to each sampler's key range.  Without animations (animation 0 only) the nodes' own transforms pose the skins."""
        if not self.skins:
            return []
        rig = self.rig if self.rig is not None else Rig()
        if animation != 0 or rig.animations:
            channels = rig.animations[animation]["channels"]  # (IndexError: no such animation)
        else:
            channels = []
        over, skin_weights = {}, {}
        for ch in channels:
            v = _sample_channel(ch, float(t))
            if ch["path"] == "weights":
                skin_weights[ch["skin"]] = v
            else:
                over.setdefault(ch["node"], {})[ch["path"]] = v
        memo = {}

        def world(ni):
            if ni not in memo:
                node = rig.nodes[ni]
                if ni in over:  # (an animated node has no `matrix`: glTF)
                    node = {k: v for k, v in node.items() if k != "matrix"}
                    node.update(over[ni])
                m = _node_matrix(node)
                parent = rig.nodes[ni].get("parent", -1)
                memo[ni] = m if parent < 0 else world(parent) @ m
            return memo[ni]

        out = []
        for k, s in enumerate(self.skins):
            pal = np.stack([world(j) @ s.inverse_bind[q].astype(np.float64) for q, j in enumerate(s.joint_nodes)])
            w = np.asarray(skin_weights.get(k, s.default_weights), np.float64).reshape(-1)
            out.append((np.ascontiguousarray(pal, np.float32), np.ascontiguousarray(w, np.float32)))
        return out

    def __post_init__(self):
        self.lights = np.ascontiguousarray(np.zeros(0, LIGHT_DTYPE) if self.lights is None else self.lights, LIGHT_DTYPE).reshape(-1)
        if self.material_textures is None:
            self.material_textures = no_material_textures(len(self.geometries))
        self.material_textures = np.ascontiguousarray(self.material_textures, MATERIAL_TEXTURES_DTYPE).reshape(len(self.geometries))
        if self.transmission is None:
            self.transmission = no_transmission(len(self.geometries))
        self.transmission = np.ascontiguousarray(self.transmission, TRANSMISSION_DTYPE).reshape(len(self.geometries))
        if self.attenuation is None:
            self.attenuation = no_attenuation(len(self.geometries))
        self.attenuation = np.ascontiguousarray(self.attenuation, ATTENUATION_DTYPE).reshape(len(self.geometries))
        if self.alpha_cutoffs is None:
            self.alpha_cutoffs = np.zeros(len(self.geometries), np.float32)
        self.alpha_cutoffs = np.ascontiguousarray(self.alpha_cutoffs, np.float32).reshape(len(self.geometries))

    def absorbing(self) -> np.ndarray:
        """(g,) bool: the geometries rt3_accel_build classifies as absorbing -- transmission > 0, solid, some sigma > 0"""
        tr = self.transmission
        return (tr["transmission"] > 0) & (tr["thin_walled"] == 0) & np.any(self.attenuation["sigma"] > 0, axis=1)

    @property
    def n_triangles(self) -> int:
        return int(self.prim_counts.sum())

    def triangle_positions(self) -> np.ndarray:
        """(n_tris, 3, 3) world positions, in global primitive order."""
        out = []
        for g, cnt in zip(self.geometries, self.prim_counts):
            io, vo = int(g["index_offset"]), int(g["vertex_offset"])
            idx = self.indices[io : io + 3 * int(cnt)].astype(np.int64) + vo
            out.append(self.vertices[idx, :3].reshape(-1, 3, 3))
        return np.concatenate(out, axis=0) if out else np.zeros((0, 3, 3), np.float32)


class MeshBuilder:
    """Accumulates (positions, normals, uvs, triangles, material) parts into a `Mesh`."""

    def __init__(self):
        self.v, self.i, self.g, self.c, self.names, self.cut, self.mt, self.tr = [], [], [], [], [], [], [], []
        self.at, self.at_src = [], []
        self.nv = 0
        self.ni = 0

    def add(self, name, pos, nrm, uv, tris, mat: Material, normalize=True):
        pos = np.asarray(pos, np.float32).reshape(-1, 3)
        if normalize:
            nrm = np.asarray(nrm, np.float64).reshape(-1, 3)
            ln = np.linalg.norm(nrm, axis=1, keepdims=True)
            nrm = nrm / np.maximum(ln, 1e-20)
        nrm = np.asarray(nrm, np.float32).reshape(-1, 3)
        uv = np.zeros((len(pos), 2), np.float32) if uv is None else np.asarray(uv, np.float32).reshape(-1, 2)
        tris = np.asarray(tris, np.uint32).reshape(-1, 3)
        assert tris.size == 0 or int(tris.max()) < len(pos)
        g = np.zeros((), GEOMETRY_DTYPE)
        g["base_color"] = (*mat.color, mat.alpha)
        g["base_color_texture_index"] = mat.texture_offset
        g["metallic_factor"] = mat.metalic_factor
        g["roughness"] = mat.roughness_factor
        g["emission"] = (*mat.emission, 0.0)
        g["index_offset"] = self.ni
        g["vertex_offset"] = self.nv
        self.v.append(np.concatenate([pos, nrm, uv], axis=1))
        self.i.append(tris.reshape(-1))
        self.g.append(g)
        self.c.append(len(tris))
        self.cut.append(mat.alpha_cutoff)
        self.mt.append((mat.metallic_roughness_texture, mat.normal_texture, mat.emissive_texture, mat.normal_scale))
        self.tr.append((mat.transmission, mat.ior, mat.thin_walled, 0))
        self.at.append((tuple(attenuation_sigma(mat.attenuation_color, mat.attenuation_distance)), 0))
        self.at_src.append((*[float(x) for x in mat.attenuation_color], float(mat.attenuation_distance)))
        self.names.append(name)
        self.nv += len(pos)
        self.ni += tris.size

    def build(self) -> Mesh:
        return Mesh(
            np.ascontiguousarray(np.concatenate(self.v, axis=0), np.float32),
            np.ascontiguousarray(np.concatenate(self.i), np.uint32),
            np.array(self.g, GEOMETRY_DTYPE),
            np.array(self.c, np.uint32),
            list(self.names),
            alpha_cutoffs=np.array(self.cut, np.float32),
            material_textures=np.array(self.mt, MATERIAL_TEXTURES_DTYPE),
            transmission=np.array(self.tr, TRANSMISSION_DTYPE),
            attenuation=np.array(self.at, ATTENUATION_DTYPE),
            attenuation_source=np.array(self.at_src, np.float64).reshape(-1, 4),
        )


# ----------------------------------------------------------------------------------------------- glTF (.glb)
_COMP = {5120: ("i1", 1), 5121: ("u1", 1), 5122: ("<i2", 2), 5123: ("<u2", 2), 5125: ("<u4", 4), 5126: ("<f4", 4)}
_NCOMP = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}


def _attenuation_gltf(mesh: Mesh, gi: int):
    """(attenuationColor, attenuationDistance) that attenuation_sigma takes back to mesh.attenuation[gi], bit for bit: the pair the sigmas
    were made from where the mesh still has it, otherwise distance 2^k with the largest sigma x distance in [0.5, 1) and colour
    exp(-sigma x distance)"""
    sigma = mesh.attenuation["sigma"][gi]
    src = mesh.attenuation_source
    if src is not None and len(src) == len(mesh.geometries) and np.array_equal(attenuation_sigma(src[gi, :3], src[gi, 3]), sigma):
        return [float(x) for x in src[gi, :3]], float(src[gi, 3])
    dist = 2.0 ** -math.ceil(math.log2(float(sigma.max())) + 1e-9)
    col = np.exp(-sigma.astype(np.float64) * dist)
    if not np.array_equal(attenuation_sigma(col, dist), sigma):
        raise ValueError(f"geometry {gi}: its absorption coefficients {sigma} have no attenuationColor / attenuationDistance that reads back exactly")
    return [float(x) for x in col], dist


def write_glb(path, mesh: Mesh) -> None:
    """One glTF mesh+node per geometry, identity transforms, u32 indices, one material per geometry; one node per punctual light
    (KHR_lights_punctual: translation, and the rotation that takes -z to the light's direction)."""
    bin_parts, views, accessors, meshes, nodes, materials = [], [], [], [], [], []
    used = []  # extensionsUsed, in order of first use
    off = 0

    def push(arr, target=None):
        nonlocal off
        b = np.ascontiguousarray(arr).tobytes()
        pad = (-len(b)) % 4
        view = {"buffer": 0, "byteOffset": off, "byteLength": len(b)}
        if target:
            view["target"] = target
        views.append(view)
        bin_parts.append(b + b"\0" * pad)
        off += len(b) + pad
        return len(views) - 1

    # skins: the rig's nodes come first, under their own indices, so that joint lists and animation channels read
    # back as they are; a skinned geometry's node follows them and is written in bind space (Skin.rest), with its joints, weights and targets
    rig = (mesh.rig or Rig()) if mesh.skins else None
    n_rig = len(rig.nodes) if rig else 0
    gl_skins, skin_at = [], {s.geometry: k for k, s in enumerate(mesh.skins)}
    for i in range(n_rig):
        rn = {k: ([float(x) for x in v] if k != "name" else v) for k, v in rig.nodes[i].items() if k != "parent"}
        kids = [c for c in range(n_rig) if rig.nodes[c].get("parent", -1) == i]
        if kids:
            rn["children"] = kids
        nodes.append(rn)
    for gi, (g, cnt) in enumerate(zip(mesh.geometries, mesh.prim_counts)):
        io, vo, cnt = int(g["index_offset"]), int(g["vertex_offset"]), int(cnt)
        idx = mesh.indices[io : io + 3 * cnt]
        later = [int(x) for x in mesh.geometries["vertex_offset"] if int(x) > vo]
        nv = (min(later) if later else len(mesh.vertices)) - vo  # keep unreferenced vertices: the round trip is exact
        v = mesh.vertices[vo : vo + nv]
        skin = mesh.skins[skin_at[gi]] if gi in skin_at else None
        if skin is not None:
            if skin.first_vertex != vo or len(skin.rest) != nv:
                raise ValueError(f"geometry {gi}: its skin does not cover the geometry's own vertex range")
            v = skin.rest
        acc = []
        for col, typ in ((slice(0, 3), "VEC3"), (slice(3, 6), "VEC3"), (slice(6, 8), "VEC2")):
            data = np.ascontiguousarray(v[:, col], "<f4")
            a = {"bufferView": push(data, 34962), "componentType": 5126, "count": nv, "type": typ}
            if typ == "VEC3" and col.start == 0:
                a["min"] = [float(x) for x in data.min(axis=0)]
                a["max"] = [float(x) for x in data.max(axis=0)]
            accessors.append(a)
            acc.append(len(accessors) - 1)
        accessors.append({"bufferView": push(idx.astype("<u4"), 34963), "componentType": 5125, "count": 3 * cnt, "type": "SCALAR"})
        ia = len(accessors) - 1
        pbr = {
            "baseColorFactor": [float(x) for x in g["base_color"]],
            "metallicFactor": float(g["metallic_factor"]),
            "roughnessFactor": float(g["roughness"]),
        }
        if int(g["base_color_texture_index"]) > -1:
            pbr["baseColorTexture"] = {"index": int(g["base_color_texture_index"])}
        mtl = {"name": f"mat{gi}", "pbrMetallicRoughness": pbr, "emissiveFactor": [float(x) for x in g["emission"][:3]]}
        mt = mesh.material_textures[gi]
        if int(mt["metallic_roughness_texture"]) > -1:
            pbr["metallicRoughnessTexture"] = {"index": int(mt["metallic_roughness_texture"])}
        if int(mt["normal_texture"]) > -1:
            mtl["normalTexture"] = {"index": int(mt["normal_texture"]), "scale": float(mt["normal_scale"])}
        if int(mt["emissive_texture"]) > -1:
            mtl["emissiveTexture"] = {"index": int(mt["emissive_texture"])}
        if float(mesh.alpha_cutoffs[gi]) > 0.0:  # masked; opaque is glTF's default and stays implicit
            mtl["alphaMode"], mtl["alphaCutoff"] = "MASK", float(mesh.alpha_cutoffs[gi])
        # glass: the three extensions' defaults -- no transmission, ior 1.5, no volume = thin-walled -- stay implicit
        tr, ext = mesh.transmission[gi], {}
        if float(tr["transmission"]) > 0.0:
            ext["KHR_materials_transmission"] = {"transmissionFactor": float(tr["transmission"])}
        if float(tr["transmission"]) > 0.0 or float(tr["ior"]) != 1.5:
            ext["KHR_materials_ior"] = {"ior": float(tr["ior"])}
        if int(tr["thin_walled"]) == 0:
            ext["KHR_materials_volume"] = {"thicknessFactor": 1.0}
        # absorbing glass: the defaults -- colour 1, infinite distance -- stay implicit
        if np.any(mesh.attenuation["sigma"][gi] > 0):
            col, dist = _attenuation_gltf(mesh, gi)
            ext.setdefault("KHR_materials_volume", {}).update({"attenuationColor": col, "attenuationDistance": dist})
        if ext:
            mtl["extensions"] = ext
            used += [k for k in ext if k not in used]
        materials.append(mtl)
        meshes.append({"name": mesh.names[gi] if gi < len(mesh.names) else f"g{gi}",
                       "primitives": [{"attributes": {"POSITION": acc[0], "NORMAL": acc[1], "TEXCOORD_0": acc[2]}, "indices": ia, "material": gi}]})
        nodes.append({"mesh": gi})
        if skin is not None:
            prim = meshes[-1]["primitives"][0]
            accessors.append({"bufferView": push(skin.joints.astype("<u2"), 34962), "componentType": 5123, "count": nv, "type": "VEC4"})
            prim["attributes"]["JOINTS_0"] = len(accessors) - 1
            accessors.append({"bufferView": push(skin.weights.astype("<f4"), 34962), "componentType": 5126, "count": nv, "type": "VEC4"})
            prim["attributes"]["WEIGHTS_0"] = len(accessors) - 1
            for t in range(len(skin.target_dpos)):
                tg = {}
                for key, arr in (("POSITION", skin.target_dpos), ("NORMAL", skin.target_dnrm)):
                    if arr is not None:
                        data = np.ascontiguousarray(arr[t], "<f4")
                        accessors.append({"bufferView": push(data, 34962), "componentType": 5126, "count": nv, "type": "VEC3",
                                          "min": [float(x) for x in data.min(axis=0)], "max": [float(x) for x in data.max(axis=0)]})
                        tg[key] = len(accessors) - 1
                prim.setdefault("targets", []).append(tg)
            if len(skin.target_dpos):
                meshes[-1]["weights"] = [float(x) for x in skin.default_weights]
            ibm = np.ascontiguousarray(skin.inverse_bind.transpose(0, 2, 1), "<f4")  # column-major
            accessors.append({"bufferView": push(ibm), "componentType": 5126, "count": len(ibm), "type": "MAT4"})
            gl_skins.append({"joints": [int(j) for j in skin.joint_nodes], "inverseBindMatrices": len(accessors) - 1})
            nodes[-1]["skin"] = len(gl_skins) - 1
    gl_lights = []
    for li, l in enumerate(mesh.lights):
        I = np.asarray(l["intensity"], np.float64)
        top = float(I.max())
        kind = ("point", "spot", "directional")[int(l["type"])]
        gl = {"type": kind, "color": [float(x / top) for x in I] if top > 0 else [0.0, 0.0, 0.0], "intensity": top}
        if float(l["range"]) > 0.0 and kind != "directional":
            gl["range"] = float(l["range"])
        if kind == "spot":
            gl["spot"] = {"innerConeAngle": float(l["inner_cone"]), "outerConeAngle": float(l["outer_cone"])}
        node = {"name": f"light{li}", "extensions": {"KHR_lights_punctual": {"light": li}}}
        if kind != "directional":
            node["translation"] = [float(x) for x in l["position"]]
        if kind != "point":  # the shortest rotation from -z to d: q = (cross(-z, d), 1 + dot(-z, d)), normalised
            d = np.asarray(l["direction"], np.float64)
            d = d / np.linalg.norm(d)
            q = np.array([d[1], -d[0], 0.0, 1.0 - d[2]])
            q = q / np.linalg.norm(q) if np.linalg.norm(q) > 1e-12 else np.array([1.0, 0.0, 0.0, 0.0])  # d = +z: half a turn about x
            node["rotation"] = [float(x) for x in q]
        gl_lights.append(gl)
        nodes.append(node)
    images, textures = [], []
    for ti, tex in enumerate(mesh.textures):  # embedded PNG (lossless), one glTF texture per image
        import io

        from PIL import Image

        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(tex, np.uint8), "RGBA").save(buf, format="PNG")
        images.append({"bufferView": push(np.frombuffer(buf.getvalue(), np.uint8)), "mimeType": "image/png"})
        textures.append({"source": ti})
    doc = {
        "asset": {"version": "2.0", "generator": "raytracer3_amd.assets"},
        "scene": 0,
        "scenes": [{"nodes": [i for i in range(len(nodes)) if i >= n_rig or rig.nodes[i].get("parent", -1) < 0]}],
        "nodes": nodes, "meshes": meshes, "materials": materials, "accessors": accessors, "bufferViews": views,
        "buffers": [{"byteLength": off}],
    }
    if gl_skins:
        doc["skins"] = gl_skins
    gl_anims = []
    for an in (rig.animations if rig else []):
        samplers, channels = [], []
        for ch in an["channels"]:
            times = np.ascontiguousarray(ch["times"], "<f4").reshape(-1)
            vals = np.ascontiguousarray(ch["values"], "<f4").reshape(len(times), -1)
            accessors.append({"bufferView": push(times), "componentType": 5126, "count": len(times), "type": "SCALAR",
                              "min": [float(times.min())], "max": [float(times.max())]})
            typ = {"translation": "VEC3", "scale": "VEC3", "rotation": "VEC4", "weights": "SCALAR"}[ch["path"]]
            accessors.append({"bufferView": push(vals), "componentType": 5126, "count": vals.size if typ == "SCALAR" else len(vals), "type": typ})
            samplers.append({"input": len(accessors) - 2, "output": len(accessors) - 1, "interpolation": ch.get("interpolation", "LINEAR")})
            node = n_rig + mesh.skins[ch["skin"]].geometry if ch["path"] == "weights" else int(ch["node"])
            channels.append({"sampler": len(samplers) - 1, "target": {"node": node, "path": ch["path"]}})
        gl_anims.append({"name": an.get("name", ""), "samplers": samplers, "channels": channels})
    if gl_anims:
        doc["animations"] = gl_anims
        doc["buffers"][0]["byteLength"] = off
    if images:
        doc["images"], doc["textures"] = images, textures
    if gl_lights:
        used.append("KHR_lights_punctual")
        doc["extensions"] = {"KHR_lights_punctual": {"lights": gl_lights}}
    if used:
        doc["extensionsUsed"] = used
    js = json.dumps(doc, separators=(",", ":")).encode()
    js += b" " * ((-len(js)) % 4)
    blob = b"".join(bin_parts)
    total = 12 + 8 + len(js) + 8 + len(blob)
    with open(path, "wb") as f:
        f.write(struct.pack("<4sII", b"glTF", 2, total))
        f.write(struct.pack("<I4s", len(js), b"JSON"))
        f.write(js)
        f.write(struct.pack("<I4s", len(blob), b"BIN\0"))
        f.write(blob)


def _node_matrix(node) -> np.ndarray:
    if "matrix" in node:
        return np.array(node["matrix"], np.float64).reshape(4, 4).T  # glTF is column-major
    m = np.eye(4)
    if "scale" in node:
        m = np.diag([*node["scale"], 1.0]) @ m
    if "rotation" in node:
        x, y, z, w = node["rotation"]
        r = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 0],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w), 0],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y), 0],
                      [0, 0, 0, 1]], np.float64)
        m = r @ m
    if "translation" in node:
        t = np.eye(4)
        t[:3, 3] = node["translation"]
        m = t @ m
    return m


class GltfMeshLoader:
    """`.glb` -> `Mesh` (assets/mod.rs:179-200 + :207-252, all primitives, transforms baked at load)."""

    extensions = ("glb",)

    @staticmethod
    def load(path) -> Mesh:
        data = Path(path).read_bytes()
        magic, version, total = struct.unpack_from("<4sII", data, 0)
        if magic != b"glTF" or version != 2:
            raise ValueError(f"{path}: not a glTF 2 binary")
        p, doc, blob = 12, None, b""
        while p < total:
            ln, typ = struct.unpack_from("<I4s", data, p)
            chunk = data[p + 8 : p + 8 + ln]
            if typ == b"JSON":
                doc = json.loads(chunk.decode())
            elif typ == b"BIN\0":
                blob = chunk
            p += 8 + ln
        if doc is None:
            raise ValueError(f"{path}: no JSON chunk")

        def accessor(i):
            a = doc["accessors"][i]
            bv = doc["bufferViews"][a["bufferView"]]
            dt, sz = _COMP[a["componentType"]]
            nc = _NCOMP[a["type"]]
            start = bv.get("byteOffset", 0) + a.get("byteOffset", 0)
            stride = bv.get("byteStride", 0) or sz * nc
            cnt = a["count"]
            if stride == sz * nc:
                arr = np.frombuffer(blob, dt, cnt * nc, start).reshape(cnt, nc)
            else:
                arr = np.stack([np.frombuffer(blob, dt, nc, start + k * stride) for k in range(cnt)])
            if a.get("normalized") and a["componentType"] != 5126:
                arr = arr.astype(np.float32) / float(np.iinfo(np.dtype(dt)).max)
            return arr

        mb = MeshBuilder()
        mats = doc.get("materials", [])
        # skins, morph targets and animations.  What cannot be represented -- JOINTS_1, sparse accessors, CUBICSPLINE
        # samplers, more than SKIN_MAX_TARGETS targets or SKIN_MAX_JOINTS joints -- leaves the primitive a static one, with a warning.
        gl_nodes = doc.get("nodes", [])
        parents = [-1] * len(gl_nodes)
        for i, nd in enumerate(gl_nodes):
            for c in nd.get("children", []):
                parents[c] = i
        cubic = set()  # (node, path) pairs a CUBICSPLINE sampler drives
        for an in doc.get("animations", []):
            for ch in an.get("channels", []):
                if an["samplers"][ch["sampler"]].get("interpolation", "LINEAR") == "CUBICSPLINE" and "node" in ch.get("target", {}):
                    cubic.add((ch["target"]["node"], "weights" if ch["target"]["path"] == "weights" else "trs"))
        skins, skin_nodes = [], []

        def skin_of(ni, node, gm, pi, prim, tris):
            """the Skin of one primitive (first_vertex and geometry are filled in by the caller), or None: neither skinned nor morphed, or
            not representable"""
            at, targets = prim["attributes"], prim.get("targets") or []
            skinned = "skin" in node and "JOINTS_0" in at and "WEIGHTS_0" in at
            if not skinned and not targets:
                return None
            gs = doc["skins"][node["skin"]] if skinned else None
            jn = list(gs["joints"]) if skinned else [ni]
            used = [at[k] for k in ("POSITION", "NORMAL", "TEXCOORD_0", "JOINTS_0", "WEIGHTS_0") if k in at]
            used += [tg[k] for tg in targets for k in ("POSITION", "NORMAL") if k in tg]
            if skinned and "inverseBindMatrices" in gs:
                used.append(gs["inverseBindMatrices"])
            chain = set()
            for j in jn:
                while j >= 0 and j not in chain:
                    chain.add(j)
                    j = parents[j]
            why = None
            if "JOINTS_1" in at or "WEIGHTS_1" in at:
                why = "more than four influences per vertex (JOINTS_1)"
            elif any("sparse" in doc["accessors"][a] for a in used):
                why = "a sparse accessor"
            elif len(targets) > SKIN_MAX_TARGETS:
                why = f"{len(targets)} morph targets (at most {SKIN_MAX_TARGETS})"
            elif len(jn) > SKIN_MAX_JOINTS:
                why = f"{len(jn)} joints (at most {SKIN_MAX_JOINTS})"
            elif any((j, "trs") in cubic for j in chain) or (targets and (ni, "weights") in cubic):
                why = "a CUBICSPLINE animation sampler"
            elif any("POSITION" not in tg for tg in targets):
                why = "a morph target without POSITION"
            if why:
                import warnings

                warnings.warn(f"{path}: primitive {pi} of mesh {gm.get('name', 'mesh')!r} has {why}: it is loaded statically")
                return None
            pos = accessor(at["POSITION"]).astype(np.float32)
            if "NORMAL" in at:
                nrm = accessor(at["NORMAL"]).astype(np.float32)
            else:  # flat normals from the bind-space geometry, like the static load's
                fn = np.cross(pos[tris[:, 1]].astype(np.float64) - pos[tris[:, 0]], pos[tris[:, 2]].astype(np.float64) - pos[tris[:, 0]])
                acc = np.zeros((len(pos), 3), np.float64)
                for k in range(3):
                    np.add.at(acc, tris[:, k], fn)
                nrm = (acc / np.maximum(np.linalg.norm(acc, axis=1, keepdims=True), 1e-20)).astype(np.float32)
            uv = accessor(at["TEXCOORD_0"]).astype(np.float32) if "TEXCOORD_0" in at else np.zeros((len(pos), 2), np.float32)
            if skinned:
                joints = accessor(at["JOINTS_0"]).astype(np.uint16)
                w = accessor(at["WEIGHTS_0"])
                weights = w.astype(np.float32) if w.dtype.kind == "f" else w.astype(np.float32) / np.float32(np.iinfo(w.dtype).max)
                if "inverseBindMatrices" in gs:
                    ibm = accessor(gs["inverseBindMatrices"]).astype(np.float32).reshape(-1, 4, 4).transpose(0, 2, 1)  # glTF is column-major
                else:
                    ibm = np.tile(np.eye(4, dtype=np.float32), (len(jn), 1, 1))
            else:
                joints = np.zeros((len(pos), 4), np.uint16)
                weights = np.tile(np.array([1, 0, 0, 0], np.float32), (len(pos), 1))
                ibm = np.eye(4, dtype=np.float32)[None]
            dpos = np.stack([accessor(tg["POSITION"]).astype(np.float32) for tg in targets]) if targets else None
            dnrm = np.stack([accessor(tg["NORMAL"]).astype(np.float32) for tg in targets]) if targets and all("NORMAL" in tg for tg in targets) else None
            dw = node.get("weights", gm.get("weights"))
            return Skin(0, np.concatenate([pos, nrm, uv], 1), joints, weights, jn, ibm, dpos, dnrm, None if dw is None else np.asarray(dw, np.float32))

        gl_lights = doc.get("extensions", {}).get("KHR_lights_punctual", {}).get("lights", [])
        lights = []

        def visit(ni, parent):
            node = doc["nodes"][ni]
            m = parent @ _node_matrix(node)
            li = node.get("extensions", {}).get("KHR_lights_punctual", {}).get("light")
            if li is not None:  # baked like the meshes: position M (0, 0, 0, 1), direction normalise(M3 (0, 0, -1)); scale leaves the intensity alone
                gl = gl_lights[li]
                kind = {"point": LIGHT_POINT, "spot": LIGHT_SPOT, "directional": LIGHT_DIRECTIONAL}[gl["type"]]
                d = m[:3, :3] @ np.array([0.0, 0.0, -1.0])
                spot = gl.get("spot", {})
                lights.append(make_light(kind, np.array(gl.get("color", [1, 1, 1]), np.float64) * gl.get("intensity", 1.0), m[:3, 3], d / np.linalg.norm(d),
                                         0.0 if kind == LIGHT_DIRECTIONAL else gl.get("range", 0.0), spot.get("innerConeAngle", 0.0),
                                         spot.get("outerConeAngle", math.pi / 4)))
            if "mesh" in node:
                gm = doc["meshes"][node["mesh"]]
                nm = np.linalg.inv(m[:3, :3]).T
                for pi, prim in enumerate(gm["primitives"]):
                    if prim.get("mode", 4) != 4:
                        continue
                    at = prim["attributes"]
                    identity = np.array_equal(m, np.eye(4))
                    pos = accessor(at["POSITION"]).astype(np.float64)
                    pos = (pos if identity else pos @ m[:3, :3].T + m[:3, 3]).astype(np.float32)
                    keep = False
                    if "NORMAL" in at:
                        nrm = accessor(at["NORMAL"])
                        keep = identity and nrm.dtype == np.float32  # stored unit normals pass through bit for bit
                        if not keep:
                            nrm = nrm.astype(np.float64) @ nm.T
                    else:
                        nrm = None
                    uv = accessor(at["TEXCOORD_0"]).astype(np.float32) if "TEXCOORD_0" in at else None
                    idx = accessor(prim["indices"]).reshape(-1).astype(np.uint32) if "indices" in prim else np.arange(len(pos), dtype=np.uint32)
                    tris = idx[: len(idx) // 3 * 3].reshape(-1, 3)
                    if nrm is None:  # flat normals from geometry
                        fn = np.cross(pos[tris[:, 1]] - pos[tris[:, 0]], pos[tris[:, 2]] - pos[tris[:, 0]])
                        nrm = np.zeros_like(pos, np.float64)
                        for k in range(3):
                            np.add.at(nrm, tris[:, k], fn)
                    mat = Material()
                    if "material" in prim:
                        gmtl = mats[prim["material"]]
                        pbr = gmtl.get("pbrMetallicRoughness", {})
                        bc = pbr.get("baseColorFactor", [1, 1, 1, 1])
                        em = np.array(gmtl.get("emissiveFactor", [0, 0, 0]), np.float64)
                        em = em * gmtl.get("extensions", {}).get("KHR_materials_emissive_strength", {}).get("emissiveStrength", 1.0)
                        tex = pbr.get("baseColorTexture", {}).get("index", -1)
                        # alphaMode MASK: alphaCutoff (default 0.5); OPAQUE and BLEND (not supported: drawn opaque) -> 0
                        cut = float(gmtl.get("alphaCutoff", 0.5)) if gmtl.get("alphaMode", "OPAQUE") == "MASK" else 0.0

                        def tex_index(info):  # a texture reference; one through another uv set than TEXCOORD_0 counts as absent
                            return int(info.get("index", -1)) if info and info.get("texCoord", 0) == 0 else -1

                        # glass: a transmission texture is ignored; no volume extension, or thicknessFactor 0, is thin-walled
                        gext = gmtl.get("extensions", {})
                        tau = float(gext.get("KHR_materials_transmission", {}).get("transmissionFactor", 0.0))
                        ior = float(gext.get("KHR_materials_ior", {}).get("ior", 1.5))
                        gvol = gext.get("KHR_materials_volume", {})
                        thin = 0 if float(gvol.get("thicknessFactor", 0.0)) > 0.0 else 1
                        att_c = tuple(float(x) for x in gvol.get("attenuationColor", (1.0, 1.0, 1.0)))
                        att_d = float(gvol.get("attenuationDistance", math.inf))
                        nt = gmtl.get("normalTexture")
                        mat = Material(tuple(bc[:3]), pbr.get("metallicFactor", 1.0), pbr.get("roughnessFactor", 1.0), tuple(em), tex, cut,
                                       float(bc[3]) if len(bc) > 3 else 1.0, tex_index(pbr.get("metallicRoughnessTexture")), tex_index(nt),
                                       tex_index(gmtl.get("emissiveTexture")), float(nt.get("scale", 1.0)) if nt else 1.0, tau, ior, thin, att_c, att_d)
                    mb.add(f"{gm.get('name', 'mesh')}.{pi}", pos, nrm, uv, tris, mat, normalize=not keep)
                    sk = skin_of(ni, node, gm, pi, prim, tris)
                    if sk is not None:
                        sk.first_vertex, sk.geometry = mb.nv - len(pos), len(mb.g) - 1
                        skins.append(sk)
                        skin_nodes.append(ni)
            for c in node.get("children", []):
                visit(c, m)

        scene = doc["scenes"][doc.get("scene", 0)]
        for root in scene["nodes"]:
            visit(root, np.eye(4))
        mesh = mb.build()
        mesh.lights = lights_array(lights)
        if skins:
            rig = Rig()
            for i, nd in enumerate(gl_nodes):
                rn = {k: nd[k] for k in ("name", "translation", "rotation", "scale", "matrix") if k in nd}
                rn["parent"] = parents[i]
                rig.nodes.append(rn)
            for an in doc.get("animations", []):
                chans = []
                for ch in an.get("channels", []):
                    smp, tgt = an["samplers"][ch["sampler"]], ch.get("target", {})
                    interp = smp.get("interpolation", "LINEAR")
                    if "node" not in tgt or interp == "CUBICSPLINE":
                        continue
                    times = accessor(smp["input"]).astype(np.float32).reshape(-1)
                    vals = np.asarray(accessor(smp["output"]), np.float32).reshape(len(times), -1)
                    if tgt["path"] == "weights":
                        chans += [dict(path="weights", skin=k, interpolation=interp, times=times, values=vals)
                                  for k, sn in enumerate(skin_nodes) if sn == tgt["node"] and vals.shape[1] == len(skins[k].target_dpos)]
                    else:
                        chans.append(dict(path=tgt["path"], node=tgt["node"], interpolation=interp, times=times, values=vals))
                rig.animations.append(dict(name=an.get("name", ""), channels=chans))
            mesh.skins, mesh.rig = skins, rig
        # textures -> images (embedded PNG / JPEG, decoded by Pillow); Material.texture_offset indexes doc["textures"]
        for tex in doc.get("textures", []):
            img = doc["images"][tex["source"]]
            if "bufferView" in img:
                bv = doc["bufferViews"][img["bufferView"]]
                raw = blob[bv.get("byteOffset", 0) : bv.get("byteOffset", 0) + bv["byteLength"]]
            else:
                raw = (Path(path).parent / img["uri"]).read_bytes()
            import io

            from PIL import Image

            mesh.textures.append(np.ascontiguousarray(np.array(Image.open(io.BytesIO(raw)).convert("RGBA"), np.uint8)))
        return mesh


def load(path) -> Mesh:
    """A scene file -> `Mesh` by its extension (GltfMeshLoader.extensions: binary glTF)."""
    if Path(path).suffix.lower().lstrip(".") in GltfMeshLoader.extensions:
        return GltfMeshLoader.load(path)
    raise ValueError(f"{path}: unsupported scene format (expected one of {GltfMeshLoader.extensions})")


# ----------------------------------------------------------------------------------------------- EXR (scanline, no compression)
def _exr_zip_pack(raw: bytes) -> bytes:
    """OpenEXR ZIP/ZIPS block: de-interleave even/odd bytes, delta-predict, deflate."""
    import zlib

    a = np.frombuffer(raw, np.uint8)
    t = np.concatenate([a[0::2], a[1::2]]).astype(np.int16)
    d = t.copy()
    d[1:] = (t[1:] - t[:-1] + 128 + 256) % 256
    return zlib.compress(d.astype(np.uint8).tobytes(), 6)


def _exr_zip_unpack(comp: bytes, size: int) -> bytes:
    import zlib

    d = np.frombuffer(zlib.decompress(comp), np.uint8)
    if len(d) != size:
        raise ValueError("EXR ZIP block has the wrong size")
    return _exr_predictor_undo(d, size)

# ---- OpenEXR RLE and PIZ codecs, restated from the published OpenEXR algorithm (ImfRle / ImfPizCompressor / ImfWav / ImfHuf).
# Parity unpinned: the reference tree ships no EXR (its `image::open("./assets/skybox2.exr")` is commented out, main.rs:94) and
# this image has no other EXR implementation to compare with; the decoders are checked against the encoders below and against the
# C++ decoder of host/assets.hpp (tests/test_host_assets.py).
def _exr_predictor_undo(d: np.ndarray, size: int) -> bytes:
    """Shared tail of ZIP and RLE blocks: undo the byte delta predictor, then re-interleave the two halves."""
    d = d.astype(np.int64)
    d[1:] -= 128
    t = (np.cumsum(d) % 256).astype(np.uint8)
    half = (size + 1) // 2
    out = np.empty(size, np.uint8)
    out[0::2] = t[:half]
    out[1::2] = t[half:]
    return out.tobytes()


def _exr_predictor_apply(raw: bytes) -> np.ndarray:
    a = np.frombuffer(raw, np.uint8)
    t = np.concatenate([a[0::2], a[1::2]]).astype(np.int64)
    d = t.copy()
    d[1:] = (t[1:] - t[:-1] + 128) % 256
    return d.astype(np.uint8)


def _exr_rle_unpack(comp: bytes, size: int) -> bytes:
    out, p = bytearray(), 0
    while p < len(comp):
        c = comp[p] - 256 if comp[p] > 127 else comp[p]
        p += 1
        if c < 0:  # -c literal bytes
            out += comp[p : p - c]
            p += -c
        else:  # the next byte c + 1 times
            out += bytes([comp[p]]) * (c + 1)
            p += 1
    if len(out) != size:
        raise ValueError("EXR RLE block has the wrong size")
    return _exr_predictor_undo(np.frombuffer(bytes(out), np.uint8), size)


def _exr_rle_pack(raw: bytes) -> bytes:
    d = _exr_predictor_apply(raw).tobytes()
    out, p, n = bytearray(), 0, len(d)
    while p < n:
        r = 1
        while p + r < n and d[p + r] == d[p] and r < 128:
            r += 1
        if r >= 3:
            out += bytes([r - 1, d[p]])
            p += r
        else:
            q = p
            while q < n and q - p < 127 and not (q + 2 < n and d[q] == d[q + 1] == d[q + 2]):
                q += 1
            out += bytes([(256 - (q - p)) & 0xFF]) + d[p:q]
            p = q
    return bytes(out)


_HUF_ENCSIZE, _HUF_DECBITS = (1 << 16) + 1, 14
_SHORT_ZERO_RUN, _LONG_ZERO_RUN = 59, 63
_SHORTEST_LONG_RUN = 2 + _LONG_ZERO_RUN - _SHORT_ZERO_RUN  # 6
_LONGEST_LONG_RUN = 255 + _SHORTEST_LONG_RUN


def _huf_canonical(lengths):
    """ImfHuf hufCanonicalCodeTable: code lengths -> canonical codes (longer codes get the numerically smaller values)."""
    n = [0] * 59
    for l in lengths:
        n[l] += 1
    c = 0
    for i in range(58, 0, -1):
        nc = (c + n[i]) >> 1
        n[i] = c
        c = nc
    codes = [0] * len(lengths)
    for i, l in enumerate(lengths):
        if l:
            codes[i] = n[l]
            n[l] += 1
    return codes


class _Bits:
    def __init__(self, data=b"", p=0):
        self.d, self.p, self.c, self.lc, self.out = data, p, 0, 0, bytearray()

    def get(self, n):
        while self.lc < n:
            self.c = ((self.c << 8) | (self.d[self.p] if self.p < len(self.d) else 0)) & 0xFFFFFFFFFFFFFFFF
            self.p += 1
            self.lc += 8
        self.lc -= n
        return (self.c >> self.lc) & ((1 << n) - 1)

    def put(self, n, v):
        self.c = (self.c << n) | v
        self.lc += n
        while self.lc >= 8:
            self.lc -= 8
            self.out.append((self.c >> self.lc) & 0xFF)
        self.c &= (1 << self.lc) - 1

    def flush(self):
        if self.lc:
            self.out.append((self.c << (8 - self.lc)) & 0xFF)
        return bytes(self.out)


def _huf_uncompress(comp: bytes, n_raw: int) -> np.ndarray:
    if n_raw == 0:
        return np.zeros(0, np.uint16)
    im, i_max, _table_len, n_bits = struct.unpack_from("<IIII", comp, 0)
    if im >= _HUF_ENCSIZE or i_max >= _HUF_ENCSIZE:
        raise ValueError("EXR PIZ: bad Huffman header")
    br = _Bits(comp, 20)
    lengths = [0] * _HUF_ENCSIZE
    s = im
    while s <= i_max:  # hufUnpackEncTable
        l = br.get(6)
        if l == _LONG_ZERO_RUN:
            s += br.get(8) + _SHORTEST_LONG_RUN
        elif l >= _SHORT_ZERO_RUN:
            s += l - _SHORT_ZERO_RUN + 2
        else:
            lengths[s] = l
            s += 1
    codes = _huf_canonical(lengths)
    data_start = 20 + _table_len
    tab_len, tab_sym, long_codes = [0] * (1 << _HUF_DECBITS), [0] * (1 << _HUF_DECBITS), {}
    for sym in range(im, i_max + 1):  # hufBuildDecTable
        l = lengths[sym]
        if not l:
            continue
        if l > _HUF_DECBITS:
            long_codes.setdefault(codes[sym] >> (l - _HUF_DECBITS), []).append((l, codes[sym], sym))
        else:
            base = codes[sym] << (_HUF_DECBITS - l)
            for k in range(base, base + (1 << (_HUF_DECBITS - l))):
                tab_len[k], tab_sym[k] = l, sym
    out = np.zeros(n_raw, np.uint16)
    d, p, end = comp, data_start, min(len(comp), data_start + (n_bits + 7) // 8)
    c, lc, produced, rlc = 0, 0, 0, i_max
    while produced < n_raw:  # hufDecode; bits past the end read as zero
        while lc < 58 and p < end:
            c = (c << 8) | d[p]
            p += 1
            lc += 8
        while lc < _HUF_DECBITS:  # past the end of the data: zero bits, like hufDecode's final shift
            c <<= 8
            p += 1
            lc += 8
            if p > end + 16:
                raise ValueError("EXR PIZ: Huffman data ends early")
        idx = (c >> (lc - _HUF_DECBITS)) & 0x3FFF
        l = tab_len[idx]
        if l:
            sym = tab_sym[idx]
        else:
            for l, code, sym in long_codes.get(idx, ()):
                while lc < l:
                    c = (c << 8) | (d[p] if p < end else 0)
                    p += 1
                    lc += 8
                if (c >> (lc - l)) & ((1 << l) - 1) == code:
                    break
            else:
                raise ValueError("EXR PIZ: invalid Huffman code")
        lc -= l
        c &= (1 << lc) - 1
        if sym == rlc:  # run: repeat the previous value
            while lc < 8:
                c = (c << 8) | (d[p] if p < end else 0)
                p += 1
                lc += 8
            lc -= 8
            run = (c >> lc) & 0xFF
            c &= (1 << lc) - 1
            if produced == 0 or produced + run > n_raw:
                raise ValueError("EXR PIZ: bad run length")
            out[produced : produced + run] = out[produced - 1]
            produced += run
        else:
            out[produced] = sym
            produced += 1
    return out


def _huf_compress(raw: np.ndarray) -> bytes:
    """Test-side encoder (hufCompress): Huffman codes of at most 58 bits, run-length pseudo symbol iM."""
    import heapq

    if len(raw) == 0:
        return b""
    freq = np.bincount(raw, minlength=_HUF_ENCSIZE).tolist()
    used = [i for i, f in enumerate(freq) if f]
    im, i_max = used[0], used[-1] + 1
    freq[i_max] = 1  # the run-length symbol
    used.append(i_max)
    lengths = [0] * _HUF_ENCSIZE
    heap = [(freq[i], i, (i,)) for i in used]
    heapq.heapify(heap)
    if len(heap) == 1:
        lengths[heap[0][1]] = 1
    while len(heap) > 1:
        fa, ka, sa = heapq.heappop(heap)
        fb, kb, sb = heapq.heappop(heap)
        for i in sa + sb:
            lengths[i] += 1
        heapq.heappush(heap, (fa + fb, min(ka, kb), sa + sb))
    if max(lengths) > 58:
        raise ValueError("Huffman code longer than 58 bits")
    codes = _huf_canonical(lengths)
    bw = _Bits()
    s = im
    while s <= i_max:  # hufPackEncTable
        l = lengths[s]
        if l == 0:
            z = 1
            while s + z <= i_max and lengths[s + z] == 0 and z < _LONGEST_LONG_RUN:
                z += 1
            if z >= 2:
                if z >= _SHORTEST_LONG_RUN:
                    bw.put(6, _LONG_ZERO_RUN)
                    bw.put(8, z - _SHORTEST_LONG_RUN)
                else:
                    bw.put(6, _SHORT_ZERO_RUN + z - 2)
                s += z
                continue
        bw.put(6, l)
        s += 1
    table = bw.flush()
    bw = _Bits()
    n_bits = 0

    def send(sym, run):  # sendCode
        nonlocal n_bits
        ls, lr = lengths[sym], lengths[i_max]
        if ls + lr + 8 < ls * run:
            bw.put(ls, codes[sym]); bw.put(lr, codes[i_max]); bw.put(8, run)
            n_bits += ls + lr + 8
        else:
            for _ in range(run + 1):
                bw.put(ls, codes[sym])
            n_bits += ls * (run + 1)

    vals = raw.tolist()
    cur, run = vals[0], 0
    for v in vals[1:]:
        if v == cur and run < 255:
            run += 1
        else:
            send(cur, run)
            run = 0
        cur = v
    send(cur, run)
    data = bw.flush()
    return struct.pack("<IIIII", im, i_max, len(table), n_bits, 0) + table + data


def _wav_levels(nx, ny):
    n, p = min(nx, ny), 1
    while p <= n:
        p <<= 1
    p >>= 1
    return p  # largest power of two <= min(nx, ny) (0 if that is 0)


def _wav_pairs(plane, a_idx, b_idx, w14, decode):
    """One butterfly over the element pairs (a, b) given as index tuples into `plane` (uint16); returns (a', b')."""
    a, b = plane[a_idx].astype(np.int64), plane[b_idx].astype(np.int64)
    if decode:
        if w14:  # wdec14(l = a, h = b)
            ls, hs = ((a + 0x8000) & 0xFFFF) - 0x8000, ((b + 0x8000) & 0xFFFF) - 0x8000
            ai = ls + (hs & 1) + (hs >> 1)
            return ai & 0xFFFF, (ai - hs) & 0xFFFF
        bb = (a - (b >> 1)) & 0xFFFF  # wdec16
        return (b + bb - 0x8000) & 0xFFFF, bb
    if w14:  # wenc14
        sa, sb = ((a + 0x8000) & 0xFFFF) - 0x8000, ((b + 0x8000) & 0xFFFF) - 0x8000
        return ((sa + sb) >> 1) & 0xFFFF, (sa - sb) & 0xFFFF
    ao = (a + 0x8000) & 0xFFFF  # wenc16
    m, dd = (ao + b) >> 1, ao - b
    m = np.where(dd < 0, (m + 0x8000) & 0xFFFF, m)
    return m, dd & 0xFFFF


def _wav2(plane: np.ndarray, mx: int, decode: bool) -> None:
    """ImfWav wav2Encode / wav2Decode on one (ny, nx) uint16 plane, in place; every level is vectorised over its 2x2 cells."""
    ny, nx = plane.shape
    w14 = mx < (1 << 14)
    top = _wav_levels(nx, ny)
    levels = []
    p = 1
    while 2 * p <= top:
        levels.append(p)
        p *= 2
    for p in (reversed(levels) if decode else levels):
        p2 = 2 * p
        ys, xs = np.arange(0, ny - p2 + 1, p2), np.arange(0, nx - p2 + 1, p2)
        yl, xl = (ys[-1] + p2 if len(ys) else 0), (xs[-1] + p2 if len(xs) else 0)
        Y, X = np.meshgrid(ys, xs, indexing="ij")
        i00, i01, i10, i11 = (Y, X), (Y, X + p), (Y + p, X), (Y + p, X + p)
        if decode:
            a, c = _wav_pairs(plane, i00, i10, w14, True)  # wdec(*px, *p10 -> i00, i10)
            b, d = _wav_pairs(plane, i01, i11, w14, True)
            tmp = plane.copy()
            tmp[i00], tmp[i10], tmp[i01], tmp[i11] = a, c, b, d
            r00, r01 = _wav_pairs(tmp, i00, i01, w14, True)
            r10, r11 = _wav_pairs(tmp, i10, i11, w14, True)
            plane[i00], plane[i01], plane[i10], plane[i11] = r00, r01, r10, r11
        else:
            a, b = _wav_pairs(plane, i00, i01, w14, False)  # wenc(*px, *p01 -> i00, i01)
            c, d = _wav_pairs(plane, i10, i11, w14, False)
            tmp = plane.copy()
            tmp[i00], tmp[i01], tmp[i10], tmp[i11] = a, b, c, d
            r00, r10 = _wav_pairs(tmp, i00, i10, w14, False)
            r01, r11 = _wav_pairs(tmp, i01, i11, w14, False)
            plane[i00], plane[i10], plane[i01], plane[i11] = r00, r10, r01, r11
        if nx & p:  # odd column: 1-D step along y
            ia, ib = (ys, np.full_like(ys, xl)), (ys + p, np.full_like(ys, xl))
            ra, rb = _wav_pairs(plane, ia, ib, w14, decode)
            plane[ia], plane[ib] = ra, rb
        if ny & p:  # odd row: 1-D step along x
            ia, ib = (np.full_like(xs, yl), xs), (np.full_like(xs, yl), xs + p)
            ra, rb = _wav_pairs(plane, ia, ib, w14, decode)
            plane[ia], plane[ib] = ra, rb


def _piz_unpack(comp: bytes, chans, w: int, n_lines: int) -> bytes:
    """PIZ block -> the uncompressed scanline block (per line: each channel's row).  chans = [(name, pixel_type)]."""
    sizes = [1 if pt == 1 else 2 for _, pt in chans]
    total = sum(sizes) * w * n_lines
    lo, hi = struct.unpack_from("<HH", comp, 0)
    bitmap = np.zeros(8192, np.uint8)
    p = 4
    if lo <= hi:
        bitmap[lo : hi + 1] = np.frombuffer(comp, np.uint8, hi - lo + 1, p)
        p += hi - lo + 1
    (length,) = struct.unpack_from("<i", comp, p)
    p += 4
    present = np.unpackbits(bitmap, bitorder="little").astype(bool)
    present[0] = True
    lut = np.zeros(65536, np.uint16)
    vals = np.nonzero(present)[0]
    lut[: len(vals)] = vals
    mx = len(vals) - 1
    buf = _huf_uncompress(comp[p : p + length], total)
    o = 0
    planes = []
    for sz in sizes:
        region = buf[o : o + sz * w * n_lines].reshape(n_lines, w, sz)
        for j in range(sz):
            plane = np.ascontiguousarray(region[:, :, j])
            _wav2(plane, mx, True)
            region[:, :, j] = plane
        planes.append(region)
        o += sz * w * n_lines
    out = bytearray()
    for y in range(n_lines):
        for region in planes:
            out += lut[region[y].reshape(-1)].astype("<u2").tobytes()
    return bytes(out)


def _piz_pack(raw: bytes, chans, w: int, n_lines: int) -> bytes:
    sizes = [1 if pt == 1 else 2 for _, pt in chans]
    src = np.frombuffer(raw, "<u2")
    regions = [np.zeros((n_lines, w, sz), np.uint16) for sz in sizes]
    o = 0
    for y in range(n_lines):
        for region, sz in zip(regions, sizes):
            region[y] = src[o : o + sz * w].reshape(w, sz)
            o += sz * w
    allv = np.concatenate([r.reshape(-1) for r in regions])
    present = np.zeros(65536, bool)
    present[allv] = True
    present[0] = False  # zero is implicit
    bitmap = np.packbits(present, bitorder="little")
    nz = np.nonzero(bitmap)[0]
    lo, hi = (int(nz[0]), int(nz[-1])) if len(nz) else (8191, 0)
    present[0] = True
    fwd = np.zeros(65536, np.uint16)
    vals = np.nonzero(present)[0]
    fwd[vals] = np.arange(len(vals), dtype=np.uint16)
    mx = len(vals) - 1
    parts = []
    for region, sz in zip(regions, sizes):
        region[...] = fwd[region]
        for j in range(sz):
            plane = np.ascontiguousarray(region[:, :, j])
            _wav2(plane, mx, False)
            region[:, :, j] = plane
        parts.append(region.reshape(-1))
    huf = _huf_compress(np.concatenate(parts))
    return struct.pack("<HH", lo, hi) + (bitmap[lo : hi + 1].tobytes() if lo <= hi else b"") + struct.pack("<i", len(huf)) + huf



def write_exr(path, rgb: np.ndarray, compression: str = "none", half: bool = False) -> None:
    """RGB float32 image -> scanline OpenEXR (channels B,G,R as FLOAT, or HALF with half=True);
    compression "none" | "rle" | "zips" | "zip" | "piz"."""
    rgb = np.asarray(rgb, np.float32)
    h, w, _ = rgb.shape
    if compression != "none" or half:
        return _write_exr_blocks(path, rgb, {"none": 0, "rle": 1, "zips": 2, "zip": 3, "piz": 4}[compression], half)

    def attr(name, typ, payload):
        return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<I", len(payload)) + payload

    chl = b"".join(n.encode() + b"\0" + struct.pack("<iBBBBii", 2, 0, 0, 0, 0, 1, 1) for n in ("B", "G", "R")) + b"\0"
    box = struct.pack("<iiii", 0, 0, w - 1, h - 1)
    hdr = (attr("channels", "chlist", chl) + attr("compression", "compression", b"\0") + attr("dataWindow", "box2i", box)
           + attr("displayWindow", "box2i", box) + attr("lineOrder", "lineOrder", b"\0") + attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
           + attr("screenWindowCenter", "v2f", struct.pack("<ff", 0.0, 0.0)) + attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0")
    head = struct.pack("<II", 20000630, 2) + hdr
    line = 8 + 12 * w
    table0 = len(head) + 8 * h
    with open(path, "wb") as f:
        f.write(head)
        f.write(np.arange(h, dtype="<u8").__mul__(line).__add__(table0).tobytes())
        for y in range(h):
            f.write(struct.pack("<iI", y, 12 * w))
            f.write(np.ascontiguousarray(rgb[y, :, ::-1].T, "<f4").tobytes())


def _exr_header(w, h, comp_code, pixel_type=2):
    def attr(name, typ, payload):
        return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<I", len(payload)) + payload

    chl = b"".join(n.encode() + b"\0" + struct.pack("<iBBBBii", pixel_type, 0, 0, 0, 0, 1, 1) for n in ("B", "G", "R")) + b"\0"
    box = struct.pack("<iiii", 0, 0, w - 1, h - 1)
    hdr = (attr("channels", "chlist", chl) + attr("compression", "compression", bytes([comp_code])) + attr("dataWindow", "box2i", box)
           + attr("displayWindow", "box2i", box) + attr("lineOrder", "lineOrder", b"\0") + attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
           + attr("screenWindowCenter", "v2f", struct.pack("<ff", 0.0, 0.0)) + attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0")
    return struct.pack("<II", 20000630, 2) + hdr


def _write_exr_blocks(path, rgb, comp_code, half):
    h, w, _ = rgb.shape
    lines_per_block = {0: 1, 1: 1, 2: 1, 3: 16, 4: 32}[comp_code]
    pt, dt = (1, "<f2") if half else (2, "<f4")
    chans = [("B", pt), ("G", pt), ("R", pt)]
    head = _exr_header(w, h, comp_code, pt)
    blocks = []
    for y0 in range(0, h, lines_per_block):
        rows = rgb[y0 : y0 + lines_per_block]
        raw = b"".join(np.ascontiguousarray(r[:, ::-1].T.astype(dt)).tobytes() for r in rows)  # per scanline: B row, G row, R row
        if comp_code == 0:
            comp = raw
        elif comp_code == 1:
            comp = _exr_rle_pack(raw)
        elif comp_code == 4:
            comp = _piz_pack(raw, chans, w, len(rows))
        else:
            comp = _exr_zip_pack(raw)
        if len(comp) >= len(raw):
            comp = raw  # the format stores a block raw when compression does not help
        blocks.append(struct.pack("<iI", y0, len(comp)) + comp)
    table0 = len(head) + 8 * len(blocks)
    offs, o = [], table0
    for b in blocks:
        offs.append(o)
        o += len(b)
    with open(path, "wb") as f:
        f.write(head)
        f.write(np.array(offs, "<u8").tobytes())
        for b in blocks:
            f.write(b)


def read_exr(path) -> np.ndarray:
    """Scanline EXR (uncompressed, RLE, ZIPS, ZIP or PIZ) with HALF / FLOAT / UINT channels -> (h, w, 3) float32 RGB (missing
    channels = 0).  The `image` crate the reference would open its skybox with (main.rs:94) reads the same set plus PXR24 / B44."""
    data = Path(path).read_bytes()
    magic, ver = struct.unpack_from("<II", data, 0)
    if magic != 20000630:
        raise ValueError(f"{path}: not an OpenEXR file")
    if ver & 0x200:
        raise ValueError(f"{path}: tiled EXR is not supported")
    p, attrs = 8, {}
    while data[p] != 0:
        e = data.index(b"\0", p); name = data[p:e].decode(); p = e + 1
        e = data.index(b"\0", p); typ = data[p:e].decode(); p = e + 1
        (ln,) = struct.unpack_from("<I", data, p); p += 4
        attrs[name] = (typ, data[p : p + ln]); p += ln
    p += 1
    comp = attrs["compression"][1][0]
    if comp not in (0, 1, 2, 3, 4):
        raise ValueError(f"{path}: EXR compression {comp} is not supported (uncompressed, RLE, ZIPS, ZIP and PIZ are; PXR24 / B44 / DWA are not)")
    lines_per_block = {0: 1, 1: 1, 2: 1, 3: 16, 4: 32}[comp]
    chans, q, cl = [], 0, attrs["channels"][1]
    while cl[q] != 0:
        e = cl.index(b"\0", q); nm = cl[q:e].decode(); q = e + 1
        (pt,) = struct.unpack_from("<i", cl, q); q += 16
        chans.append((nm, pt))
    x0, y0, x1, y1 = struct.unpack("<iiii", attrs["dataWindow"][1])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    n_blocks = (h + lines_per_block - 1) // lines_per_block
    offs = np.frombuffer(data, "<u8", n_blocks, p)
    out = np.zeros((h, w, 3), np.float32)
    line_bytes = sum({1: 2, 2: 4}.get(pt, 4) for _, pt in chans) * w
    for o in offs:
        y, size = struct.unpack_from("<iI", data, int(o))
        n_lines = min(lines_per_block, y1 + 1 - y)
        block = data[int(o) + 8 : int(o) + 8 + size]
        if comp and size < line_bytes * n_lines:  # a block that does not shrink is stored raw
            if comp == 1:
                block = _exr_rle_unpack(block, line_bytes * n_lines)
            elif comp == 4:
                block = _piz_unpack(block, chans, w, n_lines)
            else:
                block = _exr_zip_unpack(block, line_bytes * n_lines)
        q = 0
        for ly in range(n_lines):
            for nm, pt in chans:
                if pt == 2:
                    row = np.frombuffer(block, "<f4", w, q); q += 4 * w
                elif pt == 1:
                    row = np.frombuffer(block, "<f2", w, q).astype(np.float32); q += 2 * w
                else:
                    row = np.frombuffer(block, "<u4", w, q).astype(np.float32); q += 4 * w
                if nm in "RGB":
                    out[y + ly - y0, :, "RGB".index(nm)] = row
    return out


# ----------------------------------------------------------------------------------------------- bincode processed-asset cache
class _Bincode:
    """bincode 2 `standard().with_variable_int_encoding().with_big_endian()` (assets/mod.rs:135-137)."""

    def __init__(self, data: bytes):
        self.d, self.p = data, 0

    def take(self, n):
        b = self.d[self.p : self.p + n]
        if len(b) != n:
            raise ValueError("bincode: unexpected end of data")
        self.p += n
        return b

    def varint(self):
        b = self.take(1)[0]
        if b < 251:
            return b
        return int.from_bytes(self.take({251: 2, 252: 4, 253: 8, 254: 16}[b]), "big")

    def f16(self):
        return float(np.frombuffer(self.take(2), ">f2")[0])


@dataclass
class ProcessedMesh:
    """`Mesh` as serialised by `MeshSaver` (assets/mod.rs:118-125,299-314)."""

    meshlets: np.ndarray  # (n, 4) uint32: vertex_offset, triangle_offset, vertex_count, triangle_count
    materials: list  # Material
    vertices: np.ndarray  # (n, 8) float32
    indices: np.ndarray  # uint8, meshlet-local
    uploaded: bool


def read_processed_mesh(path, layout: str = "current") -> ProcessedMesh:
    """Decode a file of bevy's processed-asset cache (`imported_assets/Default/*.glb`).
    layout "current" = field order of assets/mod.rs:118-125 (meshlets, materials, vertices, indices, uploaded);
    layout "old"     = the order of the file the reference tree still ships: two leading vectors (both empty
                       there: meshlets and meshlet-local indices), materials, vertices, uploaded.
    Material = f16 BE metallic, f16 BE roughness, 3 x f16 BE colour, varint u16 texture offset (assets/mod.rs:61-73); the
    reference's decoder re-reads the metallic bytes as roughness (:88,110) -- that bug is not reproduced."""
    r = _Bincode(Path(path).read_bytes())

    def meshlets():
        n = r.varint()
        return np.array([[r.varint() for _ in range(4)] for _ in range(n)], np.uint32).reshape(n, 4)

    def materials():
        out = []
        for _ in range(r.varint()):
            metal, rough = r.f16(), r.f16()
            col = (r.f16(), r.f16(), r.f16())
            tex = r.varint()
            out.append(Material(col, metal, rough, (0.0, 0.0, 0.0), -1 if tex == 0xFFFF else tex))
        return out

    def vertices():
        n = r.varint()
        return np.frombuffer(r.take(32 * n), ">f4").reshape(n, 8).astype(np.float32)

    def bytes_vec():
        n = r.varint()
        return np.frombuffer(r.take(n), np.uint8).copy()

    if layout == "current":
        ml, mats, verts, idx = meshlets(), materials(), vertices(), bytes_vec()
    elif layout == "old":
        ml, idx = meshlets(), bytes_vec()
        mats, verts = materials(), vertices()
    else:
        raise ValueError("layout must be 'current' or 'old'")
    uploaded = bool(r.take(1)[0])
    if r.p != len(r.d):
        raise ValueError(f"bincode: {len(r.d) - r.p} trailing bytes (wrong layout?)")
    return ProcessedMesh(ml, mats, verts, idx, uploaded)


def write_processed_mesh(path, pm: ProcessedMesh) -> None:
    """Serialise in the CURRENT layout (MeshSaver, assets/mod.rs:299-314)."""

    def varint(v):
        if v < 251:
            return bytes([v])
        for tag, n in ((251, 2), (252, 4), (253, 8)):
            if v < (1 << (8 * n)):
                return bytes([tag]) + int(v).to_bytes(n, "big")
        raise ValueError("varint too large")

    out = bytearray(varint(len(pm.meshlets)))
    for m in pm.meshlets:
        for v in m:
            out += varint(int(v))
    out += varint(len(pm.materials))
    for m in pm.materials:
        out += np.array([m.metalic_factor, m.roughness_factor, *m.color], ">f2").tobytes()
        out += varint(0xFFFF if m.texture_offset < 0 else m.texture_offset)
    out += varint(len(pm.vertices)) + np.ascontiguousarray(pm.vertices, ">f4").tobytes()
    out += varint(len(pm.indices)) + bytes(np.asarray(pm.indices, np.uint8))
    out += bytes([1 if pm.uploaded else 0])
    Path(path).write_bytes(bytes(out))


def load_bluenoise(path=None) -> np.ndarray:
    """resources/bluenoise.png (256x256 RGBA8, shipped with the reference as data) -> (256,256,4) uint8."""
    from PIL import Image

    path = Path(path) if path else Path(__file__).resolve().parent.parent / "resources" / "bluenoise.png"
    return np.ascontiguousarray(np.array(Image.open(path).convert("RGBA"), np.uint8))
