"""Skins shared by tests/test_skin_cpu.py and tests/test_skin.py: random rows that cover the rule's cases, palettes,
glTF files written by hand, and the posed vertex buffer of scenes.skinned_arm().  Test infrastructure only."""
import copy
import json
import struct

import numpy as np

import ref_skin as rs
from support import rotation

F = np.float32


def palette(n_joints, seed=1, spread=1.0):
    """(n_joints, 4, 4) float32: a rotation, a scale near 1 and a translation each; joint 0 is the exact identity"""
    rng = np.random.default_rng(seed)
    out = np.tile(np.eye(4), (n_joints, 1, 1))
    for k in range(1, n_joints):
        out[k, :3, :3] = rotation(rng) * rng.uniform(0.7, 1.4)
        out[k, :3, 3] = rng.uniform(-spread, spread, 3)
    return out.astype(F)


def rows(n, n_joints, n_targets=0, with_dnrm=False, seed=0):
    """a dict of one skin's arrays over n vertices.  Row r's weights follow r % 6: one weight (in slot 2), two, four, two with the zero slots
    pointing at the last joint, all four zero, and four that do not sum to 1.  Target weights: 0 at every second target from the second
    on (a_t = 0 between non-zero ones when there are three or more)."""
    rng = np.random.default_rng(seed)
    rest = np.concatenate([rng.uniform(-2.0, 2.0, (n, 3)), rng.normal(size=(n, 3)), rng.uniform(0, 1, (n, 2))], 1).astype(F)
    joints = rng.integers(0, n_joints, (n, 4)).astype(np.uint16)
    w = rng.uniform(0.05, 1.0, (n, 4))
    kind = np.arange(n) % 6
    w[kind == 0] *= [0, 0, 1, 0]
    w[kind == 1] *= [1, 0, 0, 1]
    w[kind == 3] *= [0, 1, 1, 0]
    w[kind == 4] = 0
    joints[kind == 3, 0] = joints[kind == 3, 3] = n_joints - 1
    joints[kind == 4] = n_joints - 1
    norm = kind != 5
    w[norm] = w[norm] / np.maximum(w[norm].sum(1, keepdims=True), 1e-30)
    out = dict(rest=rest, joints=joints, weights=w.astype(F), n_joints=n_joints, dpos=None, dnrm=None, a=None)
    if n_targets:
        out["dpos"] = rng.uniform(-0.3, 0.3, (n_targets, n, 3)).astype(F)
        out["dnrm"] = rng.uniform(-0.3, 0.3, (n_targets, n, 3)).astype(F) if with_dnrm else None
        a = rng.uniform(-1.0, 1.5, n_targets)
        a[1::2] = 0.0
        out["a"] = a.astype(F)
    return out


def pose_rows(r, pal, a=None, dtype=F):
    return rs.pose(r["rest"], r["joints"], r["weights"], pal, r["dpos"], r["dnrm"], r["a"] if a is None else a, dtype=dtype)


def arm_vertices(mesh, t, animation=0):
    """mesh.vertices with every skin's range replaced by ref_skin.pose at time t"""
    v = np.ascontiguousarray(mesh.vertices, F).copy()
    for s, (pal, w) in zip(mesh.skins, mesh.pose(t, animation)):
        v[s.first_vertex:s.first_vertex + len(s.rest)] = rs.pose(s.rest, s.joints, s.weights, pal, s.target_dpos if len(s.target_dpos) else None, s.target_dnrm, w)
    return v


def posed(mesh, t, animation=0):
    m = copy.copy(mesh)
    m.vertices = arm_vertices(mesh, t, animation)
    return m


# ---- glTF by hand
def read_glb(path):
    data = open(path, "rb").read()
    n = struct.unpack_from("<I", data, 12)[0]
    return json.loads(data[20:20 + n].decode()), data[20 + n + 8:]


def write_raw_glb(path, doc, blob):
    js = json.dumps(doc, separators=(",", ":")).encode()
    js += b" " * ((-len(js)) % 4)
    blob = bytes(blob) + b"\0" * ((-len(blob)) % 4)
    doc_len = 12 + 8 + len(js) + 8 + len(blob)
    with open(path, "wb") as f:
        f.write(struct.pack("<4sII", b"glTF", 2, doc_len) + struct.pack("<I4s", len(js), b"JSON") + js + struct.pack("<I4s", len(blob), b"BIN\0") + blob)


class GlbBuilder:
    """a glTF document assembled accessor by accessor"""

    def __init__(self):
        self.blob, self.views, self.accessors = bytearray(), [], []

    def acc(self, arr, typ, comp, normalized=False):
        arr = np.ascontiguousarray(arr)
        self.views.append({"buffer": 0, "byteOffset": len(self.blob), "byteLength": arr.nbytes})
        self.blob += arr.tobytes() + b"\0" * ((-arr.nbytes) % 4)
        a = {"bufferView": len(self.views) - 1, "componentType": comp, "count": arr.size if typ == "SCALAR" else len(arr), "type": typ}
        if normalized:
            a["normalized"] = True
        self.accessors.append(a)
        return len(self.accessors) - 1

    def write(self, path, **doc):
        doc.update(asset={"version": "2.0"}, accessors=self.accessors, bufferViews=self.views, buffers=[{"byteLength": len(self.blob)}])
        write_raw_glb(path, doc, self.blob)


def triangle_rig(path, interpolation="LINEAR", joints_dtype=np.uint8, weights_dtype=np.uint8, mesh_matrix=None):
    """One triangle skinned to two joints under a scaled parent: nodes 0 parent (scale 2, translation (1, 0, 0)), 1 joint A (child of 0,
    translation (0, 1, 0)), 2 joint B (child of 1, translation (0, 0.5, 0), rotated a quarter turn about z between t = 1 and t = 3), 3 the
    mesh.  JOINTS_0 as `joints_dtype`, WEIGHTS_0 as `weights_dtype` (normalised integers or float32).  Returns the document's pieces."""
    b = GlbBuilder()
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], "<f4")
    nrm = np.tile(np.array([0, 0, 1], "<f4"), (3, 1))
    comp = {np.uint8: 5121, np.uint16: 5123, np.float32: 5126}
    top = {np.uint8: 255, np.uint16: 65535, np.float32: 1.0}[weights_dtype]
    w = np.array([[top, 0, 0, 0], [0, top, 0, 0], [top // 5 if top > 1 else 0.2, top - top // 5 if top > 1 else 0.8, 0, 0]], weights_dtype)
    j = np.array([[0, 1, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0]], joints_dtype)
    ibm = np.tile(np.eye(4, dtype="<f4"), (2, 1, 1))
    ibm[0, :3, 3] = (-0.5, 0.25, 0)
    ibm[1, :3, 3] = (0, -1, 0.5)
    prim = {"attributes": {"POSITION": b.acc(pos, "VEC3", 5126), "NORMAL": b.acc(nrm, "VEC3", 5126), "JOINTS_0": b.acc(j, "VEC4", comp[joints_dtype]),
                           "WEIGHTS_0": b.acc(w, "VEC4", comp[weights_dtype], normalized=weights_dtype != np.float32)},
            "indices": b.acc(np.array([0, 1, 2], "<u4"), "SCALAR", 5125)}
    half = float(np.sqrt(0.5))
    times = b.acc(np.array([1.0, 3.0], "<f4"), "SCALAR", 5126)
    n_keys = 6 if interpolation == "CUBICSPLINE" else 2
    quats = np.zeros((n_keys, 4), "<f4")
    quats[1 if n_keys == 6 else 0] = (0, 0, 0, 1)
    quats[4 if n_keys == 6 else 1] = (0, 0, half, half)
    mesh_node = {"mesh": 0, "skin": 0}
    if mesh_matrix is not None:
        mesh_node["matrix"] = [float(x) for x in np.asarray(mesh_matrix, np.float64).T.ravel()]
    b.write(path, scene=0, scenes=[{"nodes": [0, 3]}],
            nodes=[{"scale": [2, 2, 2], "translation": [1, 0, 0], "children": [1]}, {"translation": [0, 1, 0], "children": [2]},
                   {"translation": [0, 0.5, 0], "rotation": [0, 0, 0, 1]}, mesh_node],
            meshes=[{"name": "tri", "primitives": [prim]}],
            skins=[{"joints": [1, 2], "inverseBindMatrices": b.acc(ibm.transpose(0, 2, 1), "MAT4", 5126)}],
            animations=[{"samplers": [{"input": times, "output": b.acc(quats, "VEC4", 5126), "interpolation": interpolation}],
                         "channels": [{"sampler": 0, "target": {"node": 2, "path": "rotation"}}]}])
    return dict(pos=pos, weights=w.astype(np.float64) / top, ibm=ibm.astype(np.float64))
