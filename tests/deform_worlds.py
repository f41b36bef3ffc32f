"""Worlds of deforming meshes shared by tests/test_deform_cpu.py and tests/test_deform.py.  Test infrastructure only."""
import copy
import math

import numpy as np

import motion_worlds as mw
from raytracer3_amd import scenes
from raytracer3_amd.assets import Material, MeshBuilder

F = np.float32
EYE = mw.EYE
CLOTH_CELLS = 8
BENDER_HEIGHT, BEND2_HEIGHT = 0.9, 0.5

# the camera of motion_worlds.PARITY_CAMERA: it looks a little to the left, where the wall is missing
CAMERA = dict(position=(0.0137, 1.0071, 3.4), direction=(-0.08, -0.0033, -1.0), fov_deg=48.0)


def rest_mesh():
    """The Cornell room without its left and front walls (pixels that miss) and, in it: a cloth (an 8 x 8 grid hanging in front of the back
    wall), two blocks that bend (`bender`, `bend2`), a block that only moves (`mover`) and two small blocks that never change place
    (`resent`, `normals`)."""
    white, green = Material((0.73, 0.73, 0.73)), Material((0.12, 0.45, 0.15))
    light = Material((0.78, 0.78, 0.78), emission=(1.4, 1.2, 0.9))
    mb = MeshBuilder()
    n = 4
    mb.add("floor", *scenes._grid([-1, 0, -1], [0, 0, 5], [2, 0, 0], n, n), white)
    mb.add("ceiling", *scenes._grid([-1, 2, -1], [2, 0, 0], [0, 0, 5], n, n), white)
    mb.add("back", *scenes._grid([-1, 0, -1], [2, 0, 0], [0, 2, 0], n, n), white)
    mb.add("right", *scenes._grid([1, 0, -1], [0, 0, 5], [0, 2, 0], n, n), green)
    mb.add("panel", *scenes._grid([-0.35, 1.995, -0.35], [0.7, 0, 0], [0, 0, 0.7], 2, 2), light)
    mb.add("cloth", *scenes._grid([-0.95, 0.85, -0.6], [0.7, 0, 0], [0, 0.9, 0], CLOTH_CELLS, CLOTH_CELLS), Material((0.2, 0.5, 0.8)))
    scenes._box(mb, "bender", [-0.18, 0.0, -0.18], [0.18, BENDER_HEIGHT, 0.18], Material((0.8, 0.6, 0.2)), n=3)
    scenes._box(mb, "bend2", [-0.2, 0.0, -0.2], [0.2, BEND2_HEIGHT, 0.2], Material((0.7, 0.3, 0.3)), n=2)
    scenes._box(mb, "mover", [-0.2, 0.0, -0.2], [0.2, 1.0, 0.2], white, n=2)
    scenes._box(mb, "resent", [-0.85, 0.0, 0.9], [-0.6, 0.35, 1.15], white, n=1)
    scenes._box(mb, "normals", [-0.45, 0.0, 1.3], [-0.2, 0.3, 1.55], white, n=1)
    return mb.build()


REST = rest_mesh()


def vertex_range(mesh, name):
    """[first, end) of the geometry's own vertices in the vertex buffer (MeshBuilder gives every geometry a range of its own)"""
    g = mesh.names.index(name)
    first = int(mesh.geometries["vertex_offset"][g])
    end = int(mesh.geometries["vertex_offset"][g + 1]) if g + 1 < len(mesh.geometries) else len(mesh.vertices)
    return first, end


def mesh_at(k):
    """the mesh of frame k: the cloth waves (out of its plane and a little within it), the two blocks bend sideways with their height, one
    normal word of `normals` changes from frame to frame, everything else keeps its words"""
    m = copy.copy(REST)
    v = REST.vertices.astype(np.float64)
    a, b = vertex_range(REST, "cloth")
    s, t = (v[a:b, 0] + 0.95) / 0.7, (v[a:b, 1] - 0.85) / 0.9
    v[a:b, 2] += 0.06 * np.sin(2 * math.pi * (1.5 * s + 0.11 * k)) * (1.0 - 0.6 * t)
    v[a:b, 0] += 0.03 * np.sin(2 * math.pi * (t + 0.07 * k))
    for name, height, amp in (("bender", BENDER_HEIGHT, 0.22), ("bend2", BEND2_HEIGHT, -0.15)):
        a, b = vertex_range(REST, name)
        h = v[a:b, 1] / height
        v[a:b, 0] += amp * math.sin(0.35 * k + 0.4) * h * h
    a, b = vertex_range(REST, "normals")
    v[a, 4] = 0.5 + 0.01 * k  # a normal word only (the G-buffer normal of that corner turns a little: it is not a position)
    m.vertices = np.ascontiguousarray(v, F)
    return m


def instances_at(k):
    """the placements of frame k: the room, the cloth and the two still blocks under the identity; `bender` placed twice (one placement
    turns and slides, the other stands, scaled); `bend2` and `mover` slide"""
    g = REST.names.index
    return [
        (0, 5, EYE),                                                                              # the room: unmoved
        (g("cloth"), 1, EYE),                                                                     # deformed, identity, unmoved
        (g("bender"), 1, mw.f32(mw.translate(0.52 + 0.02 * k, 0.0, -0.35) @ mw.rot_y(17.0 + 3.0 * k))),  # deformed and moved
        (g("bender"), 1, mw.f32(mw.translate(-0.1, 0.0, 0.35) @ mw.scale(0.8, 0.9, 0.8))),         # the same mesh again: deformed, unmoved
        (g("bend2"), 1, mw.f32(mw.translate(0.5, 0.0, 0.8 + 0.015 * k))),                          # deformed and moved
        (g("mover"), 1, mw.f32(mw.translate(-0.62 + 0.025 * k, 0.0, 0.3) @ mw.rot_y(30.0))),        # moved only
        (g("resent"), 2, EYE),                                                                    # `resent` and `normals`: unmoved
    ]


def world(k):
    """(mesh, instances) of frame k"""
    return mesh_at(k), instances_at(k)


def parity_world():
    """(mesh, previous vertices, instances, previous transforms) of frame 1 against frame 0, with `bend2`'s previous matrix replaced by
    the identity"""
    mesh, inst = world(1)
    prev = [m for _, _, m in instances_at(0)]
    prev[4] = EYE.copy()
    return mesh, mesh_at(0).vertices, inst, prev


def slid_quad(shift):
    """motion_worlds.sliding_quad with the quad moved by its VERTICES instead of its matrix: (mesh at rest, mesh slid, instances)"""
    rest, inst = mw.sliding_quad((0.0, 0.0))
    slid = copy.copy(rest)
    v = rest.vertices.copy()
    a, b = vertex_range(rest, "quad")
    v[a:b, 0] += F(shift[0])
    v[a:b, 1] += F(shift[1])
    slid.vertices = v
    return rest, slid, inst
