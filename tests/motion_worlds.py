"""Worlds of moving instances shared by tests/test_motion_cpu.py and tests/test_motion.py.  Test infrastructure only."""
import math

import numpy as np

from raytracer3_amd import scenes
from raytracer3_amd.assets import Material, MeshBuilder
from support import translate

F = np.float32
EYE = np.eye(4, dtype=F)


def rot_y(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], np.float64)


def rot_z(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)


def scale(x, y, z):
    return np.diag([x, y, z, 1.0])


def about(center, m):
    """the matrix `m` applied around `center` instead of the origin"""
    return translate(*center) @ m @ translate(*(-np.asarray(center, np.float64)))


def f32(m):
    return np.asarray(m, np.float64).astype(F)


def parity_world():
    """(mesh, instances, previous transforms): the Cornell room without its left wall (pixels that miss), its two blocks at their own
    places and the tall block placed six more times.  Of the instances some did not move, one was translated, one rotated, one has a
    non-uniform scale in both frames, one had the identity as its previous matrix and one has it as its current matrix."""
    room = scenes.cornell()
    t = room.names.index("tall")
    c = np.array([-0.35, 0.6, -0.35])  # the tall block's centre
    small = scale(0.45, 0.5, 0.45)
    cur = [
        (0, 3, EYE),                                                             # floor, ceiling, back wall: unmoved
        (room.names.index("right"), 2, EYE),                                     # right wall and the light panel: unmoved
        (t, 1, EYE),                                                             # the tall block where it stands: current matrix = identity
        (t + 1, 1, f32(translate(0.05, 0.0, 0.1))),                              # the short block: previous matrix = identity
        (t, 1, f32(translate(0.9, 0.0, 0.5) @ about(c, small))),                 # unmoved, placed
        (t, 1, f32(translate(0.2, 0.55, 0.9) @ about(c, small))),                # translated
        (t, 1, f32(translate(0.75, 0.9, -0.2) @ about(c, rot_y(25.0) @ small))), # rotated
        (t, 1, f32(translate(0.3, 1.2, 0.3) @ about(c, rot_z(10.0) @ scale(0.7, 0.25, 0.4)))),  # non-uniform scale, moved
        (t, 2, f32(translate(-0.2, 0.0, 1.4) @ scale(0.6, 0.6, 0.6))),           # a two-geometry run (tall, short), translated
    ]
    prev = [
        EYE, EYE,
        f32(translate(-0.06, 0.0, 0.03) @ about(c, rot_y(-4.0))),
        EYE,
        cur[4][2].copy(),
        f32(translate(0.14, 0.55, 0.93) @ about(c, small)),
        f32(translate(0.75, 0.9, -0.2) @ about(c, rot_y(19.0) @ small)),
        f32(translate(0.33, 1.16, 0.3) @ about(c, rot_z(6.0) @ scale(0.72, 0.25, 0.38))),
        f32(translate(-0.26, 0.0, 1.38) @ scale(0.6, 0.6, 0.6)),
    ]
    return room, cur, prev


PARITY_CAMERA = dict(position=(0.0137, 1.0071, 3.4), direction=(-0.08, -0.0033, -1.0), fov_deg=48.0)


def moving_world(k, n_placed=6):
    """(mesh, instances of frame k): the Cornell room with its blocks (identity, never moving) and the tall block placed `n_placed` more
    times, shrunk: the even ones translate by 2.5 cm a frame, number 1 turns by 3 degrees a frame about its own axis, the others stand."""
    room = scenes.cornell()
    t = room.names.index("tall")
    c = np.array([-0.35, 0.6, -0.35])
    rng = np.random.default_rng(11)
    inst = [(0, len(room.geometries), EYE)]
    for j in range(n_placed):
        place = np.array([rng.uniform(-0.1, 0.9), rng.uniform(0.0, 0.9), rng.uniform(0.3, 1.4)])
        turn = rng.uniform(0.0, 90.0)
        m = translate(*place) @ about(c, rot_y(turn) @ scale(0.4, 0.45, 0.4))
        if j == 1:
            m = translate(*place) @ about(c, rot_y(turn + 3.0 * k) @ scale(0.4, 0.45, 0.4))
        elif j % 2 == 0:
            d = np.array([0.025, 0.0, 0.0]) if j % 4 == 0 else np.array([0.0, 0.015, -0.02])
            m = translate(*(k * d)) @ m
        inst.append((t, 1, f32(m)))
    return room, inst


def moving_world_moved(n_placed=6):
    """indices (into the instance list) of moving_world's instances that move"""
    return [1 + j for j in range(n_placed) if j == 1 or j % 2 == 0]


def sliding_quad(shift):
    """(mesh, instances): a wall at z = 0 facing +z and a 1 x 1 quad at z = 1 in front of it (geometry 1, its own instance) slid by
    `shift` = (dx, dy) in its own plane, under a lamp above and in front of both.  The quad's colour differs from the wall's."""
    mb = MeshBuilder()
    wall, quad = Material((0.7, 0.7, 0.7)), Material((0.2, 0.5, 0.8))
    mb.add("wall", *scenes._grid([-4, -3, 0], [8, 0, 0], [0, 6, 0], 2, 2), wall)
    mb.add("quad", *scenes._grid([-0.5, -0.5, 1], [1, 0, 0], [0, 1, 0], 2, 2), quad)
    mb.add("lamp", *scenes._grid([-2, 2.5, 0.5], [4, 0, 0], [0, 0, 4], 1, 1), Material((0.8, 0.8, 0.8), emission=(2.0, 2.0, 2.0)))  # faces down
    mesh = mb.build()
    return mesh, [(0, 1, EYE), (1, 1, f32(translate(shift[0], shift[1], 0.0))), (2, 1, EYE)]


QUAD_CAMERA = dict(position=(0.0, 0.0, 4.0), direction=(0.0, 0.0, -1.0), fov_deg=50.0)
