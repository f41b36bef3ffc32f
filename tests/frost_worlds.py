"""Scenes of the rough-transmission tests (tests/test_frost_cpu.py, tests/test_frost.py,
tests/golden/gen_frost_ref.py).  They are the worlds of glass_worlds and pane_worlds with roughness on their glass: those modules build
glass at roughness 1 (it plays no part there), so every world here sets the roughness it means."""
import numpy as np

import glass_worlds as GW
import integrator_worlds as IW
import lens_worlds as LW
import pane_worlds as PN
import punctual_worlds as PW
from raytracer3_amd import assets
from raytracer3_amd.assets import Material, MeshBuilder

F_NEE_SKY, F_SPECULAR, F_FACEFORWARD = IW.F_NEE_SKY, IW.F_SPECULAR, IW.F_FACEFORWARD
F_NEE_EMISSIVE = 32  # RT3_F_NEE_EMISSIVE of include/rt3.h


def set_roughness(mesh, **by_name):
    """the roughness factor of the named geometries, in place; returns the mesh"""
    for name, value in by_name.items():
        mesh.geometries["roughness"][mesh.names.index(name)] = value
    return mesh


def smooth(mesh):
    """every transmissive geometry at roughness 0: nothing for the build to classify"""
    mesh.geometries["roughness"][mesh.transmission["transmission"] > 0] = 0.0
    return mesh


# ---------------------------------------------------------------------------------------------------------------- the index-matched slab
SLAB_ALPHA = 0.5


def matched_slab(tilt_deg):
    """glass_worlds' solid slab at ior 1 and roughness SLAB_ALPHA under a constant sky: the direction never changes and each of the two
    crossings weighs G1(cos theta, alpha^2).  Returns (mesh, unit normal of the front face)."""
    mesh, normal, _ = GW.slab_world(ior=1.0, tilt_deg=tilt_deg)
    return set_roughness(mesh, slab_front=SLAB_ALPHA, slab_back=SLAB_ALPHA), normal


# ---------------------------------------------------------------------------------------------------------------- the edge behind a pane
EDGE_PX, EDGE_ALPHA, EDGE_PANE_DEPTH, EDGE_ROW = 30.3, 0.2, 3.0, 24
EDGE_WINDOW = (64, 48)


def edge_world(alpha):
    """glass_worlds' emissive half-plane (its edge at pixel column EDGE_PX, depth 6) behind an index-matched thin pane of roughness alpha that
    reaches far past the view, at depth EDGE_PANE_DEPTH"""
    mesh, _, _ = GW.slab_world(with_slab=False, emitter_edge_px=EDGE_PX)
    mb = MeshBuilder()
    W, H = GW.WINDOW
    GW._facing_quad(mb, "pane", -3.0 * W, 4.0 * W, -3.0 * H, 4.0 * H, EDGE_PANE_DEPTH, Material((1.0, 1.0, 1.0), 0.0, alpha, transmission=1.0, ior=1.0, thin_walled=1))
    return join(mesh, mb.build())


def join(a, b):
    """the geometries of mesh b behind those of mesh a (no textures, no lights)"""
    g = b.geometries.copy()
    g["index_offset"] += len(a.indices)
    g["vertex_offset"] += len(a.vertices)
    mesh = assets.Mesh(np.ascontiguousarray(np.concatenate([a.vertices, b.vertices]), np.float32),
                       np.ascontiguousarray(np.concatenate([a.indices, b.indices]), np.uint32), np.concatenate([a.geometries, g]),
                       np.concatenate([a.prim_counts, b.prim_counts]).astype(np.uint32), a.names + b.names)
    mesh.transmission[:] = np.concatenate([a.transmission, b.transmission])
    return mesh


# ---------------------------------------------------------------------------------------------------------------- the fixture's room
ROOM_BLOCK_ALPHA, ROOM_PANE_ALPHA = 0.3, 0.2
# name -> (flags of the reference, bounces, specular material set, transmission, reference samples per pixel, seed, frames of the code under
# test, flags the code under test adds: emitter sampling estimates the same integral)
ROOM_CASES = {
    "frost_b4": (F_FACEFORWARD | F_NEE_SKY, 4, False, 1.0, 4096, 381, 16, 0),
    "frost_spec_b6": (F_SPECULAR | F_FACEFORWARD | F_NEE_SKY, 6, True, 1.0, 4096, 382, 16, F_NEE_EMISSIVE),
}
ROOM_LENS = GW.ROOM_LENS


def frost_room(specular=False, tau=1.0):
    """glass_worlds.glass_room() with its solid block at roughness 0.3 and its thin-walled pane at roughness 0.2"""
    return set_roughness(GW.glass_room(specular, tau), block=ROOM_BLOCK_ALPHA, pane=ROOM_PANE_ALPHA)


def textured_room(specular=True, tau=0.5, factor=ROOM_BLOCK_ALPHA, value=0, texture=0):
    """frost_room with a smooth pane whose block has the roughness factor `factor` and names a metallic-roughness texture (index `texture`;
    -1: none, the texture stays in the mesh) with G = `value` in every texel.  The roughness at a hit is factor x value / 255: with
    (factor > 0, value 0) and with (factor 0, any value) the block is classified as frosted and every hit on it has roughness 0"""
    mesh = frost_room(specular, tau)
    smooth(mesh)
    k = mesh.names.index("block")
    mesh.geometries["roughness"][k] = factor
    mesh.material_textures["metallic_roughness_texture"][k] = texture
    if texture < 0:  # another geometry keeps the side table alive: the floor, at its own roughness
        mesh.material_textures["metallic_roughness_texture"][mesh.names.index("floor")] = 0
        value = 255
    mesh.textures = [np.ascontiguousarray(np.tile(np.array([0, value, 255, 255], np.uint8), (4, 4, 1)))]
    return mesh


# ---------------------------------------------------------------------------------------------------------------- panes under a light
PANE_FROSTED, PANE_CLEAR = PN.PANE, ((0.5, 1.9), 3.0, (-1.6, -0.2))
PANE_ALPHA = 0.2


PANE_EMITTER = ((-1.0, 1.5), 5.0, (-1.5, 0.0))  # an emissive quad above both panes, facing down


def two_panes(textured=False, glass=True, emitter=False):
    """pane_worlds' floor under its directional light with two thin-walled panes side by side above the camera: `frosted` (roughness
    PANE_ALPHA) and `clear` (roughness 0); glass = False: the floor alone; emitter: with PANE_EMITTER above the panes"""
    mb = MeshBuilder()
    PW._quad(mb, "floor", (-3.0, 3.0), 0.0, (-3.0, 3.0), Material(PN.ALBEDO, 0.0, 1.0))
    if emitter:
        (x0, x1), h, (z0, z1) = PANE_EMITTER
        mb.add("lamp", [[x0, h, z0], [x1, h, z0], [x1, h, z1], [x0, h, z1]], np.tile([0.0, -1.0, 0.0], (4, 1)), None, [[0, 1, 2], [0, 2, 3]],
               Material((0.0, 0.0, 0.0), 0.0, 1.0, emission=(1.0, 0.8, 0.6)))
    for name, rect, rough in (("frosted", PANE_FROSTED, PANE_ALPHA), ("clear", PANE_CLEAR, 0.0)) if glass else ():
        PW._quad(mb, name, rect[0], rect[1], rect[2], Material(PN.TINT, 0.0, rough, transmission=1.0, ior=PN.IOR, thin_walled=1), uv=True)
    mesh = mb.build()
    mesh.lights = assets.lights_array([PN.LIGHTS["directional"]])
    if textured:  # the floor names a metallic-roughness texture of full roughness: the side table of section 4j, the same surface
        mesh.material_textures["metallic_roughness_texture"][mesh.names.index("floor")] = 0
        mesh.textures = [np.ascontiguousarray(np.tile(np.array([0, 255, 0, 255], np.uint8), (2, 2, 1)))]
    return mesh


def constant_sky(rgb=GW.SKY_L):
    return LW.constant_sky(rgb)
