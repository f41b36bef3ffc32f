"""Frame description: the path-tracing counterpart of `renderer::commands` (src/renderer/mod.rs:65-106) and of the
`Camera` component (src/components/camera.rs:23-59), plus the tile-partitioned multi-GPU frame (north_star).

Per frame, three passes exactly as the old shaders were wired:
  RayTracingPass("gbuffer")        -> packed G-buffer + depth                 shaders/old/gbuffer.slang
  RayTracingPass("refrence_mode")  -> Light (RGBA32F linear radiance)          shaders/old/refrence_mode.slang
  ComputePass("postprocess")       -> display image (AgX)                      shaders/old/postprocess.slang
(or, on request, RayTracingPass("adaptive") in its place: the same paths up to a noise threshold),
with, on request, ComputePass("temporal") and / or ComputePass("denoise") between the last two (no reference counterpart: the reprojected
accumulation of DESIGN.md section 4g and the a-trous filter of section 4f), and RayTracingPass("motion") in front of "temporal" in a frame
whose instances moved (section 4h) or whose vertices were updated (section 4i),
and, as a second frame description, the probe-GI chain of the old shaders (`probe_commands`):
  gbuffer -> structured_importance_sampling -> trace_probes -> spherical_harmonic_conversion -> interpolate_probes
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math

import numpy as np

from . import _lib as L
from .render_graph import IMPORTED, ComputePass, Context, DispatchSize, ImageSize, RayTracingPass, RenderGraph, WorkSize2D

DEFAULT_FLAGS = L.F_NEE_SKY | L.F_BLUENOISE | L.F_FACEFORWARD | L.F_SPECULAR  # the full north_star estimator


class Camera:
    """components/camera.rs:23-59.  `fov` in radians, like the reference (`65.0_f32.to_radians()`, main.rs:72)."""

    def __init__(self, position, direction, fov, aspect_ratio, z_near=0.1, z_far=1000.0):
        d = np.asarray(direction, np.float32)
        self.position = np.asarray(position, np.float32)
        self.direction = d / np.float32(np.linalg.norm(d))  # Camera::new normalises, camera.rs:43
        self.fov, self.aspect_ratio, self.z_near, self.z_far = float(np.float32(fov)), float(np.float32(aspect_ratio)), z_near, z_far

    def gconst(self, window) -> L.GConst:
        """view_matrix / projection_matrix (camera.rs:52-58) + the GConst fill of renderer/mod.rs:72-78."""
        g = L.GConst()
        p = (C.c_float * 3)(*[float(x) for x in self.position])
        d = (C.c_float * 3)(*[float(x) for x in self.direction])
        L.load().rt3_camera_gconst(p, d, self.fov, self.aspect_ratio, self.z_near, self.z_far, float(window[0]), float(window[1]), C.byref(g))
        return g

    def view_matrix(self, window=(1, 1)):
        return np.array(self.gconst(window).view[:], np.float32).reshape(4, 4).T

    def projection_matrix(self, window=(1, 1)):
        return np.array(self.gconst(window).proj[:], np.float32).reshape(4, 4).T


GUIDE_IMAGES = (("position", "GuidePosition"), ("normal", "GuideNormal"), ("albedo", "GuideAlbedo"), ("emission", "GuideEmission"))


# the second set: the guide images of the previous temporal frame.  The two sets trade names once per guided temporal
# frame, as History / PrevHistory do (TEMPORAL_SWAPS)
PREV_GUIDE_IMAGES = tuple((key, "Prev" + name) for key, name in GUIDE_IMAGES)
GUIDE_SWAPS = tuple((name, "Prev" + name) for _, name in GUIDE_IMAGES)


def scene_medium(mesh, sigma_s, sigma_a=0.0, g=0.0, margin=0.0, box=None):
    """An L.Medium for PathTracer.set_medium: scattering and absorption coefficients (a number, or one per colour channel) in a box that
    defaults to the bounds of the mesh's vertices (as uploaded: instance transforms are not followed), grown by `margin` world units."""
    if box is None:
        p = np.asarray(mesh.vertices, np.float64)[:, :3]
        lo, hi = p.min(0) - margin, p.max(0) + margin
        hi = np.maximum(hi, lo + 1e-3)  # a flat world still gets a box
    else:
        lo, hi = np.asarray(box[0], np.float64), np.asarray(box[1], np.float64)
    return L.Medium(sigma_a, sigma_s, g, tuple(lo), tuple(hi))


def guide_images(rg):
    """the four guide images of a lens frame as a dict {position, normal, albedo, emission} of handles: what
    ctx.set_guide_output and ctx.set_denoise_guide_input take"""
    return {key: rg.image(ImageSize.FullScreen, L.FORMAT_R32G32B32A32_SFLOAT, name) for key, name in GUIDE_IMAGES}


def prev_guide_images(rg):
    """the guide images of the previous temporal frame, like guide_images(): the second argument of ctx.set_temporal_guide_input"""
    return {key: rg.image(ImageSize.FullScreen, L.FORMAT_R32G32B32A32_SFLOAT, name) for key, name in PREV_GUIDE_IMAGES}


def guide_prev_position_image(rg):
    """the fifth guide image of a lens frame, the samples' mean previous position: what
    ctx.set_guide_motion_output and ctx.set_temporal_guide_motion_input take"""
    return rg.image(ImageSize.FullScreen, L.FORMAT_R32G32B32A32_SFLOAT, "GuidePrevPosition")


def frame_nodes(rg, gconst, postprocess=True, denoise=False, temporal=False, motion=False, adaptive=False, *,
                gbuffer_names=("gbuffer", "gbuffer_depth"), gbuffer_node=True, trace=True, guide=False):
    """This frame's nodes in `rg` (the analogue of renderer::commands, renderer/mod.rs:65-106); returns the resource handles.  With
    `temporal`, the "temporal" node accumulates `Light` with the reprojected history into `accumulated`; with `denoise`, the "denoise"
    node filters `Light` (or `accumulated`) into `denoised`; postprocess reads the last of them.  With `motion`, the "motion" node is
    in the list too (handle `motion`); "temporal" reads its image as context state, so it is a root of its own, drawn first.  With
    `adaptive`, the "adaptive" node takes the place of "refrence_mode" (GConst.samples is then the cap; parameters: ctx.adaptive_set_params)
    and writes the image `AdaptiveMoments` as well (handle `adaptive_moments`: {S1, S2, n, stopped before the cap}).
    A frame over a `Light` that is already there (PathTracer.denoise) is the same chain with other ends: `trace=False` imports `Light`
    (no path-trace node, hence no `prev`, and no `color` unless `postprocess`), `gbuffer_node=False` imports the G-buffer too, and
    `gbuffer_names` are the images the G-buffer and its depth live in.
    With `guide` (a lens frame whose context has the guide output set, ctx.set_guide_output) the four images of guide_images() are
    declared as context-state writes of the path-trace node and, with `denoise`, as context-state reads of the "denoise" node (handle
    `guide`: the dict of guide_images); they are no bindings.  With `temporal` too (ctx.set_temporal_guide_input)
    the "temporal" node reads them as context state as well, and the previous frame's set (handle `prev_guide`: prev_guide_images).
    With `guide`, `temporal` and `motion` together no "motion" node is added: the image of
    guide_prev_position_image() (handle `guide_motion`) is a context-state write of the path-trace node
    (ctx.set_guide_motion_output) and a context-state read of "temporal" (ctx.set_temporal_guide_motion_input)."""
    full, f4 = ImageSize.FullScreen, L.FORMAT_R32G32B32A32_SFLOAT
    gbuffer = rg.image(full, L.FORMAT_R32G32B32A32_UINT, gbuffer_names[0])
    depth = rg.image(full, L.FORMAT_R32_SFLOAT, gbuffer_names[1])
    light = rg.image(full, f4, "Light")
    handles = dict(gbuffer=gbuffer, depth=depth, light=light)
    if trace:
        handles["prev"] = rg.image(full, f4, "PrevLight")
    if trace or postprocess:
        handles["color"] = rg.image(full, f4, "color")
    gb = src = guide_origin = IMPORTED
    guide_motion = guide_prev_position_image(rg) if guide and temporal and motion else None
    if gbuffer_node:
        gb = (RayTracingPass.new(rg, "gbuffer").shader("gbuffer").constants(gconst)
              .write(IMPORTED, gbuffer).write(IMPORTED, depth).launch(WorkSize2D.FullScreen))
    if trace:
        name = "adaptive" if adaptive else "refrence_mode"
        pt = (RayTracingPass.new(rg, name).shader(name).constants(gconst)
              .read(gb, gbuffer).read(gb, depth).write(IMPORTED, light).read(IMPORTED, handles["prev"]))
        if adaptive:
            handles["adaptive_moments"] = rg.image(full, f4, "AdaptiveMoments")
            pt.write(IMPORTED, handles["adaptive_moments"])
        if guide:
            for h in guide_images(rg).values():
                pt.state_write(h)
            if guide_motion is not None:
                pt.state_write(guide_motion)
        src = pt.launch(WorkSize2D.FullScreen)
        guide_origin = src
    if guide:
        handles["guide"] = guide_images(rg)
        if temporal:
            handles["prev_guide"] = prev_guide_images(rg)
    lit = light
    if guide_motion is not None:
        handles["guide_motion"] = guide_motion
    elif motion:
        handles["motion"] = motion_node(rg, gconst)[1]
    if temporal:
        src, th = temporal_node(rg, gconst, gb, gbuffer, depth, src, light, guide=handles.get("guide"), guide_origin=guide_origin,
                                prev_guide=handles.get("prev_guide"), guide_motion=guide_motion)
        handles.update(th)
        lit = th["accumulated"]
    if denoise:
        src, lit = denoise_node(rg, gconst, gb, gbuffer, depth, src, lit, guide=handles.get("guide"), guide_origin=guide_origin)
        handles["denoised"] = lit
    if postprocess:
        (ComputePass.new(rg, "postprocess").shader("postprocess").constants(gconst)
         .read(gb, depth).write(IMPORTED, handles["color"]).read(src, lit).dispatch(DispatchSize.FullScreen))
    return handles


def denoise_node(rg, gconst, gb_origin, gbuffer, depth, light_origin, light, guide=None, guide_origin=IMPORTED):
    """ComputePass("denoise"): {gbuffer, gbuffer_depth, In = `light`, Out = the image `denoised`}.  Returns (node, denoised).  `guide`: the
    dict of guide_images() the pass reads as context state (ctx.set_denoise_guide_input), written by node `guide_origin`."""
    denoised = rg.image(ImageSize.FullScreen, L.FORMAT_R32G32B32A32_SFLOAT, "denoised")
    dn = (ComputePass.new(rg, "denoise").shader("denoise").constants(gconst)
          .read(gb_origin, gbuffer).read(gb_origin, depth).read(light_origin, light).write(IMPORTED, denoised))
    for h in (guide or {}).values():
        dn.state_read(guide_origin, h)
    return dn.dispatch(DispatchSize.FullScreen), denoised


TEMPORAL_SWAPS = (("History", "PrevHistory"), ("Moments", "PrevMoments"))


def temporal_images(rg):
    """the images of the "temporal" pass besides this frame's: the previous frame's G-buffer, depth, History, Moments and the three written"""
    f4, full = L.FORMAT_R32G32B32A32_SFLOAT, ImageSize.FullScreen
    return dict(prev_gbuffer=rg.image(full, L.FORMAT_R32G32B32A32_UINT, "PrevGbuffer"), prev_depth=rg.image(full, L.FORMAT_R32_SFLOAT, "PrevDepth"),
                prev_history=rg.image(full, f4, "PrevHistory"), prev_moments=rg.image(full, f4, "PrevMoments"),
                accumulated=rg.image(full, f4, "accumulated"), history=rg.image(full, f4, "History"), moments=rg.image(full, f4, "Moments"))


def temporal_node(rg, gconst, gb_origin, gbuffer, depth, light_origin, light, guide=None, guide_origin=IMPORTED, prev_guide=None,
                  guide_motion=None):
    """ComputePass("temporal"): {gbuffer, gbuffer_depth, In = `light`, PrevGbuffer, PrevDepth, PrevHistory, PrevMoments, Out = `accumulated`,
    History, Moments}.  The previous view is context state (ctx.set_prev_view).  Returns (node, the handles of temporal_images).  `guide`
    and `prev_guide`: the dicts of guide_images() and prev_guide_images() the pass reads as context state (ctx.set_temporal_guide_input),
    the first written by node `guide_origin`; `guide_motion`: the image of guide_prev_position_image(), written by that node too and read
    as context state (ctx.set_temporal_guide_motion_input)."""
    t = temporal_images(rg)
    tn = (ComputePass.new(rg, "temporal").shader("temporal").constants(gconst)
          .read(gb_origin, gbuffer).read(gb_origin, depth).read(light_origin, light)
          .read(IMPORTED, t["prev_gbuffer"]).read(IMPORTED, t["prev_depth"]).read(IMPORTED, t["prev_history"]).read(IMPORTED, t["prev_moments"])
          .write(IMPORTED, t["accumulated"]).write(IMPORTED, t["history"]).write(IMPORTED, t["moments"]))
    for h in (guide or {}).values():
        tn.state_read(guide_origin, h)
    for h in (prev_guide or {}).values():
        tn.state_read(IMPORTED, h)
    if guide_motion is not None:
        tn.state_read(guide_origin, guide_motion)
    return tn.dispatch(DispatchSize.FullScreen), t


def motion_node(rg, gconst):
    """RayTracingPass("motion"): {Motion}, where each pixel's surface point was one frame ago under the previous instance matrices
    (ctx.set_prev_transforms).  "temporal" reads the image as context state (ctx.set_temporal_motion_input), not through an edge: draw this
    node (rg.draw_frame(motion)) before the frame.  Returns (node, motion)."""
    motion = rg.image(ImageSize.FullScreen, L.FORMAT_R32G32B32A32_SFLOAT, "Motion")
    mn = RayTracingPass.new(rg, "motion").shader("motion").constants(gconst).write(IMPORTED, motion).launch(WorkSize2D.FullScreen)
    return mn, motion


def _instance_key(instances):
    """(the geometry runs, the matrices' float32 words) of an instance list"""
    return ([(int(f), int(n)) for f, n, _ in instances],
            [np.ascontiguousarray(np.asarray(m, np.float32)).view(np.uint32).tolist() for _, _, m in instances])


class _TemporalHistory:
    """What the next temporal frame needs to know of the last one: its view, the instance list it was rendered with, and whether the
    context holds the vertex positions as they were then."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.prev_gconst = None     # the view of the frame whose G-buffer / History / Moments the images hold; None = no history
        self.instances = None       # the list the structure was built for; None = never set
        self.prev_instances = None  # ... and the one the last temporal frame was rendered with
        self.snapshot = False       # the context holds a snapshot of the vertex positions (ctx.snapshot_vertices)
        self.verts_updated = False  # vertices updated since the last temporal frame (the snapshot was taken before the first upload)

    def reset(self):
        self.prev_gconst = None
        self.verts_updated = False
        if self.snapshot:
            self.ctx.forget_prev_vertices()
            self.snapshot = False

    def scene_set(self):
        self.snapshot = False  # (new vertices: the context forgot it)
        self.reset()

    def instances_set(self, instances):
        """A list with other geometry runs (another count included), and the first list set, start the history over."""
        if self.instances is None or _instance_key(instances)[0] != _instance_key(self.instances)[0]:
            self.reset()
        self.instances = instances

    def vertices_updated(self):
        """before the upload: between temporal frames the positions of the last one are kept, once per frame interval"""
        if self.prev_gconst is not None and not self.verts_updated:
            self.ctx.snapshot_vertices()
            self.snapshot = True
        self.verts_updated = True

    def begin_frame(self):
        """Hand the context what moved since the last temporal frame; returns whether anything did (the frame then needs "motion")."""
        # instances that moved: hand over the last frame's matrices
        moved = (self.prev_gconst is not None and self.instances is not None and self.prev_instances is not None
                 and _instance_key(self.instances) != _instance_key(self.prev_instances))
        self.ctx.set_prev_transforms([m for _, _, m in self.prev_instances] if moved else None)
        # vertices updated: vertices_updated() took the snapshot, "motion" follows the deformed geometries.  No update since: the snapshot
        # is brought up to the current positions (a copy of the ranges last updated), so nothing is deformed
        deformed = self.prev_gconst is not None and self.verts_updated and self.snapshot
        if self.snapshot and not deformed:
            self.ctx.snapshot_vertices()
        return moved or deformed

    def end_frame(self, gconst):
        self.prev_gconst = L.GConst()
        C.memmove(C.byref(self.prev_gconst), C.byref(gconst), C.sizeof(gconst))
        self.prev_instances = self.instances
        self.verts_updated = False


class PathTracer:
    """One GPU's share of the frame.  `rank` / `n_ranks` select the interleaved 64x64 tiles this process renders."""

    def __init__(self, window, device=0, rank=0, n_ranks=1, ctx=None):
        self.window = (int(window[0]), int(window[1]))
        self.ctx = Context(device) if ctx is None else ctx
        self.rank, self.n_ranks = rank, n_ranks
        self.ctx.set_tile_partition(self.window[0], self.window[1], rank, n_ranks)
        self.rg = RenderGraph(self.ctx, self.window)
        self.handles = {}
        self.comm_ready = False  # True once init_comm() has joined librt3's RCCL communicator
        self._stage = None       # rehearsal path only: staging buffer of the host-moved gather
        self.host_group = None   # process group of the host-moved gather (None = the default group)
        self._history = _TemporalHistory(self.ctx)
        self._glass_lens = False  # the lens in force is the pinhole set_scene switched on for a scene with glass
        self._fog_lens = False  # ... or the one set_medium switched on for a medium
        self._medium_on = False  # set_medium's medium is on (some coefficient > 0)
        self._scene_set = False   # set_scene has built a structure (set_pane_shadows rebuilds it)
        self._guide = False       # set_guide: lens frames write guide images, and "denoise" is guided by them
        self._guide_temporal = False    # set_guide(temporal=True): temporal lens frames write them too, and "temporal" reads two sets
        self._temporal_guided = False   # the history images were written by a guided "temporal" (the other kind of frame starts over)

    def close(self):
        self.ctx.close()

    def set_scene(self, mesh, sky=None, bluenoise=None, *, instances=None, options=()):
        """Upload the world and build its acceleration structure once.  `options`: (L.OPT_*, value) pairs set first; `instances`: the list
        set_instances() would take, placed before the build.  A mesh with glass (Mesh.transmission) needs per-sample camera rays: with no
        lens on, set_lens(0, 1, 0) -- the per-sample pinhole -- is switched on, and off again by the next set_scene without glass.  A lens
        the caller set stays."""
        for opt, value in options:
            self.ctx.set_option(opt, value)
        self.ctx.upload_mesh(mesh)  # (with the mesh's punctual lights, when it has some)
        if not len(getattr(mesh, "lights", ())):
            self.ctx.set_lights(None)  # the lights belong to the world: a scene without them replaces the previous scene's
        if instances is not None:
            instances = self._upload_instances(instances)
        if sky is not None:
            self.ctx.set_sky(sky)
        if bluenoise is not None:
            self.ctx.set_bluenoise(bluenoise)
        self.ctx.build_accel()
        self._scene_set = True
        # skins: the mesh's, in its order; the vertex buffer holds the static load until pose()
        self._posed_mesh = mesh if getattr(mesh, "skins", None) else None
        for s in getattr(mesh, "skins", None) or []:
            self.ctx.add_skin(s.first_vertex, s.joints, s.weights, len(s.joint_nodes), s.rest, s.target_dpos, s.target_dnrm)
        tr = getattr(mesh, "transmission", None)
        glass = tr is not None and len(tr) and bool(np.any(tr["transmission"] > 0))
        if glass and not self.ctx.get_lens()[1]:
            self.ctx.set_lens(L.LensParams(0.0, 1.0, 0.0))
            self._glass_lens = True
        elif not glass and self._glass_lens:
            self.ctx.set_lens(None)
            self._glass_lens = False
        if glass and self._fog_lens:  # the pinhole set_medium switched on is the glass's from here on: the next scene without glass ends it
            self._fog_lens = False
            self._glass_lens = True
        if self._medium_on and not self.ctx.get_lens()[1]:  # the medium outlives the scene, and needs the pinhole too
            self.ctx.set_lens(L.LensParams(0.0, 1.0, 0.0))
            self._fog_lens = True
        self._history.scene_set()
        if instances is not None:
            self._history.instances_set(instances)

    def set_medium(self, medium=None):
        """Fog for the frames that follow (ctx.set_medium): an L.Medium -- one axis-aligned box of homogeneous medium
        with single scattering; scene_medium() makes one over a mesh's bounds -- or None for none, the default.  No rebuild.  A medium
        needs per-sample camera rays: with no lens on, set_lens(0, 1, 0) -- the per-sample pinhole -- is switched on, and off again by
        set_medium(None); a lens the caller set stays.  Denoise, temporal and motion frames do not see the medium."""
        self.ctx.set_medium(medium)
        on = self._medium_on = self.ctx.get_medium()[1]
        if on and not self.ctx.get_lens()[1]:
            self.ctx.set_lens(L.LensParams(0.0, 1.0, 0.0))
            self._fog_lens = True
        elif not on and self._fog_lens:
            if not self._glass_lens:
                self.ctx.set_lens(None)
            self._fog_lens = False

    def medium_info(self):
        """(traced segments that ran through the medium, in-scatter shadow rays queued) of the last frame's path-tracing launch"""
        return self.ctx.medium_info()

    def set_pane_shadows(self, on=True):
        """Pane shadows (ctx.set_pane_shadows): light is sampled through thin-walled glass -- sky, emitter and punctual
        shadow rays cross a pane attenuated by its expected transmittance instead of stopping at it.  Rebuilds, as set_scene does, when
        the mode changes and a scene is set.  Unbiased; the same image in expectation for sky and emitters, and the only way a punctual
        light shines through a window."""
        if bool(on) == self.ctx.get_pane_shadows():
            return
        self.ctx.set_pane_shadows(bool(on))
        if self._scene_set:
            self.ctx.build_accel()

    def set_rough_transmission(self, on=True):
        """Rough transmission (ctx.set_rough_transmission): glass whose material roughness is > 0 is frosted -- its
        glass vertices reflect and refract at GGX micro-normals.  Rebuilds, as set_scene does, when the mode changes and a scene is set.
        Frosted glass is lit by BSDF-sampled paths only; a frosted pane is no pane of set_pane_shadows."""
        if bool(on) == self.ctx.get_rough_transmission():
            return
        self.ctx.set_rough_transmission(bool(on))
        if self._scene_set:
            self.ctx.build_accel()

    def set_lights(self, lights=None):
        """Replace the world's punctual lights (assets.LIGHT_DTYPE; None forgets them).  No rebuild: frames with F_NEE_PUNCTUAL in their
        flags sample them from the next frame on.  Moved lights' shadows lag in temporal history like any moved light."""
        self.ctx.set_lights(lights)

    def _upload_instances(self, instances):
        instances = [(int(f), int(n), np.array(m, np.float32)) for f, n, m in instances]
        self.ctx.set_instances(instances)
        return instances

    def set_instances(self, instances):
        """Place the scene's geometries: upload the list (ctx.set_instances) and rebuild.  The next temporal frame compares it with the
        list of the last one and, where matrices differ, runs the "motion" pass so that moved instances keep their history.  A list with
        other geometry runs (another count included), and the first list set, start the history over."""
        instances = self._upload_instances(instances)
        self.ctx.build_accel()
        self._history.instances_set(instances)

    def reset_history(self):
        """the next temporal frame starts over (zeroed PrevHistory / PrevMoments: the reset rule of the "temporal" pass)"""
        self._history.reset()

    def _begin_temporal(self, gconst, denoise, gbuffer_names=("gbuffer", "gbuffer_depth"), guide=False, trace=True):
        """Before a temporal frame's nodes are built: what the last temporal frame wrote, and the G-buffer it read (the images named
        `gbuffer_names`), become `Prev*` (the images trade names, like swap_light_prev), or, with no history, zeros are uploaded; the
        previous view and the variance input of "denoise" are set.  A frame rendered without `temporal` in between overwrites the kept
        G-buffer: call reset_history() after one.  Returns whether the frame follows what moved: with the "motion" node, or, guided, with
        the guide's fifth image.
        `guide` (set_guide(temporal=True) with a lens in force): "temporal" takes its records from this frame's guide
        images and from the previous guided temporal frame's (the two sets trade names behind each such frame, _end_temporal).  The
        pinhole motion input stays 0 whatever moved; when something moved or deformed, "refrence_mode" is given the image of
        guide_prev_position_image() to write (ctx.set_guide_motion_output) and "temporal" the same image to look up
        (ctx.set_temporal_guide_motion_input), else both are set to 0.  Not with `trace` False (denoise(): the frame's
        "refrence_mode" has run already): the input is 0 and False is returned.  A guided frame after an unguided one, and the reverse,
        start the history over."""
        if guide != self._temporal_guided:
            self._history.reset()
            self._temporal_guided = guide
        rg, prev_gconst = self.rg, self._history.prev_gconst
        temporal_images(rg)
        for name, fmt in zip(gbuffer_names, (L.FORMAT_R32G32B32A32_UINT, L.FORMAT_R32_SFLOAT)):
            rg.image(ImageSize.FullScreen, fmt, name)
        if prev_gconst is not None:
            n = rg.named
            for a, b in TEMPORAL_SWAPS + ((gbuffer_names[0], "PrevGbuffer"), (gbuffer_names[1], "PrevDepth")):
                n[a], n[b] = n[b], n[a]
        t = temporal_images(rg)
        if prev_gconst is None:
            W, H = self.window
            zero = np.zeros((H, W, 4), np.float32)
            rg.upload(t["prev_history"], zero)
            rg.upload(t["prev_moments"], zero)
        self.ctx.set_prev_view(prev_gconst if prev_gconst is not None else gconst)
        self.ctx.set_denoise_variance_input(t["moments"] if denoise else 0)
        moved = self._history.begin_frame()  # "temporal" then reads the "motion" pass's image
        if guide:
            # the "motion" image is made from pinhole primary hits and does not describe the camera samples: their own mean previous position
            moved = moved and trace
            image = guide_prev_position_image(rg) if moved else 0
            self.ctx.set_temporal_guide_input(guide_images(rg), prev_guide_images(rg))
            self.ctx.set_temporal_guide_motion_input(image)
            if trace:
                self.ctx.set_guide_motion_output(image)
        elif self._guide:
            self.ctx.set_temporal_guide_input(None, None)
            self.ctx.set_temporal_guide_motion_input(0)
        self.ctx.set_temporal_motion_input(rg.image(ImageSize.FullScreen, L.FORMAT_R32G32B32A32_SFLOAT, "Motion") if moved and not guide else 0)
        return moved

    def _end_temporal(self, gconst, guide):
        """Behind a temporal frame: its view is the next one's previous view; behind a guided one the two guide sets trade names, so that
        the next "refrence_mode" writes the other set and this frame's is `Prev*`."""
        self._history.end_frame(gconst)
        if guide:
            n = self.rg.named
            for a, b in GUIDE_SWAPS:
                n[a], n[b] = n[b], n[a]

    def update_vertices(self, vertices, first=0):
        """deformed vertices (same topology): upload them and refit the acceleration structure.  Between temporal frames the positions as
        they were at the last one are kept first (ctx.snapshot_vertices, once per frame interval, before its first upload), and the next
        temporal frame runs the "motion" pass so that the deformed geometries keep their history -- or, guided by the
        camera samples (set_guide(temporal=True)), writes their mean previous position from the same snapshot (section 4w)."""
        self._history.vertices_updated()
        self.ctx.update_vertices(vertices, first)
        self.ctx.refit_accel()

    def pose(self, t, animation=0):
        """the scene's skins at time `t` of animation `animation` (Mesh.pose): every skin is posed on the device (ctx.pose_skin, DESIGN.md
        section 4z) and the acceleration structure refitted once.  For the temporal history this is update_vertices(): the snapshot is taken
        first, and the next temporal frame follows the skinned geometries."""
        mesh = getattr(self, "_posed_mesh", None)
        if mesh is None:
            raise ValueError("pose: the scene has no skins (Mesh.skins)")
        poses = mesh.pose(t, animation)
        self._history.vertices_updated()
        for k, (palette, weights) in enumerate(poses):
            self.ctx.pose_skin(k, palette, weights)
        self.ctx.refit_accel()

    def make_gconst(self, camera: Camera, samples, bounces=4, frame=0, blendfactor=1.0, flags=DEFAULT_FLAGS) -> L.GConst:
        g = camera.gconst(self.window)
        g.frame, g.samples, g.bounces, g.blendfactor = frame, samples, bounces, blendfactor
        g.pad[0] = flags
        return g

    def set_lens(self, aperture=0.0, focus=1.0, jitter=1.0):
        """Per-sample camera rays for the frames that follow (ctx.set_lens): `jitter` is the width in pixels of the
        box each sample's film point is drawn from (1 = antialiasing over the whole pixel), `aperture` the lens radius in world units
        (0 = pinhole), `focus` the view depth of the plane of focus.  set_lens(None) switches back to one primary hit per pixel.  With a
        lens, "postprocess" shows `Light` everywhere, and adaptive frames are refused unless set_adaptive_coverage(True)."""
        self._glass_lens = self._fog_lens = False  # the caller's choice from here on
        if aperture is None:
            self.ctx.set_lens(None)
        else:
            self.ctx.set_lens(L.LensParams(aperture, focus, jitter))

    def set_guide(self, on=True, temporal=False):
        """Sample-guided denoising of lens frames, off by default.  While on and a lens is in force -- set_lens, or the
        pinhole set_scene switches on for a scene with glass -- render() has "refrence_mode" write the four guide images (handle `guide`,
        guide()) from the frame's own camera samples, and render(g, denoise=True) and denoise() filter by them instead of by the pinhole
        G-buffer.  Without a lens, and for adaptive frames, everything is as with the guide off; so it is for temporal frames unless
        `temporal`: then render(g, temporal=True[, denoise=True]) writes the guide too, "temporal" takes its surface
        records from this frame's and the previous temporal frame's guide images instead of the pinhole G-buffer, and "denoise" is guided
        by this frame's with the temporal variance.  Such frames never run "motion": after set_instances() moved something or
        update_vertices() deformed something, render() has "refrence_mode" write a fifth image, the samples' mean previous position, and
        "temporal" looks that point up in the previous frame, so moved instances and deformed meshes keep their
        history under a lens as they do without one.  denoise(temporal=True) runs behind the frame's "refrence_mode" and does not follow them.
        With several ranks denoise() raises: the guide images are not gathered."""
        self._guide = bool(on)
        self._guide_temporal = self._guide and bool(temporal)
        if not self._guide:
            self.ctx.set_guide_output(None)
            self.ctx.set_guide_motion_output(0)
            self.ctx.set_denoise_guide_input(None)
            self.ctx.set_temporal_guide_input(None, None)
            self.ctx.set_temporal_guide_motion_input(0)

    def _temporal_guide_in_force(self, adaptive=False):
        """whether a temporal frame rendered now is a guided one (set_guide(temporal=True), a lens in force, not adaptive)"""
        return bool(self._guide_temporal and not adaptive and self.ctx.get_lens()[1])

    def _guide_in_force(self, denoise, temporal=False, adaptive=False):
        """Set the context's guide output and input for the frame that follows; returns whether the frame has guide images.  A tracer whose
        guide was never switched on makes no call."""
        if not self._guide:
            return False
        on = self.ctx.get_lens()[1] and (not temporal or self._guide_temporal) and not adaptive
        images = guide_images(self.rg) if on else None
        self.ctx.set_guide_output(images)
        if not (on and temporal):  # a guided temporal frame's fifth image is _begin_temporal's; every other frame writes none
            self.ctx.set_guide_motion_output(0)
        self.ctx.set_denoise_guide_input(images if denoise else None)
        return on

    def set_adaptive_coverage(self, on=True):
        """Coverage mode of adaptive frames (ctx.adaptive_set_coverage): with a lens set -- by set_lens, or by set_scene
        for a scene with glass -- render(g, adaptive=...) samples every pixel of the rank to the threshold, each sample from its own camera
        ray, instead of being refused.  Off by default; render() never switches it on.  Without a lens it changes nothing."""
        self.ctx.adaptive_set_coverage(bool(on))

    def set_roulette(self, start_bounce=2, min_survival=0.0625):
        """Russian roulette for the frames that follow (ctx.set_roulette): the extension rays of vertices
        `start_bounce` .. bounces - 2 survive with probability min(1, max(largest throughput component, `min_survival`)) and carry their
        throughput divided by it.  Unbiased; noisier per sample, cheaper per sample at many bounces.  set_roulette(None) switches it off,
        the default."""
        if start_bounce is None:
            self.ctx.set_roulette(None)
        else:
            self.ctx.set_roulette(L.RouletteParams(start_bounce, min_survival))

    def set_textured_emitters(self, on=True):
        """Textured emitters for the frames that follow (ctx.set_textured_emitters): under F_NEE_EMISSIVE the light
        sampler also picks the triangles whose emission is a factor times an emissive texture (lamps, screens, signs of a glTF asset),
        which are otherwise found by BSDF-sampled rays alone.  Same expectation, less noise where such emitters are small.  Off by
        default; no rebuild is needed."""
        self.ctx.set_textured_emitters(bool(on))

    def roulette_info(self):
        """(extension rays tested, of them ended) of the last frame's path-tracing launch"""
        return self.ctx.roulette_info()

    def commands(self, gconst: L.GConst, postprocess=True, denoise=False, temporal=False, motion=False, adaptive=False, guide=False):
        """Build this frame's nodes (frame_nodes).  `denoise` and `temporal` need the whole window on this rank: with several ranks use
        denoise().  `temporal` also needs the state that render(temporal=True) keeps (previous view, history images); `guide` the
        context state that render() sets under set_guide()."""
        self.rg.begin_frame()
        self.handles = frame_nodes(self.rg, gconst, postprocess, denoise, temporal, motion, adaptive, guide=guide)
        return self.handles

    @contextlib.contextmanager
    def _whole_window(self):
        """The tile partition switched off for the launches enqueued inside: a chain that reads other tiles' pixels runs for the whole
        window on this rank.  Launches read the partition when they are enqueued: safe to restore behind them."""
        W, H = self.window
        if self.n_ranks > 1:
            self.ctx.set_tile_partition(W, H, 0, 1)
        try:
            yield
        finally:
            if self.n_ranks > 1:
                self.ctx.set_tile_partition(W, H, self.rank, self.n_ranks)

    def denoise(self, gconst, wait=True, temporal=False, denoise=True):
        """Filter the `Light` of the last render() into `denoised` with the "denoise" pass (parameters: ctx.set_denoise_params).  A tap
        reads pixels of other tiles, so with several ranks this runs on the rank that holds the assembled frame -- after
        gather_light(..., download=False) on its root -- with the partition switched off around it, like render_probes: the G-buffer is
        rendered again for the whole window (primary rays only), then the gathered `Light` is filtered.  Returns the handles.
        With `temporal` the "temporal" pass runs first on the same footing (history as in render(temporal=True); call it once per
        frame; the whole-window G-buffer is rendered into images of its own, which render() does not touch, on one rank too) and
        "denoise" -- unless `denoise` is False -- filters its `accumulated` image with the temporal variance."""
        rg = self.rg
        tguide = temporal and self._temporal_guide_in_force()
        # the last render()'s guide images (set_guide)
        guide = tguide or bool(self._guide and denoise and not temporal and self.ctx.get_lens()[1])
        if guide and self.n_ranks > 1:
            raise ValueError("denoise() with the sample guide on (set_guide) needs the whole frame's guide images on this rank, and they are not "
                             "gathered: render on one rank, or switch the guide off")
        names = ("TemporalGbuffer", "TemporalDepth") if temporal else ("gbuffer", "gbuffer_depth")  # render() must not overwrite the kept one
        moved = temporal and self._begin_temporal(gconst, denoise, names, guide=tguide, trace=False)
        if denoise and not temporal:
            self.ctx.set_denoise_variance_input(0)
        if self._guide:
            self.ctx.set_denoise_guide_input(guide_images(rg) if guide and denoise else None)
        rg.begin_frame()
        h = frame_nodes(rg, gconst, False, denoise, temporal, moved, gbuffer_names=names, gbuffer_node=self.n_ranks > 1 or temporal, trace=False,
                        guide=guide)
        self.handles = {k: v for k, v in self.handles.items() if k != "motion"} | h  # earlier frames' handles stay, but for a stale `motion`
        with self._whole_window():
            if moved:  # on the whole window, like the G-buffer
                rg.draw_frame(h["motion"])
            rg.draw_frame(h["denoised"] if denoise else (h["accumulated"] if temporal else h["light"]), wait=wait)
        if temporal:
            self._end_temporal(gconst, tguide)
        return self.handles

    def probe_commands(self, gconst: L.GConst):
        """The probe-GI frame: one probe per 16x16 pixel block, 8x8 rays per probe in the probe atlas.  Returns the handles; `Light`
        receives the interpolated image.  Under a tile partition (n_ranks > 1) the chain runs REPLICATED: it reads the whole G-buffer
        (jittered neighbours, probes up to two cells away, red marks scattered to other pixels) and is launch-bound at well under a
        millisecond, so every rank renders it for the full window (render_probes switches the partition off around it) and the
        frame-end gather of each rank's own tiles assembles the same image on the root as a single rank would produce."""
        rg = self.rg
        rg.begin_frame()
        W, H = self.window
        px, py = W // 16, H // 16
        asize = ImageSize.XY(px * 8, py * 8)
        gbuffer = rg.image(ImageSize.FullScreen, L.FORMAT_R32G32B32A32_UINT, "gbuffer")
        depth = rg.image(ImageSize.FullScreen, L.FORMAT_R32_SFLOAT, "gbuffer_depth")
        light = rg.image(ImageSize.FullScreen, L.FORMAT_R32G32B32A32_SFLOAT, "Light")
        directions = rg.image(asize, L.FORMAT_R16_UINT, "probe_directions")
        debug = rg.image(asize, L.FORMAT_R32_SFLOAT, "probe_debug")
        atlas = rg.image(asize, L.FORMAT_R32G32B32A32_SFLOAT, "probe_atlas")
        prev_atlas = rg.image(asize, L.FORMAT_R32G32B32A32_SFLOAT, "prev_probe_atlas")
        sh = rg.buffer(sh_buffer_bytes(px, py), "sh_coeficents")
        gb = (RayTracingPass.new(rg, "gbuffer").shader("gbuffer").constants(gconst)
              .write(IMPORTED, gbuffer).write(IMPORTED, depth).launch(WorkSize2D.FullScreen))
        sis = (ComputePass.new(rg, "structured_importance_sampling").shader("structured_importance_sampling").constants(gconst)
               .read(gb, gbuffer).read(gb, depth).write(IMPORTED, directions).write(IMPORTED, debug).read(IMPORTED, atlas)
               .dispatch(DispatchSize.XY(px, py)))
        tp = (RayTracingPass.new(rg, "trace_probes").shader("trace_probes").constants(gconst)
              .read(gb, gbuffer).read(gb, depth).read(sis, directions).write(IMPORTED, atlas).read(IMPORTED, prev_atlas)
              .launch(WorkSize2D.XY(px * 8, py * 8)))
        shc = (ComputePass.new(rg, "spherical_harmonic_conversion").shader("spherical_harmonic_conversion").constants(gconst)
               .write(IMPORTED, sh).read(tp, atlas).dispatch(DispatchSize.XY(px, py)))
        (ComputePass.new(rg, "interpolate_probes").shader("interpolate_probes").constants(gconst)
         .read(gb, gbuffer).read(gb, depth).read(shc, sh).write(IMPORTED, light).dispatch(DispatchSize.FullScreen))
        self.handles = dict(gbuffer=gbuffer, depth=depth, light=light, directions=directions, debug=debug, atlas=atlas, prev_atlas=prev_atlas, sh=sh)
        return self.handles

    def render_probes(self, gconst, wait=True):
        h = self.probe_commands(gconst)
        with self._whole_window():  # replicas: the whole window on every rank (see probe_commands)
            self.rg.draw_frame(h["light"], wait=wait)
        return h

    def copy_atlas_to_prev(self):
        """Temporal blend input of trace_probes (prev_probe_atlas, trace_probes.slang:12,74)."""
        W, H = self.window
        self.rg.upload(self.handles["prev_atlas"], self.rg.download(self.handles["atlas"], (H // 16 * 8, W // 16 * 8, 4), np.float32))

    def render(self, gconst, postprocess=False, wait=True, denoise=False, temporal=False, adaptive=None):
        """One frame.  `temporal` accumulates it with the reprojected history of the previous temporal frame (this object keeps two sets
        of history images, the previous G-buffer, depth and GConst, and starts from zeros after set_scene / reset_history); with
        `denoise` too, the filter reads the accumulated image and its temporal variance.  One rank only: see denoise().  After
        set_instances() moved something or update_vertices() deformed something, the frame has the "motion" node as well (handle `motion`)
        and "temporal" follows the instances and the deformed geometries.
        `adaptive`: an L.AdaptiveParams (or True for the parameters the context holds): the "adaptive" pass renders `Light` instead of
        "refrence_mode", with gconst.samples as the cap; its Moments image is the handle `adaptive_moments` (adaptive_moments(),
        sample_counts(), ctx.adaptive_info()).
        Under set_guide(True, temporal=True) with a lens in force a temporal frame is guided by the camera samples:
        handles `guide` and `prev_guide`, and no "motion" node whatever moved.  After set_instances() moved something or update_vertices()
        deformed something such a frame has "refrence_mode" write the samples' mean previous position as a fifth guide image (handle
        `guide_motion`), which "temporal" looks up in the previous frame."""
        if adaptive is not None and adaptive is not True and adaptive is not False:
            self.ctx.adaptive_set_params(adaptive)
        adaptive_on = adaptive is not None and adaptive is not False
        tguide = temporal and self._temporal_guide_in_force(adaptive_on)
        motion = temporal and self._begin_temporal(gconst, denoise, guide=tguide)
        if denoise and not temporal:
            self.ctx.set_denoise_variance_input(0)
        guide = self._guide_in_force(denoise, temporal, adaptive_on)
        h = self.commands(gconst, postprocess, denoise, temporal, motion, adaptive=adaptive_on, guide=guide)
        if motion and not tguide:
            self.rg.draw_frame(h["motion"])
        self.rg.draw_frame(h["color"] if postprocess else (h["denoised"] if denoise else (h["accumulated"] if temporal else h["light"])), wait=wait)
        if temporal:
            self._end_temporal(gconst, tguide)
        return h

    # ---- results
    def _download(self, key, dtype=np.float32, channels=(4,)):
        W, H = self.window
        return self.rg.download(self.handles[key], (H, W, *channels), dtype)

    def light(self):
        return self._download("light")

    def color(self):
        return self._download("color")

    def denoised(self):
        return self._download("denoised")

    def accumulated(self):
        """Out of the "temporal" pass"""
        return self._download("accumulated")

    def history(self):
        """(History, Moments) of the "temporal" pass"""
        return self._download("history"), self._download("moments")

    def guide(self):
        """the guide images of the last lens frame rendered under set_guide(): {position, normal, albedo, emission} -> (H, W, 4) float32"""
        W, H = self.window
        return {k: self.rg.download(h, (H, W, 4), np.float32) for k, h in self.handles["guide"].items()}

    def adaptive_moments(self):
        """Moments of the "adaptive" pass: {S1, S2, n, 1 = stopped before the cap} per foreground pixel, 0 for background; in coverage mode
        (set_adaptive_coverage with a lens) per pixel of this rank, background included"""
        return self._download("adaptive_moments")

    def sample_counts(self):
        """the samples each pixel got in the last adaptive frame (H, W) uint32; 0 = background, or, in coverage mode (set_adaptive_coverage with a
        lens), only a pixel of another rank"""
        return self.adaptive_moments()[..., 2].astype(np.uint32)

    def motion(self):
        """the "motion" pass's image of the last frame that had one"""
        return self._download("motion")

    def gbuffer(self):
        return self._download("gbuffer", np.uint32), self._download("depth", channels=())

    def copy_light_to_prev(self):
        """Progressive accumulation: PrevLight <- Light (refrence_mode.slang:11,61-65), through the host (tests)."""
        self.rg.upload(self.handles["prev"], self.light())

    def swap_light_prev(self):
        """Progressive accumulation without a copy: the two images trade names, so the next frame's `PrevLight` is this frame's
        `Light` (refrence_mode.slang:10-11,61-65; the reference's two images are distinct resources as well)."""
        n = self.rg.named
        n["Light"], n["PrevLight"] = n["PrevLight"], n["Light"]

    def load_prev(self, image):
        """Resume a progressive render: `image` (H, W, 4) float32 becomes the next frame's `PrevLight` (checkpoint row)."""
        W, H = self.window
        h = self.rg.image(ImageSize.FullScreen, L.FORMAT_R32G32B32A32_SFLOAT, "PrevLight")
        self.rg.upload(h, np.ascontiguousarray(image, np.float32).reshape(H, W, 4))

    # ---- multi-GPU: ONE gather of the per-rank tile buffers at frame end (include/rt3.h: rt3_gather_tiles, RCCL inside librt3)
    def tile_pixel_count(self, rank):
        return self.ctx.tile_pixel_count(rank, self.n_ranks)

    def init_comm(self, uid: bytes):
        """Collective over all ranks: join librt3's own RCCL communicator.  `uid` is rank 0's `ctx.comm_unique_id()`, carried to the
        other ranks by the host (bench.py: through the torch.distributed key-value store)."""
        self.ctx.comm_init(uid, self.rank, self.n_ranks)
        self.comm_ready = True

    def gather_light(self, dist=None, torch=None, dst=0, download=True):
        """Assemble the frame on rank `dst` from every rank's tiles of `Light` with the frame's one collective.
        With a communicator (`init_comm`): `rt3_gather_tiles`, enqueued on librt3's stream, no host synchronisation.
        Without one (REHEARSAL on a one-GPU box, `RT3_DIST_BACKEND=gloo`): the same layout and the same single untile launch
        (`rt3_gather_layout` / `rt3_gather_unpack`), the bytes moved through host tensors by `exchange_tiles_host`.
        Returns the full (H, W, 4) image on `dst` (None elsewhere); with download=False the assembled frame stays in `dst`'s HBM
        (the `Light` image) and True is returned on `dst` instead.  With n_ranks == 1 no collective is issued."""
        img = self.handles["light"]
        if self.n_ranks > 1:
            if self.comm_ready:
                self.ctx.gather_tiles(img, dst)
            else:
                off = self.ctx.gather_layout(img, dst, self.n_ranks)
                mine = None
                if self.rank != dst:
                    n = self.tile_pixel_count(self.rank)
                    if self._stage is None:
                        self._stage = self.rg.buffer(max(n, 1) * 16, "gather_stage")
                    ptr, _ = self.rg.device_ptr(self._stage)
                    self.ctx.check(self.ctx.lib.rt3_image_pack_tiles(self.ctx.h, img, self.rank, self.n_ranks, C.c_void_p(ptr)))
                    mine = self.rg.download(self._stage, (max(n, 1), 4), np.float32)[:n]
                recv = exchange_tiles_host(dist, torch, self.rank, self.n_ranks, off, mine, dst, group=self.host_group)
                if self.rank == dst and off[-1]:
                    if self._stage is None:
                        self._stage = self.rg.buffer(off[-1] * 16, "gather_stage")
                    self.rg.upload(self._stage, recv)
                    self.ctx.gather_unpack(img, dst, self.n_ranks, self.rg.device_ptr(self._stage)[0])
            if self.rank != dst:
                return None
        return self.light() if download else True


def gather_offsets(counts, root):
    """Pixel offsets of the frame-end gather's receive buffer (what `rt3_gather_layout` returns): ranks in ascending order, exact
    counts, nothing from `root` itself (its tiles are already in its image).  n_ranks + 1 entries."""
    off = [0]
    for r, c in enumerate(counts):
        off.append(off[-1] + (0 if r == root else int(c)))
    return off


def exchange_tiles_host(dist, torch, rank, n_ranks, offsets, mine, dst=0, group=None):
    """Host-memory stand-in for the RCCL exchange inside `rt3_gather_tiles` (gloo: CPU tests, one-GPU rehearsal): every rank
    but `dst` sends its packed tiles (n x 4 float32) point to point; `dst` receives rank r's at offsets[r]..offsets[r+1] of ONE
    contiguous buffer, all receives posted together.  Returns that buffer on `dst`, None elsewhere."""
    if rank != dst:
        if mine is not None and len(mine):
            dist.send(torch.from_numpy(np.ascontiguousarray(mine, np.float32)), dst, group=group)
        return None
    recv = torch.empty((offsets[-1], 4), dtype=torch.float32)
    reqs = [dist.irecv(recv[offsets[r]:offsets[r + 1]], src=r, group=group) for r in range(n_ranks) if r != dst and offsets[r + 1] > offsets[r]]
    for q in reqs:
        q.wait()
    return recv.numpy()


def zcurve(x, y):
    """ZCurveToLinearIndex (shaders/include/math.slang:105-117)"""
    def explode(v):
        v = (v | (v << 8)) & 0x00FF00FF
        v = (v | (v << 4)) & 0x0F0F0F0F
        v = (v | (v << 2)) & 0x33333333
        return (v | (v << 1)) & 0x55555555
    return explode(x) | (explode(y) << 1)


def sh_buffer_bytes(probes_x, probes_y):
    """Bytes of the float3x3 buffer spherical_harmonic_conversion writes at zcurve(3 * gx + c, gy) (48 B per element)."""
    return 48 * (zcurve(probes_x * 3 - 1, probes_y - 1) + 1)


def default_camera(window, position, direction, fov_deg):
    return Camera(position, direction, math.radians(fov_deg), window[0] / window[1])
