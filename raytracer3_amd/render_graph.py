"""Host-side mirror of the reference's per-frame pass graph, driving librt3.so through its C ABI.

Reference (src/renderer/render_graph/*):
  * `RenderGraph::image / buffer / import` name-keyed transient resources        mod.rs:422-483
  * `RayTracingPass::new(rg, name).shader(..).entry(..).constants(&c).read(origin, h).write(origin, h)
        .read_write(origin, h).launch(WorkSize2D)`                                executions.rs:80-101, build.rs:66-209,371-399
  * `ComputePass::new(rg, name)....dispatch(DispatchSize)`                        executions.rs:15-36
  * execution order = reverse DFS over `origin` edges from the node touching the output image, de-duplicated
                                                                                  bake.rs:29-49
  * bindings = one u32 handle per non-attachment edge in builder order           bake.rs:51-83
Barriers / image layouts / descriptor heaps are Vulkan mechanics and have no HIP counterpart (single in-order stream).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L

IMPORTED = 0xFFFFFFFFFFFFFFFF  # render_graph/mod.rs:38  (`!0`)


class ImageSize:
    """build.rs:211-229"""

    def __init__(self, kind, a=0, b=0):
        self.kind, self.a, self.b = kind, a, b

    FullScreen = None  # filled below

    @staticmethod
    def FractionalFullScreen(dx, dy):
        return ImageSize("frac", dx, dy)

    @staticmethod
    def XY(x, y):
        return ImageSize("xy", x, y)

    def size(self, window):
        w, h = window
        if self.kind == "full":
            return w, h
        if self.kind == "frac":
            return -(-w // self.a), -(-h // self.b)
        return self.a, self.b


ImageSize.FullScreen = ImageSize("full")


class WorkSize2D:
    """executions.rs:57-78 : FullScreen = WINDOW_SIZE exactly (no group rounding)."""

    def __init__(self, kind, a=0, b=0):
        self.kind, self.a, self.b = kind, a, b

    FullScreen = None

    @staticmethod
    def FractionalFullScreen(x, y):
        return WorkSize2D("frac", x, y)

    @staticmethod
    def X(x):
        return WorkSize2D("x", x)

    @staticmethod
    def XY(x, y):
        return WorkSize2D("xy", x, y)

    def size(self, window):
        w, h = window
        return {"full": (w, h), "frac": (-(-w // max(self.a, 1)), -(-h // max(self.b, 1))), "x": (self.a, 1), "xy": (self.a, self.b)}[self.kind]


WorkSize2D.FullScreen = WorkSize2D("full")


class DispatchSize:
    """build.rs:231-263 : FullScreen = ceil(W/8) x ceil(H/8) x 1 groups."""

    def __init__(self, kind, a=0, b=0, c=0):
        self.kind, self.a, self.b, self.c = kind, a, b, c

    FullScreen = None

    @staticmethod
    def X(x):
        return DispatchSize("xyz", x, 1, 1)

    @staticmethod
    def XY(x, y):
        return DispatchSize("xyz", x, y, 1)

    @staticmethod
    def XYZ(x, y, z):
        return DispatchSize("xyz", x, y, z)

    def size(self, window):
        w, h = window
        if self.kind == "full":
            return -(-w // 8), -(-h // 8), 1
        return self.a, self.b, self.c


DispatchSize.FullScreen = DispatchSize("full")


@dataclass
class NodeEdge:  # render_graph/mod.rs:109-126
    origin: int | None
    edge_type: str  # ShaderRead | ShaderWrite | ShaderReadWrite
    resource: int


@dataclass
class Node:  # render_graph/mod.rs:101-107
    name: str
    kind: str  # "raytracing" | "compute"
    path: str
    entry: str
    size: object
    constants: object
    edges: list = field(default_factory=list)


class Context:
    """Owns the rt3_ctx (Context::new + RayTracingContext::new, renderer/mod.rs:32-45)."""

    def __init__(self, device: int = 0):
        self.lib = L.load()
        h = C.c_void_p()
        rc = self.lib.rt3_create(device, C.byref(h))
        if rc != 0:
            raise L.Rt3Error(rc, self.lib.rt3_last_error(None).decode())
        self.h = h

    def check(self, rc):
        if rc != 0:
            raise L.Rt3Error(rc, self.last_error())

    def close(self):
        if getattr(self, "h", None):
            self.lib.rt3_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_name(self):
        buf = C.create_string_buffer(256)
        self.check(self.lib.rt3_device_name(self.h, buf, 256))
        return buf.value.decode()

    def set_option(self, opt, value):
        self.check(self.lib.rt3_set_option(self.h, opt, int(value)))

    # ---- world buffers (world/mod.rs:83-125)
    def upload_mesh(self, mesh):
        v = np.ascontiguousarray(mesh.vertices, np.float32)
        i = np.ascontiguousarray(mesh.indices, np.uint32)
        g = np.ascontiguousarray(mesh.geometries)
        pc = np.ascontiguousarray(mesh.prim_counts, np.uint32)
        self.check(self.lib.rt3_scene_set_vertices(self.h, v.ctypes.data, len(v)))
        self.__dict__.pop("_skin_shapes", None)  # (rt3_scene_set_vertices forgets the skins)
        self.check(self.lib.rt3_scene_set_indices(self.h, i.ctypes.data, len(i)))
        self.check(self.lib.rt3_scene_set_geometry(self.h, g.ctypes.data, pc.ctypes.data, len(g)))
        cut = getattr(mesh, "alpha_cutoffs", None)
        if cut is not None and np.any(np.asarray(cut) != 0):  # alpha-masked geometry; opaque scenes make no call
            self.set_alpha_cutoffs(cut)
        mt = getattr(mesh, "material_textures", None)
        if mt is not None and len(mt) and any(np.any(mt[k] >= 0) for k in ("metallic_roughness_texture", "normal_texture", "emissive_texture")):
            self.set_material_textures(mt)  # material textures; scenes without them make no call
        tr = getattr(mesh, "transmission", None)
        if tr is not None and len(tr) and np.any(tr["transmission"] > 0):
            self.set_transmission(tr)  # glass; scenes without it make no call
        at = getattr(mesh, "attenuation", None)
        if at is not None and len(at) and np.any(at["sigma"] > 0):
            self.set_attenuation(at)  # absorbing glass; scenes without it make no call
        lights = getattr(mesh, "lights", None)
        if lights is not None and len(lights):  # punctual lights; scenes without them make no call
            self.set_lights(lights)
        for i, t in enumerate(getattr(mesh, "textures", None) or []):  # base-colour textures, RGBA8 sRGB
            t = np.ascontiguousarray(t, np.uint8)
            self.check(self.lib.rt3_scene_set_texture(self.h, i, t.ctypes.data, t.shape[1], t.shape[0]))

    def set_alpha_cutoffs(self, cutoffs):
        """per-geometry alpha cutoffs (glTF alphaMode MASK; 0 = opaque, [] = all opaque); rt3_scene_set_alpha_cutoffs, next build_accel()"""
        c = np.ascontiguousarray(cutoffs, np.float32).reshape(-1)
        self.check(self.lib.rt3_scene_set_alpha_cutoffs(self.h, c.ctypes.data, len(c)))

    def set_material_textures(self, table):
        """per-geometry metallic-roughness / normal / emissive texture indices and normal scale (assets.MATERIAL_TEXTURES_DTYPE; [] = none);
        rt3_scene_set_material_textures, next build_accel()"""
        from .assets import MATERIAL_TEXTURES_DTYPE

        t = np.ascontiguousarray(table, MATERIAL_TEXTURES_DTYPE).reshape(-1)
        self.check(self.lib.rt3_scene_set_material_textures(self.h, t.ctypes.data if len(t) else None, len(t)))

    def set_transmission(self, table):
        """per-geometry glass: transmission, index of refraction, thin-walled (assets.TRANSMISSION_DTYPE; [] = none);
        rt3_scene_set_transmission, next build_accel().  A built scene with glass needs a lens for "refrence_mode" (set_lens)."""
        from .assets import TRANSMISSION_DTYPE

        t = np.ascontiguousarray(table, TRANSMISSION_DTYPE).reshape(-1)
        self.check(self.lib.rt3_scene_set_transmission(self.h, t.ctypes.data if len(t) else None, len(t)))

    def set_attenuation(self, table):
        """per-geometry absorption coefficients sigma rgb, per world-space unit of length (assets.ATTENUATION_DTYPE, or an (n, 3) array;
        [] = none); rt3_scene_set_attenuation, next build_accel().  Only solid glass absorbs."""
        from .assets import ATTENUATION_DTYPE

        a = np.asarray(table)
        if a.dtype != ATTENUATION_DTYPE:
            sig = np.asarray(table, np.float32).reshape(-1, 3)
            a = np.zeros(len(sig), ATTENUATION_DTYPE)
            a["sigma"] = sig
        a = np.ascontiguousarray(a, ATTENUATION_DTYPE).reshape(-1)
        self.check(self.lib.rt3_scene_set_attenuation(self.h, a.ctypes.data if len(a) else None, len(a)))

    def attenuation_info(self):
        """flattened geometries the built structure holds as absorbing (rt3_attenuation_info): 0 = no table, k_absorb is not launched"""
        n = C.c_uint32(0)
        self.check(self.lib.rt3_attenuation_info(self.h, C.byref(n)))
        return int(n.value)

    def set_pane_shadows(self, on):
        """pane shadows (rt3_scene_set_pane_shadows): shadow rays cross thin-walled glass attenuated.  A mode of the
        context (set_geometry keeps it); a change takes effect at the next build_accel()."""
        self.check(self.lib.rt3_scene_set_pane_shadows(self.h, int(on)))

    def get_pane_shadows(self):
        on = C.c_int32(0)
        self.check(self.lib.rt3_scene_get_pane_shadows(self.h, C.byref(on)))
        return bool(on.value)

    def pane_shadow_info(self):
        """flattened geometries the built structure holds as panes (rt3_pane_shadow_info): 0 while the mode is off"""
        n = C.c_uint32(0)
        self.check(self.lib.rt3_pane_shadow_info(self.h, C.byref(n)))
        return int(n.value)

    def set_rough_transmission(self, on):
        """rough transmission (rt3_scene_set_rough_transmission): glass with roughness > 0 scatters through GGX
        microfacets.  A mode of the context (set_geometry keeps it); a change takes effect at the next build_accel()."""
        self.check(self.lib.rt3_scene_set_rough_transmission(self.h, int(on)))

    def get_rough_transmission(self):
        on = C.c_int32(0)
        self.check(self.lib.rt3_scene_get_rough_transmission(self.h, C.byref(on)))
        return bool(on.value)

    def rough_transmission_info(self):
        """flattened geometries the built structure holds as frosted (rt3_rough_transmission_info): 0 while the mode is off"""
        n = C.c_uint32(0)
        self.check(self.lib.rt3_rough_transmission_info(self.h, C.byref(n)))
        return int(n.value)

    def set_instances(self, instances):
        """instances: [(geometry_first, geometry_count, 4x4 matrix as numpy, object -> world)] -- Instance + Transform of
        src/renderer/world/mod.rs:46-60; [] = every geometry once under the identity.  Takes effect at the next build_accel()."""
        arr = (L.Instance * max(1, len(instances)))()
        for k, (first, count, m) in enumerate(instances):
            arr[k].geometry_first, arr[k].geometry_count = int(first), int(count)
            arr[k].transform[:] = [float(x) for x in np.asarray(m, np.float32).T.ravel()]  # column-major, like glam's Mat4
        self.check(self.lib.rt3_scene_set_instances(self.h, C.byref(arr), len(instances)))

    def set_prev_transforms(self, transforms=None):
        """the previous frame's 4x4 object -> world matrices, one per instance of the set_instances list, for the "motion" pass
        (rt3_scene_set_prev_transforms); None or [] forgets them: every instance counts as unmoved.  No rebuild is needed."""
        n = 0 if transforms is None else len(transforms)
        arr = np.ascontiguousarray([np.asarray(m, np.float32).T.ravel() for m in transforms], np.float32).reshape(n, 16) if n else None
        self.check(self.lib.rt3_scene_set_prev_transforms(self.h, arr.ctypes.data if n else None, n))

    def set_lights(self, lights=None):
        """the world's punctual lights (assets.LIGHT_DTYPE records; rt3_scene_set_lights), sampled under F_NEE_PUNCTUAL; None or [] forgets
        them.  No rebuild is needed: the next frame sees them."""
        from .assets import LIGHT_DTYPE

        arr = np.ascontiguousarray(np.zeros(0, LIGHT_DTYPE) if lights is None else lights, LIGHT_DTYPE).reshape(-1)
        self.check(self.lib.rt3_scene_set_lights(self.h, arr.ctypes.data if len(arr) else None, len(arr)))

    def light_masses(self, flags):
        """(n_emitters, n_punctual, masses uint32 in CDF units) of the light table that `flags` samples: emitter triangles first, then the
        punctual lights in set_lights order (rt3_light_masses)"""
        ne, npu = C.c_uint32(), C.c_uint32()
        self.check(self.lib.rt3_light_masses(self.h, int(flags), C.byref(ne), C.byref(npu), None))
        mass = np.zeros(ne.value + npu.value, np.uint32)
        if len(mass):
            self.check(self.lib.rt3_light_masses(self.h, int(flags), C.byref(ne), C.byref(npu), mass.ctypes.data))
        return ne.value, npu.value, mass

    def light_table(self, flags):
        """(records (n, 16) float32, cdf (n,) uint32, guide (cells + 1,) uint32, primitive ids (n,) uint32, areas (n,) float32, cells, shift) of
        the light table that `flags` samples, as the shading kernel reads it (rt3_light_table): record words {A, p_sel / area} {E1, Le.r}
        {E2, Le.g} {normal, Le.b}; entries in light_masses' order.  Empty arrays and cells = 0 when the combination samples nothing."""
        ne, npu, _ = self.light_masses(flags)
        cells, shift = C.c_uint32(), C.c_uint32()
        self.check(self.lib.rt3_light_table(self.h, int(flags), None, None, None, None, None, C.byref(cells), C.byref(shift)))
        n = ne + npu
        rec, cdf = np.zeros((n, 16), np.float32), np.zeros(n, np.uint32)
        guide = np.zeros(cells.value + 1 if n else 0, np.uint32)
        prim, area = np.zeros(n, np.uint32), np.zeros(n, np.float32)
        if n:
            self.check(self.lib.rt3_light_table(self.h, int(flags), rec.ctypes.data, cdf.ctypes.data, guide.ctypes.data, prim.ctypes.data, area.ctypes.data,
                                                C.byref(cells), C.byref(shift)))
        return rec, cdf, guide, prim, area, cells.value, shift.value

    def set_textured_emitters(self, on=True):
        """textured emitters (rt3_scene_set_textured_emitters): F_NEE_EMISSIVE also samples the geometries whose
        emission carries an emissive texture.  A mode of the light table alone: no rebuild is needed, the next frame sees it."""
        self.check(self.lib.rt3_scene_set_textured_emitters(self.h, int(on)))

    def get_textured_emitters(self):
        on = C.c_int32(0)
        self.check(self.lib.rt3_scene_get_textured_emitters(self.h, C.byref(on)))
        return bool(on.value)

    def light_emit_tex(self, flags):
        """the side array of the light table that `flags` samples (rt3_light_emit_tex): (uv (n, 3, 2) float32, emissive texture index (n,)
        int32, -1 = none), entries in light_masses' order; empty arrays when the table holds no textured emitter"""
        n = C.c_uint32()
        self.check(self.lib.rt3_light_emit_tex(self.h, int(flags), C.byref(n), None))
        out = np.zeros((n.value, 8), np.uint32)
        if n.value:
            self.check(self.lib.rt3_light_emit_tex(self.h, int(flags), C.byref(n), out.ctypes.data))
        return out[:, :6].copy().view(np.float32).reshape(-1, 3, 2), out[:, 6].copy().view(np.int32)

    def selftest_emit_radiance(self, flags, entries, b1, b2):
        """Self-test op 42: the emitter-side radiance Le (*) emissive texture of the table entries `entries` at barycentrics
        (1 - b1 - b2, b1, b2), over the light table `flags` samples.  Returns (n, 3) float32."""
        entries = np.ascontiguousarray(entries, np.uint32).reshape(-1)
        n = len(entries)
        rows = np.zeros((n, 3), np.uint32)
        rows[:, 0] = entries
        rows[:, 1] = np.ascontiguousarray(b1, np.float32).reshape(-1).view(np.uint32)
        rows[:, 2] = np.ascontiguousarray(b2, np.float32).reshape(-1).view(np.uint32)
        inp = np.concatenate([np.array([flags], np.uint32), rows.reshape(-1)])
        out = np.zeros((max(n, 1), 3), np.uint32)
        self.check(self.lib.rt3_selftest_eval(self.h, L.SELFTEST_EMIT_RADIANCE, inp.ctypes.data, n, out.ctypes.data))
        return out[:n].view(np.float32)

    def selftest_emit_tex_queue(self, flags, frame, bounces, bounce, s0, dims, pixels, records, groups, count=None):
        """Self-test op 43: k_emit_tex on the emitter shadow queue `records` (n, 4) of 32-bit words {contribution r, g, b, path id}, whose
        length word says `count` (n without), launched with `groups` workgroups over the pixel words `pixels` and the light table `flags`
        samples.  Returns the contributions (n, 3) uint32 afterwards.  The library fails the call when the kernel wrote anything else."""
        pixels = np.ascontiguousarray(pixels, np.uint32).reshape(-1)
        records = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 4)
        n = len(records)
        head = np.array([frame, bounces, bounce, s0, dims, len(pixels), groups, n if count is None else count, flags], np.uint32)
        inp = np.concatenate([head, pixels, records.reshape(-1)])
        out = np.zeros(3 * max(n, 1), np.uint32)
        self.check(self.lib.rt3_selftest_eval(self.h, L.SELFTEST_EMIT_TEX_QUEUE, inp.ctypes.data, n, out.ctypes.data))
        return out[: 3 * n].reshape(n, 3)

    def selftest_emit_mean(self, flags):
        """Self-test op 44: the mean texel (n, 3) float32 k_emit_tex_power found for every entry of the light table `flags` samples
        (1 1 1 for an entry without texture)"""
        ne, npu, _ = self.light_masses(flags)
        n = ne + npu
        out = np.zeros((max(n, 1), 3), np.float32)
        inp = np.array([flags], np.uint32)
        self.check(self.lib.rt3_selftest_eval(self.h, L.SELFTEST_EMIT_MEAN, inp.ctypes.data, n, out.ctypes.data))
        return out[:n]

    def selftest_light_table(self, power, area, k=()):
        """Self-test op 40: the light table's quantise, scan, CDF and guide kernels on the float32 powers and areas of n lights (the launch
        shapes and scratch layout of the context's own table), then light_find on the values `k` (< 2^23).  Returns (cells, shift, total,
        cdf (n,) uint32, p_sel / area (n,) float32, guide (cells + 1,) uint32, found (len(k),) uint32).  The library fails the call when a
        kernel wrote anything else."""
        power = np.ascontiguousarray(power, np.float32).reshape(-1)
        area = np.ascontiguousarray(area, np.float32).reshape(-1)
        k = np.ascontiguousarray(k, np.uint32).reshape(-1)
        n, n_k = len(power), len(k)
        assert len(area) == n
        cells = 1
        while cells < n and cells < (1 << 20):
            cells <<= 1
        inp = np.concatenate([np.array([n, n_k], np.uint32), power.view(np.uint32), area.view(np.uint32), k])
        out = np.zeros(3 + 2 * n + cells + 1 + n_k, np.uint32)
        self.check(self.lib.rt3_selftest_eval(self.h, L.SELFTEST_LIGHT_TABLE, inp.ctypes.data, n, out.ctypes.data))
        assert int(out[0]) == cells
        o = 3
        cdf, w = out[o:o + n], out[o + n:o + 2 * n].view(np.float32)
        guide = out[o + 2 * n:o + 2 * n + cells + 1]
        return int(out[0]), int(out[1]), int(out[2]), cdf, w, guide, out[o + 2 * n + cells + 1:]

    def snapshot_vertices(self):
        """the positions the vertex buffer holds now become the previous frame's (rt3_scene_snapshot_vertices): the "motion" pass follows
        geometries that update_vertices() deforms afterwards.  A device-side copy of the ranges updated since the last snapshot."""
        self.check(self.lib.rt3_scene_snapshot_vertices(self.h))

    def forget_prev_vertices(self):
        """no previous positions (rt3_scene_forget_prev_vertices): "motion" sees no deformed geometry"""
        self.check(self.lib.rt3_scene_forget_prev_vertices(self.h))

    def deformed_geometries(self, n):
        """one bool per geometry of the uploaded mesh (`n` of them): does a position word inside its vertex span differ from the snapshot?
        (rt3_scene_deformed_geometries)"""
        flags = np.zeros(int(n), np.uint8)
        self.check(self.lib.rt3_scene_deformed_geometries(self.h, flags.ctypes.data, len(flags)))
        return flags.astype(bool)

    # ---- skins
    def add_skin(self, first_vertex, joints, weights, n_joints, rest=None, target_dpos=None, target_dnrm=None):
        """a skin over vertices [first_vertex, first_vertex + len(joints)) (rt3_scene_add_skin): joints (n, 4) uint16, weights (n, 4), rest
        (n, 8) Vertex rows or None = the range's current contents, target_dpos / target_dnrm (n_targets, n, 3) or None.  Returns its index."""
        j = np.ascontiguousarray(joints, np.uint16).reshape(-1, 4)
        w = np.ascontiguousarray(weights, np.float32).reshape(-1, 4)
        n = len(j)
        r = None if rest is None else np.ascontiguousarray(rest, np.float32).reshape(-1, 8)
        dp = None if target_dpos is None or len(target_dpos) == 0 else np.ascontiguousarray(target_dpos, np.float32).reshape(-1, n, 3)
        dn = None if target_dnrm is None or len(target_dnrm) == 0 else np.ascontiguousarray(target_dnrm, np.float32).reshape(-1, n, 3)
        if len(w) != n or (r is not None and len(r) != n) or (dn is not None and (dp is None or len(dn) != len(dp))):
            raise ValueError("add_skin: the arrays disagree about the vertex or target count")
        d = L.SkinDesc(int(first_vertex), n, int(n_joints), 0 if dp is None else len(dp), None if r is None else r.ctypes.data, j.ctypes.data, w.ctypes.data,
                       None if dp is None else dp.ctypes.data, None if dn is None else dn.ctypes.data)
        out = C.c_uint32()
        self.check(self.lib.rt3_scene_add_skin(self.h, C.byref(d), C.byref(out)))
        self.__dict__.setdefault("_skin_shapes", {})[out.value] = (int(n_joints), d.n_targets)  # what pose_skin's arrays must hold
        return out.value

    def clear_skins(self):
        """forget every skin (rt3_scene_clear_skins); the vertex buffer keeps what the last pose wrote"""
        self.check(self.lib.rt3_scene_clear_skins(self.h))
        self.__dict__.pop("_skin_shapes", None)

    def pose_skin(self, skin, palette, target_weights=None):
        """pose skin `skin` (rt3_scene_pose_skin): palette (n_joints, 4, 4), matrices that act on column vectors like set_instances', and the
        target weights.  Stream-ordered, no wait; a built structure is stale until refit_accel()."""
        m = np.ascontiguousarray(np.asarray(palette, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))  # column-major, like glam's Mat4
        a = None if target_weights is None or len(target_weights) == 0 else np.ascontiguousarray(target_weights, np.float32).reshape(-1)
        shape = self.__dict__.get("_skin_shapes", {}).get(int(skin))
        if shape is not None and (len(m), 0 if a is None else len(a)) != shape:  # (the library reads as many as the skin has)
            raise ValueError(f"pose_skin: skin {skin} has {shape[0]} joints and {shape[1]} targets")
        self.check(self.lib.rt3_scene_pose_skin(self.h, int(skin), m.ctypes.data, None if a is None else a.ctypes.data))

    def skin_info(self):
        """(number of skins, device bytes they hold) (rt3_skin_info)"""
        n, b = C.c_uint32(), C.c_uint64()
        self.check(self.lib.rt3_skin_info(self.h, C.byref(n), C.byref(b)))
        return n.value, b.value

    def download_vertices(self, first, n):
        """rows [first, first + n) of the vertex buffer as the device holds them, (n, 8) float32 (rt3_scene_download_vertices); synchronises"""
        out = np.zeros((int(n), 8), np.float32)
        self.check(self.lib.rt3_scene_download_vertices(self.h, out.ctypes.data if n else None, int(first), int(n)))
        return out

    def set_sky(self, rgb):
        s = np.ascontiguousarray(rgb, np.float32)
        self.check(self.lib.rt3_scene_set_sky(self.h, s.ctypes.data, s.shape[1], s.shape[0]))

    def set_bluenoise(self, rgba):
        b = np.ascontiguousarray(rgba, np.uint8)
        self.check(self.lib.rt3_scene_set_bluenoise(self.h, b.ctypes.data, b.shape[1], b.shape[0]))

    def build_accel(self) -> int:
        out = C.c_uint32()
        self.check(self.lib.rt3_accel_build(self.h, C.byref(out)))
        return out.value

    def update_vertices(self, vertices, first=0):
        """overwrite vertices [first, first + len(vertices)) in place (rt3_scene_update_vertices; rows of the 8-float Vertex).  A built
        structure is stale until refit_accel() or build_accel()."""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 8)
        self.check(self.lib.rt3_scene_update_vertices(self.h, v.ctypes.data, int(first), len(v)))

    def refit_accel(self) -> int:
        """recompute the boxes of the last build from the current vertices, same topology (rt3_accel_refit)"""
        out = C.c_uint32()
        self.check(self.lib.rt3_accel_refit(self.h, C.byref(out)))
        return out.value

    def light_info(self):
        """(n_emitters, cdf_total) of the RT3_F_NEE_EMISSIVE emitter table (rt3_light_info)"""
        n, t = C.c_uint32(), C.c_uint64()
        self.check(self.lib.rt3_light_info(self.h, C.byref(n), C.byref(t)))
        return n.value, t.value

    def light_download(self):
        """(primitive ids uint32, areas float32, masses uint32 in CDF units) of the emitter table (rt3_light_download)"""
        n, _ = self.light_info()
        prim, area, mass = np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros(n, np.uint32)
        self.check(self.lib.rt3_light_download(self.h, prim.ctypes.data, area.ctypes.data, mass.ctypes.data))
        return prim, area, mass

    def accel_import(self, nodes, tris):
        """install a tree built elsewhere over the same triangles (rt3_accel_download's format)"""
        n = np.ascontiguousarray(nodes)
        t = np.ascontiguousarray(tris)
        self.check(self.lib.rt3_accel_import(self.h, n.ctypes.data, n.nbytes, t.ctypes.data, t.nbytes))

    def accel_info(self):
        """(n_nodes, n_tris, levels, node_bytes)"""
        a, b, c, d = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        self.check(self.lib.rt3_accel_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    def accel_levels(self):
        """(n_meshes, n_meshes_built, n_top_nodes, accel_bytes) of the last build: rt3_accel_levels (instance mode 0: 0, 0, 0, bytes)"""
        a, b, c, d = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        self.check(self.lib.rt3_accel_levels(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    def exit_table_info(self):
        """(cells, tried, occluded, in_use) of k_shadow's exit table (rt3_accel_exit_table_info): 0 cells = no table"""
        a, b, c, d = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        self.check(self.lib.rt3_accel_exit_table_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    def accel_download(self):
        nn, nt, _, nb = self.accel_info()
        nodes = np.empty((nn, nb // 4), np.uint32)
        tris = np.empty((nt, 12), np.uint32)
        self.check(self.lib.rt3_accel_download(self.h, nodes.ctypes.data, nodes.nbytes, tris.ctypes.data, tris.nbytes))
        return nodes, tris

    def sky_download(self, w, h):
        """(alias words, RGB9E5 texels, marginal CDF, realised (u,v) density)"""
        al, tx, cm, pu = np.empty((h, w), np.uint32), np.empty((h, w), np.uint32), np.empty(h, np.float32), np.empty((h, w), np.float32)
        self.check(self.lib.rt3_sky_download(self.h, al.ctypes.data, tx.ctypes.data, cm.ctypes.data, pu.ctypes.data))
        return al, tx, cm, pu

    def trace_rays(self, rays, any_hit=False, counts=False, repeat=1):
        """rays (8, n) float32 host SoA -> (t,u,v,prim[,n_nodes,n_tris], kernel_ms)"""
        rays = np.ascontiguousarray(rays, np.float32)
        n = rays.shape[1]
        t, u, v = (np.zeros(n, np.float32) for _ in range(3))
        prim = np.zeros(n, np.uint32)
        cn = np.zeros(n, np.uint32) if counts else None
        ct = np.zeros(n, np.uint32) if counts else None
        ms = C.c_double()
        self.check(self.lib.rt3_trace_rays(self.h, rays.ctypes.data, n, int(any_hit), t.ctypes.data, u.ctypes.data, v.ctypes.data, prim.ctypes.data,
                                           cn.ctypes.data if counts else None, ct.ctypes.data if counts else None, repeat, C.byref(ms)))
        return (t, u, v, prim, cn, ct, ms.value) if counts else (t, u, v, prim, ms.value)

    def selftest(self, op, inp, out_words, out_dtype=np.uint32):
        """Evaluate device function `op` (include/rt3.h: rt3_selftest_eval) on the rows of `inp` (32-bit words)."""
        inp = np.ascontiguousarray(inp)
        assert inp.dtype.itemsize == 4
        n = inp.shape[0]
        out = np.zeros((n, out_words), out_dtype)
        self.check(self.lib.rt3_selftest_eval(self.h, op, inp.ctypes.data, n, out.ctypes.data))
        return out

    def set_denoise_params(self, params=None, **kw):
        """parameters of the "denoise" pass (rt3_denoise_set_params): an L.DenoiseParams, or its fields as keywords; nothing = the defaults"""
        if params is None and kw:
            params = L.DenoiseParams(**kw)
        self.check(self.lib.rt3_denoise_set_params(self.h, C.byref(params) if params is not None else None))

    def set_denoise_variance_input(self, moments_image=0):
        """the "temporal" pass's Moments image whose variance "denoise" starts from (rt3_denoise_set_variance_input); 0 = none"""
        self.check(self.lib.rt3_denoise_set_variance_input(self.h, int(moments_image)))

    def set_temporal_params(self, params=None, **kw):
        """parameters of the "temporal" pass (rt3_temporal_set_params): an L.TemporalParams, or its fields as keywords; nothing = the defaults"""
        if params is None and kw:
            params = L.TemporalParams(**kw)
        self.check(self.lib.rt3_temporal_set_params(self.h, C.byref(params) if params is not None else None))

    def set_prev_view(self, gconst=None):
        """the previous frame's GConst for the "temporal" pass (rt3_temporal_set_prev_view); None forgets it"""
        if gconst is None:
            self.check(self.lib.rt3_temporal_set_prev_view(self.h, None, 0))
        else:
            self.check(self.lib.rt3_temporal_set_prev_view(self.h, C.byref(gconst), C.sizeof(gconst)))

    def set_temporal_motion_input(self, motion_image=0):
        """the "motion" pass's image that "temporal" follows moved instances with (rt3_temporal_set_motion_input); 0 = none"""
        self.check(self.lib.rt3_temporal_set_motion_input(self.h, int(motion_image)))

    def adaptive_set_params(self, params=None, **kw):
        """parameters of the "adaptive" pass (rt3_adaptive_set_params): an L.AdaptiveParams, or its fields as keywords; nothing = the defaults"""
        if params is None and kw:
            params = L.AdaptiveParams(**kw)
        self.check(self.lib.rt3_adaptive_set_params(self.h, C.byref(params) if params is not None else None))

    def adaptive_info(self):
        """(rounds, paths_traced, pixels_capped) of the last "adaptive" launch (rt3_adaptive_info)"""
        r, p, k = C.c_uint32(), C.c_uint64(), C.c_uint32()
        self.check(self.lib.rt3_adaptive_info(self.h, C.byref(r), C.byref(p), C.byref(k)))
        return r.value, p.value, k.value

    def adaptive_set_coverage(self, on):
        """coverage mode of the "adaptive" pass (rt3_adaptive_set_coverage): with a lens set the pass lists every pixel
        of the rank and starts each sample from its own camera ray, instead of refusing.  A mode of the context: it outlives scene changes."""
        self.check(self.lib.rt3_adaptive_set_coverage(self.h, int(on)))

    def adaptive_coverage(self):
        on = C.c_int()
        self.check(self.lib.rt3_adaptive_get_coverage(self.h, C.byref(on)))
        return bool(on.value)

    def set_lens(self, params=None, **kw):
        """per-sample camera rays (rt3_camera_set_lens): an L.LensParams, or its fields as keywords; nothing = off"""
        if params is None and kw:
            params = L.LensParams(**kw)
        self.check(self.lib.rt3_camera_set_lens(self.h, C.byref(params) if params is not None else None))

    def get_lens(self):
        """(L.LensParams last set, whether a lens is on) (rt3_camera_get_lens)"""
        p, on = L.LensParams(), C.c_int()
        self.check(self.lib.rt3_camera_get_lens(self.h, C.byref(p), C.byref(on)))
        return p, bool(on.value)

    @staticmethod
    def _guide_images(images):
        """an L.GuideImages from one, from a dict with its four names, or from four handles in the order position, normal, albedo, emission"""
        if images is None or isinstance(images, L.GuideImages):
            return images
        if isinstance(images, dict):
            return L.GuideImages(**{k: int(images[k]) for k in ("position", "normal", "albedo", "emission")})
        return L.GuideImages(*[int(h) for h in images])

    def set_guide_output(self, images=None):
        """the four RGBA32F images a lens frame's "refrence_mode" writes its guide into (rt3_camera_set_guide_output):
        an L.GuideImages, a dict {position, normal, albedo, emission} or four handles in that order; None = off, the default"""
        g = self._guide_images(images)
        self.check(self.lib.rt3_camera_set_guide_output(self.h, C.byref(g) if g is not None else None))

    def get_guide_output(self):
        """(L.GuideImages last set, whether the output is on) (rt3_camera_get_guide_output)"""
        g, on = L.GuideImages(), C.c_int()
        self.check(self.lib.rt3_camera_get_guide_output(self.h, C.byref(g), C.byref(on)))
        return g, bool(on.value)

    def set_denoise_guide_input(self, images=None):
        """the guide images "denoise" reads in the G-buffer's place (rt3_denoise_set_guide_input); None = the G-buffer, the default"""
        g = self._guide_images(images)
        self.check(self.lib.rt3_denoise_set_guide_input(self.h, C.byref(g) if g is not None else None))

    def set_temporal_guide_input(self, current=None, previous=None):
        """the guide images of this frame and of the previous one that "temporal" takes its surface records from in the G-buffer's place
        (rt3_temporal_set_guide_input); both None = the G-buffer, the default; one None is refused"""
        cur, prev = self._guide_images(current), self._guide_images(previous)
        self.check(self.lib.rt3_temporal_set_guide_input(self.h, C.byref(cur) if cur is not None else None, C.byref(prev) if prev is not None else None))

    def selftest_guide_queue(self, pixels, records, nsb, samples, first, last, groups, prefill=None):
        """Self-test op 39: k_lens_guide on the camera and hit queues `records` (nsb * npix, 10) of 32-bit words {o xyz, d xyz, t, bu, bv, prim}
        (record sample_in_batch * npix + pixel index) over the pixel words `pixels` and the built scene, launched with `groups`
        workgroups; `prefill` (npix, 16): the four images' words at the listed pixels before the launch (zeros without).  Returns them
        afterwards, (npix, 16) uint32: {position, normal, albedo, emission}.  The library fails the call when the kernel wrote anything else."""
        pixels = np.ascontiguousarray(pixels, np.uint32).reshape(-1)
        records = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 10)
        npix, n = len(pixels), len(records)
        head = np.array([npix, nsb, samples, int(first), int(last), groups], np.uint32)
        inp = np.concatenate([head, pixels, records.reshape(-1)])
        out = np.zeros(16 * max(npix, 1), np.uint32)
        if prefill is not None:
            out[: 16 * npix] = np.ascontiguousarray(prefill).view(np.uint32).reshape(-1)
        self.check(self.lib.rt3_selftest_eval(self.h, L.SELFTEST_GUIDE_QUEUE, inp.ctypes.data, n, out.ctypes.data))
        return out[: 16 * npix].reshape(npix, 16)

    def set_guide_motion_output(self, image=0):
        """the fifth guide image a lens frame's "refrence_mode" writes beside the four: the samples' mean previous position
        (rt3_camera_set_guide_motion_output); an RGBA32F image handle, 0 = off, the default"""
        self.check(self.lib.rt3_camera_set_guide_motion_output(self.h, int(image)))

    def get_guide_motion_output(self):
        """the handle last set (rt3_camera_get_guide_motion_output); 0: off"""
        image = C.c_uint32()
        self.check(self.lib.rt3_camera_get_guide_motion_output(self.h, C.byref(image)))
        return int(image.value)

    def set_temporal_guide_motion_input(self, image=0):
        """the image of set_guide_motion_output as the point a guided "temporal" looks up in the previous frame
        (rt3_temporal_set_guide_motion_input); 0 = none, the default"""
        self.check(self.lib.rt3_temporal_set_guide_motion_input(self.h, int(image)))

    def selftest_guide_prev_queue(self, pixels, records, nsb, samples, first, last, groups, prefill=None):
        """Self-test op 41: k_lens_guide_prev on the queues of selftest_guide_queue, over the built scene and the context's current motion
        tables (set_prev_transforms, snapshot_vertices); `prefill` (npix, 4): the image's words at the listed pixels before the launch
        (zeros without).  Returns them afterwards, (npix, 4) uint32.  The library fails the call when the kernel wrote anything else."""
        pixels = np.ascontiguousarray(pixels, np.uint32).reshape(-1)
        records = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 10)
        npix, n = len(pixels), len(records)
        head = np.array([npix, nsb, samples, int(first), int(last), groups], np.uint32)
        inp = np.concatenate([head, pixels, records.reshape(-1)])
        out = np.zeros(4 * max(npix, 1), np.uint32)
        if prefill is not None:
            out[: 4 * npix] = np.ascontiguousarray(prefill).view(np.uint32).reshape(-1)
        self.check(self.lib.rt3_selftest_eval(self.h, L.SELFTEST_GUIDE_PREV_QUEUE, inp.ctypes.data, n, out.ctypes.data))
        return out[: 4 * npix].reshape(npix, 4)

    def set_roulette(self, params=None, **kw):
        """Russian roulette on extension rays (rt3_path_set_roulette): an L.RouletteParams, or its fields as keywords;
        nothing = off"""
        if params is None and kw:
            params = L.RouletteParams(**kw)
        self.check(self.lib.rt3_path_set_roulette(self.h, C.byref(params) if params is not None else None))

    def get_roulette(self):
        """(L.RouletteParams last set, whether roulette is on) (rt3_path_get_roulette)"""
        p, on = L.RouletteParams(), C.c_int()
        self.check(self.lib.rt3_path_get_roulette(self.h, C.byref(p), C.byref(on)))
        return p, bool(on.value)

    def roulette_info(self):
        """(extension rays tested, of them ended) of the last "refrence_mode" / "adaptive" launch (rt3_path_roulette_info); synchronises"""
        t, e = C.c_uint64(), C.c_uint64()
        self.check(self.lib.rt3_path_roulette_info(self.h, C.byref(t), C.byref(e)))
        return t.value, e.value

    def selftest_roulette_queue(self, frame, bounces, bounce, s0, min_survival, pixels, records, groups, prefill=None):
        """Self-test op 34: k_roulette on the queue `records` (n, 11) of 32-bit words {o xyz, pdf, d xyz, path id, T rgb}, launched with `groups`
        workgroups over the pixel words `pixels`; `prefill` (n, 11): the destination queue's words before the launch (zeros without).
        Returns (count, tested, ended, the destination queue (n, 11) uint32 afterwards)."""
        pixels = np.ascontiguousarray(pixels, np.uint32).reshape(-1)
        records = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 11)
        n = len(records)
        head = np.array([frame, bounces, bounce, s0, np.float32(min_survival).view(np.uint32), len(pixels), groups], np.uint32)
        inp = np.concatenate([head, pixels, records.reshape(-1)])
        out = np.zeros(3 + 11 * n, np.uint32)
        if prefill is not None:
            out[3:] = np.ascontiguousarray(prefill).view(np.uint32).reshape(-1)
        self.check(self.lib.rt3_selftest_eval(self.h, L.SELFTEST_ROULETTE_QUEUE, inp.ctypes.data, n, out.ctypes.data))
        return int(out[0]), int(out[1]), int(out[2]), out[3:].reshape(n, 11)

    def selftest_adaptive_compact(self, W, H, dilate, mask, records, prefill_xy=None, prefill_bn=None):
        """Self-test op 35: the "adaptive" pass's list compaction on the list `records` (n, 2) of 32-bit words {x | y << 16, blue-noise word}
        under the window-space `mask` (H, W) of bytes; `prefill_xy` (n,) and `prefill_bn` (n, 2): the destination lists' words before the
        launch (zeros without).  Returns (count, the exclusive block offsets (n_blocks,), the destination xy list (n,), the destination
        {xy, blue-noise} list (n, 2)), all uint32."""
        mask = np.ascontiguousarray(mask, np.uint8).reshape(-1)
        records = np.ascontiguousarray(records, np.uint32).reshape(-1, 2)
        n = len(records)
        n_blocks = -(-n // L.ADAPTIVE_TILE)
        inp = np.zeros(4 + -(-len(mask) // 4) + 2 * n, np.uint32)
        inp[:4] = W, H, dilate, n
        inp[4:].view(np.uint8)[:len(mask)] = mask
        inp[len(inp) - 2 * n:] = records.reshape(-1)
        out = np.zeros(2 + n_blocks + 3 * n, np.uint32)
        if prefill_xy is not None:
            out[2 + n_blocks:2 + n_blocks + n] = np.ascontiguousarray(prefill_xy, np.uint32).reshape(-1)
        if prefill_bn is not None:
            out[2 + n_blocks + n:] = np.ascontiguousarray(prefill_bn, np.uint32).reshape(-1)
        self.check(self.lib.rt3_selftest_eval(self.h, L.SELFTEST_ADAPTIVE_COMPACT, inp.ctypes.data, n, out.ctypes.data))
        assert int(out[1]) == n_blocks
        return int(out[0]), out[2:2 + n_blocks], out[2 + n_blocks:2 + n_blocks + n], out[2 + n_blocks + n:].reshape(n, 2)

    def selftest_absorb(self, rows):
        """Self-test op 36: the absorption rule on rows (n, 13) float32 {T rgb, sigma rgb, t, d xyz, n xyz}.  Returns (T' (n, 3) float32,
        applied (n,) bool)."""
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 13)
        out = np.zeros((len(rows), 4), np.uint32)
        self.check(self.lib.rt3_selftest_eval(self.h, L.SELFTEST_ABSORB, rows.ctypes.data, len(rows), out.ctypes.data))
        return out[:, :3].copy().view(np.float32), out[:, 3] != 0

    def selftest_absorb_queue(self, records, groups):
        """Self-test op 37: k_absorb on the queue `records` (n, 10) of 32-bit words {d xyz, t, u, v, prim, T rgb} over the built scene,
        launched with `groups` workgroups.  Returns T' (n, 3) uint32.  The library fails the call when the kernel wrote anything but the
        throughput words of the n records."""
        records = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 10)
        n = len(records)
        inp = np.concatenate([np.array([groups], np.uint32), records.reshape(-1)])
        out = np.zeros(3 * max(n, 1), np.uint32)
        self.check(self.lib.rt3_selftest_eval(self.h, L.SELFTEST_ABSORB_QUEUE, inp.ctypes.data, n, out.ctypes.data))
        return out[: 3 * n].reshape(n, 3)

    def set_medium(self, medium=None, **kw):
        """fog (rt3_scene_set_medium): an L.Medium, or its fields as keywords; nothing = off.  Needs per-sample camera
        rays (set_lens); the acceleration structure stays as it is."""
        if medium is None and kw:
            medium = L.Medium(**kw)
        self.check(self.lib.rt3_scene_set_medium(self.h, C.byref(medium) if medium is not None else None))

    def get_medium(self):
        """(L.Medium last set, whether a medium is on) (rt3_scene_get_medium)"""
        m, on = L.Medium(), C.c_int()
        self.check(self.lib.rt3_scene_get_medium(self.h, C.byref(m), C.byref(on)))
        return m, bool(on.value)

    def medium_info(self):
        """(traced segments that ran through the medium, in-scatter shadow rays queued) of the last "refrence_mode" / "adaptive" launch
        (rt3_medium_info); synchronises"""
        a, b = C.c_uint64(), C.c_uint64()
        self.check(self.lib.rt3_medium_info(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def selftest_fog(self, rows):
        """Self-test op 45: the fog rule on rows (n, 20) float32 {o, d, t, box_min, box_max, sigma_a, sigma_s, u}.  Returns (in medium (n,)
        bool, {t0, t1, s, pdf, Tr rgb} (n, 7) float32)."""
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 20)
        out = np.zeros((len(rows), 8), np.uint32)
        self.check(self.lib.rt3_selftest_eval(self.h, L.SELFTEST_FOG, rows.ctypes.data, len(rows), out.ctypes.data))
        return out[:, 0] != 0, out[:, 1:].copy().view(np.float32)

    def selftest_fog_segment(self, records, pixels, groups, flags, frame, bounces, segment, s0=0, miss_radiance=False):
        """Self-test op 46, kind 0: k_fog_segment with the context's medium on the queue `records` (n, 12) of 32-bit words {o xyz, d xyz, t,
        prim, T rgb, path id}, launched with `groups` workgroups over the pixel words `pixels`.  Returns a dict: counts (2,), segments, rays,
        T (n, 3) uint32, radiance (n, 4) uint32, queues: two (n, 12) uint32 arrays {x, c.r, w_l, c.g, c.b, path id, tmax, 0}."""
        pixels = np.ascontiguousarray(pixels, np.uint32).reshape(-1)
        records = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 12)
        n = len(records)
        head = np.array([0, groups, flags, frame, bounces, segment, s0, len(pixels), int(miss_radiance)], np.uint32)
        inp = np.concatenate([head, pixels, records.reshape(-1)])
        out = np.zeros(4 + 31 * n, np.uint32)
        self.check(self.lib.rt3_selftest_eval(self.h, L.SELFTEST_FOG_QUEUE, inp.ctypes.data, n, out.ctypes.data))
        body = out[4:]
        return dict(counts=out[0:2].copy(), segments=int(out[2]), rays=int(out[3]), T=body[: 3 * n].reshape(n, 3), radiance=body[3 * n : 7 * n].reshape(n, 4),
                    queues=[body[7 * n + 12 * n * k : 7 * n + 12 * n * (k + 1)].reshape(n, 12) for k in range(2)])

    def selftest_fog_shadow(self, records, groups, with_tmax):
        """Self-test op 46, kinds 1 and 2: k_fog_shadow with the context's medium on the shadow queue `records` (n, 11) of 32-bit words
        {o xyz, c.r, d xyz, c.g, c.b, path id, tmax}; without `with_tmax` the rays run to the box's exit.  Returns the contributions (n, 3)
        uint32 after the launch."""
        records = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 11)
        n = len(records)
        head = np.array([2 if with_tmax else 1, groups, 0, 0, 1, 0, 0, 1, 0], np.uint32)
        inp = np.concatenate([head, np.zeros(1, np.uint32), records.reshape(-1)])
        out = np.zeros(3 * max(n, 1), np.uint32)
        self.check(self.lib.rt3_selftest_eval(self.h, L.SELFTEST_FOG_QUEUE, inp.ctypes.data, n, out.ctypes.data))
        return out[: 3 * n].reshape(n, 3)

    def stats_reset(self):
        self.check(self.lib.rt3_stats_reset(self.h))

    def stats(self) -> L.Stats:
        s = L.Stats()
        self.check(self.lib.rt3_stats_get(self.h, C.byref(s)))
        return s

    def pass_launch(self, name, x, y, z, gconst, bindings, entry="main") -> int:
        """rt3_pass_launch of pass `name` over x * y * z with the handles `bindings`; returns the code (check() raises on one)"""
        b = (C.c_uint32 * max(1, len(bindings)))(*bindings)
        return self.lib.rt3_pass_launch(self.h, name.encode(), entry.encode(), x, y, z, C.byref(gconst), C.sizeof(gconst), b, len(bindings))

    def last_error(self) -> str:
        return self.lib.rt3_last_error(self.h).decode()

    def wait(self):
        self.check(self.lib.rt3_frame_wait(self.h))

    def set_tile_partition(self, w, h, rank, n_ranks):
        self.check(self.lib.rt3_set_tile_partition(self.h, w, h, rank, n_ranks))

    def tile_pixel_count(self, rank, n_ranks):
        out = C.c_uint32()
        self.check(self.lib.rt3_tile_pixel_count(self.h, rank, n_ranks, C.byref(out)))
        return out.value

    # ---- frame-end gather (include/rt3.h: rt3_comm_* / rt3_gather_*)
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(L.COMM_ID_BYTES)
        rc = self.lib.rt3_comm_unique_id(buf)
        if rc != 0:
            raise L.Rt3Error(rc, self.lib.rt3_last_error(None).decode())
        return buf.raw

    def comm_init(self, uid: bytes, rank: int, n_ranks: int):
        assert len(uid) == L.COMM_ID_BYTES
        self.check(self.lib.rt3_comm_init(self.h, C.c_char_p(uid), rank, n_ranks))

    def comm_destroy(self):
        self.check(self.lib.rt3_comm_destroy(self.h))

    def gather_tiles(self, image, root=0):
        self.check(self.lib.rt3_gather_tiles(self.h, image, root))

    def gather_layout(self, image, root, n_ranks):
        off = (C.c_uint64 * (n_ranks + 1))()
        self.check(self.lib.rt3_gather_layout(self.h, image, root, n_ranks, off))
        return [int(x) for x in off]

    def gather_unpack(self, image, root, n_ranks, recv_device_ptr):
        self.check(self.lib.rt3_gather_unpack(self.h, image, root, n_ranks, C.c_void_p(recv_device_ptr)))


class NodeBuilder:
    """build.rs:32-209"""

    def __init__(self, rg, name, kind):
        if any(n.name == name for n in rg.nodes):
            raise ValueError(f"Node name {name} allready used")  # build.rs:57-59 (panic there)
        self.rg = rg
        self.node = Node(name, kind, "", "main", WorkSize2D.FullScreen if kind == "raytracing" else DispatchSize.FullScreen, None)

    def shader(self, path):
        self.node.path = path
        return self

    def entry(self, entry):
        self.node.entry = entry
        return self

    def constants(self, c):
        self.node.constants = c
        return self

    def _edge(self, origin, handle, typ):
        if typ == "ShaderRead" and origin != IMPORTED:  # build.rs:96-107
            prev = [e for e in self.rg.nodes[origin].edges if e.resource == handle]
            if not prev:
                raise ValueError("Origin doesnt write to handle")
            if prev[0].edge_type == "ShaderRead":
                raise ValueError("Origin contains handle but does not write to it")
        self.node.edges.append(NodeEdge(None if origin == IMPORTED else origin, typ, handle))
        return self

    def read(self, origin, handle):
        return self._edge(origin, handle, "ShaderRead")

    def write(self, last_read, handle):
        return self._edge(last_read, handle, "ShaderWrite")

    def read_write(self, origin, handle):
        return self._edge(origin, handle, "ShaderReadWrite")

    # Context-state edges (no reference counterpart): an image the pass reaches through a context setter (ctx.set_guide_output,
    # ctx.set_denoise_guide_input), not through its bindings.  They order the nodes like any edge and are left out of the binding list.
    def state_write(self, handle):
        return self._edge(IMPORTED, handle, "StateWrite")

    def state_read(self, origin, handle):
        if origin != IMPORTED and not any(e.resource == handle and e.edge_type != "StateRead" for e in self.rg.nodes[origin].edges):
            raise ValueError("Origin doesnt write to handle")
        self.node.edges.append(NodeEdge(None if origin == IMPORTED else origin, "StateRead", handle))
        return self

    def _build(self):
        seen = set()
        for e in self.node.edges:  # build.rs:195-198
            if e.resource in seen:
                raise ValueError(f"resource: {e.resource} is duplicate")
            seen.add(e.resource)
        self.rg.nodes.append(self.node)
        return len(self.rg.nodes) - 1

    def launch(self, size=None):  # RayTracingPass, build.rs:380-383
        assert self.node.kind == "raytracing"
        self.node.size = size or WorkSize2D.FullScreen
        return self._build()

    def dispatch(self, size=None):  # ComputePass, build.rs:395-398
        assert self.node.kind == "compute"
        self.node.size = size or DispatchSize.FullScreen
        return self._build()


class RayTracingPass:
    @staticmethod
    def new(rg, name):  # executions.rs:86-101
        return NodeBuilder(rg, name, "raytracing")


class ComputePass:
    @staticmethod
    def new(rg, name):  # executions.rs:21-36
        return NodeBuilder(rg, name, "compute")


class RenderGraph:
    """render_graph/mod.rs:291-532 reduced to what a HIP stream needs: named resources + per-frame node list."""

    def __init__(self, ctx: Context, window):
        self.ctx, self.window = ctx, (int(window[0]), int(window[1]))
        self.nodes: list[Node] = []
        self.named: dict[str, int] = {}
        self.frame_number = 0

    # mod.rs:440-483 : created on first use, looked up by name afterwards
    def image(self, size: ImageSize, fmt: int, name: str) -> int:
        if name in self.named:
            return self.named[name]
        w, h = size.size(self.window)
        out = C.c_uint32()
        self.ctx.check(self.ctx.lib.rt3_image_create(self.ctx.h, w, h, fmt, C.byref(out)))
        self.named[name] = out.value
        return out.value

    def buffer(self, size: int, name: str) -> int:
        if name in self.named:
            return self.named[name]
        out = C.c_uint32()
        self.ctx.check(self.ctx.lib.rt3_buffer_create(self.ctx.h, size, C.byref(out)))
        self.named[name] = out.value
        return out.value

    def import_image(self, device_ptr: int, w: int, h: int, fmt: int, name: str) -> int:  # mod.rs:426-438
        out = C.c_uint32()
        self.ctx.check(self.ctx.lib.rt3_image_import(self.ctx.h, C.c_void_p(device_ptr), w, h, fmt, C.byref(out)))
        self.named[name] = out.value
        return out.value

    def begin_frame(self):  # mod.rs:656-686
        self.nodes = []

    def bake(self, root: int):  # bake.rs:29-49
        order = []

        def flatten(n):
            order.append(n)
            for e in self.nodes[n].edges:
                if e.origin is not None:
                    flatten(e.origin)

        flatten(root)
        out = []
        for n in reversed(order):
            if n not in out:
                out.append(n)
        return out

    def draw_frame(self, output: int, wait: bool = False):
        """mod.rs:534-655 : find the root (the node touching `output`, :553-562), bake, execute in order."""
        roots = [i for i, n in enumerate(self.nodes) if any(e.resource == output for e in n.edges)]
        if not roots:
            raise ValueError("no node touches the output resource")
        for ni in self.bake(roots[-1]):
            n = self.nodes[ni]
            x, y, z = (*n.size.size(self.window), 1) if n.kind == "raytracing" else n.size.size(self.window)
            bindings = [e.resource for e in n.edges if not e.edge_type.startswith("State")]  # bake.rs:51-83
            self.ctx.check(self.ctx.pass_launch(n.path, x, y, z, n.constants, bindings, n.entry))
        self.frame_number += 1
        if wait:
            self.ctx.wait()

    def download(self, handle: int, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype)
        self.ctx.check(self.ctx.lib.rt3_resource_download(self.ctx.h, handle, out.ctypes.data, out.nbytes))
        return out

    def upload(self, handle: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        self.ctx.check(self.ctx.lib.rt3_resource_upload(self.ctx.h, handle, arr.ctypes.data, arr.nbytes))

    def device_ptr(self, handle: int):
        p, n = C.c_void_p(), C.c_size_t()
        self.ctx.check(self.ctx.lib.rt3_resource_device_ptr(self.ctx.h, handle, C.byref(p), C.byref(n)))
        return p.value, n.value
