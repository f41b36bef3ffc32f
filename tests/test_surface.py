"""The surface stage ON the GPU (rt3_selftest_eval op 29, hit_info): every row is first asserted bit for bit equal to the oracle's
orc_hit_info, then held to the float64 reference within the derived bounds by the checks of test_surface_cpu.py -- on the same world and
the same hits, in both instance modes (one batched launch per mode).  And the cases the host must refuse without launching."""
import numpy as np
import pytest

import surface_worlds as SW
import test_surface_cpu as S
from raytracer3_amd import _lib as L
from raytracer3_amd.render_graph import Context

pytestmark = pytest.mark.gpu

world = S.world  # the module-scoped fixture: the same world, hits and float64 reference


def context(mesh, instances, mode):
    ctx = Context(0)
    ctx.set_option(L.OPT_INSTANCE_MODE, mode)
    ctx.upload_mesh(mesh)
    ctx.set_instances(instances)
    ctx.build_accel()
    return ctx


class Device:
    """S.Oracle's interface on op 29; the one launch is compared with the oracle bit for bit before anything else sees it"""

    def __init__(self, mesh, instances, hits, mode):
        self.name = f"gpu, instance mode {mode}"
        ctx = context(mesh, instances, mode)
        try:
            self.words = ctx.selftest(L.SELFTEST_HIT_INFO, SW.hit_rows(*hits), 11)
        finally:
            ctx.close()
        want = S.Oracle(mesh, instances).hit_info(*hits).view(np.uint32)
        bad = np.flatnonzero((self.words != want).any(1))
        assert bad.size == 0, (mode, bad[:4], hits[0][bad[:4]], self.words[bad[:4]], want[bad[:4]])
        self.hits = hits

    def hit_info(self, prim, bu, bv):
        assert prim is self.hits[0]
        return self.words.view(np.float32)


@pytest.fixture(scope="module")
def devices(world):
    mesh, instances, hits, _ = world
    return [Device(mesh, instances, hits, mode) for mode in (0, 1)]


def test_hit_info_equals_the_oracle_in_both_instance_modes(devices):
    assert np.array_equal(devices[0].words, devices[1].words)


def test_hit_info_matches_float64(devices, world):
    S.check_world_reaches_the_edges(world)
    for dev in devices:
        n = S.check_normals(dev, world)
        a, by_size = S.check_albedo(dev, world)
        S.check_material(dev, world)
        print(f"hit_info ({dev.name}): normals worst error / bound {n:.3f}, albedo worst error / bound {a:.3f}, by texture size {by_size}")


def test_hit_info_refuses_what_it_cannot_index(world):
    mesh, instances, hits, _ = world
    rows = SW.hit_rows(*hits)[:64].copy()
    out = np.full((64, 11), 0xDEADBEEF, np.uint32)

    def call(ctx, r):
        return ctx.lib.rt3_selftest_eval(ctx.h, L.SELFTEST_HIT_INFO, r.ctypes.data, len(r), out.ctypes.data)

    ctx = Context(0)
    try:
        assert call(ctx, rows) == L.E_STATE  # nothing uploaded, nothing built
        ctx.upload_mesh(mesh)
        ctx.set_instances(instances)
        assert call(ctx, rows) == L.E_STATE  # a scene without an acceleration structure
        ctx.build_accel()
        n_prims = int(sum(mesh.prim_counts[f:f + c].sum() for f, c, _ in instances))
        assert call(ctx, rows) == L.RT3_OK and (out != 0xDEADBEEF).all()
        out[:] = 0xDEADBEEF
        bad = rows.copy()
        bad[37, 0] = n_prims  # one past the last flattened primitive, in the middle of the batch
        assert call(ctx, bad) == L.E_INVALID and (out == 0xDEADBEEF).all()
        bad[37, 0] = 0xFFFFFFFF
        assert call(ctx, bad) == L.E_INVALID and (out == 0xDEADBEEF).all()
        bad[37, 0] = n_prims - 1
        assert call(ctx, bad) == L.RT3_OK
        out[:] = 0xDEADBEEF
        ctx.update_vertices(mesh.vertices[:3])  # the structure is stale until a refit or a rebuild
        assert call(ctx, rows) == L.E_STATE and (out == 0xDEADBEEF).all()
        assert "vertices were updated" in ctx.last_error()
        ctx.refit_accel()
        assert call(ctx, rows) == L.RT3_OK
    finally:
        ctx.close()
