"""RT3_F_NEE_EMISSIVE without a GPU: the ABI declares it, the binding exposes it, and the two references the GPU tests
(tests/test_nee_emissive.py) measure against -- the emitter table in numpy and the point-to-parallel-rectangle form factor -- are right."""
import re
from pathlib import Path

import numpy as np

from raytracer3_amd import _lib as L
from raytracer3_amd import assets, scenes

ROOT = Path(__file__).resolve().parent.parent
CDF_TOTAL = 1 << 23


def emitter_table(mesh, instances=None):
    """numpy reference of the emitter table: (flattened prim ids, fp64 world areas, integer masses on 2^23 units).  `instances`: the
    [(first, count, 4x4 object -> world)] of Context.set_instances, None = every geometry once under the identity."""
    g = mesh.geometries
    if not instances:
        instances = [(0, len(g), np.eye(4))]
    prims, areas, lum = [], [], []
    base = 0
    for f, n, m in instances:
        m = np.asarray(m, np.float64)
        for k in range(f, f + n):
            cnt = int(mesh.prim_counts[k])
            le = 12.0 * np.asarray(g["emission"][k][:3], np.float64)
            if np.any(le != 0.0) and cnt:
                io = int(g["index_offset"][k])
                idx = mesh.indices[io:io + 3 * cnt].astype(np.int64).reshape(-1, 3) + int(g["vertex_offset"][k])
                p = mesh.vertices[idx, :3].astype(np.float64) @ m[:3, :3].T + m[:3, 3]
                a = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
                prims.append(base + np.arange(cnt))
                areas.append(a)
                lum.append(np.full(cnt, le @ [0.299, 0.587, 0.114]))
            base += cnt
    if not prims:
        return np.zeros(0, np.uint32), np.zeros(0), np.zeros(0, np.uint32)
    prim, area, lu = np.concatenate(prims), np.concatenate(areas), np.concatenate(lum)
    return prim.astype(np.uint32), area, masses(area * np.maximum(lu, 0.0))


def masses(power):
    """selection masses on the 2^-23 grid: floor of the scaled cumulative power, differenced (they sum to 2^23 exactly)"""
    c = np.cumsum(np.asarray(power, np.float64))
    if len(c) == 0 or c[-1] <= 0:
        return np.zeros(len(c), np.uint32)
    cdf = np.floor(c / c[-1] * CDF_TOTAL).astype(np.int64)
    cdf[-1] = CDF_TOTAL
    return np.diff(np.concatenate([[0], cdf])).astype(np.uint32)


def rect_form_factor(x1, x2, z1, z2, h):
    """form factor from a point with normal +y to the parallel rectangle [x1, x2] x [z1, z2] at height h above it (cosine-weighted
    fraction of the hemisphere): the corner formula, odd in both arguments, summed by inclusion / exclusion"""
    def corner(a, b):
        A, B = np.asarray(a, np.float64) / h, np.asarray(b, np.float64) / h
        sa, sb = np.sqrt(1.0 + A * A), np.sqrt(1.0 + B * B)
        return (A / sa * np.arctan(B / sa) + B / sb * np.arctan(A / sb)) / (2.0 * np.pi)
    return corner(x2, z2) - corner(x1, z2) - corner(x2, z1) + corner(x1, z1)


def test_header_declares_flag_and_functions():
    h = (ROOT / "include" / "rt3.h").read_text()
    assert re.search(r"#define RT3_F_NEE_EMISSIVE 32u", h)
    assert re.search(r"int rt3_light_info\(rt3_ctx \*ctx, uint32_t \*n_emitters, uint64_t \*cdf_total\);", h)
    assert re.search(r"int rt3_light_download\(rt3_ctx \*ctx, uint32_t \*prim, float \*area, uint32_t \*mass", h)


def test_binding_exposes_flag_and_functions():
    assert L.F_NEE_EMISSIVE == 32
    assert "rt3_light_info" in L.EXPORTS and "rt3_light_download" in L.EXPORTS
    # distinct from every other flag
    others = (L.F_NEE_SKY, L.F_BLUENOISE, L.F_SPECULAR, L.F_FACEFORWARD, L.F_PROBE_RADIANCE)
    assert all(L.F_NEE_EMISSIVE & f == 0 for f in others)


def test_emitter_table_reference_cornell():
    mesh = scenes.cornell()
    prim, area, mass = emitter_table(mesh)
    k = mesh.names.index("panel")
    first = int(np.sum(mesh.prim_counts[:k]))
    assert np.array_equal(prim, first + np.arange(int(mesh.prim_counts[k])))
    assert abs(area.sum() - 0.49) < 1e-6  # the 0.7 x 0.7 panel
    assert int(mass.sum()) == CDF_TOTAL
    # one geometry: masses proportional to area up to the one unit of quantisation
    assert np.all(np.abs(mass - area / area.sum() * CDF_TOTAL) <= 1.0 + 1e-9)


def test_emitter_table_reference_instances_and_masses():
    mesh = scenes.cornell()
    k = mesh.names.index("panel")
    m = np.eye(4)
    m[:3, :3] *= 2.0  # twice as large: four times the area and the power
    m[:3, 3] = (0.0, -2.0, 0.0)
    prim, area, mass = emitter_table(mesh, [(0, len(mesh.geometries), np.eye(4)), (k, 1, m)])
    n = int(mesh.prim_counts[k])
    assert len(prim) == 2 * n and prim[n] == mesh.n_triangles
    assert np.allclose(area[n:], 4.0 * area[:n])
    assert int(mass.sum()) == CDF_TOTAL
    assert abs(mass[n:].sum() / mass[:n].sum() - 4.0) < 1e-5
    # masses are proportional to power within one unit each
    p = np.random.default_rng(1).random(1000) ** 4
    q = masses(p)
    assert int(q.sum()) == CDF_TOTAL
    assert np.all(np.abs(q - p / p.sum() * CDF_TOTAL) <= 1.0 + 1e-9)
    assert len(emitter_table(scenes.atrium(0.2))[0]) > 0
    assert len(emitter_table(assets.Mesh(mesh.vertices, mesh.indices, mesh.geometries[:k], mesh.prim_counts[:k], mesh.names[:k], []))[0]) == 0


def test_rect_form_factor_matches_monte_carlo():
    rng = np.random.default_rng(7)
    n = 2_000_000
    # cosine-weighted directions about +y: the fraction that crosses the rectangle is the form factor
    u0, u1 = rng.random(n), rng.random(n)
    r, phi = np.sqrt(u1), 2 * np.pi * u0
    dx, dy, dz = r * np.cos(phi), np.sqrt(1.0 - u1), r * np.sin(phi)
    for (x1, x2, z1, z2, h) in ((-0.5, 0.5, -0.5, 0.5, 1.0), (0.2, 1.3, -0.4, 0.9, 0.7), (-2.0, -1.0, 0.5, 3.0, 1.5)):
        t = h / dy
        x, z = dx * t, dz * t
        mc = np.mean((x >= x1) & (x <= x2) & (z >= z1) & (z <= z2))
        f = rect_form_factor(x1, x2, z1, z2, h)
        assert abs(mc - f) < 5 * np.sqrt(f * (1 - f) / n) + 1e-4, (mc, f)
    # the whole plane is the whole hemisphere
    assert abs(rect_form_factor(-1e7, 1e7, -1e7, 1e7, 1.0) - 1.0) < 1e-6
