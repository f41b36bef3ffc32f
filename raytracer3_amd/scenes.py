"""Deterministic procedural stand-ins for the assets the reference tree does not ship
(/root/reference/.MISSING_LARGE_BLOBS: resources/sponza_scene.glb, resources/skybox2.exr) -- SURVEY.md section 8d.

* `atrium(detail)`  Sponza stand-in: two-storey colonnade around an open-roofed court, floor tiles, draped curtains,
                    emissive ceiling panels.  detail=1.0 -> 262 144 +- 2 % triangles, AABB 29.8 x 12.4 x 18.3 m.
* `cornell()`       closed Cornell box with an emissive ceiling panel (reference semantics need no sky).
* `cornell_ref()`   the box of the ONE image the reference tree holds (resources/refrence.png, a Blender-Cycles render): the eight
                    unit cubes and eight materials of the reference's processed asset `imported_assets/Default/box.glb`, placed
                    (the asset lost its node transforms and its emission) so that a render from CORNELL_REF_CAMERA lines up with
                    that image.  Informational: Cycles is not this estimator and the display transforms differ.
* `glass_cornell()` the Cornell box with a solid glass sphere and a thin-walled tinted pane.
* `amber_cornell()` the Cornell box with absorbing glass: an amber block and two green spheres of two sizes.
* `skinned_arm()`   the open Cornell room with a three-joint skinned tube, one morph target and a bend animation.
* `sky(w, h)`       equirect RGB32F gradient sky + 0.5 degree sun disc (peak radiance 5e4).
All surfaces carry normals facing the side they are meant to be seen from.
"""
from __future__ import annotations

import numpy as np

from .assets import Material, Mesh, MeshBuilder

ATRIUM_SEED = 0x5F0A2A
SKY_SEED = 7
ATRIUM_CAMERA = dict(position=(-10.0, 2.0, 0.0), direction=(1.0, 0.1, 0.0), fov_deg=65.0)
# slightly off-axis: an exactly symmetric view sends rays through the shared diagonals of the wall quads, where the fp32
# Moeller-Trumbore test is not watertight (known limitations)
CORNELL_CAMERA = dict(position=(0.0137, 1.0071, 3.4), direction=(0.0041, -0.0033, -1.0), fov_deg=40.0)


# Fitted to /root/reference/resources/refrence.png (1920x1080): least squares over the eight interior corners of the box as they
# appear in the image (box interior = the asset's unit cube [-1, 1]^3, open towards +z), no camera roll: 7 px RMS.
CORNELL_REF_CAMERA = dict(position=(-0.18653, 0.33087, 7.38676), direction=(0.018591, -0.058248, -0.998129), fov_deg=22.8837)
CORNELL_REF_EMISSION = 0.48  # GeometryInfo.emission of the light cube (x 12 in hit_info); chosen by tests/experiments/fit_cornell_ref.py


def _grid(origin, du, dv, nu, nv, normal=None, disp=None):
    """(nu x nv) quad grid spanning origin + s*du + t*dv, s,t in [0,1]; CCW seen from cross(du,dv)."""
    o, du, dv = (np.asarray(a, np.float64) for a in (origin, du, dv))
    s, t = np.meshgrid(np.linspace(0, 1, nu + 1), np.linspace(0, 1, nv + 1), indexing="xy")
    pos = o + s[..., None] * du + t[..., None] * dv
    n = np.cross(du, dv) if normal is None else np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    nrm = np.broadcast_to(n, pos.shape).copy()
    if disp is not None:
        pos, nrm = disp(pos, nrm, s, t)
    uv = np.stack([s, t], -1)
    i = np.arange(nu)[None, :] + (nu + 1) * np.arange(nv)[:, None]
    a, b, c, d = i, i + 1, i + nu + 2, i + nu + 1
    tris = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], -2).reshape(-1, 3)
    return pos.reshape(-1, 3), nrm.reshape(-1, 3), uv.reshape(-1, 2), tris


def _box(mb, name, lo, hi, mat, n=1, inward=False):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    e = hi - lo
    faces = [  # origin, du, dv with cross(du,dv) pointing outward
        (lo + [0, 0, e[2]], [e[0], 0, 0], [0, e[1], 0]),  # +z
        (lo + [e[0], 0, 0], [-e[0], 0, 0], [0, e[1], 0]),  # -z
        (lo + [e[0], 0, e[2]], [0, 0, -e[2]], [0, e[1], 0]),  # +x
        (lo, [0, 0, e[2]], [0, e[1], 0]),  # -x
        (lo + [0, e[1], e[2]], [e[0], 0, 0], [0, 0, -e[2]]),  # +y
        (lo, [e[0], 0, 0], [0, 0, e[2]]),  # -y
    ]
    P, N, U, T, off = [], [], [], [], 0
    for o, du, dv in faces:
        if inward:
            du, dv = dv, du
        p, nn, uv, t = _grid(o, du, dv, n, n)
        P.append(p); N.append(nn); U.append(uv); T.append(t + off); off += len(p)
    mb.add(name, np.concatenate(P), np.concatenate(N), np.concatenate(U), np.concatenate(T), mat)


def _cylinder(mb, name, base, radius, height, nseg, nring, mat, flute=0.0):
    th = np.linspace(0, 2 * np.pi, nseg + 1)
    y = np.linspace(0, 1, nring + 1)
    T, Y = np.meshgrid(th, y, indexing="xy")
    r = radius * (1.0 + flute * np.cos(12 * T)) * (1.0 - 0.12 * Y + 0.10 * np.exp(-((Y - 0.02) / 0.04) ** 2) + 0.10 * np.exp(-((Y - 0.98) / 0.04) ** 2))
    pos = np.stack([base[0] + r * np.cos(T), base[1] + Y * height, base[2] + r * np.sin(T)], -1)
    nrm = np.stack([np.cos(T), np.zeros_like(T), np.sin(T)], -1)
    uv = np.stack([T / (2 * np.pi), Y], -1)
    i = np.arange(nseg)[None, :] + (nseg + 1) * np.arange(nring)[:, None]
    a, b, c, d = i, i + 1, i + nseg + 2, i + nseg + 1
    tris = np.stack([np.stack([a, c, b], -1), np.stack([a, d, c], -1)], -2).reshape(-1, 3)  # outward
    mb.add(name, pos.reshape(-1, 3), nrm.reshape(-1, 3), uv.reshape(-1, 2), tris, mat)


def _arch(mb, name, p0, p1, rise, tube, nseg, nring, mat):
    """Half-ellipse tube from p0 to p1 (same height), bulging up by `rise`."""
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    mid, half = 0.5 * (p0 + p1), 0.5 * (p1 - p0)
    L = np.linalg.norm(half)
    ax = half / L
    a = np.linspace(np.pi, 0, nseg + 1)
    centre = mid + np.cos(a)[:, None] * half + np.sin(a)[:, None] * np.array([0, rise, 0])
    tang = -np.sin(a)[:, None] * half + np.cos(a)[:, None] * np.array([0, rise, 0])
    tang /= np.linalg.norm(tang, axis=1, keepdims=True)
    side = np.cross(ax, [0, 1, 0]); side /= np.linalg.norm(side)
    up = np.cross(side[None, :], tang)
    ph = np.linspace(0, 2 * np.pi, nring + 1)
    nrm = np.cos(ph)[None, :, None] * up[:, None, :] + np.sin(ph)[None, :, None] * side[None, None, :]
    pos = centre[:, None, :] + tube * nrm
    uv = np.stack(np.meshgrid(ph / (2 * np.pi), np.linspace(0, 1, nseg + 1), indexing="xy"), -1)
    i = np.arange(nring)[None, :] + (nring + 1) * np.arange(nseg)[:, None]
    a_, b_, c_, d_ = i, i + 1, i + nring + 2, i + nring + 1
    tris = np.stack([np.stack([a_, b_, c_], -1), np.stack([a_, c_, d_], -1)], -2).reshape(-1, 3)
    # orientation check: make the geometric normal agree with the shading normal
    P, N = pos.reshape(-1, 3), nrm.reshape(-1, 3)
    fn = np.cross(P[tris[:, 1]] - P[tris[:, 0]], P[tris[:, 2]] - P[tris[:, 0]])
    if np.sum(np.einsum("ij,ij->i", fn, N[tris[:, 0]])) < 0:
        tris = tris[:, ::-1]
    mb.add(name, P, N, uv.reshape(-1, 2), tris, mat)


def _sphere(mb, name, centre, radius, nseg, nring, mat):
    th = np.linspace(0, 2 * np.pi, nseg + 1)
    ph = np.linspace(0, np.pi, nring + 1)
    T, Pp = np.meshgrid(th, ph, indexing="xy")
    nrm = np.stack([np.sin(Pp) * np.cos(T), np.cos(Pp), np.sin(Pp) * np.sin(T)], -1)
    pos = np.asarray(centre, np.float64) + radius * nrm
    uv = np.stack([T / (2 * np.pi), Pp / np.pi], -1)
    i = np.arange(nseg)[None, :] + (nseg + 1) * np.arange(nring)[:, None]
    a, b, c, d = i, i + 1, i + nseg + 2, i + nseg + 1
    tris = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], -2).reshape(-1, 3)
    P, N = pos.reshape(-1, 3), nrm.reshape(-1, 3)
    fn = np.cross(P[tris[:, 1]] - P[tris[:, 0]], P[tris[:, 2]] - P[tris[:, 0]])
    area = np.linalg.norm(fn, axis=1)
    tris = tris[area > 1e-12]  # drop the degenerate pole triangles
    fn = fn[area > 1e-12]
    if np.sum(np.einsum("ij,ij->i", fn, N[tris[:, 0]])) < 0:
        tris = tris[:, ::-1]
    mb.add(name, P, N, uv.reshape(-1, 2), tris, mat)


def atrium(detail: float = 1.0, seed: int = ATRIUM_SEED) -> Mesh:
    """Sponza stand-in.  `detail` scales the tessellation (1.0 = full ~262k triangles; 0.1 ~ a few thousand)."""
    rng = np.random.default_rng(seed)
    alb = rng.uniform(0.2, 0.8, size=(24, 3))
    mats = []
    for k in range(24):
        rough = 0.5 if k % 5 == 0 else 1.0
        metal = 1.0 if k in (7, 19) else 0.0
        mats.append(Material(tuple(float(x) for x in alb[k]), metal, rough))
    emissive = Material((0.8, 0.8, 0.8), 0.0, 1.0, emission=(1.0, 0.95, 0.85))
    mb = MeshBuilder()
    X, Y, Z = 14.9, 12.4, 9.15  # half extents in x,z ; full height
    q = lambda n: max(1, int(round(n * detail)))  # noqa: E731

    # floor: 60 x 36 tiles in two alternating materials (normals up)
    nx, nz = q(60), q(36)
    for par in (0, 1):
        P, N, U, T, off = [], [], [], [], 0
        for ix in range(nx):
            for iz in range(nz):
                if (ix + iz) % 2 != par:
                    continue
                o = [-X + 2 * X * ix / nx, 0.0, -Z + 2 * Z * iz / nz]
                p, n, uv, t = _grid(o, [0, 0, 2 * Z / nz], [2 * X / nx, 0, 0], 1, 1)
                P.append(p); N.append(n); U.append(uv); T.append(t + off); off += 4
        if P:
            mb.add(f"floor{par}", np.concatenate(P), np.concatenate(N), np.concatenate(U), np.concatenate(T), mats[par])
    # outer walls (normals inward)
    wq = (q(40), q(16))
    p = _grid([-X, 0, -Z], [2 * X, 0, 0], [0, Y, 0], *wq); mb.add("wall_z-", *p, mats[2])
    p = _grid([X, 0, Z], [-2 * X, 0, 0], [0, Y, 0], *wq); mb.add("wall_z+", *p, mats[3])
    p = _grid([-X, 0, Z], [0, 0, -2 * Z], [0, Y, 0], *wq); mb.add("wall_x-", *p, mats[4])
    p = _grid([X, 0, -Z], [0, 0, 2 * Z], [0, Y, 0], *wq); mb.add("wall_x+", *p, mats[5])
    # ceiling ring around an open skylight x in [-8,8], z in [-4,4] (normals down)
    hx, hz = 8.0, 4.0
    cq = (q(24), q(8))
    p = _grid([-X, Y, -Z], [0, 0, Z - hz], [2 * X, 0, 0], *cq[::-1]); mb.add("ceil_z-", *p, mats[6])
    p = _grid([-X, Y, hz], [0, 0, Z - hz], [2 * X, 0, 0], *cq[::-1]); mb.add("ceil_z+", *p, mats[6])
    p = _grid([-X, Y, -hz], [0, 0, 2 * hz], [X - hx, 0, 0], *cq[::-1]); mb.add("ceil_x-", *p, mats[6])
    p = _grid([hx, Y, -hz], [0, 0, 2 * hz], [X - hx, 0, 0], *cq[::-1]); mb.add("ceil_x+", *p, mats[6])
    # gallery (upper floor ring at y = 6 around the court x in [-9.6,9.6], z in [-5.6,5.6]): slabs with thickness
    gx, gz, gy = 9.6, 5.6, 6.0
    _box(mb, "gallery_z-", [-X, gy - 0.3, -Z], [X, gy, -gz], mats[8], n=q(6))
    _box(mb, "gallery_z+", [-X, gy - 0.3, gz], [X, gy, Z], mats[8], n=q(6))
    _box(mb, "gallery_x-", [-X, gy - 0.3, -gz], [-gx, gy, gz], mats[9], n=q(6))
    _box(mb, "gallery_x+", [gx, gy - 0.3, -gz], [X, gy, gz], mats[9], n=q(6))
    # colonnade: columns on the court rectangle, both storeys, arches between neighbours
    cx, cz = 9.0, 5.0
    xs = np.linspace(-cx, cx, 7)
    zs = np.linspace(-cz, cz, 4)
    ring = [(x, -cz) for x in xs] + [(cx, z) for z in zs[1:]] + [(x, cz) for x in xs[::-1][1:]] + [(-cx, z) for z in zs[::-1][1:-1]]
    seg, rings = q(32), q(20)
    for storey, (y0, hgt) in enumerate(((0.0, 5.0), (gy, 5.2))):
        for k, (x, z) in enumerate(ring):
            _cylinder(mb, f"col{storey}_{k}", (x, y0, z), 0.33 if storey == 0 else 0.26, hgt, seg, rings, mats[10 + (k % 3)], flute=0.03)
        for k in range(len(ring)):
            (xa, za), (xb, zb) = ring[k], ring[(k + 1) % len(ring)]
            _arch(mb, f"arch{storey}_{k}", (xa, y0 + hgt, za), (xb, y0 + hgt, zb), 0.7, 0.16, q(28), q(12), mats[13 + storey])
    # curtains: 16 sin-displaced sheets hanging between upper columns (double sided look via two-sided shading)
    ncur = 16
    # remaining triangle budget goes to the curtains so that detail=1 lands on 262 144 +- 2 %
    so_far = sum(mb.c)
    extras = 8 * 2 * q(48) * q(24) + 4 * 8 + 12 * 6 * 2  # spheres + panels + plinths (estimate)
    target = int(262144 * detail * detail) if detail < 1.0 else 262144
    per = max(8, (target - so_far - extras) // ncur)
    cn = max(2, int(np.sqrt(per / 2.0)))
    cu, cv = cn, max(2, per // (2 * cn))
    for k in range(ncur):
        (xa, za), (xb, zb) = ring[(2 * k) % len(ring)], ring[(2 * k + 1) % len(ring)]
        ph = float(rng.uniform(0, 2 * np.pi))
        amp = float(rng.uniform(0.10, 0.22))

        def disp(pos, nrm, s, t, ph=ph, amp=amp):
            n0 = nrm[0, 0]
            w = amp * np.sin(6 * np.pi * s + ph) * (0.35 + 0.65 * t) + 0.05 * np.sin(2 * np.pi * t * 3 + ph)
            dws = amp * 6 * np.pi * np.cos(6 * np.pi * s + ph) * (0.35 + 0.65 * t)
            pos = pos + w[..., None] * n0
            du = pos[0, -1] - pos[0, 0]
            du = du / np.linalg.norm(du)
            length = np.linalg.norm(pos[0, -1] - pos[0, 0])
            nn = n0[None, None, :] - (dws / length)[..., None] * du[None, None, :]
            return pos, nn

        o = np.array([xa, gy + 4.6, za]); du = np.array([xb - xa, 0, zb - za]); dv = np.array([0, -3.6, 0])
        # face the court centre
        n = np.cross(du, dv)
        if np.dot(n, -o * [1, 0, 1]) < 0:
            o, du = o + du, -du
        p = _grid(o + np.cross(du, dv) / np.linalg.norm(np.cross(du, dv)) * 0.45, du, dv, cu, cv, disp=disp)
        mb.add(f"curtain{k}", *p, mats[15 + (k % 6)])
    # decorative spheres on plinths in the court
    for k in range(8):
        x = -7.0 + 2.0 * k; z = 2.5 if k % 2 else -2.5
        _box(mb, f"plinth{k}", [x - 0.35, 0.0, z - 0.35], [x + 0.35, 0.8, z + 0.35], mats[21], n=1)
        _sphere(mb, f"sphere{k}", (x, 1.25, z), 0.45, q(48), q(24), mats[7] if k % 4 == 0 else (mats[19] if k % 4 == 2 else mats[22]))
    # 4 emissive ceiling panels under the ceiling ring (emission 1.0 -> x12 in hit_info)
    for k, (x, z) in enumerate(((-11.5, -6.5), (11.5, -6.5), (-11.5, 6.5), (11.5, 6.5))):
        p = _grid([x - 1.2, Y - 0.05, z - 0.8], [0, 0, 1.6], [2.4, 0, 0], 2, 2)
        mb.add(f"panel{k}", *p, emissive)
    return mb.build()


def cornell() -> Mesh:
    """Closed Cornell box, 2 x 2 x 2 m centred at (0,1,0): red/green side walls, two blocks, emissive ceiling panel."""
    white = Material((0.73, 0.73, 0.73)); red = Material((0.65, 0.05, 0.05)); green = Material((0.12, 0.45, 0.15))
    light = Material((0.78, 0.78, 0.78), emission=(1.4, 1.2, 0.9))
    mb = MeshBuilder()
    n = 4
    mb.add("floor", *_grid([-1, 0, -1], [0, 0, 2], [2, 0, 0], n, n), white)
    mb.add("ceiling", *_grid([-1, 2, -1], [2, 0, 0], [0, 0, 2], n, n), white)
    mb.add("back", *_grid([-1, 0, -1], [2, 0, 0], [0, 2, 0], n, n), white)
    mb.add("front", *_grid([1, 0, 4], [-2, 0, 0], [0, 2, 0], n, n), white)  # behind the camera: closes the box
    mb.add("floor2", *_grid([-1, 0, 1], [0, 0, 3], [2, 0, 0], n, n), white)
    mb.add("ceiling2", *_grid([-1, 2, 1], [2, 0, 0], [0, 0, 3], n, n), white)
    mb.add("left", *_grid([-1, 0, 4], [0, 0, -5], [0, 2, 0], n, n), red)
    mb.add("right", *_grid([1, 0, -1], [0, 0, 5], [0, 2, 0], n, n), green)
    mb.add("panel", *_grid([-0.35, 1.995, -0.35], [0.7, 0, 0], [0, 0, 0.7], 2, 2), light)
    _box(mb, "tall", [-0.65, 0.0, -0.65], [-0.05, 1.2, -0.05], white, n=2)
    _box(mb, "short", [0.1, 0.0, 0.0], [0.7, 0.6, 0.6], white, n=2)
    return mb.build()


def cornell_ref(asset_path=None, emission: float = CORNELL_REF_EMISSION) -> Mesh:
    """The Cornell box of resources/refrence.png rebuilt from the reference's own processed asset.

    `imported_assets/Default/box.glb` (bincode, older `Mesh` layout; tests/golden/processed_box.glb.bin is a byte-identical copy
    so that this also works where /root/reference is absent) holds 8 unit cubes (24 vertices each: position, face normal, uv)
    and 8 materials -- 0.8 grey x3, blue, red, green, 0.5 grey, 0.8 grey with roughness 0.5 -- but neither node transforms nor
    emission.  Cube k takes material k; which cube is which wall is decided by its colour, the placements below
    are read off the image: open front, black outside, a flat emissive box just under the ceiling (its side faces are what
    lights the ceiling in the image: the render is direct light only -- the unlit front of the small box is pure black)."""
    from pathlib import Path

    from .assets import read_processed_mesh

    path = Path(asset_path) if asset_path else Path(__file__).resolve().parent.parent / "tests" / "golden" / "processed_box.glb.bin"
    pm = read_processed_mesh(path, "old")
    if len(pm.materials) != 8 or len(pm.vertices) != 8 * 24:
        raise ValueError("expected the reference's box asset: 8 cubes x 24 vertices, 8 materials")

    def role(m):
        r, g, b = m.color
        if b > 0.5 and r < 0.1:
            return "right"
        if r > 0.5 and g < 0.1:
            return "left"
        if g > 0.5 and r < 0.1:
            return "floor"
        if abs(r - 0.5) < 0.01:
            return "short"
        return "light" if m.roughness_factor < 0.9 else "grey"

    t = 0.05  # wall thickness (never seen: the outside is black)
    place = {  # role -> (half size, centre, rotation about +y in degrees)
        "floor": ((1 + 2 * t, t, 1.0), (0.0, -1 - t, 0.0), 0.0),
        "ceiling": ((1 + 2 * t, t, 1.0), (0.0, 1 + t, 0.0), 0.0),
        "back": ((1 + 2 * t, 1 + 2 * t, t), (0.0, 0.0, -1 - t), 0.0),
        "left": ((t, 1.0, 1.0), (-1 - t, 0.0, 0.0), 0.0),
        "right": ((t, 1.0, 1.0), (1 + t, 0.0, 0.0), 0.0),
        "tall": ((0.247, 0.455, 0.25), (-0.535, -0.545, -0.37), -10.0),
        "short": ((0.215, 0.19, 0.22), (0.28, -0.81, 0.27), 0.0),
        "light": ((0.455, 0.02, 0.625), (-0.015, 0.975, -0.025), 0.0),
    }
    greys = iter(("back", "ceiling", "tall"))
    mb = MeshBuilder()
    for k, m in enumerate(pm.materials):
        r = role(m)
        name = next(greys) if r == "grey" else r
        half, centre, rot = place[name]
        v = pm.vertices[24 * k : 24 * k + 24].astype(np.float64)
        c, sn = np.cos(np.radians(rot)), np.sin(np.radians(rot))
        R = np.array([[c, 0.0, sn], [0.0, 1.0, 0.0], [-sn, 0.0, c]])
        pos = (v[:, :3] * np.asarray(half)) @ R.T + np.asarray(centre)
        nrm = v[:, 3:6] @ R.T  # axis-aligned face normals: unchanged by the axis-aligned scale
        tris = []
        for f in np.unique(np.round(v[:, 3:6]), axis=0):  # the four vertices of each face, fanned counter-clockwise about the outward normal
            idx = np.nonzero((np.round(v[:, 3:6]) == f).all(1))[0]
            assert len(idx) == 4
            ctr = v[idx, :3].mean(0)
            a = np.cross(f, [1.0, 0.0, 0.0]) if abs(f[0]) < 0.5 else np.cross(f, [0.0, 1.0, 0.0])
            bq = np.cross(f, a)
            ang = np.arctan2((v[idx, :3] - ctr) @ bq, (v[idx, :3] - ctr) @ a)
            q = idx[np.argsort(ang)]
            tris += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
        mat = Material(m.color, m.metalic_factor, m.roughness_factor, (emission,) * 3 if name == "light" else (0.0, 0.0, 0.0))
        mb.add(name, pos, nrm, v[:, 6:8], np.asarray(tris), mat)
    return mb.build()


def textured_cornell() -> Mesh:
    """The Cornell box with base-colour textures (hit_logic.slang:31-33): checker floor, gradient back wall."""
    mesh = cornell()
    yy, xx = np.mgrid[0:64, 0:64]
    checker = np.where(((xx // 8) + (yy // 8)) % 2 == 0, 230, 40).astype(np.uint8)
    t0 = np.stack([checker, checker, (checker // 2 + 60).astype(np.uint8), np.full_like(checker, 255)], -1)
    yy, xx = np.mgrid[0:32, 0:48]
    t1 = np.stack([(xx * 5).astype(np.uint8), (yy * 7).astype(np.uint8), np.full(xx.shape, 128, np.uint8), np.full(xx.shape, 255, np.uint8)], -1)
    mesh.textures = [np.ascontiguousarray(t0), np.ascontiguousarray(t1)]
    for name, tex in (("floor", 0), ("floor2", 0), ("back", 1)):
        g = mesh.names.index(name)
        mesh.geometries["base_color_texture_index"][g] = tex
        mesh.geometries["base_color"][g] = (1.0, 1.0, 1.0, 1.0)
        vo = int(mesh.geometries["vertex_offset"][g])
        later = [int(x) for x in mesh.geometries["vertex_offset"] if int(x) > vo]
        mesh.vertices[vo : (min(later) if later else len(mesh.vertices)), 6:8] *= 3.0  # repeat addressing: uv up to 3
    return mesh


def lit_room() -> Mesh:
    """The Cornell box with its panel switched off and three punctual lights instead (KHR_lights_punctual): a warm
    point lamp between the blocks, a spot from the ceiling onto the tall block, a dim cool sun slanting in from the open side.  Render it
    with F_NEE_PUNCTUAL in the flags; without the flag it is black."""
    from .assets import LIGHT_DIRECTIONAL, LIGHT_POINT, LIGHT_SPOT, lights_array, make_light

    mesh = cornell()
    mesh.geometries["emission"][mesh.names.index("panel")] = 0.0
    mesh.lights = lights_array([
        make_light(LIGHT_POINT, (2.4, 1.8, 1.1), position=(0.15, 0.45, 0.35), range=6.0),
        make_light(LIGHT_SPOT, (9.0, 9.0, 8.0), position=(-0.3, 1.9, 0.1), direction=(-0.1, -1.0, -0.25), inner_cone=0.25, outer_cone=0.55),
        make_light(LIGHT_DIRECTIONAL, (0.25, 0.3, 0.4), direction=(0.2, -0.5, -1.0)),
    ])
    return mesh


def cutout_cornell() -> Mesh:
    """The Cornell box with alpha-masked cutout geometry (glTF alphaMode MASK): a tilted lattice panel (hard 0 / 255
    alpha, cutoff 0.5) and overlapping leaf quads at different depths whose alpha is a smooth gradient (cutoffs 0.3, 0.5, 0.7, uv repeated),
    one more quad masked by base_color[3] alone (no texture).  Opaque emitter and walls."""
    mesh = cornell()
    yy, xx = np.mgrid[0:64, 0:64]
    bars = ((xx % 16) < 5) | ((yy % 16) < 5)  # lattice: bars opaque, cells cut away
    lattice = np.stack([np.full(xx.shape, 150, np.uint8), np.full(xx.shape, 110, np.uint8), np.full(xx.shape, 60, np.uint8),
                        np.where(bars, 255, 0).astype(np.uint8)], -1)
    r = np.hypot((xx + 0.5) / 64.0 - 0.5, (yy + 0.5) / 64.0 - 0.5) * 2.0  # leaf: alpha falls off from the centre, a hard notch on one side
    a = np.clip(255.0 * (1.0 - r), 0.0, 255.0)
    a = np.where((xx > 44) & (np.abs(yy - 32) < 4), 0.0, a)
    leaf = np.stack([(60 + xx).astype(np.uint8), (140 + yy).astype(np.uint8), np.full(xx.shape, 50, np.uint8), np.round(a).astype(np.uint8)], -1)
    mb = MeshBuilder()
    mb.add("lattice", *_grid([-0.8, 0.2, -0.2], [1.3, 0.0, 0.5], [0.2, 1.4, -0.3], 3, 3), Material((1.0, 1.0, 1.0), texture_offset=0, alpha_cutoff=0.5))
    for k, (z, cut) in enumerate(((0.4, 0.3), (0.7, 0.5), (1.0, 0.7))):
        p, n, uv, t = _grid([-0.5 + 0.25 * k, 0.3 + 0.2 * k, z], [0.8, 0.0, 0.1], [0.0, 0.8, 0.05], 2, 2)
        mb.add(f"leaf{k}", p, n, uv * (1.0 + k), t, Material((1.0, 1.0, 1.0), texture_offset=1, alpha_cutoff=cut))
    mb.add("veil", *_grid([0.2, 0.9, 0.3], [0.6, 0.0, 0.0], [0.0, 0.6, 0.2], 1, 1), Material((0.9, 0.6, 0.6), alpha_cutoff=0.5, alpha=0.6))
    cut = mb.build()
    n_geo, n_idx, n_vtx = len(mesh.geometries), len(mesh.indices), len(mesh.vertices)
    g = cut.geometries.copy()
    g["index_offset"] += n_idx
    g["vertex_offset"] += n_vtx
    return Mesh(np.ascontiguousarray(np.concatenate([mesh.vertices, cut.vertices]), np.float32),
                np.ascontiguousarray(np.concatenate([mesh.indices, cut.indices]), np.uint32), np.concatenate([mesh.geometries, g]),
                np.concatenate([mesh.prim_counts, cut.prim_counts]).astype(np.uint32), mesh.names + cut.names,
                [np.ascontiguousarray(lattice), np.ascontiguousarray(leaf)],
                np.concatenate([mesh.alpha_cutoffs, cut.alpha_cutoffs]).astype(np.float32))


def glass_cornell() -> Mesh:
    """The Cornell box with glass: a solid glass sphere (ior 1.5, a UV sphere with smooth normals) resting on the
    short block and a thin-walled, green-tinted pane standing in front of the tall one.  Render it with a lens (PathTracer.set_scene
    switches the per-sample pinhole on)."""
    mesh = cornell()
    mb = MeshBuilder()
    _sphere(mb, "glass_sphere", [0.4, 0.9, 0.3], 0.3, 48, 24, Material((1.0, 1.0, 1.0), 0.0, 0.0, transmission=1.0, ior=1.5, thin_walled=0))
    mb.add("glass_pane", *_grid([-0.9, 0.0, 0.45], [0.75, 0.0, 0.3], [0.0, 1.4, 0.0], 1, 1),
           Material((0.7, 0.95, 0.8), 0.0, 0.0, transmission=1.0, ior=1.5, thin_walled=1))
    add = mb.build()
    g = add.geometries.copy()
    g["index_offset"] += len(mesh.indices)
    g["vertex_offset"] += len(mesh.vertices)
    return Mesh(np.ascontiguousarray(np.concatenate([mesh.vertices, add.vertices]), np.float32),
                np.ascontiguousarray(np.concatenate([mesh.indices, add.indices]), np.uint32), np.concatenate([mesh.geometries, g]),
                np.concatenate([mesh.prim_counts, add.prim_counts]).astype(np.uint32), mesh.names + add.names,
                transmission=np.concatenate([mesh.transmission, add.transmission]))


def frosted_cornell() -> Mesh:
    """glass_cornell() with roughness on its glass: the sphere at 0.3, the pane at 0.15.  Under
    PathTracer.set_rough_transmission(True) the sphere is matte-translucent and the room behind the pane is blurred; without the mode it is
    glass_cornell()'s picture."""
    mesh = glass_cornell()
    mesh.geometries["roughness"][mesh.names.index("glass_sphere")] = 0.3
    mesh.geometries["roughness"][mesh.names.index("glass_pane")] = 0.15
    return mesh


def _append(mesh: Mesh, add: Mesh) -> Mesh:
    """`mesh` followed by the geometries of `add`, with the glass and absorption tables of both"""
    g = add.geometries.copy()
    g["index_offset"] += len(mesh.indices)
    g["vertex_offset"] += len(mesh.vertices)
    return Mesh(np.ascontiguousarray(np.concatenate([mesh.vertices, add.vertices]), np.float32),
                np.ascontiguousarray(np.concatenate([mesh.indices, add.indices]), np.uint32), np.concatenate([mesh.geometries, g]),
                np.concatenate([mesh.prim_counts, add.prim_counts]).astype(np.uint32), mesh.names + add.names,
                transmission=np.concatenate([mesh.transmission, add.transmission]),
                attenuation=np.concatenate([mesh.attenuation, add.attenuation]),
                attenuation_source=np.concatenate([mesh.attenuation_source if mesh.attenuation_source is not None
                                                   else np.tile([1.0, 1.0, 1.0, np.inf], (len(mesh.geometries), 1)), add.attenuation_source]))


def amber_cornell(absorb=True) -> Mesh:
    """The glass Cornell box with absorbing glass: an amber block of solid glass leaning against the short block, and two
    green spheres of the same glass, one of twice the other's radius -- the large one is the darker and the more saturated.  `absorb` False:
    the same geometry with every attenuation at its default, which launches nothing new."""
    inf = float("inf")
    amber = dict(attenuation_color=(0.95, 0.55, 0.12), attenuation_distance=0.25 if absorb else inf)
    green = dict(attenuation_color=(0.35, 0.9, 0.45), attenuation_distance=0.3 if absorb else inf)
    mb = MeshBuilder()
    _sphere(mb, "green_sphere_large", [0.4, 0.9, 0.3], 0.3, 48, 24, Material((1.0, 1.0, 1.0), 0.0, 0.0, transmission=1.0, ior=1.5, thin_walled=0, **green))
    _sphere(mb, "green_sphere_small", [0.0, 0.152, 0.85], 0.15, 32, 16, Material((1.0, 1.0, 1.0), 0.0, 0.0, transmission=1.0, ior=1.5, thin_walled=0, **green))
    _box(mb, "amber_block", [-0.8, 0.002, 0.25], [-0.35, 0.8, 0.5], Material((1.0, 1.0, 1.0), 0.0, 0.0, transmission=1.0, ior=1.5, thin_walled=0, **amber))
    return _append(cornell(), mb.build())


SUNLIT_ROOM_CAMERA = dict(position=(0.0, 1.3, 2.6), direction=(-0.25, -0.12, -1.0), fov_deg=60.0)


def sunlit_room() -> Mesh:
    """A closed room, 4 x 2.6 x 6, whose only light comes through one window: an opening in the +x wall closed by a thin-walled, faintly
    green pane, with the sky and a directional "sun" outside.  Render it under sky(), with F_NEE_SKY | F_NEE_PUNCTUAL
    and PathTracer.set_pane_shadows(True): without pane shadows the sun never enters and the sky arrives only by paths that happen to
    cross the pane.  A diffuse block stands in the patch of sunlight."""
    from .assets import LIGHT_DIRECTIONAL, lights_array, make_light

    mb = MeshBuilder()
    wall, floor = Material((0.74, 0.72, 0.68), 0.0, 1.0), Material((0.55, 0.42, 0.3), 0.0, 0.8)
    x0, x1, y0, y1, z0, z1 = -2.0, 2.0, 0.0, 2.6, -3.0, 3.0
    wy0, wy1, wz0, wz1 = 0.7, 2.1, -1.6, 0.4  # the window in the wall x = x1
    mb.add("floor", *_grid([x0, y0, z1], [x1 - x0, 0, 0], [0, 0, z0 - z1], 1, 1), floor)
    mb.add("ceiling", *_grid([x0, y1, z0], [x1 - x0, 0, 0], [0, 0, z1 - z0], 1, 1), wall)
    mb.add("back", *_grid([x0, y0, z0], [x1 - x0, 0, 0], [0, y1 - y0, 0], 1, 1), wall)
    mb.add("front", *_grid([x1, y0, z1], [x0 - x1, 0, 0], [0, y1 - y0, 0], 1, 1), wall)
    mb.add("left", *_grid([x0, y0, z1], [0, 0, z0 - z1], [0, y1 - y0, 0], 1, 1), Material((0.6, 0.3, 0.25), 0.0, 1.0))
    # the +x wall around the window: below, above, and the two sides (normals -x: du along +z, dv along +y)
    for name, (a0, a1, b0, b1) in (("right_below", (z0, z1, y0, wy0)), ("right_above", (z0, z1, wy1, y1)),
                                   ("right_far", (z0, wz0, wy0, wy1)), ("right_near", (wz1, z1, wy0, wy1))):
        mb.add(name, *_grid([x1, b0, a0], [0, 0, a1 - a0], [0, b1 - b0, 0], 1, 1), wall)
    mb.add("window", *_grid([x1, wy0, wz0], [0, 0, wz1 - wz0], [0, wy1 - wy0, 0], 1, 1),
           Material((0.85, 0.95, 0.88), 0.0, 0.0, transmission=1.0, ior=1.5, thin_walled=1))
    _box(mb, "block", [-0.6, 0.0, -1.3], [0.2, 0.7, -0.5], Material((0.3, 0.45, 0.7), 0.0, 0.9))
    mesh = mb.build()
    mesh.lights = lights_array([make_light(LIGHT_DIRECTIONAL, (6.0, 5.4, 4.6), direction=(-1.0, -0.55, -0.2))])
    return mesh


MATERIAL_SEED = 20240607


def material_cornell(seed: int = MATERIAL_SEED) -> Mesh:
    """The Cornell box with material textures: the floor's roughness, metalness and normals come from maps (a
    brushed, tiled metal: factors 1, everything in the textures, as exporters write it) and the ceiling panel's emission from an emissive
    map (a grid of lamps).  The textures are generated from `seed`."""
    rng = np.random.default_rng(seed)
    mesh = cornell()
    n = 64
    yy, xx = np.mgrid[0:n, 0:n]
    tile = ((xx // 16) + (yy // 16)) % 2
    noise = rng.integers(0, 40, (n, n))
    rough = np.where(tile == 0, 60, 170) + noise  # G: polished and dull tiles
    metal = np.where(tile == 0, 255, 30)  # B
    mr = np.stack([np.zeros_like(rough), rough, metal, np.full_like(rough, 255)], -1).astype(np.uint8)
    # normal map of a height field: tile bevels plus seeded ripples; c = (-dh/dx, -dh/dy, 1) normalised, stored as (c + 1) / 2
    fx, fy = (xx % 16) / 16.0, (yy % 16) / 16.0
    height = 0.6 * np.minimum(np.minimum(fx, 1 - fx), np.minimum(fy, 1 - fy)).clip(0, 0.15)
    for _ in range(4):
        kx, ky, ph = rng.integers(1, 5), rng.integers(1, 5), rng.uniform(0, 2 * np.pi)
        height = height + 0.01 * np.sin(2 * np.pi * (kx * xx + ky * yy) / n + ph)
    dx = (np.roll(height, -1, 1) - np.roll(height, 1, 1)) * (n / 2.0) * 0.25
    dy = (np.roll(height, -1, 0) - np.roll(height, 1, 0)) * (n / 2.0) * 0.25
    c = np.stack([-dx, -dy, np.ones_like(dx)], -1)
    c /= np.linalg.norm(c, axis=-1, keepdims=True)
    nm = np.concatenate([np.round((c * 0.5 + 0.5) * 255.0), np.full((n, n, 1), 255.0)], -1).astype(np.uint8)
    lamps = (((xx % 16) - 8) ** 2 + ((yy % 16) - 8) ** 2 < 30).astype(np.uint8)
    em = np.stack([lamps * 255, lamps * 240, lamps * 200, np.full_like(lamps, 255)], -1).astype(np.uint8)
    mesh.textures = [np.ascontiguousarray(t) for t in (mr, nm, em)]
    light = int(np.flatnonzero((mesh.geometries["emission"][:, :3] != 0).any(1))[0])
    for g, name in enumerate(mesh.names):
        if name.startswith("floor"):
            mesh.geometries["base_color"][g] = (0.9, 0.85, 0.8, 1.0)
            mesh.geometries["metallic_factor"][g] = mesh.geometries["roughness"][g] = 1.0
            mesh.material_textures["metallic_roughness_texture"][g], mesh.material_textures["normal_texture"][g] = 0, 1
            mesh.material_textures["normal_scale"][g] = 1.5
            vo = int(mesh.geometries["vertex_offset"][g])
            later = [int(x) for x in mesh.geometries["vertex_offset"] if int(x) > vo]
            mesh.vertices[vo : (min(later) if later else len(mesh.vertices)), 6:8] *= 2.0
    mesh.material_textures["emissive_texture"][light] = 2
    mesh.geometries["emission"][light, :3] *= 3.0  # the lamps cover about a third of the panel
    return mesh


NEON_ROOM_CAMERA = dict(position=(0.6, 1.3, 1.7), direction=(-0.25, -0.05, -1.0), fov_deg=65.0)


def neon_sign_texture() -> np.ndarray:
    """64 x 16 RGBA8: black, with a few bright strokes (two bars, a rule and a dot).  Columns 0 .. 16 stay black."""
    t = np.zeros((16, 64, 4), np.uint8)
    t[..., 3] = 255
    t[2:14, 20:23, :3] = (255, 255, 255)
    t[2:14, 25:28, :3] = (255, 200, 255)
    t[7:9, 36:60, :3] = (255, 255, 230)
    t[11:13, 44:46, :3] = (200, 255, 255)
    return np.ascontiguousarray(t)


def neon_room() -> Mesh:
    """A closed 4 x 3 x 4 m room lit only by a thin sign on its back wall: the sign's emission is a factor times an
    emissive texture that is mostly black (neon_sign_texture), and its uvs run from -0.5 to 1.5, so the texture repeats twice along it.  Two
    boxes stand on the floor.  Without rt3_scene_set_textured_emitters only BSDF-sampled rays find the strokes."""
    mb = MeshBuilder()
    grey = Material((0.7, 0.7, 0.7))
    mb.add("floor", *_grid([-2, 0, 2], [4, 0, 0], [0, 0, -4], 4, 4), Material((0.6, 0.55, 0.5)))
    mb.add("ceiling", *_grid([-2, 3, -2], [4, 0, 0], [0, 0, 4], 2, 2), grey)
    mb.add("back", *_grid([-2, 0, -2], [4, 0, 0], [0, 3, 0], 2, 2), grey)
    mb.add("front", *_grid([2, 0, 2], [-4, 0, 0], [0, 3, 0], 2, 2), grey)
    mb.add("left", *_grid([-2, 0, 2], [0, 0, -4], [0, 3, 0], 2, 2), Material((0.65, 0.3, 0.3)))
    mb.add("right", *_grid([2, 0, -2], [0, 0, 4], [0, 3, 0], 2, 2), Material((0.3, 0.4, 0.65)))
    _box(mb, "box0", [-1.3, 0.0, -1.1], [-0.5, 1.0, -0.3], Material((0.8, 0.8, 0.75)))
    _box(mb, "box1", [0.4, 0.0, -0.3], [1.2, 0.5, 0.6], Material((0.75, 0.8, 0.8)))
    pos, nrm, uv, tris = _grid([-1.0, 1.9, -1.98], [2.0, 0, 0], [0, 0.3, 0], 8, 1)
    uv = uv.copy()
    uv[:, 0] = uv[:, 0] * 2.0 - 0.5
    mb.add("sign", pos, nrm, uv, tris, Material((0.1, 0.1, 0.1), emission=(8.0, 2.0, 6.0), emissive_texture=0))
    mesh = mb.build()
    mesh.textures = [neon_sign_texture()]
    return mesh


SKINNED_ARM_CAMERA = dict(position=(0.0137, 1.0071, 3.4), direction=(-0.08, -0.0033, -1.0), fov_deg=48.0)
# (the foot's coordinates and the segment length are binary fractions: the bind pose's palette is then the exact identity)
SKINNED_ARM_BASE, SKINNED_ARM_SEGMENT, SKINNED_ARM_RADIUS = (0.0625, 0.0, 0.625), 0.5, 0.17


def skinned_arm() -> Mesh:
    """The Cornell room without its left and front walls and, in it, an arm: a tube of three segments of 0.5 m standing
    on the floor, skinned to a chain of three joints (the root at its foot, one at each later segment's start) with weights that pass
    smoothly from a segment to the next, and one morph target, a bulge around the first joint above the root.  One animation of two seconds:
    the two upper joints bend about z and straighten again while the bulge swells and goes.  Mesh.vertices is the rest pose."""
    from .assets import Rig, Skin

    white, green = Material((0.73, 0.73, 0.73)), Material((0.12, 0.45, 0.15))
    light = Material((0.78, 0.78, 0.78), emission=(1.4, 1.2, 0.9))
    mb = MeshBuilder()
    n = 4
    mb.add("floor", *_grid([-1, 0, -1], [0, 0, 5], [2, 0, 0], n, n), white)
    mb.add("ceiling", *_grid([-1, 2, -1], [2, 0, 0], [0, 0, 5], n, n), white)
    mb.add("back", *_grid([-1, 0, -1], [2, 0, 0], [0, 2, 0], n, n), white)
    mb.add("right", *_grid([1, 0, -1], [0, 0, 5], [0, 2, 0], n, n), green)
    mb.add("panel", *_grid([-0.35, 1.995, -0.35], [0.7, 0, 0], [0, 0, 0.7], 2, 2), light)
    base, seg, radius = np.array(SKINNED_ARM_BASE), SKINNED_ARM_SEGMENT, SKINNED_ARM_RADIUS
    nseg, nring = 16, 24
    th, y = np.linspace(0, 2 * np.pi, nseg + 1), np.linspace(0, 1, nring + 1)
    T, Y = np.meshgrid(th, y, indexing="xy")
    H = 3.0 * seg * Y
    radial = np.stack([np.cos(T), np.zeros_like(T), np.sin(T)], -1)
    pos = (base + radius * radial + np.stack([np.zeros_like(H), H, np.zeros_like(H)], -1)).reshape(-1, 3)
    i = np.arange(nseg)[None, :] + (nseg + 1) * np.arange(nring)[:, None]
    a, b, c, d = i, i + 1, i + nseg + 2, i + nseg + 1
    tris = np.stack([np.stack([a, c, b], -1), np.stack([a, d, c], -1)], -2).reshape(-1, 3)  # outward
    first = mb.nv
    mb.add("arm", pos, radial.reshape(-1, 3), np.stack([T / (2 * np.pi), Y], -1).reshape(-1, 2), tris, Material((0.8, 0.55, 0.4)))
    mesh = mb.build()
    h = H.reshape(-1)

    def smooth(x):
        x = np.clip(x, 0.0, 1.0)
        return x * x * (3.0 - 2.0 * x)

    t1, t2 = smooth((h - 0.7 * seg) / (0.6 * seg)), smooth((h - 1.7 * seg) / (0.6 * seg))
    weights = np.stack([1.0 - t1, t1 - t2, t2, np.zeros_like(h)], 1).astype(np.float32)
    joints = np.tile(np.array([0, 1, 2, 0], np.uint16), (len(h), 1))
    bulge = (0.09 * np.exp(-(((h - seg) / (0.45 * seg)) ** 2)))[:, None] * radial.reshape(-1, 3)
    ibm = np.tile(np.eye(4), (3, 1, 1))
    for k in range(3):
        ibm[k, :3, 3] = -(base + [0.0, k * seg, 0.0])
    mesh.skins = [Skin(first, mesh.vertices[first:].copy(), joints, weights, [0, 1, 2], ibm, bulge[None], None, np.zeros(1, np.float32), len(mesh.geometries) - 1)]

    def about_z(deg):
        r = np.radians(deg) / 2.0
        return [0.0, 0.0, float(np.sin(r)), float(np.cos(r))]

    times = np.array([0.0, 1.0, 2.0], np.float32)
    nodes = [dict(name="shoulder", translation=[float(x) for x in base], parent=-1),
             dict(name="elbow", translation=[0.0, seg, 0.0], rotation=about_z(0.0), parent=0),
             dict(name="wrist", translation=[0.0, seg, 0.0], rotation=about_z(0.0), parent=1)]
    channels = [dict(path="rotation", node=1, interpolation="LINEAR", times=times, values=np.array([about_z(0), about_z(50), about_z(0)], np.float32)),
                dict(path="rotation", node=2, interpolation="LINEAR", times=times, values=np.array([about_z(0), about_z(-70), about_z(0)], np.float32)),
                dict(path="weights", skin=0, interpolation="LINEAR", times=times, values=np.array([[0.0], [1.0], [0.0]], np.float32))]
    mesh.rig = Rig(nodes, [dict(name="bend", channels=channels)])
    return mesh


def sky(width: int = 2048, height: int = 1024, seed: int = SKY_SEED) -> np.ndarray:
    """Equirect RGB32F sky: horizon-to-zenith gradient, ground bounce, soft cloud noise, 0.5 degree sun (5e4)."""
    rng = np.random.default_rng(seed)
    v = (np.arange(height) + 0.5) / height
    u = (np.arange(width) + 0.5) / width
    U, V = np.meshgrid(u, v, indexing="xy")
    theta = np.pi * V
    phi = 2 * np.pi * (U - 0.5)
    d = np.stack([np.cos(phi) * np.sin(theta), np.cos(theta), np.sin(phi) * np.sin(theta)], -1)
    up = np.clip(d[..., 1], 0, 1)
    zen, hor, gnd = np.array([0.18, 0.36, 0.9]), np.array([0.9, 0.95, 1.0]), np.array([0.18, 0.16, 0.14])
    t = up[..., None] ** 0.45
    col = hor * (1 - t) + zen * t
    col = np.where(d[..., 1:2] < 0, gnd * (1.0 + 0.5 * d[..., 1:2]), col)
    # low-frequency cloud modulation from a few random sinusoids (deterministic)
    cl = np.zeros_like(U)
    for _ in range(6):
        fx, fy = rng.integers(1, 6), rng.integers(1, 5)
        cl += rng.uniform(0.05, 0.15) * np.sin(2 * np.pi * (fx * U + rng.uniform()) ) * np.sin(np.pi * fy * V + rng.uniform(0, 6.28))
    col = col * (1.0 + np.where(d[..., 1] > 0, cl, 0)[..., None])
    sun_dir = np.array([0.30, 0.88, 0.25]); sun_dir /= np.linalg.norm(sun_dir)
    cosang = d @ sun_dir
    ang = np.degrees(np.arccos(np.clip(cosang, -1, 1)))
    sun = np.where(ang < 0.25, 5.0e4, 0.0) + 40.0 * np.exp(-(ang / 2.5) ** 2)
    col = col + sun[..., None] * np.array([1.0, 0.93, 0.82])
    return np.ascontiguousarray(np.maximum(col, 0.0), np.float32)
