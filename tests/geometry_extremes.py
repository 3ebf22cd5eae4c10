"""Scenes and rays at geometric extremes, shared by tests/test_walk_ref.py (CPU: the restatement against the oracle) and
tests/test_gpu_geometry_extremes.py (GPU: every walk against the restatement).

Each family is the random soup's generator (scenes.build_random_soup: centroids in [-1, 1]^3, corners within 0.15 of them) after a world-space map,
baked into the mesh itself, so every instance transform is the identity and the engine's world-space records are the float32 numbers built here.
Every family comes in two sizes: 40 triangles (the scene stays in LDS: kLdsSceneTexels, at most 112 entries) and 600 (compact and wide streams
with 16-bit links)."""
import json
import math
import os

import numpy as np

from strolle_amd import Camera, CameraMode, Instance, Light, Material, Mesh, Sun, scenes
from strolle_amd.api import RAY_DTYPE, look_at_transform, perspective_infinite_reverse_rh

PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "geometry_extremes.json")
SIZES = (40, 600)
N_RAYS, N_BUNDLE = 4096, 1024
FLT_MAX = np.float32(3.4028235e38)
IDENTITY = np.eye(4, dtype=np.float32)[:3]
MESH, MATERIAL, INSTANCE = 7, 1, 77


def _soup(n, rng):
    c = rng.uniform(-1, 1, (n, 1, 3))
    return c + rng.uniform(-0.15, 0.15, (n, 3, 3))


def _flat(y):
    def f(n, rng):
        p = _soup(n, rng); p[..., 1] = y
        return p
    return f


def _straddle(n, rng):
    p = _soup(n, rng) * 5000.0; p[..., 0] += 65000.0      # x of the centroids on [60000, 70000]: f16 bounds finite on one side of 65504, infinite on the other
    return p


def _stadium(n, rng):
    p = _soup(n - 2, rng) * 0.05
    w, y, cx, cz = 1.0e4, -0.5, 3000.0, -2000.0      # off centre: the quad's diagonal, an edge of both its triangles, stays 5,000 units from the soup
    quad = np.array([[(cx - w, y, cz - w), (cx + w, y, cz - w), (cx + w, y, cz + w)], [(cx - w, y, cz - w), (cx + w, y, cz + w), (cx - w, y, cz + w)]])
    return np.concatenate([p, quad])


def _concentric(n, rng):
    k = 64 if n >= 128 else n // 2
    p = _soup(n - k, rng)
    base = np.array([(-0.6, -0.5, 0.1), (0.7, -0.4, -0.2), (0.0, 0.8, 0.3)])
    c = base.mean(0)
    copies = c + (base - c)[None] * np.linspace(0.25, 1.0, k)[:, None, None]      # coplanar: one ray, up to 64 equal t
    return np.concatenate([p, copies])


def _slivers(n, rng):
    p = _soup(n, rng)
    k = max(2, n // 20)
    idx = rng.choice(n, k, replace=False)
    p[idx[: k // 2], 2] = p[idx[: k // 2], 1]                                    # two equal vertices
    s = rng.uniform(0.2, 0.8, (k - k // 2, 1))
    p[idx[k // 2:], 2] = p[idx[k // 2:], 0] + s * (p[idx[k // 2:], 1] - p[idx[k // 2:], 0])   # three collinear ones (up to float32 rounding)
    return p


def _mapped(scale=1.0, offset=(0.0, 0.0, 0.0)):
    return lambda n, rng: _soup(n, rng) * scale + np.asarray(offset, np.float64)


# name -> (positions(n, rng) in float64, what it reaches)
FAMILIES = {
    "unit": (_soup, "control: the scale every other test uses"),
    "offset_1e3_x": (_mapped(1.0, (1000.0, 0.0, 0.0)), "f16 step 0.5 units, slab error x 10^3"),
    "offset_far": (_mapped(1.0, (-3000.0, 2000.0, 5000.0)), "f16 step 1-4 units on every axis"),
    "scale_1e2": (_mapped(100.0), "large boxes, large t"),
    "scale_1e3": (_mapped(1000.0), "large boxes, large t"),
    "beyond_f16_x": (_mapped(100.0, (1.0e5, 0.0, 0.0)), "every x bound +inf / 65504"),
    "beyond_f16_neg": (_mapped(100.0, (-1.0e5, -1.0e5, -1.0e5)), "every bound -inf / -65504"),
    "straddle_f16": (_straddle, "finite and infinite bounds in one tree"),
    "small": (_mapped(0.05), "subnormal f16 bounds, the det cutoff"),
    "flat_0": (_flat(0.0), "zero Morton extent, zero-thickness boxes"),
    "flat_1000": (_flat(1000.3), "a plane f16 cannot represent"),
    "flat_1024": (_flat(1024.0), "a plane f16 represents exactly: zero-thickness f16 boxes a thousand units out"),
    "stadium": (_stadium, "every small centroid in one Morton cell"),
    "coincident_twice": (_soup, "each triangle twice (two instances of one mesh): equal Morton codes"),
    "coincident_concentric": (_concentric, "64 coplanar concentric copies of one triangle (20 of the 40): exact ties in t"),
    "slivers": (_slivers, "5 % zero-area records among ones that can be hit"),
}
# the winning slot of a tie is ambiguous by construction; t, hit / miss and occlusion are not. The flat families belong here: all their triangles lie in
# one plane and overlap, so a ray through an overlap has as many equal t as triangles there.
TIED = ("coincident_twice", "coincident_concentric", "flat_0", "flat_1000", "flat_1024")
CASES = [(f, n) for f in FAMILIES for n in SIZES]


def case_seed(family, n):
    return 1000 * list(FAMILIES).index(family) + n


def positions(family, n):
    """(n_mesh, 3, 3) float32 mesh positions of the family, world space (the instance transform is the identity)"""
    rng = np.random.default_rng(case_seed(family, n))
    n_mesh = n // 2 if family == "coincident_twice" else n
    return FAMILIES[family][0](n_mesh, rng).astype(np.float32)


def instance_handles(family):
    return (INSTANCE, INSTANCE + 1) if family == "coincident_twice" else (INSTANCE,)


def build_extreme(e, family, n, translation=None):
    """One opaque material, one mesh, one instance (two of the same mesh and transform in coincident_twice). `translation`: the instances' translation."""
    pos = positions(family, n)
    e1, e2 = pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]
    nrm = np.cross(e1, e2).astype(np.float64); ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.maximum(ln, 1e-300), np.array([0.0, 1.0, 0.0]))
    e.set_blue_noise(scenes.load_blue_noise())
    e.insert_material(MATERIAL, Material(base_color=(0.7, 0.7, 0.7, 1.0)))
    e.insert_mesh(MESH, Mesh(pos, np.repeat(nrm[:, None], 3, 1).astype(np.float32)))
    move(e, family, translation)
    lo, hi = pos.reshape(-1, 3).min(0), pos.reshape(-1, 3).max(0)
    e.insert_light(1, Light.point(((lo + hi) / 2 + (hi - lo)).tolist(), 0.1, (1.0, 1.0, 1.0), float(np.linalg.norm(hi - lo)) * 4))
    e.update_sun(Sun(azimuth=0.0, altitude=-1.0))
    return pos


def move(e, family, translation=None):
    x = IDENTITY.copy()
    if translation is not None:
        x[:, 3] = np.asarray(translation, np.float32)
    for h in instance_handles(family):
        e.insert_instance(h, Instance(MESH, MATERIAL, x))


def quarter_extent(family, pos):
    """the refit configuration's move: a quarter of the family's extent (of ray_box: the stadium's soup stays where float32 resolves it) along each axis"""
    p = (pos[:-2] if family == "stadium" else pos).reshape(-1, 3)
    return ((p.max(0) - p.min(0)) * np.float32(0.25)).astype(np.float32)


def box_of(triangles):
    """bounding box of read_scene(1) records (tests/test_gpu_ray_query.py scene_box)"""
    tris = np.ascontiguousarray(triangles).view(np.float32).reshape(-1, 9, 4)[:, [0, 3, 6], :3].reshape(-1, 3)
    return tris.min(0), tris.max(0)


def ray_box(family, triangles):
    """The box the family's rays and camera are generated relative to: the scene's bounding box. The stadium's is that of its small soup, reaching down to
    the quad's plane: a ray that starts thousands of units out on the quad cannot resolve a triangle 0.01 units wide in float32 (one ulp of its origin is a
    tenth of the triangle), so nearly every such ray would be ambiguous and say nothing. The quad still spans every ray that points down."""
    if family != "stadium":
        return box_of(triangles)
    recs = np.ascontiguousarray(triangles).view(np.float32).reshape(-1, 36)
    lo, hi = box_of(recs[:-2])
    qlo, _ = box_of(recs[-2:])
    lo = lo.copy(); lo[1] = min(lo[1], qlo[1])
    return lo, hi


def t_max_mix(n, rng, scale):
    """tests/test_gpu_ray_query.py t_max_mix: unbounded (inf, FLT_MAX) and bounded t_max, with the degenerate ones (0, negative, NaN) among them"""
    t = rng.uniform(0.05, 1.0, n).astype(np.float32) * np.float32(scale)
    k = rng.integers(0, 10, n)
    t[k < 3] = np.inf
    t[k == 3] = FLT_MAX
    t[k == 4] = rng.choice(np.array([0.0, -1.0, np.nan], np.float32), int((k == 4).sum()))
    return t


def make_rays(origins, dirs, t_max):
    r = np.zeros(len(origins), RAY_DTYPE)
    r["origin"] = origins; r["direction"] = dirs; r["t_max"] = t_max
    return r


def family_rays(family, n, triangles):
    """N_RAYS rays relative to the bounding box of the read_scene(1) records `triangles`: first the coherent bundle (N_BUNDLE rays from one point outside the
    box through a grid on it, unbounded), then the mix: origins inside the box and up to 20 % outside it, un-normalised directions of length 0.25-4 (six in ten
    aimed at or just beside a triangle, so that a sparse scene is hit at all and edges are grazed; the others anywhere), one in twenty axis-parallel per
    axis, all-zero directions, the t_max mix; for the flat families origins exactly on the plane with directions inside it."""
    rng = np.random.default_rng(case_seed(family, n) + 7)
    lo, hi = ray_box(family, triangles)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    ext = np.maximum(hi - lo, 1e-3 * float(np.linalg.norm(hi - lo)))     # a flat box still gets origins off its plane
    centre = (lo + hi) / 2
    # the bundle: from a point outside, through a 32 x 32 grid on the box's middle plane across its thinnest axis
    thin = int(np.argmin(hi - lo)); a, b = [k for k in range(3) if k != thin]
    eye = centre.copy(); eye[thin] += 1.5 * float(np.linalg.norm(hi - lo)); eye[a] += 0.1 * ext[a]
    g = (np.arange(32) + 0.5) / 32
    ga, gb = np.meshgrid(g, g, indexing="xy")
    target = np.tile(centre, (N_BUNDLE, 1)); target[:, a] = lo[a] + ga.reshape(-1) * (hi - lo)[a]; target[:, b] = lo[b] + gb.reshape(-1) * (hi - lo)[b]
    eye32 = np.tile(eye.astype(np.float32), (N_BUNDLE, 1))
    bundle = make_rays(eye32, (target.astype(np.float32) - eye32), np.full(N_BUNDLE, np.inf, np.float32))
    m = N_RAYS - N_BUNDLE
    o = rng.uniform(lo - 0.2 * ext, hi + 0.2 * ext, (m, 3)).astype(np.float32)
    d = rng.normal(size=(m, 3)).astype(np.float32) * rng.uniform(0.25, 4.0, (m, 1)).astype(np.float32)
    k = rng.integers(0, 20, m)
    verts = np.ascontiguousarray(triangles).view(np.float32).reshape(-1, 9, 4)[:, [0, 3, 6], :3].astype(np.float64)
    pick = verts[rng.integers(0, len(verts), m)]
    bu, bv = rng.uniform(-0.15, 1.0, m), rng.uniform(-0.15, 1.0, m)
    fold = bu + bv > 1.0; bu[fold], bv[fold] = 1.0 - bu[fold], 1.0 - bv[fold]
    aim = pick[:, 0] + bu[:, None] * (pick[:, 1] - pick[:, 0]) + bv[:, None] * (pick[:, 2] - pick[:, 0]) - o
    aim *= (rng.uniform(0.25, 4.0, (m, 1)) / np.maximum(np.linalg.norm(aim, axis=1, keepdims=True), 1e-30))
    d[k >= 8] = aim[k >= 8].astype(np.float32)
    for axis in range(3):
        sel = k == axis
        keep = d[sel, axis].copy(); d[sel] = 0.0; d[sel, axis] = keep
    d[k == 3] = 0.0
    if family.startswith("flat"):
        on = (k == 4) | (k == 5)
        o[on, 1] = np.float32(lo[1]); d[on, 1] = 0.0                  # on the plane, inside it
    t = t_max_mix(m, rng, float(np.linalg.norm(ext)) / 1.5)          # (directions average 1.5 long: bounded rays end inside the scene)
    return np.concatenate([bundle, make_rays(o, d, t)])


def family_camera(lo, hi, size=(96, 64), mode=CameraMode.REFERENCE, depth=0) -> Camera:
    """looks at the box's centre from outside it, across its thinnest axis and a little askew"""
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    diag = float(np.linalg.norm(hi - lo)); centre = (lo + hi) / 2
    thin = int(np.argmin(hi - lo))
    off = np.array([0.25, 0.35, 0.3]); off[thin] = 1.0
    eye = centre + off * diag * 0.9
    up = (0.0, 1.0, 0.0) if thin != 1 else (0.0, 0.0, -1.0)
    w, h = size
    return Camera(mode=mode, denoise=True, depth=depth, size=(w, h), transform=look_at_transform(eye.tolist(), centre.tolist(), up),
                  projection=perspective_infinite_reverse_rh(math.pi / 4.0, w / h, 0.1))


def oracle_trace(orac, rays):
    """or_probe_trace_rays: (hit, t, slot, point, occluded) of the oracle's own walk over its own tree, on the CPU — bounded as the scene queries'
    checkers bound it (tests/test_gpu_ray_query.py oracle_closest / oracle_occluded)"""
    import ctypes as C
    from oracle_binding import oracle_lib
    fn = oracle_lib().or_probe_trace_rays
    fn.restype = None; fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    n = len(rays)
    rays = np.ascontiguousarray(rays)
    dist, point, slot, occ = np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    fn(orac._h, rays.ctypes.data, n, dist.ctypes.data, point.ctypes.data, slot.ctypes.data, occ.ctypes.data)
    with np.errstate(invalid="ignore"):
        hit = (dist < FLT_MAX) & (dist < rays["t_max"])
    return hit, np.where(hit, dist, FLT_MAX), np.where(hit, slot.astype(np.int64), -1), np.where(hit[:, None], point, 0), occ == 1


_cases = {}


def oracle_case(family, n, moved=False):
    """The family's scene in the oracle, its rays, the restatement's answer and the oracle's; computed once per process, shared and left unchanged.
    moved: after the refit configuration's move (the instances translated by quarter_extent)."""
    import walk_ref
    from oracle_binding import OracleEngine
    key = (case_key(family, n), moved)
    if key not in _cases:
        orac = OracleEngine()
        try:
            pos = build_extreme(orac, family, n); orac.tick()
            if moved:
                move(orac, family, quarter_extent(family, pos)); orac.tick()
            tris = orac.read_scene(1).copy()
            lo, hi = box_of(tris)
            rays = family_rays(family, n, tris)
            extent = float(np.linalg.norm(hi.astype(np.float64) - lo.astype(np.float64)))
            ref = walk_ref.trace(*walk_ref.records(tris), rays)
            _cases[key] = dict(triangles=tris, lo=lo, hi=hi, extent=extent, rays=rays, ref=ref, oracle=oracle_trace(orac, rays))
        finally:
            orac.close()
    return _cases[key]


def same_triangle(triangles, a, b):
    """slots a and b name triangles with the same nine float32 vertex coordinates (the same slot, or coincident copies)"""
    v = np.ascontiguousarray(triangles).view(np.float32).reshape(-1, 9, 4)[:, [0, 3, 6], :3].reshape(-1, 9)
    return np.all(v[a].view(np.uint32) == v[b].view(np.uint32), axis=1)


def load_profile():
    with open(PROFILE) as f:
        return json.load(f)


def case_key(family, n):
    return f"{family}/{n}"
