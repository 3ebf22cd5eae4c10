"""The scenes and the input matrix of the light-shafts tests (include/strolle_hip.h "light shafts"), shared by tests/test_shafts_abi.py
(the restatement against the float64 definition, on the CPU) and tests/test_gpu_shafts.py (st_light_shafts_process against the
restatement): two slat scenes, synthetic colour and depth planes, the camera, the lights, the descs and the list of cases.

The slat scenes: a floor and a wall of sixteen upright slats at x = 3 with gaps as wide as the slats, between a low sun in the +x sky and
the volume the camera looks through, so that the sun and the two lights behind the wall throw shafts across the view. `slats` has 34
triangles (its tree fits LDS: the <true, 16-bit> instantiation); `slats600` cuts every slat into 17 strips, 546 triangles (the
<false, 16-bit> one), still within walk_ref's brute-force reach."""
import numpy as np

import fog_cases
from strolle_amd import Instance, Light, Material, Mesh, Sun, light_shafts_desc, scenes

F = np.float32
nan, inf = float("nan"), float("inf")
FLT_MAX = np.finfo(np.float32).max
SIZES = [(72, 52), (41, 23), (9, 9), (5, 5), (1, 1)]
EYE, TARGET = (0.0, 1.2, 3.0), (0.3, 1.0, -5.0)
SUN_DIRECTION = (0.8, 0.5, -0.15)           # towards the sun: low, behind the wall
POINT, SPOT, MISSING = 11, 12, 99            # light handles; MISSING is never inserted
LIGHTS = {
    POINT: Light.point((4.5, 1.5, -4.0), 0.1, (40.0, 30.0, 20.0), 14.0),
    SPOT: Light.spot((4.0, 3.0, -1.0), 0.05, (10.0, 60.0, 90.0), 12.0, (-0.9, -0.5, -0.3), 0.7),
}
IDENTITY = np.eye(4, dtype=np.float32)[:3]


def _quad(a, b, c, d):
    return [[a, b, c], [a, c, d]]


def slat_positions(strips):
    tris = _quad((-8.0, 0.0, 4.0), (8.0, 0.0, 4.0), (8.0, 0.0, -14.0), (-8.0, 0.0, -14.0))   # the floor
    for k in range(16):
        z0 = 1.0 - 0.7 * k
        z1 = z0 - 0.35
        for s in range(strips):
            y0, y1 = 4.0 * s / strips, 4.0 * (s + 1) / strips
            tris += _quad((3.0, y0, z0), (3.0, y0, z1), (3.0, y1, z1), (3.0, y1, z0))
    return np.array(tris, np.float32)


def build_slats(e, strips=1, lights=True):
    """strips = 1: `slats` (34 triangles); strips = 17: `slats600` (546)"""
    pos = slat_positions(strips)
    nrm = np.cross(pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0])
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    e.set_blue_noise(scenes.load_blue_noise())
    e.insert_material(1, Material(base_color=(0.7, 0.7, 0.7, 1.0)))
    e.insert_mesh(7, Mesh(pos, np.repeat(nrm[:, None], 3, 1).astype(np.float32)))
    e.insert_instance(77, Instance(7, 1, IDENTITY.copy()))
    if lights:
        for h, l in LIGHTS.items():
            e.insert_light(h, l)
    e.update_sun(Sun(azimuth=0.0, altitude=-1.0))
    return len(pos)


SCENES = {"slats": 1, "slats600": 17}


def camera(size):
    return scenes.camera_for(size, EYE, TARGET)


def transform(size):
    return np.asarray(camera(size).transform, np.float32).T.reshape(-1).copy()


def projection(size):
    return np.asarray(camera(size).projection, np.float32).T.reshape(-1).copy()


def depth(kind, w, h, seed=4):
    """distances along the rays: a plane seen at a slant, a step edge, all sky, and the step with entries no frame holds"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    if kind == "plane":
        return (3.0 + 6.0 * x / max(w, 2) + 1.5 * y / max(h, 2)).astype(np.float32)
    if kind == "sky":
        return np.full((h, w), FLT_MAX, np.float32)
    z = np.where(x + 0.5 * y < 0.55 * w, 2.5, 9.0).astype(np.float32) * (1.0 + 0.01 * rng.random((h, w))).astype(np.float32)
    if kind == "odd":
        n = max(1, w * h // 40)
        for v in (nan, 0.0, -2.0, inf, FLT_MAX, 1e-30):
            z[rng.integers(0, h, n), rng.integers(0, w, n)] = v
        if w >= 4 and h >= 4:
            z[0:2, 0:2] = nan; z[2:4, 0:2] = 0.0   # whole blocks without a valid depth
    return z


BASE = dict(density=0.08, max_distance=12.0, intensity=1.5, scatter=(0.9, 0.8, 0.6))
SUN = dict(sun_color=(6.0, 5.0, 4.0), sun_direction=SUN_DIRECTION)


def cases():
    """(name, (w, h), depth kind, desc) of every synthetic case: every source alone, all of them with the extinction flag, a missing
    handle, g in {-0.6, 0, 0.8}, steps 1 / 4 / 16 / 64, both divisors, the four depth fields, every size"""
    D = light_shafts_desc
    return [
        ("sun-d2-s16-plane", (72, 52), "plane", D(steps=16, divisor=2, anisotropy=0.8, **BASE, **SUN)),
        ("sun-d1-s4-step", (41, 23), "step", D(steps=4, divisor=1, anisotropy=0.0, **BASE, **SUN)),
        ("point-d2-s16-plane", (41, 23), "plane", D(steps=16, divisor=2, anisotropy=-0.6, lights=(POINT,), **BASE)),
        ("spot-d1-s16-odd", (41, 23), "odd", D(steps=16, divisor=1, anisotropy=0.0, lights=(SPOT,), **BASE)),
        ("all-ext-d2-s4-step", (72, 52), "step", D(steps=4, divisor=2, anisotropy=0.8, lights=(SPOT, POINT), light_extinction=True, **BASE, **SUN)),
        ("all-d2-s16-odd", (41, 23), "odd", D(steps=16, divisor=2, anisotropy=-0.6, lights=(POINT, SPOT), **BASE, **SUN)),
        ("missing-d2-s1-plane", (9, 9), "plane", D(steps=1, divisor=2, anisotropy=0.0, lights=(MISSING, POINT), **BASE)),
        ("sun-d1-s64-plane", (9, 9), "plane", D(steps=64, divisor=1, anisotropy=0.8, **BASE, **SUN)),
        ("all-d2-s64-odd", (5, 5), "odd", D(steps=64, divisor=2, anisotropy=0.0, lights=(POINT, SPOT), **BASE, **SUN)),
        ("sky-d2-s4", (41, 23), "sky", D(steps=4, divisor=2, anisotropy=0.8, lights=(POINT,), **BASE, **SUN)),
        ("all-d1-s16-1x1", (1, 1), "plane", D(steps=16, divisor=1, anisotropy=0.8, lights=(POINT, SPOT), **BASE, **SUN)),
        ("all-d2-s4-1x1", (1, 1), "step", D(steps=4, divisor=2, anisotropy=0.0, lights=(POINT, SPOT), **BASE, **SUN)),
    ]


def inputs(size, kind):
    w, h = size
    return fog_cases.image(w, h), depth(kind, w, h), transform(size), projection(size)


def table_lights(d, present=LIGHTS):
    """the restatement's lights for a desc: the handles that name a light, in the desc's order"""
    import shafts_ref
    return [shafts_ref.table_light(present[int(d.lights[i])]) for i in range(d.light_count) if int(d.lights[i]) in present]
