"""The input matrix of the fog tests (include/strolle_hip.h "fog"), shared by tests/test_fog_abi.py (the restatement against the float64
definition) and tests/test_gpu_fog.py (st_fog_process against the restatement): images, depth fields, camera transforms, descs and the
list of cases. Not the full product: every factor at every level at least once and every pair of {falloff, height, lobe, sky}."""
import math

import numpy as np

import fog_ref as R
from strolle_amd import FogFalloff, fog_desc, scenes

F = np.float32
nan, inf = float("nan"), float("inf")
SIZE = (72, 52)
SIZES = [(72, 52), (33, 21), (64, 8), (5, 5), (1, 1)]   # partial groups both ways; a second group one pixel wide; exactly the groups; one partial group twice


def image(w, h, seed=11):
    """HDR colours with fireflies, negatives, NaN, infinities, values above 65504 and alpha != 1"""
    rng = np.random.default_rng(seed)
    img = np.exp(rng.standard_normal((h, w, 4)) * 2.0).astype(np.float32)
    img[rng.random((h, w)) < 0.01] *= 300.0
    img[rng.random((h, w)) < 0.03] *= -1.0
    n = max(1, w * h // 150)
    for v in (nan, inf, -inf, 0.0, -0.0, 1e30, 70000.0):
        img[rng.integers(0, h, n), rng.integers(0, w, n), rng.integers(0, 3, n)] = v
    return img


def depth(kind, w, h, seed=6):
    """distances along the rays"""
    rng = np.random.default_rng(seed)
    if kind == "ramp":
        return np.broadcast_to(np.linspace(1.0, 9.0, w, dtype=np.float32), (h, w)).copy()
    by, bx = (h + 7) // 8, (w + 7) // 8   # three layers in 8 x 8 blocks with noise and sky ...
    z = rng.choice(np.array([1.1, 3.0, 20.0], np.float32), (by, bx))
    z[rng.random((by, bx)) < 0.15] = R.FLT_MAX
    if by * bx > 1:
        z[0, 0], z[-1, -1] = 3.0, R.FLT_MAX   # (both kinds of pixel at every size but 1 x 1)
    z = np.repeat(np.repeat(z, 8, 0), 8, 1)[:h, :w].copy()
    z = np.where(z == R.FLT_MAX, z, z * (1.0 + 0.01 * rng.random((h, w)))).astype(np.float32)
    if kind == "blocks":                  # ... and depths no frame holds
        n = max(1, w * h // 200)
        for v in (nan, inf, -inf, 0.0, -2.0, 1e-30):
            z[rng.integers(0, h, n), rng.integers(0, w, n)] = v
    return z


DEPTHS = ("ramp", "layers", "blocks")


def projection(w, h):
    """the 16 floats of the Cornell camera's projection at this size, column major (45 degrees: P[5] = 2.414)"""
    return np.asarray(scenes.cornell_camera((w, h)).projection, np.float32).T.reshape(-1).copy()


def _rot(axis, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def transform(rotation=np.eye(3), position=(0.0, 0.0, 0.0)):
    m = np.eye(4)
    m[:3, :3] = rotation
    m[:3, 3] = position
    return m.T.reshape(-1).astype(np.float32)   # column major


TRANSFORMS = {
    "identity": transform(),
    "pitched": transform(_rot("x", -30.0), (1.0, 2.0, 3.0)),                     # 30 degrees down
    "rolled": transform(_rot("y", 25.0) @ _rot("z", 40.0), (-2.0, 1.5, 0.5)),    # rolled 40 degrees and yawed
    "high": transform(_rot("x", -20.0), (0.0, 50.0, 0.0)),                       # 50 m above the reference height
    "low": transform(_rot("x", 35.0), (0.0, -50.0, 0.0)),                        # 50 m below it, looking up
}

FALLOFF = {
    0: dict(falloff=FogFalloff.LINEAR, start=2.0, end=15.0),
    1: dict(falloff=FogFalloff.EXPONENTIAL, density=0.15),
    2: dict(falloff=FogFalloff.EXPONENTIAL_SQUARED, density=0.08),
    3: dict(falloff=FogFalloff.ATMOSPHERIC, extinction=(0.05, 0.1, 0.0), inscattering=(0.08, 0.0, 0.12)),   # one channel of each is 0
}
HEIGHT = dict(height_falloff=0.2, height_reference=0.0)
LOBE = dict(light_color=(1.0, 0.6, 0.0), light_exponent=8.0, light_direction=(0.3, 0.5, -0.8))
SKY = dict(sky_distance=40.0)
# every pair of {falloff, height, lobe, sky}: each falloff with a (height, lobe, sky) triple and its complement, the four triples chosen so
# that every pair of the three switches takes its four values
TRIPLES = {0: (0, 0, 0), 1: (0, 1, 1), 2: (1, 0, 1), 3: (1, 1, 0)}


def desc(falloff, height, lobe, sky, alpha=1.0, rgb=(0.5, 0.6, 0.7), **more):
    kw = dict(FALLOFF[falloff])
    for on, part in ((height, HEIGHT), (lobe, LOBE), (sky, SKY)):
        if on:
            kw.update(part)
    kw.update(more)
    return fog_desc(color=tuple(rgb) + (alpha,), **kw)


def _eight():
    out = []
    for f, t in TRIPLES.items():
        out.append((f,) + t)
        out.append((f,) + tuple(1 - v for v in t))
    return out


def cases():
    """(name, (w, h), depth kind, transform name, desc) of every synthetic case"""
    out = []
    names = list(TRANSFORMS)
    for i, (f, hh, l, s) in enumerate(_eight()):
        for j, kind in enumerate(DEPTHS):
            t = names[(i + j) % len(names)]
            out.append((f"f{f}h{hh}l{l}s{s}-{kind}-{t}", SIZE, kind, t, desc(f, hh, l, s, alpha=1.0 if (i + j) % 2 else 0.75)))
    # the camera far above and far below the reference height with b = 0.2 (E0 = e^-10, e^10), every falloff; and with b = 2 and a far sky,
    # where the exponent of E0 and k reach their clamps
    for t in ("high", "low"):
        for f in range(4):
            out.append((f"f{f}-b0.2-{t}", SIZE, "layers", t, desc(f, 1, 1, 1)))
        out.append((f"f1-b2-{t}", SIZE, "layers", t, desc(1, 1, 0, 1, height_falloff=2.0, sky_distance=1.0e4, density=1e-35 if t == "low" else 1.0e34)))   # (E0 = e^80, e^-80: densities that leave g between 0 and 1)
    for size in SIZES[1:]:
        out.append((f"small-{size[0]}x{size[1]}-a", size, "blocks", "rolled", desc(1, 1, 1, 1)))
        out.append((f"small-{size[0]}x{size[1]}-b", size, "layers", "pitched", desc(3, 1, 1, 0, alpha=0.5)))
    return out


def inputs(size, kind, tname):
    w, h = size
    return image(w, h), depth(kind, w, h), TRANSFORMS[tname], projection(w, h)
