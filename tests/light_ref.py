"""What the direct-lighting estimators converge to, defined in float64 from what the caller handed to the API: lights, Material fields, meshes,
transforms and the camera. No reservoir, no random number and no engine record is read here.

Light::radiance (light.rs:143-207) is a deterministic function of the primary hit and the light. ReSTIR DI picks ONE light per pixel and frame and
weights it by 1 / (its probability), so for a pixel from which every light is either wholly visible or wholly hidden the long-run mean of its output is
a plain sum over the visible lights:

    DI_DIFFUSE     sum_i  L_i (1 - metallic) / pi                              (di_resolving.rs: the base colour is multiplied in by the composition)
    DI_SPECULAR    sum_i  L_i spec_i
    REFERENCE      emissive + sum_i L_i (base (1 - metallic) / pi + spec_i)    at depth 0; deeper paths add what the bounce sees
    IMAGE          emissive + base . DI_DIFFUSE + DI_SPECULAR                  plus GI, which has no closed form

    L_i      = colour . f_angle . f_dist . f_cosine
    l        = centre - point
    f_angle  = 1 for a point light; saturate(1 - (angle(spot_dir, point - centre) / spot_angle)^3) for a spot
    f_dist   = 1 where the range is infinite; saturate(1 - (|l|^2 / range^2)^2)^2 / max(|l|^2, 1e-4) otherwise
    f_cosine = saturate(n . normalize(l))
    spec_i   = intensity . D G F / (4 n.l n.v)  (brdf.rs:9-186) with the sphere light's representative point: r = reflect(-v, n),
               c = (l . r) r - l, p = l + c saturate(radius / |c|), ls = normalize(p), a = clamp(roughness, 0.089^2, 1),
               intensity = (a / saturate(a + radius / (2 |p|)))^2, h = normalize(ls + v), D = a^2 / (pi ((n.h a^2 - n.h) n.h + 1)^2),
               G = g(n.v) g(n.l) with g(x) = x / (x (1 - k) + k), k = a^2 / 2, f0 = 0.16 reflectance^2 (1 - metallic) + base metallic,
               f90 = saturate(50 . 0.33 (f0.r + f0.g + f0.b)), F = f0 + (f90 - f0) max(1 - l.h, 0.001)^5; 0 where metallic <= 0, n.l <= 0 or n.v <= 0

The primary hit is surface_ref's (walk_ref's brute force over all triangles). The ReSTIR modes read it back from the G-buffer, so there the material
passes through the G-buffer's quantisation (pack here, surface_ref.decode_gbuffer back) and the point is ray.at(depth - 0.01) (hit.rs:8-81); Reference
mode shades the unquantised material at point + 0.01 normal (ref_shading.rs).

Visibility: a light is LIT at a pixel if no triangle crosses any segment from the hit point to `ENDS` points on the sphere of 1.3 x its radius around
its centre, HIDDEN if every such segment is crossed, and otherwise the pixel is AMBIGUOUS (a penumbra: its mean depends on how the light's disk is
sampled, which is the estimator's business, not the definition's). 1.3 covers both samplers: ray_bnoise aims at a disk of the light's radius
perpendicular to the light direction but ends its ray at the light's DISTANCE, up to sqrt(1 + (r/d)^2) further out than the centre; ray_wnoise stays on
the sphere."""
from dataclasses import dataclass

import numpy as np

import surface_ref
import walk_ref

NUDGE = 0.01
ROUGHNESS_FLOOR = 0.089 ** 2
ENDS = 256
REACH = 1.3
RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("t_min", np.float32), ("direction", np.float32, 3), ("t_max", np.float32)])
LIT, HIDDEN, AMBIGUOUS = 0, 1, 2
MARGIN = 1e-5          # walk_ref's decision margin below which float32 may decide the PRIMARY ray the other way (a pixel centre on a shared edge): not held


def _dot(a, b):
    return np.einsum("...i,...i->...", a, b)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def saturate(x):
    return np.clip(x, 0.0, 1.0)


# ----------------------------------------------------------------------------- camera (camera.rs:80-93)
def camera_rays(camera):
    """(origins [n,3], unit directions [n,3]) float64, row-major: the pixel centre unprojected at NDC depth 1 (near) and float32 epsilon (far) through
    transform . inverse(projection)"""
    w, h = camera.size
    m = np.asarray(camera.transform, np.float32).astype(np.float64) @ np.linalg.inv(np.asarray(camera.projection, np.float32).astype(np.float64))
    x, y = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    nx, ny = (x * 2.0 / w - 1.0).ravel(), -(y * 2.0 / h - 1.0).ravel()

    def unproject(z):
        p = np.stack([nx, ny, np.full_like(nx, z), np.ones_like(nx)], 1) @ m.T
        return p[:, :3] / p[:, 3:]
    near, far = unproject(1.0), unproject(walk_ref.F32_EPS)
    return near, _unit(far - near)


def make_rays(origins, dirs, t_max=np.inf):
    r = np.zeros(len(origins), RAY_DTYPE)
    r["origin"] = origins; r["direction"] = dirs; r["t_max"] = t_max
    return r


# ----------------------------------------------------------------------------- the G-buffer's quantisation (gbuffer.rs:8-124)
def _oct_encode(n):
    n = n / np.abs(n).sum(axis=1, keepdims=True)
    t = 1.0 - np.abs(n[:, [1, 0]])
    fold = np.where(n[:, 2:3] >= 0, n[:, :2], np.copysign(t, n[:, :2]))
    return fold * 0.5 + 0.5


def _byte(x, top=255.0):
    """`clamp(x, 0, 1) * top as u32` in float32: truncation"""
    return np.floor(np.clip(np.asarray(x, np.float64), 0.0, 1.0).astype(np.float32) * np.float32(top)).astype(np.uint32)


def pack_gbuffer(surf: surface_ref.Surface, reflectance):
    """The two G-buffer words of a surface_ref.Surface, [n,4] float32 each, as GBufferEntry::pack writes them"""
    n = len(surf.depth)
    d0, d1 = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    d0[:, 0] = surf.depth
    with np.errstate(all="ignore"):
        d0[:, 1:3] = _oct_encode(surf.normal)
    w = _byte(surf.metallic) | (_byte(np.sqrt(surf.roughness)) << 8) | (_byte(reflectance) << 16) | (1 << 24)
    d0[:, 3] = w.astype(np.uint32).view(np.float32)
    d1[:, :3] = surf.emissive
    g = np.clip(surf.base_color, 0.0, None) ** (1.0 / 2.2)
    c = _byte(g[:, 0]) | (_byte(g[:, 1]) << 8) | (_byte(g[:, 2]) << 16) | (_byte(g[:, 3], 63.0) << 24)
    d1[:, 3] = c.astype(np.uint32).view(np.float32)
    return d0, d1


# ----------------------------------------------------------------------------- the hit a lighting pass shades
@dataclass
class Hits:
    hit: np.ndarray           # bool [n]
    point: np.ndarray         # [n,3] the nudged point the light is evaluated at
    view: np.ndarray          # [n,3] v = -ray direction
    normal: np.ndarray        # [n,3]
    base_color: np.ndarray    # [n,3]
    emissive: np.ndarray      # [n,3]
    metallic: np.ndarray
    roughness: np.ndarray
    reflectance: np.ndarray
    instance: np.ndarray      # index into scene.instances, -1 on a miss
    margin: np.ndarray        # walk_ref's decision margin of the primary ray


def primary_hits(scene: surface_ref.Scene, camera, gbuffer: bool = True) -> Hits:
    """The hit every pixel's lighting is evaluated at. gbuffer=True: as the ReSTIR passes rebuild it from the G-buffer (quantised material, decoded normal,
    ray.at(depth - 0.01)); False: as Reference mode shades it (the material as stated, point + 0.01 normal)."""
    o, d = camera_rays(camera)
    surf = surface_ref.surface(scene, make_rays(o, d))
    hit = surf.ans.hit
    mat_of = np.array([m for _, _, m, _, _ in scene.instances])
    refl = np.array([float(np.float32(scene.materials[mat_of[i]].reflectance)) if i >= 0 else 0.0 for i in surf.instance])
    if gbuffer:
        g = surface_ref.decode_gbuffer(*pack_gbuffer(surf, refl))
        point = o + d * (g["depth"] - NUDGE)[:, None]
        normal, base, emis, metal, rough, refl = g["normal"], g["base_color"][:, :3], g["emissive"], g["metallic"], g["roughness"], g["reflectance"]
    else:
        point = surf.ans.point + surf.normal * NUDGE
        normal, base, emis, metal, rough = surf.normal, surf.base_color[:, :3], surf.emissive, surf.metallic, surf.roughness
    return Hits(hit, point, -d, normal, base, emis, metal, rough, refl, surf.instance, surf.ans.decision_margin)


# ----------------------------------------------------------------------------- light.rs:143-207
def spot_direction(direction):
    """The direction a spot light keeps: octahedrally encoded into two float32 and decoded again (light.rs:25-79)"""
    e = _oct_encode(np.asarray(direction, np.float32).astype(np.float64)[None]).astype(np.float32).astype(np.float64)
    return surface_ref._oct_decode(e)[0]


def f_angle(light, point):
    if light.kind == 0:
        return np.ones(len(point))
    to_point = point - np.asarray(light.position, np.float32).astype(np.float64)
    cos = _dot(_unit(to_point), spot_direction(light.direction))
    return saturate(1.0 - (np.arccos(np.clip(cos, -1.0, 1.0)) / float(np.float32(light.angle))) ** 3)


def f_dist(light, point):
    rng = float(np.float32(light.range))
    if np.isinf(rng):
        return np.ones(len(point))
    l = np.asarray(light.position, np.float32).astype(np.float64) - point
    l2 = _dot(l, l)
    smooth = saturate(1.0 - (l2 / rng ** 2) ** 2)
    return smooth * smooth / np.maximum(l2, 1e-4)


def f_cosine(light, point, normal):
    l = np.asarray(light.position, np.float32).astype(np.float64) - point
    return saturate(_dot(normal, _unit(l)))


def incident(light, point, normal):
    """L [n,3] = colour . f_angle . f_dist . f_cosine"""
    colour = np.asarray(light.color, np.float32).astype(np.float64)
    return colour[None, :] * (f_angle(light, point) * f_dist(light, point) * f_cosine(light, point, normal))[:, None]


def diffuse_factor(metallic):
    """(1 - metallic) / pi: what DI resolving multiplies L by; the base colour comes in with the composition"""
    return (1.0 - np.asarray(metallic, np.float64)) / np.pi


def specular_brdf(normal, l, v, base_color, metallic, roughness, reflectance):
    """brdf.rs specular_brdf_eval for unit l and v, [n,3]"""
    n_rows = len(normal)
    a = np.clip(roughness, ROUGHNESS_FLOOR, 1.0)
    with np.errstate(all="ignore"):
        h = _unit(l + v)
    n_l, n_h, l_h, n_v = (saturate(_dot(normal, l)), saturate(_dot(normal, h)), saturate(_dot(l, h)), saturate(_dot(normal, v)))
    a2 = a * a
    dd = (n_h * a2 - n_h) * n_h + 1.0
    k = a2 / 2.0
    with np.errstate(all="ignore"):
        dist = a2 / (np.pi * dd * dd)
        mask = (n_v / (n_v * (1.0 - k) + k)) * (n_l / (n_l * (1.0 - k) + k))
        f0 = (0.16 * reflectance ** 2 * (1.0 - metallic))[:, None] + base_color * metallic[:, None]
        f90 = saturate(f0.sum(axis=1) * (50.0 * 0.33))
        fres = f0 + (f90[:, None] - f0) * (np.maximum(1.0 - l_h, 0.001) ** 5)[:, None]
        out = (dist * mask / (4.0 * n_l * n_v))[:, None] * fres
    dead = (metallic <= 0.0) | (n_l <= 0.0) | (n_v <= 0.0)
    out[dead] = 0.0
    assert out.shape == (n_rows, 3)
    return out


def specular_factor(light, hits: Hits):
    """spec_i [n,3]: the representative point of the sphere light, its intensity, and the BRDF towards it"""
    l = np.asarray(light.position, np.float32).astype(np.float64) - hits.point
    v, n = hits.view, hits.normal
    radius = float(np.float32(light.radius))
    r = -v - 2.0 * _dot(n, -v)[:, None] * n
    c = _dot(l, r)[:, None] * r - l
    with np.errstate(all="ignore"):
        p = l + c * saturate(radius / np.linalg.norm(c, axis=1))[:, None]
    inv_len = 1.0 / np.linalg.norm(p, axis=1)
    a = np.clip(hits.roughness, ROUGHNESS_FLOOR, 1.0)
    intensity = (a / saturate(a + radius * 0.5 * inv_len)) ** 2
    return intensity[:, None] * specular_brdf(n, p * inv_len[:, None], v, hits.base_color, hits.metallic, hits.roughness, hits.reflectance)


# ----------------------------------------------------------------------------- visibility classes
def sphere_ends(count: int = ENDS):
    """`count` unit vectors: a Fibonacci lattice, with the six axis points in front so the extremes are always among them"""
    k = np.arange(count - 6) + 0.5
    z = 1.0 - 2.0 * k / (count - 6)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    s = np.sqrt(1.0 - z * z)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    return np.concatenate([axes, np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)])


def visibility(scene: surface_ref.Scene, lights, hits: Hits, ends: int = ENDS):
    """[n_lights, n_pixels] of LIT / HIDDEN / AMBIGUOUS (misses are AMBIGUOUS): walk_ref.trace over all triangles along the segments hit point -> end"""
    (p0, e1, e2), _, _ = surface_ref.records(scene)
    dirs = sphere_ends(ends)
    n = len(hits.point)
    out = np.full((len(lights), n), AMBIGUOUS, np.int8)
    rows = np.flatnonzero(hits.hit)
    for i, light in enumerate(lights):
        centre = np.asarray(light.position, np.float32).astype(np.float64)
        end = centre[None, None, :] + dirs[None, :, :] * (REACH * float(np.float32(light.radius)))
        origin = np.broadcast_to(hits.point[rows, None, :], (len(rows), len(dirs), 3))
        seg = (end - origin).reshape(-1, 3)
        rays = np.zeros(len(seg), np.dtype([("origin", np.float64, 3), ("direction", np.float64, 3), ("t_max", np.float64)]))
        rays["origin"] = origin.reshape(-1, 3); rays["direction"] = seg; rays["t_max"] = 1.0
        crossed = walk_ref.trace(p0, e1, e2, rays).occluded.reshape(len(rows), len(dirs))
        out[i, rows] = np.where(~crossed.any(axis=1), LIT, np.where(crossed.all(axis=1), HIDDEN, AMBIGUOUS))
    return out


# ----------------------------------------------------------------------------- the expectation of each mode
@dataclass
class Expectation:
    value: np.ndarray         # [h, w, 3] float64
    held: np.ndarray          # [h, w] bool: the pixel hits geometry, decidedly (MARGIN), and no light is ambiguous there
    lit: np.ndarray           # [n_lights, h, w] bool
    hidden: np.ndarray        # [n_lights, h, w] bool
    hits: Hits


MODES = ("DI_DIFFUSE", "DI_SPECULAR", "REFERENCE", "IMAGE")


def expectation(scene: surface_ref.Scene, lights, camera, mode: str, ends: int = ENDS, geometry=None) -> Expectation:
    """The closed form of `mode` (a name of MODES) at every pixel. REFERENCE and IMAGE are their direct part: what a bounce or GI adds is not in it.
    geometry: (primary_hits, visibility) of the same scene, camera and hit kind, if the caller has them already."""
    assert mode in MODES, mode
    w, h = camera.size
    hits = geometry[0] if geometry else primary_hits(scene, camera, gbuffer=mode != "REFERENCE")
    vis = geometry[1] if geometry else visibility(scene, lights, hits, ends)
    value = np.zeros((w * h, 3))
    for i, light in enumerate(lights):
        L = incident(light, hits.point, hits.normal) * (vis[i] == LIT)[:, None]
        diff = diffuse_factor(hits.metallic)[:, None]
        if mode == "DI_DIFFUSE":
            value += L * diff
        elif mode == "DI_SPECULAR":
            value += L * specular_factor(light, hits)
        else:
            value += L * (diff * hits.base_color + specular_factor(light, hits))
    if mode in ("REFERENCE", "IMAGE"):
        value += hits.emissive
    value[~hits.hit] = 0.0
    held = hits.hit & ~(vis == AMBIGUOUS).any(axis=0) & (hits.margin >= MARGIN)
    return Expectation(value.reshape(h, w, 3), held.reshape(h, w), (vis == LIT).reshape(-1, h, w), (vis == HIDDEN).reshape(-1, h, w), hits)
