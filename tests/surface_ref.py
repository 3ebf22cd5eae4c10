"""What the renderer reads off the winning triangle, defined in float64 from what the caller handed to the API — mesh positions, normals and uvs, each
instance's 3x4 transform and its previous one, Material fields, image pixels as uint8, cameras. Nothing here reads read_scene records, atlas rectangles
or anything else an engine derived: the bake (TriangleSlots::write, the device bake) and the atlas placement are under test, not trusted. No tree is built:
which triangle wins, its (u, v), t, the point and the ambiguity margin are walk_ref.trace's, over world vertices formed here as M . p in float64 and
rounded to float32 (the engine intersects float32 records; tests/test_surface_ref.py holds the baked positions to these within 2 ulp of the extent).

    normal     n_i = normalize(inverse(M3x3)^T . n_i_mesh)                                       (triangle.rs:16-37, mesh_triangle.rs:47-86)
               n = normalize((1-u-v) n0 + u n1 + v n2) * sign(e1 . (d x e2))                      (triangle.rs:64-113: inv_det's sign)
               an interpolated normal shorter than 1e-3 before the last normalise is UNDEFINED
    uv         (1-u-v) uv0 + u uv1 + v uv2
    texture    wrap (material.rs:86-92), position wrap(uv) . (w, h) - 0.5 in the image, bilinear over the image's own texels, sRGB -> linear per
               texel before filtering, alpha = byte / 255, times the material's factor; a sample whose four taps do not all lie inside the image
               is a BORDER sample (the engines filter over the atlas there and read a neighbouring rectangle, by design); so is one
               within float32's resolution of that
    channels   base colour = factor x texture; roughness = perceptual_roughness^2 x texture.G; metallic = metallic x texture.B
               (material.rs:44-58: the multiplier is (1, roughness, metallic, 1), read back as .zy); emissive = factor.rgb x texture.rgb;
               depth = |origin - point|                                                           (prim_raster.rs)
    motion     screen(camera, p) - screen(prev_camera, prev_M . M^-1 . p) in pixels, zero where v . v < 0.001  (prim_raster.rs:21-27)

Where the reference deviates from the textbook this file restates the reference:
    wrap(t) for t <= 0 is 1 - (-t % 1): an exact integer t <= 0 (0 included) wraps to 1.0, not 0.0; for t > 0 an exact integer wraps to 0.0
    (material.rs:86-92). Everywhere else it is t - floor(t)."""
from dataclasses import dataclass, field

import numpy as np

import walk_ref

UNDEFINED_NORMAL = 1e-3
ATLAS_EXTENT = 8192          # images.rs:28-29: no rectangle lies further out than this
VELOCITY_CUT = 0.001


# ----------------------------------------------------------------------------- the scene as the caller states it
@dataclass
class Scene:
    meshes: dict = field(default_factory=dict)        # handle -> (positions [n,3,3], normals [n,3,3], uvs [n,3,2]) float32
    materials: dict = field(default_factory=dict)     # handle -> strolle_amd.Material
    images: dict = field(default_factory=dict)        # handle -> uint8 [h, w, 4]
    instances: list = field(default_factory=list)     # (handle, mesh, material, xform [3,4] float32, previous xform [3,4] float32), in insertion order


def world_vertices(positions, xform):
    """M . p in float64, rounded to float32"""
    M = np.asarray(xform, np.float32).astype(np.float64).reshape(3, 4)
    p = np.asarray(positions, np.float32).astype(np.float64)
    return (p @ M[:, :3].T + M[:, 3]).astype(np.float32)


def world_normals(normals, xform):
    """normalize(inverse(M3x3)^T . n); a zero normal stays zero"""
    M3 = np.asarray(xform, np.float32).astype(np.float64).reshape(3, 4)[:, :3]
    n = np.asarray(normals, np.float32).astype(np.float64) @ np.linalg.inv(M3)        # (inverse^T . n)^T = n^T . inverse
    ln = np.linalg.norm(n, axis=-1, keepdims=True)
    return np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)


def records(scene: Scene):
    """(p0, e1, e2) float32 of every triangle in slot order (instances in insertion order, each its mesh's triangles), and per slot the instance's index in
    scene.instances and the triangle's index in its mesh"""
    verts, inst, tri = [], [], []
    for i, (_, mesh, _, xform, _) in enumerate(scene.instances):
        v = world_vertices(scene.meshes[mesh][0], xform)
        verts.append(v); inst.append(np.full(len(v), i)); tri.append(np.arange(len(v)))
    v = np.concatenate(verts)
    return (v[:, 0].copy(), (v[:, 1] - v[:, 0]).astype(np.float32), (v[:, 2] - v[:, 0]).astype(np.float32)), np.concatenate(inst), np.concatenate(tri)


# ----------------------------------------------------------------------------- texture
def srgb_to_linear(byte):
    """the exact sRGB curve of a byte"""
    c = np.asarray(byte, np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def wrap(t):
    """material.rs:86-92: `if t > 0.0 { t % 1.0 } else { 1.0 - (-t % 1.0) }` (Rust's % truncates)"""
    t = np.asarray(t, np.float64)
    return np.where(t > 0, np.fmod(t, 1.0), 1.0 - np.fmod(-t, 1.0))


def linear_texels(image):
    """uint8 [h, w, 4] -> float64: RGB through the sRGB curve, alpha = byte / 255"""
    img = np.asarray(image, np.uint8)
    return np.concatenate([srgb_to_linear(img[..., :3]), img[..., 3:].astype(np.float64) / 255.0], axis=-1)


def sample_image(image, uv):
    """(value [n,4], border [n], slope [n]) of the image at hit uvs (before any factor). slope: the largest absolute difference between adjacent texels
    (along x or y, any channel) in the 4 x 4 block around the taps, clamped to the image — the 3 x 3 neighbourhood of each tap."""
    tex = linear_texels(image); h, w = tex.shape[:2]
    uv = np.asarray(uv, np.float64)
    fx, fy = wrap(uv[:, 0]) * w - 0.5, wrap(uv[:, 1]) * h - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0)[:, None], (fy - y0)[:, None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    # float32 places the position within about 2^-24 x (atlas coordinate + |uv| x size) texels; four times that from an edge a tap may fall outside
    guard = 2.0 ** -22 * (ATLAS_EXTENT + np.abs(uv).max(axis=1) * max(w, h))
    border = (fx < guard) | (fy < guard) | (fx > w - 1 - guard) | (fy > h - 1 - guard)
    cx = lambda x: np.clip(x, 0, w - 1)
    cy = lambda y: np.clip(y, 0, h - 1)
    a, b, c, d = tex[cy(y0), cx(x0)], tex[cy(y0), cx(x0 + 1)], tex[cy(y0 + 1), cx(x0)], tex[cy(y0 + 1), cx(x0 + 1)]
    top, bot = a + (b - a) * tx, c + (d - c) * tx
    value = top + (bot - top) * ty
    block = tex[cy(y0[:, None, None] + np.arange(-1, 3)[None, :, None]), cx(x0[:, None, None] + np.arange(-1, 3)[None, None, :])]     # [n, 4, 4, 4]
    slope = np.maximum(np.abs(np.diff(block, axis=1)).max(axis=(1, 2, 3)), np.abs(np.diff(block, axis=2)).max(axis=(1, 2, 3)))
    return value, border, slope


# ----------------------------------------------------------------------------- the surface at a ray's closest hit
@dataclass
class Surface:
    ans: walk_ref.Answer      # hit, t, slot, (u, v), point, margin
    instance: np.ndarray      # index into scene.instances, -1 on a miss
    triangle: np.ndarray      # index into the instance's mesh, -1 on a miss
    normal: np.ndarray        # [n,3]
    undefined: np.ndarray     # the interpolated normal is shorter than 1e-3 (or not finite)
    uv: np.ndarray            # [n,2]
    base_color: np.ndarray    # [n,4]
    emissive: np.ndarray      # [n,3]
    roughness: np.ndarray
    metallic: np.ndarray
    depth: np.ndarray
    border: np.ndarray        # any of the material's texture samples is a border sample
    slope: np.ndarray         # [n,3]: per texture (base colour, metallic-roughness, emissive), 0 where the material has none
    textured: np.ndarray      # [n,3] bool


def surface(scene: Scene, rays) -> Surface:
    (p0, e1, e2), inst_of, tri_of = records(scene)
    ans = walk_ref.trace(p0, e1, e2, rays)
    n = len(rays); hit = ans.hit; slot = np.where(hit, ans.slot, 0)
    u, v = ans.uv[:, 0], ans.uv[:, 1]; w0 = 1.0 - u - v
    nrm, uvs = [], []
    for _, mesh, _, xform, _ in scene.instances:
        nrm.append(world_normals(scene.meshes[mesh][1], xform)); uvs.append(np.asarray(scene.meshes[mesh][2], np.float32).astype(np.float64))
    nrm, uvs = np.concatenate(nrm)[slot], np.concatenate(uvs)[slot]
    raw = w0[:, None] * nrm[:, 0] + u[:, None] * nrm[:, 1] + v[:, None] * nrm[:, 2]
    ln = np.linalg.norm(raw, axis=1)
    undefined = hit & ~(ln >= UNDEFINED_NORMAL)
    d = rays["direction"].astype(np.float64)
    E1, E2 = e1.astype(np.float64)[slot], e2.astype(np.float64)[slot]
    det = np.einsum("ij,ij->i", E1, np.cross(d, E2))
    with np.errstate(all="ignore"):
        normal = raw / ln[:, None] * np.where(det < 0, -1.0, 1.0)[:, None]
    uv = w0[:, None] * uvs[:, 0] + u[:, None] * uvs[:, 1] + v[:, None] * uvs[:, 2]
    base, emis = np.zeros((n, 4)), np.zeros((n, 3)); rough, metal = np.zeros(n), np.zeros(n)
    border = np.zeros(n, bool); slope = np.zeros((n, 3)); textured = np.zeros((n, 3), bool)
    mat_of = np.array([m for _, _, m, _, _ in scene.instances])[inst_of[slot]]
    for handle, m in scene.materials.items():
        rows = np.flatnonzero(hit & (mat_of == handle))
        if not len(rows):
            continue
        out = []
        for k, (tex, factor) in enumerate(((m.base_color_texture, np.asarray(m.base_color, np.float32).astype(np.float64)),
                                           (m.metallic_roughness_texture, np.array([1.0, float(np.float32(m.perceptual_roughness)) ** 2, float(np.float32(m.metallic)), 1.0])),
                                           (m.emissive_texture, np.asarray(m.emissive, np.float32).astype(np.float64)))):
            if tex:
                val, bd, sl = sample_image(scene.images[tex], uv[rows])
                border[rows] |= bd; slope[rows, k] = sl; textured[rows, k] = True
                out.append(factor * val)
            else:
                out.append(np.tile(factor, (len(rows), 1)))
        base[rows] = out[0]; rough[rows] = out[1][:, 1]; metal[rows] = out[1][:, 2]; emis[rows] = out[2][:, :3]
    depth = np.linalg.norm(ans.point - rays["origin"].astype(np.float64), axis=1)
    z = ~hit
    for a in (normal, uv, base, emis, rough, metal, depth):
        a[z] = 0
    return Surface(ans, np.where(hit, inst_of[slot], -1), np.where(hit, tri_of[slot], -1), normal, undefined, uv, base, emis, rough, metal, depth, border, slope, textured)


# ----------------------------------------------------------------------------- motion
def _mat4(a):
    return np.asarray(a, np.float32).astype(np.float64).reshape(4, 4)


def to_screen(camera, points):
    """camera.rs: clip = projection . inverse(transform) . (p, 1); ndc = clip.xy / clip.w, y flipped; (0.5 ndc + 0.5) . size, in pixels"""
    pv = _mat4(camera.projection) @ np.linalg.inv(_mat4(camera.transform))
    clip = np.concatenate([points, np.ones((len(points), 1))], axis=1) @ pv.T
    with np.errstate(all="ignore"):
        ndc = clip[:, :2] / clip[:, 3:4]
    ndc[:, 1] = -ndc[:, 1]
    return (0.5 * ndc + 0.5) * np.asarray(camera.size, np.float64)


def affine4(xform):
    m = np.eye(4); m[:3] = np.asarray(xform, np.float32).astype(np.float64).reshape(3, 4)
    return m


def velocity(scene: Scene, surf: Surface, camera, prev_camera):
    """(velocity [n,2] in pixels, ambiguous [n]): zero where v . v < 0.001; ambiguous where the float64 v . v lies within a factor 2 of 0.001"""
    n = len(surf.instance)
    prev = np.zeros((n, 3))
    for i, (_, _, _, xform, prev_xform) in enumerate(scene.instances):
        rows = surf.instance == i
        back = affine4(prev_xform) @ np.linalg.inv(affine4(xform))
        prev[rows] = surf.ans.point[rows] @ back[:3, :3].T + back[:3, 3]
    vel = to_screen(camera, surf.ans.point) - to_screen(prev_camera, prev)
    vv = np.einsum("ij,ij->i", vel, vel)
    vel[~(vv >= VELOCITY_CUT)] = 0
    vel[~surf.ans.hit] = 0
    return vel, surf.ans.hit & (vv > VELOCITY_CUT / 2) & (vv < VELOCITY_CUT * 2)


# ----------------------------------------------------------------------------- the two G-buffer words (gbuffer.rs:132-164)
def _oct_decode(e):
    """normal.rs: octahedral decode of (x, y) in [0, 1]^2"""
    f = e * 2.0 - 1.0
    n = np.stack([f[:, 0], f[:, 1], 1.0 - np.abs(f[:, 0]) - np.abs(f[:, 1])], 1)
    t = np.clip(-n[:, 2], 0.0, 1.0)
    n[:, 0] += np.where(n[:, 0] >= 0, -t, t); n[:, 1] += np.where(n[:, 1] >= 0, -t, t)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def decode_gbuffer(d0, d1):
    """numpy decode of PRIM_GBUFFER_D0 / D1 ([n,4] float32 each): d0 = (depth, oct normal x, oct normal y, bytes: metallic | roughness | reflectance),
    d1 = (emissive rgb as stored, base colour packed 8/8/8/6 bits gamma 2.2). Returns a dict; `codes` holds the raw integer fields."""
    d0 = np.ascontiguousarray(d0, np.float32); d1 = np.ascontiguousarray(d1, np.float32)
    w = d0[:, 3].copy().view(np.uint32); c = d1[:, 3].copy().view(np.uint32)
    mb, rb, fb = (w & 0xFF), (w >> 8) & 0xFF, (w >> 16) & 0xFF
    col = np.stack([c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF, (c >> 24) & 0x3F], 1).astype(np.float64)
    base = np.concatenate([(col[:, :3] / 255.0) ** 2.2, (col[:, 3:] / 63.0) ** 2.2], 1)
    return dict(depth=d0[:, 0].astype(np.float64), normal=_oct_decode(d0[:, 1:3].astype(np.float64)), metallic=mb / 255.0, roughness=(rb / 255.0) ** 2,
                reflectance=fb / 255.0, emissive=d1[:, :3].astype(np.float64), base_color=base,
                codes=dict(metallic=mb.astype(np.int64), roughness=rb.astype(np.int64), base_color=col.astype(np.int64)))
