"""Normal mapping (include/strolle_hip.h "normal mapping") twice over:

map_f64   the DEFINITION, in float64, from what the caller handed to the API (surface_ref.Scene and surface_ref.surface: mesh arrays, transforms,
          Material fields, image bytes). No read_scene record and no atlas rectangle: the bake and the atlas placement are under test, not trusted.
map_f32   the RESTATEMENT of st_traverse.h normal_map_apply: the same float32 operations in the same order, from what the engine itself reports — the
          unmapped normal and uv of a hit, the world records and uv corners of read_scene(1), the material's rectangle of read_scene(3), the atlas
          as the rectangles place the image bytes. A HIP build owes it every bit.

    nf = s n                                      s = sign of 1 / det: the flip that made n face the ray
    (du1, dv1) = uv1 - uv0   (du2, dv2) = uv2 - uv0   d = du1 dv2 - du2 dv1
    Pu = (e1 dv2 - e2 dv1) / d                    Pv = (e2 du1 - e1 du2) / d
    T  = normalize(Pu - nf (nf . Pu))             C = nf x T
    h  = (C . Pv <= 0) ? +1 : -1                  B = h C
    m  = bilinear texel at uv, byte / 255 (never the sRGB curve)
    t  = (2 m.x - 1, 2 m.y - 1, max(2 m.z - 1, 0))
    n' = s normalize(t.x T + t.y B + t.z nf)
    n' = n, bit for bit, without a map and where |d| lies outside [TINY, FLT_MAX] or |Pu - nf (nf . Pu)| or the last length outside [SHORT, LONG]."""
from dataclasses import dataclass

import numpy as np

import surface_ref as sr

TINY, SHORT, LONG = 1e-30, 1e-18, 1e18     # kNormalMapTiny, kNormalMapShort, kNormalMapLong
F32_MAX = float(np.float32(3.4028235e38))
HANDEDNESS_AMBIGUOUS = 1e-3   # |cos| between C and Pv below which float32 may decide h the other way
F = np.float32


# ----------------------------------------------------------------------------- the restatement (float32; st_traverse.h normal_map_apply)
def _dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross32(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0], a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1)


def _det_usable(d):
    with np.errstate(invalid="ignore"):
        return (np.abs(d) >= F(TINY)) & (np.abs(d) <= F(F32_MAX))


def _length_usable(l):
    with np.errstate(invalid="ignore"):
        return (l >= F(SHORT)) & (l <= F(LONG))


def _wrap32(t):
    """st_device.h mat_wrap"""
    frac = lambda x: x - np.floor(x)
    with np.errstate(invalid="ignore"):
        return np.where(t > 0, frac(t), F(1.0) - frac(-t)).astype(F)


def sample_map_f32(atlas, rect, uv):
    """st_device.h sample_normal_map: atlas uint8 [H, W, 4]; rect float32 [n, 4] (x, y, w, h as fractions of the atlas); uv float32 [n, 2].
    Returns (m float32 [n, 3], taps int64 [n, 4] = x0, y0, x0 + 1, y0 + 1 before the clamp)."""
    ah, aw = atlas.shape[:2]
    uv = np.asarray(uv, F); rect = np.asarray(rect, F)
    with np.errstate(all="ignore"):
        ux = rect[:, 0] + _wrap32(uv[:, 0]) * rect[:, 2]
        uy = rect[:, 1] + _wrap32(uv[:, 1]) * rect[:, 3]
        ux = np.where(np.isnan(ux), F(0), ux); uy = np.where(np.isnan(uy), F(0), uy)
        fx = ux * F(aw) - F(0.5); fy = uy * F(ah) - F(0.5)
        x0, y0 = np.floor(fx), np.floor(fy)
        tx, ty = (fx - x0)[:, None], (fy - y0)[:, None]
        ix = np.clip(x0, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64); iy = np.clip(y0, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)
    lut = (np.arange(256, dtype=F) / F(255.0)).astype(F)                             # unorm8_eval
    tex = lambda x, y: lut[atlas[np.clip(y, 0, ah - 1), np.clip(x, 0, aw - 1), :3]]
    p00, p10, p01, p11 = tex(ix, iy), tex(ix + 1, iy), tex(ix, iy + 1), tex(ix + 1, iy + 1)
    top = p00 + (p10 - p00) * tx
    bot = p01 + (p11 - p01) * tx
    return (top + (bot - top) * ty).astype(F), np.stack([ix, iy, ix + 1, iy + 1], 1)


def map_f32(n, s, uv, e1, e2, uv0, uv1, uv2, rect, atlas):
    """Per hit, all float32: n [k,3] the unmapped normal, s [k] = +-1, uv [k,2], e1 / e2 [k,3], uv0..2 [k,2], rect [k,4] (all zero: no map), atlas uint8
    [H,W,4]. Returns (n' float32 [k,3], mapped bool [k]: the map changed the answer's definition (n' is not n by rule), taps [k,4])."""
    n, uv, e1, e2, uv0, uv1, uv2, rect = (np.ascontiguousarray(a, F) for a in (n, uv, e1, e2, uv0, uv1, uv2, rect))
    s = np.asarray(s, F)[:, None]
    k = len(n)
    has_map = np.any(rect != 0, axis=1)
    with np.errstate(all="ignore"):
        nf = n * s
        du1, dv1 = (uv1[:, 0] - uv0[:, 0])[:, None], (uv1[:, 1] - uv0[:, 1])[:, None]
        du2, dv2 = (uv2[:, 0] - uv0[:, 0])[:, None], (uv2[:, 1] - uv0[:, 1])[:, None]
        d = du1 * dv2 - du2 * dv1
        ok = has_map & _det_usable(d[:, 0])
        pu = (e1 * dv2 - e2 * dv1) / d
        pv = (e2 * du1 - e1 * du2) / d
        q = pu - nf * _dot32(nf, pu)[:, None]
        l = np.sqrt(_dot32(q, q))
        ok &= _length_usable(l)
        T = q * (F(1.0) / l)[:, None]
        C = _cross32(nf, T)
        B = C * np.where(_dot32(C, pv) <= 0, F(1.0), F(-1.0))[:, None]
        m, taps = sample_map_f32(atlas, rect, uv) if has_map.any() else (np.zeros((k, 3), F), np.zeros((k, 4), np.int64))
        tx, ty, tz = F(2.0) * m[:, 0] - F(1.0), F(2.0) * m[:, 1] - F(1.0), np.maximum(F(2.0) * m[:, 2] - F(1.0), F(0.0))
        w = (T * tx[:, None] + B * ty[:, None]) + nf * tz[:, None]
        kk = np.sqrt(_dot32(w, w))
        ok &= _length_usable(kk)
        out = (w * (F(1.0) / kk)[:, None]) * s
    out = np.where(ok[:, None], out, n).astype(F)
    assert out.dtype == F
    return out, ok, taps


def ray_sign(direction, e1, e2):
    """s = copysign(1, 1 / det) with det = e1 . (d x e2) as Triangle::hit forms it in float32 (st_traverse.h traverse)"""
    d, e1, e2 = (np.asarray(a, F) for a in (direction, e1, e2))
    det = _dot32(e1, _cross32(d, e2))
    return np.where(np.signbit(det), F(-1.0), F(1.0))


def build_atlas(images, rects, height):
    """the atlas as the rectangles (x, y, w, h in texels; Engine.image_rect) place the image bytes; everything else zero"""
    atlas = np.zeros((height, sr.ATLAS_EXTENT, 4), np.uint8)
    for h, px in images.items():
        x, y, w, hh = rects[h]
        atlas[y:y + hh, x:x + w] = px
    return atlas


# ----------------------------------------------------------------------------- the definition (float64; from the arrays handed to the API)
@dataclass
class Mapped:
    normal: np.ndarray         # [n,3]: n' (n itself where nothing is mapped)
    mapped: np.ndarray         # the hit's material has a map and no degeneracy rule applies
    border: np.ndarray         # a tap outside the image (the engines filter over the atlas there), or within float32's resolution of that
    near_degenerate: np.ndarray  # d, |q| or the last length within a factor 2 of TINY (or not finite); or h decided by a cosine below HANDEDNESS_AMBIGUOUS
    slope: np.ndarray          # radians of n' per texel of sample position: 2 x the map's largest adjacent-texel difference around the taps / |t|
    sign: np.ndarray           # s


def sample_map_f64(image, uv):
    """(m [n,3], border [n], slope [n]) — surface_ref.sample_image with the bytes decoded as byte / 255"""
    tex = np.asarray(image, np.uint8)[..., :3].astype(np.float64) / 255.0
    h, w = tex.shape[:2]
    uv = np.asarray(uv, np.float64)
    fx, fy = sr.wrap(uv[:, 0]) * w - 0.5, sr.wrap(uv[:, 1]) * h - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0)[:, None], (fy - y0)[:, None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    guard = 2.0 ** -22 * (sr.ATLAS_EXTENT + np.abs(uv).max(axis=1) * max(w, h))
    border = (fx < guard) | (fy < guard) | (fx > w - 1 - guard) | (fy > h - 1 - guard)
    cx = lambda x: np.clip(x, 0, w - 1)
    cy = lambda y: np.clip(y, 0, h - 1)
    a, b, c, d = tex[cy(y0), cx(x0)], tex[cy(y0), cx(x0 + 1)], tex[cy(y0 + 1), cx(x0)], tex[cy(y0 + 1), cx(x0 + 1)]
    top, bot = a + (b - a) * tx, c + (d - c) * tx
    block = tex[cy(y0[:, None, None] + np.arange(-1, 3)[None, :, None]), cx(x0[:, None, None] + np.arange(-1, 3)[None, None, :])]
    slope = np.maximum(np.abs(np.diff(block, axis=1)).max(axis=(1, 2, 3)), np.abs(np.diff(block, axis=2)).max(axis=(1, 2, 3)))
    return top + (bot - top) * ty, border, slope


def map_f64(scene: sr.Scene, surf: sr.Surface, rays) -> Mapped:
    """the mapped normal of every ray's closest hit (surf = surface_ref.surface(scene, rays))"""
    n = len(rays)
    hit = surf.ans.hit; slot = np.where(hit, surf.ans.slot, 0)
    (_, e1, e2), inst_of, _ = sr.records(scene)
    E1, E2 = e1.astype(np.float64)[slot], e2.astype(np.float64)[slot]
    uvs = np.concatenate([np.asarray(scene.meshes[mesh][2], np.float32).astype(np.float64) for _, mesh, _, _, _ in scene.instances])[slot]
    det = np.einsum("ij,ij->i", E1, np.cross(rays["direction"].astype(np.float64), E2))
    s = np.where(det < 0, -1.0, 1.0)
    out = surf.normal.copy()
    mapped = np.zeros(n, bool); border = np.zeros(n, bool); near = np.zeros(n, bool); slope = np.zeros(n)
    mat_of = np.array([m for _, _, m, _, _ in scene.instances])[inst_of[slot]]
    for handle, mat in scene.materials.items():
        rows = np.flatnonzero(hit & (mat_of == handle))
        if not len(rows) or not mat.normal_map_texture:
            continue
        nf = surf.normal[rows] * s[rows, None]
        d1, d2 = uvs[rows, 1] - uvs[rows, 0], uvs[rows, 2] - uvs[rows, 0]
        with np.errstate(all="ignore"):
            d = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
            pu = (E1[rows] * d2[:, 1:2] - E2[rows] * d1[:, 1:2]) / d[:, None]
            pv = (E2[rows] * d1[:, 0:1] - E1[rows] * d2[:, 0:1]) / d[:, None]
            q = pu - nf * np.einsum("ij,ij->i", nf, pu)[:, None]
            l = np.linalg.norm(q, axis=1)
            T = q / l[:, None]
            C = np.cross(nf, T)
            cpv = np.einsum("ij,ij->i", C, pv)
            B = C * np.where(cpv <= 0, 1.0, -1.0)[:, None]
            m, bd, sl = sample_map_f64(scene.images[mat.normal_map_texture], surf.uv[rows])
            t = np.stack([2 * m[:, 0] - 1, 2 * m[:, 1] - 1, np.maximum(2 * m[:, 2] - 1, 0.0)], 1)
            w = T * t[:, 0:1] + B * t[:, 1:2] + nf * t[:, 2:3]
            k = np.linalg.norm(w, axis=1)
            det_ok = lambda x, f: np.isfinite(x) & (np.abs(x) >= TINY * f) & (np.abs(x) <= F32_MAX / f)
            len_ok = lambda x, f: np.isfinite(x) & (x >= SHORT * f) & (x <= LONG / f)
            ok = det_ok(d, 1) & len_ok(l, 1) & len_ok(k, 1)
            cosine = np.abs(cpv) / (np.linalg.norm(C, axis=1) * np.linalg.norm(pv, axis=1))
            # within a factor 2 of a threshold on either side, a handedness float32 may decide the other way, or a quotient e / d near float32's range
            big = np.maximum(np.abs(pu).max(axis=1), np.abs(pv).max(axis=1))
            near[rows] = ok & (~det_ok(d, 2) | ~len_ok(l, 2) | ~len_ok(k, 2) | ~(cosine >= HANDEDNESS_AMBIGUOUS) | ~(big <= F32_MAX / 2))
            near[rows] |= ~ok & det_ok(d, 0.5) & len_ok(l, 0.5) & len_ok(k, 0.5)
            out[rows] = np.where(ok[:, None], (w / k[:, None]) * s[rows, None], surf.normal[rows])
            slope[rows] = np.where(ok, 2.0 * sl / np.maximum(k, TINY), 0.0)
        mapped[rows] = ok; border[rows] = bd
    return Mapped(out, mapped, border, near, slope, s)
