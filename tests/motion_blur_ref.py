"""Numpy restatement of include/strolle_hip.h "motion blur": pack, the tile maximum, the neighbour maximum and the gather. Everything is
float32, evaluated in the header's order; min, max and clamp01 follow the post-processing section's NaN rule."""
import numpy as np

from ref_num import COLOUR_CLAMP, FLT_MAX, clamp01, colour, frame_depth, max2, min2  # noqa: F401  (re-exported)

F = np.float32
NO_JITTER = 1
TILE, DEFAULT_SAMPLES, DEFAULT_RADIUS, DEFAULT_SOFTNESS = 32, 8, 32.0, 0.05
BAYER = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], np.float32)


def resolve(samples=0, max_radius=0.0, depth_softness=0.0):
    """the descriptor's defaults applied: (S, R, e_s)"""
    return (int(samples) or DEFAULT_SAMPLES, F(max_radius) if F(max_radius) != 0 else F(DEFAULT_RADIUS),
            F(depth_softness) if F(depth_softness) != 0 else F(DEFAULT_SOFTNESS))


def pack(velocity, shutter, max_radius=0.0):
    """(h, w, 2) velocities -> (v (h, w, 2), r (h, w))"""
    R = resolve(max_radius=max_radius)[1]
    V = np.asarray(velocity, np.float32)
    with np.errstate(all="ignore"):
        h = F(0.5) * F(shutter)
        vx, vy = V[..., 0] * h, V[..., 1] * h
        r = np.sqrt(vx * vx + vy * vy).astype(np.float32)
        rest = ~(r >= F(0.5))
        over = ~rest & (r > R)
        k = R / np.where(over, r, F(1))
        vx = np.where(rest, F(0), np.where(over, vx * k, vx)).astype(np.float32)
        vy = np.where(rest, F(0), np.where(over, vy * k, vy)).astype(np.float32)
        r = np.where(rest, F(0), np.where(over, R, r)).astype(np.float32)
    return np.stack([vx, vy], -1), r


def tile_max(v, r):
    """(ty, tx, 3): (v.x, v.y, r) of each tile's pixel with the largest r, the first in row-major order among equals"""
    h, w = r.shape
    ty, tx = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
    out = np.zeros((ty, tx, 3), np.float32)
    for j in range(ty):
        for i in range(tx):
            rr = r[j * TILE:(j + 1) * TILE, i * TILE:(i + 1) * TILE]
            y, x = np.unravel_index(int(np.argmax(rr)), rr.shape)   # argmax: the first occurrence in row-major order
            out[j, i] = (*v[j * TILE + y, i * TILE + x], rr[y, x])
    return out


def neighbour_max(tiles):
    ty, tx = tiles.shape[:2]
    out = np.zeros_like(tiles)
    for j in range(ty):
        for i in range(tx):
            best = None
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    y, x = j + dy, i + dx
                    if 0 <= y < ty and 0 <= x < tx and (best is None or tiles[y, x, 2] > best[2]):
                        best = tiles[y, x]
            out[j, i] = best
    return out


def jitter(w, h, flags=0):
    if flags & NO_JITTER:
        return np.zeros((h, w), np.float32)
    b = BAYER[np.arange(h)[:, None] & 3, np.arange(w)[None, :] & 3]
    return ((b + F(0.5)) / F(16) - F(0.5)).astype(np.float32)


def cone(d, r):
    with np.errstate(all="ignore"):
        return np.where(r > 0, clamp01(F(1) - d / np.where(r > 0, r, F(1))), F(0)).astype(np.float32)


def cyl(d, r):
    with np.errstate(all="ignore"):
        rs = np.where(r > 0, r, F(1)).astype(np.float32)
        q = clamp01((d - F(0.95) * rs) / (F(1.05) * rs - F(0.95) * rs))
        return np.where(r > 0, F(1) - q * q * (F(3) - F(2) * q), F(0)).astype(np.float32)


def gather(color, r, z, nb, samples=0, depth_softness=0.0, flags=0, details=None):
    """color (h, w, 3 or 4), packed r and Z (h, w), nb = neighbour_max(...) -> (h, w, 4): the blurred colour, or C(X) itself where the
    tile is at rest"""
    C = np.asarray(color, np.float32)
    h, w = r.shape
    S, _, es = resolve(samples, 0.0, depth_softness)
    n = np.repeat(np.repeat(nb, TILE, 0), TILE, 1)[:h, :w]
    nx, ny, rn = n[..., 0], n[..., 1], n[..., 2]
    j = jitter(w, h, flags)
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    fx, fy = x + F(0.5), y + F(0.5)
    with np.errstate(all="ignore"):
        w0 = F(1) / max2(r, F(0.5))
        c0 = colour(C)
        acc = c0 * w0[..., None]
        wsum = w0.copy()
        taps = []
        for i in range(S):
            t = ((F(i) + F(0.5) + j) * F(2)) / F(S) - F(1)
            px, py = fx + nx * t, fy + ny * t
            yx = min2(max2(np.floor(px), F(0)), F(w - 1)).astype(np.int64)
            yy = min2(max2(np.floor(py), F(0)), F(h - 1)).astype(np.int64)
            ry, zy = r[yy, yx], z[yy, yx]
            d = np.abs(t) * rn
            e = max2(es * min2(z, zy), F(1e-6))
            f = clamp01(F(1) - (zy - z) / e)
            b = clamp01(F(1) - (z - zy) / e)
            wt = (f * cone(d, ry) + b * cone(d, r)) + (cyl(d, ry) * cyl(d, r)) * F(2)
            acc = acc + c0[yy, yx] * wt[..., None]
            wsum = wsum + wt
            taps.append((yx, yy, wt))
        res = acc / wsum[..., None]
    if details is not None:
        details["taps"] = taps
        details["wsum"] = wsum
    out = np.concatenate([res, np.ones((h, w, 1), np.float32)], -1).astype(np.float32)
    rest = rn < F(0.5)
    src = C if C.shape[-1] == 4 else np.concatenate([C, np.ones((h, w, 1), np.float32)], -1)
    out[rest] = src[rest]
    return out


def motion_blur(color, velocity, depth, shutter=0.5, samples=0, max_radius=0.0, depth_softness=0.0, flags=0, details=None):
    """(h, w, 4) composed colours, (h, w, 2) velocities, (h, w) depths -> (h, w, 4) in front of bloom / the display transform"""
    v, r = pack(velocity, shutter, max_radius)
    tiles = tile_max(v, r)
    nb = neighbour_max(tiles)
    if details is not None:
        details.update(v=v, r=r, tiles=tiles, neighbours=nb)
    return gather(color, r, np.asarray(depth, np.float32), nb, samples, depth_softness, flags, details)
