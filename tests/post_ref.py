"""numpy restatement of output post-processing (include/strolle_hip.h "post-processing"): the look-ups, the three resampling filters and
FXAA in float32 with the header's order of operations. It is the normative statement: k_post.hip follows it bit for bit in both builds.
Where the prose leaves a choice, the choice is written here: min2(a, b) is a when a < b or b is NaN, else b (max2 likewise with >); an
axis whose fraction is 0 takes the texel itself; resampling positions are evaluated in integers; FXAA's sums are grouped as in fxaa()
below; a tie between the two gradients goes to the negative side (N or W), a tie between the two end distances to the positive end."""
import numpy as np

import display_ref
from ref_num import max2, min2  # noqa: F401  (re-exported)

F = np.float32
NEAREST, BILINEAR, CATMULL_ROM = range(3)
EDGE_THRESHOLD, EDGE_THRESHOLD_MIN, SUBPIXEL = 0.166, 0.0833, 0.75
WALK = (1.0, 2.0, 3.0, 4.0, 5.0, 6.5, 8.5, 10.5, 12.5, 14.5, 18.5, 26.5)   # steps of 1 1 1 1 1 1.5 2 2 2 2 4 8 pixels


def axis_float(p):
    """continuous positions (float32) -> (i0, f): the texels i0, i0 + 1 and the blend fraction"""
    q = np.asarray(p, np.float32) - F(0.5)
    i0 = np.floor(q)
    return i0.astype(np.int64), (q - i0).astype(np.float32)


def axis_resample(n_src: int, n_dst: int):
    """output indices 0..n_dst-1 -> (i0, f, nearest) at the source position (o + 0.5) n_src / n_dst, evaluated in integers"""
    o = np.arange(n_dst, dtype=np.int64)
    n, d = (2 * o + 1) * n_src - n_dst, 2 * n_dst
    i0 = n // d
    f = (n - i0 * d).astype(np.float32) / F(d)
    return i0, f.astype(np.float32), ((2 * o + 1) * n_src) // d


def _blend(a, b, f):
    return np.where(f == 0, a, a + (b - a) * f).astype(np.float32)


def bilinear(img, ix, fx, iy, fy):
    """img (H, W, C) or (H, W); ix, fx, iy, fy broadcast against each other: x first, then y"""
    img = np.asarray(img, np.float32)
    h, w = img.shape[:2]
    ix, fx, iy, fy = np.broadcast_arrays(ix, fx, iy, fy)
    x0, x1, y0, y1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1), np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    if img.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    with np.errstate(all="ignore"):
        top = _blend(img[y0, x0], img[y0, x1], fx)
        bot = _blend(img[y1, x0], img[y1, x1], fx)
        return _blend(top, bot, fy)


def catmull_rom_weights(f):
    f = np.asarray(f, np.float32)
    w0 = ((F(-0.5) * f + F(1)) * f - F(0.5)) * f
    w1 = ((F(1.5) * f - F(2.5)) * f) * f + F(1)
    w2 = ((F(-1.5) * f + F(2)) * f + F(0.5)) * f
    w3 = ((F(0.5) * f - F(0.5)) * f) * f
    return w0, w1, w2, w3


def _cr_axis(t, f):
    w0, w1, w2, w3 = catmull_rom_weights(f)
    return np.where(f == 0, t[1], ((t[0] * w0 + t[1] * w1) + t[2] * w2) + t[3] * w3).astype(np.float32)


def catmull_rom(img, ix, fx, iy, fy):
    img = np.asarray(img, np.float32)
    h, w = img.shape[:2]
    ix, fx, iy, fy = np.broadcast_arrays(ix, fx, iy, fy)
    xs = [np.clip(ix + k, 0, w - 1) for k in (-1, 0, 1, 2)]
    ys = [np.clip(iy + k, 0, h - 1) for k in (-1, 0, 1, 2)]
    fxe, fye = fx[..., None], fy[..., None]
    with np.errstate(all="ignore"):
        rows = [_cr_axis([img[y, x] for x in xs], fxe) for y in ys]
        v = _cr_axis(rows, fye)
        inner = [img[ys[1], xs[1]], img[ys[1], xs[2]], img[ys[2], xs[1]], img[ys[2], xs[2]]]
        lo = min2(min2(min2(inner[0], inner[1]), inner[2]), inner[3])
        hi = max2(max2(max2(inner[0], inner[1]), inner[2]), inner[3])
        return np.where((fxe == 0) & (fye == 0), inner[0], min2(max2(v, lo), hi)).astype(np.float32)   # on a texel: the texel, NaN included


def _rgb1(rgb):
    return np.concatenate([rgb.astype(np.float32), np.ones(rgb.shape[:-1] + (1,), np.float32)], -1)


def resample(img, out_w: int, out_h: int, flt: int) -> np.ndarray:
    """(H, W, 3 or 4) -> (out_h, out_w, 4) float32, alpha 1"""
    rgb = np.asarray(img, np.float32)[..., :3]
    h, w = rgb.shape[:2]
    ix, fx, nx = axis_resample(w, out_w)
    iy, fy, ny = axis_resample(h, out_h)
    if flt == NEAREST:
        return _rgb1(rgb[ny[:, None], nx[None, :]])
    fn = bilinear if flt == BILINEAR else catmull_rom
    return _rgb1(fn(rgb, ix[None, :], fx[None, :], iy[:, None], fy[:, None]))


def luma(img) -> np.ndarray:
    c = np.asarray(img, np.float32)[..., :3]
    with np.errstate(all="ignore"):
        c = np.where(c > 0, np.where(c < 1, c, F(1)), F(0)).astype(np.float32)
        return np.sqrt(display_ref.luma(c[..., 0], c[..., 1], c[..., 2])).astype(np.float32)


def fxaa(img, edge_threshold: float = 0.0, edge_threshold_min: float = 0.0, subpixel: float = SUBPIXEL, details=None) -> np.ndarray:
    """(H, W, 3 or 4) display-referred colour -> (H, W, 4) float32, alpha 1. Thresholds of 0 mean the defaults. `details` (a dict) receives the
    intermediate planes."""
    rgb = np.asarray(img, np.float32)[..., :3]
    h, w = rgb.shape[:2]
    t = F(edge_threshold if edge_threshold != 0 else EDGE_THRESHOLD)
    tmin = F(edge_threshold_min if edge_threshold_min != 0 else EDGE_THRESHOLD_MIN)
    L = luma(rgb)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")

    def at(dy, dx):
        return L[np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)]

    M, N, S, E, W = at(0, 0), at(-1, 0), at(1, 0), at(0, 1), at(0, -1)
    NW, NE, SW, SE = at(-1, -1), at(-1, 1), at(1, -1), at(1, 1)
    two = F(2)
    with np.errstate(all="ignore"):
        mx = np.maximum(np.maximum(np.maximum(N, W), np.maximum(S, M)), E)
        mn = np.minimum(np.minimum(np.minimum(N, W), np.minimum(S, M)), E)
        rng = mx - mn
        edge = ~(rng < np.maximum(tmin, mx * t))
        eh = np.abs((NW + SW) - two * W) + two * np.abs((N + S) - two * M) + np.abs((NE + SE) - two * E)
        ev = np.abs((NW + NE) - two * N) + two * np.abs((W + E) - two * M) + np.abs((SW + SE) - two * S)
        horz = eh >= ev
        neg, pos = np.where(horz, N, W), np.where(horz, S, E)
        gn, gp = np.abs(neg - M), np.abs(pos - M)
        pick_n = gn >= gp
        gs = F(0.25) * np.where(pick_n, gn, gp)
        A = F(0.5) * (np.where(pick_n, neg, pos) + M)
        cx, cy = xs.astype(np.float32) + F(0.5), ys.astype(np.float32) + F(0.5)
        half = np.where(pick_n, F(-0.5), F(0.5)).astype(np.float32)
        px, py = np.where(horz, cx, cx + half).astype(np.float32), np.where(horz, cy + half, cy).astype(np.float32)
        dist = [np.full((h, w), WALK[-1], np.float32) for _ in range(2)]
        delta = [np.zeros((h, w), np.float32) for _ in range(2)]
        done = [np.zeros((h, w), bool) for _ in range(2)]
        for d in WALK:
            for side, sign in ((0, F(-1)), (1, F(1))):
                qx, qy = np.where(horz, px + sign * F(d), px).astype(np.float32), np.where(horz, py, py + sign * F(d)).astype(np.float32)
                ix, fx = axis_float(qx)
                iy, fy = axis_float(qy)
                dl = bilinear(L, ix, fx, iy, fy) - A
                live = ~done[side]
                delta[side] = np.where(live, dl, delta[side]).astype(np.float32)
                dist[side] = np.where(live, F(d), dist[side]).astype(np.float32)
                done[side] = done[side] | (np.abs(dl) >= gs)
        near_n = dist[0] < dist[1]
        off_edge = F(0.5) - np.where(near_n, dist[0], dist[1]) / (dist[0] + dist[1])
        good = (np.where(near_n, delta[0], delta[1]) < 0) != ((M - A) < 0)
        off_edge = np.where(good, off_edge, F(0)).astype(np.float32)
        a = np.abs((((N + S) + (E + W)) * two + ((NW + NE) + (SW + SE))) / F(12) - M) / rng
        a = np.where(a < 1, a, F(1)).astype(np.float32)
        s = ((F(-2) * a + F(3)) * a) * a
        off_sub = (s * s) * F(subpixel)
        off = np.where(off_edge > off_sub, off_edge, off_sub).astype(np.float32)
        signed = np.where(pick_n, -off, off).astype(np.float32)
        ix, fx = axis_float(np.where(horz, cx, cx + signed))
        iy, fy = axis_float(np.where(horz, cy + signed, cy))
        moved = bilinear(rgb, ix, fx, iy, fy)
    if details is not None:
        details.update(luma=L, edge=edge, horizontal=horz, pick_negative=pick_n, distance_negative=dist[0], distance_positive=dist[1],
                       offset_edge=off_edge, offset_sub=off_sub, offset=off, good=good)
    return _rgb1(np.where(edge[..., None], moved, rgb))


def process(img, fxaa_on: bool = False, out_size=None, flt: int = BILINEAR, edge_threshold: float = 0.0, edge_threshold_min: float = 0.0,
            subpixel: float = SUBPIXEL) -> np.ndarray:
    """what st_post_process / a camera's post-processing computes from an RGBA32F image, before the output format: (OH, OW, 4) float32"""
    x = np.asarray(img, np.float32)
    h, w = x.shape[:2]
    x = fxaa(x, edge_threshold, edge_threshold_min, subpixel) if fxaa_on else _rgb1(x[..., :3])
    ow, oh = out_size if out_size else (w, h)
    return x if (ow, oh) == (w, h) else resample(x, ow, oh, flt)


def to_format(img, fmt: int) -> np.ndarray:
    """RGBA32F as it is, RGBA16F round to nearest even, the 8-bit formats through display_ref.srgb8 (h, w, 4 bytes in memory order)"""
    img = np.asarray(img, np.float32)
    if fmt == 0:
        return img
    if fmt == 1:
        with np.errstate(all="ignore"):
            return img.astype(np.float16)
    rgb = display_ref.srgb8(img[..., :3]).astype(np.uint8)
    if fmt == 3:
        rgb = rgb[..., ::-1]
    return np.concatenate([rgb, np.full(rgb.shape[:-1] + (1,), 255, np.uint8)], -1)


def half_plane(w: int, h: int, slope: float, offset: float):
    """(point-sampled 0 / 1 image, analytic pixel coverage) of the half-plane y > offset + slope x, both (h, w) float64"""
    ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    sampled = (ys > offset + slope * xs).astype(np.float64)
    n = 64   # coverage: the exact integral along x of the clipped column height, by n-point midpoint rule in x (the edge is linear in x)
    cov = np.zeros((h, w))
    for k in range(n):
        x = xs - 0.5 + (k + 0.5) / n
        cov += np.clip((ys + 0.5) - (offset + slope * x), 0.0, 1.0)
    return sampled, cov / n
