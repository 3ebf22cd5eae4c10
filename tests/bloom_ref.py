"""Numpy restatement of include/strolle_hip.h "bloom": the plan (level count, mip sizes, blend factors), the prefilter, the 13-tap
downsample, the 3 x 3 tent upsample, the chain and the composite. Everything that touches colour is float32, evaluated in the header's
order; the blend factors are host arithmetic in double and are passed in (a test feeds what st_bloom_plan reports, or `factors` below)."""
import numpy as np

from ref_num import max2, min2  # noqa: F401  (re-exported)

F = np.float32
ADDITIVE, FIREFLY_SUPPRESS = 1, 2
DEFAULT_LEVELS, MAX_LEVELS, DEFAULT_CLAMP = 6, 8, 65504.0
GROUP_WEIGHTS = (0.125, 0.125, 0.125, 0.125, 0.5)
TENT = ((0.0625, 0.125, 0.0625), (0.125, 0.25, 0.125), (0.0625, 0.125, 0.0625))


def luma(c):
    return F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1] + F(0.0722) * c[..., 2]


def plan_sizes(width: int, height: int, levels: int = 0):
    """[(w, h)] of the mips: the requested count (0 = 6) reduced so that the last mip has both sides >= 2"""
    out, w, h = [], width, height
    for _ in range(levels or DEFAULT_LEVELS):
        w, h = (w + 1) // 2, (h + 1) // 2
        if w < 2 or h < 2:
            break
        out.append((w, h))
    return out


def factors(levels: int, intensity, low_frequency_boost, curvature, high_pass_frequency, additive: bool) -> np.ndarray:
    """the blend factor of each of `levels` (effective) levels: double arithmetic on the float32 fields, rounded to float32"""
    intensity, boost, curvature, f = (float(F(v)) for v in (intensity, low_frequency_boost, curvature, high_pass_frequency))
    x = np.arange(levels, dtype=np.float64) / max(levels - 1, 1)
    lf = (1.0 - np.power(1.0 - x, 1.0 / (1.0 - curvature))) * boost
    if not additive:
        lf = lf * (1.0 - intensity)
    hp = 1.0 - np.clip((x - f) / f, 0.0, 1.0)
    return ((intensity + lf) * hp).astype(np.float32)


def prefilter(rgb, clamp: float = 0.0, threshold: float = 0.0, softness: float = 0.0) -> np.ndarray:
    rgb = np.asarray(rgb, np.float32)[..., :3]
    with np.errstate(all="ignore"):
        c = min2(max2(rgb, F(0)), F(clamp if clamp else DEFAULT_CLAMP))
        if F(threshold) > 0:
            t = F(threshold)
            knee = t * F(softness)
            lo, k2, div = F(t - knee), F(F(2) * knee), F(F(4) * knee + F(1e-4))
            m = max2(max2(c[..., 0], c[..., 1]), c[..., 2])
            s = min2(max2(m - lo, F(0)), k2)
            s = (s * s) / div
            w = max2(m - t, s) / max2(m, F(1e-4))
            c = c * w[..., None]
    return c.astype(np.float32)


def _texels(img, ys, xs):
    h, w = img.shape[:2]
    return img[np.clip(ys, 0, h - 1)[:, None], np.clip(xs, 0, w - 1)[None, :]]


def downsample(src, firefly: bool = False) -> np.ndarray:
    """(h, w, 3) -> (ceil(h / 2), ceil(w / 2), 3); `src` is already prefiltered where the header says P(t)"""
    src = np.asarray(src, np.float32)
    h, w = src.shape[:2]
    ys, xs = 2 * np.arange((h + 1) // 2), 2 * np.arange((w + 1) // 2)
    q = F(0.25)

    def S(dx, dy):
        return ((_texels(src, ys + dy, xs + dx) + _texels(src, ys + dy, xs + dx + 1))
                + (_texels(src, ys + dy + 1, xs + dx) + _texels(src, ys + dy + 1, xs + dx + 1))) * q

    with np.errstate(all="ignore"):
        a, b, c = S(-2, -2), S(0, -2), S(2, -2)
        d, e, f = S(-2, 0), S(0, 0), S(2, 0)
        g, hh, i = S(-2, 2), S(0, 2), S(2, 2)
        j, k, l, m = S(-1, -1), S(1, -1), S(-1, 1), S(1, 1)
        groups = [(((a + b) + d) + e) * q, (((b + c) + e) + f) * q, (((d + e) + g) + hh) * q, (((e + f) + hh) + i) * q, (((j + k) + l) + m) * q]
        ws = [np.full(groups[0].shape[:2], F(x), np.float32) for x in GROUP_WEIGHTS]
        if firefly:
            ws = [x * (F(1) / (F(1) + luma(gr))) for x, gr in zip(ws, groups)]
        r = groups[0] * ws[0][..., None] + groups[1] * ws[1][..., None]
        for gr, x in zip(groups[2:], ws[2:]):
            r = r + gr * x[..., None]
        if firefly:
            r = r / ((((ws[0] + ws[1]) + ws[2]) + ws[3]) + ws[4])[..., None]
    return r.astype(np.float32)


def upsample(src, out_w: int, out_h: int) -> np.ndarray:
    """the 3 x 3 tent of bilinear look-ups: (h, w, 3) -> (out_h, out_w, 3)"""
    src = np.asarray(src, np.float32)

    def axis(n):
        x = np.arange(n)
        return (x + 1) // 2 - 1, np.where(x % 2 == 1, F(0.25), F(0.75)).astype(np.float32)

    (ix, fx), (iy, fy) = axis(out_w), axis(out_h)
    fx, fy = fx[None, :, None], fy[:, None, None]

    def B(ox, oy):
        t00, t10 = _texels(src, iy + oy, ix + ox), _texels(src, iy + oy, ix + ox + 1)
        t01, t11 = _texels(src, iy + oy + 1, ix + ox), _texels(src, iy + oy + 1, ix + ox + 1)
        top, bot = t00 + (t10 - t00) * fx, t01 + (t11 - t01) * fx
        return top + (bot - top) * fy

    with np.errstate(all="ignore"):
        u = None
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                term = B(ox, oy) * F(TENT[oy + 1][ox + 1])
                u = term if u is None else u + term
    return u.astype(np.float32)


def _blend(base, up, b, additive):
    b = F(b)
    with np.errstate(all="ignore"):
        return (base + up * b if additive else base * (F(1) - b) + up * b).astype(np.float32)


def bloom(frame, blend_factors, flags: int = 0, threshold: float = 0.0, softness: float = 0.0, clamp: float = 0.0, details=None) -> np.ndarray:
    """(h, w, 3 or 4) composed colours -> (h, w, 3) colours c' in front of the display transform; len(blend_factors) is the level count L
    (0: the frame's own colours)"""
    frame = np.asarray(frame, np.float32)[..., :3]
    h, w = frame.shape[:2]
    L = len(blend_factors)
    if L == 0:
        return frame.copy()
    additive, firefly = bool(flags & ADDITIVE), bool(flags & FIREFLY_SUPPRESS)
    mips = [downsample(prefilter(frame, clamp, threshold, softness), firefly)]
    for _ in range(1, L):
        mips.append(downsample(mips[-1]))
    if details is not None:
        details["down"] = [m.copy() for m in mips]
    for k in range(L - 1, 0, -1):
        mh, mw = mips[k - 1].shape[:2]
        mips[k - 1] = _blend(mips[k - 1], upsample(mips[k], mw, mh), blend_factors[k], additive)
    if details is not None:
        details["up"] = mips
    return _blend(frame, upsample(mips[0], w, h), blend_factors[0], additive)


def rgba(rgb) -> np.ndarray:
    return np.concatenate([rgb, np.ones(rgb.shape[:2] + (1,), np.float32)], -1).astype(np.float32)
