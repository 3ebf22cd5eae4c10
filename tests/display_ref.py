"""numpy restatement of the camera display transform (include/strolle_hip.h "display transforms"): the operators in float32 with the
header's order of operations, the metering histogram, the kept-rank mean and the adaptation step, and the output formats' encodings."""
import math

import numpy as np

F = np.float32
NONE, REINHARD, REINHARD_LUMINANCE, ACES_FITTED, PBR_NEUTRAL = range(5)
BINS = 64
M_IN = ((0.59719, 0.35458, 0.04823), (0.07600, 0.90834, 0.01566), (0.02840, 0.13383, 0.83777))
M_OUT = ((1.60475, -0.53108, -0.07367), (-0.10208, 1.10813, -0.00605), (-0.00327, -0.07276, 1.07602))


def luma(r, g, b):
    return F(0.2126) * r + F(0.7152) * g + F(0.0722) * b


def _rows(m, r, g, b):
    return [F(row[0]) * r + F(row[1]) * g + F(row[2]) * b for row in m]


def transform(c, tonemap: int, s) -> np.ndarray:
    """(..., 3 or 4) composed colours -> (..., 4) float32 display colours, alpha 1"""
    c = np.asarray(c, np.float32)
    s = F(s)
    with np.errstate(all="ignore"):
        r, g, b = c[..., 0] * s, c[..., 1] * s, c[..., 2] * s
        if tonemap != NONE:
            z = F(0)
            r, g, b = np.fmax(r, z), np.fmax(g, z), np.fmax(b, z)
        one = F(1)
        if tonemap == REINHARD:
            r, g, b = r / (one + r), g / (one + g), b / (one + b)
        elif tonemap == REINHARD_LUMINANCE:
            d = one + luma(r, g, b)
            r, g, b = r / d, g / d, b / d
        elif tonemap == ACES_FITTED:
            def fit(v):
                return (v * (v + F(0.0245786)) - F(0.000090537)) / (v * (F(0.983729) * v + F(0.4329510)) + F(0.238081))
            v = [fit(x) for x in _rows(M_IN, r, g, b)]
            r, g, b = [np.fmin(np.fmax(x, F(0)), one) for x in _rows(M_OUT, *v)]
        elif tonemap == PBR_NEUTRAL:
            x = np.fmin(r, np.fmin(g, b))
            offset = np.where(x < F(0.08), x - F(6.25) * x * x, F(0.04)).astype(np.float32)
            r, g, b = r - offset, g - offset, b - offset
            peak = np.fmax(r, np.fmax(g, b))
            d = F(0.24)
            npk = one - d * d / (peak + d - F(0.76))
            q = npk / peak
            w = one - one / (F(0.15) * (peak - npk) + one)
            comp = [(x * q) * (one - w) + npk * w for x in (r, g, b)]
            keep = peak < F(0.76)
            r, g, b = [np.where(keep, x, y).astype(np.float32) for x, y in zip((r, g, b), comp)]
        out = np.stack([r, g, b, np.ones_like(r)], -1).astype(np.float32)
    return out


def manual_scale(exposure_ev: float) -> np.float32:
    return F(2.0 ** float(exposure_ev))


def srgb8(x) -> np.ndarray:
    """clamp, IEC 61966-2-1 encode, round to nearest (float64; the device's encode agrees within 1 LSB)"""
    x = np.clip(np.nan_to_num(np.asarray(x, np.float64), nan=0.0), 0.0, 1.0)
    y = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)
    return np.floor(y * 255.0 + 0.5).astype(np.int32)


def bins(c, ev_min: float, ev_max: float) -> np.ndarray:
    """the metering bin of every pixel of (..., 3 or 4) composed colours"""
    c = np.asarray(c, np.float32)
    y = luma(c[..., 0], c[..., 1], c[..., 2])
    per_ev = F(BINS) / (F(ev_max) - F(ev_min))
    with np.errstate(all="ignore"):
        t = np.floor((np.log2(y) - F(ev_min)) * per_ev)
        k = np.fmin(np.fmax(t, F(0)), F(BINS - 1))
    return np.where(y > 0, k, 0).astype(np.int64)


def histogram(c, ev_min: float, ev_max: float) -> np.ndarray:
    return np.bincount(bins(c, ev_min, ev_max).ravel(), minlength=BINS).astype(np.int64)


def log2_y(c) -> np.ndarray:
    c = np.asarray(c, np.float32)
    with np.errstate(all="ignore"):
        return np.log2(luma(c[..., 0], c[..., 1], c[..., 2]).astype(np.float64))


def metered_ev(counts, low: float, high: float, ev_min: float, ev_max: float):
    """count-weighted mean of the kept bins' centres (ranks [floor(low N), ceil(high N))); None when nothing is kept"""
    counts = np.asarray(counts, np.int64)
    n = int(counts.sum())
    lo, hi = math.floor(float(F(low)) * n), math.ceil(float(F(high)) * n)
    width = (float(F(ev_max)) - float(F(ev_min))) / BINS
    cum, kept, total = 0, 0, 0.0
    for k, cnt in enumerate(counts):
        k0, k1 = max(cum, lo), min(cum + int(cnt), hi)
        cum += int(cnt)
        if k1 > k0:
            kept += k1 - k0
            total += (k1 - k0) * (float(F(ev_min)) + (k + 0.5) * width)
    return None if kept == 0 else F(total / kept)


def adapt(adapted, metered, primed: bool, step_up: float, step_down: float) -> np.float32:
    adapted, metered = F(adapted), F(metered)
    if not primed:
        return metered
    if step_up > 0 and metered - adapted > F(step_up):
        return F(adapted + F(step_up))
    if step_down > 0 and adapted - metered > F(step_down):
        return F(adapted - F(step_down))
    return metered


def auto_scale(compensation_ev: float, adapted_ev) -> np.float32:
    return F(F(0.18) * np.exp2(F(compensation_ev) - F(adapted_ev)))
