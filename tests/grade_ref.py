"""Two statements of include/strolle_hip.h "colour grading", written independently of each other.

`grade_f32` is the numpy restatement: float32, one operation per stated operation, in the header's order, with fog_ref's two polynomials
(exp2p, log2p); min, max and clamp01 follow the post-processing section's NaN rule; the display transform is display_ref's. The kernel
matches it bit for bit.

`grade_f64` is the definition in float64 with numpy's log2 and power, from the same float32 inputs and the same float32 parameters.

A look-up table is an (N, N, N, 3) array indexed [b, g, r] (red fastest when flattened, a .cube file's order)."""
import numpy as np

import display_ref
from fog_ref import exp2p, log2p, pow_  # noqa: F401  (re-exported)
from ref_num import COLOUR_CLAMP, clamp01, max2, min2

F = np.float32
UNIT, LOG2 = 0, 1
DITHER = 1
WHITE_BALANCE, CONTRAST, SATURATION, CDL, LUT, DITHER_STEP = 1, 2, 4, 8, 16, 32
G1 = F(1.0 / 2.2)   # the float nearest 1 / 2.2
Q = (103.0, 71.0, 97.0)
LIN2LMS = np.array([[0.390405, 0.549941, 0.00892632], [0.0708416, 0.963172, 0.00135775], [0.0231082, 0.128021, 0.936245]], np.float64)
LMS2LIN = np.array([[2.85847, -1.62879, -0.0248910], [-0.210182, 1.15820, 0.000324281], [-0.0418120, -0.118169, 1.06867]], np.float64)
W1 = np.array([0.949237, 1.03542, 1.08728], np.float64)


# ---------------------------------------------------------------- host constants
def white_balance_f64(temperature, tint):
    """M = LMS2LIN diag(w1 / w2) LIN2LMS in float64 from the float32 fields, the two products in that order, each sum left to right"""
    t, u = float(F(temperature)), float(F(tint))
    x = 0.31271 - t * (0.1 if t < 0.0 else 0.05)
    y = 2.87 * x - 3.0 * x * x - 0.27509507 + 0.05 * u
    X, Y, Z = x / y, 1.0, (1.0 - x - y) / y
    w2 = np.array([0.7328 * X + 0.4296 * Y - 0.1624 * Z, -0.7036 * X + 1.6975 * Y + 0.0061 * Z, 0.0030 * X + 0.0136 * Y + 0.9834 * Z])
    a = LMS2LIN * (W1 / w2)[None, :]
    m = np.empty((3, 3), np.float64)
    for r in range(3):
        for c in range(3):
            m[r, c] = (a[r, 0] * LIN2LMS[0, c] + a[r, 1] * LIN2LMS[1, c]) + a[r, 2] * LIN2LMS[2, c]
    return m


def steps(d, lut=None):
    """the ST_GRADE_STEP_* bits that run: the LUT step by whether a table is given"""
    s = 0
    if F(d.temperature) != 0 or F(d.tint) != 0:
        s |= WHITE_BALANCE
    if F(d.contrast) != 1:
        s |= CONTRAST
    if F(d.saturation) != 1:
        s |= SATURATION
    if F(d.cdl_saturation) != 1 or any(F(d.slope[i]) != 1 or F(d.offset[i]) != 0 or F(d.power[i]) != 1 for i in range(3)):
        s |= CDL
    if lut is not None:
        s |= LUT
    if d.flags & DITHER:
        s |= DITHER_STEP
    return s


def inv_range(d):
    return F(1.0 / (float(F(d.lut_ev_max)) - float(F(d.lut_ev_min))))


def dither_delta(x, y, k):
    """delta of channel k at the frame coordinates (x, y), float32"""
    d = (171 * np.asarray(x, np.int64) + 231 * np.asarray(y, np.int64)).astype(np.float32)
    t = (d / F(Q[k])).astype(np.float32)
    t = (t - np.floor(t)).astype(np.float32)
    return ((t - F(0.5)) / F(255)).astype(np.float32)


def _coords(h, w, origin):
    x, y = np.meshgrid(np.arange(w, dtype=np.int64) + int(origin[0]), np.arange(h, dtype=np.int64) + int(origin[1]))
    return x, y


def _order(f):
    """the three axes by descending f, ties in the order r, g, b: (h, w, 3) indices a, b, c"""
    return np.argsort(-f, axis=-1, kind="stable")


# ---------------------------------------------------------------- the restatement
def tetrahedral_f32(u, lut):
    """(..., 3) coordinates in [0, 1] -> the table read tetrahedrally, float32, the header's order of operations"""
    lut = np.asarray(lut, np.float32)
    n = lut.shape[0]
    flat = lut.reshape(-1, 3)
    p = (u * F(n - 1)).astype(np.float32)
    i = np.minimum(np.floor(p).astype(np.int64), n - 2)
    f = (p - i.astype(np.float32)).astype(np.float32)
    o = _order(f)
    stride = np.array([1, n, n * n], np.int64)
    i0 = (i[..., 2] * n + i[..., 1]) * n + i[..., 0]
    fa, fb, fc = (np.take_along_axis(f, o[..., k:k + 1], -1)[..., 0] for k in range(3))
    sa, sb = stride[o[..., 0]], stride[o[..., 1]]
    t0, t1, t2, t3 = flat[i0], flat[i0 + sa], flat[i0 + sa + sb], flat[i0 + 1 + n + n * n]
    w0, w1, w2 = (F(1) - fa)[..., None], (fa - fb)[..., None], (fb - fc)[..., None]
    return (((t0 * w0 + t1 * w1) + t2 * w2) + t3 * fc[..., None]).astype(np.float32)


def _pow3(v, p):
    return np.stack([pow_(v[..., k], p) for k in range(3)], -1)


def grade_f32(color, d, tonemap=None, scale=1.0, lut=None, M=None, origin=(0, 0)):
    """(h, w, 4) texels of the node's plane -> (h, w, 4) float32 in front of the output format. `d`: a StColorGradingDesc (or anything with
    its fields); tonemap None: no display; lut: the live table or None; M: the plan's matrix (default: white_balance_f64 rounded once);
    origin: the frame coordinates of color[0, 0] (dither)."""
    c = np.asarray(color, np.float32).copy()
    if c.shape[-1] == 3:
        c = np.concatenate([c, np.ones(c.shape[:-1] + (1,), np.float32)], -1)
    h, w = c.shape[:2]
    s = steps(d, lut)
    with np.errstate(all="ignore"):
        if s & (WHITE_BALANCE | CONTRAST | SATURATION):
            v = min2(max2(c[..., :3], F(0)), F(COLOUR_CLAMP))
            if s & WHITE_BALANCE:
                m = np.asarray(white_balance_f64(d.temperature, d.tint) if M is None else M, np.float64).astype(np.float32)
                r, g, b = v[..., 0], v[..., 1], v[..., 2]
                v = np.stack([max2((m[k, 0] * r + m[k, 1] * g) + m[k, 2] * b, F(0)) for k in range(3)], -1)
            if s & CONTRAST:
                v = (F(0.18) * _pow3((v / F(0.18)).astype(np.float32), d.contrast)).astype(np.float32)
            if s & SATURATION:
                y = display_ref.luma(v[..., 0], v[..., 1], v[..., 2])[..., None]
                v = max2(y + (v - y) * F(d.saturation), F(0))
            c = np.concatenate([min2(v, F(COLOUR_CLAMP)), np.ones((h, w, 1), np.float32)], -1)
        if tonemap is not None:
            c = display_ref.transform(c, int(tonemap), scale)
        if s & (CDL | LUT | DITHER_STEP):
            v = c[..., :3].astype(np.float32)
            if s & CDL:
                v = np.stack([max2(v[..., k] * F(d.slope[k]) + F(d.offset[k]), F(0)) for k in range(3)], -1)
                v = np.stack([pow_(v[..., k], d.power[k]) if F(d.power[k]) != 1 else v[..., k] for k in range(3)], -1)
                if F(d.cdl_saturation) != 1:
                    y = display_ref.luma(v[..., 0], v[..., 1], v[..., 2])[..., None]
                    v = max2(y + (v - y) * F(d.cdl_saturation), F(0))
            if s & LUT:
                if d.lut_domain == LOG2:
                    safe = np.where(v > 0, v, F(1)).astype(np.float32)
                    u = np.where(v > 0, clamp01((log2p(safe) - F(d.lut_ev_min)) * inv_range(d)), F(0)).astype(np.float32)
                else:
                    u = clamp01(v)
                L = tetrahedral_f32(u, lut)
                v = L if F(d.lut_strength) == 1 else (v + (L - v) * F(d.lut_strength)).astype(np.float32)
            if s & DITHER_STEP:
                x, y = _coords(h, w, origin)
                v = np.stack([pow_(max2(pow_(max2(v[..., k], F(0)), G1) + dither_delta(x, y, k), F(0)), F(2.2)) for k in range(3)], -1)
            c = np.concatenate([v.astype(np.float32), np.ones((h, w, 1), np.float32)], -1)
    return c.astype(np.float32)


# ---------------------------------------------------------------- the definition
def _luma64(v):
    return (float(F(0.2126)) * v[..., 0] + float(F(0.7152)) * v[..., 1] + float(F(0.0722)) * v[..., 2])[..., None]


def display_f64(c, tonemap, s):
    """the display section's operators in float64, with the kernels' float32 constants"""
    f = lambda x: float(F(x))   # noqa: E731
    v = c * float(F(s))
    if tonemap == 0:
        return v
    v = np.maximum(v, 0.0)
    if tonemap == 1:
        return v / (1.0 + v)
    if tonemap == 2:
        return v / (1.0 + _luma64(v))
    if tonemap == 3:
        mi = np.array([[f(x) for x in row] for row in display_ref.M_IN])
        mo = np.array([[f(x) for x in row] for row in display_ref.M_OUT])
        a = v @ mi.T
        a = (a * (a + f(0.0245786)) - f(0.000090537)) / (a * (f(0.983729) * a + f(0.4329510)) + f(0.238081))
        return np.clip(a @ mo.T, 0.0, 1.0)
    x = v.min(-1, keepdims=True)
    v = v - np.where(x < f(0.08), x - f(6.25) * x * x, f(0.04))
    peak = v.max(-1, keepdims=True)
    d = f(0.24)
    safe = np.where(peak < f(0.76), 1.0, peak)
    npk = 1.0 - d * d / (safe + d - f(0.76))
    wgt = 1.0 - 1.0 / (f(0.15) * (safe - npk) + 1.0)
    return np.where(peak < f(0.76), v, v * (npk / safe) * (1.0 - wgt) + npk * wgt)


def tetrahedral_f64(u, lut):
    lut = np.asarray(lut, np.float32).astype(np.float64)
    n = lut.shape[0]
    flat = lut.reshape(-1, 3)
    p = u * (n - 1)
    i = np.minimum(np.floor(p).astype(np.int64), n - 2)
    f = p - i
    o = _order(f)
    stride = np.array([1, n, n * n], np.int64)
    i0 = (i[..., 2] * n + i[..., 1]) * n + i[..., 0]
    fa, fb, fc = (np.take_along_axis(f, o[..., k:k + 1], -1) for k in range(3))
    sa, sb = stride[o[..., 0]], stride[o[..., 1]]
    return flat[i0] * (1.0 - fa) + flat[i0 + sa] * (fa - fb) + flat[i0 + sa + sb] * (fb - fc) + flat[i0 + 1 + n + n * n] * fc


def grade_f64(color, d, tonemap=None, scale=1.0, lut=None, origin=(0, 0)):
    """the same grade in float64 from finite float32 inputs: (h, w, 3)"""
    v = np.asarray(color, np.float32).astype(np.float64)[..., :3]
    h, w = v.shape[:2]
    s = steps(d, lut)
    f = lambda x: float(F(x))   # noqa: E731
    with np.errstate(all="ignore"):
        if s & (WHITE_BALANCE | CONTRAST | SATURATION):
            v = np.clip(v, 0.0, COLOUR_CLAMP)
            if s & WHITE_BALANCE:
                v = np.maximum(v @ white_balance_f64(d.temperature, d.tint).T, 0.0)
            if s & CONTRAST:
                v = f(0.18) * np.power(v / f(0.18), f(d.contrast))
            if s & SATURATION:
                y = _luma64(v)
                v = np.maximum(y + (v - y) * f(d.saturation), 0.0)
            v = np.minimum(v, COLOUR_CLAMP)
        if tonemap is not None:
            v = display_f64(v, int(tonemap), scale)
        if s & CDL:
            v = np.maximum(v * np.array([f(x) for x in d.slope]) + np.array([f(x) for x in d.offset]), 0.0)
            v = np.power(v, np.array([f(x) for x in d.power]))
            y = _luma64(v)
            v = np.maximum(y + (v - y) * f(d.cdl_saturation), 0.0)
        if s & LUT:
            if d.lut_domain == LOG2:
                u = np.where(v > 0, np.clip((np.log2(np.where(v > 0, v, 1.0)) - f(d.lut_ev_min)) / (f(d.lut_ev_max) - f(d.lut_ev_min)), 0.0, 1.0), 0.0)
            else:
                u = np.clip(v, 0.0, 1.0)
            L = tetrahedral_f64(u, lut)
            v = v + (L - v) * f(d.lut_strength)
        if s & DITHER_STEP:
            x, y = _coords(h, w, origin)
            n = (171 * x + 231 * y).astype(np.float64)
            t = np.stack([n / q - np.floor(n / q) for q in Q], -1)
            v = np.power(np.maximum(np.power(np.maximum(v, 0.0), 1.0 / 2.2) + (t - 0.5) / 255.0, 0.0), 2.2)
    return v
