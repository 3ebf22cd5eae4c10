"""Two statements of include/strolle_hip.h "lens effects", written independently of each other, and the plan's host constants in numpy.

`lens_f32` is the numpy restatement: float32, one operation per stated operation, in the header's order; min, max and the colour clamp
follow the post-processing section's NaN rule (ref_num), the look-up is post_ref.bilinear, the display transform display_ref's, the hash
integer-only. The kernel matches it bit for bit.

`lens_f64` is the definition in float64 from the same float32 inputs and the same float32 descriptor, with its own host constants in
double (never rounded to float). `tap_spread` is what the tolerance between the two scales with: a float32 source position is uncertain
by a few ulps of the coordinate, and what that moves the look-up by is bounded by how much the texels around the tap differ.

`plan_f64` restates st_lens_plan (the tap table, the fit, scale_eff, the steps) in float64, rounded as the header says."""
import numpy as np

import display_ref
import post_ref
from ref_num import COLOUR_CLAMP, colour, min2

F = np.float32
FIT, VIGNETTE_ROUND, GRAIN_ANIMATE = 1, 2, 4
DISTORTION, FRINGE, VIGNETTE, GRAIN = 1, 2, 4, 8
MAX_TAPS = 16
M32 = np.uint64(0xffffffff)


# ---------------------------------------------------------------- host constants
class Plan:
    """the fields of StLensPlan; the float ones as float32 unless `exact` (then Python floats: the definition's constants)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _round_towards_zero(x):
    f = F(x)
    if float(f) > x:
        f = np.nextafter(f, F(0))
    return F(f)


def tap_table_f64(d):
    """(tap_scale, tap_weight (n, 3)) in float64 from the float32 fields"""
    fringe = float(F(d.fringe))
    if fringe == 0.0:
        return np.ones(1), np.ones((1, 3))
    n = int(d.fringe_taps)
    t = np.arange(n, dtype=np.float64) / (n - 1)
    tent = np.stack([np.maximum(1.0 - 2.0 * t, 0.0), 1.0 - np.abs(2.0 * t - 1.0), np.maximum(2.0 * t - 1.0, 0.0)], -1)
    total = np.zeros(3)
    for i in range(n):   # summed in index order
        total = total + tent[i]
    return 1.0 + fringe * (2.0 * t - 1.0), tent / total


def _f_of(d, r2):
    return (float(F(d.k2)) * r2 + float(F(d.k1))) * r2 + 1.0


def fit_f64(d, w, h, t_max):
    """the largest factor on `scale` at which the outermost tap of every border pixel's centre stays in [0, W] x [0, H], unrounded"""
    cx, cy = 0.5 * w, 0.5 * h
    inv = 1.0 / (cx * cx + cy * cy)
    xs = np.concatenate([np.arange(w), np.arange(w), np.zeros(h), np.full(h, w - 1)]).astype(np.float64)
    ys = np.concatenate([np.zeros(w), np.full(w, h - 1), np.arange(h), np.arange(h)]).astype(np.float64)
    u, v = (xs + 0.5) - cx, (ys + 0.5) - cy
    g = _f_of(d, (u * u + v * v) * inv) * float(F(d.scale)) * t_max
    with np.errstate(divide="ignore"):
        bound = np.concatenate([np.where(u != 0, cx / (np.abs(u) * g), np.inf), np.where(v != 0, cy / (np.abs(v) * g), np.inf)])
    return float(bound.min())


def plan_f64(d, w, h, exact=False):
    """st_lens_plan in numpy. exact: nothing is rounded to float (the definition's constants)"""
    cx, cy = 0.5 * w, 0.5 * h
    inv = 1.0 / (cx * cx + cy * cy)
    ts, tw = tap_table_f64(d)
    n = len(ts)
    ts32 = ts.astype(np.float32)
    steps = FRINGE if float(F(d.fringe)) != 0.0 else 0
    fit = 1.0
    if d.flags & FIT:
        fit = fit_f64(d, w, h, float(ts.max()) if exact else float(ts32.max()))
        fit = 1.0 if not np.isfinite(fit) else (fit if exact else float(_round_towards_zero(fit)))
    scale_eff = float(F(d.scale)) * fit
    if not exact:
        scale_eff = float(F(scale_eff))
    if F(d.k1) != 0 or F(d.k2) != 0 or scale_eff != 1.0:
        steps |= DISTORTION
    if F(d.vignette_intensity) != 0:
        steps |= VIGNETTE
    if F(d.grain_intensity) != 0:
        steps |= GRAIN
    if exact:
        return Plan(steps=steps, taps=n, cx=cx, cy=cy, inv_hd2=inv, fit=fit, scale_eff=scale_eff, tap_scale=ts, tap_weight=tw)
    scale = np.zeros(MAX_TAPS, np.float32); scale[:n] = ts32
    weight = np.zeros((MAX_TAPS, 3), np.float32); weight[:n] = tw.astype(np.float32)
    return Plan(steps=steps, taps=n, cx=F(cx), cy=F(cy), inv_hd2=F(inv), fit=F(fit), scale_eff=F(scale_eff), tap_scale=scale, tap_weight=weight)


def plan_of(p):
    """a Plan from the library's StLensPlan"""
    return Plan(steps=int(p.steps), taps=int(p.taps), cx=F(p.cx), cy=F(p.cy), inv_hd2=F(p.inv_hd2), fit=F(p.fit), scale_eff=F(p.scale_eff),
                tap_scale=np.array(list(p.tap_scale), np.float32), tap_weight=np.array([list(r) for r in p.tap_weight], np.float32))


# ---------------------------------------------------------------- the pieces
def pcg(v):
    """one PCG round on uint32 values (held in uint64 and masked: numpy's own wrap-around is not relied on)"""
    v = (np.asarray(v, np.uint64) * np.uint64(747796405) + np.uint64(2891336453)) & M32
    w = ((((v >> ((v >> np.uint64(28)) + np.uint64(4))) ^ v) & M32) * np.uint64(277803737)) & M32
    return ((w >> np.uint64(22)) ^ w) & M32


def grain_eta(x, y, size, seed):
    """eta of the pixels (x, y), float32: triangular in (-1, 1), exact"""
    s = np.uint64(int(seed) & 0xffffffff)
    cx, cy = np.asarray(x, np.uint64) // np.uint64(size), np.asarray(y, np.uint64) // np.uint64(size)
    h = pcg((cx + pcg((cy + s) & M32)) & M32)
    lo, hi = (h & np.uint64(0xffff)).astype(np.float32), (h >> np.uint64(16)).astype(np.float32)
    return (((lo + hi) - F(65535)) / F(65536)).astype(np.float32)


def seed_of(d, frame=0):
    return (int(d.grain_seed) + (int(frame) if d.flags & GRAIN_ANIMATE else 0)) & 0xffffffff


def _uv32(w, h, plan):
    x, y = np.meshgrid(np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64))
    u = ((x.astype(np.float32) + F(0.5)) - plan.cx).astype(np.float32)
    v = ((y.astype(np.float32) + F(0.5)) - plan.cy).astype(np.float32)
    return x, y, u, v


def positions_f32(d, plan, w, h):
    """the source positions (px, py) of every tap of every pixel, float32: (taps, h, w) each"""
    _, _, u, v = _uv32(w, h, plan)
    r2 = ((u * u + v * v) * plan.inv_hd2).astype(np.float32)
    g = np.ones((h, w), np.float32)
    if plan.steps & DISTORTION:
        g = ((((F(d.k2) * r2 + F(d.k1)) * r2 + F(1)) * plan.scale_eff)).astype(np.float32)
    px, py = [], []
    for i in range(plan.taps):
        s = (g * plan.tap_scale[i]).astype(np.float32)
        px.append((u * s + plan.cx).astype(np.float32)); py.append((v * s + plan.cy).astype(np.float32))
    return np.stack(px), np.stack(py)


# ---------------------------------------------------------------- the restatement
def lens_f32(color, d, plan=None, tonemap=None, scale=1.0, frame=0, force_gather=False):
    """(h, w, 4) texels of the node's plane -> (h, w, 4) float32 in front of the output format. `d`: a StLensDesc (or anything with its
    fields); plan: the library's plan as plan_of gives it (default: plan_f64); tonemap None: no display; frame: the camera's frame counter
    (ST_LENS_GRAIN_ANIMATE); force_gather: the debug seam's instantiation."""
    c = np.asarray(color, np.float32).copy()
    h, w = c.shape[:2]
    plan = plan_f64(d, w, h) if plan is None else plan
    s = plan.steps
    with np.errstate(all="ignore"):
        if s or force_gather:
            x, y, u, v = _uv32(w, h, plan)
            r2 = ((u * u + v * v) * plan.inv_hd2).astype(np.float32)
            src = colour(c)
            if (s & (DISTORTION | FRINGE)) or force_gather:
                px, py = positions_f32(d, plan, w, h)
                o = np.zeros((h, w, 3), np.float32)
                for i in range(plan.taps):
                    wt = plan.tap_weight[i]
                    if wt[0] == 0 and wt[1] == 0 and wt[2] == 0:
                        continue
                    ix, fx = post_ref.axis_float(px[i]); iy, fy = post_ref.axis_float(py[i])
                    o = (o + post_ref.bilinear(src, ix, fx, iy, fy) * wt[None, None, :]).astype(np.float32)
            else:
                o = src
            if s & VIGNETTE:
                if d.flags & VIGNETTE_ROUND:
                    m = r2
                else:
                    a, b = (u / plan.cx).astype(np.float32), (v / plan.cy).astype(np.float32)
                    m = ((a * a + b * b) * F(0.5)).astype(np.float32)
                q = (F(1) + m * F(d.vignette_falloff)).astype(np.float32)
                fall = (F(1) / (q * q)).astype(np.float32)
                k = ((F(1) - F(d.vignette_intensity)) + F(d.vignette_intensity) * fall).astype(np.float32)
                o = (o * k[..., None]).astype(np.float32)
            if s & GRAIN:
                eta = grain_eta(x, y, int(d.grain_size), seed_of(d, frame))
                k = (F(1) + F(d.grain_intensity) * eta).astype(np.float32)
                o = (o * k[..., None]).astype(np.float32)
            c = np.concatenate([min2(o, F(COLOUR_CLAMP)), np.ones((h, w, 1), np.float32)], -1)
        if tonemap is not None:
            c = display_ref.transform(c, int(tonemap), scale)
    return c.astype(np.float32)


# ---------------------------------------------------------------- the definition
def _bilinear64(src, px, py):
    h, w = src.shape[:2]
    qx, qy = px - 0.5, py - 0.5
    ix, iy = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
    fx, fy = (qx - ix)[..., None], (qy - iy)[..., None]
    x0, x1, y0, y1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1), np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    top = src[y0, x0] * (1.0 - fx) + src[y0, x1] * fx
    bot = src[y1, x0] * (1.0 - fx) + src[y1, x1] * fx
    return top * (1.0 - fy) + bot * fy


def _spread64(src, px, py):
    """max - min per channel over the 4 x 4 texels around the tap (indices clamped): the 2 x 2 it reads and their neighbours, which a
    position moved across a texel centre reads instead"""
    h, w = src.shape[:2]
    ix, iy = np.floor(px - 0.5).astype(np.int64), np.floor(py - 0.5).astype(np.int64)
    lo, hi = None, None
    for dy in range(-1, 3):
        for dx in range(-1, 3):
            t = src[np.clip(iy + dy, 0, h - 1), np.clip(ix + dx, 0, w - 1)]
            lo, hi = (t, t) if lo is None else (np.minimum(lo, t), np.maximum(hi, t))
    return hi - lo


def lens_f64(color, d, tonemap=None, scale=1.0, frame=0, spread=False):
    """the same node in float64 from finite float32 inputs: (h, w, 3); with `spread` also tap_spread, (h, w, 3): the weighted sum over the
    taps of the texels' max - min around each tap, times the pixel's vignette and grain factor (0 for a pixel without taps)"""
    import grade_ref
    src = np.clip(np.asarray(color, np.float32).astype(np.float64)[..., :3], 0.0, COLOUR_CLAMP)
    h, w = src.shape[:2]
    p = plan_f64(d, w, h, exact=True)
    f = lambda x: float(F(x))   # noqa: E731
    x, y = np.meshgrid(np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64))
    u, v = (x + 0.5) - p.cx, (y + 0.5) - p.cy
    r2 = (u * u + v * v) * p.inv_hd2
    o, sp = src, np.zeros_like(src)
    if p.steps & (DISTORTION | FRINGE):
        g = _f_of(d, r2) * p.scale_eff if p.steps & DISTORTION else np.ones_like(r2)
        o = np.zeros_like(src)
        for i in range(p.taps):
            px, py = u * (g * p.tap_scale[i]) + p.cx, v * (g * p.tap_scale[i]) + p.cy
            o = o + _bilinear64(src, px, py) * p.tap_weight[i]
            sp = sp + _spread64(src, px, py) * p.tap_weight[i]
    k = np.ones_like(r2)
    if p.steps & VIGNETTE:
        m = r2 if d.flags & VIGNETTE_ROUND else ((u / p.cx) ** 2 + (v / p.cy) ** 2) * 0.5
        a = f(d.vignette_intensity)
        k = k * ((1.0 - a) + a / (1.0 + m * f(d.vignette_falloff)) ** 2)
    if p.steps & GRAIN:
        k = k * (1.0 + f(d.grain_intensity) * grain_eta(x, y, int(d.grain_size), seed_of(d, frame)).astype(np.float64))
    o = np.minimum(o * k[..., None], COLOUR_CLAMP) if p.steps else o
    if tonemap is not None:
        o = grade_ref.display_f64(o, int(tonemap), scale)
    return (o, sp * k[..., None]) if spread else o
