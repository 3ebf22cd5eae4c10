"""numpy restatement of the upscale stage (include/strolle_hip.h "upscaling"): the edge-adaptive upscaler and the contrast-adaptive
sharpening step in float32 with the header's order of operations. It is the normative statement: k_upscale.hip follows it bit for bit in
both builds. Where the prose leaves a choice, the choice is written here: the stencils go f, g, j, k and each adds along x, then along y;
the twelve taps are summed in the order b c e f g h i j k l n o; min2 / max2 are the post-processing section's.

upscale_f32 / sharpen_f32 are the restatement; upscale_f64 / sharpen_f64 are the definition: the same formulas carried in float64 from
the same clamped float32 texels and the exact fractions, every product and sum rounded to 53 bits instead of 24. What the two share is
this file's `_upscale` / `_sharpen` with the number type as an argument, so the definition guards the restatement's rounding, not its
reading of the formulas: that is what the hand-computed cases of tests/test_upscale_abi.py are for."""
import numpy as np

import post_ref
from ref_num import max2 as _max32, min2 as _min32

F = np.float32
DENOISE = 1
R2_MIN = 1.0 / 32768.0
# tap offsets (dx, dy) from (x0, y0), in the summation order
TAPS = {"b": (0, -1), "c": (1, -1), "e": (-1, 0), "f": (0, 0), "g": (1, 0), "h": (2, 0), "i": (-1, 1), "j": (0, 1), "k": (1, 1), "l": (2, 1),
        "n": (0, 2), "o": (1, 2)}
# the four stencils, in order: centre, weight's factors, arms (top, left, right, bottom)
STENCILS = (("f", "b", "e", "g", "j"), ("g", "c", "f", "h", "k"), ("j", "f", "i", "k", "n"), ("k", "g", "j", "l", "o"))


def unit(img):
    """post_unit of the first three channels: into [0, 1], NaN -> 0; float32 (a float64 image, the definition's own, stays float64)"""
    c = np.asarray(img)[..., :3]
    T = np.float64 if c.dtype == np.float64 else np.float32
    c = c.astype(T)
    with np.errstate(all="ignore"):
        return np.where(c > 0, np.where(c < 1, c, T(1)), T(0)).astype(T)


def _mm(T):
    if T == np.float32:
        return _min32, _max32
    return (lambda a, b: np.where((a < b) | (b != b), a, b)), (lambda a, b: np.where((a > b) | (b != b), a, b))


def _luma(c, T):
    return T(0.5) * c[..., 2] + (T(0.5) * c[..., 0] + c[..., 1])


def _axis(n_src, n_dst, T):
    o = np.arange(n_dst, dtype=np.int64)
    n, d = (2 * o + 1) * n_src - n_dst, 2 * n_dst
    i0 = n // d
    if T == np.float32:
        f = ((n - i0 * d).astype(np.float32) / F(d)).astype(np.float32)   # post_ref.axis_resample
    else:
        f = (n - i0 * d).astype(np.float64) / np.float64(d)
    return i0, f


def _upscale(img, ow, oh, T, details=None):
    src = unit(img).astype(T)
    h, w = src.shape[:2]
    mn, mx = _mm(T)
    x0, fx = _axis(w, ow, T)
    y0, fy = _axis(h, oh, T)
    x0, fx, y0, fy = x0[None, :], fx[None, :], y0[:, None], fy[:, None]
    x0, fx, y0, fy = np.broadcast_arrays(x0, fx, y0, fy)
    one = T(1)
    with np.errstate(all="ignore"):
        tap = {k: src[np.clip(y0 + dy, 0, h - 1), np.clip(x0 + dx, 0, w - 1)] for k, (dx, dy) in TAPS.items()}
        L = {k: _luma(v, T) for k, v in tap.items()}
        ws = ((one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy)
        dirx = np.zeros(fx.shape, T); diry = np.zeros(fx.shape, T); ln = np.zeros(fx.shape, T)

        def arm(p, q, r, wgt):
            m = mx(np.abs(r - q), np.abs(q - p))
            t = np.where(m > 0, mn(np.abs(r - p) / np.where(m > 0, m, one), one), T(0)).astype(T)
            return (r - p) * wgt, (t * t) * wgt

        for (cq, top, left, right, bottom), wgt in zip(STENCILS, ws):
            dx_, l_ = arm(L[left], L[cq], L[right], wgt)
            dirx = dirx + dx_; ln = ln + l_
            dy_, l_ = arm(L[top], L[cq], L[bottom], wgt)
            diry = diry + dy_; ln = ln + l_
        r2 = dirx * dirx + diry * diry
        small = r2 < T(R2_MIN)
        s = np.sqrt(np.where(small, one, r2)).astype(T)
        dirx = np.where(small, one, dirx / s).astype(T); diry = np.where(small, T(0), diry / s).astype(T)
        ln = T(0.5) * ln
        ln = ln * ln
        stretch = (dirx * dirx + diry * diry) / mx(np.abs(dirx), np.abs(diry))
        l2x = one + (stretch - one) * ln
        l2y = one - T(0.5) * ln
        lob = T(0.5) + ((T(0.25) - T(0.04)) - T(0.5)) * ln
        clp = one / lob
        sc = np.zeros(fx.shape + (3,), T); sw = np.zeros(fx.shape, T)
        weights = {}
        for k, (dx, dy) in TAPS.items():
            ox, oy = T(dx) - fx, T(dy) - fy
            vx = (ox * dirx + oy * diry) * l2x
            vy = (-ox * diry + oy * dirx) * l2y
            d2 = mn(vx * vx + vy * vy, clp)
            tb = T(0.4) * d2 - one
            wb = T(1.5625) * (tb * tb) - T(0.5625)
            ta = lob * d2 - one
            wk = wb * (ta * ta)
            weights[k] = wk
            sc = sc + tap[k] * wk[..., None]
            sw = sw + wk
        ok = sw > 0
        v = np.where(ok[..., None], sc / np.where(ok, sw, one)[..., None], tap["f"]).astype(T)
        lo = mn(mn(mn(tap["f"], tap["g"]), tap["j"]), tap["k"])
        hi = mx(mx(mx(tap["f"], tap["g"]), tap["j"]), tap["k"])
        out = mn(mx(v, lo), hi).astype(T)
    if details is not None:
        details.update(dir_x=dirx, dir_y=diry, r2=r2, len=ln, lob=lob, clp=clp, len2_x=l2x, len2_y=l2y, weights=weights, wsum=sw,
                       fallback=int(np.count_nonzero(~ok)), wsum_min=float(sw.min()))
    return out


def _sharpen(img, sharpness, denoise, T, details=None):
    c = unit(img).astype(T)
    h, w = c.shape[:2]
    mn, mx = _mm(T)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")

    def at(dy, dx):
        return c[np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)]

    e, b, d, f, hh = at(0, 0), at(-1, 0), at(0, -1), at(0, 1), at(1, 0)
    one, four, zero = T(1), T(4), T(0)
    with np.errstate(all="ignore"):
        mn4 = mn(mn(mn(b, d), f), hh)
        mx4 = mx(mx(mx(b, d), f), hh)
        hit_min = np.where(mx4 == 0, zero, mn(mn4, e) / (four * np.where(mx4 == 0, one, mx4))).astype(T)
        den = four * mn4 - four
        hit_max = np.where(den == 0, zero, (one - mx(mx4, e)) / np.where(den == 0, one, den)).astype(T)
        lobe_c = mx(-hit_min, hit_max)
        lobe = mx(T(-0.1875), mn(mx(mx(lobe_c[..., 0], lobe_c[..., 1]), lobe_c[..., 2]), zero)) * T(sharpness)
        nz = np.zeros(lobe.shape, T)
        if denoise:
            bL, dL, fL, hL, eL = (_luma(v, T) for v in (b, d, f, hh, e))
            rng = mx(mx(mx(mx(bL, dL), fL), hL), eL) - mn(mn(mn(mn(bL, dL), fL), hL), eL)
            q = T(0.25)
            nz = np.where(rng == 0, zero, mn(np.abs((((q * bL + q * dL) + q * fL) + q * hL) - eL) / np.where(rng == 0, one, rng), one)).astype(T)
            lobe = lobe * (one - T(0.5) * nz)
        if details is not None:
            details.update(lobe=lobe, noise=nz)
        lb = lobe[..., None]
        return (((((lb * b + lb * d) + lb * hh) + lb * f) + e) / (four * lb + one)).astype(T)


def _rgb1(rgb):
    return np.concatenate([rgb, np.ones(rgb.shape[:-1] + (1,), rgb.dtype)], -1)


def upscale_f32(img, out_w, out_h, details=None):
    """(H, W, 3 or 4) -> (out_h, out_w, 4) float32, alpha 1"""
    return _rgb1(_upscale(img, out_w, out_h, np.float32, details))


def upscale_f64(img, out_w, out_h, details=None):
    return _rgb1(_upscale(img, out_w, out_h, np.float64, details))


def sharpen_f32(img, sharpness, denoise=False, details=None):
    """(H, W, 3 or 4) -> (H, W, 4) float32, alpha 1; `details` receives the lobe and the noise term nz per pixel"""
    return _rgb1(_sharpen(img, sharpness, denoise, np.float32, details))


def sharpen_f64(img, sharpness, denoise=False):
    return _rgb1(_sharpen(img, sharpness, denoise, np.float64))


def _process(img, out_size, sharpness, denoise, up, sh):
    x = np.asarray(img)
    h, w = x.shape[:2]
    ow, oh = out_size if out_size and tuple(out_size) != (0, 0) else (w, h)
    if (ow, oh) != (w, h):
        x = up(x, ow, oh)
    if F(sharpness) > 0:
        x = sh(x, sharpness, denoise)
    return x


def process(img, out_size=None, sharpness=0.0, denoise=False):
    """what st_upscale_process / a camera's upscale stage computes from an RGBA32F image, before the output format: (OH, OW, 4) float32.
    A call that asks for neither step copies the colour as it is, alpha 1 (post_ref.process)."""
    h, w = np.asarray(img).shape[:2]
    ow, oh = out_size if out_size and tuple(out_size) != (0, 0) else (w, h)
    if (ow, oh) == (w, h) and not F(sharpness) > 0:
        return post_ref.process(img)
    return _process(img, out_size, sharpness, denoise, upscale_f32, sharpen_f32)


def process_f64(img, out_size=None, sharpness=0.0, denoise=False, details=None):
    """the definition of the same; the sharpening step reads the float64 upscaled colour"""
    return _process(img, out_size, sharpness, denoise, lambda x, ow, oh: upscale_f64(x, ow, oh, details), sharpen_f64)
