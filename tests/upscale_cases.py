"""The inputs the CPU and GPU tests of the upscale stage share (tests/test_upscale_abi.py, tests/test_gpu_upscale.py): the slanted-edge
fixture of analytic coverage, the synthetic images, the matrix of sizes, and the float64 comparison's bookkeeping. A plain module."""
import math

import numpy as np

import post_ref
import upscale_ref as U

F = np.float32
EDGE_SOURCE = (48, 34)                         # the fixture's source size
EDGE_ANGLES = (20.0, 33.0, 58.0)               # degrees off the x axis: asserted
EDGE_AXIS_ANGLES = (0.0, 90.0)                 # recorded, not asserted
EDGE_RATIOS = {"2/1": (2, 1), "3/2": (3, 2)}


def edge(w, h, angle_deg, scale=1.0):
    """analytic coverage (h, w) float64 of a half-plane whose edge passes through the image's centre at `angle_deg` off the x axis; `scale`
    is the size of this image relative to the source (the same edge at another resolution)"""
    cx, cy = w / 2.0 + 0.37 * scale, h / 2.0 - 0.21 * scale
    if angle_deg == 90.0:   # a vertical edge: the transposed horizontal one
        return post_ref.half_plane(h, w, 0.0, cx)[1].T.copy()
    slope = math.tan(math.radians(angle_deg))
    return post_ref.half_plane(w, h, slope, cy - slope * cx)[1]


def grey(plane):
    p = np.asarray(plane, np.float32)
    return np.stack([p, p, p, np.ones_like(p)], -1)


def edge_rms(angle_deg, ratio):
    """(the restatement's, Catmull-Rom's) RMS error against the coverage rendered at the output size, from the coverage at the source size"""
    num, den = ratio
    w, h = EDGE_SOURCE
    ow, oh = w * num // den, h * num // den
    src = grey(edge(w, h, angle_deg))
    want = edge(ow, oh, angle_deg, num / den)
    up = U.upscale_f32(src, ow, oh)[..., 0].astype(np.float64)
    cr = post_ref.resample(src, ow, oh, post_ref.CATMULL_ROM)[..., 0].astype(np.float64)
    return float(np.sqrt(np.mean((up - want) ** 2))), float(np.sqrt(np.mean((cr - want) ** 2)))


# ---------------------------------------------------------------- the matrix of st_upscale_process
def images():
    """name -> (H, W, 4) float32: display-referred noise, the slanted edges, a checker, a ramp, and a spoiled image with values below 0,
    above 1, infinities and NaN. Every source size of the matrix is cut from the top-left corner of these 52-row, 72-column images."""
    rng = np.random.default_rng(23)
    h, w = 52, 72
    noise = rng.random((h, w, 4)).astype(np.float32)
    s1 = edge(w, h, 33.0)
    s2 = edge(w, h, 58.0)[:, ::-1]
    slanted = np.stack([0.1 + 0.8 * s1, 0.9 - 0.7 * s2 * s1, 0.2 + 0.6 * s2, np.ones_like(s1)], -1).astype(np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    checker = grey(np.where(((xs // 3) + (ys // 2)) % 2 == 0, 0.85, 0.1))
    ramp = np.stack([xs / (w - 1.0), ys / (h - 1.0), (xs + ys) / (w + h - 2.0), np.ones((h, w))], -1).astype(np.float32)
    spoiled = (rng.standard_normal((h, w, 4)) * 0.8 + 0.5).astype(np.float32)
    n = 40
    for v in (np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 7.5, -3.0):
        spoiled[rng.integers(0, h, n), rng.integers(0, w, n), rng.integers(0, 3, n)] = v
    return {"noise": noise, "slanted": slanted, "checker": checker, "ramp": ramp, "spoiled": spoiled}


SOURCES = ((1, 1), (2, 2), (3, 2), (5, 5), (9, 7), (37, 23), (72, 52))


def outputs(w, h):
    """name -> (ow, oh) for a w x h source: equal, +1 pixel, 4/3, 3/2, 2x, 3x, and (for the largest source) one axis equal and the sizes
    around the kernels' 64 x 4 tile"""
    o = {"equal": (w, h), "+1": (w + 1, h + 1), "4/3": (-(-w * 4 // 3), -(-h * 4 // 3)), "3/2": (-(-w * 3 // 2), -(-h * 3 // 2)), "2x": (2 * w, 2 * h),
         "3x": (3 * w, 3 * h)}
    if (w, h) == (72, 52):
        o["one axis equal"] = (144, 52)
    if (w, h) == (37, 23):   # output widths 63, 64, 65 and 129; heights 23 .. 26 and 47 cross the tile height of 4
        o.update({"w63": (63, 23), "w64": (64, 24), "w65": (65, 25), "w129": (129, 26), "h47": (40, 47)})
    return o


def cases():
    """(image name, (w, h), output name, (ow, oh), sharpness, denoise): every source against every output with sharpness 1 and the
    noise limiter on; the other sharpness values and the limiter off at the 3/2 ratio (sharpness and the limiter do not meet the sizes)"""
    out = []
    names = list(images())
    for si, (w, h) in enumerate(SOURCES):
        for oi, (oname, osize) in enumerate(outputs(w, h).items()):
            img = names[(si + oi) % len(names)]
            out.append((img, (w, h), oname, osize, 1.0, True))
            if oname in ("3/2", "equal"):
                for sharp, den in ((0.0, False), (0.25, False), (0.25, True), (1.0, False)):
                    if oname == "equal" and sharp == 0.0:
                        continue   # neither step: the copy, tested on its own
                    out.append((img, (w, h), oname, osize, sharp, den))
    for img in names:   # every image at the largest source, 3/2 and 2x
        for oname in ("3/2", "2x"):
            out.append((img, (72, 52), oname, outputs(72, 52)[oname], 0.25, True))
    return out


def source(name, size):
    w, h = size
    return np.ascontiguousarray(images()[name][:h, :w])


# ---------------------------------------------------------------- the float64 comparison
def r2_deviation(img, out_size):
    """the restatement's worst deviation of r2 from the definition's on one case, relative to max(r2, 1/32768): rounding errors scale with
    the value, and next to the threshold — where the figure is used — the denominator is the threshold"""
    d32, d64 = {}, {}
    U.upscale_f32(img, out_size[0], out_size[1], d32)
    U.upscale_f64(img, out_size[0], out_size[1], d64)
    return float((np.abs(d32["r2"].astype(np.float64) - d64["r2"]) / np.maximum(d64["r2"], U.R2_MIN)).max())


def f64_comparison(img, out_size, sharpness, denoise, margin):
    """One case: (the restatement's result, the definition's colour, the pixels left out of their comparison). A pixel is left out when
    its float64 r2 lies within `margin` of 1/32768, the one branch whose sides differ by more than rounding (below it the kernel's direction
    is (1, 0), above it the gradient's); the sharpening step spreads a left-out pixel to its four neighbours."""
    h, w = img.shape[:2]
    ow, oh = out_size
    d64 = {}
    got = U.process(img, out_size, sharpness, denoise)
    want = U.process_f64(img, out_size, sharpness, denoise, d64)[..., :3]
    skip = np.zeros((oh, ow), bool)
    if d64:
        skip = np.abs(d64["r2"] - U.R2_MIN) <= margin
        if sharpness > 0:
            s = skip.copy()
            s[1:] |= skip[:-1]; s[:-1] |= skip[1:]; s[:, 1:] |= skip[:, :-1]; s[:, :-1] |= skip[:, 1:]
            skip = s
    return got, want, skip


def deviation(got, want, skip):
    """the worst channel of |got - want| over the pixels that are compared"""
    dev = np.abs(np.asarray(got)[..., :3].astype(np.float64) - want).max(-1)
    return float(dev[~skip].max()) if (~skip).any() else 0.0
