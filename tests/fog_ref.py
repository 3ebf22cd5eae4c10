"""Two statements of include/strolle_hip.h "fog", written independently of each other.

`fog_f32` is the numpy restatement: float32, one operation per stated operation, in the header's order, with the header's two polynomials
(exp2p, log2p) restated here; min, max and clamp01 follow the post-processing section's NaN rule. The kernel matches it bit for bit.

`fog_f64` is the definition in float64 with numpy's exp, expm1 and power, and no clamp except those that change the mathematical result
(the k and E0 clamps at +-80, clamp01 of the linear ramp, the cosine's [0, 1], the colour clamp)."""
import numpy as np

from ref_num import COLOUR_CLAMP, FLT_MAX, clamp01, frame_depth, max2, min2  # noqa: F401  (re-exported)

F = np.float32
LINEAR, EXPONENTIAL, EXPONENTIAL_SQUARED, ATMOSPHERIC = 0, 1, 2, 3
SKY, FOLLOW_SUN = 1, 2


# ---------------------------------------------------------------- the two polynomials, from the header text
def scale2(z, n):
    """z 2^n in float32, with two multiplications when n leaves [-126, 127]"""
    z, n = np.asarray(z, np.float32).copy(), np.asarray(n, np.int64).copy()
    big, small = n > 127, n < -126
    z = np.where(big, z * F(2.0 ** 127), z).astype(np.float32)
    n = np.where(big, np.minimum(n - 127, 127), n)
    z = np.where(small, z * F(2.0 ** -126), z).astype(np.float32)
    n = np.where(small, np.maximum(n + 126, -126), n)
    return (z * np.ldexp(F(1), n.astype(np.int32)).astype(np.float32)).astype(np.float32)


def exp2p(x):
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        ok = (x == x) & (x <= F(127.999)) & (x >= F(-150.0))
        xs = np.where(ok, x, F(0)).astype(np.float32)
        px = np.floor(xs)
        i = px.astype(np.int64)
        f = (xs - px).astype(np.float32)
        up = f > F(0.5)
        i = i + up
        f = np.where(up, f - F(1), f).astype(np.float32)
        p = F(1.535336188319500e-4) * f + F(1.339887440266574e-3)
        for c in (9.618437357674640e-3, 5.550332471162809e-2, 2.402264791363012e-1, 6.931472028550421e-1, 1.0):
            p = p * f + F(c)
        r = scale2(p.astype(np.float32), i)
        r = np.where(x > F(127.999), F(np.inf), r)
        r = np.where(x < F(-150.0), F(0), r)
        return np.where(x != x, x, r).astype(np.float32)


def log2p(x):
    """x > 0 and finite"""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        b = x.view(np.uint32)
        sub = (b & np.uint32(0x7f800000)) == 0
        x = np.where(sub, x * F(8388608.0), x).astype(np.float32)
        e = np.where(sub, -23, 0).astype(np.int64)
        b = x.view(np.uint32)
        e = e + ((b >> np.uint32(23)) & np.uint32(0xff)).astype(np.int64) - 126
        m = ((b & np.uint32(0x007fffff)) | np.uint32(0x3f000000)).view(np.float32)
        low = m < F(0.707106781186547524)
        e = np.where(low, e - 1, e)
        m = np.where(low, (m + m) - F(1), m - F(1)).astype(np.float32)
        z = m * m
        y = F(7.0376836292e-2) * m - F(1.1514610310e-1)
        for sign, c in ((1, 1.1676998740e-1), (-1, 1.2420140846e-1), (1, 1.4249322787e-1), (-1, 1.6668057665e-1), (1, 2.0000714765e-1), (-1, 2.4999993993e-1),
                        (1, 3.3333331174e-1)):
            y = y * m + F(c) if sign > 0 else y * m - F(c)
        y = y * m * z
        y = y - F(0.5) * z
        r = y * F(0.44269504088896340736)
        r = r + m * F(0.44269504088896340736)
        r = r + y
        r = r + m
        r = r + e.astype(np.float32)
        return r.astype(np.float32)


def exp_(x):
    return exp2p(np.asarray(x, np.float32) * F(1.44269504088896341))


def pow_(s, p):
    s = np.asarray(s, np.float32)
    safe = np.where(s == 0, F(1), s).astype(np.float32)
    return np.where(s == 0, F(0), exp2p(F(p) * log2p(safe))).astype(np.float32)


# ---------------------------------------------------------------- step 0
def lobe_on(d):
    return any(float(v) != 0.0 for v in d.light_color)


def host_constants(d, transform, sun=None):
    """(L as three float32, E0 as float32): computed in double from the float32 fields, rounded once"""
    L = np.zeros(3, np.float32)
    if lobe_on(d):
        v = np.array([float(F(x)) for x in (sun if (d.flags & FOLLOW_SUN) else d.light_direction)], np.float64)
        L = (v / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])).astype(np.float32)
    arg = -float(F(d.height_falloff)) * (float(F(transform[13])) - float(F(d.height_reference)))
    return L, F(np.exp(min(max(arg, -80.0), 80.0)))


# ---------------------------------------------------------------- the restatement
def fog_f32(color, depth, transform, projection, d, sun=None, details=None):
    """(h, w, 4) composed colours and (h, w) distances along the rays of a camera with `transform` and `projection` (16 floats each, column
    major) -> (h, w, 4) in front of depth of field. `d`: a StFogDesc (or anything with its fields); `sun`: ST_FOG_FOLLOW_SUN's direction."""
    C = np.asarray(color, np.float32)
    D = np.asarray(depth, np.float32)
    h, w = D.shape
    M = np.asarray(transform, np.float32).reshape(16)
    P = np.asarray(projection, np.float32).reshape(16)
    L, E0 = host_constants(d, M, sun)
    a, b = F(d.color[3]), F(d.height_falloff)
    with np.errstate(all="ignore"):
        # 1. ray
        x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
        ndc_x = (x + F(0.5)) * F(2) / F(w) - F(1)
        ndc_y = -((y + F(0.5)) * F(2) / F(h) - F(1))
        ax, ay = (ndc_x + P[8]) / P[0], (ndc_y + P[9]) / P[5]
        c = F(1) / np.sqrt((ax * ax + ay * ay) + F(1)).astype(np.float32)
        vx, vy, vz = ax * c, ay * c, -c
        wv = [(M[i] * vx + M[4 + i] * vy + M[8 + i] * vz).astype(np.float32) for i in range(3)]
        dy = wv[1]
        # 2. distance
        hit = D > 0
        sky = hit & (D >= FLT_MAX)
        fogged = hit & (~sky | bool(d.flags & SKY))
        dd = np.where(sky, F(d.sky_distance), D).astype(np.float32)
        dd = np.where(fogged, dd, F(1)).astype(np.float32)
        # 3. height
        if b == 0:
            de = dd
        else:
            k = min2(max2((b * dy) * dd, F(-80)), F(80))
            ks = np.where(np.abs(k) < F(0.03125), F(1), k).astype(np.float32)
            G = np.where(np.abs(k) < F(0.03125), F(1) - k * (F(0.5) - k * F(0.16666667)), (F(1) - exp_(-ks)) / ks).astype(np.float32)
            de = min2(dd * (E0 * G), F(FLT_MAX))
        # 4. factors
        if d.falloff == ATMOSPHERIC:
            ge = np.stack([(F(1) - exp_(-(F(d.extinction[i]) * de))) * a for i in range(3)], -1).astype(np.float32)
            gi = np.stack([(F(1) - exp_(-(F(d.inscattering[i]) * de))) * a for i in range(3)], -1).astype(np.float32)
        else:
            if d.falloff == LINEAR:
                g = clamp01((de - F(d.start)) / (F(d.end) - F(d.start)))
            elif d.falloff == EXPONENTIAL:
                g = F(1) - exp_(-(F(d.density) * de))
            else:
                u = F(d.density) * de
                g = F(1) - exp_(-(u * u))
            ge = gi = np.repeat((g * a).astype(np.float32)[..., None], 3, -1)
        fogged &= (ge != 0).any(-1) | (gi != 0).any(-1)
        # 5. colour
        Fc = np.broadcast_to(np.array([F(v) for v in d.color[:3]], np.float32), (h, w, 3))
        s = None
        if lobe_on(d):
            s = min2(max2((wv[0] * L[0] + wv[1] * L[1]) + wv[2] * L[2], F(0)), F(1))
            lobe = pow_(s, d.light_exponent)
            Fc = np.stack([min2(F(d.color[i]) + F(d.light_color[i]) * lobe, F(FLT_MAX)) for i in range(3)], -1)
        cc = min2(max2(C[..., :3], F(0)), F(COLOUR_CLAMP))
        rgb = (cc * (F(1) - ge) + Fc * gi).astype(np.float32)
    out = np.concatenate([rgb, np.ones((h, w, 1), np.float32)], -1)
    src = C if C.shape[-1] == 4 else np.concatenate([C, np.ones((h, w, 1), np.float32)], -1)
    out[~fogged] = src[~fogged]
    if details is not None:
        details.update(L=L, E0=E0, dy=dy, w=wv, de=de, ge=ge, gi=gi, F=Fc, s=s, fogged=fogged, cc=cc)
    return out


# ---------------------------------------------------------------- the definition
def fog_f64(color, depth, transform, projection, d, sun=None, details=None):
    """the same medium in float64 from the same float32 inputs: (h, w, 3) and the mask of the pixels the fog changes"""
    C = np.asarray(color, np.float32).astype(np.float64)
    D = np.asarray(depth, np.float32).astype(np.float64)
    h, w = D.shape
    M = np.asarray(transform, np.float32).astype(np.float64).reshape(4, 4).T   # M[r, c]
    P = np.asarray(projection, np.float32).astype(np.float64).reshape(16)
    with np.errstate(all="ignore"):
        px, py = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
        ax = ((2.0 * px / w - 1.0) + P[8]) / P[0]
        ay = (-(2.0 * py / h - 1.0) + P[9]) / P[5]
        view = np.stack([ax, ay, -np.ones_like(ax)], -1) / np.sqrt(ax * ax + ay * ay + 1.0)[..., None]
        world = view @ M[:3, :3].T
        hit = D > 0
        sky = hit & (D >= FLT_MAX)
        fogged = hit & (~sky | bool(d.flags & SKY))
        dist = np.where(sky, float(F(d.sky_distance)), D)
        dist = np.where(fogged, dist, 1.0)
        b = float(F(d.height_falloff))
        if b != 0.0:
            e0 = np.exp(np.clip(-b * (M[1, 3] - float(F(d.height_reference))), -80.0, 80.0))
            k = np.clip(b * world[..., 1] * dist, -80.0, 80.0)
            G = np.where(k == 0.0, 1.0, -np.expm1(-k) / np.where(k == 0.0, 1.0, k))
            dist = np.minimum(dist * e0 * G, float(FLT_MAX))
        a = float(F(d.color[3]))
        if d.falloff == ATMOSPHERIC:
            ge = -np.expm1(-np.array([float(F(v)) for v in d.extinction]) * dist[..., None]) * a
            gi = -np.expm1(-np.array([float(F(v)) for v in d.inscattering]) * dist[..., None]) * a
        else:
            if d.falloff == LINEAR:
                g = np.clip((dist - float(F(d.start))) / (float(F(d.end)) - float(F(d.start))), 0.0, 1.0)
            elif d.falloff == EXPONENTIAL:
                g = -np.expm1(-float(F(d.density)) * dist)
            else:
                g = -np.expm1(-np.square(float(F(d.density)) * dist))
            ge = gi = np.repeat((g * a)[..., None], 3, -1)
        fogged &= (ge != 0).any(-1) | (gi != 0).any(-1)
        fog_colour = np.broadcast_to(np.array([float(F(v)) for v in d.color[:3]]), (h, w, 3))
        if lobe_on(d):
            v = np.array([float(F(x)) for x in (sun if (d.flags & FOLLOW_SUN) else d.light_direction)], np.float64)
            cos = np.clip(world @ (v / np.linalg.norm(v)), 0.0, 1.0)
            fog_colour = fog_colour + np.array([float(F(x)) for x in d.light_color]) * np.power(cos, float(F(d.light_exponent)))[..., None]
        cc = np.clip(np.where(C[..., :3] != C[..., :3], 0.0, C[..., :3]), 0.0, COLOUR_CLAMP)
        rgb = cc * (1.0 - ge) + fog_colour * gi
    out = np.where(fogged[..., None], rgb, C[..., :3])
    if details is not None:
        details.update(fogged=fogged, cc=cc, F=fog_colour, ge=ge, gi=gi)
    return out, fogged
