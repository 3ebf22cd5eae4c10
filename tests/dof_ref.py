"""Numpy restatement of include/strolle_hip.h "depth of field": the host constants, planar depth, focus, pack, the near-field tile maximum,
the neighbour maximum and the gather. Everything per pixel is float32, evaluated in the header's order; min, max and clamp01 follow the
post-processing section's NaN rule. The tap table is the library's (st_dof_plan): the last bit of a libm's and of numpy's cos may differ,
so `taps_double` below is only what that table is checked against, to within one float ulp."""
import numpy as np

from ref_num import COLOUR_CLAMP, FLT_MAX, clamp01, colour, frame_depth, max2, min2  # noqa: F401  (re-exported)

F = np.float32
AUTOFOCUS, PLANAR_DEPTH = 1, 2
TILE, DEFAULT_SAMPLES, DEFAULT_RADIUS, DEFAULT_STOPS, DEFAULT_SENSOR = 32, 32, 32.0, 1.0, 0.01866
GOLDEN_ANGLE = 2.399963229728653


def taps_double(samples):
    """the tap table in numpy's own double arithmetic: (S, 3) float64 of (rho cos th, rho sin th, rho)"""
    k = np.arange(samples, dtype=np.float64)
    rho, th = np.sqrt((k + 0.5) / samples), k * GOLDEN_ANGLE
    return np.stack([rho * np.cos(th), rho * np.sin(th), rho], -1)


def constants(projection, height, aperture_f_stops=0.0, sensor_height=0.0):
    """step 0: (f, K) as float32, computed in double from the float32 fields"""
    hs = float(F(sensor_height)) if F(sensor_height) != 0 else float(F(DEFAULT_SENSOR))
    n = float(F(aperture_f_stops)) if F(aperture_f_stops) != 0 else float(F(DEFAULT_STOPS))
    f = 0.5 * hs * float(F(projection[5]))
    k = 0.5 * f * f / (n * hs) * float(height)
    return F(f), F(k)


def planar(depth, projection, flags=0):
    """step 1: (h, w) distances along the rays -> Z along the optical axis"""
    D = np.asarray(depth, np.float32)
    h, w = D.shape
    P = np.asarray(projection, np.float32).reshape(16)
    with np.errstate(all="ignore"):
        if flags & PLANAR_DEPTH:
            z = D.copy()
        else:
            x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
            ndc_x = (x + F(0.5)) * F(2) / F(w) - F(1)
            ndc_y = -((y + F(0.5)) * F(2) / F(h) - F(1))
            ax, ay = (ndc_x + P[8]) / P[0], (ndc_y + P[9]) / P[5]
            c = F(1) / np.sqrt((ax * ax + ay * ay) + F(1)).astype(np.float32)
            z = (D * c).astype(np.float32)
        return np.where(D >= FLT_MAX, FLT_MAX, z).astype(np.float32)


def focus(z, f, K, focal_distance, flags=0, focus_x=0.0, focus_y=0.0):
    """step 2: (s, A)"""
    h, w = z.shape
    s = F(focal_distance)
    if flags & AUTOFOCUS:
        px = min(int(np.floor(F(focus_x) * F(w))), w - 1)
        py = min(int(np.floor(F(focus_y) * F(h))), h - 1)
        zf = z[py, px]
        if zf > 0 and zf < FLT_MAX:
            s = F(zf)
    m = max2(F(s - F(f)), F(1e-6))
    with np.errstate(all="ignore"):
        return s, F(F(K) / m)


def pack(z, s, A, max_radius=0.0):
    """step 3: the signed circle of confusion, in pixels"""
    R = F(max_radius) if F(max_radius) != 0 else F(DEFAULT_RADIUS)
    with np.errstate(all="ignore"):
        coc = np.where(z > 0, A * (F(1) - s / np.where(z > 0, z, F(1))), F(0)).astype(np.float32)
    return min2(max2(coc, -R), R)


def tile_max(coc):
    """step 4: (ty, tx) the largest -coc over each tile's pixels with coc < 0, 0 when there is none"""
    h, w = coc.shape
    ty, tx = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
    near = np.where(coc < 0, -coc, F(0)).astype(np.float32)
    out = np.zeros((ty, tx), np.float32)
    for j in range(ty):
        for i in range(tx):
            out[j, i] = near[j * TILE:(j + 1) * TILE, i * TILE:(i + 1) * TILE].max()
    return out


def neighbour_max(tiles):
    """step 5"""
    ty, tx = tiles.shape
    out = np.zeros_like(tiles)
    for j in range(ty):
        for i in range(tx):
            out[j, i] = tiles[max(j - 1, 0):j + 2, max(i - 1, 0):i + 2].max()
    return out


def gather(color, coc, z, nb, taps, details=None):
    """step 6: color (h, w, 3 or 4), the packed coc and Z (h, w), nb = neighbour_max(...), taps (S, 3) float32 -> (h, w, 4)"""
    C = np.asarray(color, np.float32)
    T = np.asarray(taps, np.float32)
    h, w = coc.shape
    n = np.repeat(np.repeat(nb, TILE, 0), TILE, 1)[:h, :w]
    rx = np.abs(coc)
    rg = max2(rx, n)
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    fx, fy = x + F(0.5), y + F(0.5)
    with np.errstate(all="ignore"):
        c0 = colour(C)
        acc = c0.copy()
        wsum = np.ones((h, w), np.float32)
        seen = []
        for k in range(T.shape[0]):
            px, py = fx + T[k, 0] * rg, fy + T[k, 1] * rg
            yx = min2(max2(np.floor(px), F(0)), F(w - 1)).astype(np.int64)
            yy = min2(max2(np.floor(py), F(0)), F(h - 1)).astype(np.int64)
            d = T[k, 2] * rg
            ry = np.abs(coc[yy, yx])
            ry = np.where(z[yy, yx] > z, min2(ry, rx), ry).astype(np.float32)
            q = clamp01((ry - d) + F(0.5))
            wt = (q * q * (F(3) - F(2) * q)).astype(np.float32)
            acc = acc + c0[yy, yx] * wt[..., None]
            wsum = wsum + wt
            seen.append((yx, yy, wt))
        res = acc / wsum[..., None]
    if details is not None:
        details.update(taps=seen, wsum=wsum, r_g=rg)
    out = np.concatenate([res, np.ones((h, w, 1), np.float32)], -1).astype(np.float32)
    sharp = rg < F(0.5)
    src = C if C.shape[-1] == 4 else np.concatenate([C, np.ones((h, w, 1), np.float32)], -1)
    out[sharp] = src[sharp]
    return out


def dof(color, depth, projection, taps, focal_distance=10.0, aperture_f_stops=0.0, sensor_height=0.0, max_radius=0.0, flags=0, focus_x=0.0, focus_y=0.0,
        details=None):
    """(h, w, 4) composed colours and (h, w) distances along the rays, rendered with `projection` (16 floats, column major) -> (h, w, 4) in
    front of motion blur / bloom / the display transform. `taps`: st_dof_plan's table."""
    D = np.asarray(depth, np.float32)
    f, K = constants(projection, D.shape[0], aperture_f_stops, sensor_height)
    z = planar(D, projection, flags)
    s, A = focus(z, f, K, focal_distance, flags, focus_x, focus_y)
    coc = pack(z, s, A, max_radius)
    tiles = tile_max(coc)
    nb = neighbour_max(tiles)
    if details is not None:
        details.update(f=f, K=K, z=z, s=s, A=A, coc=coc, tiles=tiles, neighbours=nb)
    return gather(color, coc, z, nb, taps, details)


def dof_desc(color, depth, projection, taps, d, details=None):
    """`dof` with a StDofDesc's fields"""
    return dof(color, depth, projection, taps, d.focal_distance, d.aperture_f_stops, d.sensor_height, d.max_radius, d.flags, d.focus_x, d.focus_y, details)
