"""Two statements of include/strolle_hip.h "light shafts", written independently of each other.

`shafts_f32` is the numpy restatement: float32, one operation per stated operation, in the header's order; visibility comes from the
`occluded` callable, which is handed StRay records (geometry_extremes.RAY_DTYPE) and answers one bool per ray — the checker's occlusion
probe, an engine's st_scene_occluded, or walk_ref's brute force. Given those bits both builds match it bit for bit.

`shafts_f64` is the definition in float64: the same stratified single-scattering sum with numpy's exp, sqrt and arccos, no restated
polynomial, visibility by brute force over all triangles (walk_ref.trace), whose per-ray decision margin says which cells are ambiguous."""
import numpy as np

from fog_ref import exp_
from geometry_extremes import RAY_DTYPE
from ref_num import COLOUR_CLAMP, FLT_MAX, clamp01, max2, min2  # noqa: F401  (re-exported)

F = np.float32
FOLLOW_SUN, LIGHT_EXTINCTION = 1, 2
BAYER = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], np.float32)
JITTER = ((BAYER + F(0.5)) / F(16)).astype(np.float32)   # [cy & 3][cx & 3]
PI32 = F(3.14159265358979323846)


def acos_approx(v):
    """glam's acos_approx as the header states it"""
    v = np.asarray(v, np.float32)
    x = np.abs(v)
    omx = (F(1) - x).astype(np.float32)
    omx = np.where(omx < 0, F(0), omx).astype(np.float32)
    root = np.sqrt(omx).astype(np.float32)
    r = F(-0.0012624911) * x + F(0.0066700901)
    for sign, c in ((-1, 0.0170881256), (1, 0.0308918810), (-1, 0.0501743046), (1, 0.0889789874), (-1, 0.2145988016), (1, 1.5707963050)):
        r = (r * x + F(c)) if sign > 0 else (r * x - F(c))
    r = (r * root).astype(np.float32)
    return np.where(v >= 0, r, PI32 - r).astype(np.float32)


def sun_on(d):
    return any(float(v) != 0.0 for v in d.sun_color)


def host_constants(d, sun=None):
    """(k1, k2, k3, L) as float32: computed in double from the float32 fields, rounded once"""
    g = float(F(d.anisotropy))
    k1, k2, k3 = F((1.0 - g * g) / (4.0 * np.pi)), F(1.0 + g * g), F(2.0 * g)
    L = None
    if sun_on(d):
        v = np.array([float(F(x)) for x in (sun if (d.flags & FOLLOW_SUN) else d.sun_direction)], np.float64)
        n = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        if n > 0:
            L = (v / n).astype(np.float32)
    return k1, k2, k3, L


def table_light(light):
    """an api.Light as the light table holds it: (kind 1 point / 2 spot, centre, radius, colour, range, (ex, ey) the encoded direction, angle)"""
    kind = 1 if light.kind == 0 else 2
    e = (F(0), F(0))
    if kind == 2:
        n = np.array(light.direction, np.float32)
        s = (np.abs(n[0]) + np.abs(n[1])) + np.abs(n[2])
        n = (n / s).astype(np.float32)
        if n[2] >= 0:
            ex, ey = n[0], n[1]
        else:
            ex, ey = np.copysign(F(1) - np.abs(n[1]), n[0]), np.copysign(F(1) - np.abs(n[0]), n[1])
        e = (F(ex * F(0.5) + F(0.5)), F(ey * F(0.5) + F(0.5)))
    return dict(kind=kind, centre=np.array(light.position, np.float32), radius=F(light.radius), colour=np.array(light.color, np.float32), range=F(light.range), e=e,
                angle=F(light.angle))


def cell_rays(transform, projection, w, h, divisor, cw, ch):
    """step 1's ray of every cell: three (ch, cw) float32 arrays"""
    M, P = np.asarray(transform, np.float32).reshape(16), np.asarray(projection, np.float32).reshape(16)
    cx, cy = np.meshgrid(np.arange(cw, dtype=np.uint32), np.arange(ch, dtype=np.uint32))
    fx = (cx * np.uint32(divisor)).astype(np.float32) + F(0.5) * F(divisor)
    fy = (cy * np.uint32(divisor)).astype(np.float32) + F(0.5) * F(divisor)
    ndc_x = fx * F(2) / F(w) - F(1)
    ndc_y = -(fy * F(2) / F(h) - F(1))
    ax, ay = (ndc_x + P[8]) / P[0], (ndc_y + P[9]) / P[5]
    c = F(1) / np.sqrt((ax * ax + ay * ay) + F(1)).astype(np.float32)
    vx, vy, vz = ax * c, ay * c, -c
    return [(M[i] * vx + M[4 + i] * vy + M[8 + i] * vz).astype(np.float32) for i in range(3)]


def cell_depth(D, divisor):
    """(d_c, any valid) per cell: the checkerboard min / max over the block's pixels with D > 0"""
    D = np.asarray(D, np.float32)
    h, w = D.shape
    ch, cw = (h + divisor - 1) // divisor, (w + divisor - 1) // divisor
    with np.errstate(invalid="ignore"):
        valid = D > 0
    lo = np.full((ch * divisor, cw * divisor), np.inf, np.float32); hi = np.full_like(lo, -np.inf)
    lo[:h, :w] = np.where(valid, D, np.inf); hi[:h, :w] = np.where(valid, D, -np.inf)
    lo = lo.reshape(ch, divisor, cw, divisor).min((1, 3)); hi = hi.reshape(ch, divisor, cw, divisor).max((1, 3))
    anyv = np.zeros((ch * divisor, cw * divisor), bool); anyv[:h, :w] = valid
    anyv = anyv.reshape(ch, divisor, cw, divisor).any((1, 3))
    cx, cy = np.meshgrid(np.arange(cw), np.arange(ch))
    d_c = np.where(((cx + cy) & 1) == 1, hi, lo)
    return np.where(anyv, d_c, F(0)).astype(np.float32), anyv


def _phase(k1, k2, k3, c):
    q = (k2 - k3 * c).astype(np.float32)
    return (k1 / (q * np.sqrt(q).astype(np.float32)).astype(np.float32)).astype(np.float32)


def _rays(o, t_max, d):
    r = np.zeros(len(t_max), RAY_DTYPE)
    r["origin"] = o; r["t_max"] = t_max; r["direction"] = d
    return r


def march_f32(depth, transform, projection, d, lights, occluded, sun=None, details=None):
    """steps 1 and 2: the (ch, cw, 4) cell plane and the number of shadow rays. `lights`: table_light dicts of the handles that name a light."""
    D = np.asarray(depth, np.float32)
    h, w = D.shape
    div, steps = int(d.divisor), int(d.steps)
    ch, cw = (h + div - 1) // div, (w + div - 1) // div
    k1, k2, k3, L = host_constants(d, sun)
    M = np.asarray(transform, np.float32).reshape(16)
    density, max_d = F(d.density), F(d.max_distance)
    cells = np.zeros((ch, cw, 4), np.float32)
    n_rays = 0
    log = [] if details is not None else None
    with np.errstate(all="ignore"):
        d_c, live = cell_depth(D, div)
        wv = cell_rays(M, projection, w, h, div, cw, ch)
        idx = np.nonzero(live.reshape(-1))[0]
        wx, wy, wz = (a.reshape(-1)[idx] for a in wv)
        dc = d_c.reshape(-1)[idx]
        cyy, cxx = np.divmod(idx, cw)
        j = JITTER[cyy & 3, cxx & 3]
        d_end = min2(dc, max_d)
        delta = (d_end / F(steps)).astype(np.float32)
        n = len(idx)
        sun_e = None
        if L is not None:
            c = min2(max2((wx * L[0] + wy * L[1]) + wz * L[2], F(-1)), F(1))
            ph = _phase(k1, k2, k3, c)
            sun_e = np.stack([F(d.sun_color[i]) * ph for i in range(3)], -1).astype(np.float32)
            sun_cast = (sun_e != 0).any(-1)
        S = np.zeros((n, 3), np.float32)
        for k in range(steps):
            t = ((F(k) + j) * delta).astype(np.float32)
            p = np.stack([(M[12 + i] + wcomp * t).astype(np.float32) for i, wcomp in enumerate((wx, wy, wz))], -1)
            A = np.zeros((n, 3), np.float32)
            if sun_e is not None and sun_cast.any():
                sel = np.nonzero(sun_cast)[0]
                rays = _rays(p[sel], np.full(len(sel), FLT_MAX, np.float32), np.broadcast_to(L, (len(sel), 3)))
                occ = np.asarray(occluded(rays), bool)
                n_rays += len(sel)
                if log is not None:
                    log.append((idx[sel], k, -1, rays, occ))
                lit = sel[~occ]
                A[lit] = (A[lit] + sun_e[lit]).astype(np.float32)
            for li, l in enumerate(lights):
                v = (l["centre"][None, :] - p).astype(np.float32)
                l2 = ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(np.float32)
                ln = np.sqrt(l2).astype(np.float32)
                outside = ln > l["radius"]
                dirn = (v / ln[:, None]).astype(np.float32)
                f_angle = np.ones(n, np.float32)
                if l["kind"] != 1:
                    ex, ey = l["e"][0] * F(2) - F(1), l["e"][1] * F(2) - F(1)
                    nz = (F(1) - np.abs(ex)) - np.abs(ey)
                    tt = max2(-nz, F(0))
                    nx, ny = F(ex - np.copysign(tt, ex)), F(ey - np.copysign(tt, ey))
                    nz = F(nz)
                    u = -v
                    n2 = F(F(nx * nx + ny * ny) + nz * nz)
                    cosang = (((nx * u[:, 0] + ny * u[:, 1]) + nz * u[:, 2]).astype(np.float32) / np.sqrt((n2 * l2).astype(np.float32)).astype(np.float32)).astype(np.float32)
                    r = (acos_approx(cosang) / l["angle"]).astype(np.float32)
                    f_angle = clamp01(F(1) - (r * r) * r)
                f_dist = np.ones(n, np.float32)
                if l["range"] != np.inf:
                    inv_r2 = F(F(1) / F(l["range"] * l["range"]))
                    f = (l2 * inv_r2).astype(np.float32)
                    sm = clamp01(F(1) - f * f)
                    f_dist = ((sm * sm).astype(np.float32) / max2(l2, F(0.0001))).astype(np.float32)
                fe = (f_angle * f_dist).astype(np.float32)
                if d.flags & LIGHT_EXTINCTION:
                    fe = (fe * exp_(-(density * ln))).astype(np.float32)
                c = min2(max2((wx * dirn[:, 0] + wy * dirn[:, 1]) + wz * dirn[:, 2], F(-1)), F(1))
                ph = _phase(k1, k2, k3, c)
                e = np.stack([((l["colour"][i] * fe).astype(np.float32) * ph).astype(np.float32) for i in range(3)], -1)
                cast = outside & ~((e == 0).all(-1))
                sel = np.nonzero(cast)[0]
                if len(sel) == 0:
                    continue
                rays = _rays(p[sel], (ln[sel] - l["radius"]).astype(np.float32), dirn[sel])
                occ = np.asarray(occluded(rays), bool)
                n_rays += len(sel)
                if log is not None:
                    log.append((idx[sel], k, li, rays, occ))
                lit = sel[~occ]
                A[lit] = (A[lit] + e[lit]).astype(np.float32)
            m = ((exp_(-(density * t)) * delta).astype(np.float32) * density).astype(np.float32)
            for i in range(3):
                S[:, i] = (S[:, i] + (m * F(d.scatter[i])).astype(np.float32) * A[:, i]).astype(np.float32)
        S = min2(max2(S, F(0)), F(FLT_MAX))
        flat = cells.reshape(-1, 4)
        flat[idx, :3] = S
        flat[idx, 3] = dc
    if details is not None:
        details.update(d_c=d_c, live=live, w=wv, log=log, k=(k1, k2, k3), L=L)
    return cells, n_rays


def apply_f32(color, depth, cells, d):
    """step 3"""
    C = np.asarray(color, np.float32)
    D = np.asarray(depth, np.float32)
    h, w = D.shape
    ch, cw = cells.shape[:2]
    max_d = F(d.max_distance)
    with np.errstate(all="ignore"):
        if int(d.divisor) == 1:
            Sp = cells[..., :3].copy()
        else:
            x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
            ux, uy = (x + F(0.5)) * F(0.5) - F(0.5), (y + F(0.5)) * F(0.5) - F(0.5)
            flx, fly = np.floor(ux), np.floor(uy)
            fx, fy = (ux - flx).astype(np.float32), (uy - fly).astype(np.float32)
            ix, iy = flx.astype(np.int64), fly.astype(np.int64)
            d_p = min2(D, max_d)
            Sp = np.zeros((h, w, 3), np.float32); total = np.zeros((h, w), np.float32)
            for k in range(4):
                qx, qy = np.clip(ix + (k & 1), 0, cw - 1), np.clip(iy + (k >> 1), 0, ch - 1)
                c = cells[qy, qx]
                live = c[..., 3] > 0
                b = ((fx if k & 1 else F(1) - fx) * (fy if k >> 1 else F(1) - fy)).astype(np.float32)
                ratio = (np.abs(min2(c[..., 3], max_d) - d_p).astype(np.float32) / d_p).astype(np.float32)
                wgt = (b * (F(1) / (F(0.001) + ratio)).astype(np.float32)).astype(np.float32)
                for i in range(3):
                    Sp[..., i] = np.where(live, (Sp[..., i] + wgt * c[..., i]).astype(np.float32), Sp[..., i])
                total = np.where(live, (total + wgt).astype(np.float32), total)
            ok = total > 0
            Sp = np.where(ok[..., None], (Sp / np.where(ok, total, F(1))[..., None]).astype(np.float32), F(0)).astype(np.float32)
        add = (F(d.intensity) * Sp).astype(np.float32)
        changed = (D > 0) & ~((add == 0).all(-1))
        cc = min2(max2(C[..., :3], F(0)), F(COLOUR_CLAMP))
        rgb = min2((cc + add).astype(np.float32), F(FLT_MAX))
    out = C.copy()
    out[changed, :3] = rgb[changed]
    return out, changed


def shafts_f32(color, depth, transform, projection, d, lights, occluded, sun=None, details=None):
    """(h, w, 4) colours and (h, w) distances -> ((h, w, 4) behind the node, the number of shadow rays)"""
    cells, n_rays = march_f32(depth, transform, projection, d, lights, occluded, sun, details)
    out, changed = apply_f32(color, depth, cells, d)
    if details is not None:
        details.update(cells=cells, changed=changed)
    return out, n_rays


# ---------------------------------------------------------------- the definition
def march_f64(depth, transform, projection, d, lights, triangles, sun=None):
    """the cell plane's S in float64 and, per cell, the smallest decision margin of its shadow rays (brute force over `triangles`,
    read_scene(1) records). Which rays are cast follows the definition's own E phase."""
    import walk_ref
    D = np.asarray(depth, np.float32)
    h, w = D.shape
    div, steps = int(d.divisor), int(d.steps)
    ch, cw = (h + div - 1) // div, (w + div - 1) // div
    recs = walk_ref.records(triangles)
    M = np.asarray(transform, np.float32).astype(np.float64).reshape(4, 4).T
    P = np.asarray(projection, np.float32).astype(np.float64).reshape(16)
    g = float(F(d.anisotropy)); sigma = float(F(d.density)); max_d = float(F(d.max_distance))

    def phase(c):
        return (1.0 - g * g) / (4.0 * np.pi) / np.power(1.0 + g * g - 2.0 * g * c, 1.5)

    def visible(o, tmax, dirn):
        a = walk_ref.trace(*recs, _rays(o.astype(np.float32), tmax.astype(np.float32), dirn.astype(np.float32)))
        return ~a.occluded, a.decision_margin

    d_c, live = cell_depth(D, div)
    S = np.zeros((ch, cw, 3)); margin = np.full((ch, cw), np.inf)
    idx = np.nonzero(live.reshape(-1))[0]
    cyy, cxx = np.divmod(idx, cw)
    px, py = cxx * div + 0.5 * div, cyy * div + 0.5 * div
    ax = ((2.0 * px / w - 1.0) + P[8]) / P[0]; ay = (-(2.0 * py / h - 1.0) + P[9]) / P[5]
    view = np.stack([ax, ay, -np.ones_like(ax)], -1) / np.sqrt(ax * ax + ay * ay + 1.0)[:, None]
    wd = view @ M[:3, :3].T
    o = M[:3, 3]
    d_end = np.minimum(d_c.reshape(-1)[idx].astype(np.float64), max_d)
    delta = d_end / steps
    j = JITTER[cyy & 3, cxx & 3].astype(np.float64)
    acc = np.zeros((len(idx), 3)); mar = np.full(len(idx), np.inf)
    Ls = None
    if sun_on(d):
        v = np.array([float(F(x)) for x in (sun if (d.flags & FOLLOW_SUN) else d.sun_direction)], np.float64)
        Ls = v / np.linalg.norm(v)
    with np.errstate(all="ignore"):
        for k in range(steps):
            t = (k + j) * delta
            p = o[None] + wd * t[:, None]
            A = np.zeros((len(idx), 3))
            if Ls is not None:
                e = np.array([float(F(x)) for x in d.sun_color])[None] * phase(np.clip(wd @ Ls, -1, 1))[:, None]
                vis, m = visible(p, np.full(len(idx), FLT_MAX), np.broadcast_to(Ls, p.shape))
                A += e * vis[:, None]; mar = np.minimum(mar, m)
            for l in lights:
                v = l["centre"].astype(np.float64)[None] - p
                ln = np.linalg.norm(v, axis=1)
                dirn = v / ln[:, None]
                fa = np.ones(len(idx))
                if l["kind"] != 1:
                    ex, ey = float(l["e"][0]) * 2 - 1, float(l["e"][1]) * 2 - 1
                    nz = 1 - abs(ex) - abs(ey); tt = max(-nz, 0.0)
                    nrm = np.array([ex - np.copysign(tt, ex), ey - np.copysign(tt, ey), nz]); nrm /= np.linalg.norm(nrm)
                    ang = np.arccos(np.clip(-(dirn @ nrm), -1, 1))
                    fa = np.clip(1 - (ang / float(l["angle"])) ** 3, 0, 1)
                fd = np.ones(len(idx))
                if l["range"] != np.inf:
                    f = ln * ln / float(l["range"]) ** 2
                    fd = np.clip(1 - f * f, 0, 1) ** 2 / np.maximum(ln * ln, 1e-4)
                fe = fa * fd
                if d.flags & LIGHT_EXTINCTION:
                    fe = fe * np.exp(-sigma * ln)
                e = l["colour"].astype(np.float64)[None] * (fe * phase(np.clip(np.einsum("ij,ij->i", wd, dirn), -1, 1)))[:, None]
                cast = (ln > float(l["radius"])) & (e != 0).any(-1)
                sel = np.nonzero(cast)[0]
                if len(sel):
                    vis, m = visible(p[sel], ln[sel] - float(l["radius"]), dirn[sel])
                    A[sel] += e[sel] * vis[:, None]; mar[sel] = np.minimum(mar[sel], m)
            acc += (np.exp(-sigma * t) * delta * sigma)[:, None] * np.array([float(F(x)) for x in d.scatter])[None] * A
    S.reshape(-1, 3)[idx] = acc
    margin.reshape(-1)[idx] = mar
    return S, d_c, margin


def shafts_f64(color, depth, transform, projection, d, lights, triangles, sun=None):
    """((h, w, 3) in float64, the mask of pixels every one of whose cells is unambiguous at `threshold` is the caller's: per-cell margins are returned)"""
    S, d_c, margin = march_f64(depth, transform, projection, d, lights, triangles, sun)
    C = np.asarray(color, np.float32).astype(np.float64)
    D = np.asarray(depth, np.float32).astype(np.float64)
    h, w = D.shape
    ch, cw = S.shape[:2]
    max_d = float(F(d.max_distance))
    pix_margin = np.full((h, w), np.inf)
    with np.errstate(all="ignore"):
        if int(d.divisor) == 1:
            Sp = S.copy(); pix_margin = margin.copy()
        else:
            x, y = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
            ux, uy = x * 0.5 - 0.5, y * 0.5 - 0.5
            ix, iy = np.floor(ux).astype(int), np.floor(uy).astype(int)
            fx, fy = ux - ix, uy - iy
            d_p = np.minimum(D, max_d)
            Sp = np.zeros((h, w, 3)); total = np.zeros((h, w))
            for k in range(4):
                qx, qy = np.clip(ix + (k & 1), 0, cw - 1), np.clip(iy + (k >> 1), 0, ch - 1)
                di = d_c[qy, qx].astype(np.float64)
                wgt = (fx if k & 1 else 1 - fx) * (fy if k >> 1 else 1 - fy) / (1e-3 + np.abs(np.minimum(di, max_d) - d_p) / d_p)
                wgt = np.where(di > 0, wgt, 0.0)
                Sp += wgt[..., None] * S[qy, qx]; total += wgt
                pix_margin = np.minimum(pix_margin, np.where(wgt > 0, margin[qy, qx], np.inf))
            Sp = np.where((total > 0)[..., None], Sp / np.where(total > 0, total, 1.0)[..., None], 0.0)
        add = float(F(d.intensity)) * Sp
        changed = (D > 0) & (add != 0).any(-1)
        cc = np.clip(np.where(C[..., :3] != C[..., :3], 0.0, C[..., :3]), 0.0, COLOUR_CLAMP)
    return np.where(changed[..., None], cc + add, C[..., :3]), pix_margin
