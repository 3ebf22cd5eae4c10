"""A tree-free float64 restatement of the ray queries: of ALL triangles, which one does this ray hit first?

Every traversal test elsewhere compares a walk with another walk over the same kind of tree. This module builds no tree. It takes the engine's own
world-space triangles (read_scene(1): float32 vertices as the engine baked them, so no transform arithmetic is second-guessed) and float32 StRay
records, and restates Triangle::hit (strolle-gpu/src/triangle.rs:64-113) in float64 over all triangles at once, in the contract's order:

    e1 = p1 - p0, e2 = p2 - p0          (float32, as the hit test forms them; everything after is float64)
    det = e1 . (d x e2);  |det| < f32 epsilon -> miss
    u, v;  u < 0 | u > 1 | v < 0 | u + v > 1 -> miss
    t <= 0 -> miss;  closest t below t_max wins
    an all-zero direction, t_max <= 0 and a NaN t_max are misses.  Blend / alpha materials are out of scope: every material is opaque.

Besides the answer it returns a float64 MARGIN per ray that says how close the decision was; a ray whose margin is below a threshold is ambiguous:
float32 arithmetic may legitimately decide it the other way. The margin is the smallest of these dimensionless quantities:
    the distance of (u, v, 1 - u - v) of the winner from 0;                         | |det| - eps | / eps of the winner;
    t |d| / |origin - p0| and |t - t_max| / t of the winner;                           the cosine between the ray and the winner's plane (grazing hits);
    the distance from acceptance of every rejected triangle that would otherwise have won;
    the relative gap in t to the runner-up (`decision_margin` leaves it out, see `Answer`)."""
from dataclasses import dataclass

import numpy as np

F32_EPS = float(np.float32(1.1920929e-07))
F32_MAX = float(np.float32(3.4028235e38))
CHUNK_BYTES = 48 << 20          # per float64 [rays, triangles, 3] temporary: 4,096 rays x 1,200 triangles stay under a few hundred MB in all


@dataclass
class Answer:
    hit: np.ndarray          # bool: closest hit with 0 < t < t_max
    t: np.ndarray            # float64, inf on a miss
    slot: np.ndarray         # int64 triangle slot of the winner (index into the records), -1 on a miss
    uv: np.ndarray           # float64 (n, 2): barycentric (u, v) of the winner, 0 on a miss
    point: np.ndarray        # float64 (n, 3): origin + t * direction, 0 on a miss
    occluded: np.ndarray     # bool: any hit with len = t_max (the same decision as `hit`, restated for the any-hit query)
    margin: np.ndarray       # float64: min of every quantity above
    decision_margin: np.ndarray   # float64: the same without the runner-up gap: hit / miss, t and occlusion do not depend on WHICH of two tied triangles wins


def records(triangles: np.ndarray):
    """read_scene(1) (144 B per triangle) -> the hit-test records (p0, e1, e2), float32 as Triangle::hit forms them."""
    tri = np.ascontiguousarray(triangles).view(np.float32).reshape(-1, 9, 4)[:, [0, 3, 6], :3]
    p0 = tri[:, 0].copy()
    return p0, (tri[:, 1] - tri[:, 0]).astype(np.float32), (tri[:, 2] - tri[:, 0]).astype(np.float32)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def trace(p0, e1, e2, rays) -> Answer:
    """Closest hit and occlusion of every ray (StRay records) against every triangle (float32 p0, e1, e2 of `records`)."""
    P0, E1, E2 = (np.asarray(a, np.float32).astype(np.float64) for a in (p0, e1, e2))
    n_tri, n = len(P0), len(rays)
    O = rays["origin"].astype(np.float64); D = rays["direction"].astype(np.float64); TM = rays["t_max"].astype(np.float64)
    area2 = np.linalg.norm(_cross(E1, E2), axis=1)
    out = Answer(np.zeros(n, bool), np.full(n, np.inf), np.full(n, -1, np.int64), np.zeros((n, 2)), np.zeros((n, 3)), np.zeros(n, bool),
                 np.full(n, np.inf), np.full(n, np.inf))
    valid = (TM > 0) & np.any(D != 0, axis=1)        # NaN t_max: the comparison is False
    if n_tri == 0:
        return out
    step = max(1, CHUNK_BYTES // (n_tri * 24))
    for a in range(0, n, step):
        s = slice(a, min(n, a + step))
        o, d, tm = O[s, None, :], D[s, None, :], TM[s, None]
        with np.errstate(all="ignore"):
            pvec = _cross(d, E2[None]); det = _dot(E1[None], pvec)
            tvec = o - P0[None]; qvec = _cross(tvec, E1[None])
            u = _dot(tvec, pvec) / det; v = _dot(d, qvec) / det; t = _dot(E2[None], qvec) / det
            ok = ~(np.abs(det) < F32_EPS) & ~((u < 0) | (u > 1) | (v < 0) | (u + v > 1) | (t <= 0)) & (t < tm) & valid[s, None]
            dlen = np.linalg.norm(d, axis=-1)
            # the criteria of acceptance, each dimensionless and positive where it holds
            crit = np.minimum.reduce([(np.abs(det) - F32_EPS) / F32_EPS, u, v, 1.0 - u - v, t * dlen / np.linalg.norm(tvec, axis=-1), (tm - t) / np.abs(t) + np.zeros_like(t)])
            crit = np.where(np.isnan(crit), -1.0, crit)      # det == 0: u, v, t are NaN / inf; such a triangle is at least the whole cutoff from a hit
            graze = np.abs(det) / (area2[None] * dlen)
        tk = np.where(ok, t, np.inf)
        win = np.argmin(tk, axis=1); rows = np.arange(tk.shape[0])
        t1 = tk[rows, win]; hit = np.isfinite(t1)
        tk2 = tk.copy(); tk2[rows, win] = np.inf
        t2 = tk2.min(axis=1)
        with np.errstate(all="ignore"):
            gap = np.where(hit & np.isfinite(t2), (t2 - t1) / t1, np.inf)
            # a rejected triangle matters only where accepting it would change the answer: in front of the winner (or of t_max when nothing is hit)
            could_win = ~ok & ~(t >= t1[:, None]) & valid[s, None]
            near_miss = np.where(could_win, -crit, np.inf).min(axis=1)
        m_win = np.where(hit, np.minimum(crit[rows, win], graze[rows, win]), np.inf)
        decision = np.minimum(m_win, near_miss)
        out.hit[s] = hit; out.t[s] = t1; out.slot[s] = np.where(hit, win, -1)
        out.uv[s] = np.where(hit[:, None], np.stack([u[rows, win], v[rows, win]], -1), 0.0)
        out.point[s] = np.where(hit[:, None], O[s] + D[s] * np.where(hit, t1, 0.0)[:, None], 0.0)
        out.decision_margin[s] = decision; out.margin[s] = np.minimum(decision, gap)
    out.occluded = out.hit.copy()
    return out
