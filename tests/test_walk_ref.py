"""tests/walk_ref.py — the tree-free float64 restatement of the ray queries — at cases worked out by hand, and against the oracle (or_probe_trace_rays,
on the CPU) for every family, size and ray set of tests/geometry_extremes.py.

The second part is where the two numbers of profiles/geometry_extremes.json are pinned that the GPU tests (tests/test_gpu_geometry_extremes.py) read:
the ambiguity threshold and the t tolerance of each family. Both are measured against the oracle — the reference side — by
tools/geometry_extremes_profile.py, never against a HIP build; this file asserts that the committed figures are what that measurement gives, and the
CONDITION that keeps the threshold honest: at most 2 % of a family's rays ambiguous, at least 10 % non-ambiguous hits. A threshold that grew to
swallow a GPU failure would fail here, without a GPU."""
import importlib.util
import os

import numpy as np
import pytest

import geometry_extremes as gx
import walk_ref
from strolle_amd import Engine
from strolle_amd.api import RAY_DTYPE

EPS = walk_ref.F32_EPS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("geometry_extremes_profile", os.path.join(ROOT, "tools", "geometry_extremes_profile.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def _rays(rows):
    """rows of (origin, direction, t_max)"""
    r = np.zeros(len(rows), RAY_DTYPE)
    for i, (o, d, t) in enumerate(rows):
        r["origin"][i] = o; r["direction"][i] = d; r["t_max"][i] = t
    return r


def _trace(tri, rows):
    """one triangle (three vertices) against rays"""
    tri = np.asarray(tri, np.float32)
    return walk_ref.trace(tri[None, 0], (tri[1] - tri[0])[None], (tri[2] - tri[0])[None], _rays(rows))


# the unit right triangle in the plane z = 0: p0 = (0, 0, 0), e1 = (1, 0, 0), e2 = (0, 1, 0); a ray down -z from height 2 through (x, y) has u = x, v = y, t = 2
UNIT = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
INF = np.inf


def _down(x, y, t_max=INF, z=2.0, dz=-1.0):
    return ((x, y, z), (0.0, 0.0, dz), t_max)


def test_interior_edge_vertex_and_just_outside():
    a = _trace(UNIT, [_down(0.25, 0.25), _down(0.5, 0.0), _down(0.5, 0.5), _down(0.0, 0.0), _down(1.0, 0.0), _down(0.0, 1.0),
                      _down(0.5, -1e-6), _down(-1e-6, 0.5), _down(0.5 + 1e-6, 0.5), _down(1.0 + 1e-6, 0.0)])
    assert a.hit.tolist() == [True] * 6 + [False] * 4            # u = 0, v = 0, u + v = 1 and the vertices are hits: the contract rejects u < 0, v < 0, u + v > 1
    assert np.allclose(a.t[:6], 2.0, rtol=1e-15) and np.all(np.isinf(a.t[6:]))
    assert a.slot.tolist() == [0] * 6 + [-1] * 4
    assert np.allclose(a.uv[0], (0.25, 0.25)) and np.allclose(a.uv[2], (0.5, 0.5)) and np.allclose(a.point[0], (0.25, 0.25, 0.0))
    assert np.array_equal(a.occluded, a.hit)
    # the margin: the interior ray is a quarter of the triangle from every edge; the edge and vertex rays are decided by nothing; the misses by 1e-6 (float32 inputs)
    assert a.margin[0] == pytest.approx(0.25)
    assert np.all(a.margin[1:6] == 0.0)
    assert np.all((a.margin[6:] > 0.5e-6) & (a.margin[6:] < 2e-6))
    assert np.all(a.point[6:] == 0) and np.all(a.uv[6:] == 0)


def test_the_det_cutoff_by_scaling_the_triangle_and_by_scaling_the_direction():
    # det = e1 . (d x e2) = -dz * s^2 for the unit triangle scaled by s and d = (0, 0, dz): the cutoff |det| < 2^-23 sits at s = 2^-11.5 for dz = -1
    s_below, s_above = np.float32(2.0 ** -11.5) * np.float32(0.999), np.float32(2.0 ** -11.5) * np.float32(1.001)
    for s, want in ((s_below, False), (s_above, True)):
        tri = np.asarray(UNIT, np.float32) * s
        a = _trace(tri, [_down(0.25 * s, 0.25 * s)])
        det = float(s) ** 2
        assert (det >= EPS) == want and a.hit[0] == want, (s, det)
        assert a.margin[0] == pytest.approx(abs(det - EPS) / EPS, rel=1e-6)          # about 2e-3: the cutoff decides, nothing else is close
    # the same triangle, the direction's length scaled instead: |det| = |dz|. The hit's t scales with 1 / |dz|: t = 2 / |dz|
    below, above = np.float32(EPS) * np.float32(0.99), np.float32(EPS) * np.float32(1.01)
    a = _trace(UNIT, [_down(0.25, 0.25, dz=-below), _down(0.25, 0.25, dz=-above), _down(0.25, 0.25, dz=-np.float32(EPS))])
    assert a.hit.tolist() == [False, True, True]                 # |det| == eps is not below it
    assert a.t[1] == pytest.approx(2.0 / float(above)) and a.margin[2] == 0.0
    assert a.margin[0] == pytest.approx(0.01, rel=1e-3) and a.margin[1] == pytest.approx(0.01, rel=1e-3)


def test_a_ray_that_starts_on_the_plane_a_back_face_and_a_ray_inside_the_plane():
    a = _trace(UNIT, [_down(0.25, 0.25, z=0.0),                       # starts on the triangle's plane: t = 0 is a miss (t <= 0)
                      _down(0.25, 0.25, z=-2.0, dz=1.0),              # from behind: det < 0, still a hit (no culling), t = 2
                      _down(0.25, 0.25, z=-2.0, dz=-1.0),             # pointing away: t = -2
                      ((-1.0, 0.25, 0.0), (1.0, 0.0, 0.0), INF)])     # inside the plane: det = 0
    assert a.hit.tolist() == [False, True, False, False]
    assert a.t[1] == 2.0 and np.allclose(a.uv[1], (0.25, 0.25))
    assert a.margin[0] == 0.0 and a.margin[2] >= 0.25 and a.margin[3] == 1.0      # det = 0 is the whole cutoff away from a hit


def test_t_max_at_below_and_above_the_hit_and_the_rays_that_never_hit():
    a = _trace(UNIT, [_down(0.25, 0.25, 2.0), _down(0.25, 0.25, 1.5), _down(0.25, 0.25, 3.0), _down(0.25, 0.25, np.float32(3.4028235e38)),
                      _down(0.25, 0.25, 0.0), _down(0.25, 0.25, -1.0), _down(0.25, 0.25, np.nan), ((0.25, 0.25, 2.0), (0.0, 0.0, 0.0), INF)])
    assert a.hit.tolist() == [False, False, True, True, False, False, False, False]        # t < t_max: a hit AT t_max is a miss
    assert np.array_equal(a.occluded, a.hit)
    assert a.margin[0] == 0.0 and a.margin[1] == pytest.approx(0.25) and a.margin[2] == pytest.approx(0.25)   # |t - t_max| / t = 0.25 both ways; above: as close as the edges
    assert np.all(np.isinf(a.margin[4:]))                       # misses by contract: nothing about them is close


def test_the_closest_of_several_and_the_gap_to_the_runner_up():
    near = np.asarray(UNIT, np.float32) + np.float32([0, 0, 1.0])       # z = 1: t = 1
    tris = np.stack([np.asarray(UNIT, np.float32), near, near])          # slot 1 and 2 coincide
    p0, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    a = walk_ref.trace(p0, e1, e2, _rays([_down(0.25, 0.25), _down(0.25, 0.25, 1.5)]))
    assert a.hit.all() and np.all(a.t == 1.0) and set(a.slot.tolist()) <= {1, 2}
    assert np.all(a.margin == 0.0) and np.all(a.decision_margin == pytest.approx(0.25))   # WHICH of the two wins is undecided; that one wins, and its t, are not
    b = walk_ref.trace(p0[:2], e1[:2], e2[:2], _rays([_down(0.25, 0.25)]))
    assert b.slot[0] == 1 and b.margin[0] == pytest.approx(0.25)         # runner-up at t = 2: a relative gap of 1


def test_the_work_is_chunked():
    rng = np.random.default_rng(1)
    pos = gx.positions("unit", 600)
    p0, e1, e2 = pos[:, 0], pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]
    rays = gx.make_rays(rng.uniform(-1, 1, (300, 3)), rng.normal(size=(300, 3)), np.full(300, np.inf, np.float32))
    whole = walk_ref.trace(p0, e1, e2, rays)
    old = walk_ref.CHUNK_BYTES
    try:
        walk_ref.CHUNK_BYTES = 600 * 24 * 7          # seven rays at a time
        parts = walk_ref.trace(p0, e1, e2, rays)
    finally:
        walk_ref.CHUNK_BYTES = old
    for f in ("hit", "t", "slot", "uv", "point", "margin", "decision_margin"):
        assert np.array_equal(getattr(whole, f), getattr(parts, f)), f
    assert 4096 * 1200 * 24 <= 32 * walk_ref.CHUNK_BYTES, "4,096 rays x 1,200 triangles must not ask for one temporary of more than 48 MB at a time"


# ----------------------------------------------------------------------------- against the oracle, per family
@pytest.fixture(scope="module")
def profile():
    return gx.load_profile()["cases"]


def test_the_profile_lists_every_case(profile):
    assert sorted(profile) == sorted(gx.case_key(f, n) for f, n in gx.CASES)


@pytest.mark.parametrize("family,n", gx.CASES, ids=[gx.case_key(f, n) for f, n in gx.CASES])
def test_the_engines_bake_the_records_the_family_states(family, n):
    """identity instance transforms: the product's host bake, the oracle's and the float32 positions built in numpy are the same numbers, so the
    restatement's input second-guesses no transform arithmetic"""
    e = Engine(device=-1)
    try:
        pos = gx.build_extreme(e, family, n); e.tick()
        mine = e.read_scene(1).copy()
    finally:
        e.close()
    case = gx.oracle_case(family, n)
    assert np.array_equal(mine.view(np.uint32), case["triangles"].view(np.uint32))
    verts = mine.view(np.float32).reshape(-1, 9, 4)[:, [0, 3, 6], :3]
    assert len(verts) == n and np.array_equal(verts[:len(pos)], pos)
    assert len(case["rays"]) == gx.N_RAYS


@pytest.mark.parametrize("moved", [False, True], ids=["built", "moved"])
@pytest.mark.parametrize("family,n", gx.CASES, ids=[gx.case_key(f, n) for f, n in gx.CASES])
def test_the_oracle_agrees_with_brute_force_beyond_the_threshold(family, n, moved, profile):
    """hit / miss, winning slot and occlusion on every non-ambiguous ray; t and the hit point within the tolerance — for the scene as built and after the
    refit configuration's move. Then the condition: the oracle ALONE leaves at most 2 % of the rays ambiguous and at least 10 % non-ambiguous hits."""
    tool = _tool()
    prof = profile[gx.case_key(family, n)]
    thr, tol = prof["threshold"], prof["t_tolerance"]
    case = gx.oracle_case(family, n, moved)
    ref = case["ref"]; hit, t, slot, point, occ = case["oracle"]
    decision, other = tool.disagreements(case, family)
    print(f"{family}/{n} moved={moved}: {int(decision.sum())} decisions and {int(other.sum())} slots differ; largest margins "
          f"{ref.decision_margin[decision].max(initial=0.0):.3g} / {ref.margin[other].max(initial=0.0):.3g}, threshold {thr:.3g}")
    assert not (decision & (ref.decision_margin >= thr)).any(), "the oracle decides a non-ambiguous ray differently from brute force"
    assert not (other & (ref.margin >= thr)).any(), "the oracle finds another triangle than brute force on a non-ambiguous ray"
    amb_share, hit_share = tool.shares(case, family, thr)
    sure = hit & ref.hit & (ref.decision_margin >= thr)
    dev = np.abs(t[sure].astype(np.float64) - ref.t[sure]) / ref.t[sure]
    pdev = np.abs(point[sure].astype(np.float64) - ref.point[sure]).max(axis=1)
    print(f"  worst t deviation {dev.max():.3g} (x 4 = {4 * dev.max():.3g}, tolerance {tol:.3g}); point {pdev.max() / case['extent']:.3g} of the extent; "
          f"ambiguous {amb_share:.4f}, non-ambiguous hits {hit_share:.4f}")
    assert 4.0 * dev.max() <= tol, "the tolerance in the profile is below 4 x the oracle's own deviation"
    assert np.all(pdev <= tol * case["extent"]), "the oracle's own hit point is outside the tolerance scaled by the extent"
    # the committed figures are the measurement's, not wider: re-measured here, for both scenes at once
    if not moved:
        again = tool.measure(family, n)
        assert prof["threshold"] == again["threshold"] and prof["t_tolerance"] == again["t_tolerance"], (prof["threshold"], again["threshold"], prof["t_tolerance"], again["t_tolerance"])
    # the condition
    assert amb_share <= 0.02, f"{amb_share:.4f} of the rays are ambiguous"
    assert hit_share >= 0.10, f"only {hit_share:.4f} of the rays are non-ambiguous hits"


def test_the_ray_sets_hold_what_they_promise():
    for family in ("unit", "flat_1000", "beyond_f16_neg"):
        case = gx.oracle_case(family, 600)
        r = case["rays"]; d = r["direction"][gx.N_BUNDLE:]; o = r["origin"][gx.N_BUNDLE:]
        zero = np.sum(d == 0, axis=1)
        assert (zero == 3).sum() > 50 and all(((zero == 2) & (d[:, k] != 0)).sum() > 50 for k in range(3)), "axis-parallel and all-zero directions"
        ln = np.linalg.norm(d[zero < 2].astype(np.float64), axis=1)
        assert ln.min() < 0.5 and ln.max() > 3.0, "un-normalised directions"
        lo, hi = case["lo"].astype(np.float64), case["hi"].astype(np.float64)
        outside = np.any((o < lo) | (o > hi), axis=1)
        assert 0.2 < outside.mean() < (0.9 if not family.startswith("flat") else 1.0) and (~outside).sum() > 30, "origins inside the box and outside it"
        t = r["t_max"][gx.N_BUNDLE:]
        assert np.isnan(t).any() and (t == 0).any() and (t < 0).any() and np.isinf(t).any() and (t == gx.FLT_MAX).any() and (np.isfinite(t) & (t > 0) & (t < 1e30)).any()
        assert np.all(r["origin"][:gx.N_BUNDLE] == r["origin"][0]), "the bundle starts at one point"
        if family.startswith("flat"):
            on = (o[:, 1] == case["lo"][1]) & (d[:, 1] == 0) & (zero < 3)
            assert on.sum() > 100, "origins on the plane with directions inside it"
