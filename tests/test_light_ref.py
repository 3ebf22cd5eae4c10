"""CPU: the float64 definition of the lighting estimators' expectation (light_ref.py) at hand-worked cases, the shares every case of light_cases.py
states, the recorded profile's invariants, and two of its rows re-run in full on the oracle."""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import light_cases as lc
import light_ref as lr
from strolle_amd import Buffer, CameraMode, Light

UP = np.array([[0.0, 1.0, 0.0]])
O = np.zeros((1, 3))


def _hits(point=O, view=UP, normal=UP, base=(1.0, 0.5, 0.25), metallic=1.0, roughness=0.25, reflectance=0.5):
    one = np.ones(1)
    return lr.Hits(np.array([True]), np.asarray(point, float), np.asarray(view, float), np.asarray(normal, float), np.array([base], float), np.zeros((1, 3)),
                   metallic * one, roughness * one, reflectance * one, np.zeros(1, int), np.full(1, np.inf))


# ----------------------------------------------------------------------------- the definition, by hand
def test_one_light_straight_above():
    inf = Light.point((0.0, 2.0, 0.0), 0.1, (3.0, 2.0, 1.0), math.inf)
    assert np.array_equal(lr.incident(inf, O, UP), [[3.0, 2.0, 1.0]])                       # f_angle = f_dist = f_cosine = 1
    near = Light.point((0.0, 2.0, 0.0), 0.1, (3.0, 2.0, 1.0), 4.0)
    # |l|^2 = 4, (4 / 16)^2 = 1/16, (15/16)^2 = 225/256, / 4
    assert lr.f_dist(near, O)[0] == pytest.approx(225.0 / 1024.0, rel=1e-15)
    assert lr.incident(near, O, UP)[0] == pytest.approx(np.array([3.0, 2.0, 1.0]) * 225.0 / 1024.0, rel=1e-15)
    assert lr.diffuse_factor(np.array([0.0, 0.25, 1.0])) == pytest.approx([1 / math.pi, 0.75 / math.pi, 0.0], rel=1e-15)


def test_cone_edge():
    spot = Light.spot((0.0, 2.0, 0.0), 0.05, (1.0, 1.0, 1.0), math.inf, (0.0, -1.0, 0.0), 0.5)
    assert lr.spot_direction(spot.direction) == pytest.approx([0.0, -1.0, 0.0], abs=1e-15)
    at = lambda angle: np.array([[2.0 * math.tan(angle), 0.0, 0.0]])
    assert lr.f_angle(spot, O)[0] == 1.0                                                     # on the axis
    assert lr.f_angle(spot, at(0.25))[0] == pytest.approx(1.0 - 0.125, rel=1e-12)            # half way: 1 - (1/2)^3
    assert lr.f_angle(spot, at(0.5))[0] == pytest.approx(0.0, abs=1e-12)                     # the edge
    assert lr.f_angle(spot, at(0.5 + 1e-6))[0] == 0.0 and lr.f_angle(spot, at(1.2))[0] == 0.0  # beyond it: clamped, not negative
    assert lr.f_angle(Light.point((0.0, 2.0, 0.0), 0.05, (1.0,) * 3, 5.0), at(1.2))[0] == 1.0  # a point light has no cone
    # a direction that is not unit and does not survive two float32 exactly: what the light keeps is the decoded one, to float32's resolution
    d = lr.spot_direction((0.3, -2.0, 0.7))
    assert np.linalg.norm(d) == pytest.approx(1.0, abs=1e-15) and d == pytest.approx(np.array([0.3, -2.0, 0.7]) / math.sqrt(0.09 + 4 + 0.49), abs=3e-7)


def test_both_range_clamps():
    light = Light.point((0.0, 1.0, 0.0), 0.01, (1.0, 1.0, 1.0), 2.0)
    far = np.array([[0.0, 1.0, 2.0], [0.0, 1.0, 2.5], [0.0, -1.5, 0.0]])                    # at the range and beyond it: saturate, not negative, not squared back up
    assert np.array_equal(lr.f_dist(light, far), [0.0, 0.0, 0.0])
    inside = np.array([[0.0, 1.0, 1.0]])                                                    # |l|^2 = 1: (1 - 1/16)^2 / 1
    assert lr.f_dist(light, inside)[0] == pytest.approx(225.0 / 256.0, rel=1e-15)
    close = np.array([[0.0, 1.0, 0.005]])                                                   # |l|^2 = 2.5e-5 < 1e-4: the divisor stops at 1e-4
    assert lr.f_dist(light, close)[0] == pytest.approx((1.0 - (2.5e-5 / 4.0) ** 2) ** 2 / 1e-4, rel=1e-12)
    assert lr.f_dist(Light.point((0.0, 1.0, 0.0), 0.01, (1.0,) * 3, math.inf), far).tolist() == [1.0, 1.0, 1.0]


def test_grazing_incidence():
    assert lr.f_cosine(Light.point((10.0, 0.0, 0.0), 0.1, (1.0,) * 3, 50.0), O, UP)[0] == 0.0          # in the surface's plane
    assert lr.f_cosine(Light.point((10.0, -0.5, 0.0), 0.1, (1.0,) * 3, 50.0), O, UP)[0] == 0.0         # below it: clamped
    assert lr.f_cosine(Light.point((3.0, 3.0, 0.0), 0.1, (1.0,) * 3, 50.0), O, UP)[0] == pytest.approx(math.sqrt(0.5), rel=1e-15)
    # a light's position is float32: 1/64 is exact there
    assert lr.f_cosine(Light.point((10.0, 1 / 64, 0.0), 0.1, (1.0,) * 3, 50.0), O, UP)[0] == pytest.approx((1 / 64) / math.sqrt(100.0 + 1 / 4096), rel=1e-12)
    # the specular factor dies with n.l as well
    assert np.array_equal(lr.specular_factor(Light.point((10.0, -0.5, 0.0), 0.1, (1.0,) * 3, 50.0), _hits()), np.zeros((1, 3)))


def test_specular_straight_above_by_hand():
    """n = v = l: h = n, D = 1 / (pi a^2), G = 1, F = f0 (+ (f90 - f0) 0.001^5), so spec = f0 / (4 pi a^2) times the sphere light's intensity"""
    light = Light.point((0.0, 2.0, 0.0), 0.125, (1.0,) * 3, math.inf)     # a radius float32 holds exactly
    a = 0.25
    intensity = (a / (a + 0.125 * 0.5 / 2.0)) ** 2
    f0 = np.array([1.0, 0.5, 0.25])
    f = f0 + (1.0 - f0) * 0.001 ** 5
    assert lr.specular_factor(light, _hits())[0] == pytest.approx(intensity * f / (4.0 * math.pi * a * a), rel=1e-13)
    # the roughness clamp: a mirror (roughness 0) is shaded as roughness 0.089^2
    a = 0.089 ** 2
    intensity = (a / (a + 0.125 * 0.5 / 2.0)) ** 2
    assert lr.specular_factor(light, _hits(roughness=0.0))[0] == pytest.approx(intensity * f / (4.0 * math.pi * a * a), rel=1e-13)
    # a dielectric's f0 = 0.16 reflectance^2 (1 - metallic) + base metallic, f90 = saturate(16.5 sum f0)
    m, refl = 0.5, 0.5
    f0 = 0.16 * refl * refl * (1 - m) + np.array([1.0, 0.5, 0.25]) * m
    f = f0 + (min(1.0, 16.5 * f0.sum()) - f0) * 0.001 ** 5
    a = 0.25
    intensity = (a / (a + 0.125 * 0.5 / 2.0)) ** 2
    assert lr.specular_factor(light, _hits(metallic=m))[0] == pytest.approx(intensity * f / (4.0 * math.pi * a * a), rel=1e-13)


def test_no_metal_no_specular():
    light = Light.point((0.5, 2.0, 0.3), 0.1, (1.0,) * 3, math.inf)
    assert np.array_equal(lr.specular_factor(light, _hits(metallic=0.0)), np.zeros((1, 3)))
    assert lr.specular_factor(light, _hits(metallic=1e-3)).min() > 0.0


def test_view_from_behind_no_specular():
    light = Light.point((0.5, 2.0, 0.3), 0.1, (1.0,) * 3, math.inf)
    for view in ([[1.0, 0.0, 0.0]], [[0.6, -0.8, 0.0]]):                                     # n.v = 0 and n.v < 0
        assert np.array_equal(lr.specular_factor(light, _hits(view=view)), np.zeros((1, 3)))


def test_camera_ray_is_the_engines():
    from surface_families import camera_rays
    cam = lc.CASES["odd"].camera(CameraMode.IMAGE)
    want = camera_rays(cam)
    o, d = lr.camera_rays(cam)
    assert np.abs(o - want["origin"]).max() < 1e-5 and np.abs(d - want["direction"]).max() < 1e-5


def test_primary_hit_is_the_oracles_gbuffer():
    """pack_gbuffer + decode_gbuffer against the words the oracle itself writes: the tilted, non-uniformly scaled metallic floor"""
    from oracle_binding import OracleEngine
    import surface_ref
    case = lc.CASES["tilted"]
    e = OracleEngine()
    case.build(e); e.set_seed(1)
    cam = e.create_camera(case.camera(CameraMode.IMAGE))
    e.tick(); e.render_camera(cam)
    planes = {b: e.read_buffer(cam, b).reshape(-1, 4) for b in (Buffer.PRIM_GBUFFER_D0_A, Buffer.PRIM_GBUFFER_D0_B, Buffer.PRIM_GBUFFER_D1_A, Buffer.PRIM_GBUFFER_D1_B)}
    e.close()
    d0, d1 = ((planes[Buffer.PRIM_GBUFFER_D0_A], planes[Buffer.PRIM_GBUFFER_D1_A]) if planes[Buffer.PRIM_GBUFFER_D0_A].any()
              else (planes[Buffer.PRIM_GBUFFER_D0_B], planes[Buffer.PRIM_GBUFFER_D1_B]))
    want = surface_ref.decode_gbuffer(d0, d1)
    hits = lc._geometry("tilted", True)[0]
    assert hits.hit.all() and (want["depth"] > 0).all()
    assert np.abs(hits.normal - want["normal"]).max() < 1e-6
    for name, got in (("metallic", hits.metallic), ("roughness", hits.roughness), ("reflectance", hits.reflectance), ("base_color", hits.base_color)):
        w = want[name][:, :3] if name == "base_color" else want[name]
        assert np.array_equal(got, w), name
    o, d = lr.camera_rays(case.camera(CameraMode.IMAGE))
    assert np.abs(hits.point - (o + d * (want["depth"] - 0.01)[:, None])).max() < 1e-5
    n = hits.normal[0]
    assert abs(n[0]) > 0.02 and abs(n[2]) > 0.02, "the tilt is there"
    m = np.asarray(case.floor_xform, np.float64)[:, :3]
    naive = m @ np.array([0.0, 1.0, 0.0]); naive /= np.linalg.norm(naive)
    assert np.abs(n - naive).max() > 0.05, "M . n and inverse-transpose(M) . n differ: the normal path matters"


# ----------------------------------------------------------------------------- the shares
@pytest.mark.parametrize("case_name", list(lc.ALL_CASES))
def test_case_shares(case_name):
    exp = lc.expectation(case_name, "DI_DIFFUSE")
    sh = lc.shares(exp)
    assert exp.hits.hit.all(), "every pixel hits geometry"
    assert sh["ambiguous"] <= lc.MAX_AMBIGUOUS, sh
    assert min(sh["lit"]) >= lc.MIN_LIT, sh
    if case_name == "occluder":
        assert max(sh["hidden"]) >= lc.MIN_HIDDEN_OCCLUDER, sh
        assert (exp.held & (exp.hits.instance.reshape(exp.held.shape) == 1)).sum() >= 16, "the occluder's own top is held to the definition too"
    lights = lc.ALL_CASES[case_name].lights
    for light in lights:
        gap = np.linalg.norm(exp.hits.point - np.asarray(light.position, float), axis=1).min()
        assert gap > 2.0 * light.radius, "no hit point inside a light"
    w, h = lc.ALL_CASES[case_name].size
    assert exp.value.shape == (h, w, 3)


def test_cases_reach_the_edges_they_are_there_for():
    cone = lc.expectation("cone", "DI_DIFFUSE").value.sum(axis=2)
    assert (cone == 0).mean() > 0.1 and (cone > 0).mean() > 0.3, f"the cone's edge crosses the frame: {(cone > 0).mean():.2f} lit"
    beyond = lc.expectation("beyond", "DI_DIFFUSE")
    dark = [b for b in lc.blocks(lc.SIZE) if not beyond.value[b[1]:b[3], b[0]:b[2]].any()]
    assert len(dark) >= 1, "a whole block beyond the light's range"
    _, den, names = lc.denominators(beyond)
    defs, _ = lc.sums(beyond.value, beyond.held)
    assert ((defs == 0) & (den > 0)).any(), "where the definition is 0 the comparison is absolute, in units of an average block"
    assert len(lc.CASES["many"].lights) > 16
    assert lc.expectation("metallic", "DI_SPECULAR").value.min() >= 0 and lc.expectation("metallic", "DI_SPECULAR").value.sum() > 0
    assert not lc.expectation("three", "DI_SPECULAR").value.any(), "metallic 0: no specular light at all"
    w, h = lc.CASES["odd"].size
    assert w % 8 and h % 8 and w % 2


# ----------------------------------------------------------------------------- the profile
@pytest.fixture(scope="module")
def profile():
    return lc.load_profile()


def test_profile_covers_the_matrix(profile):
    assert (profile["warmup"], profile["frames"]) == (lc.WARMUP, lc.FRAMES) and tuple(profile["seeds_16"]) == lc.SEEDS16
    assert [(r["case"], r["mode"]) for r in profile["rows"]] == lc.MATRIX
    for c, shares in profile["shares"].items():
        assert shares == pytest.approx(lc.shares(lc.expectation(c, "DI_DIFFUSE")))
    assert profile["b"] >= 0.002


@pytest.mark.parametrize("case_name,mode", lc.MATRIX, ids=[f"{c}-{m}" for c, m in lc.MATRIX])
def test_profile_invariants(profile, case_name, mode):
    """|r_o - 1| <= 4 sigma_seed / sqrt(16) + b for every statistic the definition holds; the recorded arrays are the definition's statistics"""
    rec = lc.recorded(case_name, mode)
    _, _, names = lc.denominators(lc.expectation(case_name, lc.DEFINED_BY.get(mode, mode)))
    assert all(len(rec[k]) == len(names) for k in rec)
    dev, sigma = lc.recorded_deviation(case_name, mode, rec), rec["sigma_seed"]
    row = next(r for r in profile["rows"] if (r["case"], r["mode"]) == (case_name, mode))
    assert np.allclose(dev[:3], row["frame_deviation"], atol=1e-5) and np.allclose(sigma[:3] / 4.0, row["frame_standard_error"], atol=1e-5)
    held = np.array([not lc.oracle_held(profile, case_name, mode, n) for n in names])
    excess = np.abs(dev) - (4.0 * sigma / 4.0 + profile["b"])
    bad = np.flatnonzero(held & (excess > 0))
    assert not len(bad), f"{names[bad[0]]}: the oracle's deviation {dev[bad[0]]:+.5f} with sigma_seed {sigma[bad[0]]:.5f} and b {profile['b']:.5f}"


def test_profile_allowance_is_the_rule(profile):
    """b is twice the largest frame-sum deviation of a diffuse, Reference or Image row beyond 3 standard errors, or 0.002"""
    worst = 0.0
    for case_name, mode in lc.MATRIX:
        if mode in ("DI_DIFFUSE", "REFERENCE", "IMAGE"):
            dev, se = np.abs(lc.recorded_deviation(case_name, mode)[:3]), lc.recorded(case_name, mode)["sigma_seed"][:3] / 4.0
            worst = max([worst] + [float(d) for d, e in zip(dev, se) if d > 3.0 * e])
    assert profile["b"] == pytest.approx(2.0 * worst if worst else 0.002, rel=1e-9)


RERUN = [("beyond", "DI_DIFFUSE"), ("metallic", "DI_SPECULAR")]


@pytest.mark.parametrize("case_name,mode", RERUN, ids=[f"{c}-{m}" for c, m in RERUN])
def test_profile_row_reproduces(case_name, mode):
    """16 seeds x 1,064 frames again: seeds make the oracle deterministic, and the sums are exactly rounded, so the recorded sums come back to the bit"""
    rec = lc.recorded(case_name, mode)
    exp = lc.expectation(case_name, mode)
    case = lc.CASES[case_name]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:            # the oracle's calls release the interpreter lock
        means = list(pool.map(lambda s: lc.oracle_mean(case, mode, s), lc.SEEDS16))
    got16, _ = lc.sums(lc.pooled(means), exp.held)
    got8, _ = lc.sums(lc.pooled(means[:8]), exp.held)
    assert np.array_equal(got16, rec["sum_16"]) and np.array_equal(got8, rec["sum_8"])
    per_seed = np.array([lc.deviations(m, exp)[0] for m in means])
    assert np.allclose(per_seed.std(axis=0, ddof=1), rec["sigma_seed"], rtol=1e-6, atol=1e-12)
