"""CPU tests of light shafts (include/strolle_hip.h "light shafts"): the entry points are exported, declared and bound by the Rust facade,
StLightShaftsDesc has one layout in the header, api.py and ffi.rs, every argument error occurs on a host-only engine, set / get / clear
round-trip there, the node and a window exclude each other through all three window setters, the plan, the process call says that it
needs a device, the numpy restatement (shafts_ref.shafts_f32) at cases worked out by hand, the float64 definition against closed forms,
and the reference side: the restatement with the checker's occlusion probe against the definition with brute-force visibility on both
slat scenes over the GPU test's matrix, which is where profiles/light_shafts.json's threshold and tolerance come from."""
import ctypes as C
import importlib.util
import json
import math
import os
import re

import numpy as np
import pytest

import shafts_cases as K
import shafts_ref as R
import output_chain_abi as A
from fog_ref import exp_
from strolle_amd import Engine, Light, StrolleError, Tonemap, display_desc, light_shafts_desc, light_shafts_plan, scenes
from output_chain_abi import ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE, host_camera as _host_camera
from strolle_amd import api
from strolle_amd.api import dist_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("st_camera_set_light_shafts", "st_camera_get_light_shafts", "st_light_shafts_plan", "st_light_shafts_process")
FIELDS = ["struct_size", "flags", "steps", "divisor", "density", "anisotropy", "max_distance", "intensity", "scatter", "_pad", "sun_color", "_pad2", "sun_direction",
          "light_count", "lights"]
OFFSETS = [0, 4, 8, 12, 16, 20, 24, 28, 32, 44, 48, 60, 64, 76, 80]
F = np.float32
inf, nan = float("inf"), float("nan")
PERSPECTIVE = [1.5, 0, 0, 0, 0, 2.0, 0, 0, 0, 0, 0, -1.0, 0, 0, 0.1, 0]
ORTHOGRAPHIC = [0.5, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, -0.01, 0, 0, 0, 1.0, 1.0]
IDENTITY = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0]


def _tool():
    spec = importlib.util.spec_from_file_location("shafts_bench", os.path.join(ROOT, "tools", "shafts_bench.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def test_entry_points_are_exported_declared_and_bound():
    A.exports_header_and_ffi_agree("StLightShaftsDesc", FIELDS, ENTRY_POINTS, [("ST_SHAFTS_FOLLOW_SUN", 1), ("ST_SHAFTS_LIGHT_EXTINCTION", 2)])
    facade = open(os.path.join(ROOT, "rust", "strolle-hip", "src", "lib.rs")).read()
    assert "pub fn set_light_shafts(" in facade and "ffi::st_camera_set_light_shafts(" in facade
    assert api.SHAFTS_FOLLOW_SUN == R.FOLLOW_SUN == 1 and api.SHAFTS_LIGHT_EXTINCTION == R.LIGHT_EXTINCTION == 2


def test_desc_layout_agrees_between_c_and_ctypes(tmp_path):
    got = A.c_layout(tmp_path, "StLightShaftsDesc", FIELDS, ["ST_SHAFTS_FOLLOW_SUN", "ST_SHAFTS_LIGHT_EXTINCTION", "ST_SHAFTS_MAX_LIGHTS"])
    assert got == [144] + OFFSETS + [1, 2, 8]


def _d(**kw):
    """a valid desc, then `kw` over it (a tuple replaces a whole array, name_i one element)"""
    d = light_shafts_desc(steps=16, divisor=2, density=0.1, anisotropy=0.5, max_distance=20.0, intensity=1.0, scatter=(0.9, 0.8, 0.7), sun_color=(1.0, 0.5, 0.25),
                          sun_direction=(0.0, 1.0, 0.0), lights=(3, 4))
    for k, v in kw.items():
        m = re.fullmatch(r"(\w+?)_(\d)", k)
        if m and hasattr(d, m.group(1)) and not hasattr(d, k):
            getattr(d, m.group(1))[int(m.group(2))] = v
        elif isinstance(v, tuple):
            setattr(d, k, (C.c_float * len(v))(*v))
        else:
            setattr(d, k, v)
    return d


BAD = [dict(struct_size=140), dict(struct_size=148), dict(struct_size=0), dict(flags=4), dict(flags=0x80000001), dict(steps=0), dict(steps=65), dict(divisor=0), dict(divisor=3),
       dict(divisor=4), dict(density=-0.1), dict(density=nan), dict(density=inf), dict(anisotropy=0.96), dict(anisotropy=-0.96), dict(anisotropy=nan),
       dict(max_distance=0.0), dict(max_distance=-1.0), dict(max_distance=inf), dict(max_distance=nan), dict(intensity=-1.0), dict(intensity=nan), dict(intensity=inf),
       dict(scatter_0=-0.1), dict(scatter_1=1.1), dict(scatter_2=nan), dict(sun_color_0=-1.0), dict(sun_color_1=nan), dict(sun_color_2=inf),
       dict(sun_direction=(0.0, 0.0, 0.0)), dict(sun_direction=(nan, 1.0, 0.0)), dict(sun_direction=(0.0, inf, 0.0)), dict(light_count=9), dict(light_count=0xffffffff)]
GOOD = [dict(flags=f) for f in range(4)] + [dict(steps=1), dict(steps=64), dict(divisor=1), dict(density=0.0), dict(anisotropy=0.95), dict(anisotropy=-0.95), dict(anisotropy=0.0),
        dict(max_distance=1e30), dict(intensity=0.0), dict(scatter=(0.0, 0.0, 0.0)), dict(scatter=(1.0, 1.0, 1.0)), dict(sun_color=(0.0, 0.0, 0.0), sun_direction=(0.0, 0.0, 0.0)),
        dict(sun_color=(0.0, 0.0, 0.0), sun_direction=(nan, nan, nan)), dict(flags=1, sun_direction=(0.0, 0.0, 0.0)), dict(sun_direction=(0.0, 0.0, 1e-30)), dict(light_count=0),
        dict(light_count=8), dict(_pad=nan), dict(_pad2=123.0)]


def test_argument_errors_on_a_host_only_engine():
    e, cam = _host_camera()
    def still_off(kw):
        assert not e.get_light_shafts(cam)[1], kw   # a refused desc leaves the setting as it was

    A.argument_errors(e, cam, "camera_set_light_shafts", "camera_get_light_shafts", _d, BAD, GOOD, each_bad=still_off)
    with pytest.raises(StrolleError):
        e.set_light_shafts(cam, steps=100)
    e.close()


def test_process_checks_its_arguments_and_needs_a_device():
    e, cam = _host_camera()
    b, h = e._b, e._h
    d = _d()
    fake = C.c_void_p(4096)   # never dereferenced: the checks and the missing device come first
    manual, auto = display_desc(tonemap=Tonemap.ACES_FITTED, exposure_ev=1.0), display_desc(auto_exposure=True)
    persp, ident = (C.c_float * 16)(*PERSPECTIVE), (C.c_float * 16)(*IDENTITY)

    def proj(**kw):
        p = list(PERSPECTIVE)
        for k, v in kw.items():
            p[int(k[1:])] = v
        return (C.c_float * 16)(*p)

    def sp(desc=d, display=None, transform=ident, projection=persp, color=fake, depth=fake, w=64, hh=48, dst=fake, fmt=0, engine=h):
        return b.light_shafts_process(engine, C.byref(desc) if desc is not None else None, C.byref(display) if display is not None else None, transform, projection, color,
                                      depth, w, hh, dst, fmt, None)

    assert sp() == ST_ERR_NO_DEVICE and sp(display=manual) == ST_ERR_NO_DEVICE and sp(desc=_d(flags=3)) == ST_ERR_NO_DEVICE   # it takes ST_SHAFTS_FOLLOW_SUN
    assert sp(engine=None) == ST_ERR_INVALID_ARGUMENT
    for kw in (dict(desc=None), dict(transform=None), dict(projection=None), dict(color=None), dict(depth=None), dict(dst=None), dict(w=0), dict(hh=0), dict(w=16385),
               dict(hh=16385), dict(fmt=4), dict(fmt=-1), dict(display=auto), dict(desc=_d(struct_size=8)), dict(desc=_d(steps=0)), dict(desc=_d(density=nan)),
               dict(projection=(C.c_float * 16)(*ORTHOGRAPHIC)), dict(projection=proj(p15=1.0)), dict(projection=proj(p5=0.0)), dict(projection=proj(p0=inf))):
        assert sp(**kw) == ST_ERR_INVALID_ARGUMENT, kw
    assert sp(w=16384, hh=1) == ST_ERR_NO_DEVICE
    with pytest.raises(StrolleError):
        e.light_shafts_process(d, IDENTITY, PERSPECTIVE, 4096, 4096, 64, 48, 4096)
    e.close()


def _values(d):
    return [list(getattr(d, f)) if hasattr(getattr(d, f), "__len__") else getattr(d, f) for f in FIELDS]


def test_set_get_round_trip_and_survival_on_a_host_only_engine():
    e, cam = _host_camera()
    d0, on0 = e.get_light_shafts(cam)
    assert not on0 and d0.struct_size == C.sizeof(api.StLightShaftsDesc) and all(v == 0 or v == [0] * len(v) for v in _values(d0)[1:])
    want = light_shafts_desc(steps=24, divisor=1, density=0.07, anisotropy=-0.3, max_distance=33.0, intensity=2.0, scatter=(0.1, 0.2, 0.3), sun_color=(3.0, 2.0, 1.0),
                             sun_direction=(0.1, 0.9, 0.2), lights=(5, 6, 7), follow_sun=True, light_extinction=True)
    assert want.flags == 3 and want.light_count == 3
    e.set_light_shafts(cam, want)
    got, on = e.get_light_shafts(cam)
    assert on and _values(got) == _values(want)
    e.tick()
    e.update_camera(cam, scenes.cornell_camera((80, 48)))   # a resize reallocates the camera: the setting stays
    got, on = e.get_light_shafts(cam)
    assert on and _values(got) == _values(want)
    e.set_light_shafts(cam, None)
    got, on = e.get_light_shafts(cam)
    assert not on and got.steps == 24   # the last desc stays readable
    stale = _d(light_count=1)
    stale.lights[5] = 1234   # beyond light_count: not kept
    e.set_light_shafts(cam, stale)
    assert list(e.get_light_shafts(cam)[0].lights) == [3, 0, 0, 0, 0, 0, 0, 0]
    e.delete_camera(cam)
    e.close()


def test_light_shafts_and_a_window_exclude_each_other_on_a_host_only_engine():
    e, cam = _host_camera()
    d = _d()
    A.node_and_window_exclude_each_other(e, cam, "camera_set_light_shafts", d, lambda: e.get_light_shafts(cam)[1])
    e.close()
    ranks = []
    for r in range(2):
        e = Engine(device=-1)
        scenes.build_cornell(e)
        cam = e.create_camera(scenes.cornell_camera((64, 48)))
        e.dist_init_local(r, 2, 9292)
        ranks.append((e, cam))
    (e0, c0), (e1, c1) = ranks
    e0.set_light_shafts(c0, d)
    with pytest.raises(StrolleError, match="light shafts"):
        e0.dist_set_partition(c0)
    with pytest.raises(StrolleError, match="light shafts"):
        e0.dist_set_grid(c0, dist_grid(64, 48, 2))
    e0.set_light_shafts(c0, None)
    e0.dist_set_partition(c0)
    e1.dist_set_grid(c1, dist_grid(64, 48, 2))
    for e, cam in ranks:
        with pytest.raises(StrolleError, match="window"):
            e.set_light_shafts(cam, d)
        assert not e.get_light_shafts(cam)[1]
        e.dist_shutdown(); e.close()


def test_plan_cell_counts_and_the_jitter_table():
    for (w, h) in K.SIZES + [(1920, 1080), (16384, 3)]:
        for div in (1, 2):
            cells, jitter = light_shafts_plan(_d(divisor=div), w, h)
            assert cells == ((w + div - 1) // div, (h + div - 1) // div)
            assert np.array_equal(jitter.view(np.uint32), R.JITTER.view(np.uint32))
    assert sorted((R.JITTER * 16 - 0.5).reshape(-1).tolist()) == list(range(16)) and R.JITTER[1, 2] == F(14.5 / 16) and R.JITTER[3, 0] == F(15.5 / 16)
    for bad in (dict(w=0), dict(h=0), dict(w=16385)):
        with pytest.raises(StrolleError):
            light_shafts_plan(_d(), bad.get("w", 8), bad.get("h", 8))
    with pytest.raises(StrolleError):
        light_shafts_plan(_d(steps=0), 8, 8)


# ---------------------------------------------------------------- the restatement by hand
LOOK = np.array(IDENTITY, np.float32)            # the camera at the origin looking down -z
P1 = np.array(PERSPECTIVE, np.float32)
NEVER = lambda rays: np.zeros(len(rays), bool)   # noqa: E731
ALWAYS = lambda rays: np.ones(len(rays), bool)   # noqa: E731


def _one(d, z=5.0, lights=(), occluded=NEVER, colour=(0.25, 0.5, 1.0, 0.75), size=(1, 1), **kw):
    w, h = size
    img = np.broadcast_to(np.array(colour, np.float32), (h, w, 4)).copy()
    depth = np.full((h, w), z, np.float32) if np.isscalar(z) else np.asarray(z, np.float32)
    det = {}
    out, n = R.shafts_f32(img, depth, LOOK, P1, d, list(lights), occluded, details=det, **kw)
    return out, n, det, img


def test_reference_one_cell_one_step_the_sun_alone():
    """1 x 1 frame, divisor 1, one step: the ray is -z, j = 0.5 / 16, t = j d, S = exp(-sigma t) d sigma scatter sun_color / (4 pi)"""
    d = light_shafts_desc(steps=1, divisor=1, density=0.25, anisotropy=0.0, max_distance=100.0, intensity=2.0, scatter=(1.0, 0.5, 0.0), sun_color=(8.0, 8.0, 8.0),
                          sun_direction=(0.0, 2.0, 0.0))
    out, n, det, img = _one(d, z=4.0)
    assert n == 1 and [float(v) for v in (det["w"][0][0, 0], det["w"][1][0, 0], det["w"][2][0, 0])] == [0.0, 0.0, -1.0]
    rays = det["log"][0][3]
    t = F(F(0.5 / 16) * F(4.0))
    assert np.array_equal(rays["origin"][0], np.array([0, 0, -t], np.float32)) and np.array_equal(rays["direction"][0], np.array([0, 1, 0], np.float32))
    assert rays["t_max"][0] == R.FLT_MAX
    k1 = F(1.0 / (4.0 * math.pi))
    m = F(F(exp_(F(-(F(0.25) * t))) * F(4.0)) * F(0.25))
    S = [F(F(m * F(s)) * F(F(8.0) * k1)) for s in (1.0, 0.5, 0.0)]
    assert np.array_equal(det["cells"][0, 0], np.array(S + [4.0], np.float32))
    want = [F(F(c) + F(F(2.0) * s)) for c, s in zip((0.25, 0.5, 1.0), S)] + [F(0.75)]
    assert np.array_equal(out[0, 0], np.array(want, np.float32))
    assert abs(float(S[0]) - math.exp(-0.25 * 0.125) * 4 * 0.25 * 8 / (4 * math.pi)) < 1e-6
    # the same sample in shadow: nothing is added, the pixel keeps its four words
    out, n, det, img = _one(d, z=4.0, occluded=ALWAYS)
    assert n == 1 and np.array_equal(out.view(np.uint32), img.view(np.uint32))
    # max_distance ends the march: d_end = 2
    d.max_distance = 2.0
    _, _, det, _ = _one(d, z=4.0)
    assert det["log"][0][3]["origin"][0][2] == -F(F(0.5 / 16) * F(2.0)) and det["cells"][0, 0, 3] == 4.0


def test_reference_phase_function():
    k1, k2, k3, _ = R.host_constants(light_shafts_desc(anisotropy=0.0))
    assert (k1, k2, k3) == (F(1 / (4 * math.pi)), F(1), F(0)) and R._phase(k1, k2, k3, F(-1)) == R._phase(k1, k2, k3, F(1)) == k1   # isotropic
    for g in (-0.6, 0.8, 0.95):
        k1, k2, k3, _ = R.host_constants(light_shafts_desc(anisotropy=g))
        gg = float(F(g))
        for c in (-1.0, 1.0, 0.3):
            want = (1 - gg * gg) / (4 * math.pi) / (1 + gg * gg - 2 * gg * c) ** 1.5
            # q = k2 - k3 c cancels: k2, k3 c and the difference are each rounded at magnitude <= 2 (3 x 2^-24 x 2 absolute), q^-1.5 takes
            # 1.5 x that relative to q (as small as 0.0025 at g = 0.95), and k1, the product, the root and the quotient add four roundings
            q = 1 + gg * gg - 2 * gg * c
            assert abs(float(R._phase(k1, k2, k3, F(c))) / want - 1) <= 1.5 * 6 * 2.0 ** -24 / q + 4 * 2.0 ** -24, (g, c)
    # forward scattering towards the sun, one cell: the ray (0, 0, -1) and the sun at (0, 0, -1): c = 1
    d = light_shafts_desc(steps=1, divisor=1, density=0.1, anisotropy=0.8, sun_color=(1.0, 1.0, 1.0), sun_direction=(0.0, 0.0, -3.0))
    _, _, det, _ = _one(d)
    k1, k2, k3, L = det["k"] + (det["L"],)
    assert np.array_equal(L, np.array([0, 0, -1], np.float32))
    q = F(k2 - k3 * F(1))
    m = F(F(exp_(F(-(F(0.1) * F(F(0.5 / 16) * F(5.0))))) * F(5.0)) * F(0.1))
    assert det["cells"][0, 0, 0] == F(m * F(k1 / F(q * np.sqrt(q))))


def test_reference_spot_cone_range_edge_and_radius():
    base = dict(steps=1, divisor=1, density=0.1, anisotropy=0.0, max_distance=100.0)
    # the sample of z = 16 is at (0, 0, -0.5). A spot 2 m above it pointing straight down: on the axis f_angle = 1
    down = R.table_light(Light.spot((0.0, 2.0, -0.5), 0.1, (10.0, 10.0, 10.0), 50.0, (0.0, -1.0, 0.0), 0.5))
    _, n, det, _ = _one(light_shafts_desc(lights=(1,), **base), z=16.0, lights=[down])
    assert n == 1
    ray = det["log"][0][3][0]
    assert np.array_equal(ray["direction"], np.array([0, 1, 0], np.float32)) and ray["t_max"] == F(F(2.0) - F(0.1))
    f = F(F(4.0) * F(F(1) / F(2500.0))); sm = F(F(1) - F(f * f))
    e = F(F(F(10.0) * F(F(1.0) * F(F(sm * sm) / F(4.0)))) * F(1 / (4 * math.pi)))
    m = F(F(exp_(F(-(F(0.1) * F(0.5)))) * F(16.0)) * F(0.1))
    assert det["cells"][0, 0, 0] == F(m * e)
    # pointing sideways: the sample is 90 degrees off the axis, outside a 0.5 rad cone: E = 0 and NO ray
    side = R.table_light(Light.spot((0.0, 2.0, -0.5), 0.1, (10.0, 10.0, 10.0), 50.0, (1.0, 0.0, 0.0), 0.5))
    out, n, det, img = _one(light_shafts_desc(lights=(1,), **base), z=16.0, lights=[side])
    assert n == 0 and det["log"] == [] and np.array_equal(out.view(np.uint32), img.view(np.uint32))
    # out of range: |v| = 2 >= range 2 -> smooth factor 0 -> no ray; just inside it a ray
    for rng, want in ((2.0, 0), (1.9, 0), (2.2, 1)):
        far = R.table_light(Light.point((0.0, 2.0, -0.5), 0.1, (10.0, 10.0, 10.0), rng))
        assert _one(light_shafts_desc(lights=(1,), **base), z=16.0, lights=[far])[1] == want, rng
    # a black light casts nothing; an infinite range has f_dist = 1
    assert _one(light_shafts_desc(lights=(1,), **base), z=16.0, lights=[R.table_light(Light.point((0.0, 2.0, -0.5), 0.1, (0.0, 0.0, 0.0), 50.0))])[1] == 0
    _, n, det, _ = _one(light_shafts_desc(lights=(1,), **base), z=16.0, lights=[R.table_light(Light.point((0.0, 2.0, -0.5), 0.1, (3.0, 0.0, 0.0), inf))])
    assert n == 1 and det["cells"][0, 0, 0] == F(m * F(F(3.0) * F(1 / (4 * math.pi)))) and det["cells"][0, 0, 1] == 0
    # the sample inside the light's radius contributes nothing and casts nothing; on its surface likewise (len > radius is false)
    for radius, want in ((2.5, 0), (2.0, 0), (1.99, 1)):
        assert _one(light_shafts_desc(lights=(1,), **base), z=16.0, lights=[R.table_light(Light.point((0.0, 2.0, -0.5), radius, (3.0, 3.0, 3.0), inf))])[1] == want, radius
    # the extinction flag multiplies by exp(-sigma |v|)
    _, _, det, _ = _one(light_shafts_desc(lights=(1,), light_extinction=True, **base), z=16.0, lights=[R.table_light(Light.point((0.0, 2.0, -0.5), 0.1, (3.0, 0.0, 0.0), inf))])
    assert det["cells"][0, 0, 0] == F(m * F(F(F(3.0) * F(F(1.0) * exp_(F(-(F(0.1) * F(2.0)))))) * F(1 / (4 * math.pi))))


def test_reference_checkerboard_depth_and_empty_blocks():
    z = np.array([[1.0, 2.0, 5.0, 6.0, 9.0], [3.0, 4.0, 7.0, nan, 0.0], [nan, 0.0, -1.0, R.FLT_MAX, 2.0], [-0.0, nan, 3.0, inf, 1.0]], np.float32)
    d_c, live = R.cell_depth(z, 2)
    # cells (cx + cy) even: min; odd: max; NaN / 0 / negative entries do not count; sky and +inf do; a partial block takes what it has
    assert np.array_equal(d_c, np.array([[1.0, 7.0, 9.0], [0.0, 3.0, 2.0]], np.float32)) and np.array_equal(live, [[True, True, True], [False, True, True]])
    # columns 2..3 alone: cell (0, 0) is even: min(5, 6, 7) = 5; cell (0, 1) is odd: max(3, FLT_MAX, +inf) = +inf (-1 does not count)
    sub, _ = R.cell_depth(z[:, 2:4], 2)
    assert sub[0, 0] == 5.0 and sub[1, 0] == inf
    d1, live1 = R.cell_depth(z, 1)
    assert np.array_equal(live1, z > 0) and np.array_equal(d1[live1], z[live1])
    # an empty block: the cell is all zero, no ray, and its pixels pass through
    d = light_shafts_desc(steps=4, divisor=2, density=0.1, sun_color=(1.0, 1.0, 1.0))
    out, n, det, img = _one(d, z=np.array([[nan, 0.0], [-3.0, -0.0]], np.float32), size=(2, 2))
    assert n == 0 and not det["cells"].any() and np.array_equal(out.view(np.uint32), img.view(np.uint32))


def test_reference_one_divisor_2_pixel_across_a_depth_edge():
    """pixel (2, 1) of a 4 x 4 frame: u = (0.75, 0.25), cells (0..1, 0..1), bilinear weights .25 .75 / x .75 .25; the pixel is at 2 m, the
    cells at 2, 8, 2 and 0 (empty)"""
    d = light_shafts_desc(steps=1, divisor=2, density=0.1, max_distance=50.0, intensity=1.0)
    cells = np.zeros((2, 2, 4), np.float32)
    cells[0, 0] = (1.0, 0.0, 0.0, 2.0); cells[0, 1] = (0.0, 1.0, 0.0, 8.0); cells[1, 0] = (0.0, 0.0, 1.0, 2.0); cells[1, 1] = (9.0, 9.0, 9.0, 0.0)
    img = np.zeros((4, 4, 4), np.float32); img[..., 3] = 0.5
    z = np.full((4, 4), 2.0, np.float32)
    out, changed = R.apply_f32(img, z, cells, d)
    near = F(F(1) / F(F(0.001) + F(F(0.0) / F(2.0))))        # 1000
    far = F(F(1) / F(F(0.001) + F(F(6.0) / F(2.0))))
    w00, w10, w01 = F(F(F(0.25) * F(0.75)) * near), F(F(F(0.75) * F(0.75)) * far), F(F(F(0.25) * F(0.25)) * near)
    total = F(F(w00 + w10) + w01)
    assert np.array_equal(out[1, 2], np.array([F(w00 / total), F(w10 / total), F(w01 / total), 0.5], np.float32))
    assert out[1, 2, 1] < 0.001 and out[1, 2, 0] > 0.74   # the cell across the edge hardly counts
    # all four cells empty: S_p = 0, the pixel passes through
    out, changed = R.apply_f32(img, z, np.zeros((2, 2, 4), np.float32), d)
    assert not changed.any() and np.array_equal(out.view(np.uint32), img.view(np.uint32))


def test_reference_every_pass_through_rule():
    img = np.array([[[nan, -1.0, 70000.0, 0.3]]], np.float32)
    base = dict(steps=2, divisor=1, density=0.1, sun_color=(1.0, 1.0, 1.0))
    for kw, z in ((base, nan), (base, 0.0), (base, -4.0), (dict(base, density=0.0), 5.0), (dict(base, intensity=0.0), 5.0), (dict(base, scatter=(0.0, 0.0, 0.0)), 5.0),
                  (dict(base, sun_color=(0.0, 0.0, 0.0)), 5.0)):
        out, n, _, _ = _one(light_shafts_desc(**kw), z=z, colour=img[0, 0])
        assert np.array_equal(out.view(np.uint32), img.view(np.uint32)), (kw, z)
    assert _one(light_shafts_desc(**dict(base, sun_color=(0.0, 0.0, 0.0))), z=5.0)[1] == 0   # no sun: no ray
    # otherwise: colour clamped to [0, 65504] (NaN -> 0) plus the shafts, own alpha
    out, n, det, _ = _one(light_shafts_desc(**base), z=5.0, colour=img[0, 0])
    s = det["cells"][0, 0, :3]
    assert n == 2 and np.array_equal(out[0, 0], np.array([F(0) + s[0], F(0) + s[1], F(65504.0) + s[2], 0.3], np.float32))
    out, _, _, _ = _one(light_shafts_desc(**base), z=inf)   # +inf and sky: the march ends at max_distance
    assert np.isfinite(out).all()


# ---------------------------------------------------------------- the definition against closed forms
def test_definition_empty_scene_closed_form():
    """no occluder, the sun, g = 0: the stratified sum against sigma_s E (1 - e^(-sigma d)) / (4 pi sigma) within sigma d^2 / (2 steps) (times the integrand's scale)"""
    tris = np.zeros((0, 36), np.float32)
    for steps, dist, sigma in ((16, 6.0, 0.2), (64, 20.0, 0.05), (4, 3.0, 0.5)):
        d = light_shafts_desc(steps=steps, divisor=1, density=sigma, anisotropy=0.0, max_distance=100.0, intensity=1.0, scatter=(1.0, 0.6, 0.2), sun_color=(5.0, 5.0, 5.0))
        z = np.full((3, 5), dist, np.float32)
        out, _ = R.shafts_f64(np.zeros((3, 5, 4), np.float32), z, LOOK, np.array(K.projection((5, 3))), d, [], tris)
        s = float(F(sigma))
        for i, alb in enumerate((1.0, float(F(0.6)), float(F(0.2)))):
            exact = alb * 5.0 * (1 - math.exp(-s * dist)) / (4 * math.pi)
            bound = alb * 5.0 / (4 * math.pi) * s * (s * dist * dist / (2 * steps))
            assert np.abs(out[..., i] - exact).max() <= bound, (steps, i)
        # and the restatement with nothing occluded agrees with the definition to float32 precision
        got, n = R.shafts_f32(np.zeros((3, 5, 4), np.float32), z, LOOK, np.array(K.projection((5, 3))), d, [], NEVER)
        assert n == 15 * steps and np.abs(got[..., :3] - out).max() <= 1e-5 * out.max()


def test_definition_half_plane_occluder_closed_form():
    """the sun straight overhead and a roof over z < -4: along the central ray (0, 0, -1) the samples with t < 4 are lit, the others shadowed:
    sigma_s E (1 - e^(-4 sigma)) / (4 pi sigma), within the stratified bound plus one stratum"""
    roof = np.array([[[-100.0, 3.0, -4.0], [100.0, 3.0, -4.0], [100.0, 3.0, -100.0]], [[-100.0, 3.0, -4.0], [100.0, 3.0, -100.0], [-100.0, 3.0, -100.0]]], np.float32)
    tris = np.zeros((2, 9, 4), np.float32); tris[:, [0, 3, 6], :3] = roof
    tris = tris.reshape(2, 36)
    for steps in (8, 32):
        sigma, dist = 0.15, 10.0
        d = light_shafts_desc(steps=steps, divisor=1, density=sigma, anisotropy=0.0, max_distance=100.0, intensity=1.0, scatter=(1.0, 1.0, 1.0), sun_color=(2.0, 2.0, 2.0),
                              sun_direction=(0.0, 1.0, 0.0))
        z = np.full((1, 1), dist, np.float32)
        out, margin = R.shafts_f64(np.zeros((1, 1, 4), np.float32), z, LOOK, np.array(K.projection((1, 1))), d, [], tris)
        s = float(F(sigma))
        exact = 2.0 * (1 - math.exp(-s * 4.0)) / (4 * math.pi)
        delta = dist / steps
        bound = 2.0 / (4 * math.pi) * s * (s * dist * dist / (2 * steps) + delta)
        assert abs(out[0, 0, 0] - exact) <= bound and out[0, 0, 0] > 0, steps
        free, _ = R.shafts_f64(np.zeros((1, 1, 4), np.float32), z, LOOK, np.array(K.projection((1, 1))), d, [], np.zeros((0, 36), np.float32))
        assert out[0, 0, 0] < 0.8 * free[0, 0, 0]   # the roof does darken: (1 - e^-0.6) / (1 - e^-1.5) = 0.58


# ---------------------------------------------------------------- the reference side
@pytest.fixture(scope="module")
def profile():
    with open(os.path.join(ROOT, "profiles", "light_shafts.json")) as f:
        return json.load(f)["reference"]


@pytest.mark.parametrize("scene", list(K.SCENES))
def test_the_probe_restatement_agrees_with_the_definition_and_fixes_the_profile(scene, profile):
    tool = _tool()
    m = tool.measure_reference(scene)
    prof = profile[scene]
    print(scene, m)
    assert m["triangles"] == (34 if scene == "slats" else 546) and m["triangles"] <= (56 if scene == "slats" else 600)
    # the committed figures are the measurement's, not wider
    assert prof["threshold"] == m["threshold"] and prof["tolerance"] == m["tolerance"], (prof, m)
    assert 4.0 * m["worst_deviation"] <= prof["tolerance"] * 1.001
    # the conditions, from the restatement with the probe's visibility alone
    assert m["ambiguous_cell_share"] <= 0.02, m
    assert m["mixed_cell_share"] >= 0.10, m
    # and pixel by pixel: every non-ambiguous pixel of every case within the tolerance
    ref = tool.reference_scene(scene)
    for name, c in ref["cases"].items():
        sure = tool.pixel_cell_margin(c) >= prof["threshold"]
        dev = tool.deviation(c["got"], c["want"])
        assert not (np.nan_to_num(dev[sure]) > prof["tolerance"]).any(), name


def test_the_slat_scenes_bake_the_same_records_in_the_engine_and_the_checker():
    from oracle_binding import OracleEngine
    for scene, strips in K.SCENES.items():
        e, o = Engine(device=-1), OracleEngine()
        try:
            n = K.build_slats(e, strips); K.build_slats(o, strips)
            e.tick(); o.tick()
            a, b = e.read_scene(1), o.read_scene(1)
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)) and n == (34 if strips == 1 else 546)
        finally:
            e.close(); o.close()


def test_product_sources_name_the_new_kernels_and_slots():
    src = os.path.join(ROOT, "strolle_amd", "csrc")
    kernels = open(os.path.join(src, "st_kernels.h")).read()
    assert re.search(r"KS_FOG,.*\n\s*KS_SHAFTS_MARCH, KS_SHAFTS_APPLY,", kernels) and '"shafts_march"' in kernels and '"shafts_apply"' in kernels
    mk = open(os.path.join(src, "Makefile")).read()
    assert " k_shafts" in mk and " st_shafts" in mk
    hip = open(os.path.join(src, "k_shafts.hip")).read()
    assert hip.index("#pragma clang fp contract(off)") > hip.index('#include "k_common.h"')   # behind the includes: the inlined walk stays k_query.hip's
    assert "ST_LAUNCH_TRACE(k_shafts_march" in hip and "ST_SCENE_PROLOGUE" in hip
