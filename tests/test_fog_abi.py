"""CPU tests of fog (include/strolle_hip.h "fog"): the entry points are exported, declared and bound by the Rust facade, StFogDesc has one
layout in the header, api.py and ffi.rs, every argument error occurs on a host-only engine, set / get / clear round-trip there (also across
st_camera_update), a window and fog go together in either order through all three window setters, st_fog_process says that it needs a
device, the numpy restatement (fog_ref.fog_f32) at cases worked out by hand, and the restatement against the float64 definition
(fog_ref.fog_f64) over the GPU test's whole input matrix."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import fog_cases as K
import fog_ref as R
import output_chain_abi as A
from strolle_amd import Engine, FogFalloff, StrolleError, Tonemap, display_desc, fog_desc, scenes
from output_chain_abi import ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE, ST_OK, host_camera as _host_camera
from strolle_amd import api
from strolle_amd.api import dist_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("st_camera_set_fog", "st_camera_get_fog", "st_fog_process")
FIELDS = ["struct_size", "falloff", "flags", "_pad", "color", "start", "end", "density", "height_falloff", "height_reference", "sky_distance", "extinction",
          "inscattering", "light_color", "light_exponent", "light_direction", "_pad2"]
OFFSETS = [0, 4, 8, 12, 16, 32, 36, 40, 44, 48, 52, 56, 68, 80, 92, 96, 108]
F = np.float32
inf, nan = float("inf"), float("nan")
PERSPECTIVE = [1.5, 0, 0, 0, 0, 2.0, 0, 0, 0, 0, 0, -1.0, 0, 0, 0.1, 0]   # column major, infinite reverse-z: [15] == 0
ORTHOGRAPHIC = [0.5, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, -0.01, 0, 0, 0, 1.0, 1.0]
IDENTITY = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0]
FALLOFFS = ("LINEAR", "EXPONENTIAL", "EXPONENTIAL_SQUARED", "ATMOSPHERIC")


def test_entry_points_are_exported_declared_and_bound():
    A.exports_header_and_ffi_agree("StFogDesc", FIELDS, ENTRY_POINTS, [("ST_FOG_%s" % n, k) for k, n in enumerate(FALLOFFS)] + [("ST_FOG_SKY", 1), ("ST_FOG_FOLLOW_SUN", 2)])
    for k, name in enumerate(FALLOFFS):
        assert int(FogFalloff[name]) == getattr(R, name) == k
    assert api.FOG_SKY == R.SKY == 1 and api.FOG_FOLLOW_SUN == R.FOLLOW_SUN == 2


def test_desc_layout_agrees_between_c_and_ctypes(tmp_path):
    got = A.c_layout(tmp_path, "StFogDesc", FIELDS, ["ST_FOG_%s" % n for n in FALLOFFS] + ["ST_FOG_SKY", "ST_FOG_FOLLOW_SUN"])
    assert got == [112] + OFFSETS + [0, 1, 2, 3, 1, 2]


def _d(**kw):
    """a desc with every field valid for every falloff and flag, then `kw` over it (a tuple replaces a whole array, name_i one element)"""
    d = fog_desc(FogFalloff.EXPONENTIAL, color=(0.5, 0.6, 0.7, 0.9), start=1.0, end=20.0, density=0.1, height_falloff=0.1, height_reference=1.0, sky_distance=50.0,
                 extinction=(0.1, 0.2, 0.3), inscattering=(0.3, 0.2, 0.1), light_color=(1.0, 0.5, 0.25), light_exponent=8.0, light_direction=(0.0, 1.0, 0.0))
    d.flags = 0
    for k, v in kw.items():
        m = re.fullmatch(r"(\w+?)_(\d)", k)
        if m and hasattr(d, m.group(1)) and not hasattr(d, k):
            getattr(d, m.group(1))[int(m.group(2))] = v
        elif isinstance(v, tuple):
            setattr(d, k, (C.c_float * len(v))(*v))
        else:
            setattr(d, k, v)
    return d


BAD = [dict(struct_size=108), dict(struct_size=116), dict(struct_size=0), dict(falloff=4), dict(falloff=0xffffffff), dict(flags=4), dict(flags=0x80000001),
       dict(color_0=-0.1), dict(color_1=nan), dict(color_2=inf), dict(color_3=-0.01), dict(color_3=1.01), dict(color_3=nan),
       dict(falloff=0, start=nan), dict(falloff=0, end=inf), dict(falloff=0, start=5.0, end=5.0), dict(falloff=0, start=6.0, end=5.0), dict(falloff=0, start=-inf),
       dict(falloff=1, density=-1.0), dict(falloff=1, density=nan), dict(falloff=2, density=inf), dict(falloff=2, density=-0.5),
       dict(falloff=3, extinction_1=-1.0), dict(falloff=3, extinction_0=nan), dict(falloff=3, inscattering_2=inf), dict(falloff=3, inscattering_0=-2.0),
       dict(height_falloff=-0.1), dict(height_falloff=nan), dict(height_falloff=inf), dict(height_reference=nan), dict(height_reference=inf),
       dict(flags=1, sky_distance=0.0), dict(flags=1, sky_distance=-1.0), dict(flags=1, sky_distance=nan), dict(flags=3, sky_distance=inf),
       dict(light_color_0=-1.0), dict(light_color_1=nan), dict(light_color_2=inf),
       dict(light_exponent=0.0), dict(light_exponent=-8.0), dict(light_exponent=nan), dict(light_exponent=inf),
       dict(light_direction=(0.0, 0.0, 0.0)), dict(light_direction=(nan, 1.0, 0.0)), dict(light_direction=(0.0, inf, 0.0))]
# only the fields the falloff and the flags name are looked at
GOOD = [dict(falloff=f) for f in range(4)] + [dict(flags=1), dict(flags=2), dict(flags=3), dict(color=(0.0, 0.0, 0.0, 0.0)), dict(color_0=1e30), dict(color_3=1.0),
        dict(falloff=1, start=nan, end=-inf), dict(falloff=0, density=nan), dict(falloff=0, start=-5.0, end=-4.0), dict(falloff=1, extinction_0=nan, inscattering_1=-1.0),
        dict(falloff=3, density=-1.0, start=9.0, end=1.0), dict(density=0.0), dict(falloff=3, extinction=(0.0, 0.0, 0.0), inscattering=(0.0, 0.0, 0.0)),
        dict(height_falloff=0.0), dict(height_reference=-1e30), dict(sky_distance=nan), dict(flags=1, sky_distance=1e30),
        dict(light_color=(0.0, 0.0, 0.0), light_exponent=nan, light_direction=(0.0, 0.0, 0.0)), dict(flags=2, light_direction=(0.0, 0.0, 0.0)),
        dict(flags=2, light_direction=(nan, nan, nan)), dict(light_direction=(0.0, 0.0, 1e-30)), dict(light_exponent=1e-3), dict(_pad=123), dict(_pad2=nan)]


def test_argument_errors_on_a_host_only_engine():
    e, cam = _host_camera()
    def still_off(kw):
        assert not e.get_fog(cam)[1], kw   # a refused desc leaves the setting as it was

    A.argument_errors(e, cam, "camera_set_fog", "camera_get_fog", _d, BAD, GOOD, each_bad=still_off)
    with pytest.raises(StrolleError):
        e.set_fog(cam, falloff=7)
    e.close()


def test_process_checks_its_arguments_and_needs_a_device():
    e, cam = _host_camera()
    b, h = e._b, e._h
    d = _d()
    fake = C.c_void_p(4096)   # never dereferenced: the checks and the missing device come first
    manual, auto = display_desc(tonemap=Tonemap.ACES_FITTED, exposure_ev=1.0), display_desc(auto_exposure=True)
    bad_display = display_desc(tonemap=Tonemap.REINHARD)
    bad_display.tonemap = 9
    persp, ident = (C.c_float * 16)(*PERSPECTIVE), (C.c_float * 16)(*IDENTITY)

    def proj(**kw):
        p = list(PERSPECTIVE)
        for k, v in kw.items():
            p[int(k[1:])] = v
        return (C.c_float * 16)(*p)

    def fp(desc=d, display=None, transform=ident, projection=persp, color=fake, depth=fake, w=64, hh=48, dst=fake, fmt=0, engine=h):
        return b.fog_process(engine, C.byref(desc) if desc is not None else None, C.byref(display) if display is not None else None, transform, projection, color, depth,
                             w, hh, dst, fmt, None)

    assert fp() == ST_ERR_NO_DEVICE and fp(display=manual) == ST_ERR_NO_DEVICE and fp(desc=_d(flags=1, falloff=3)) == ST_ERR_NO_DEVICE
    assert fp(engine=None) == ST_ERR_INVALID_ARGUMENT
    for kw in (dict(desc=None), dict(transform=None), dict(projection=None), dict(color=None), dict(depth=None), dict(dst=None), dict(w=0), dict(hh=0), dict(w=16385),
               dict(hh=16385), dict(fmt=4), dict(fmt=-1), dict(display=auto), dict(display=bad_display), dict(desc=_d(struct_size=8)), dict(desc=_d(falloff=4)),
               dict(desc=_d(density=nan)), dict(desc=_d(flags=2)), dict(desc=_d(flags=3)), dict(projection=(C.c_float * 16)(*ORTHOGRAPHIC)), dict(projection=proj(p15=1.0)),
               dict(projection=proj(p5=0.0)), dict(projection=proj(p5=nan)), dict(projection=proj(p5=-2.0)), dict(projection=proj(p0=0.0)), dict(projection=proj(p0=inf))):
        assert fp(**kw) == ST_ERR_INVALID_ARGUMENT, kw
    assert fp(w=16384, hh=1) == ST_ERR_NO_DEVICE and fp(projection=proj(p0=-1.5, p8=0.1, p9=-0.2)) == ST_ERR_NO_DEVICE
    with pytest.raises(StrolleError):
        e.fog_process(d, IDENTITY, PERSPECTIVE, 4096, 4096, 64, 48, 4096)
    e.close()


def _values(d):
    return [list(getattr(d, f)) if hasattr(getattr(d, f), "__len__") else getattr(d, f) for f in FIELDS]


def test_set_get_clear_round_trips_and_survival_on_a_host_only_engine():
    e, cam = _host_camera()
    d0, on0 = e.get_fog(cam)
    assert not on0 and d0.struct_size == C.sizeof(api.StFogDesc) and all(v == 0 or v == [0.0] * len(v) for v in _values(d0)[1:])
    want = fog_desc(FogFalloff.ATMOSPHERIC, color=(0.1, 0.2, 0.3, 0.8), extinction=(0.01, 0.02, 0.03), inscattering=(0.03, 0.02, 0.01), height_falloff=0.25,
                    height_reference=-2.0, sky_distance=300.0, light_color=(1.0, 0.9, 0.8), light_exponent=16.0, light_direction=(1.0, 2.0, 3.0))
    assert want.flags == api.FOG_SKY and want.falloff == 3
    e.set_fog(cam, want)
    got, on = e.get_fog(cam)
    assert on and _values(got) == _values(want)
    e.tick()
    e.update_camera(cam, scenes.cornell_camera((80, 48)))   # a resize reallocates the camera: the setting stays
    got, on = e.get_fog(cam)
    assert on and _values(got) == _values(want)
    e.set_fog(cam, None)
    got, on = e.get_fog(cam)
    assert not on and got.falloff == 3   # the last desc stays readable
    e.set_fog(cam, density=0.05)
    got, on = e.get_fog(cam)
    assert on and got.falloff == FogFalloff.EXPONENTIAL and got.density == F(0.05) and got.flags == 0 and list(got.color) == [1.0, 1.0, 1.0, 1.0]
    # the pads are not kept
    e.set_fog(cam, _d(_pad=7, _pad2=3.0))
    got, _ = e.get_fog(cam)
    assert got._pad == 0 and got._pad2 == 0.0
    # fog_desc: a three-component colour gets alpha 1; follow_sun and sky_distance set the flags
    d = fog_desc(color=(0.2, 0.3, 0.4), follow_sun=True, sky_distance=10.0)
    assert list(d.color) == [F(0.2), F(0.3), F(0.4), 1.0] and d.flags == 3 and d.light_exponent == 8.0
    e.delete_camera(cam)
    e.close()


def test_fog_and_a_window_go_together_in_either_order_on_a_host_only_engine():
    e, cam = _host_camera()
    b, h = e._b, e._h
    d = _d()
    assert b.camera_set_window(h, cam, 0, 0, 32, 48) == ST_OK
    assert b.camera_set_fog(h, cam, C.byref(d)) == ST_OK                      # the window came first
    assert e.get_fog(cam)[1]
    assert b.camera_set_window(h, cam, 16, 8, 64, 48) == ST_OK                # fog came first
    assert b.camera_set_rows(h, cam, 0, 24) == ST_OK
    assert b.camera_set_window(h, cam, 0, 0, 0, 0) == ST_OK
    e.close()
    # st_dist_set_partition and st_dist_set_grid: two ranks through the in-process transport
    ranks = []
    for r in range(2):
        e = Engine(device=-1)
        scenes.build_cornell(e)
        cam = e.create_camera(scenes.cornell_camera((64, 48)))
        e.dist_init_local(r, 2, 9192)
        ranks.append((e, cam))
    (e0, c0), (e1, c1) = ranks
    e0.set_fog(c0, d)                                                         # fog, then the tile
    e0.dist_set_partition(c0)
    e1.dist_set_grid(c1, dist_grid(64, 48, 2))                                # the tile, then fog
    e1.set_fog(c1, d)
    for e, cam in ranks:
        assert e.get_fog(cam)[1]
        e.dist_shutdown(); e.close()


# ---------------------------------------------------------------- fog_f32 at cases worked out by hand
# W = H = 2, P[0] = P[5] = 1, no lens shift: the four pixels have ndc = (+-0.5, +-0.5), ax ax + ay ay + 1 = 1.5. A one-pixel frame looks
# along the axis: ndc = (0, 0), v = (0, 0, -1), so w = -M.col2: the third column of the transform picks the ray.
PROJ1 = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 0, -1.0, 0, 0, 0.1, 0]


def _along(direction, position=(0.0, 0.0, 0.0)):
    """a transform whose -col2 is `direction` (the ray of a one-pixel frame); the other two columns do not matter there"""
    m = np.eye(4)
    m[:3, 2] = [-v for v in direction]
    m[:3, 3] = position
    return m.T.reshape(-1).astype(np.float32)


def _one(d, D, colour=(0.25, 0.5, 1.0, 0.5), M=None, details=None):
    out = R.fog_f32(np.array([[colour]], np.float32), np.array([[D]], np.float32), _along((0, 0, -1)) if M is None else M, PROJ1, d, details=details)
    return out[0, 0]


def test_restatement_linear_and_exponential_by_hand():
    fogc = (2.0, 4.0, 8.0, 1.0)
    lin = fog_desc(FogFalloff.LINEAR, color=fogc, start=2.0, end=6.0)
    src = (0.25, 0.5, 1.0, 0.5)
    assert np.array_equal(_one(lin, 2.0), np.array(src, np.float32))            # at start g = 0: the pixel passes through, alpha kept
    assert np.array_equal(_one(lin, 1.0), np.array(src, np.float32))
    assert _one(lin, 6.0).tolist() == [2.0, 4.0, 8.0, 1.0]                      # at end g = 1: the fog colour, alpha 1
    assert _one(lin, 100.0).tolist() == [2.0, 4.0, 8.0, 1.0]
    assert _one(lin, 4.0).tolist() == [0.125 + 1.0, 0.25 + 2.0, 0.5 + 4.0, 1.0]  # the midpoint g = 0.5: c 0.5 + F 0.5, exact
    # a = 0.5 halves the cover: at end out = c 0.5 + F 0.5
    assert _one(fog_desc(FogFalloff.LINEAR, color=(2.0, 4.0, 8.0, 0.5), start=2.0, end=6.0), 6.0).tolist() == [1.125, 2.25, 4.5, 1.0]
    # EXPONENTIAL at d = 1 / density: g = 1 - exp2p(-1 * 1.4427), the polynomial's value of 1 - 1 / e to a few ulp
    ex = fog_desc(FogFalloff.EXPONENTIAL, color=(0.0, 0.0, 0.0, 1.0), density=0.25)
    det = {}
    out = _one(ex, 4.0, (1.0, 1.0, 1.0, 1.0), details=det)
    g = F(1) - R.exp2p(F(-1.0) * F(1.44269504088896341))
    assert det["ge"][0, 0, 0] == g and abs(float(g) - (1 - math.exp(-1))) < 2e-7
    assert out[0] == F(1) - g and abs(float(out[0]) - math.exp(-1)) < 2e-7
    # EXPONENTIAL_SQUARED: u = density d, g = 1 - exp(-(u u)): at u = 2 the exponent is -4
    sq = fog_desc(FogFalloff.EXPONENTIAL_SQUARED, color=(0.0, 0.0, 0.0, 1.0), density=0.5)
    R.fog_f32(np.ones((1, 1, 4), np.float32), np.array([[4.0]], np.float32), _along((0, 0, -1)), PROJ1, sq, details=det)
    assert abs(float(det["ge"][0, 0, 0]) - (1 - math.exp(-4))) < 2e-7
    # a = 0 and density 0: every factor is 0, the pixel passes through with its own words
    poison = (nan, -3.0, 1e30, 0.25)
    for d in (fog_desc(FogFalloff.EXPONENTIAL, color=(1.0, 1.0, 1.0, 0.0), density=1.0), fog_desc(FogFalloff.EXPONENTIAL, density=0.0),
              fog_desc(FogFalloff.ATMOSPHERIC, color=(1.0, 1.0, 1.0, 0.0), extinction=(1.0, 1.0, 1.0), inscattering=(1.0, 1.0, 1.0))):
        assert np.array_equal(_one(d, 5.0, poison).view(np.uint32), np.array(poison, np.float32).view(np.uint32))
    # ... while a fogged pixel clamps its colour: NaN and negatives to 0, large values to 65504
    full = fog_desc(FogFalloff.LINEAR, color=(0.0, 0.0, 0.0, 0.5), start=0.0, end=1.0)
    assert _one(full, 2.0, poison).tolist() == [0.0, 0.0, 32752.0, 1.0]


def test_restatement_every_pass_through_rule():
    d = fog_desc(FogFalloff.EXPONENTIAL, color=(1.0, 1.0, 1.0, 1.0), density=1.0)
    sky = fog_desc(FogFalloff.EXPONENTIAL, color=(1.0, 1.0, 1.0, 1.0), density=1.0, sky_distance=3.0)
    src = np.array((nan, -inf, 7.0, 0.3), np.float32)
    for D in (0.0, -0.0, -2.0, nan, -inf):                                       # D not > 0
        for dd in (d, sky):
            assert np.array_equal(_one(dd, D, src).view(np.uint32), src.view(np.uint32)), D
    for D in (R.FLT_MAX, inf):                                                   # sky: kept without ST_FOG_SKY, fogged at sky_distance with it
        assert np.array_equal(_one(d, D, src).view(np.uint32), src.view(np.uint32))
        assert np.array_equal(_one(sky, D, src), _one(d, 3.0, src)) and _one(sky, D, src)[3] == 1.0
    assert _one(d, 1e-30, (0.5, 0.5, 0.5, 0.5)).tolist() == [0.5, 0.5, 0.5, 0.5]  # an optical depth below half an ulp of 1: g = 0 in float32
    assert np.array_equal(R.frame_depth(np.array([0.0, 2.5], np.float32)), np.array([R.FLT_MAX, 2.5], np.float32))


def test_restatement_height_by_hand():
    # b = 0.5, the camera at y0 = 2 above the reference 0: E0 = exp(-1). A horizontal ray: k = 0, G = 1, d_e = d E0
    d = fog_desc(FogFalloff.LINEAR, color=(0.0, 0.0, 0.0, 1.0), start=0.0, end=1e9, height_falloff=0.5, height_reference=0.0)
    det = {}
    _one(d, 8.0, M=_along((1, 0, 0), (0, 2.0, 0)), details=det)
    E0 = F(math.exp(-1.0))
    assert det["E0"] == E0 and det["dy"][0, 0] == 0.0 and det["de"][0, 0] == F(8) * E0
    # straight up: k = b d = 4: d_e = d E0 (1 - e^-4) / 4, less than the horizontal ray's; straight down: k = -4, (1 - e^4) / -4, more
    _one(d, 8.0, M=_along((0, 1, 0), (0, 2.0, 0)), details=det)
    up = float(det["de"][0, 0])
    assert abs(up - 8 * math.exp(-1) * (1 - math.exp(-4)) / 4) < 1e-6 * up
    _one(d, 8.0, M=_along((0, -1, 0), (0, 2.0, 0)), details=det)
    down = float(det["de"][0, 0])
    assert abs(down - 8 * math.exp(-1) * (math.exp(4) - 1) / 4) < 1e-6 * down and up < 8 * math.exp(-1) < down
    # both sides of the series switch at |k| = 1 / 32: b d = 0.5 * d, so d = 0.0624 (k = 0.0312, the series) and d = 0.0626 (k = 0.0313, the quotient)
    for dist, series in ((0.0624, True), (0.0626, False), (0.0625, False)):
        _one(d, dist, M=_along((0, 1, 0)), details=det)
        k = F(F(0.5) * F(1.0)) * F(dist)
        G = F(1) - k * (F(0.5) - k * F(0.16666667)) if series else (F(1) - R.exp_(-k)) / k
        assert (abs(k) < F(0.03125)) == series and det["de"][0, 0] == F(dist) * (F(1) * G), dist
        assert abs(float(G) - (1 - math.exp(-float(k))) / float(k)) < 4e-6
    # k at both clamps: b dy d = +-0.5 * 1000: G = (1 - e^-80) / 80 = 1 / 80, and (1 - e^80) / -80
    _one(d, 1000.0, M=_along((0, 1, 0)), details=det)
    assert abs(float(det["de"][0, 0]) - 1000.0 / 80.0) < 1e-3
    _one(d, 1000.0, M=_along((0, -1, 0)), details=det)
    assert abs(float(det["de"][0, 0]) / (1000.0 * (math.exp(80) - 1) / 80.0) - 1) < 1e-5
    # E0's exponent at both clamps, and d_e held at FLT_MAX
    hi = fog_desc(FogFalloff.LINEAR, start=0.0, end=1.0, height_falloff=2.0)
    assert R.host_constants(hi, _along((1, 0, 0), (0, 100.0, 0)))[1] == F(math.exp(-80.0))
    assert R.host_constants(hi, _along((1, 0, 0), (0, -100.0, 0)))[1] == F(math.exp(80.0))
    _one(hi, 1e6, M=_along((0, -1, 0), (0, -100.0, 0)), details=det)
    assert det["de"][0, 0] == R.FLT_MAX


def test_restatement_light_lobe_and_atmospheric_by_hand():
    lobe = dict(light_color=(4.0, 0.0, 2.0), light_exponent=8.0, light_direction=(0.0, 0.0, -5.0))   # any length: normalised on the host
    d = fog_desc(FogFalloff.LINEAR, color=(1.0, 1.0, 1.0, 1.0), start=0.0, end=1.0, **lobe)
    black = (0.0, 0.0, 0.0, 1.0)
    assert R.host_constants(d, _along((0, 0, -1)))[0].tolist() == [0.0, 0.0, -1.0]
    assert _one(d, 5.0, black).tolist() == [5.0, 1.0, 3.0, 1.0]                  # s = 1: log2p(1) = 0, exp2p(0) = 1, F = color + light_color
    assert _one(d, 5.0, black, M=_along((1, 0, 0))).tolist() == [1.0, 1.0, 1.0, 1.0]     # s = 0: pow is 0
    assert _one(d, 5.0, black, M=_along((0, 0, 1))).tolist() == [1.0, 1.0, 1.0, 1.0]     # behind: max(-1, 0) = 0
    out = _one(d, 5.0, black, M=_along((math.sqrt(0.75), 0, -0.5)))              # cos 60 degrees: 0.5^8 = 1 / 256
    assert abs(float(out[0]) - (1 + 4 / 256)) < 2e-6 and out[1] == 1.0 and abs(float(out[2]) - (1 + 2 / 256)) < 2e-6
    # a transform with scale: s is held at 1, so the glow is no brighter than on the axis
    assert _one(d, 5.0, black, M=_along((0, 0, -3))).tolist() == [5.0, 1.0, 3.0, 1.0]
    # the lobe follows the sun with ST_FOG_FOLLOW_SUN
    sun = fog_desc(FogFalloff.LINEAR, color=(1.0, 1.0, 1.0, 1.0), start=0.0, end=1.0, light_color=(4.0, 0.0, 2.0), follow_sun=True)
    out = R.fog_f32(np.array([[black]], np.float32), np.array([[5.0]], np.float32), _along((0, 0, -1)), PROJ1, sun, sun=(0.0, 0.0, -1.0))
    assert out[0, 0].tolist() == [5.0, 1.0, 3.0, 1.0]
    # ATMOSPHERIC with one channel's extinction 0: that channel keeps its colour and only gains the in-scattered light
    atm = fog_desc(FogFalloff.ATMOSPHERIC, color=(1.0, 1.0, 1.0, 1.0), extinction=(0.0, 0.5, 1e9), inscattering=(0.5, 0.0, 1e9))
    det = {}
    out = _one(atm, 2.0, (0.25, 0.5, 1.0, 1.0), details=det)
    g = float(F(1) - R.exp2p(F(-1.0) * F(1.44269504088896341)))
    assert det["ge"][0, 0, 0] == 0.0 and det["gi"][0, 0, 1] == 0.0 and det["ge"][0, 0, 2] == 1.0 and det["gi"][0, 0, 2] == 1.0
    assert abs(float(out[0]) - (0.25 + g)) < 1e-6 and abs(float(out[1]) - 0.5 * (1 - g)) < 1e-6 and out[2] == 1.0
    # the ray of an off-axis pixel: W = H = 2, pixel (1, 0) has ndc = (0.5, 0.5), c = 1 / sqrt(1.5)
    R.fog_f32(np.zeros((2, 2, 4), np.float32), np.ones((2, 2), np.float32), IDENTITY, PROJ1, fog_desc(density=1.0), details=det)
    c = F(1) / np.sqrt(F(F(0.25) + F(0.25)) + F(1))
    assert [float(v[0, 1]) for v in det["w"]] == [float(F(0.5) * c), float(F(0.5) * c), float(-c)]


# ---------------------------------------------------------------- the restatement against the definition
def restatement_vs_definition():
    """the worst |fog_f32 - fog_f64| / (max c' + max F) over the input matrix, finite-depth pixels only; tools/fog_bench.py writes it to
    profiles/fog.json. A pixel whose factors underflow to 0 in float32 alone passes through there and not in the definition: it is compared
    where its colour is its own clamp (elsewhere the two differ by the clamp, by the rule and not by rounding)."""
    worst, where, pixels = 0.0, None, 0
    for name, size, kind, t, d in K.cases():
        img, z, M, P = K.inputs(size, kind, t)
        d32, d64 = {}, {}
        a = R.fog_f32(img, z, M, P, d, details=d32)
        b, fogged = R.fog_f64(img, z, M, P, d, details=d64)
        clean = np.isfinite(img).all(-1) & np.isfinite(z)
        assert not np.isnan(a[clean]).any(), f"{name}: NaN from finite inputs"
        assert np.isfinite(a[clean & (img[..., :3] <= 65504).all(-1)]).all(), name
        m = np.isfinite(z) & (z > 0) & (z < R.FLT_MAX) & fogged
        assert not (d32["fogged"] & ~fogged).any(), name
        own = ((img[..., :3] >= 0) & (img[..., :3] <= 65504)).all(-1)
        m &= d32["fogged"] | own
        if not m.any():
            continue
        with np.errstate(all="ignore"):
            err = np.abs(a[..., :3].astype(np.float64) - b).max(-1) / (d64["cc"].max(-1) + d64["F"].max(-1))
        pixels += int(m.sum())
        if err[m].max() > worst:
            worst, where = float(err[m].max()), name
    return worst, where, pixels


def test_restatement_agrees_with_the_float64_definition():
    """Measured on the input matrix: 8.7e-7 (profiles/fog.json restatement_vs_definition); the bound is four times that figure, the margin
    the surface-attribute tests give a measured deviation, which leaves room for another libm."""
    recorded = json.load(open(os.path.join(ROOT, "profiles", "fog.json")))["restatement_vs_definition"]["worst"]
    worst, where, pixels = restatement_vs_definition()
    print(f"restatement against the definition: worst {worst:.3e} at {where} over {pixels} pixels; recorded {recorded:.3e}, bound {4 * recorded:.3e}")
    assert pixels > 50000 and 0 < recorded < 2e-6
    assert worst <= 4 * recorded, (worst, where)
