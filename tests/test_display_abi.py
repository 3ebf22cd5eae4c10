"""CPU tests of camera display transforms (include/strolle_hip.h "display transforms"): the entry points are exported, declared and bound by
the Rust facade, StDisplayDesc has one layout in the header, api.py and ffi.rs, every argument error occurs on a host-only engine, set / get
round-trip there, the device-only calls say so, and the numpy restatement (display_ref.py) gives hand-computed values."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import display_ref as R
import output_chain_abi as A
from strolle_amd import StrolleError, Tonemap, display_desc, scenes
from output_chain_abi import ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE, ST_ERR_UNKNOWN_CAMERA, ST_OK, host_camera as _host_camera
from strolle_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("st_camera_set_display", "st_camera_get_display", "st_camera_exposure", "st_debug_camera_histogram")
FIELDS = ["struct_size", "tonemap", "flags", "exposure_ev", "ev_min", "ev_max", "low_fraction", "high_fraction", "max_ev_step_up", "max_ev_step_down"]


def test_entry_points_are_exported_declared_and_bound():
    _, ffi = A.exports_header_and_ffi_agree("StDisplayDesc", FIELDS, ENTRY_POINTS, [("ST_TONEMAP_%s" % t.name, t.value) for t in Tonemap])
    assert "pub const ST_DISPLAY_AUTO_EXPOSURE: u32 = 1;" in ffi


def test_desc_layout_agrees_between_c_and_ctypes(tmp_path):
    got = A.c_layout(tmp_path, "StDisplayDesc", FIELDS, ["ST_DISPLAY_AUTO_EXPOSURE", "ST_TONEMAP_ACES_FITTED", "ST_TONEMAP_PBR_NEUTRAL"])
    assert got == [40] + [4 * k for k in range(len(FIELDS))] + [1, 3, 4]
    assert got[-3:] == [api.DISPLAY_AUTO_EXPOSURE, Tonemap.ACES_FITTED, Tonemap.PBR_NEUTRAL]


def _d(**kw):
    d = display_desc(Tonemap.ACES_FITTED, auto_exposure=True)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_errors_on_a_host_only_engine():
    e, cam = _host_camera()
    b, h = e._b, e._h

    def st(d, camera=cam, engine=h):
        return b.camera_set_display(engine, camera, C.byref(d) if d is not None else None)

    assert st(_d()) == ST_OK and st(None) == ST_OK
    assert st(_d(), engine=None) == ST_ERR_INVALID_ARGUMENT
    assert st(_d(), camera=cam + 99) == ST_ERR_UNKNOWN_CAMERA and st(None, camera=cam + 99) == ST_ERR_UNKNOWN_CAMERA
    inf, nan = float("inf"), float("nan")
    bad = [_d(struct_size=36), _d(struct_size=44), _d(struct_size=0), _d(tonemap=5), _d(tonemap=0xffffffff), _d(flags=2), _d(flags=0x80000001)]
    for f in FIELDS[3:]:
        bad += [_d(**{f: nan}), _d(**{f: inf}), _d(**{f: -inf})]
    bad += [_d(ev_min=2.0, ev_max=2.0), _d(ev_min=3.0, ev_max=-3.0), _d(low_fraction=-0.01), _d(high_fraction=1.01),
            _d(low_fraction=0.5, high_fraction=0.5), _d(low_fraction=0.6, high_fraction=0.4), _d(max_ev_step_up=-0.1), _d(max_ev_step_down=-1e-6)]
    for d in bad:
        assert st(d) == ST_ERR_INVALID_ARGUMENT, [getattr(d, f) for f in FIELDS]
        for f in FIELDS[3:]:   # a non-finite field is refused with auto off too
            if not math.isfinite(getattr(d, f)):
                d.flags = 0
                assert st(d) == ST_ERR_INVALID_ARGUMENT, f
    # with auto off the auto-only fields are stored unchecked
    loose = _d(flags=0, ev_min=5.0, ev_max=-5.0, low_fraction=2.0, high_fraction=-1.0, max_ev_step_up=-3.0)
    assert st(loose) == ST_OK
    got, on = e.display(cam)
    assert on and [getattr(got, f) for f in FIELDS] == [getattr(loose, f) for f in FIELDS]
    # edge values that are valid
    for d in (_d(low_fraction=0.0, high_fraction=1.0), _d(max_ev_step_up=0.0, max_ev_step_down=0.0), _d(exposure_ev=-20.0, ev_min=-30.0, ev_max=30.0)):
        assert st(d) == ST_OK
    # get: pointers may be NULL; unknown camera
    assert b.camera_get_display(h, cam, None, None) == ST_OK
    assert b.camera_get_display(h, cam + 99, None, None) == ST_ERR_UNKNOWN_CAMERA
    # device-only calls
    s = C.c_float()
    bins = (C.c_uint32 * 64)()
    assert b.camera_exposure(h, cam, C.byref(s), None, None) == ST_ERR_NO_DEVICE
    assert b.debug_camera_histogram(h, cam, bins) == ST_ERR_NO_DEVICE
    assert b.camera_exposure(h, cam + 99, None, None, None) == ST_ERR_UNKNOWN_CAMERA
    assert b.debug_camera_histogram(h, cam, None) == ST_ERR_INVALID_ARGUMENT
    with pytest.raises(StrolleError):
        e.exposure(cam)
    with pytest.raises(StrolleError):
        e.set_display(cam, tonemap=9)
    e.close()


def test_set_get_round_trip_on_a_host_only_engine():
    e, cam = _host_camera()
    d0, on0 = e.display(cam)
    assert not on0 and d0.struct_size == C.sizeof(api.StDisplayDesc) and all(getattr(d0, f) == 0 for f in FIELDS[1:])
    want = display_desc(Tonemap.PBR_NEUTRAL, exposure_ev=-1.25, auto_exposure=True, ev_min=-10.0, ev_max=6.0, low_fraction=0.05,
                        high_fraction=0.95, max_ev_step_up=0.5, max_ev_step_down=0.25)
    e.set_display(cam, want)
    got, on = e.display(cam)
    assert on and [getattr(got, f) for f in FIELDS] == [getattr(want, f) for f in FIELDS]
    e.tick()
    e.update_camera(cam, scenes.cornell_camera((80, 48)))   # a resize reallocates the camera: the display stays
    got, on = e.display(cam)
    assert on and got.tonemap == Tonemap.PBR_NEUTRAL and got.ev_min == -10.0
    e.set_display(cam, None)
    got, on = e.display(cam)
    assert not on and got.tonemap == Tonemap.PBR_NEUTRAL   # the last desc stays readable
    e.set_display(cam, tonemap=Tonemap.REINHARD, exposure_ev=2.0)
    got, on = e.display(cam)
    assert on and got.tonemap == Tonemap.REINHARD and got.flags == 0 and got.exposure_ev == 2.0
    e.delete_camera(cam)
    e.close()


def test_auto_exposure_and_a_window_exclude_each_other_on_a_host_only_engine():
    e, cam = _host_camera()
    b, h = e._b, e._h
    auto = _d()
    assert b.camera_set_window(h, cam, 0, 0, 32, 48) == ST_OK
    assert b.camera_set_display(h, cam, C.byref(auto)) == ST_ERR_INVALID_ARGUMENT   # the window came first
    manual = _d(flags=0)
    assert b.camera_set_display(h, cam, C.byref(manual)) == ST_OK                  # manual exposure works with windows
    assert b.camera_set_window(h, cam, 0, 0, 0, 0) == ST_OK                         # back to the whole frame
    assert b.camera_set_display(h, cam, C.byref(auto)) == ST_OK
    assert b.camera_set_window(h, cam, 16, 0, 64, 48) == ST_ERR_INVALID_ARGUMENT   # auto came first
    assert b.camera_set_window(h, cam, 0, 8, 64, 48) == ST_ERR_INVALID_ARGUMENT
    assert b.camera_set_window(h, cam, 0, 0, 64, 48) == ST_OK                       # the whole frame is no tile
    e.close()


# ---------------------------------------------------------------- display_ref.py against values worked out by hand
def _one(c, op, s=1.0):
    return R.transform(np.array([c], np.float32), op, s)[0, :3].astype(np.float64)


def test_reference_operators_at_hand_computed_values():
    nan, inf = float("nan"), float("inf")
    # NONE: exposure only, negatives and NaN pass
    got = _one([1.0, -2.0, nan], R.NONE, 4.0)
    assert got[0] == 4.0 and got[1] == -8.0 and math.isnan(got[2])
    assert R.manual_scale(-1.0) == np.float32(0.5) and R.manual_scale(3.0) == np.float32(8.0)
    # REINHARD: x / (1 + x); negatives and NaN -> 0
    assert np.allclose(_one([1.0, 3.0, 0.0], R.REINHARD), [0.5, 0.75, 0.0], rtol=0, atol=1e-7)
    assert np.array_equal(_one([-1.0, nan, 0.0], R.REINHARD), [0.0, 0.0, 0.0])
    assert np.allclose(_one([1e30, 1.0, 1.0], R.REINHARD), [1.0, 0.5, 0.5], atol=1e-7)
    # REINHARD_LUMINANCE: grey 1 -> Y = 1 -> 0.5; a red pixel of 1: Y = 0.2126
    assert np.allclose(_one([1.0, 1.0, 1.0], R.REINHARD_LUMINANCE), [0.5, 0.5, 0.5], atol=1e-7)
    assert np.allclose(_one([1.0, 0.0, 0.0], R.REINHARD_LUMINANCE), [1 / 1.2126, 0.0, 0.0], rtol=1e-6)
    assert np.allclose(_one([-5.0, 2.0, nan], R.REINHARD_LUMINANCE), [0.0, 2 / (1 + 2 * 0.7152), 0.0], rtol=1e-6)
    # ACES fitted: black -> clamp(M_out * (-0.000090537 / 0.238081)) = 0; grey 0.18 -> 0.1056; huge -> 1 (rows of M_out sum to 1)
    assert np.array_equal(_one([0.0, 0.0, 0.0], R.ACES_FITTED), [0.0, 0.0, 0.0])
    v = 0.18 * (0.59719 + 0.35458 + 0.04823)
    f = (v * (v + 0.0245786) - 0.000090537) / (v * (0.983729 * v + 0.4329510) + 0.238081)
    grey = (1.60475 - 0.53108 - 0.07367) * f
    assert np.allclose(_one([0.18, 0.18, 0.18], R.ACES_FITTED), [grey] * 3, rtol=1e-4) and abs(grey - 0.10559) < 1e-5
    assert np.allclose(_one([1e6, 1e6, 1e6], R.ACES_FITTED), [1.0, 1.0, 1.0], atol=1e-5)
    assert np.array_equal(_one([-1.0, nan, -inf], R.ACES_FITTED), [0.0, 0.0, 0.0])
    # PBR neutral: below the knee only the offset; grey 0.5 -> x = 0.5 >= 0.08, offset 0.04 -> 0.46
    assert np.allclose(_one([0.5, 0.5, 0.5], R.PBR_NEUTRAL), [0.46, 0.46, 0.46], atol=1e-7)
    x = 0.05
    assert np.allclose(_one([x, 0.3, 0.6], R.PBR_NEUTRAL), [x - (x - 6.25 * x * x), 0.3 - (x - 6.25 * x * x), 0.6 - (x - 6.25 * x * x)], atol=1e-7)
    assert np.array_equal(_one([0.0, 0.0, 0.0], R.PBR_NEUTRAL), [0.0, 0.0, 0.0])
    # above the knee: white 2 -> peak 1.96, np = 1 - 0.0576 / 1.44 = 0.96, colour 0.96 (grey stays grey)
    assert np.allclose(_one([2.0, 2.0, 2.0], R.PBR_NEUTRAL), [0.96, 0.96, 0.96], atol=1e-6)
    # a saturated red of 4: x = 0 -> offset 0; peak 4, np = 1 - 0.0576 / 3.48; r = np, g = b = np * g_mix
    npk = 1 - 0.0576 / 3.48
    w = 1 - 1 / (0.15 * (4 - npk) + 1)
    assert np.allclose(_one([4.0, 0.0, 0.0], R.PBR_NEUTRAL), [npk, npk * w, npk * w], atol=1e-6)
    # exposure multiplies before the operator
    assert np.array_equal(_one([0.25, 0.5, 1.0], R.REINHARD, 4.0), _one([1.0, 2.0, 4.0], R.REINHARD))
    assert R.transform(np.zeros((2, 3, 3), np.float32), R.ACES_FITTED, 1.0).shape == (2, 3, 4)


def test_reference_metering_at_hand_computed_values():
    # bins over [-8, 8): 4 bins per EV; Y = 1 -> log2 = 0 -> bin 32; Y = 0.18 -> log2 = -2.47 -> bin floor(22.1) = 22
    c = np.array([[1, 1, 1], [0.18, 0.18, 0.18], [0, 0, 0], [-1, -1, -1], [np.nan, 0, 0], [np.inf, 0, 0], [1e-30, 1e-30, 1e-30], [1e30, 0, 0]], np.float32)
    assert list(R.bins(c, -8.0, 8.0)) == [32, 22, 0, 0, 0, 63, 0, 63]
    h = R.histogram(c, -8.0, 8.0)
    assert h.sum() == len(c) and h[0] == 4 and h[63] == 2
    # kept ranks: 10 pixels, [0.1, 0.9) keeps ranks 1..8; bins 10 x 5 and 20 x 5 -> centre mean of 4 and 4 pixels
    counts = np.zeros(64, np.int64); counts[10] = 5; counts[20] = 5
    centre = lambda k: -8.0 + (k + 0.5) * 0.25
    assert R.metered_ev(counts, 0.1, 0.9, -8.0, 8.0) == np.float32((4 * centre(10) + 4 * centre(20)) / 8)
    # a partial bin at the high end: [0, 0.55) of 10 keeps ceil(5.5) = 6 ranks -> 5 in bin 10 and 1 in bin 20
    assert R.metered_ev(counts, 0.0, 0.55, -8.0, 8.0) == np.float32((5 * centre(10) + centre(20)) / 6)
    assert R.metered_ev(np.zeros(64), 0.1, 0.9, -8.0, 8.0) is None
    # adaptation: first frame takes the target; later steps are bounded, within the bound it lands on the target
    assert R.adapt(-2.0, 3.0, False, 0.5, 0.5) == np.float32(3.0)
    assert R.adapt(-2.0, 3.0, True, 0.5, 0.5) == np.float32(-1.5)
    assert R.adapt(2.0, -3.0, True, 0.5, 0.25) == np.float32(1.75)
    assert R.adapt(2.0, 2.3, True, 0.5, 0.5) == np.float32(2.3)
    assert R.adapt(-2.0, 3.0, True, 0.0, 0.0) == np.float32(3.0)
    assert R.auto_scale(0.0, math.log2(0.18)) == pytest.approx(1.0, rel=1e-6)
    assert R.auto_scale(1.0, 0.0) == np.float32(0.36)
    assert list(R.srgb8([0.0, 1.0, 2.0, -1.0, 0.5])) == [0, 255, 255, 0, 188]
