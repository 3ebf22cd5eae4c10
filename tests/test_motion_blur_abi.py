"""CPU tests of motion blur (include/strolle_hip.h "motion blur"): the entry points are exported, declared and bound by the Rust facade,
StMotionBlurDesc has one layout in the header, api.py and ffi.rs, every argument error occurs on a host-only engine, set / get round-trip
there (also across st_camera_update), a window and the blur exclude each other in both orders, st_motion_blur_process says that it needs a
device, and the numpy restatement (motion_blur_ref.py) at cases worked out by hand."""
import ctypes as C
import os

import numpy as np
import pytest

import motion_blur_ref as R
import output_chain_abi as A
from strolle_amd import StrolleError, Tonemap, display_desc, motion_blur_desc, scenes
from output_chain_abi import ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE, host_camera as _host_camera
from strolle_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("st_camera_set_motion_blur", "st_camera_get_motion_blur", "st_motion_blur_process")
FIELDS = ["struct_size", "flags", "samples", "shutter", "max_radius", "depth_softness"]
F = np.float32


def test_entry_points_are_exported_declared_and_bound():
    A.exports_header_and_ffi_agree("StMotionBlurDesc", FIELDS, ENTRY_POINTS, [("ST_MOTION_BLUR_NO_JITTER", 1)])
    assert api.MOTION_BLUR_NO_JITTER == R.NO_JITTER == 1


def test_desc_layout_agrees_between_c_and_ctypes(tmp_path):
    got = A.c_layout(tmp_path, "StMotionBlurDesc", FIELDS, ["ST_MOTION_BLUR_NO_JITTER"])
    assert got == [24, 0, 4, 8, 12, 16, 20, 1]


def _d(**kw):
    d = motion_blur_desc(shutter=0.5, samples=8, max_radius=16.0, depth_softness=0.1)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


inf, nan = float("inf"), float("nan")
BAD = [dict(struct_size=20), dict(struct_size=28), dict(struct_size=0), dict(flags=2), dict(flags=0x80000001), dict(samples=1), dict(samples=3),
       dict(samples=31), dict(samples=34), dict(samples=64), dict(samples=0xffffffff), dict(shutter=nan), dict(shutter=inf), dict(shutter=-0.01),
       dict(shutter=4.01), dict(max_radius=nan), dict(max_radius=inf), dict(max_radius=-1.0), dict(max_radius=32.5),
       dict(depth_softness=nan), dict(depth_softness=inf), dict(depth_softness=-0.1), dict(depth_softness=1.01)]
GOOD = [dict(flags=1), dict(samples=0), dict(samples=2), dict(samples=32), dict(shutter=0.0), dict(shutter=4.0), dict(max_radius=0.0),
        dict(max_radius=32.0), dict(max_radius=0.25), dict(depth_softness=0.0), dict(depth_softness=1.0)]


def test_argument_errors_on_a_host_only_engine():
    e, cam = _host_camera()
    A.argument_errors(e, cam, "camera_set_motion_blur", "camera_get_motion_blur", _d, BAD, GOOD)
    with pytest.raises(StrolleError):
        e.set_motion_blur(cam, samples=5)
    e.close()


def test_process_checks_its_arguments_and_needs_a_device():
    e, cam = _host_camera()
    b, h = e._b, e._h
    d = _d()
    fake = C.c_void_p(4096)   # never dereferenced: the checks and the missing device come first
    manual, auto = display_desc(tonemap=Tonemap.ACES_FITTED, exposure_ev=1.0), display_desc(auto_exposure=True)
    bad_display = display_desc(tonemap=Tonemap.REINHARD)
    bad_display.tonemap = 9

    def mp(desc=d, display=None, color=fake, vel=fake, depth=fake, w=64, hh=48, dst=fake, fmt=0, engine=h):
        return b.motion_blur_process(engine, C.byref(desc) if desc is not None else None, C.byref(display) if display is not None else None, color, vel, depth,
                                     w, hh, dst, fmt, None)

    assert mp() == ST_ERR_NO_DEVICE and mp(display=manual) == ST_ERR_NO_DEVICE
    assert mp(engine=None) == ST_ERR_INVALID_ARGUMENT
    for kw in (dict(desc=None), dict(color=None), dict(vel=None), dict(depth=None), dict(dst=None), dict(w=0), dict(hh=0), dict(w=16385), dict(hh=16385),
               dict(fmt=4), dict(fmt=-1), dict(display=auto), dict(display=bad_display), dict(desc=_d(struct_size=8)), dict(desc=_d(samples=7)),
               dict(desc=_d(shutter=nan))):
        assert mp(**kw) == ST_ERR_INVALID_ARGUMENT, kw
    assert mp(w=16384, hh=1) == ST_ERR_NO_DEVICE
    with pytest.raises(StrolleError):
        e.motion_blur_process(d, 4096, 4096, 4096, 64, 48, 4096)
    e.close()


def test_set_get_round_trip_and_survival_on_a_host_only_engine():
    e, cam = _host_camera()
    d0, on0 = e.get_motion_blur(cam)
    assert not on0 and d0.struct_size == C.sizeof(api.StMotionBlurDesc) and all(getattr(d0, f) == 0 for f in FIELDS[1:])
    want = motion_blur_desc(shutter=1.25, samples=12, max_radius=20.0, depth_softness=0.2, jitter=False)
    e.set_motion_blur(cam, want)
    got, on = e.get_motion_blur(cam)
    assert on and [getattr(got, f) for f in FIELDS] == [getattr(want, f) for f in FIELDS]
    e.tick()
    e.update_camera(cam, scenes.cornell_camera((80, 48)))   # a resize reallocates the camera: the setting stays
    got, on = e.get_motion_blur(cam)
    assert on and [getattr(got, f) for f in FIELDS] == [getattr(want, f) for f in FIELDS]
    e.set_motion_blur(cam, None)
    got, on = e.get_motion_blur(cam)
    assert not on and got.samples == 12   # the last desc stays readable
    e.set_motion_blur(cam, shutter=0.5)
    assert e.get_motion_blur(cam)[1] and e.get_motion_blur(cam)[0].samples == 0
    e.delete_camera(cam)
    e.close()


def test_the_blur_and_a_window_exclude_each_other_on_a_host_only_engine():
    e, cam = _host_camera()
    d = _d()
    A.node_and_window_exclude_each_other(e, cam, "camera_set_motion_blur", d, lambda: e.get_motion_blur(cam)[1])
    e.close()


# ---------------------------------------------------------------- motion_blur_ref.py at cases worked out by hand
def test_reference_pack_rest_clamp_and_nan():
    V = np.array([[[0.6, 0.0], [100.0, 0.0], [nan, 1.0], [3.0, 4.0], [0.0, -1.0]]], np.float32)
    # shutter 1: h = 0.5. (0.6, 0) -> |v| = 0.3 < 0.5: at rest. (100, 0) -> v = 50, above R = 4: k = 4 / 50, v = 50 k, r = 4 exactly.
    # NaN -> r is NaN, "not r >= 0.5": at rest. (3, 4) -> v = (1.5, 2), r = sqrt(2.25 + 4) = 2.5: kept. (0, -1) -> r = 0.5: kept (>= 0.5)
    v, r = R.pack(V, 1.0, 4.0)
    assert r.tolist() == [[0.0, 4.0, 0.0, 2.5, 0.5]]
    assert v[0, 0].tolist() == [0.0, 0.0] and v[0, 2].tolist() == [0.0, 0.0]
    assert v[0, 1, 0] == F(50) * (F(4) / F(50)) and v[0, 1, 1] == 0.0 and abs(float(v[0, 1, 0]) - 4.0) < 1e-6
    assert v[0, 3].tolist() == [1.5, 2.0] and v[0, 4].tolist() == [0.0, -0.5]
    # the default radius is 32; a zero shutter puts everything at rest
    assert R.pack(V, 1.0)[1].tolist() == [[0.0, 32.0, 0.0, 2.5, 0.5]]
    assert not R.pack(V, 0.0)[1].any()
    assert np.array_equal(R.frame_depth(np.array([0.0, 2.5], np.float32)), np.array([R.FLT_MAX, 2.5], np.float32))


def test_reference_tile_and_neighbour_tie_rules():
    w, h = 70, 40   # 3 x 2 tiles; the last column of tiles is 6 pixels wide, the last row 8 pixels high
    V = np.zeros((h, w, 2), np.float32)
    V[9, 3] = (0.0, 10.0)     # tile (0, 0), row 9: the later of two equal maxima
    V[7, 5] = (10.0, 0.0)     # tile (0, 0), row 7: the first in row-major order
    V[2, 66] = (0.0, -10.0)   # tile (2, 0)
    V[20, 40] = (3.0, 0.0)    # tile (1, 0): a smaller one
    v, r = R.pack(V, 2.0)     # shutter 2: h = 1, v = V
    assert r[9, 3] == r[7, 5] == r[2, 66] == 10.0 and r[20, 40] == 3.0
    t = R.tile_max(v, r)
    assert t.shape == (2, 3, 3)
    assert t[0, 0].tolist() == [10.0, 0.0, 10.0] and t[0, 1].tolist() == [3.0, 0.0, 3.0] and t[0, 2].tolist() == [0.0, -10.0, 10.0]
    assert not t[1].any()     # tiles at rest have vector 0
    n = R.neighbour_max(t)
    # tile (1, 0) sees 10 in (dy, dx) = (0, -1) and (0, 1): the first wins. Tile (1, 1) sees them at (-1, -1) and (-1, 1): likewise.
    assert n[0, 1].tolist() == [10.0, 0.0, 10.0] and n[1, 1].tolist() == [10.0, 0.0, 10.0]
    assert n[0, 0].tolist() == [10.0, 0.0, 10.0] and n[1, 0].tolist() == [10.0, 0.0, 10.0]
    # tile (2, 0): (0, -1) has 3, itself 10. Tile (2, 1): (-1, -1) has 3, (-1, 0) has 10
    assert n[0, 2].tolist() == [0.0, -10.0, 10.0] and n[1, 2].tolist() == [0.0, -10.0, 10.0]


def test_reference_one_gather_pixel_with_two_taps_by_hand():
    w, h = 40, 8
    V = np.zeros((h, w, 2), np.float32)
    V[..., 0] = 8.0                       # shutter 1 -> v = (4, 0), r = 4 everywhere: n = (4, 0), r_n = 4
    Z = np.full((h, w), 10.0, np.float32)
    Cc = np.zeros((h, w, 4), np.float32)
    Cc[..., 3] = 1.0
    Cc[3, 10, 0], Cc[3, 8, 0], Cc[3, 12, 0] = 1.0, 2.0, 4.0
    d = {}
    out = R.motion_blur(Cc, V, Z, shutter=1.0, samples=2, flags=R.NO_JITTER, details=d)
    # S = 2, j = 0: t = ((0 + 0.5) 2) / 2 - 1 = -0.5 and ((1 + 0.5) 2) / 2 - 1 = 0.5; p.x = 10.5 -+ 2 -> texels 8 and 12 of row 3
    (x0, y0, w0), (x1, y1, w1) = d["taps"]
    assert (x0[3, 10], y0[3, 10], x1[3, 10], y1[3, 10]) == (8, 3, 12, 3)
    # d = 0.5 * 4 = 2; equal depths: f = b = 1; cone(2, 4) = 0.5; cyl(2, 4) = 1 (2 < 0.95 * 4); w = (0.5 + 0.5) + (1 * 1) * 2 = 3
    assert w0[3, 10] == 3.0 and w1[3, 10] == 3.0
    # w_0 = 1 / 4; sum = 1 * 0.25 + 2 * 3 + 4 * 3 = 18.25; wsum = 6.25
    assert d["wsum"][3, 10] == 6.25
    assert out[3, 10, 0] == F(18.25) / F(6.25) and out[3, 10, 1] == 0.0 and out[3, 10, 3] == 1.0
    # at the left edge both coordinates clamp: pixel (0, 3) taps texel 0 (p.x = -1.5 -> floor -2 -> 0) and texel 2
    assert (x0[3, 0], x1[3, 0]) == (0, 2)
    # a tap across a depth edge further than e = 0.05 * min(Z) behind the pixel: b = 1 (the pixel is in front), f = 0
    Z2 = Z.copy()
    Z2[:, 12] = 20.0
    d2 = {}
    R.motion_blur(Cc, V, Z2, shutter=1.0, samples=2, flags=R.NO_JITTER, details=d2)
    assert d2["taps"][1][2][3, 10] == 0.5 + 2.0   # (0 * 0.5 + 1 * 0.5) + 2
    # with the whole field at rest the colour passes with its own bits
    Cc[0, 0] = (np.nan, np.inf, -1.0, 0.5)
    rest = R.motion_blur(Cc, V * 0, Z, shutter=1.0, samples=2)
    assert np.array_equal(rest.view(np.uint32), Cc.view(np.uint32))


def test_reference_bayer_jitter():
    j = R.jitter(8, 8)
    assert j[0, 0] == -0.46875 and j[0, 1] == 0.03125 and j[3, 3] == -0.15625 and j[3, 0] == 0.46875 and j[1, 2] == (14.5 / 16 - 0.5)
    assert np.array_equal(j[:4, :4], j[4:, 4:]) and sorted(((j[:4, :4] + 0.5) * 16 - 0.5).ravel().tolist()) == list(range(16))
    assert not R.jitter(8, 8, R.NO_JITTER).any()
