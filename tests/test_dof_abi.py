"""CPU tests of depth of field (include/strolle_hip.h "depth of field"): the entry points are exported, declared and bound by the Rust
facade, StDofDesc has one layout in the header, api.py and ffi.rs, every argument error occurs on a host-only engine, set / get round-trip
there (also across st_camera_update), a window and depth of field exclude each other in both orders through all three window setters,
st_dof_plan's sample count, tile counts and tap table, st_dof_process says that it needs a device, and the numpy restatement (dof_ref.py)
at cases worked out by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dof_ref as R
import output_chain_abi as A
from strolle_amd import Engine, StrolleError, Tonemap, display_desc, dof_desc, dof_plan, scenes
from output_chain_abi import ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE, ST_OK, host_camera as _host_camera
from strolle_amd import api
from strolle_amd.api import dist_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("st_camera_set_dof", "st_camera_get_dof", "st_dof_plan", "st_dof_process")
FIELDS = ["struct_size", "flags", "samples", "focal_distance", "aperture_f_stops", "sensor_height", "max_radius", "focus_x", "focus_y", "_pad"]
F = np.float32
PERSPECTIVE = [1.5, 0, 0, 0, 0, 2.0, 0, 0, 0, 0, 0, -1.0, 0, 0, 0.1, 0]   # column major, infinite reverse-z: [15] == 0
ORTHOGRAPHIC = [0.5, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, -0.01, 0, 0, 0, 1.0, 1.0]


def test_entry_points_are_exported_declared_and_bound():
    header, _ = A.exports_header_and_ffi_agree("StDofDesc", FIELDS, ENTRY_POINTS, [("ST_DOF_AUTOFOCUS", 1), ("ST_DOF_PLANAR_DEPTH", 2)])
    assert api.DOF_AUTOFOCUS == R.AUTOFOCUS == 1 and api.DOF_PLANAR_DEPTH == R.PLANAR_DEPTH == 2
    # the three new kernel slots need a larger profiler table, and api.py sizes its array with the constant
    assert re.search(r"ST_PROFILE_MAX_KERNELS = 64\b", header) and api.PROFILE_MAX_KERNELS == 64


def test_desc_layout_agrees_between_c_and_ctypes(tmp_path):
    got = A.c_layout(tmp_path, "StDofDesc", FIELDS, ["ST_DOF_AUTOFOCUS", "ST_DOF_PLANAR_DEPTH"])
    assert got == [40, 0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 1, 2]


def _d(**kw):
    d = dof_desc(focal_distance=3.0, aperture_f_stops=2.0, sensor_height=0.024, samples=16, max_radius=16.0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


inf, nan = float("inf"), float("nan")
BAD = [dict(struct_size=36), dict(struct_size=44), dict(struct_size=0), dict(flags=4), dict(flags=0x80000001), dict(samples=1), dict(samples=3),
       dict(samples=65), dict(samples=0xffffffff), dict(focal_distance=0.0), dict(focal_distance=-1.0), dict(focal_distance=nan), dict(focal_distance=inf),
       dict(aperture_f_stops=-1.0), dict(aperture_f_stops=nan), dict(aperture_f_stops=inf), dict(sensor_height=-0.01), dict(sensor_height=nan),
       dict(sensor_height=inf), dict(max_radius=nan), dict(max_radius=inf), dict(max_radius=-1.0), dict(max_radius=32.5),
       dict(flags=1, focus_x=-0.01), dict(flags=1, focus_x=1.01), dict(flags=1, focus_y=nan), dict(flags=3, focus_y=1.5), dict(flags=1, focus_x=inf)]
GOOD = [dict(flags=1), dict(flags=2), dict(flags=3, focus_x=1.0, focus_y=0.0), dict(samples=0), dict(samples=4), dict(samples=5), dict(samples=64),
        dict(focal_distance=1e-3), dict(focal_distance=1e30), dict(aperture_f_stops=0.0), dict(aperture_f_stops=22.0), dict(sensor_height=0.0),
        dict(max_radius=0.0), dict(max_radius=32.0), dict(max_radius=0.25), dict(focus_x=7.0, focus_y=nan), dict(_pad=123)]   # without AUTOFOCUS the point is not looked at


def _plan_status(b, kw, status):
    assert b.dof_plan(C.byref(_d(**kw)), 64, 48, None, None, None) == status, kw


def test_argument_errors_on_a_host_only_engine():
    e, cam = _host_camera()
    b = e._b
    A.argument_errors(e, cam, "camera_set_dof", "camera_get_dof", _d, BAD, GOOD,
                      each_bad=lambda kw: _plan_status(b, kw, ST_ERR_INVALID_ARGUMENT),
                      each_good=lambda kw: _plan_status(b, kw, ST_OK))
    assert b.dof_plan(None, 64, 48, None, None, None) == ST_ERR_INVALID_ARGUMENT
    assert b.dof_plan(C.byref(_d()), 16385, 48, None, None, None) == ST_ERR_INVALID_ARGUMENT
    assert b.dof_plan(C.byref(_d()), 64, 16385, None, None, None) == ST_ERR_INVALID_ARGUMENT
    with pytest.raises(StrolleError):
        e.set_dof(cam, samples=3)
    with pytest.raises(StrolleError):
        dof_plan(_d(samples=2), 64, 48)
    e.close()


def test_process_checks_its_arguments_and_needs_a_device():
    e, cam = _host_camera()
    b, h = e._b, e._h
    d = _d()
    fake = C.c_void_p(4096)   # never dereferenced: the checks and the missing device come first
    manual, auto = display_desc(tonemap=Tonemap.ACES_FITTED, exposure_ev=1.0), display_desc(auto_exposure=True)
    bad_display = display_desc(tonemap=Tonemap.REINHARD)
    bad_display.tonemap = 9
    persp = (C.c_float * 16)(*PERSPECTIVE)

    def proj(**kw):
        p = list(PERSPECTIVE)
        for k, v in kw.items():
            p[int(k[1:])] = v
        return (C.c_float * 16)(*p)

    def dp(desc=d, display=None, projection=persp, color=fake, depth=fake, w=64, hh=48, dst=fake, fmt=0, engine=h):
        return b.dof_process(engine, C.byref(desc) if desc is not None else None, C.byref(display) if display is not None else None, projection, color, depth,
                             w, hh, dst, fmt, None)

    assert dp() == ST_ERR_NO_DEVICE and dp(display=manual) == ST_ERR_NO_DEVICE and dp(desc=_d(flags=3, focus_x=0.5, focus_y=0.5)) == ST_ERR_NO_DEVICE
    assert dp(engine=None) == ST_ERR_INVALID_ARGUMENT
    for kw in (dict(desc=None), dict(projection=None), dict(color=None), dict(depth=None), dict(dst=None), dict(w=0), dict(hh=0), dict(w=16385), dict(hh=16385),
               dict(fmt=4), dict(fmt=-1), dict(display=auto), dict(display=bad_display), dict(desc=_d(struct_size=8)), dict(desc=_d(samples=3)),
               dict(desc=_d(focal_distance=nan)), dict(projection=(C.c_float * 16)(*ORTHOGRAPHIC)), dict(projection=proj(p15=1.0)), dict(projection=proj(p5=0.0)),
               dict(projection=proj(p5=nan)), dict(projection=proj(p5=-2.0)), dict(projection=proj(p0=0.0)), dict(projection=proj(p0=inf))):
        assert dp(**kw) == ST_ERR_INVALID_ARGUMENT, kw
    assert dp(w=16384, hh=1) == ST_ERR_NO_DEVICE and dp(projection=proj(p0=-1.5, p8=0.1, p9=-0.2)) == ST_ERR_NO_DEVICE
    with pytest.raises(StrolleError):
        e.dof_process(d, PERSPECTIVE, 4096, 4096, 64, 48, 4096)
    e.close()


def test_set_get_round_trip_defaults_and_survival_on_a_host_only_engine():
    e, cam = _host_camera()
    d0, on0 = e.get_dof(cam)
    assert not on0 and d0.struct_size == C.sizeof(api.StDofDesc) and all(getattr(d0, f) == 0 for f in FIELDS[1:])
    want = dof_desc(focal_distance=2.5, aperture_f_stops=2.8, sensor_height=0.024, samples=12, max_radius=20.0, autofocus=(0.25, 0.75))
    assert want.flags == api.DOF_AUTOFOCUS
    e.set_dof(cam, want)
    got, on = e.get_dof(cam)
    assert on and [getattr(got, f) for f in FIELDS] == [getattr(want, f) for f in FIELDS]
    e.tick()
    e.update_camera(cam, scenes.cornell_camera((80, 48)))   # a resize reallocates the camera: the setting stays
    got, on = e.get_dof(cam)
    assert on and [getattr(got, f) for f in FIELDS] == [getattr(want, f) for f in FIELDS]
    e.set_dof(cam, None)
    got, on = e.get_dof(cam)
    assert not on and got.samples == 12   # the last desc stays readable
    e.set_dof(cam, focal_distance=4.0)
    got, on = e.get_dof(cam)
    assert on and (got.samples, got.aperture_f_stops, got.sensor_height, got.max_radius, got.flags) == (0, 0.0, 0.0, 0.0, 0) and got.focal_distance == 4.0
    # dof_desc()'s defaults: Bevy's focal distance; everything else 0 = the library's default
    d = dof_desc()
    assert (d.focal_distance, d.samples, d.aperture_f_stops, d.sensor_height, d.max_radius, d.flags) == (10.0, 0, 0.0, 0.0, 0.0, 0)
    assert dof_plan(d, 64, 48)[0] == R.DEFAULT_SAMPLES == 32
    e.delete_camera(cam)
    e.close()


def test_depth_of_field_and_a_window_exclude_each_other_on_a_host_only_engine():
    e, cam = _host_camera()
    d = _d()
    A.node_and_window_exclude_each_other(e, cam, "camera_set_dof", d, lambda: e.get_dof(cam)[1])
    e.close()
    # st_dist_set_partition and st_dist_set_grid: two ranks through the in-process transport
    ranks = []
    for r in range(2):
        e = Engine(device=-1)
        scenes.build_cornell(e)
        cam = e.create_camera(scenes.cornell_camera((64, 48)))
        e.dist_init_local(r, 2, 9191)
        ranks.append((e, cam))
    (e0, c0), (e1, c1) = ranks
    e0.set_dof(c0, d)
    with pytest.raises(StrolleError, match="depth of field"):
        e0.dist_set_partition(c0)
    with pytest.raises(StrolleError, match="depth of field"):
        e0.dist_set_grid(c0, dist_grid(64, 48, 2))
    e0.set_dof(c0, None)
    e0.dist_set_partition(c0)
    e1.dist_set_grid(c1, dist_grid(64, 48, 2))
    for e, cam in ranks:
        with pytest.raises(StrolleError, match="window"):
            e.set_dof(cam, d)                                                 # the tile came first
        assert not e.get_dof(cam)[1]
        e.dist_shutdown(); e.close()


def test_plan_sample_count_tile_counts_and_the_tap_table():
    for samples, (w, h), tiles in ((0, (72, 52), (3, 2)), (4, (33, 21), (2, 1)), (7, (32, 32), (1, 1)), (64, (5, 5), (1, 1)), (32, (1920, 1080), (60, 34)),
                                   (16, (16384, 16384), (512, 512))):
        n, t, T = dof_plan(_d(samples=samples), w, h)
        S = samples or 32
        assert n == S and t == tiles and T.shape == (S, 3) and T.dtype == np.float32
        want = R.taps_double(S)
        # computed in double and rounded once: within one float ulp of numpy's own double computation (the last bit of cos may differ)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert (np.abs(T.astype(np.float64) - want) <= ulp).all(), samples
        assert np.array_equal(T[:, 2], np.sqrt((np.arange(S) + 0.5) / S).astype(np.float32))   # sqrt is correctly rounded in both
        assert T[0, 1] == 0.0 and T[0, 0] == T[0, 2] and (T[:, 2] < 1).all() and (np.diff(T[:, 2]) > 0).all()
    # the raw call zeroes the table behind the last tap and accepts NULL outputs
    b = api.load_library()
    taps = (C.c_float * 192)(*([7.0] * 192))
    n, tiles = C.c_uint32(), (C.c_uint32 * 2)()
    assert b.st_dof_plan(C.byref(_d(samples=4)), 72, 52, C.byref(n), tiles, taps) == ST_OK
    assert n.value == 4 and list(tiles) == [3, 2] and not any(taps[12:]) and taps[2] != 0.0


# ---------------------------------------------------------------- dof_ref.py at cases worked out by hand
# h_s = 2^-5 and P[5] = 2 give f = 0.5 * 2^-5 * 2 = 2^-5 exactly; N = 2^-4 and H = 64 give K = 0.5 f f / (N h_s) H = 0.5 * 2^-10 / 2^-9 * 64 = 16.
# s = 2.03125 puts m = s - f = 2 and A = K / m = 8: every step below is exact in float32.
HS, STOPS, HEIGHT, S0 = 0.03125, 0.0625, 64, 2.03125
PROJ = [1.0, 0, 0, 0, 0, 2.0, 0, 0, 0, 0, 0, -1.0, 0, 0, 0.1, 0]


def _taps(samples):
    return dof_plan(_d(samples=samples), 64, 64)[2]


def test_reference_constants_coc_clamp_and_focus_by_hand():
    f, K = R.constants(PROJ, HEIGHT, STOPS, HS)
    assert f == F(0.03125) and K == F(16)
    # the defaults: f = 0.5 * 0.01866 * P[5] and N = 1, computed in double from the float fields
    fd = 0.5 * float(F(0.01866)) * 2.0
    assert R.constants(PROJ, 48) == (F(fd), F(0.5 * fd * fd / float(F(0.01866)) * 48))
    Z = np.full((HEIGHT, 8), S0, np.float32)
    Z[0, :5] = [S0, R.FLT_MAX, 2 * S0, 0.5, 0.0]
    Z[1, 0] = nan
    Z[1, 1] = -3.0
    z = R.planar(Z, PROJ, R.PLANAR_DEPTH)
    assert np.array_equal(z.view(np.uint32), Z.view(np.uint32))           # planar depth passes as it is
    s, A = R.focus(z, f, K, S0)
    assert s == F(S0) and A == F(8)
    coc = R.pack(z, s, A)
    # Z = s: A (1 - 1) = 0. FLT_MAX: s / FLT_MAX is far below half an ulp of 1, so 1 - it = 1 and coc = A. 2 s: A / 2. 0.5: 8 (1 - 4.0625) = -24.5.
    # Z = 0, Z < 0 and NaN are "not Z > 0": 0
    assert coc[0, :5].tolist() == [0.0, 8.0, 4.0, -24.5, 0.0] and coc[1, 0] == 0.0 and coc[1, 1] == 0.0
    # the clamp at R
    assert R.pack(z, s, A, 4.0)[0, :5].tolist() == [0.0, 4.0, 4.0, -4.0, 0.0]
    assert R.pack(z, s, F(80), 0.0)[0, :4].tolist() == [0.0, 32.0, 32.0, -32.0]   # the default R is 32
    # autofocus on a hit takes that pixel's Z; on sky, on Z = 0 and on NaN it falls back to focal_distance
    s2, A2 = R.focus(z, f, K, S0, R.AUTOFOCUS, 2.5 / 8, 0.0)               # floor(0.3125 * 8) = 2 -> pixel (2, 0): Z = 4.0625
    assert s2 == F(4.0625) and A2 == F(16) / F(4.03125)
    assert R.pack(z, s2, A2)[0, 2] == 0.0 and R.pack(z, s2, A2)[0, 0] == A2 * (F(1) - F(2))   # the near side is negative
    for fx, fy in ((1.5 / 8, 0.0), (4.5 / 8, 0.0), (0.0, 1.5 / HEIGHT)):
        assert R.focus(z, f, K, S0, R.AUTOFOCUS, fx, fy) == (F(S0), F(8)), (fx, fy)
    assert R.focus(z, f, K, S0, R.AUTOFOCUS, 1.0, 1.0)[0] == F(S0)         # (1, 1) is the last pixel, not one past it
    # a focus distance inside the focal length: m is held at 1e-6
    assert R.focus(z, f, K, 0.01)[1] == F(16) / F(1e-6)
    assert np.array_equal(R.frame_depth(np.array([0.0, 2.5], np.float32)), np.array([R.FLT_MAX, 2.5], np.float32))


def test_reference_planar_depth_by_hand():
    # W = H = 4, P[0] = 1, P[5] = 2, no lens shift: pixel (3, 0) has ndc = (0.75, 0.75): ax = 0.75, ay = 0.375; c = 1 / sqrt(0.5625 + 0.140625 + 1)
    D = np.full((4, 4), 2.0, np.float32)
    D[3, 3] = R.FLT_MAX
    D[2, 2] = inf
    z = R.planar(D, PROJ)
    c = F(1) / np.sqrt(F(F(0.5625) + F(0.140625)) + F(1))
    assert z[0, 3] == F(2) * c and z[0, 0] == z[0, 3] == z[3, 0]           # symmetric about the axis
    assert z[1, 1] == F(2) * (F(1) / np.sqrt(F(F(0.0625) + F(0.015625)) + F(1)))
    assert z[3, 3] == R.FLT_MAX and z[2, 2] == R.FLT_MAX                   # sky stays FLT_MAX
    # a lens shift moves the axis: with P[8] = 0.25 the pixel whose ndc_x is -0.25 looks along it
    shifted = list(PROJ); shifted[8] = 0.25; shifted[9] = -0.25
    z2 = R.planar(D, shifted)
    assert z2[2, 1] == F(2) * (F(1) / np.sqrt(F(F(0) + F(0.0625)) + F(1)))   # ndc = (-0.25, -0.25): ax = 0, ay = -0.5 / 2 = -0.25


def test_reference_tile_and_neighbour_maxima():
    w, h = 70, 40   # 3 x 2 tiles; the last column of tiles is 6 pixels wide, the last row 8 pixels high
    coc = np.full((h, w), 5.0, np.float32)        # the far field does not count, however blurred
    coc[31, 31] = -3.0                            # the corner of tile (0, 0)
    coc[2, 66] = -7.5
    coc[3, 67] = -2.0
    t = R.tile_max(coc)
    assert t.tolist() == [[3.0, 0.0, 7.5], [0.0, 0.0, 0.0]]
    n = R.neighbour_max(t)
    assert n.tolist() == [[3.0, 7.5, 7.5], [3.0, 7.5, 7.5]]
    assert R.neighbour_max(np.array([[2.0]], np.float32)).tolist() == [[2.0]]


def test_reference_one_gather_pixel_with_four_taps_by_hand():
    T = _taps(4)
    w = h = 40
    coc = np.full((h, w), 4.0, np.float32)        # a uniform far field: r_g = 4 everywhere, no near field
    z = np.full((h, w), 9.0, np.float32)
    Cc = np.zeros((h, w, 4), np.float32)
    Cc[..., 3] = 0.25
    # pixel (20, 20): tap k lands at 20.5 + 4 T[k].xy. rho = sqrt(1/8, 3/8, 5/8, 7/8) = 0.354, 0.612, 0.791, 0.935; th = 0, 137.5, 275.0, 412.5 degrees
    #   k = 0: (20.5 + 1.414, 20.5)             -> texel (21, 20)
    #   k = 1: (20.5 - 1.806, 20.5 + 1.655)     -> texel (18, 22)
    #   k = 2: (20.5 + 0.276, 20.5 - 3.150)     -> texel (20, 17)
    #   k = 3: (20.5 + 2.277, 20.5 + 2.970)     -> texel (22, 23)
    Cc[20, 20, 0], Cc[20, 21, 0], Cc[22, 18, 0], Cc[17, 20, 0], Cc[23, 22, 0] = 1.0, 2.0, 4.0, 8.0, 16.0
    d = {}
    out = R.gather(Cc, coc, z, np.zeros((2, 2), np.float32), T, d)
    assert [(int(x[20, 20]), int(y[20, 20])) for x, y, _ in d["taps"]] == [(21, 20), (18, 22), (20, 17), (22, 23)]
    # d = 4 rho: 1.41, 2.45, 3.16: (4 - d) + 0.5 >= 1, q = 1, w = 1 (3 - 2) = 1. k = 3: q = (4 - 4 T[3].z) + 0.5 = 0.758, w = q q (3 - 2 q)
    q3 = F(F(4) - T[3, 2] * F(4)) + F(0.5)
    w3 = F(F(q3 * q3) * F(F(3) - F(2) * q3))
    assert 0.75 < q3 < 0.77 and [float(wt[20, 20]) for _, _, wt in d["taps"]] == [1.0, 1.0, 1.0, float(w3)]
    wsum = F(F(4) + w3)
    assert d["wsum"][20, 20] == wsum
    assert out[20, 20, 0] == F(F(15) + F(16) * w3) / wsum and out[20, 20, 1] == 0.0 and out[20, 20, 3] == 1.0   # 1 + 2 + 4 + 8 = 15; alpha 1
    # at the corner both coordinates clamp: pixel (0, 0), tap 1 (p = (-1.31, 2.15)) reads texel (0, 2), tap 2 (p = (0.78, -2.65)) texel (0, 0)
    assert (int(d["taps"][1][0][0, 0]), int(d["taps"][1][1][0, 0])) == (0, 2) and (int(d["taps"][2][0][0, 0]), int(d["taps"][2][1][0, 0])) == (0, 0)
    # with everything in focus the colour passes with its own bits, alpha included
    Cc[0, 0] = (nan, inf, -1.0, 0.5)
    sharp = R.gather(Cc, coc * 0, z, np.zeros((2, 2), np.float32), T)
    assert np.array_equal(sharp.view(np.uint32), Cc.view(np.uint32))
    # ... and 0.49 is still "in focus" while 0.5 is not
    assert np.array_equal(R.gather(Cc, coc * 0 + F(0.49), z, np.zeros((2, 2), np.float32), T).view(np.uint32), Cc.view(np.uint32))
    assert (R.gather(Cc, coc * 0 + F(0.5), z, np.zeros((2, 2), np.float32), T)[..., 3] == 1).all()


def test_reference_background_clamp_and_near_field_by_hand():
    T = _taps(16)
    w = h = 40
    # left half: mid-ground, |coc| = 1; right half: far behind it, |coc| = 8. No near field.
    coc = np.full((h, w), 1.0, np.float32); coc[:, 20:] = 8.0
    z = np.full((h, w), 3.0, np.float32); z[:, 20:] = 30.0
    Cc = np.zeros((h, w, 4), np.float32); Cc[:, 20:, 0] = 100.0
    d = {}
    out = R.gather(Cc, coc, z, np.zeros((2, 2), np.float32), T, d)
    # a mid-ground pixel beside the edge: taps behind it count with min(8, 1) = 1, the weights of a uniform |coc| = 1 field, so its weight
    # sum is the one of a pixel deep inside the left half; without the clamp every tap on the right would weigh 1
    assert d["wsum"][20, 19] == d["wsum"][20, 5]
    hit = [(int(x[20, 19]), float(wt[20, 19])) for x, _, wt in d["taps"] if x[20, 19] >= 20]
    assert hit and all(wt < 1.0 for _, wt in hit[1:])
    # the far pixel beside the edge gathers with r_g = 8; a mid-ground tap is closer, so it keeps its own r_Y = 1 and counts only within
    # d < 1.5: tap 0 (d = 8 sqrt(1 / 32) = 1.41) may, tap 1 (d = 8 sqrt(3 / 32) = 2.45) and later ones may not
    far = [(int(x[20, 20]), float(wt[20, 20]), k) for k, (x, _, wt) in enumerate(d["taps"]) if x[20, 20] < 20]
    assert far and all(wt == 0.0 for _, wt, k in far if k >= 1)
    assert out[20, 19, 0] < 100.0 * len(hit) / 16 and abs(float(out[20, 30, 0]) - 100.0) < 1e-3   # (17 roundings of a sum and one division: a few ulp of 100)
    # a near-field pixel (coc = -6) in the corner of a tile: n = 6 in the four tiles that meet there, and in-focus pixels around it gather
    # with r_g = 6 and pick it up where 6 - d >= -0.5; far from it they weigh nothing but themselves and come back as c(X)
    w = h = 64
    coc = np.zeros((h, w), np.float32); coc[31, 31] = -6.0
    z = np.full((h, w), 5.0, np.float32); z[31, 31] = 1.0
    Cc = np.full((h, w, 4), 0.25, np.float32); Cc[31, 31, :3] = 50.0
    nb = R.neighbour_max(R.tile_max(coc))
    assert nb.tolist() == [[6.0, 6.0], [6.0, 6.0]]
    out = R.gather(Cc, coc, z, nb, T)
    changed = (out[..., 0] != F(0.25))
    ys, xs = np.nonzero(changed)
    assert changed.sum() > 1 and (np.hypot(xs - 31, ys - 31) <= 6.5 + np.sqrt(2)).all()
    assert out[0, 0].tolist() == [0.25, 0.25, 0.25, 1.0] and out[31, 31, 0] == 50.0   # (the blob itself: every tap is a sharp texel behind it, r_Y = min(0, 6) = 0, weight 0)
