"""CPU tests of the lens effects (include/strolle_hip.h "lens effects"): the entry points are exported, declared and bound by the Rust
facade, StLensDesc and StLensPlan have one layout in the header, api.py and ffi.rs, every argument error occurs on a host-only engine,
set / get / clear round-trip there (also across st_camera_update), the node and a window exclude each other through all three window
setters, st_lens_plan against numpy float64 (the tap table, the fit, the steps), the numpy restatement (lens_ref.lens_f32) at cases worked
out by hand, properties of the definition, and the restatement against the float64 definition (lens_ref.lens_f64) over the GPU test's
whole input matrix, which fixes the tolerance the GPU test uses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lens_cases as K
import lens_ref as R
import output_chain_abi as A
from output_chain_abi import ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE, ST_OK, host_camera as _host_camera
from strolle_amd import Engine, StrolleError, Tonemap, api, display_desc, lens_desc, lens_plan, scenes
from strolle_amd.api import dist_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("st_camera_set_lens", "st_camera_get_lens", "st_lens_plan", "st_lens_process")
FIELDS = ["struct_size", "flags", "k1", "k2", "scale", "fringe", "fringe_taps", "vignette_intensity", "vignette_falloff", "grain_intensity", "grain_size", "grain_seed"]
OFFSETS = [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44]
PLAN_FIELDS = ["steps", "taps", "cx", "cy", "inv_hd2", "fit", "scale_eff", "tap_scale", "tap_weight"]
PLAN_OFFSETS = [0, 4, 8, 12, 16, 20, 24, 28, 92]
CONSTANTS = [("ST_LENS_FIT", 1), ("ST_LENS_VIGNETTE_ROUND", 2), ("ST_LENS_GRAIN_ANIMATE", 4), ("ST_LENS_STEP_DISTORTION", 1), ("ST_LENS_STEP_FRINGE", 2),
             ("ST_LENS_STEP_VIGNETTE", 4), ("ST_LENS_STEP_GRAIN", 8), ("ST_LENS_MAX_TAPS", 16)]
F = np.float32
inf, nan = float("inf"), float("nan")


def test_entry_points_are_exported_declared_and_bound():
    header, ffi = A.exports_header_and_ffi_agree("StLensDesc", FIELDS, ENTRY_POINTS, CONSTANTS)
    assert (api.LENS_FIT, api.LENS_VIGNETTE_ROUND, api.LENS_GRAIN_ANIMATE) == (R.FIT, R.VIGNETTE_ROUND, R.GRAIN_ANIMATE) == (1, 2, 4)
    assert (api.LENS_STEP_DISTORTION, api.LENS_STEP_FRINGE, api.LENS_STEP_VIGNETTE, api.LENS_STEP_GRAIN) == (R.DISTORTION, R.FRINGE, R.VIGNETTE, R.GRAIN)
    assert api.LENS_MAX_TAPS == R.MAX_TAPS == 16
    assert re.findall(r"pub (\w+):", re.search(r"pub struct StLensPlan \{(.*?)\n\}", ffi, re.S).group(1)) == PLAN_FIELDS == [f for f, _ in api.StLensPlan._fields_]
    assert re.search(r"\bint st_debug_set_lens_gather\(", header) and "pub fn st_debug_set_lens_gather(" in ffi and hasattr(api.load_library(), "st_debug_set_lens_gather")
    assert '"lens effects"' in header and "lens effects" in header[header.index("ST_PASS_POST = 1u << 30"):][:900]   # the launch group's comment names the node


def test_desc_and_plan_layouts_agree_between_c_and_ctypes(tmp_path):
    got = A.c_layout(tmp_path, "StLensDesc", FIELDS, [n for n, _ in CONSTANTS])
    assert got == [48] + OFFSETS + [v for _, v in CONSTANTS]
    assert C.sizeof(api.StLensDesc) % 8 == 0
    (tmp_path / "plan").mkdir()
    assert A.c_layout(tmp_path / "plan", "StLensPlan", PLAN_FIELDS) == [284] + PLAN_OFFSETS


def _d(**kw):
    """a desc with every step active, then `kw` over it"""
    d = lens_desc(k1=-0.2, k2=0.03, scale=1.1, fit=True, fringe=0.03, fringe_taps=5, vignette_intensity=0.5, vignette_falloff=1.5, vignette_round=True, grain_intensity=0.2,
                  grain_size=2, grain_seed=77, grain_animate=True)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


BAD = [dict(struct_size=44), dict(struct_size=56), dict(struct_size=0), dict(flags=8), dict(flags=0x80000001),
       dict(k1=nan), dict(k1=inf), dict(k2=-inf), dict(k2=nan), dict(k1=0.32, k2=0.0), dict(k1=-0.32, k2=0.0), dict(k1=0.0, k2=0.2), dict(k1=0.2, k2=-0.08), dict(k1=-0.2, k2=0.08),
       dict(scale=0.24), dict(scale=4.01), dict(scale=0.0), dict(scale=-1.0), dict(scale=nan), dict(scale=inf),
       dict(fringe=-0.01), dict(fringe=0.11), dict(fringe=nan), dict(fringe=inf), dict(fringe_taps=2), dict(fringe_taps=0), dict(fringe_taps=17), dict(fringe_taps=0xffffffff),
       dict(vignette_intensity=-0.1), dict(vignette_intensity=1.01), dict(vignette_intensity=nan), dict(vignette_falloff=0.0), dict(vignette_falloff=-1.0),
       dict(vignette_falloff=nan), dict(vignette_falloff=inf),
       dict(grain_intensity=-0.1), dict(grain_intensity=1.0), dict(grain_intensity=nan), dict(grain_intensity=inf), dict(grain_size=0), dict(grain_size=9)]
GOOD = [dict(), dict(flags=0), dict(flags=7), dict(k1=0.0, k2=0.0), dict(k1=0.3, k2=0.0), dict(k1=-0.3, k2=0.0), dict(k1=0.0, k2=-0.1875), dict(k1=0.25, k2=-0.04), dict(k1=0.3125, k2=0.0),
        dict(scale=0.25), dict(scale=4.0), dict(fringe=0.1), dict(fringe_taps=3), dict(fringe_taps=16), dict(fringe=0.0, fringe_taps=0), dict(fringe=0.0, fringe_taps=99),
        dict(vignette_intensity=1.0), dict(vignette_intensity=0.0, vignette_falloff=nan), dict(vignette_intensity=0.0, vignette_falloff=-5.0), dict(vignette_falloff=1e30),
        dict(grain_intensity=0.999), dict(grain_intensity=0.0, grain_size=0), dict(grain_intensity=0.0, grain_size=1000), dict(grain_size=1), dict(grain_size=8),
        dict(grain_seed=0xffffffff)]


def test_argument_errors_on_a_host_only_engine():
    e, cam = _host_camera()

    def still_off(kw):
        assert not e.get_lens(cam)[1], kw   # a refused desc leaves the setting as it was
        plan = api.StLensPlan()
        assert e._b.lens_plan(C.byref(_d(**kw)), 64, 48, C.byref(plan)) == ST_ERR_INVALID_ARGUMENT, kw   # the plan call holds the same checks

    def plans(kw):
        assert e._b.lens_plan(C.byref(_d(**kw)), 64, 48, None) == ST_OK, kw

    A.argument_errors(e, cam, "camera_set_lens", "camera_get_lens", _d, BAD, GOOD, each_bad=still_off, each_good=plans)
    assert e._b.lens_plan(None, 64, 48, None) == ST_ERR_INVALID_ARGUMENT
    for w, h in ((0, 48), (64, 0), (16385, 48), (64, 16385)):
        assert e._b.lens_plan(C.byref(_d()), w, h, None) == ST_ERR_INVALID_ARGUMENT, (w, h)
    assert e._b.lens_plan(C.byref(_d()), 16384, 1, None) == ST_OK
    with pytest.raises(StrolleError):
        e.set_lens(cam, scale=0.0)
    with pytest.raises(StrolleError):
        lens_plan(lens_desc(k1=1.0), 64, 48)
    assert e._b.debug_set_lens_gather(e._h, 1) == ST_OK and e._b.debug_set_lens_gather(None, 1) == ST_ERR_INVALID_ARGUMENT
    e.close()


def test_process_checks_its_arguments_and_needs_a_device():
    e, cam = _host_camera()
    b, h = e._b, e._h
    d = _d(flags=R.FIT | R.VIGNETTE_ROUND)
    fake = C.c_void_p(4096)   # never dereferenced: the checks and the missing device come first
    manual, auto = display_desc(tonemap=Tonemap.ACES_FITTED, exposure_ev=1.0), display_desc(auto_exposure=True)
    bad_display = display_desc(tonemap=Tonemap.REINHARD)
    bad_display.tonemap = 9

    def lp(desc=d, display=None, src=fake, w=64, hh=48, dst=fake, fmt=0, engine=h):
        return b.lens_process(engine, C.byref(desc) if desc is not None else None, C.byref(display) if display is not None else None, src, w, hh, dst, fmt, None)

    assert lp() == ST_ERR_NO_DEVICE and lp(display=manual) == ST_ERR_NO_DEVICE and lp(desc=lens_desc()) == ST_ERR_NO_DEVICE
    assert lp(engine=None) == ST_ERR_INVALID_ARGUMENT
    for kw in (dict(desc=None), dict(src=None), dict(dst=None), dict(w=0), dict(hh=0), dict(w=16385), dict(hh=16385), dict(fmt=4), dict(fmt=-1), dict(display=auto),
               dict(display=bad_display), dict(desc=_d(struct_size=8)), dict(desc=_d(scale=nan)), dict(desc=_d(flags=16)),
               dict(desc=_d()), dict(desc=_d(flags=R.GRAIN_ANIMATE)), dict(desc=lens_desc(grain_animate=True))):   # a stateless call has no frame counter
        assert lp(**kw) == ST_ERR_INVALID_ARGUMENT, kw
    assert lp(w=16384, hh=1) == ST_ERR_NO_DEVICE
    with pytest.raises(StrolleError):
        e.lens_process(d, 4096, 64, 48, 4096)
    e.close()


def _values(d):
    return [getattr(d, f) for f in FIELDS]


def test_set_get_clear_round_trips_and_survival_on_a_host_only_engine():
    e, cam = _host_camera()
    d0, on0 = e.get_lens(cam)
    assert not on0 and d0.struct_size == C.sizeof(api.StLensDesc) and all(v == 0 for v in _values(d0)[1:])
    want = _d()
    e.set_lens(cam, want)
    got, on = e.get_lens(cam)
    assert on and _values(got) == _values(want) and got.grain_seed == 77 and got.flags == 7
    e.tick()
    e.update_camera(cam, scenes.cornell_camera((80, 48)))   # a resize reallocates the camera: the setting stays
    got, on = e.get_lens(cam)
    assert on and _values(got) == _values(want)
    e.set_exact(True); e.set_exact(False)                    # ... and across an arithmetic switch
    assert e.get_lens(cam)[1]
    e.set_lens(cam, None)
    got, on = e.get_lens(cam)
    assert not on and got.scale == F(1.1)   # the last desc stays readable
    e.set_lens(cam, vignette_intensity=0.5)
    got, on = e.get_lens(cam)
    assert on and got.vignette_intensity == 0.5 and got.scale == 1.0 and got.flags == 0 and got.k1 == 0 and got.fringe == 0 and got.grain_intensity == 0
    p = lens_plan(lens_desc(), 64, 48)                       # the defaults are neutral
    assert p.steps == 0 and p.taps == 1 and p.fit == 1 and p.scale_eff == 1
    e.delete_camera(cam)
    e.close()


def test_the_node_and_a_window_exclude_each_other_on_a_host_only_engine():
    e, cam = _host_camera()
    A.node_and_window_exclude_each_other(e, cam, "camera_set_lens", _d(), lambda: e.get_lens(cam)[1])
    e.close()
    # st_dist_set_partition and st_dist_set_grid: two ranks through the in-process transport, in either order
    ranks = []
    for r in range(2):
        e = Engine(device=-1)
        scenes.build_cornell(e)
        cam = e.create_camera(scenes.cornell_camera((64, 48)))
        e.dist_init_local(r, 2, 9393)
        ranks.append((e, cam))
    (e0, c0), (e1, c1) = ranks
    e0.set_lens(c0, _d())                                                        # the node, then the tile
    with pytest.raises(StrolleError, match="lens effects"):
        e0.dist_set_partition(c0)
    with pytest.raises(StrolleError, match="lens effects"):
        e0.dist_set_grid(c0, dist_grid(64, 48, 2))
    e0.set_lens(c0, None)
    e0.dist_set_partition(c0)
    e1.dist_set_grid(c1, dist_grid(64, 48, 2))                                   # the tile, then the node
    for e, cam in ranks:
        with pytest.raises(StrolleError, match="lens effects on a camera with a window"):
            e.set_lens(cam, _d())
        assert not e.get_lens(cam)[1]
        e.dist_shutdown(); e.close()


# ---------------------------------------------------------------- st_lens_plan against numpy float64
def _same_plan(lib, mine, what):
    for f in ("steps", "taps", "cx", "cy", "inv_hd2", "fit", "scale_eff"):
        assert getattr(lib, f) == getattr(mine, f), (what, f, getattr(lib, f), getattr(mine, f))
    assert np.array_equal(lib.tap_scale, mine.tap_scale) and np.array_equal(lib.tap_weight, mine.tap_weight), what


def test_the_plan_states_the_tap_table():
    p = R.plan_of(lens_plan(lens_desc(), 72, 52))
    assert p.steps == 0 and p.taps == 1 and p.tap_scale[0] == 1 and p.tap_weight[0].tolist() == [1, 1, 1] and not p.tap_scale[1:].any() and not p.tap_weight[1:].any()
    assert (p.cx, p.cy) == (36.0, 26.0) and p.inv_hd2 == F(1.0 / (36.0 ** 2 + 26.0 ** 2))
    for n in (3, 4, 16):
        d = lens_desc(fringe=0.05, fringe_taps=n)
        p = R.plan_of(lens_plan(d, 72, 52))
        _same_plan(p, R.plan_f64(d, 72, 52), n)
        assert p.steps == R.FRINGE and p.taps == n and not p.tap_scale[n:].any() and not p.tap_weight[n:].any()
        t = np.arange(n) / (n - 1)
        want = 1.0 + float(F(0.05)) * (2.0 * t - 1.0)
        assert np.array_equal(p.tap_scale[:n], want.astype(np.float32)) and p.tap_scale[0] == F(1.0 - float(F(0.05))) and p.tap_scale[n - 1] == F(1.0 + float(F(0.05)))
        sums = p.tap_weight[:n].astype(np.float64).sum(0)
        assert (np.abs(sums - 1.0) <= n * 2.0 ** -25).all(), (n, sums)     # each weight is rounded once: half an ulp of a value below 1 each
        assert (p.tap_weight[:n] >= 0).all() and (p.tap_weight[:n].sum(1) > 0).all()   # no tap is skipped
        assert p.tap_weight[0, 0] > 0 and p.tap_weight[0, 1] == 0 and p.tap_weight[0, 2] == 0 and p.tap_weight[n - 1].tolist()[:2] == [0, 0]
    p = R.plan_of(lens_plan(lens_desc(fringe=0.05, fringe_taps=3), 72, 52))
    assert p.tap_weight[:3].tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]           # the classic three single-channel taps
    p = R.plan_of(lens_plan(lens_desc(fringe=0.05, fringe_taps=4), 72, 52))         # t = 0, 1/3, 2/3, 1: red (1, 1/3) / (4/3), green (2/3, 2/3) / (4/3)
    assert np.array_equal(p.tap_weight[:4], np.array([[0.75, 0, 0], [0.25, 0.5, 0], [0, 0.5, 0.25], [0, 0, 0.75]], np.float64).astype(np.float32))


def _positions64(d, p, w, h):
    """every tap's source position of every pixel in float64 from the plan's (float) fit and tap scales: (taps, h, w) each"""
    cx, cy = 0.5 * w, 0.5 * h
    y, x = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    u, v = x - cx, y - cy
    r2 = (u * u + v * v) / (cx * cx + cy * cy)
    g = ((float(F(d.k2)) * r2 + float(F(d.k1))) * r2 + 1.0) * float(F(d.scale))
    s = g[None] * p.tap_scale[:p.taps].astype(np.float64)[:, None, None]
    return u[None] * s, v[None] * s, cx, cy


COEFFS = {"barrel": dict(k1=-0.2, k2=0.03), "pincushion": dict(k1=0.15, k2=0.05), "mixed": dict(k1=-0.25, k2=0.03), "mixed2": dict(k1=0.2, k2=-0.06)}


@pytest.mark.parametrize("size", [(72, 52), (5, 5), (1, 1)])
def test_the_plan_fit_keeps_every_tap_inside_and_is_the_largest_that_does(size):
    w, h = size
    for name, co in COEFFS.items():
        for fringe in (0.0, 0.08):
            for scale in (1.0, 0.7):
                d = lens_desc(fit=True, scale=scale, fringe=fringe, fringe_taps=7, **co)
                p = R.plan_of(lens_plan(d, w, h))
                _same_plan(p, R.plan_f64(d, w, h), (name, fringe, size))
                if size == (1, 1):
                    assert p.fit == 1 and p.scale_eff == F(scale)             # an axis with offset 0 constrains nothing
                    continue
                su, sv, cx, cy = _positions64(d, p, w, h)
                for k, ok in ((1.0, True), (1.001, False)):
                    fit = float(p.fit) * k
                    inside = (np.abs(su * fit) <= cx * (1 + 1e-12)).all() and (np.abs(sv * fit) <= cy * (1 + 1e-12)).all()
                    assert inside == ok, (name, fringe, scale, size, k, float(p.fit))
                assert p.scale_eff == F(float(F(scale)) * float(p.fit)) and p.steps & R.DISTORTION
    # without the flag fit is 1, and with scale 1 and no coefficients the distortion step is off
    p = R.plan_of(lens_plan(lens_desc(k1=-0.2), w, h))
    assert p.fit == 1 and p.scale_eff == 1 and p.steps == R.DISTORTION
    assert lens_plan(lens_desc(), w, h).steps == 0 and lens_plan(lens_desc(scale=2.0), w, h).steps == R.DISTORTION
    # the identity map under ST_LENS_FIT: the border pixel's centre goes to the frame's edge, W / (W - 1) on the binding axis
    if w > 1:
        p = lens_plan(lens_desc(fit=True), w, h)
        assert abs(p.fit - min(w / (w - 1), h / (h - 1))) <= 2.0 ** -23 * 2 and p.steps == R.DISTORTION


def test_the_plan_agrees_with_numpy_over_the_whole_matrix():
    for name, size, _kind, kw, _op in K.cases():
        d = K.build(kw)
        _same_plan(R.plan_of(lens_plan(d, *size)), R.plan_f64(d, *size), name)


# ---------------------------------------------------------------- lens_f32 at cases worked out by hand
def _img(w, h, fill=(1.0, 1.0, 1.0, 0.5)):
    return np.broadcast_to(np.array(fill, np.float32), (h, w, 4)).copy()


def test_restatement_the_identity_keeps_the_bits():
    img = K.image((9, 7), spoil=True)
    img[0, 0] = (nan, -0.0, inf, 0.25)
    for d in (lens_desc(), lens_desc(fringe_taps=9, vignette_falloff=3.0, grain_size=4, grain_seed=5, vignette_round=True)):
        out = R.lens_f32(img, d)
        assert np.array_equal(out.view(np.uint32), img.view(np.uint32))       # neutral: the pixels' own bits, NaN and alpha included
    # the gather at g = 1 and tap_scale 1 lands on the texel's centre: colour(texel), alpha 1
    out = R.lens_f32(img, lens_desc(), force_gather=True)
    assert np.array_equal(out[..., :3], R.colour(img)) and (out[..., 3] == 1).all() and out[0, 0].tolist() == [0.0, 0.0, 65504.0, 1.0]
    px, py = R.positions_f32(lens_desc(), R.plan_f64(lens_desc(), 9, 7), 9, 7)
    assert np.array_equal(px[0], np.broadcast_to(np.arange(9, dtype=np.float32) + F(0.5), (7, 9))) and np.array_equal(py[0][:, 0], np.arange(7, dtype=np.float32) + F(0.5))


def test_restatement_one_pixel_under_k1_by_hand():
    """8 x 4, k1 = -0.25, pixel (7, 3): cx = 4, cy = 2, u = 3.5, v = 1.5, r2 = (12.25 + 2.25) / 20 = 0.725, f = 1 - 0.25 * 0.725 = 0.81875;
    source position (3.5 f + 4, 1.5 f + 2) = (6.865625, 3.228125): q = (6.365625, 2.728125), texels x 6 and 7, rows 2 and 3, fractions
    0.365625 and 0.728125"""
    w, h = 8, 4
    d = lens_desc(k1=-0.25)
    p = R.plan_f64(d, w, h)
    assert (p.cx, p.cy, p.inv_hd2) == (4.0, 2.0, F(0.05)) and p.steps == R.DISTORTION and p.scale_eff == 1
    r2 = F(F(3.5) * F(3.5) + F(1.5) * F(1.5)) * F(0.05)
    f = F(F(F(0.0) * r2 + F(-0.25)) * r2) + F(1)
    assert abs(float(r2) - 0.725) < 1e-7 and abs(float(f) - 0.81875) < 1e-7
    px, py = R.positions_f32(d, p, w, h)
    assert px[0][3, 7] == F(F(3.5) * F(f * F(1)) + F(4)) and py[0][3, 7] == F(F(1.5) * F(f * F(1)) + F(2))
    assert abs(float(px[0][3, 7]) - 6.865625) < 1e-6 and abs(float(py[0][3, 7]) - 3.228125) < 1e-6
    fx, fy = F(px[0][3, 7] - F(0.5)) - F(6), F(py[0][3, 7] - F(0.5)) - F(2)
    for (tx, ty), wgt in (((6, 2), (1 - fx) * (1 - fy)), ((7, 2), fx * (1 - fy)), ((6, 3), (1 - fx) * fy), ((7, 3), fx * fy)):
        img = np.zeros((h, w, 4), np.float32)
        img[ty, tx, :3] = 1.0
        got = R.lens_f32(img, d)[3, 7]
        assert abs(float(got[0]) - float(wgt)) <= 2.0 ** -23 and got[3] == 1.0, (tx, ty, got, wgt)   # the four bilinear weights
    img = np.zeros((h, w, 4), np.float32); img[1, 5, :3] = 1.0
    assert R.lens_f32(img, d)[3, 7, 0] == 0.0                                                      # no other texel reaches the pixel
    # the centre of an even frame lies between four pixels: pixel (4, 2) has u = v = 0.5, r2 = 0.025
    assert abs(float(px[0][2, 4]) - (0.5 * (1 - 0.25 * 0.025) + 4)) < 1e-6


def test_restatement_the_corner_pixel_under_fit():
    """barrel + ST_LENS_FIT: the corner pixel's tap lands on or inside the frame's border, so with clamped indices it reads the corner
    texel and its neighbours only; pincushion: the binding pixel is an edge midpoint"""
    w, h = 16, 8
    for co in COEFFS.values():
        d = lens_desc(fit=True, **co)
        p = R.plan_f64(d, w, h)
        px, py = R.positions_f32(d, p, w, h)
        assert px.min() >= -1e-5 and px.max() <= w + 1e-5 and py.min() >= -1e-5 and py.max() <= h + 1e-5
        assert max(px.max() / w, py.max() / h) > 1 - 1e-6                      # ... and one tap touches it: the fit is tight
    d = lens_desc(fit=True, k1=-0.2, k2=0.03)
    img = np.zeros((h, w, 4), np.float32); img[0, 0, :3] = 7.0; img[0, 1, :3] = 7.0; img[1, 0, :3] = 7.0; img[1, 1, :3] = 7.0
    out = R.lens_f32(img, d)
    assert abs(float(out[0, 0, 0]) - 7.0) < 1e-5 and out[h - 1, w - 1, 0] == 0.0


def test_restatement_a_three_tap_fringe_splits_a_step_edge():
    """a vertical white / black step at the frame's right quarter: the red tap (scale 1 - fringe) samples nearer the centre, the blue tap
    farther out, so left of the centre line of the step red and blue land on opposite sides; green (scale 1) keeps the step"""
    w, h = 64, 9
    img = np.zeros((h, w, 4), np.float32)
    img[:, :48, :3] = 1.0                                # white for x < 48, black from 48 on
    d = lens_desc(fringe=0.1, fringe_taps=3)
    out = R.lens_f32(img, d)
    row = out[4]
    assert np.array_equal(row[:, 1], img[4, :, 1])       # green: the centre tap at scale 1 is the identity
    # pixel 46: u = 14.5; red reads x = 32 + 14.5 * 0.9 = 45.05 (white), blue x = 32 + 14.5 * 1.1 = 47.95 -> between texels 47 and 48
    assert row[46, 0] == 1.0 and 0.0 < row[46, 2] < 1.0
    # pixel 50: u = 18.5; red reads 48.65 (texels 48, 49: black), blue 52.35 (black) ; pixel 49: red 47.75 -> mostly white, blue black
    assert row[50, 0] == 0.0 and row[50, 2] == 0.0 and row[49, 0] > 0.5 and row[49, 2] == 0.0 and row[49, 1] == 0.0
    red_edge, blue_edge = np.argmax(row[:, 0] < 0.5), np.argmax(row[:, 2] < 0.5)
    assert blue_edge < 48 < red_edge                     # the red and the blue edge land on opposite sides of the green one
    assert (out[..., 3] == 1).all()


def test_restatement_a_constant_image_stays_constant_under_fringe():
    for n in (3, 4, 16):
        for value in (1.0, 0.3, 1000.0):
            img = _img(40, 11, (value, value, value, 0.2))
            out = R.lens_f32(img, lens_desc(fringe=0.07, fringe_taps=n))
            # the weights sum to 1 within n half-ulps, each product and each of the n - 1 sums rounds once
            assert np.abs(out[..., :3].astype(np.float64) / float(F(value)) - 1.0).max() <= 2 * n * 2.0 ** -24, (n, value)
        out = R.lens_f32(_img(40, 11), lens_desc(fringe=0.07, fringe_taps=3))
        assert (out[..., :3] == 1).all()                 # three single-channel taps of weight 1: exactly


def test_restatement_the_vignette_by_hand():
    w, h = 9, 5                                          # odd: pixel (4, 2) is the centre, u = v = 0
    for rnd in (False, True):
        d = lens_desc(vignette_intensity=0.5, vignette_falloff=1.0, vignette_round=rnd)
        out = R.lens_f32(_img(w, h, (2.0, 4.0, 8.0, 0.3)), d)
        assert out[2, 4].tolist() == [2.0, 4.0, 8.0, 1.0]                    # the centre: m = 0, q = 1, factor (1 - a) + a = 1 exactly
        # the corner pixel (8, 4): u = 4, v = 2; round: r2 = 20 / 26.5; ellipse: ((4 / 4.5)^2 + (2 / 2.5)^2) / 2
        m = 20.0 / 26.5 if rnd else ((4 / 4.5) ** 2 + (2 / 2.5) ** 2) / 2
        want = 0.5 + 0.5 / (1 + m) ** 2
        assert abs(float(out[4, 8, 0]) / 2.0 - want) < 1e-6 and out[4, 8, 0] == out[0, 0, 0] == out[0, 8, 0] == out[4, 0, 0]
        # the edge midpoint (8, 2): u = 4, v = 0; round: 16 / 26.5; ellipse: (4 / 4.5)^2 / 2
        m = 16.0 / 26.5 if rnd else (4 / 4.5) ** 2 / 2
        assert abs(float(out[2, 8, 1]) / 4.0 - (0.5 + 0.5 / (1 + m) ** 2)) < 1e-6
    # at the frame's very corner both shapes have m = 1; with falloff 1 and intensity 1 that is 1 / 4: the outermost pixel is a little brighter
    out = R.lens_f32(_img(1001, 601), lens_desc(vignette_intensity=1.0, vignette_falloff=1.0))
    assert 0.25 < out[0, 0, 0] < 0.2515
    assert R.lens_f32(_img(3, 3), lens_desc(vignette_intensity=1.0, vignette_falloff=1e30))[0, 0, 0] == 0.0   # q overflows to inf: fall 0, no NaN


def test_restatement_grain_eta_by_hand_and_cells():
    def pcg(v):
        v = (v * 747796405 + 2891336453) & 0xffffffff
        w = (((v >> ((v >> 28) + 4)) ^ v) * 277803737) & 0xffffffff
        return (w >> 22) ^ w

    for (x, y), size, seed in (((0, 0), 1, 0), ((5, 3), 1, 12345), ((16383, 16383), 3, 0xffffffff), ((7, 2), 8, 99)):
        hsh = pcg((x // size + pcg((y // size + seed) & 0xffffffff)) & 0xffffffff)
        want = ((hsh & 0xffff) + (hsh >> 16) - 65535) / 65536
        got = R.grain_eta(np.array([x]), np.array([y]), size, seed)[0]
        assert float(got) == want and -1 < want < 1, (x, y, size, seed)          # exact: every step is an integer below 2^24 or a power of two
    assert pcg(0) == (lambda w: (w >> 22) ^ w)((((2891336453 >> ((2891336453 >> 28) + 4)) ^ 2891336453) * 277803737) & 0xffffffff)
    d = lens_desc(grain_intensity=0.5, grain_size=2, grain_seed=3)
    out = R.lens_f32(_img(8, 6), d)
    cells = out[..., 0].reshape(3, 2, 4, 2)
    assert (cells == cells[:, :1, :, :1]).all() and len(np.unique(out[..., 0])) > 6   # one value per 2 x 2 cell, and the cells differ
    assert (out[..., 0] == out[..., 1]).all() and (out[..., 3] == 1).all() and (out[..., :3] > 0.5).all() and (out[..., :3] < 1.5).all()
    eta = R.grain_eta(np.array([2]), np.array([4]), 2, 3)[0]
    assert out[4, 2, 0] == F(1) * (F(1) + F(0.5) * eta)
    # ST_LENS_GRAIN_ANIMATE: the frame counter is added to the seed, modulo 2^32; without the flag the frame does not matter
    da = lens_desc(grain_intensity=0.5, grain_size=2, grain_seed=0xffffffff, grain_animate=True)
    assert R.seed_of(da, 3) == 2 and R.seed_of(d, 3) == 3
    assert not np.array_equal(R.lens_f32(_img(8, 6), da, frame=1), R.lens_f32(_img(8, 6), da, frame=2))
    assert np.array_equal(R.lens_f32(_img(8, 6), d, frame=1), R.lens_f32(_img(8, 6), d, frame=2))


def test_restatement_a_nan_and_a_negative_texel_next_to_a_tap():
    w, h = 8, 4
    img = _img(w, h, (2.0, 2.0, 2.0, 1.0))
    img[2, 6] = (nan, -5.0, inf, nan); img[3, 7] = (-inf, 1e30, -0.0, 0.0)
    d = lens_desc(k1=-0.25)                               # pixel (7, 3) reads texels (6..7, 2..3): see the case by hand above
    out = R.lens_f32(img, d)
    assert np.isfinite(out).all() and (out[..., 3] == 1).all()
    clean = img.copy(); clean[2, 6] = (0.0, 0.0, 65504.0, 1.0); clean[3, 7] = (0.0, 65504.0, 0.0, 1.0)
    assert np.array_equal(out, R.lens_f32(clean, d))      # every texel goes through colour() before it is weighed
    assert out[3, 7, 0] < 2.0 and out[3, 7, 1] > 2.0 and out[3, 7, 2] > 2.0
    # a pointwise step starts from colour(texel) too; the result is held at 65504
    out = R.lens_f32(img, lens_desc(grain_intensity=0.9, grain_seed=1))
    assert np.isfinite(out).all() and out[2, 6, 0] == 0.0 and out[2, 6, 1] == 0.0 and out[..., :3].max() <= 65504.0


# ---------------------------------------------------------------- properties of the definition
def test_definition_distortion_with_fit_samples_inside_the_frame():
    """a frame that is 1 inside and would read 1000 outside (no clamping: positions checked directly) — every f64 tap position of every
    matrix case with ST_LENS_FIT lies in [0, W] x [0, H]"""
    n = 0
    for name, size, _kind, kw, _op in K.cases():
        if not kw.get("fit"):
            continue
        d = K.build(kw)
        w, h = size
        su, sv, cx, cy = _positions64(d, R.plan_of(lens_plan(d, w, h)), w, h)
        fit = float(lens_plan(d, w, h).fit)
        assert (np.abs(su * fit) <= cx * (1 + 1e-12)).all() and (np.abs(sv * fit) <= cy * (1 + 1e-12)).all(), name
        n += 1
    assert n >= 15


def test_definition_a_radial_image_stays_radial_under_distortion():
    w = h = 41
    y, x = np.meshgrid(np.arange(h) + 0.5 - h / 2, np.arange(w) + 0.5 - w / 2, indexing="ij")
    rad = np.hypot(x, y)
    img = np.concatenate([np.repeat((1.0 + np.cos(rad * 0.2))[..., None], 3, -1), np.ones((h, w, 1))], -1).astype(np.float32)   # smooth in r
    for co in COEFFS.values():
        out = R.lens_f64(img, lens_desc(scale=0.8, **co))[..., 0]
        assert np.abs(out - out[::-1, :]).max() < 1e-12 and np.abs(out - out[:, ::-1]).max() < 1e-12 and np.abs(out - out.T).max() < 1e-12   # the square's symmetries, exactly
        # and the value is a function of the radius: against the profile sampled at the mapped radius, within bilinear interpolation's error
        r2 = (x * x + y * y) / (2 * (w / 2) ** 2)
        g = ((co["k2"] * r2 + co["k1"]) * r2 + 1.0) * 0.8
        want = 1.0 + np.cos(rad * g * 0.2)
        inner = rad < 18
        assert np.abs(out - want)[inner].max() < 0.01, co


def test_definition_the_vignette_is_monotone_in_r():
    w, h = 64, 48
    y, x = np.meshgrid(np.arange(h) + 0.5 - h / 2, np.arange(w) + 0.5 - w / 2, indexing="ij")
    for rnd in (False, True):
        out = R.lens_f64(_img(w, h), lens_desc(vignette_intensity=0.8, vignette_falloff=2.0, vignette_round=rnd))[..., 0]
        m = (x * x + y * y) if rnd else (x / (w / 2)) ** 2 + (y / (h / 2)) ** 2
        order = np.argsort(m.ravel(), kind="stable")
        assert (np.diff(out.ravel()[order]) <= 1e-15).all() and out.max() < 1.0 and out.min() > 0.2
        f32 = R.lens_f32(_img(w, h), lens_desc(vignette_intensity=0.8, vignette_falloff=2.0, vignette_round=rnd))[..., 0]
        # ... and so is the restatement, up to its own rounding: m, q, q q, the quotient, a fall and the sum round once each, eight half-ulps of a value below 1
        assert (np.diff(f32.ravel()[order]) <= 2.0 ** -21).all()


def test_definition_grain_has_the_triangular_moments():
    w, h = 72, 52
    n = w * h
    for seed in (0, 1, 12345):
        out = R.lens_f64(_img(w, h), lens_desc(grain_intensity=0.5, grain_size=1, grain_seed=seed))[..., 0]
        eta = (out - 1.0) / 0.5
        sigma = (1.0 / 6.0) ** 0.5                        # the sum of two uniforms over (-1, 1) / 2 each: variance 2 (1 / 12)
        assert abs(eta.mean()) <= 3 * sigma / n ** 0.5, (seed, eta.mean())
        # the variance's own standard error: sqrt((mu4 - sigma^4) / n) with mu4 = 1 / 15 for the triangular law
        assert abs(eta.var() - 1.0 / 6.0) <= 3 * ((1.0 / 15.0 - 1.0 / 36.0) / n) ** 0.5, (seed, eta.var())
        assert eta.min() > -1 and eta.max() < 1


# ---------------------------------------------------------------- the restatement against the definition
def restatement_vs_definition():
    """(a, b, the case of a, the case of b, pixels): over the whole input matrix on unspoiled inputs, every pixel and channel counted, in
    front of the display transform (the operator is display_ref's; the spread has no meaning behind it). rel = |lens_f32 - lens_f64| /
    max(1, |lens_f64|), spread = lens_ref's tap spread / max(1, |lens_f64|); a = max rel where spread == 0, b = max (rel - a) / spread
    elsewhere. tools/lens_bench.py --restatement writes them to profiles/lens.json"""
    rows, a, where_a, pixels = [], 0.0, None, 0
    for name, size, kind, kw, _op in K.cases():
        d = K.build(kw)
        img = K.image(size, False, kind)
        got = R.lens_f32(img, d, R.plan_of(lens_plan(d, *size)))
        assert np.isfinite(got).all(), f"{name}: a non-finite value from finite inputs"
        want, spread = R.lens_f64(img, d, spread=True)
        den = np.maximum(1.0, np.abs(want))
        rel, spread = np.abs(got[..., :3].astype(np.float64) - want) / den, spread / den
        pixels += rel.shape[0] * rel.shape[1]
        rows.append((name, rel, spread))
        flat = rel[spread == 0]
        if flat.size and flat.max() > a:
            a, where_a = float(flat.max()), name
    b, where_b = 0.0, None
    for name, rel, spread in rows:
        m = spread > 0
        if m.any():
            worst = float((np.maximum(rel[m] - a, 0.0) / spread[m]).max())
            if worst > b:
                b, where_b = worst, name
    return a, b, where_a, where_b, pixels


def test_restatement_agrees_with_the_float64_definition():
    """The bound is four times the two constants recorded in profiles/lens.json (restatement_vs_definition), the project's usual margin;
    the GPU test holds both builds to the definition within the same bound."""
    a, b, where_a, where_b, pixels = restatement_vs_definition()
    ta, tb = K.tolerance()
    print(f"restatement against the definition: a {a:.3e} at {where_a}, b {b:.3e} at {where_b} over {pixels} pixels; bound {ta:.3e} + {tb:.3e} spread")
    assert pixels > 50000 and 0 < ta < 1e-5 and 0 < tb < 1e-3
    assert a <= ta and b <= tb, (a, where_a, b, where_b)
