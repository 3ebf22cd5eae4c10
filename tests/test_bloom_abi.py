"""CPU tests of bloom (include/strolle_hip.h "bloom"): the entry points are exported, declared and bound by the Rust facade, StBloomDesc has
one layout in the header, api.py and ffi.rs, every argument error occurs on a host-only engine, set / get round-trip there (also across
st_camera_update), a window and bloom exclude each other in both orders, st_bloom_plan's sizes and factors, st_bloom_process says that it
needs a device, and the numpy restatement (bloom_ref.py) at hand-computed cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bloom_ref as R
import output_chain_abi as A
from parity import bits_equal_mask
from strolle_amd import Engine, StrolleError, Tonemap, bloom_desc, display_desc, scenes
from output_chain_abi import ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE, ST_OK, host_camera as _host_camera
from strolle_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("st_camera_set_bloom", "st_camera_get_bloom", "st_bloom_plan", "st_bloom_process", "st_debug_set_bloom_tail")
FIELDS = ["struct_size", "flags", "levels", "intensity", "low_frequency_boost", "low_frequency_boost_curvature", "high_pass_frequency",
          "threshold", "threshold_softness", "clamp"]
F = np.float32


def test_entry_points_are_exported_declared_and_bound():
    header, _ = A.exports_header_and_ffi_agree("StBloomDesc", FIELDS, ENTRY_POINTS, [("ST_BLOOM_ADDITIVE", 1), ("ST_BLOOM_FIREFLY_SUPPRESS", 2)])
    assert re.search(r"ST_BLOOM_ADDITIVE = 1, ST_BLOOM_FIREFLY_SUPPRESS = 2\b", header)
    assert (api.BLOOM_ADDITIVE, api.BLOOM_FIREFLY_SUPPRESS) == (R.ADDITIVE, R.FIREFLY_SUPPRESS) == (1, 2)


def test_desc_layout_agrees_between_c_and_ctypes(tmp_path):
    got = A.c_layout(tmp_path, "StBloomDesc", FIELDS, ["ST_BLOOM_ADDITIVE", "ST_BLOOM_FIREFLY_SUPPRESS"])
    assert got == [40] + [4 * k for k in range(len(FIELDS))] + [1, 2]


def _d(**kw):
    d = bloom_desc(intensity=0.3, levels=5, threshold=0.8, threshold_softness=0.5, clamp=100.0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


inf, nan = float("inf"), float("nan")
BAD = [dict(struct_size=36), dict(struct_size=44), dict(struct_size=0), dict(flags=4), dict(flags=0x80000001), dict(levels=9), dict(levels=0xffffffff),
       dict(intensity=nan), dict(intensity=inf), dict(intensity=-0.01), dict(intensity=1.01), dict(flags=2, intensity=1.5),
       dict(low_frequency_boost=nan), dict(low_frequency_boost=-0.1), dict(low_frequency_boost=1.1),
       dict(low_frequency_boost_curvature=nan), dict(low_frequency_boost_curvature=-0.1), dict(low_frequency_boost_curvature=1.0),
       dict(high_pass_frequency=nan), dict(high_pass_frequency=0.0), dict(high_pass_frequency=-0.5), dict(high_pass_frequency=1.01),
       dict(threshold=nan), dict(threshold=inf), dict(threshold=-1.0), dict(threshold_softness=nan), dict(threshold_softness=-0.1),
       dict(threshold_softness=1.1), dict(clamp=nan), dict(clamp=inf), dict(clamp=-1.0)]
GOOD = [dict(levels=0), dict(levels=1), dict(levels=8), dict(intensity=0.0), dict(intensity=1.0), dict(flags=1, intensity=7.5), dict(flags=3),
        dict(low_frequency_boost=0.0), dict(low_frequency_boost=1.0), dict(low_frequency_boost_curvature=0.0), dict(high_pass_frequency=1.0),
        dict(threshold=0.0), dict(threshold_softness=0.0), dict(threshold_softness=1.0), dict(clamp=0.0)]


def _plan_status(b, kw, status):
    assert b.bloom_plan(C.byref(_d(**kw)), 64, 48, None, None, None) == status, kw


def test_argument_errors_on_a_host_only_engine():
    e, cam = _host_camera()
    b = e._b
    A.argument_errors(e, cam, "camera_set_bloom", "camera_get_bloom", _d, BAD, GOOD,
                      each_bad=lambda kw: _plan_status(b, kw, ST_ERR_INVALID_ARGUMENT),
                      each_good=lambda kw: _plan_status(b, kw, ST_OK))
    assert b.bloom_plan(None, 64, 48, None, None, None) == ST_ERR_INVALID_ARGUMENT
    with pytest.raises(StrolleError):
        e.set_bloom(cam, levels=12)
    e.close()


def test_bloom_process_checks_its_arguments_and_needs_a_device():
    e, cam = _host_camera()
    b, h = e._b, e._h
    d = _d()
    fake = C.c_void_p(4096)   # never dereferenced: the checks and the missing device come first
    manual, auto = display_desc(tonemap=Tonemap.ACES_FITTED, exposure_ev=1.0), display_desc(auto_exposure=True)
    bad_display = display_desc(tonemap=Tonemap.REINHARD)
    bad_display.tonemap = 9

    def bp(desc=d, display=None, src=fake, w=64, hh=48, dst=fake, fmt=0, engine=h):
        return b.bloom_process(engine, C.byref(desc) if desc is not None else None, C.byref(display) if display is not None else None, src, w, hh, dst, fmt, None)

    assert bp() == ST_ERR_NO_DEVICE and bp(display=manual) == ST_ERR_NO_DEVICE
    assert bp(engine=None) == ST_ERR_INVALID_ARGUMENT
    for kw in (dict(desc=None), dict(src=None), dict(dst=None), dict(w=0), dict(hh=0), dict(w=16385), dict(fmt=4), dict(fmt=-1),
               dict(display=auto), dict(display=bad_display), dict(desc=_d(struct_size=8)), dict(desc=_d(levels=9)), dict(desc=_d(clamp=nan))):
        assert bp(**kw) == ST_ERR_INVALID_ARGUMENT, kw
    with pytest.raises(StrolleError):
        e.bloom_process(d, 4096, 64, 48, 4096)
    e.close()


def test_set_get_round_trip_and_survival_on_a_host_only_engine():
    e, cam = _host_camera()
    d0, on0 = e.bloom(cam)
    assert not on0 and d0.struct_size == C.sizeof(api.StBloomDesc) and all(getattr(d0, f) == 0 for f in FIELDS[1:])
    want = bloom_desc(intensity=0.25, additive=True, firefly_suppress=True, levels=7, low_frequency_boost=0.5, low_frequency_boost_curvature=0.75,
                      high_pass_frequency=0.5, threshold=1.5, threshold_softness=0.25, clamp=512.0)
    e.set_bloom(cam, want)
    got, on = e.bloom(cam)
    assert on and [getattr(got, f) for f in FIELDS] == [getattr(want, f) for f in FIELDS]
    e.tick()
    e.update_camera(cam, scenes.cornell_camera((80, 48)))   # a resize reallocates the camera: the setting stays
    got, on = e.bloom(cam)
    assert on and [getattr(got, f) for f in FIELDS] == [getattr(want, f) for f in FIELDS]
    e.set_bloom(cam, None)
    got, on = e.bloom(cam)
    assert not on and got.levels == 7   # the last desc stays readable
    e.set_bloom(cam, intensity=0.1)
    assert e.bloom(cam)[1] and e.bloom(cam)[0].levels == 0
    e.delete_camera(cam)
    e.close()


def test_bloom_and_a_window_exclude_each_other_on_a_host_only_engine():
    e, cam = _host_camera()
    d = _d()
    A.node_and_window_exclude_each_other(e, cam, "camera_set_bloom", d, lambda: e.bloom(cam)[1])
    e.close()


def test_plan_sizes_for_even_odd_and_tiny_frames():
    e = Engine(device=-1)
    cases = {(1920, 1080, 6): [(960, 540), (480, 270), (240, 135), (120, 68), (60, 34), (30, 17)],
             (1920, 1080, 0): [(960, 540), (480, 270), (240, 135), (120, 68), (60, 34), (30, 17)],
             (71, 53, 8): [(36, 27), (18, 14), (9, 7), (5, 4), (3, 2), (2, 1)][:5],
             (64, 48, 8): [(32, 24), (16, 12), (8, 6), (4, 3), (2, 2)],
             (64, 48, 2): [(32, 24), (16, 12)],
             (3, 3, 6): [(2, 2)], (4, 3, 1): [(2, 2)], (2, 2, 6): [], (1, 1, 6): [], (2, 100, 3): [], (5, 1, 3): [], (16384, 3, 8): [(8192, 2)]}
    for (w, h, levels), want in cases.items():
        n, sizes, fac = e.bloom_plan(bloom_desc(levels=levels), w, h)
        assert (n, sizes) == (len(want), want) and len(fac) == n, (w, h, levels, sizes)
        assert R.plan_sizes(w, h, levels) == want
    # entries past the level count are zero
    n, sizes, fac = C.c_uint32(), (C.c_uint32 * 16)(), (C.c_float * 8)()
    for k in range(16):
        sizes[k] = 77
    d = bloom_desc(levels=8)
    assert e._b.bloom_plan(C.byref(d), 9, 9, C.byref(n), sizes, fac) == ST_OK
    assert n.value == 3 and list(sizes) == [5, 5, 3, 3, 2, 2] + [0] * 10 and list(fac)[3:] == [0.0] * 5   # 9 -> 5 -> 3 -> 2 (-> 1: too small)
    assert e._b.bloom_plan(C.byref(d), 16385, 9, None, None, None) == ST_ERR_INVALID_ARGUMENT
    e.close()


def test_plan_factors_against_numpy_within_one_ulp():
    e = Engine(device=-1)
    rng = np.random.default_rng(3)
    descs = [bloom_desc(), bloom_desc(intensity=0.3, additive=True, low_frequency_boost=0.2, low_frequency_boost_curvature=0.0, high_pass_frequency=0.4),
             bloom_desc(intensity=1.0), bloom_desc(intensity=0.0, low_frequency_boost=0.0), bloom_desc(intensity=5.0, additive=True, high_pass_frequency=1 / 3)]
    for _ in range(20):
        descs.append(bloom_desc(intensity=rng.random(), additive=bool(rng.integers(2)), low_frequency_boost=rng.random(),
                                low_frequency_boost_curvature=rng.random() * 0.99, high_pass_frequency=1.0 - rng.random() * 0.95))
    for d in descs:
        for levels, size in ((1, (64, 48)), (2, (64, 48)), (6, (1920, 1080)), (8, (1920, 1080)), (8, (40, 40))):
            d.levels = levels
            n, _, got = e.bloom_plan(d, *size)
            want = R.factors(n, d.intensity, d.low_frequency_boost, d.low_frequency_boost_curvature, d.high_pass_frequency, bool(d.flags & 1))
            ulp = np.spacing(np.abs(want).astype(np.float32))
            assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all(), (levels, size, got, want)
    # Bevy's natural preset at six levels: the first level blends by the intensity alone, the last adds the whole boost
    n, _, got = e.bloom_plan(bloom_desc(intensity=0.15, levels=6), 1920, 1080)
    assert got[0] == F(0.15) and abs(float(got[5]) - (0.15 + 0.7 * 0.85)) < 1e-6
    e.close()


# ---------------------------------------------------------------- bloom_ref.py at hand-computed cases
def test_reference_group_weights_sum_to_one_and_a_constant_stays_constant():
    assert sum(R.GROUP_WEIGHTS) == 1.0 and sum(sum(r) for r in R.TENT) == 1.0
    img = np.full((37, 50, 3), (0.5, 2.0, 8.0), np.float32)   # powers of two: every sum in the chain is exact
    for firefly in (False, True):
        down = R.downsample(img, firefly)
        assert down.shape == (19, 25, 3)
        # (firefly: five weights, their products, two sums of five and a division: a dozen roundings of half an ulp each at most)
        assert np.allclose(down, img[:19, :25], rtol=12 * 2.0 ** -24, atol=0) if firefly else np.array_equal(down, img[:19, :25])
    assert np.array_equal(R.upsample(img[:19, :25], 50, 37), img)
    fac = R.factors(4, 0.3, 0.7, 0.95, 1.0, False)
    out = R.bloom(img, fac)
    # a blend c (1 - b) + u b rounds four times (1 - b, two products, the sum); an upsample of a constant that is no power of two rounds at
    # each of its 9 + 8 + 12 operations: at most (4 + 29) / 2 ulp per level, and L levels feed the result
    assert np.allclose(out, img, rtol=4 * 17 * 2.0 ** -23, atol=0), "the energy-conserving chain keeps a constant image to float rounding"
    grey = np.full((20, 20, 3), 0.3, np.float32)
    assert np.allclose(R.bloom(grey, R.factors(3, 0.2, 0.5, 0.5, 1.0, False)), grey, rtol=3 * 17 * 2.0 ** -23, atol=0)


def test_reference_single_bright_texel_taps_by_hand_and_symmetry_to_rounding():
    img = np.zeros((33, 33, 3), np.float32)
    img[16, 16] = 64.0
    # mirror symmetry about the centre texel holds for the downsample taps only where the grid is symmetric: a 2 x 2 block in an even image
    img2 = np.zeros((32, 32, 3), np.float32)
    img2[15:17, 15:17] = 64.0
    out = R.bloom(img2, R.factors(3, 0.5, 0.7, 0.5, 1.0, True), flags=R.ADDITIVE)
    glow = out - img2
    # (to float rounding: the sums run left to right and x is blended before y, so a mirrored tap order rounds differently)
    for other in (glow[::-1], glow[:, ::-1], glow.transpose(1, 0, 2)):
        assert np.allclose(glow, other, rtol=1e-5, atol=1e-7)
    assert glow[15, 15, 0] > glow[12, 12, 0] > glow[8, 8, 0] > 0.0 and np.isfinite(out).all()
    # one level, the 13 taps by hand: the texel (16, 16) of a 33 x 33 image lies in e = S(0, 0) and j = S(-1, -1) of destination (8, 8):
    # e = j = 64 / 4 = 16 -> G0..G3 = 16 / 4 = 4 each (e is in all four) and G4 = 4 -> 4 * 4 * 0.125 + 4 * 0.5 = 4
    down = R.downsample(img)
    assert down[8, 8, 0] == 4.0
    # destination (7, 7) sees it in S(2, 2) = i (G3 only: 4 * 0.125 = 0.5) and in m = S(1, 1) (16 / 4 = 4 -> * 0.5 = 2)
    assert down[7, 7, 0] == 2.5 and down[9, 9, 0] == 0.5 + 0.0
    # the single texel on the diagonal of a square image: its whole response is symmetric under x <-> y, to rounding (x is blended before y).
    # (On an odd-sized image the 2 : 1 grid itself is not mirror-symmetric about the texel, hence the even image and the 2 x 2 block above.)
    one = R.bloom(img, R.factors(3, 0.5, 0.7, 0.5, 1.0, True), flags=R.ADDITIVE) - img
    assert np.allclose(one, one.transpose(1, 0, 2), rtol=1e-5, atol=1e-7) and one[16, 16, 0] > one[12, 12, 0] > one[6, 6, 0] > 0.0


def test_reference_additive_with_zero_intensity_returns_the_input_bit_for_bit():
    rng = np.random.default_rng(2)
    img = np.exp(rng.standard_normal((19, 23, 3)) * 3).astype(np.float32)
    img[3, 4, 0], img[5, 5, 1], img[0, 0, 2] = np.inf, np.nan, -7.0
    fac = R.factors(4, 0.0, 0.0, 0.5, 1.0, True)
    assert not fac.any()
    out = R.bloom(img, fac, flags=R.ADDITIVE)
    assert bits_equal_mask(out, img).all()


def test_reference_prefilter_knee():
    t, soft = 2.0, 0.5   # knee = 1: the soft curve runs over m in [1, 3]
    def w(m):
        c = R.prefilter(np.array([[[m, m * 0.5, 0.0]]], np.float32), 0.0, t, soft)
        return float(c[0, 0, 0]) / m
    # m = threshold - knee: s = 0, max(m - t, 0) = max(-1, 0) = 0
    assert w(1.0) == 0.0
    # m = threshold: s = min(1, 2)^2 / (4 + 1e-4) = 0.249994; max(0, s) / 2
    assert abs(w(2.0) - (1.0 / 4.0001) / 2.0) < 1e-7
    # m = threshold + knee: s = 2^2 / 4.0001 = 0.99998 < m - t = 1: the hard branch, (3 - 2) / 3
    assert abs(w(3.0) - 1.0 / 3.0) < 1e-7
    assert w(0.5) == 0.0 and abs(w(10.0) - 0.8) < 1e-7
    # no threshold: only the clamp
    c = R.prefilter(np.array([[[-1.0, np.nan, 1e9], [np.inf, 0.25, -np.inf]]], np.float32), 100.0)
    assert np.array_equal(c, np.array([[[0, 0, 100], [100, 0.25, 0]]], np.float32))
    assert np.array_equal(R.prefilter(np.array([[[np.inf, 1e9, 3.0]]], np.float32)), np.array([[[65504, 65504, 3]]], np.float32))


def test_reference_nan_and_inf_texels_leave_every_other_pixel_finite():
    rng = np.random.default_rng(4)
    img = rng.random((40, 52, 3)).astype(np.float32)
    bad = [(3, 4, np.nan), (20, 30, np.inf), (39, 51, -np.inf), (0, 0, np.nan), (17, 2, np.inf)]
    for y, x, v in bad:
        img[y, x, 1] = v
    for flags in (0, R.ADDITIVE, R.FIREFLY_SUPPRESS, R.ADDITIVE | R.FIREFLY_SUPPRESS):
        for thr in (0.0, 0.5):
            d = {}
            out = R.bloom(img, R.factors(4, 0.3, 0.7, 0.9, 1.0, bool(flags & 1)), flags=flags, threshold=thr, softness=0.5, details=d)
            assert all(np.isfinite(m).all() for m in d["down"] + d["up"]), "the pyramid is finite"
            mask = np.ones(img.shape, bool)
            for y, x, _ in bad:
                mask[y, x, 1] = False
            assert np.isfinite(out[mask]).all()
            assert np.isnan(out[3, 4, 1]) and out[20, 30, 1] == np.inf and out[39, 51, 1] == -np.inf
