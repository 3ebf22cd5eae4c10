"""CPU tests of output post-processing (include/strolle_hip.h "post-processing"): the entry points are exported, declared and bound by the
Rust facade, StPostDesc has one layout in the header, api.py and ffi.rs, every argument error occurs on a host-only engine, set / get /
output-size round-trip there (also across st_camera_update), a window and post-processing exclude each other in both orders, st_post_process
says that it needs a device, and the numpy restatement (post_ref.py) gives hand-computed values and makes a slanted edge more accurate."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import output_chain_abi as A
import post_ref as R
from parity import bits_equal_mask
from strolle_amd import PassBit, ResampleFilter, StrolleError, post_desc, scenes
from output_chain_abi import ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE, ST_ERR_UNKNOWN_CAMERA, ST_OK, host_camera as _host_camera
from strolle_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("st_camera_set_post", "st_camera_get_post", "st_camera_output_size", "st_post_process")
FIELDS = ["struct_size", "flags", "output_width", "output_height", "filter", "fxaa_edge_threshold", "fxaa_edge_threshold_min", "fxaa_subpixel"]
F = np.float32


def test_entry_points_are_exported_declared_and_bound():
    header, ffi = A.exports_header_and_ffi_agree("StPostDesc", FIELDS, ENTRY_POINTS, [("ST_RESAMPLE_%s" % t.name, t.value) for t in ResampleFilter])
    assert "pub const ST_POST_FXAA: u32 = 1;" in ffi and "pub const ST_PASS_POST: u64 = 1 << 30;" in ffi
    assert re.search(r"ST_PASS_POST = 1u << 30\b", header) and PassBit.POST == 1 << 30


def test_desc_layout_agrees_between_c_and_ctypes(tmp_path):
    got = A.c_layout(tmp_path, "StPostDesc", FIELDS, ["ST_POST_FXAA", "ST_RESAMPLE_BILINEAR", "ST_RESAMPLE_CATMULL_ROM", "(int)ST_PASS_POST"])
    assert got == [32] + [4 * k for k in range(len(FIELDS))] + [1, 1, 2, 1 << 30]
    assert got[-4:-1] == [api.POST_FXAA, ResampleFilter.BILINEAR, ResampleFilter.CATMULL_ROM]


def _d(**kw):
    d = post_desc(fxaa=True, output_size=(128, 96), filter=ResampleFilter.CATMULL_ROM)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_errors_on_a_host_only_engine():
    e, cam = _host_camera()
    b, h = e._b, e._h

    def st(d, camera=cam, engine=h):
        return b.camera_set_post(engine, camera, C.byref(d) if d is not None else None)

    assert st(_d()) == ST_OK and st(None) == ST_OK
    assert st(_d(), engine=None) == ST_ERR_INVALID_ARGUMENT
    assert st(_d(), camera=cam + 99) == ST_ERR_UNKNOWN_CAMERA and st(None, camera=cam + 99) == ST_ERR_UNKNOWN_CAMERA
    inf, nan = float("inf"), float("nan")
    bad = [_d(struct_size=28), _d(struct_size=36), _d(struct_size=0), _d(flags=2), _d(flags=0x80000001), _d(filter=3), _d(filter=0xffffffff),
           _d(output_width=0), _d(output_height=0), _d(output_width=16385), _d(output_height=16385), _d(output_width=0xffffffff),
           _d(fxaa_edge_threshold=nan), _d(fxaa_edge_threshold=inf), _d(fxaa_edge_threshold=-0.1), _d(fxaa_edge_threshold=-inf),
           _d(fxaa_edge_threshold_min=nan), _d(fxaa_edge_threshold_min=inf), _d(fxaa_edge_threshold_min=-1e-6),
           _d(fxaa_subpixel=nan), _d(fxaa_subpixel=-0.01), _d(fxaa_subpixel=1.01), _d(fxaa_subpixel=inf)]
    for d in bad:
        assert st(d) == ST_ERR_INVALID_ARGUMENT, [getattr(d, f) for f in FIELDS]
        if d.flags == 1:   # a bad field is refused with FXAA off too
            d.flags = 0
            assert st(d) == ST_ERR_INVALID_ARGUMENT, [getattr(d, f) for f in FIELDS]
    # edge values that are valid
    for d in (_d(output_width=16384, output_height=1), _d(output_width=0, output_height=0), _d(fxaa_subpixel=0.0), _d(fxaa_subpixel=1.0),
              _d(fxaa_edge_threshold=0.0, fxaa_edge_threshold_min=0.0), _d(flags=0, filter=0)):
        assert st(d) == ST_OK, [getattr(d, f) for f in FIELDS]
    # get / output size: pointers may be NULL; unknown camera
    assert b.camera_get_post(h, cam, None, None) == ST_OK and b.camera_output_size(h, cam, None, None) == ST_OK
    assert b.camera_get_post(h, cam + 99, None, None) == ST_ERR_UNKNOWN_CAMERA
    assert b.camera_output_size(h, cam + 99, None, None) == ST_ERR_UNKNOWN_CAMERA
    assert b.camera_get_post(None, cam, None, None) == ST_ERR_INVALID_ARGUMENT and b.camera_output_size(None, cam, None, None) == ST_ERR_INVALID_ARGUMENT
    with pytest.raises(StrolleError):
        e.set_post(cam, filter=7)
    e.close()


def test_post_process_checks_its_arguments_and_needs_a_device():
    e, cam = _host_camera()
    b, h = e._b, e._h
    d = _d()
    fake = C.c_void_p(4096)   # never dereferenced: the checks and the missing device come first

    def pp(desc=d, src=fake, w=64, hh=48, dst=fake, fmt=0, engine=h):
        return b.post_process(engine, C.byref(desc) if desc is not None else None, src, w, hh, dst, fmt, None)

    assert pp() == ST_ERR_NO_DEVICE
    assert pp(engine=None) == ST_ERR_INVALID_ARGUMENT
    for kw in (dict(desc=None), dict(src=None), dict(dst=None), dict(w=0), dict(hh=0), dict(w=16385), dict(fmt=4), dict(fmt=-1),
               dict(desc=_d(struct_size=8)), dict(desc=_d(filter=9)), dict(desc=_d(fxaa_subpixel=2.0)), dict(desc=_d(output_width=0))):
        assert pp(**kw) == ST_ERR_INVALID_ARGUMENT, kw
    with pytest.raises(StrolleError):
        e.post_process(d, 4096, 64, 48, 4096)
    e.close()


def test_set_get_and_output_size_round_trip_on_a_host_only_engine():
    e, cam = _host_camera()
    d0, on0 = e.post(cam)
    assert not on0 and d0.struct_size == C.sizeof(api.StPostDesc) and all(getattr(d0, f) == 0 for f in FIELDS[1:])
    assert e.output_size(cam) == (64, 48)
    want = post_desc(fxaa=True, output_size=(200, 120), filter=ResampleFilter.CATMULL_ROM, fxaa_edge_threshold=0.125, fxaa_edge_threshold_min=0.0625,
                     fxaa_subpixel=0.5)
    e.set_post(cam, want)
    got, on = e.post(cam)
    assert on and [getattr(got, f) for f in FIELDS] == [getattr(want, f) for f in FIELDS]
    assert e.output_size(cam) == (200, 120)
    e.tick()
    e.update_camera(cam, scenes.cornell_camera((80, 48)))   # a resize reallocates the camera: the setting and its explicit output size stay
    got, on = e.post(cam)
    assert on and [getattr(got, f) for f in FIELDS] == [getattr(want, f) for f in FIELDS] and e.output_size(cam) == (200, 120)
    e.set_post(cam, fxaa=True)                               # no explicit size: the output follows the render size
    assert e.output_size(cam) == (80, 48)
    e.update_camera(cam, scenes.cornell_camera((96, 64)))
    assert e.output_size(cam) == (96, 64) and e.post(cam)[1]
    e.set_post(cam, output_size=(48, 32), filter=ResampleFilter.NEAREST)
    assert e.output_size(cam) == (48, 32)
    e.set_post(cam, None)
    got, on = e.post(cam)
    assert not on and (got.output_width, got.output_height) == (48, 32) and e.output_size(cam) == (96, 64)   # the last desc stays readable; off = the render size
    e.delete_camera(cam)
    e.close()


def test_post_and_a_window_exclude_each_other_on_a_host_only_engine():
    e, cam = _host_camera()
    b, h = e._b, e._h
    for d in (_d(), post_desc(fxaa=True), post_desc(output_size=(128, 96))):
        A.node_and_window_exclude_each_other(e, cam, "camera_set_post", d, lambda: e.post(cam)[1])
        assert b.camera_set_window(h, cam, 0, 0, 0, 0) == ST_OK
    e.close()


# ---------------------------------------------------------------- post_ref.py against values worked out by hand
def test_reference_catmull_rom_weights():
    w = np.stack(R.catmull_rom_weights(F([0.0, 0.5, 0.25]))).astype(np.float64)
    assert np.array_equal(w[:, 0], [0.0, 1.0, 0.0, 0.0])
    assert np.array_equal(w[:, 1], [-0.0625, 0.5625, 0.5625, -0.0625])
    assert np.array_equal(w[:, 2], [-0.0703125, 0.8671875, 0.2265625, -0.0234375])   # -9/128, 111/128, 29/128, -3/128
    f = np.linspace(0, 1, 33).astype(np.float32)
    assert np.allclose(np.sum(R.catmull_rom_weights(f), 0), 1.0, atol=1e-6)


def _at(img, x, y, fn=R.bilinear):
    ix, fx = R.axis_float(F(x))
    iy, fy = R.axis_float(F(y))
    return fn(np.asarray(img, np.float32), ix, fx, iy, fy)


def test_reference_look_ups_at_hand_computed_values():
    img = np.array([[0.0, 1.0], [2.0, 3.0]], np.float32)
    assert _at(img, 0.25, 0.25) == 0.0      # beyond the corner texel's centre: both axes clamp
    assert _at(img, 1.75, 1.9) == 3.0
    assert _at(img, 1.0, 0.25) == 0.5       # on the top edge: halfway between 0 and 1, rows clamp
    assert _at(img, 0.1, 1.0) == 1.0        # on the left edge: halfway between 0 and 2
    assert _at(img, 1.0, 1.0) == 1.5        # the centre of the four texels
    assert _at(img, 0.75, 0.5) == 0.25 and _at(img, 0.5, 1.25) == 1.5
    assert _at(img, 1.5, 1.5) == 3.0 and _at(img, 0.5, 0.5) == 0.0   # on a texel centre: the texel
    # an infinity next to a texel centre does not leak in (f == 0 takes the texel itself)
    hot = np.array([[1.0, np.inf], [np.nan, 2.0]], np.float32)
    assert _at(hot, 0.5, 0.5) == 1.0 and _at(hot, 1.5, 1.5) == 2.0
    # Catmull-Rom: on a texel the texel; halfway along a ramp the mean (the ramp is reproduced), clamped to the inner texels at an overshoot
    ramp = np.tile(np.arange(6, dtype=np.float32), (6, 1))[..., None]
    assert _at(ramp, 2.5, 2.5, R.catmull_rom)[0] == 2.0 and _at(ramp, 3.0, 2.5, R.catmull_rom)[0] == 2.5
    assert abs(float(_at(ramp, 2.75, 3.2, R.catmull_rom)[0]) - 2.25) < 1e-6
    step = np.tile(np.array([0, 0, 0, 1, 1, 1], np.float32), (6, 1))[..., None]
    # halfway between texels 1 and 2 (both 0) the unclamped cubic gives -0.0625 * 1: the clamp to the inner texels makes it 0
    assert _at(step, 2.0, 2.5, R.catmull_rom)[0] == 0.0 and _at(step, 5.0, 2.5, R.catmull_rom)[0] == 1.0
    assert _at(step, 3.0, 2.5, R.catmull_rom)[0] == 0.5


def test_reference_resampling_of_a_2x2_image():
    img = np.array([[0.0, 3.0], [6.0, 9.0]], np.float32)[..., None].repeat(3, -1)
    near = R.resample(img, 4, 4, R.NEAREST)
    assert np.array_equal(near[..., 0], [[0, 0, 3, 3], [0, 0, 3, 3], [6, 6, 9, 9], [6, 6, 9, 9]]) and (near[..., 3] == 1).all()
    # output pixel 1 samples 1.5 * 2 / 4 = 0.75: a quarter of the way from texel 0 to texel 1
    bil = R.resample(img, 4, 4, R.BILINEAR)
    assert np.array_equal(bil[..., 0], [[0, 0.75, 2.25, 3], [1.5, 2.25, 3.75, 4.5], [4.5, 5.25, 6.75, 7.5], [6, 6.75, 8.25, 9]])
    # exact 2 : 1 bilinear is the 2 x 2 mean; nearest takes floor of the position (1.0 -> texel 1)
    big = np.arange(16, dtype=np.float32).reshape(4, 4)[..., None].repeat(3, -1)
    assert np.array_equal(R.resample(big, 2, 2, R.BILINEAR)[..., 0], [[2.5, 4.5], [10.5, 12.5]])
    assert np.array_equal(R.resample(big, 2, 2, R.NEAREST)[..., 0], [[5, 7], [13, 15]])
    # 3 : 2 non-uniform: 3 columns from 2 sample 1/3, 1, 5/3
    got = R.resample(img, 3, 2, R.BILINEAR)[0, :, 0]
    assert got[0] == 0.0 and got[1] == 1.5 and got[2] == 3.0


def test_reference_identity_at_equal_sizes():
    rng = np.random.default_rng(5)
    img = (rng.standard_normal((13, 17, 4)) * 4).astype(np.float32)
    img[3, 4, 0], img[7, 7, 1], img[0, 0, 2], img[12, 16, 0] = np.inf, np.nan, -np.inf, np.nan
    for flt in (R.NEAREST, R.BILINEAR, R.CATMULL_ROM):
        out = R.resample(img, 17, 13, flt)
        assert bits_equal_mask(out[..., :3], img[..., :3]).all() and (out[..., 3] == 1).all(), flt
    assert bits_equal_mask(R.process(img)[..., :3], img[..., :3]).all()
    # the integer positions are exact where the float product (ox + 0.5) * W is not: 16383.5 * 12289 needs 29 bits
    i0, f, near = R.axis_resample(12289, 12289)
    assert np.array_equal(i0, np.arange(12289)) and not f.any() and np.array_equal(near, np.arange(12289))


def _grey(rows):
    return np.asarray(rows, np.float32)[..., None].repeat(3, -1)


def test_reference_fxaa_at_hand_computed_values():
    # uniform: nothing moves, NaN / negative / huge texels included (their luma is clamped; the colour is copied)
    flat = np.full((6, 7, 3), 0.3, np.float32)
    assert np.array_equal(R.fxaa(flat)[..., :3], flat) and (R.fxaa(flat)[..., 3] == 1).all()
    # a step below the threshold: luma sqrt(0.5) = 0.7071 against sqrt(0.55) = 0.7416, range 0.0345 < max(0.0833, 0.166 * 0.74)
    low = _grey(np.where(np.arange(8)[None, :] < 4, 0.5, 0.55) * np.ones((6, 1)))
    assert np.array_equal(R.fxaa(low)[..., :3], low)
    # ... and above it with lower thresholds: something moves
    assert not np.array_equal(R.fxaa(low, 0.01, 0.01)[..., :3], low)
    # a 5 x 5 image: rows 0-1 white (but texel (0, 1) black), rows 2-4 black; luma = value (white's luma is 1 within an ulp)
    img = np.zeros((5, 5), np.float32)
    img[0, :], img[1, 1:] = 1.0, 1.0
    d = {}
    out = R.fxaa(_grey(img), details=d)[..., 0].astype(np.float64)
    # pixel (2, 1), white above the edge: M = N = E = W = NW = NE = 1, S = SW = SE = 0. range 1; edgeH = 1 + 2 + 1 = 4, edgeV = 0: horizontal.
    # |N - M| = 0 < |S - M| = 1: the positive side (S), gradient 1, local average 0.5. The walk runs along y = 2.0 (rows 1 and 2 blended
    # evenly: 0.5 under white, 0 under the black texel): the negative side meets luma 0 at distance 2 (x = 0: |0 - 0.5| >= 0.25), the
    # positive side never ends (clamped white): 26.5. The nearer end's delta (-0.5) is negative, the centre's (1 - 0.5) is not: the edge
    # offset 0.5 - 2 / 28.5 counts. Subpixel: |(2 * 3 + 2) / 12 - 1| / 1 = 1/3, s = (3 - 2/3) / 9 = 7/27, offset (7/27)^2 * 0.75 = 0.0504:
    # smaller. The colour is row 1 moved 0.4298 towards row 2: 1 - 0.4298 = 0.5 + 2 / 28.5.
    assert d["edge"][1, 2] and d["horizontal"][1, 2] and not d["pick_negative"][1, 2]
    assert d["distance_negative"][1, 2] == 2.0 and d["distance_positive"][1, 2] == 26.5 and d["good"][1, 2]
    assert abs(float(d["offset_edge"][1, 2]) - (0.5 - 2 / 28.5)) < 1e-6 and abs(float(d["offset_sub"][1, 2]) - 0.75 * (7 / 27) ** 2) < 1e-6
    assert abs(out[1, 2] - (0.5 + 2 / 28.5)) < 1e-6
    # pixel (2, 2), black below the edge: picks N (a tie is impossible: |N - M| = 1 > 0); its nearer end's delta and its own have the same
    # sign, so only the subpixel term moves it: 0 + (1 - 0) * 0.75 * (7/27)^2
    assert d["pick_negative"][2, 2] and not d["good"][2, 2] and d["offset_edge"][2, 2] == 0.0
    assert abs(out[2, 2] - 0.75 * (7 / 27) ** 2) < 1e-6
    # far from the edge nothing moves
    assert out[4, 2] == 0.0 and not d["edge"][4, 2] and out[0, 3] == 1.0
    # subpixel 0 on an edge whose span is not "good": the pixel stays
    assert R.fxaa(_grey(img), subpixel=0.0)[2, 2, 0] == 0.0


SLOPES = {"1/8": (1 / 8, 17.3), "1/3": (1 / 3, 5.2), "-1/5": (-1 / 5, 33.1)}


def slanted_edge_errors(slope, offset, w=96, h=48):
    """mean absolute error against the analytic pixel coverage of the half-plane, before and after the restatement's FXAA"""
    sampled, coverage = R.half_plane(w, h, slope, offset)
    out = R.fxaa(_grey(sampled))[..., 0].astype(np.float64)
    return float(np.abs(sampled - coverage).mean()), float(np.abs(out - coverage).mean())


@pytest.mark.parametrize("name", list(SLOPES))
def test_fxaa_brings_a_slanted_edge_closer_to_its_coverage(name):
    before, after = slanted_edge_errors(*SLOPES[name])
    print(f"slope {name}: mean absolute error {before:.6f} -> {after:.6f}")
    assert after < before
