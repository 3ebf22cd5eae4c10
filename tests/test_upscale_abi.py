"""CPU tests of the upscale stage (include/strolle_hip.h "upscaling"): the entry points are exported, declared and bound by the Rust facade,
StUpscaleDesc has one layout in the header, api.py and ffi.rs, every argument error occurs on a host-only engine, set / get / output size
round-trip there, a window and the stage — and a resizing StPostDesc and the stage — exclude each other in both orders, st_upscale_process
says that it needs a device; the numpy restatement (upscale_ref.py) gives values worked out by hand, stays within a recorded tolerance of
its float64 definition over the GPU test's matrix, and brings slanted edges closer to their analytic coverage than Catmull-Rom does."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import output_chain_abi as A
import upscale_cases as K
import upscale_ref as U
from output_chain_abi import ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE, ST_OK, host_camera as _host_camera
from parity import bits_equal_mask
from strolle_amd import StrolleError, api, post_desc, scenes, upscale_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("st_camera_set_upscale", "st_camera_get_upscale", "st_upscale_process")
FIELDS = ["struct_size", "flags", "output_width", "output_height", "sharpness", "_pad"]
F = np.float32


def test_entry_points_are_exported_declared_and_bound():
    header, ffi = A.exports_header_and_ffi_agree("StUpscaleDesc", FIELDS, ENTRY_POINTS, [("ST_UPSCALE_DENOISE", 1)])
    assert "pub _pad: [u32; 3]," in ffi and "uint32_t _pad[3];" in header and api.UPSCALE_DENOISE == 1


def test_desc_layout_agrees_between_c_and_ctypes(tmp_path):
    got = A.c_layout(tmp_path, "StUpscaleDesc", FIELDS, ["ST_UPSCALE_DENOISE"])
    assert got == [32, 0, 4, 8, 12, 16, 20, 1]


def _d(**kw):
    d = upscale_desc(output_size=(128, 96), sharpness=0.5, denoise=True)
    pad = kw.pop("pad", None)
    for k, v in kw.items():
        setattr(d, k, v)
    if pad is not None:
        d._pad[pad] = 1
    return d


BAD = [dict(struct_size=28), dict(struct_size=36), dict(struct_size=0), dict(flags=2), dict(flags=0x80000001), dict(pad=0), dict(pad=1), dict(pad=2),
       dict(output_width=0), dict(output_height=0), dict(output_width=16385, output_height=96), dict(output_width=128, output_height=16385),
       dict(output_width=0xffffffff), dict(output_width=63), dict(output_height=47), dict(output_width=1, output_height=1),
       dict(sharpness=float("nan")), dict(sharpness=-0.01), dict(sharpness=1.01), dict(sharpness=float("inf")), dict(sharpness=-float("inf"))]
GOOD = [dict(output_width=16384, output_height=48), dict(output_width=64, output_height=16384), dict(output_width=0, output_height=0),
        dict(output_width=64, output_height=48), dict(output_width=65, output_height=48), dict(sharpness=0.0), dict(sharpness=1.0), dict(flags=0),
        dict(output_width=0, output_height=0, sharpness=0.0, flags=0)]


def test_argument_errors_on_a_host_only_engine():
    e, cam = _host_camera()   # renders 64 x 48
    A.argument_errors(e, cam, "camera_set_upscale", "camera_get_upscale", _d, BAD, GOOD)
    with pytest.raises(StrolleError):
        e.set_upscale(cam, sharpness=2.0)
    e.close()


def test_upscale_process_checks_its_arguments_and_needs_a_device():
    e, cam = _host_camera()
    b, h = e._b, e._h
    src, dst = C.c_void_p(1 << 20), C.c_void_p(1 << 30)   # never dereferenced: the checks and the missing device come first

    def up(desc=_d(), s=src, w=64, hh=48, d=dst, fmt=0, engine=h):
        return b.upscale_process(engine, C.byref(desc) if desc is not None else None, s, w, hh, d, fmt, None)

    assert up() == ST_ERR_NO_DEVICE
    assert up(engine=None) == ST_ERR_INVALID_ARGUMENT
    for kw in (dict(desc=None), dict(s=None), dict(d=None), dict(w=0), dict(hh=0), dict(w=16385), dict(fmt=4), dict(fmt=-1), dict(desc=_d(struct_size=8)),
               dict(desc=_d(flags=4)), dict(desc=_d(pad=1)), dict(desc=_d(sharpness=2.0)), dict(desc=_d(output_width=0)), dict(w=129), dict(hh=97)):
        assert up(**kw) == ST_ERR_INVALID_ARGUMENT, kw
    # src and dst overlapping: the same pointer, dst inside src, src inside dst (64 x 48 RGBA32F is 49152 B, 128 x 96 RGBA32F 196608 B)
    base = 1 << 20
    for s, d in ((base, base), (base, base + 49152 - 1), (base + 196608 - 1, base), (base + 1000, base)):
        assert up(s=C.c_void_p(s), d=C.c_void_p(d)) == ST_ERR_INVALID_ARGUMENT, (s, d)
    for s, d in ((base, base + 49152), (base + 196608, base)):   # touching is not overlapping
        assert up(s=C.c_void_p(s), d=C.c_void_p(d)) == ST_ERR_NO_DEVICE, (s, d)
    assert up(s=C.c_void_p(base + 49152), d=C.c_void_p(base), fmt=2) == ST_ERR_NO_DEVICE   # an 8-bit destination is a quarter of that
    with pytest.raises(StrolleError):
        e.upscale_process(_d(), 1 << 20, 64, 48, 1 << 30)
    e.close()


def test_set_get_and_output_size_round_trip_on_a_host_only_engine():
    e, cam = _host_camera()
    d0, on0 = e.upscale(cam)
    assert not on0 and d0.struct_size == 32 and d0.flags == 0 and d0.output_width == 0 and d0.sharpness == 0 and list(d0._pad) == [0, 0, 0]
    assert e.output_size(cam) == (64, 48)
    want = upscale_desc(output_size=(200, 120), sharpness=0.25, denoise=True)
    e.set_upscale(cam, want)
    got, on = e.upscale(cam)
    assert on and [got.flags, got.output_width, got.output_height, got.sharpness] == [1, 200, 120, 0.25]
    assert e.output_size(cam) == (200, 120)
    e.tick()
    e.update_camera(cam, scenes.cornell_camera((80, 48)))   # a resize reallocates the camera: the setting and its output size stay
    assert e.upscale(cam)[1] and e.output_size(cam) == (200, 120)
    for size in ((201, 48), (80, 121)):                      # a render size larger than the live output size: refused, the camera as it was
        with pytest.raises(StrolleError):
            e.update_camera(cam, scenes.cornell_camera(size))
        assert e.output_size(cam) == (200, 120)
    e.update_camera(cam, scenes.cornell_camera((200, 120)))  # equal is allowed: sharpen only from here
    e.update_camera(cam, scenes.cornell_camera((80, 48)))
    e.set_upscale(cam, sharpness=0.5)                        # no output size: the output follows the render size
    assert e.output_size(cam) == (80, 48)
    e.update_camera(cam, scenes.cornell_camera((96, 64)))
    assert e.output_size(cam) == (96, 64) and e.upscale(cam)[1]
    e.set_exact(True); e.set_exact(False)                    # the setting survives an arithmetic switch
    assert e.upscale(cam)[1] and e.upscale(cam)[0].sharpness == 0.5
    e.set_upscale(cam, output_size=(192, 128))
    assert e.output_size(cam) == (192, 128)
    e.set_upscale(cam, None)
    got, on = e.upscale(cam)
    assert not on and (got.output_width, got.output_height) == (192, 128) and e.output_size(cam) == (96, 64)   # the last desc stays readable
    e.update_camera(cam, scenes.cornell_camera((300, 200)))  # off: no limit on the render size
    e.delete_camera(cam)
    e.close()


def test_upscale_and_a_window_exclude_each_other_on_a_host_only_engine():
    e, cam = _host_camera()
    b, h = e._b, e._h
    for d in (_d(), upscale_desc(sharpness=1.0), upscale_desc(output_size=(128, 96)), upscale_desc()):
        A.node_and_window_exclude_each_other(e, cam, "camera_set_upscale", d, lambda: e.upscale(cam)[1])
        assert b.camera_set_window(h, cam, 0, 0, 0, 0) == ST_OK
    e.set_upscale(cam, _d())
    assert b.camera_set_window(h, cam, 16, 0, 64, 48) == ST_ERR_INVALID_ARGUMENT
    assert "a window on a camera with upscaling" in b.last_error().decode() and "tile edges" in b.last_error().decode()
    e.set_upscale(cam, None)
    assert b.camera_set_window(h, cam, 16, 0, 64, 48) == ST_OK
    assert b.camera_set_upscale(h, cam, C.byref(_d())) == ST_ERR_INVALID_ARGUMENT
    assert "upscaling on a camera with a window" in b.last_error().decode()
    e.close()


def test_upscale_and_a_resizing_post_desc_exclude_each_other_on_a_host_only_engine():
    e, cam = _host_camera()
    b, h = e._b, e._h
    resize, fxaa, same = post_desc(fxaa=True, output_size=(128, 96)), post_desc(fxaa=True), post_desc(fxaa=True, output_size=(64, 48))
    # post-processing that resizes, then the stage: refused (whatever the stage asks for), and the stage stays off
    e.set_post(cam, resize)
    for d in (_d(), upscale_desc(sharpness=1.0), upscale_desc()):
        assert b.camera_set_upscale(h, cam, C.byref(d)) == ST_ERR_INVALID_ARGUMENT
        assert "upscaling on a camera with post-processing that resizes: one stage owns the resize" in b.last_error().decode()
        assert not e.upscale(cam)[1] and e.output_size(cam) == (128, 96)
    assert b.camera_set_upscale(h, cam, None) == ST_OK
    # FXAA alone — no output size, or the render size spelt out — is fine in either order
    for p in (fxaa, same):
        e.set_post(cam, p); e.set_upscale(cam, _d())
        assert e.output_size(cam) == (128, 96) and e.post(cam)[1] and e.upscale(cam)[1]
        e.set_upscale(cam, None); e.set_upscale(cam, _d()); e.set_post(cam, p)
        e.set_upscale(cam, None)
    # the stage, then post-processing that resizes: refused, and post-processing stays as it was
    e.set_post(cam, fxaa); e.set_upscale(cam, _d())
    assert b.camera_set_post(h, cam, C.byref(resize)) == ST_ERR_INVALID_ARGUMENT
    assert "post-processing that resizes on a camera with upscaling: one stage owns the resize" in b.last_error().decode()
    assert e.post(cam)[0].output_width == 0 and e.post(cam)[1]
    # ... and a render size that would turn a spelt-out output size of post-processing into a resize is refused too
    e.set_post(cam, same)
    with pytest.raises(StrolleError):
        e.update_camera(cam, scenes.cornell_camera((80, 48)))
    assert e.output_size(cam) == (128, 96)
    e.set_upscale(cam, None)
    e.set_post(cam, resize)
    assert e.output_size(cam) == (128, 96)
    e.close()


# ---------------------------------------------------------------- upscale_ref.py against values worked out by hand
def _grey(rows):
    return K.grey(np.asarray(rows, np.float32))


def _weights(dir_x, dir_y, l2x, l2y, lob, fx, fy):
    """the twelve tap weights from the header's formulas in Python floats, and which taps the d2 clamp caught"""
    out, clamped = {}, set()
    for k, (dx, dy) in U.TAPS.items():
        ox, oy = dx - fx, dy - fy
        vx, vy = (ox * dir_x + oy * dir_y) * l2x, (-ox * dir_y + oy * dir_x) * l2y
        d2 = vx * vx + vy * vy
        if d2 > 1.0 / lob:
            d2 = 1.0 / lob; clamped.add(k)
        out[k] = (1.5625 * (0.4 * d2 - 1.0) ** 2 - 0.5625) * (lob * d2 - 1.0) ** 2
    return out, clamped


def test_reference_constant_image_comes_back_exactly():
    for v in (0.0, 1.0, 0.3, 0.7071, 1e-30):
        img = np.full((7, 9, 4), v, np.float32)
        for size in ((9, 7), (10, 8), (12, 10), (18, 14), (27, 21), (18, 7)):
            out = U.process(img, size)
            assert out.shape == (size[1], size[0], 4) and (out[..., :3] == F(v)).all() and (out[..., 3] == 1).all(), (v, size)
    # outside [0, 1] the stage clips: display-referred
    hot = np.full((4, 4, 4), 7.5, np.float32)
    hot[1, 1] = np.nan; hot[2, 2] = -3.0
    out = U.process(hot, (8, 8))
    assert np.isfinite(out).all() and out.min() >= 0 and out.max() <= 1


def test_reference_upscale_on_a_vertical_step_worked_out_by_hand():
    # 6 x 6, columns 0 0 0 1 1 1, to 12 x 12. Output pixel (5, 5): n = 11 * 6 - 12 = 54, d = 24: x0 = y0 = 2, fx = fy = 0.25. Lumas are
    # 2 v. Stencil weights 0.5625, 0.1875, 0.1875, 0.0625. Along x the stencils on column 2 see 0 0 2 and those on column 3 see 0 2 2: r - p = 2,
    # m = 2, t = 1 each: dir.x = 2, len = 1; along y everything is flat: dir.y = 0. r2 = 4, dir = (1, 0), len = (0.5)^2 = 0.25, stretch = 1,
    # len2 = (1, 0.875), lob = 0.5 - 0.29 * 0.25 = 0.4275, clp = 1 / 0.4275.
    img = _grey(np.tile((np.arange(6) >= 3).astype(np.float32), (6, 1)))
    d = {}
    out = U.upscale_f32(img, 12, 12, d)
    at = lambda k: float(d[k][5, 5])   # noqa: E731
    assert (at("dir_x"), at("dir_y"), at("r2"), at("len"), at("len2_x"), at("len2_y")) == (1.0, 0.0, 4.0, 0.25, 1.0, 0.875)
    assert abs(at("lob") - 0.4275) < 1e-7 and abs(at("clp") - 1 / 0.4275) < 1e-6
    want, clamped = _weights(1.0, 0.0, 1.0, 0.875, 0.4275, 0.25, 0.25)
    # the d2 clamp: h and l lie 1.75 to the right (d2 > 3.06), n and o 1.75 * 0.875 below (d2 > 2.34), beyond clp = 2.339: their weight is 0
    assert clamped == {"h", "l", "n", "o"} and all(abs(want[k]) < 1e-30 for k in clamped)
    for k in U.TAPS:
        assert abs(float(d["weights"][k][5, 5]) - want[k]) < 2e-7, k
    assert abs(want["f"] - 0.78540706) < 1e-7 and abs(want["j"] - 0.27673659) < 1e-7 and abs(want["b"] + 0.03783237) < 1e-7   # tap f lies 0.25, 0.25 * 0.875 away
    # without the clamp tap h would weigh in: (1.5625 (0.4 * 3.1103 - 1)^2 - 0.5625) (0.4275 * 3.1103 - 1)^2 = -0.0518
    assert abs((1.5625 * (0.4 * 3.1103 - 1) ** 2 - 0.5625) * (0.4275 * 3.1103 - 1) ** 2 + 0.0518) < 1e-3
    # the white taps are those of columns 3 and 4, c g h k l o, of which h l o weigh nothing: the pixel is (w_c + w_g + w_k) / sum
    assert abs(float(out[5, 5, 0]) - (want["c"] + want["g"] + want["k"]) / sum(want.values())) < 1e-6 and abs(float(out[5, 5, 0]) - 0.13748105) < 1e-7
    assert abs(float(d["wsum"][5, 5]) - 1.1339002) < 1e-6 and d["fallback"] == 0


def test_reference_upscale_on_a_45_degree_step_worked_out_by_hand():
    # 6 x 6, v = 1 where x + y >= 6, to 12 x 12; pixel (5, 5) again: x0 = y0 = 2, fx = fy = 0.25. Lumas: h k l n o are 2, the other seven 0.
    # Stencil f sees nothing. g: along x f g h = 0 0 2, along y c g k = 0 0 2: both add 2 w_g to dir and w_g to len. j likewise with w_j;
    # k: j k l = 0 2 2 and g k o = 0 2 2: 2 w_k and w_k. dir = (0.875, 0.875), len = 2 * 0.4375 = 0.875; r2 = 1.53125; dir = (1, 1) / sqrt 2;
    # len = 0.4375^2 = 0.19140625; stretch = sqrt 2; len2 = (1 + 0.41421356 * 0.19140625, 1 - 0.095703125); lob = 0.5 - 0.29 * 0.19140625.
    x = np.arange(6)
    img = _grey((x[None, :] + x[:, None] >= 6).astype(np.float32))
    d = {}
    out = U.upscale_f32(img, 12, 12, d)
    at = lambda k: float(d[k][5, 5])   # noqa: E731
    s = math.sqrt(0.5)
    assert at("r2") == 1.53125 and at("len") == 0.19140625 and at("len2_y") == 0.904296875
    assert abs(at("dir_x") - s) < 1e-7 and abs(at("dir_y") - s) < 1e-7 and abs(at("len2_x") - (1 + (math.sqrt(2) - 1) * 0.19140625)) < 2e-7
    assert abs(at("lob") - 0.4444921875) < 1e-7
    want, clamped = _weights(s, s, 1 + (math.sqrt(2) - 1) * 0.19140625, 0.904296875, 0.4444921875, 0.25, 0.25)
    assert clamped == {"h", "l", "n", "o"}
    for k in U.TAPS:
        assert abs(float(d["weights"][k][5, 5]) - want[k]) < 3e-7, k
    assert abs(want["b"] - want["e"]) < 1e-12 and abs(want["g"] - want["j"]) < 1e-12 and abs(want["c"] - want["i"]) < 1e-12   # the diagonal's symmetry
    assert abs(want["f"] - 0.72017230) < 1e-7 and abs(want["k"] + 0.03638803) < 1e-7
    # the only white tap with a weight is k, and it is negative: the sum is below 0 and the clamp to f g j k brings it back to 0
    assert out[5, 5, 0] == 0.0
    assert np.abs(out[..., 0] - out[..., 0].T).max() < 1e-6   # the image is symmetric about its main diagonal; so is the result, but for the order of the sums


def test_reference_r2_threshold_on_both_sides():
    # a vertical ramp v = a y: every stencil adds (2 a * 2) w along y: dir = (0, 4 a), r2 = 16 a^2 against 1 / 32768 = 3.05e-5
    y = np.arange(6, dtype=np.float64)[:, None] * np.ones((1, 6))
    for a, want_dir in ((0.001, (1.0, 0.0)), (0.002, (0.0, 1.0))):
        d = {}
        U.upscale_f32(_grey(a * y), 12, 12, d)
        r2 = float(d["r2"][5, 5])
        assert abs(r2 - 16 * a * a) < 1e-9 and (r2 < U.R2_MIN) == (a == 0.001)
        assert (float(d["dir_x"][5, 5]), float(d["dir_y"][5, 5])) == want_dir, a
    assert U.R2_MIN == 2.0 ** -15


def test_reference_sharpen_guards_and_the_flat_field():
    for v in (0.0, 1.0):   # all black: mx4 == 0 guards hitMin; all white: 4 mn4 - 4 == 0 guards hitMax; either way the lobe is 0
        d = {}
        out = U.sharpen_f32(np.full((4, 5, 4), v, np.float32), 1.0, True, d)
        assert (out[..., :3] == v).all() and (d["lobe"] == 0).all() and np.isfinite(out).all()
    # flat 0.4: hitMin = 0.4 / 1.6 = 0.25, hitMax = 0.6 / (1.6 - 4) = -0.25: lobe_c = -0.25, held to -0.1875, times sharpness; the range of
    # the lumas is 0, so the noise term is 0 and the limiter's factor 1
    for sharp in (1.0, 0.5, 0.25):
        d = {}
        out = U.sharpen_f32(np.full((4, 5, 4), 0.4, np.float32), sharp, True, d)
        assert (d["lobe"] == F(-0.1875) * F(sharp)).all() and (d["noise"] == 0).all()
        assert np.abs(out[..., :3].astype(np.float64) - 0.4).max() < 1e-7


def test_reference_sharpen_on_one_noisy_pixel_with_and_without_the_limiter():
    # 0.5 everywhere, 0.8 in the middle. At the middle: mn4 = mx4 = 0.5: hitMin = 0.5 / 2 = 0.25, hitMax = (1 - 0.8) / (2 - 4) = -0.1:
    # lobe = -0.1: (4 * -0.1 * 0.5 + 0.8) / (1 - 0.4) = 1: the outlier is pushed to white. With the limiter: lumas 1 1 1 1 and 1.6, range 0.6,
    # nz = |1 - 1.6| / 0.6 = 1: lobe = -0.05: (-0.1 + 0.8) / 0.8 = 0.875.
    f = np.full((5, 5), 0.5, np.float32)
    f[2, 2] = 0.8
    d0, d1 = {}, {}
    plain, limited = U.sharpen_f32(_grey(f), 1.0, False, d0), U.sharpen_f32(_grey(f), 1.0, True, d1)
    assert abs(float(d0["lobe"][2, 2]) + 0.1) < 1e-7 and abs(float(plain[2, 2, 0]) - 1.0) < 1e-6
    assert abs(float(d1["noise"][2, 2]) - 1.0) < 1e-6 and abs(float(d1["lobe"][2, 2]) + 0.05) < 1e-7 and abs(float(limited[2, 2, 0]) - 0.875) < 1e-6
    # its left neighbour: b d h = 0.5, f = 0.8, e = 0.5: hitMin = 0.5 / 3.2, hitMax = (1 - 0.8) / -2 = -0.1: lobe -0.1:
    # (-0.1 * 2.3 + 0.5) / 0.6 = 0.45; limited: lumas 1 1 1.6 1 and 1: nz = |1.15 - 1| / 0.6 = 0.25: lobe -0.0875: (0.5 - 0.20125) / 0.65
    assert abs(float(plain[2, 1, 0]) - 0.45) < 1e-6 and abs(float(limited[2, 1, 0]) - 0.29875 / 0.65) < 1e-6
    assert (plain[0, 0, :3] == 0.5).all()


def test_reference_sharpness_zero_is_skipping_the_step():
    img = K.source("noise", (37, 23))
    up = U.upscale_f32(img, 55, 35)
    assert bits_equal_mask(U.process(img, (55, 35), 0.0, True), up).all()
    assert bits_equal_mask(U.process(img, (55, 35), 0.5, False), U.sharpen_f32(up, 0.5, False)).all()
    assert bits_equal_mask(U.process(img, None, 0.5, True), U.sharpen_f32(img, 0.5, True)).all()
    assert bits_equal_mask(U.process(img, (0, 0), 0.0)[..., :3], img[..., :3]).all()   # neither step: the copy, unclamped
    assert not bits_equal_mask(U.process(img, (55, 35), 0.5), up).all()


# ---------------------------------------------------------------- the restatement against its float64 definition
def r2_margin():
    """four times the restatement's worst relative r2 deviation over the matrix, as an absolute distance from the threshold"""
    worst = max(K.r2_deviation(K.source(name, size), osize) for name, size, _o, osize, _s, _d in K.cases() if osize != size)
    return worst, 4.0 * worst * U.R2_MIN


def restatement_vs_definition(margin):
    """over the GPU test's matrix, every pixel counted but those within `margin` of the r2 threshold: the worst deviation of the restatement
    from the definition, the largest fraction of a case's pixels left out, the smallest weight sum and the fall-backs to tap f"""
    worst, left_out, wsum_min, fallback, where = 0.0, 0.0, math.inf, 0, None
    for case in K.cases():
        name, size, oname, osize, sharp, den = case
        img = K.source(name, size)
        got, want, skip = K.f64_comparison(img, osize, sharp, den, margin)
        dev = K.deviation(got, want, skip)
        if osize != size:
            d = {}
            U.upscale_f32(img, osize[0], osize[1], d)
            wsum_min, fallback = min(wsum_min, d["wsum_min"]), fallback + d["fallback"]
        if dev > worst:
            worst, where = dev, "%s %dx%d -> %s sharpness %g%s" % (name, size[0], size[1], oname, sharp, " limiter" if den else "")
        left_out = max(left_out, float(skip.mean()))
    return dict(worst=worst, case=where, largest_fraction_left_out=left_out, smallest_weight_sum=wsum_min, fallbacks_to_tap_f=fallback, cases=len(K.cases()))


def recorded():
    return json.load(open(os.path.join(ROOT, "profiles", "upscale.json")))["restatement_vs_definition"]


def test_restatement_stays_within_the_recorded_tolerance_of_the_float64_definition():
    rec = recorded()
    worst_r2, margin = r2_margin()
    got = restatement_vs_definition(rec["r2_margin"])
    print(worst_r2, margin, got)
    # the tolerance is four times the restatement's own worst deviation and the margin four times its worst r2 deviation (relative, taken at
    # the threshold), both as recorded by tools/upscale_bench.py --restatement from this very matrix
    assert rec["tolerance"] == 4.0 * rec["worst"] and rec["r2_margin"] == 4.0 * rec["worst_r2_deviation"] * U.R2_MIN
    assert rec["worst"] / 2.0 <= got["worst"] <= rec["tolerance"] and rec["worst_r2_deviation"] / 2.0 <= worst_r2 <= 4.0 * rec["worst_r2_deviation"], "the record is this matrix's"
    assert rec["tolerance"] < 1e-4, "a fortieth of an 8-bit step"
    assert got["largest_fraction_left_out"] <= 0.01
    assert got["fallbacks_to_tap_f"] == 0 and got["smallest_weight_sum"] > 0.5


# ---------------------------------------------------------------- the quality claim
@pytest.mark.parametrize("ratio", list(K.EDGE_RATIOS))
@pytest.mark.parametrize("angle", K.EDGE_ANGLES)
def test_upscaling_brings_a_slanted_edge_closer_to_its_coverage_than_catmull_rom(angle, ratio):
    up, cr = K.edge_rms(angle, K.EDGE_RATIOS[ratio])
    print(f"{angle:g} degrees at {ratio}: RMS error {up:.5f} against Catmull-Rom's {cr:.5f}: {up / cr:.3f}")
    assert up < cr


def test_axis_aligned_edges_are_recorded_not_asserted():
    for angle in K.EDGE_AXIS_ANGLES:
        for ratio, r in K.EDGE_RATIOS.items():
            up, cr = K.edge_rms(angle, r)
            print(f"{angle:g} degrees at {ratio}: RMS error {up:.5f} against Catmull-Rom's {cr:.5f}: {up / cr:.3f} (the kernel is not separable: slightly worse is expected)")
            assert np.isfinite(up) and np.isfinite(cr)
