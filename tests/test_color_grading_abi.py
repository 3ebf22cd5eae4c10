"""CPU tests of colour grading (include/strolle_hip.h "colour grading"): the entry points are exported, declared and bound by the Rust facade,
StColorGradingDesc has one layout in the header, api.py and ffi.rs, every argument error occurs on a host-only engine, set / get / clear
round-trip there (also across st_camera_update), a window and grading go together through all three window setters, the plan's matrix
against numpy float64, st_lut_insert / st_lut_remove, st_decode_cube on texts written here (and, under AddressSanitizer and UBSan, on
mutated ones), the numpy restatement (grade_ref.grade_f32) at cases worked out by hand, and the restatement against the float64 definition
(grade_ref.grade_f64) over the GPU test's whole input matrix."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import grade_cases as K
import grade_ref as R
import output_chain_abi as A
from output_chain_abi import ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE, ST_OK, host_camera as _host_camera
from strolle_amd import Engine, LutDomain, StrolleError, Tonemap, api, color_grading_desc, color_grading_plan, decode_cube, display_desc, scenes
from strolle_amd.api import dist_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_ERR_PARSE, ST_ERR_UNSUPPORTED = 8, 9
ENTRY_POINTS = ("st_camera_set_color_grading", "st_camera_get_color_grading", "st_lut_insert", "st_lut_remove", "st_color_grading_plan", "st_color_grading_process",
                "st_decode_cube")
FIELDS = ["struct_size", "flags", "temperature", "tint", "contrast", "saturation", "slope", "offset", "power", "cdl_saturation", "lut", "lut_domain", "lut_ev_min",
          "lut_ev_max", "lut_strength", "_pad"]
OFFSETS = [0, 4, 8, 12, 16, 20, 24, 36, 48, 60, 64, 72, 76, 80, 84, 88]
CONSTANTS = [("ST_GRADE_DITHER", 1), ("ST_LUT_DOMAIN_UNIT", 0), ("ST_LUT_DOMAIN_LOG2", 1), ("ST_GRADE_STEP_WHITE_BALANCE", 1), ("ST_GRADE_STEP_CONTRAST", 2),
             ("ST_GRADE_STEP_SATURATION", 4), ("ST_GRADE_STEP_CDL", 8), ("ST_GRADE_STEP_LUT", 16), ("ST_GRADE_STEP_DITHER", 32)]
F = np.float32
inf, nan = float("inf"), float("nan")


def test_entry_points_are_exported_declared_and_bound():
    header, ffi = A.exports_header_and_ffi_agree("StColorGradingDesc", FIELDS, ENTRY_POINTS, CONSTANTS)
    assert int(LutDomain.UNIT) == R.UNIT == 0 and int(LutDomain.LOG2) == R.LOG2 == 1 and api.GRADE_DITHER == R.DITHER == 1
    assert (api.GRADE_STEP_WHITE_BALANCE, api.GRADE_STEP_CONTRAST, api.GRADE_STEP_SATURATION, api.GRADE_STEP_CDL, api.GRADE_STEP_LUT, api.GRADE_STEP_DITHER) \
        == (R.WHITE_BALANCE, R.CONTRAST, R.SATURATION, R.CDL, R.LUT, R.DITHER_STEP)
    plan = ["steps", "white_balance", "lut_inv_range", "_pad"]
    assert re.findall(r"pub (\w+):", re.search(r"pub struct StColorGradingPlan \{(.*?)\n\}", ffi, re.S).group(1)) == plan == [f for f, _ in api.StColorGradingPlan._fields_]


def test_desc_layout_agrees_between_c_and_ctypes(tmp_path):
    got = A.c_layout(tmp_path, "StColorGradingDesc", FIELDS, [n for n, _ in CONSTANTS])
    assert got == [96] + OFFSETS + [v for _, v in CONSTANTS]
    assert C.sizeof(api.StColorGradingPlan) == 48 and api.StColorGradingPlan.white_balance.offset == 4 and api.StColorGradingPlan.lut_inv_range.offset == 40


def _d(**kw):
    """a desc with every step active and valid in both domains, then `kw` over it (a tuple replaces a whole array, name_i one element)"""
    d = color_grading_desc(temperature=0.2, tint=-0.1, contrast=1.2, saturation=0.9, slope=(1.1, 1.0, 0.9), offset=(0.01, 0.0, -0.01), power=(1.1, 1.0, 0.9),
                           cdl_saturation=1.1, lut=7, lut_ev_min=-10.0, lut_ev_max=6.0, dither=True)
    for k, v in kw.items():
        m = re.fullmatch(r"(\w+?)_(\d)", k)
        if m and hasattr(d, m.group(1)) and not hasattr(d, k):
            getattr(d, m.group(1))[int(m.group(2))] = v
        elif isinstance(v, tuple):
            setattr(d, k, (C.c_float * len(v))(*v))
        else:
            setattr(d, k, v)
    return d


BAD = [dict(struct_size=92), dict(struct_size=104), dict(struct_size=0), dict(flags=2), dict(flags=0x80000001), dict(lut_domain=2), dict(lut_domain=0xffffffff),
       dict(temperature=nan), dict(temperature=1.01), dict(temperature=-1.01), dict(temperature=inf), dict(tint=nan), dict(tint=-inf), dict(tint=1.5),
       dict(contrast=0.0), dict(contrast=-1.0), dict(contrast=4.01), dict(contrast=nan), dict(contrast=inf),
       dict(saturation=-0.01), dict(saturation=4.01), dict(saturation=nan), dict(cdl_saturation=-0.5), dict(cdl_saturation=5.0), dict(cdl_saturation=nan),
       dict(slope_0=-0.1), dict(slope_1=16.5), dict(slope_2=nan), dict(offset_0=-1.01), dict(offset_1=1.01), dict(offset_2=inf),
       dict(power_0=0.0), dict(power_1=-1.0), dict(power_2=8.5), dict(power_0=nan),
       dict(lut_strength=-0.1), dict(lut_strength=1.1), dict(lut_strength=nan), dict(lut_ev_min=nan), dict(lut_ev_max=inf), dict(lut_ev_min=-inf),
       dict(lut_domain=1, lut_ev_min=2.0, lut_ev_max=2.0), dict(lut_domain=1, lut_ev_min=3.0, lut_ev_max=2.0), dict(lut_domain=1, lut_strength=0.5),
       dict(lut_domain=1, lut_strength=0.0)]
GOOD = [dict(), dict(flags=0), dict(flags=1), dict(lut_domain=1), dict(lut_domain=0, lut_ev_min=3.0, lut_ev_max=2.0), dict(temperature=1.0, tint=-1.0),
        dict(temperature=-1.0, tint=1.0), dict(contrast=4.0), dict(contrast=1e-3), dict(saturation=0.0), dict(saturation=4.0), dict(cdl_saturation=0.0),
        dict(slope=(0.0, 16.0, 1.0)), dict(offset=(-1.0, 1.0, 0.0)), dict(power=(8.0, 1e-3, 1.0)), dict(lut_strength=0.0), dict(lut_strength=0.5), dict(lut=0),
        dict(lut=0xffffffffffff), dict(_pad_0=123, _pad_1=0xffffffff)]


def test_argument_errors_on_a_host_only_engine():
    e, cam = _host_camera()

    def still_off(kw):
        assert not e.get_color_grading(cam)[1], kw   # a refused desc leaves the setting as it was
        plan = api.StColorGradingPlan()
        assert e._b.color_grading_plan(C.byref(_d(**kw)), C.byref(plan)) == ST_ERR_INVALID_ARGUMENT, kw   # the plan call holds the same checks

    def plans(kw):
        assert e._b.color_grading_plan(C.byref(_d(**kw)), None) == ST_OK, kw

    A.argument_errors(e, cam, "camera_set_color_grading", "camera_get_color_grading", _d, BAD, GOOD, each_bad=still_off, each_good=plans)
    assert e._b.color_grading_plan(None, None) == ST_ERR_INVALID_ARGUMENT
    with pytest.raises(StrolleError):
        e.set_color_grading(cam, contrast=0.0)
    e.close()


def test_process_checks_its_arguments_and_needs_a_device():
    e, cam = _host_camera()
    b, h = e._b, e._h
    d = _d()
    fake = C.c_void_p(4096)   # never dereferenced: the checks and the missing device come first
    manual, auto = display_desc(tonemap=Tonemap.ACES_FITTED, exposure_ev=1.0), display_desc(auto_exposure=True)
    bad_display = display_desc(tonemap=Tonemap.REINHARD)
    bad_display.tonemap = 9

    def gp(desc=d, display=None, lut=None, n=0, src=fake, w=64, hh=48, dst=fake, fmt=0, engine=h):
        return b.color_grading_process(engine, C.byref(desc) if desc is not None else None, C.byref(display) if display is not None else None, lut, n, src, w, hh, dst,
                                       fmt, None)

    assert gp() == ST_ERR_NO_DEVICE and gp(display=manual) == ST_ERR_NO_DEVICE and gp(lut=fake, n=2) == ST_ERR_NO_DEVICE and gp(lut=fake, n=65) == ST_ERR_NO_DEVICE
    assert gp(n=99) == ST_ERR_NO_DEVICE   # without a table its side is not looked at
    assert gp(engine=None) == ST_ERR_INVALID_ARGUMENT
    for kw in (dict(desc=None), dict(src=None), dict(dst=None), dict(w=0), dict(hh=0), dict(w=16385), dict(hh=16385), dict(fmt=4), dict(fmt=-1), dict(display=auto),
               dict(display=bad_display), dict(desc=_d(struct_size=8)), dict(desc=_d(contrast=nan)), dict(desc=_d(lut_domain=3)), dict(lut=fake, n=1), dict(lut=fake, n=66),
               dict(lut=fake, n=0)):
        assert gp(**kw) == ST_ERR_INVALID_ARGUMENT, kw
    assert gp(w=16384, hh=1) == ST_ERR_NO_DEVICE
    with pytest.raises(StrolleError):
        e.color_grading_process(d, 4096, 64, 48, 4096)
    e.close()


def _values(d):
    return [list(getattr(d, f)) if hasattr(getattr(d, f), "__len__") else getattr(d, f) for f in FIELDS]


def test_set_get_clear_round_trips_and_survival_on_a_host_only_engine():
    e, cam = _host_camera()
    d0, on0 = e.get_color_grading(cam)
    assert not on0 and d0.struct_size == C.sizeof(api.StColorGradingDesc) and all(v == 0 or v == [0] * len(v) for v in _values(d0)[1:])
    want = _d(lut_domain=1)
    e.set_color_grading(cam, want)
    got, on = e.get_color_grading(cam)
    assert on and _values(got) == _values(want) and got.lut == 7
    e.tick()
    e.update_camera(cam, scenes.cornell_camera((80, 48)))   # a resize reallocates the camera: the setting stays
    got, on = e.get_color_grading(cam)
    assert on and _values(got) == _values(want)
    e.set_color_grading(cam, None)
    got, on = e.get_color_grading(cam)
    assert not on and got.contrast == F(1.2)   # the last desc stays readable
    e.set_color_grading(cam, saturation=0.5)
    got, on = e.get_color_grading(cam)
    assert on and got.saturation == 0.5 and got.contrast == 1.0 and got.flags == 0 and list(got.slope) == [1.0, 1.0, 1.0] and got.lut == 0 and got.lut_strength == 1.0
    e.set_color_grading(cam, _d(_pad_0=7, _pad_1=9))   # the pads are not kept
    got, _ = e.get_color_grading(cam)
    assert list(got._pad) == [0, 0]
    assert color_grading_desc(dither=True).flags == 1 and color_grading_plan(color_grading_desc())[0] == 0   # the defaults are neutral
    e.delete_camera(cam)
    e.close()


def test_grading_and_a_window_go_together_in_either_order_on_a_host_only_engine():
    e, cam = _host_camera()
    b, h = e._b, e._h
    d = _d()
    assert b.camera_set_window(h, cam, 0, 0, 32, 48) == ST_OK
    assert b.camera_set_color_grading(h, cam, C.byref(d)) == ST_OK               # the window came first
    assert e.get_color_grading(cam)[1]
    assert b.camera_set_window(h, cam, 16, 8, 64, 48) == ST_OK                   # grading came first
    assert b.camera_set_rows(h, cam, 0, 24) == ST_OK
    assert b.camera_set_window(h, cam, 0, 0, 0, 0) == ST_OK
    e.close()
    ranks = []   # st_dist_set_partition and st_dist_set_grid: two ranks through the in-process transport
    for r in range(2):
        e = Engine(device=-1)
        scenes.build_cornell(e)
        cam = e.create_camera(scenes.cornell_camera((64, 48)))
        e.dist_init_local(r, 2, 9292)
        ranks.append((e, cam))
    (e0, c0), (e1, c1) = ranks
    e0.set_color_grading(c0, d)                                                  # grading, then the tile
    e0.dist_set_partition(c0)
    e1.dist_set_grid(c1, dist_grid(64, 48, 2))                                   # the tile, then grading
    e1.set_color_grading(c1, d)
    for e, cam in ranks:
        assert e.get_color_grading(cam)[1]
        e.dist_shutdown(); e.close()


def test_the_plan_states_the_host_constants():
    steps, M, inv = color_grading_plan(color_grading_desc())
    assert steps == 0 and np.array_equal(M, np.eye(3, dtype=np.float32)) and inv == 0       # neutral: the matrix is reported inactive
    steps, M, inv = color_grading_plan(color_grading_desc(contrast=1.1, lut=3, dither=True))
    assert steps == R.CONTRAST | R.LUT | R.DITHER_STEP and np.array_equal(M, np.eye(3, dtype=np.float32))
    for t, u in ((0.35, -0.2), (-1.0, 1.0), (1.0, -1.0), (0.0, 0.5), (-0.25, 0.0), (1e-3, 0.0)):
        d = color_grading_desc(temperature=t, tint=u, lut_domain=LutDomain.LOG2, lut_ev_min=-12.5, lut_ev_max=4.25)
        steps, M, inv = color_grading_plan(d)
        want = R.white_balance_f64(t, u)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert steps == R.WHITE_BALANCE and (np.abs(M.astype(np.float64) - want) <= ulp).all(), (t, u, M, want)
        assert inv == F(1.0 / (4.25 + 12.5)) == R.inv_range(d)
        assert np.array_equal(M, want.astype(np.float32))   # the same operations in the same order: the same double, rounded once
    # a white point moved towards warm (t > 0) lifts blue against red in the correction, and the matrix keeps grey's luminance near 1
    _, M, _ = color_grading_plan(color_grading_desc(temperature=0.5))
    grey = M @ np.ones(3, np.float32)
    assert grey[0] > grey[2] and abs(float(R.display_ref.luma(*grey)) - 1.0) < 0.1


def test_lut_insert_and_remove_check_their_arguments():
    e, cam = _host_camera()
    b, h = e._b, e._h
    t2 = (C.c_float * 24)(*([0.5] * 24))
    assert b.lut_insert(h, 5, 2, t2) == ST_OK and b.lut_insert(h, 5, 2, t2) == ST_OK   # over a live id: replaced
    assert b.lut_insert(None, 5, 2, t2) == ST_ERR_INVALID_ARGUMENT and b.lut_insert(h, 5, 2, None) == ST_ERR_INVALID_ARGUMENT
    assert b.lut_insert(h, 0, 2, t2) == ST_ERR_INVALID_ARGUMENT                          # 0 is "none"
    for n in (0, 1, 66, 1000):
        assert b.lut_insert(h, 5, n, t2) == ST_ERR_INVALID_ARGUMENT, n
    for bad in (nan, inf, -inf):
        t = (C.c_float * 24)(*([0.5] * 23 + [bad]))
        assert b.lut_insert(h, 6, 2, t) == ST_ERR_INVALID_ARGUMENT, bad
    big = np.zeros((65, 65, 65, 3), np.float32)
    e.insert_lut(9, big)
    with pytest.raises(StrolleError):
        e.insert_lut(9, np.zeros((2, 2, 3, 3), np.float32))
    e.tick()                                                                             # a host-only engine drops the edits
    assert b.lut_remove(h, 5) == ST_OK and b.lut_remove(h, 12345) == ST_OK and b.lut_remove(None, 5) == ST_ERR_INVALID_ARGUMENT
    e.set_color_grading(cam, lut=5); e.set_color_grading(cam, lut=777)                   # a handle that names none is not an error
    e.tick()
    e.close()


# ---------------------------------------------------------------- st_decode_cube
def _cube_text(n, table=None, head="", eol="\n", sep=" ", domain=True):
    table = K.lut("random", n) if table is None else table
    lines = [head] if head else []
    lines += [f"LUT_3D_SIZE{sep}{n}"]
    if domain:
        lines += ["DOMAIN_MIN 0.0 0.0 0.0", f"DOMAIN_MAX{sep}1.0{sep}1.0 1"]
    lines += [sep.join(repr(float(v)) for v in row) for row in table.reshape(-1, 3)]
    return (eol.join(lines) + eol).encode()


def _decode_status(data, size_only=False):
    lib = api.load_library()
    fn = lib.st_decode_cube
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    n = C.c_uint32(99)
    out = (C.c_float * (66 ** 3 * 3))() if not size_only else None
    return fn(data, len(data), out, 0 if size_only else len(out), C.byref(n)), n.value


def test_decode_cube_reads_what_the_header_says():
    for n in (2, 5):
        table = K.lut("random", n)
        for text in (_cube_text(n, table), _cube_text(n, table, head='TITLE "a look"\n# made by hand\n\n   \t', eol="\r\n", sep="\t"), _cube_text(n, table, domain=False),
                     _cube_text(n, table)[:-1], b"\n\n#x\n" + _cube_text(n, table) + b"\n  \n# trailing comment\n"):
            got = decode_cube(text)
            assert got.shape == (n, n, n, 3) and np.array_equal(got, table), n    # repr round-trips a float32 through its double
            assert _decode_status(text, size_only=True) == (ST_OK, n)
    assert _decode_status(b"LUT_3D_SIZE 7\n", size_only=True) == (ST_OK, 7)                    # size-only mode does not read the rows
    assert _decode_status(b"# only\nLUT_3D_SIZE 65\n0 0 0\n", size_only=True) == (ST_OK, 65)
    lib = api.load_library()
    assert lib.st_decode_cube(None, 0, None, 0, None) == ST_ERR_INVALID_ARGUMENT
    small = (C.c_float * 3)()
    n = C.c_uint32()
    text = _cube_text(2)
    fn = lib.st_decode_cube
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    assert fn(text, len(text), small, 3, C.byref(n)) == ST_ERR_INVALID_ARGUMENT               # an output buffer too small


def test_decode_cube_refuses_what_it_does_not_read():
    ok = _cube_text(2)
    rows = ok.split(b"\n")
    parse = {
        "too few rows": b"\n".join(rows[:-2]) + b"\n", "too many rows": ok + b"0 0 0\n", "no size": b"TITLE \"x\"\n0 0 0\n", "empty": b"", "only comments": b"# a\n# b\n",
        "a non-number": ok.replace(rows[5], b"0.1 abc 0.3"), "two numbers": ok.replace(rows[5], b"0.1 0.2"), "four numbers": ok.replace(rows[5], b"0.1 0.2 0.3 0.4"),
        "nan": ok.replace(rows[5], b"0.1 nan 0.3"), "leading nan": ok.replace(rows[5], b"NaN 0.2 0.3"), "inf": ok.replace(rows[5], b"0.1 0.2 inf"),
        "-inf": ok.replace(rows[5], b"-inf 0.2 0.3"), "beyond float": ok.replace(rows[5], b"1e39 0.2 0.3"), "hex": ok.replace(rows[5], b"0x1p0 0.2 0.3"),
        "size 1": b"LUT_3D_SIZE 1\n0 0 0\n", "size 66": b"LUT_3D_SIZE 66\n", "size 0": b"LUT_3D_SIZE 0\n", "size -3": b"LUT_3D_SIZE -3\n", "size 2.5": b"LUT_3D_SIZE 2.5\n",
        "size missing": b"LUT_3D_SIZE\n", "size twice": b"LUT_3D_SIZE 2\n" + ok, "size words": b"LUT_3D_SIZE two\n", "bad domain line": b"DOMAIN_MIN 0 0\n" + ok,
        "a keyword inside the table": ok.replace(rows[5], b"TITLE \"late\""),
    }
    for what, text in parse.items():
        assert _decode_status(text)[0] == ST_ERR_PARSE, what
    unsupported = {
        "1-D": b"LUT_1D_SIZE 4\n0 0 0\n1 1 1\n", "1-D beside 3-D": b"LUT_1D_SIZE 4\n" + ok, "domain min": ok.replace(b"DOMAIN_MIN 0.0 0.0 0.0", b"DOMAIN_MIN 0.0 -1.0 0.0"),
        "domain max": b"DOMAIN_MAX 2 2 2\n" + _cube_text(2, domain=False), "input range": b"LUT_3D_INPUT_RANGE 0 1\n" + ok, "unknown keyword": b"SHAPER 1\n" + ok,
    }
    for what, text in unsupported.items():
        assert _decode_status(text)[0] == ST_ERR_UNSUPPORTED, what
    with pytest.raises(StrolleError):
        decode_cube(b"LUT_1D_SIZE 4\n")


FUZZ = r"""
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "st_cube.h"
// a fixed-seed set of mutated .cube texts through decode_cube, from buffers of exactly the text's size (so a read past the end is a report)
static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (uint32_t)(state >> 11); }
int main() {
    std::string base = "TITLE \"t\"\r\n# c\n\nLUT_3D_SIZE 3\nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 1 1 1\n";
    for (int i = 0; i < 27; i++) { char row[64]; std::snprintf(row, sizeof row, "%g\t%g %g\n", i / 26.0, 1.0 - i / 26.0, 0.5); base += row; }
    const char* bits[] = {"LUT_3D_SIZE 65\n", "LUT_1D_SIZE 2\n", "nan", "inf", "-", "1e999", "\r", "\n", "\t", "#", "DOMAIN_MAX 1 1", "LUT_3D_SIZE", "0x1p3", "TITLE", "\0x", "e", "."};
    int ok = 0, parse = 0, unsupported = 0;
    for (int round = 0; round < 4000; round++) {
        std::string s = base;
        const int edits = 1 + (int)(rnd() % 4u);
        for (int k = 0; k < edits; k++) {
            const size_t at = s.empty() ? 0 : rnd() % s.size();
            switch (rnd() % 5u) {
            case 0: if (!s.empty()) s[at] = (char)(rnd() & 0xffu); break;
            case 1: s.erase(at, rnd() % 40u); break;
            case 2: s.insert(at, bits[rnd() % (sizeof bits / sizeof bits[0])]); break;
            case 3: s.resize(at); break;
            default: s.insert(at, s.substr(rnd() % (s.size() + 1u), rnd() % 60u)); break;
            }
        }
        std::vector<uint8_t> exact(s.begin(), s.end());   // no terminator, no slack
        st::CubeLut lut;
        const st::CubeResult r = st::decode_cube(exact.data(), exact.size(), &lut, (round & 7) == 0, 0, 8, 9);
        if (r.status == 0) { ok++; if ((round & 7) != 0 && lut.rgb.size() != (size_t)lut.size * lut.size * lut.size * 3u) { std::puts("size mismatch"); return 1; } }
        else if (r.status == 8) parse++;
        else if (r.status == 9) unsupported++;
        else { std::puts("unknown status"); return 1; }
        if (lut.size != 0 && (lut.size < 2 || lut.size > 65)) { std::puts("side out of range"); return 1; }
    }
    st::CubeLut lut;
    if (st::decode_cube(nullptr, 0, &lut, false, 0, 8, 9).status != 8) { std::puts("empty input"); return 1; }
    if (st::decode_cube(reinterpret_cast<const uint8_t*>(base.data()), base.size(), &lut, false, 0, 8, 9).status != 0 || lut.size != 3) { std::puts("the base text"); return 1; }
    std::printf("ok %d %d %d\n", ok > 0, parse > 0, unsupported > 0);
    return 0;
}
"""


def test_decode_cube_survives_mutated_texts_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    src = tmp_path / "cube_fuzz.cpp"
    src.write_text(FUZZ)
    exe = tmp_path / "cube_fuzz"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "strolle_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok 1 1 1", run.stdout + run.stderr


# ---------------------------------------------------------------- grade_f32 at cases worked out by hand
def _px(rgba):
    return np.array([[rgba]], np.float32)


def _one(d, rgba, **kw):
    return R.grade_f32(_px(rgba), d, **kw)[0, 0]


def test_restatement_neutral_contrast_saturation_and_cdl_by_hand():
    poison = np.array((nan, -0.0, inf, 0.25), np.float32)
    for d in (color_grading_desc(), color_grading_desc(lut=9), color_grading_desc(lut_domain=LutDomain.LOG2, lut_strength=1.0)):   # (a handle without a table: skipped)
        assert np.array_equal(_one(d, poison).view(np.uint32), poison.view(np.uint32))         # neutral: the pixel's own bits, alpha too
    assert R.steps(color_grading_desc(), None) == 0
    # contrast about mid-grey: 0.18 is a fixed point (log2p(1) = 0, exp2p(0) = 1), and 0.36 goes to 0.18 * 2^c within the polynomials' error
    for c in (0.5, 1.3, 4.0):
        d = color_grading_desc(contrast=c)
        out = _one(d, (F(0.18), F(0.18), F(0.36), 0.5))
        assert out[0] == F(0.18) and out[1] == F(0.18) and out[3] == 1.0 and abs(float(out[2]) / (0.18 * 2.0 ** c) - 1) < 1e-6
    assert _one(color_grading_desc(contrast=2.0), (0.0, nan, -3.0, 1.0)).tolist() == [0.0, 0.0, 0.0, 1.0]    # pw(0) = 0; NaN and negatives are 0
    assert _one(color_grading_desc(contrast=0.999), (1e30, inf, 65504.0, 1.0))[0] == _one(color_grading_desc(contrast=0.999), (65504.0, 0, 0, 1.0))[0]   # held at 65504 first
    # saturation 0: Y in all channels; saturation 2 pushes a channel below Y to 0
    rgb = (F(0.5), F(0.25), F(1.0))
    y = F(0.2126) * rgb[0] + F(0.7152) * rgb[1] + F(0.0722) * rgb[2]
    assert _one(color_grading_desc(saturation=0.0), rgb + (0.3,)).tolist() == [y, y, y, 1.0]
    out = _one(color_grading_desc(saturation=4.0), rgb + (0.3,))
    assert out[1] == 0.0 and out[2] == y + (F(1.0) - y) * F(4.0)
    # the CDL at slope 2, offset -0.5, power 1: 2 v - 0.5 held at 0 from below, exact in float32
    d = color_grading_desc(slope=(2.0, 2.0, 2.0), offset=(-0.5, -0.5, -0.5))
    assert _one(d, (0.75, 0.25, 0.125, 0.0)).tolist() == [1.0, 0.0, 0.0, 1.0]
    assert _one(d, (0.5, 1.0, 4.0, 0.0)).tolist() == [0.5, 1.5, 7.5, 1.0]
    # power per channel: 0.25^0.5 = 0.5 within the polynomials' error, a channel at power 1 keeps its bits; then cdl_saturation 0 gives Y
    out = _one(color_grading_desc(power=(0.5, 1.0, 2.0)), (0.25, F(0.3), 3.0, 1.0))
    assert abs(float(out[0]) - 0.5) < 1e-6 and out[1] == F(0.3) and abs(float(out[2]) - 9.0) < 1e-5
    out = _one(color_grading_desc(cdl_saturation=0.0), rgb + (1.0,))
    assert out.tolist() == [y, y, y, 1.0]
    # the display sits between the two halves: Reinhard of 1 is 0.5, then the CDL doubles it
    assert _one(color_grading_desc(slope=(2.0, 2.0, 2.0)), (1.0, 3.0, 0.0, 1.0), tonemap=Tonemap.REINHARD, scale=1.0).tolist() == [1.0, 1.5, 0.0, 1.0]


def test_restatement_the_six_tetrahedra_and_the_tie_order():
    # a 2^3 table whose red channel is a different power of two at each corner [b, g, r]: every path t0 -> t1 -> t2 -> t3 sums differently
    t = np.zeros((2, 2, 2, 3), np.float32)
    for b in range(2):
        for g in range(2):
            for r in range(2):
                t[b, g, r] = 2.0 ** (4 * b + 2 * g + r)          # corners 1, 2, 4, 8, 16, 32, 64, 128 (high corner)
    d = color_grading_desc(lut=1)

    def expect(f, order):
        """by hand: walk the axes in `order` (0 = r, 1 = g, 2 = b)"""
        step = {0: 1, 1: 2, 2: 4}
        fa, fb, fc = (f[k] for k in order)
        e1 = step[order[0]]
        e2 = e1 + step[order[1]]
        return ((F(1) * (F(1) - F(fa)) + F(2.0 ** e1) * (F(fa) - F(fb))) + F(2.0 ** e2) * (F(fb) - F(fc))) + F(128.0) * F(fc)

    cases = {(0.75, 0.5, 0.25): (0, 1, 2), (0.75, 0.25, 0.5): (0, 2, 1), (0.5, 0.75, 0.25): (1, 0, 2), (0.25, 0.75, 0.5): (1, 2, 0), (0.5, 0.25, 0.75): (2, 0, 1),
             (0.25, 0.5, 0.75): (2, 1, 0),
             # ties go r, g, b
             (0.5, 0.5, 0.25): (0, 1, 2), (0.5, 0.25, 0.5): (0, 2, 1), (0.25, 0.5, 0.5): (1, 2, 0), (0.5, 0.5, 0.5): (0, 1, 2), (0.5, 0.5, 0.75): (2, 0, 1),
             (0.75, 0.5, 0.75): (0, 2, 1)}
    seen = set()
    for f, order in cases.items():
        got = _one(d, f + (1.0,), lut=t)[0]
        assert got == expect(f, order), (f, order, got)
        seen.add(float(got))
        for other in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
            if len(set(f)) == 3 and other != order:
                assert expect(f, other) != got, (f, other)    # each ordering gives a different answer
    assert len(seen) >= 10
    # the corners themselves, and beyond them: the coordinate is held to [0, 1], NaN is 0
    assert _one(d, (0.0, 0.0, 0.0, 1.0), lut=t)[0] == 1.0 and _one(d, (1.0, 1.0, 1.0, 1.0), lut=t)[0] == 128.0 and _one(d, (1.0, 0.0, 0.0, 1.0), lut=t)[0] == 2.0
    assert _one(d, (7.0, -3.0, nan, 1.0), lut=t)[0] == 2.0 and _one(d, (0.0, 1.0, 0.0, 0.0), lut=t).tolist()[::3] == [4.0, 1.0]
    # strength: 0 keeps v's value, 0.5 is the midpoint
    assert _one(color_grading_desc(lut=1, lut_strength=0.0), (1.0, 0.0, 0.0, 1.0), lut=t)[0] == 1.0
    assert _one(color_grading_desc(lut=1, lut_strength=0.5), (1.0, 0.0, 0.0, 1.0), lut=t)[0] == 1.5


def test_restatement_identity_tables_return_their_input():
    """p = u (N - 1) rounds once, f = p - i is exact, each weight rounds once and so does each of the three sums and four products: within
    8 ulp of 1 (the table's largest value) whatever the side"""
    rng = np.random.default_rng(3)
    img = np.concatenate([rng.random((40, 40, 3)).astype(np.float32), np.ones((40, 40, 1), np.float32)], -1)
    img[0, 0, :3] = (0.0, 1.0, 0.5)
    for n in (2, 3, 17):
        out = R.grade_f32(img, color_grading_desc(lut=1), lut=K.lut("identity", n))
        assert np.abs(out[..., :3].astype(np.float64) - img[..., :3]).max() <= 8 * 2.0 ** -24, n
        assert out[0, 0].tolist() == [0.0, 1.0, 0.5, 1.0]


def test_restatement_the_log2_domain_and_dither_by_hand():
    ramp = np.zeros((2, 2, 2, 3), np.float32)
    ramp[:, :, 1, 0] = 1.0; ramp[:, 1, :, 1] = 1.0; ramp[1, :, :, 2] = 1.0     # the identity at side 2: L = u
    d = color_grading_desc(lut=1, lut_domain=LutDomain.LOG2, lut_ev_min=-4.0, lut_ev_max=4.0)
    assert R.inv_range(d) == F(0.125)
    out = _one(d, (1.0, 4.0, 0.25, 1.0), lut=ramp)                              # lg = 0, 2, -2 -> u = 0.5, 0.75, 0.25, exactly
    assert out.tolist() == [0.5, 0.75, 0.25, 1.0]
    assert _one(d, (2.0 ** -4, 2.0 ** -9, 2.0 ** 4, 1.0), lut=ramp).tolist() == [0.0, 0.0, 1.0, 1.0]   # both clamps
    assert _one(d, (1e30, inf, 2.0 ** 5, 1.0), lut=ramp).tolist() == [1.0, 1.0, 1.0, 1.0]
    assert _one(d, (0.0, -2.0, nan, 1.0), lut=ramp).tolist() == [0.0, 0.0, 0.0, 1.0]                   # v <= 0 (and NaN): u = 0
    # dither: n = 171 x + 231 y; delta_k = (frac(n / q_k) - 0.5) / 255
    for (x, y), n in (((0, 0), 0), ((1, 0), 171), ((0, 1), 231), ((16383, 16383), 402 * 16383)):
        for k, q in enumerate((103, 71, 97)):
            want = (F(F(n) / F(q)) - np.floor(F(F(n) / F(q))) - F(0.5)) / F(255)
            got = R.dither_delta(x, y, k)
            # against the exact fraction: the float quotient is off by half an ulp of n / q at most (2^-9 at the far corner), the rest by an ulp of 1
            assert got == F(want) and abs(float(got) - ((n % q) / q - 0.5) / 255) <= (float(np.spacing(F(n / q))) / 2 + 2.0 ** -23) / 255, (x, y, k)
    assert R.dither_delta(0, 0, 0) == F(-0.5) / F(255) and R.dither_delta(1, 0, 0) == (F(F(171) / F(103)) - F(1) - F(0.5)) / F(255)
    assert 402 * 16383 < 2 ** 24                                                                        # exact in float
    dd = color_grading_desc(dither=True)
    a = R.grade_f32(np.full((1, 2, 4), 0.2, np.float32), dd, origin=(0, 0))
    b = R.grade_f32(np.full((1, 1, 4), 0.2, np.float32), dd, origin=(1, 0))
    assert np.array_equal(a[0, 1], b[0, 0]) and not np.array_equal(a[0, 0], a[0, 1])                   # frame coordinates, not the window's
    lo, hi = F(0.2) ** (1 / 2.2) - 0.5 / 255, F(0.2) ** (1 / 2.2) + 0.5 / 255
    assert (a[..., :3] >= lo ** 2.2 - 1e-6).all() and (a[..., :3] <= hi ** 2.2 + 1e-6).all() and (a[..., 3] == 1).all()
    assert _one(dd, (0.0, -1.0, nan, 0.5))[3] == 1.0 and (_one(dd, (0.0, -1.0, nan, 0.5))[:3] >= 0).all()


# ---------------------------------------------------------------- the restatement against the definition
def restatement_vs_definition():
    """the worst |grade_f32 - grade_f64| / max(1, the definition's largest channel of the pixel) over the whole input matrix on unspoiled
    inputs, every pixel counted; tools/grade_bench.py writes it to profiles/grading.json"""
    worst, where, pixels = 0.0, None, 0
    for name, size, kw, op in K.cases():
        d, table = K.build(kw)
        img = K.image(size, spoil=False)
        scale = R.display_ref.manual_scale(K.EV)
        a = R.grade_f32(img, d, op, scale, lut=table)
        b = R.grade_f64(img, d, op, scale, lut=table)
        assert np.isfinite(a).all(), f"{name}: a non-finite value from finite inputs"
        err = np.abs(a[..., :3].astype(np.float64) - b).max(-1) / np.maximum(1.0, np.abs(b).max(-1))
        pixels += err.size
        if err.max() > worst:
            worst, where = float(err.max()), name
    return worst, where, pixels


def test_restatement_agrees_with_the_float64_definition():
    """The bound is four times the deviation recorded in profiles/grading.json (restatement_vs_definition), the project's usual margin,
    which leaves room for another libm; the GPU test holds both builds to the definition within the same bound."""
    recorded = json.load(open(os.path.join(ROOT, "profiles", "grading.json")))["restatement_vs_definition"]["worst"]
    worst, where, pixels = restatement_vs_definition()
    print(f"restatement against the definition: worst {worst:.3e} at {where} over {pixels} pixels; recorded {recorded:.3e}, bound {4 * recorded:.3e}")
    assert pixels > 50000 and 0 < recorded < 1e-4
    assert worst <= 4 * recorded, (worst, where)
