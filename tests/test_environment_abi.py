"""CPU tests of environment lighting (include/strolle_hip.h "environment lighting"): the entry points are exported, declared and bound by
the Rust facade, StEnvironmentDesc has the header's layout, every argument error occurs on a host-only engine, and st_decode_hdr reads
files a numpy RGBE writer produced (env_ref.py) bit for bit."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from env_ref import random_rgbe, rgbe_to_float, write_hdr
from strolle_amd import Engine, StrolleError, decode_hdr, load_hdr
from strolle_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_OK, ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE, ST_ERR_PARSE, ST_ERR_UNSUPPORTED = 0, 1, 2, 8, 9
ENTRY_POINTS = ("st_environment_set", "st_environment_set_device", "st_environment_update", "st_environment_clear", "st_decode_hdr",
                "st_debug_environment_eval", "st_debug_environment_sample", "st_debug_environment_pdf")


def test_entry_points_are_exported_declared_and_bound():
    lib = api.load_library()
    header = open(os.path.join(ROOT, "include", "strolle_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "strolle-hip", "src", "ffi.rs")).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, ffi), name
    c_body = re.search(r"typedef struct StEnvironmentDesc \{(.*?)\} StEnvironmentDesc;", re.sub(r"/\*.*?\*/", "", header, flags=re.S), re.S).group(1)
    c_fields = [d.strip().split()[-1] for d in c_body.split(";") if d.strip()]
    r_fields = re.findall(r"pub (\w+):", re.search(r"pub struct StEnvironmentDesc \{(.*?)\n\}", ffi, re.S).group(1))
    assert c_fields == r_fields == [f for f, _ in api.StEnvironmentDesc._fields_] == ["struct_size", "flags", "intensity", "yaw"]


def test_desc_layout_agrees_between_c_and_ctypes(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "strolle_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d %d\\n", '
                   'sizeof(StEnvironmentDesc), offsetof(StEnvironmentDesc, struct_size), offsetof(StEnvironmentDesc, flags), '
                   'offsetof(StEnvironmentDesc, intensity), offsetof(StEnvironmentDesc, yaw), ST_ENV_KEEP_SUN, ST_ENV_UNIFORM_SAMPLING); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    D = api.StEnvironmentDesc
    assert got == [16, 0, 4, 8, 12, 1, 2]
    assert got[:5] == [C.sizeof(D), D.struct_size.offset, D.flags.offset, D.intensity.offset, D.yaw.offset]
    assert got[5:] == [api.ENV_KEEP_SUN, api.ENV_UNIFORM_SAMPLING]


def _desc(**kw):
    d = api.environment_desc()
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_errors_on_a_host_only_engine():
    e = Engine(device=-1)
    b, h = e._b, e._h
    tex = np.ones((8, 16, 3), np.float32)
    ok = _desc()
    P = tex.ctypes.data

    def st(t=P, w=16, hh=8, ch=3, d=ok, engine=h):
        return b.environment_set(engine, t, w, hh, ch, C.byref(d) if d is not None else None)

    assert st() == ST_OK                                                   # a host-only engine validates and stores
    assert st(engine=None) == ST_ERR_INVALID_ARGUMENT                      # null pointers
    assert st(t=None) == ST_ERR_INVALID_ARGUMENT
    assert st(d=None) == ST_ERR_INVALID_ARGUMENT
    for w, hh in ((0, 8), (16, 0), (16385, 1), (1, 16385)):                # a side outside 1..16384
        assert st(w=w, hh=hh) == ST_ERR_INVALID_ARGUMENT, (w, hh)
    big = np.zeros(3, np.float32)   # (never read: the size check comes first)
    assert st(t=big.ctypes.data, w=16384, hh=2049) == ST_ERR_INVALID_ARGUMENT   # width x height > 2^25
    for ch in (0, 1, 2, 5):
        assert st(ch=ch) == ST_ERR_INVALID_ARGUMENT, ch
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):          # a negative or non-finite texel
        t = tex.copy(); t[3, 5, 1] = bad
        assert st(t=t.ctypes.data) == ST_ERR_INVALID_ARGUMENT, bad
    t4 = np.ones((8, 16, 4), np.float32); t4[..., 3] = float("nan")         # alpha is ignored
    assert st(t=t4.ctypes.data, ch=4) == ST_OK
    for d in (_desc(struct_size=12), _desc(struct_size=20), _desc(flags=4), _desc(flags=0x80000000), _desc(intensity=-0.5),
              _desc(intensity=float("nan")), _desc(intensity=float("inf")), _desc(yaw=float("nan")), _desc(yaw=float("inf"))):
        assert st(d=d) == ST_ERR_INVALID_ARGUMENT, (d.struct_size, d.flags, d.intensity, d.yaw)
        assert b.environment_update(h, C.byref(d)) == ST_ERR_INVALID_ARGUMENT
    assert b.environment_update(h, C.byref(_desc(flags=3, intensity=2.0, yaw=-1.0))) == ST_OK
    assert b.environment_update(h, None) == ST_ERR_INVALID_ARGUMENT
    assert b.environment_clear(h) == ST_OK and b.environment_clear(None) == ST_ERR_INVALID_ARGUMENT
    # the device variant and the debug seams need a device
    assert b.environment_set_device(h, P, 16, 8, 3, 0, C.byref(ok)) == ST_ERR_NO_DEVICE
    assert b.environment_set_device(h, P, 16, 8, 3, 16 * 3 * 4 - 4, C.byref(ok)) == ST_ERR_INVALID_ARGUMENT   # a pitch shorter than a row
    assert b.environment_set_device(h, P, 16, 8, 3, 16 * 3 * 4 + 2, C.byref(ok)) == ST_ERR_INVALID_ARGUMENT   # not a multiple of 4
    assert b.environment_set_device(h, None, 16, 8, 3, 0, C.byref(ok)) == ST_ERR_INVALID_ARGUMENT
    for fn in (b.debug_environment_eval, b.debug_environment_sample, b.debug_environment_pdf):
        assert fn(h, P, 4, P, None) == ST_ERR_NO_DEVICE
    # the facade: set, tick (light 0 follows on the host), update, clear
    e.set_environment(tex, intensity=2.0, yaw=0.5)
    e.tick()
    e.update_environment(intensity=0.5, keep_sun=True)
    e.clear_environment()
    e.tick()
    with pytest.raises(StrolleError):
        e.set_environment(-tex)
    e.close()


def _decode(data: bytes):
    lib = api.load_library()
    w, h = C.c_uint32(), C.c_uint32()
    st = lib.st_decode_hdr(data, len(data), None, 0, C.byref(w), C.byref(h))
    return st, w.value, h.value


@pytest.mark.parametrize("w", [1, 7, 8, 9, 31, 64, 127, 128, 129, 300])
def test_decode_matches_the_numpy_formula(w):
    rng = np.random.default_rng(w)
    h = 5
    px = random_rgbe(rng, h, w)
    want = rgbe_to_float(px)
    for rle in (True, False):
        data = write_hdr(px, rle=rle)
        got = decode_hdr(data)
        assert got.shape == (h, w, 3) and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (w, rle)
    if w >= 8:   # the writer really produced runs and literals
        data = write_hdr(px, rle=True)
        assert len(data) < len(write_hdr(px, rle=False))


def test_decode_header_variants_and_load_hdr(tmp_path):
    rng = np.random.default_rng(7)
    px = random_rgbe(rng, 3, 20)
    want = rgbe_to_float(px)
    for magic, extra in (("#?RGBE", ()), ("#?RADIANCE", ("EXPOSURE=0.25", "GAMMA=2.2", "SOFTWARE=x", "# comment"))):
        got = decode_hdr(write_hdr(px, magic=magic, extra_header=extra))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), magic
    p = tmp_path / "map.hdr"
    p.write_bytes(write_hdr(px))
    assert np.array_equal(load_hdr(str(p)), want)
    # a zero exponent is 0 whatever the mantissas, the smallest exponents give float32 denormals as the formula does
    z = np.array([[[255, 7, 1, 0], [255, 255, 255, 1], [128, 64, 2, 9], [1, 0, 0, 136], [255, 1, 0, 255]]], np.uint8)
    got = decode_hdr(write_hdr(z, rle=False))
    assert np.array_equal(got.view(np.uint32), rgbe_to_float(z).view(np.uint32))
    assert got[0, 0].tolist() == [0.0, 0.0, 0.0] and got[0, 3, 0] == 1.0


def test_decode_errors():
    rng = np.random.default_rng(3)
    px = random_rgbe(rng, 4, 40)
    good = write_hdr(px)
    assert _decode(good) == (ST_OK, 40, 4)
    head_end = good.index(b"-Y 4 +X 40\n") + len(b"-Y 4 +X 40\n")
    for cut in (0, 5, head_end - 3, head_end, head_end + 2, head_end + 10, len(good) - 1):   # truncations
        data = good[:cut]
        st = api.load_library().st_decode_hdr
        w, h = C.c_uint32(), C.c_uint32()
        out = np.zeros(40 * 4 * 3, np.float32)
        assert st(data, len(data), out.ctypes.data, out.size, C.byref(w), C.byref(h)) == ST_ERR_PARSE, cut
    flat = write_hdr(px, rle=False)
    assert api.load_library().st_decode_hdr(flat[:-1], len(flat) - 1, np.zeros(480, np.float32).ctypes.data, 480, C.byref(C.c_uint32()), C.byref(C.c_uint32())) == ST_ERR_PARSE
    assert _decode(b"P6\n1 1\n255\n\0\0\0")[0] == ST_ERR_PARSE                        # not an hdr file
    assert _decode(write_hdr(px, resolution="-Y 4 +X oops"))[0] == ST_ERR_PARSE
    for res in ("+Y 4 +X 40", "-Y 4 -X 40", "+X 40 -Y 4"):                             # other orientations
        assert _decode(write_hdr(px, resolution=res))[0] == ST_ERR_UNSUPPORTED, res
    assert _decode(write_hdr(px, fmt="32-bit_rle_xyze"))[0] == ST_ERR_UNSUPPORTED
    old = px.copy(); old[1, 3] = (1, 1, 1, 5)                                            # an old-style run marker
    data = write_hdr(old, rle=False)
    out = np.zeros(480, np.float32)
    assert api.load_library().st_decode_hdr(data, len(data), out.ctypes.data, out.size, C.byref(C.c_uint32()), C.byref(C.c_uint32())) == ST_ERR_UNSUPPORTED
    # a new-style scanline whose width disagrees, and a run that overruns its scanline
    bad = bytearray(good); i = head_end
    bad[i + 3] = 41
    assert api.load_library().st_decode_hdr(bytes(bad), len(bad), out.ctypes.data, out.size, C.byref(C.c_uint32()), C.byref(C.c_uint32())) == ST_ERR_PARSE
    bad = bytearray(good[:head_end]) + bytes([2, 2, 0, 40, 128 + 41, 7]) + good[head_end + 6:]
    assert api.load_library().st_decode_hdr(bytes(bad), len(bad), out.ctypes.data, out.size, C.byref(C.c_uint32()), C.byref(C.c_uint32())) == ST_ERR_PARSE
    with pytest.raises(StrolleError):
        decode_hdr(good[:-2])
    # a resolution the bytes cannot hold is refused before anything is allocated (also by the size query), and so is one beyond 2^26 texels
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n"
    assert _decode(head + b"-Y 16384 +X 16384\n" + bytes(64))[0] == ST_ERR_UNSUPPORTED
    assert _decode(head + b"-Y 8192 +X 8192\n" + bytes(64))[0] == ST_ERR_PARSE
    assert _decode(head + b"-Y 2 +X 4\n" + bytes(31))[0] == ST_ERR_PARSE   # flat: 4 bytes per texel
    assert _decode(head + b"-Y 2 +X 4\n" + bytes(32))[0] == ST_OK
