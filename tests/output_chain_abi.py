"""What the CPU tests of the output nodes' C ABI share (test_fog_abi, _shafts_abi, _dof_abi, _motion_blur_abi, _bloom_abi, _post_abi,
_display_abi): the agreement of exports, header and ffi.rs, the C layout program, the host-only camera, the argument-error loop over a
node's BAD and GOOD descriptors, and the sequence in which a node and a window exclude each other. The test functions, their BAD / GOOD
tables, their expected sizeof / offset lists and the hand-worked restatement cases stay in the node's own file. A plain module."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from strolle_amd import Engine, api, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_OK, ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE, ST_ERR_UNKNOWN_CAMERA = 0, 1, 2, 3


def exports_header_and_ffi_agree(struct, fields, entry_points, constants=()):
    """Every entry point is exported by the library, declared in the header and bound in ffi.rs; `struct` has `fields`, in that order, in
    the header, in ffi.rs and in api.py (an array field counts by its name); every (C name, value) of `constants` stands in the header and
    in ffi.rs. Returns (header, ffi) for what a node checks beyond that."""
    lib = api.load_library()
    header = open(os.path.join(ROOT, "include", "strolle_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "strolle-hip", "src", "ffi.rs")).read()
    for name in entry_points:
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, ffi), name
    c_body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), re.sub(r"/\*.*?\*/", "", header, flags=re.S), re.S).group(1)
    c_fields = [re.sub(r"\[\d+\]", "", n.strip()) for d in c_body.split(";") if d.strip() for n in d.strip().split(None, 1)[1].split(",")]
    r_fields = re.findall(r"pub (\w+):", re.search(r"pub struct %s \{(.*?)\n\}" % struct, ffi, re.S).group(1))
    assert c_fields == r_fields == [f for f, _ in getattr(api, struct)._fields_] == list(fields)
    for name, value in constants:
        assert re.search(r"\b%s = %d\b" % (name, value), header), name
        assert "pub const %s: u32 = %d;" % (name, value) in ffi, name
    return header, ffi


def c_layout(tmp_path, struct, fields, constants=()):
    """sizeof, every field's offset and the named constants as a C compiler sees them: [sizeof] + offsets + constants. The sizeof and
    offsets are held to ctypes' here; the caller holds the whole list to its literal one."""
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "layout.c"
    offs = ", ".join("offsetof(%s, %s)" % (struct, f) for f in fields)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "strolle_hip.h"\nint main(void) { printf("%zu' + " %zu" * len(fields) + " %d" * len(constants)
                   + '\\n", sizeof(%s), ' % struct + ", ".join([offs] + list(constants)) + "); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    D = getattr(api, struct)
    assert got[:1 + len(fields)] == [C.sizeof(D)] + [getattr(D, f).offset for f in fields]
    return got


def host_camera(size=(64, 48)):
    e = Engine(device=-1)
    scenes.build_cornell(e)
    return e, e.create_camera(scenes.cornell_camera(size))


def argument_errors(e, cam, setter, getter, make, bad, good, each_bad=None, each_good=None):
    """st_camera_set_<node> and st_camera_get_<node> (`setter`, `getter`: the binding's names) on a host-only engine: null engine, unknown
    camera, every descriptor of `bad` refused and every one of `good` taken; `make(**kw)` builds a descriptor. each_bad(kw) / each_good(kw)
    run behind each descriptor for what a node checks besides (its plan call, the setting a refusal leaves)."""
    b, h = e._b, e._h

    def st(d, camera=cam, engine=h):
        return getattr(b, setter)(engine, camera, C.byref(d) if d is not None else None)

    assert st(make()) == ST_OK and st(None) == ST_OK
    assert st(make(), engine=None) == ST_ERR_INVALID_ARGUMENT
    assert st(make(), camera=cam + 99) == ST_ERR_UNKNOWN_CAMERA and st(None, camera=cam + 99) == ST_ERR_UNKNOWN_CAMERA
    for kw in bad:
        assert st(make(**kw)) == ST_ERR_INVALID_ARGUMENT, kw
        if each_bad:
            each_bad(kw)
    for kw in good:
        assert st(make(**kw)) == ST_OK, kw
        if each_good:
            each_good(kw)
    assert getattr(b, getter)(h, cam, None, None) == ST_OK
    assert getattr(b, getter)(h, cam + 99, None, None) == ST_ERR_UNKNOWN_CAMERA
    assert getattr(b, getter)(None, cam, None, None) == ST_ERR_INVALID_ARGUMENT


def node_and_window_exclude_each_other(e, cam, setter, d, is_on):
    """A window, then the node: refused, and the node stays off. The node, then any of the window setters: refused, except the whole
    frame, which is no tile. Turning the node off is always fine and makes windows work again. `is_on()` reads the setting back."""
    b, h = e._b, e._h
    set_node = getattr(b, setter)
    assert b.camera_set_window(h, cam, 0, 0, 32, 48) == ST_OK
    assert set_node(h, cam, C.byref(d)) == ST_ERR_INVALID_ARGUMENT               # the window came first
    assert not is_on()
    assert set_node(h, cam, None) == ST_OK                                       # turning it off is always fine
    assert b.camera_set_window(h, cam, 0, 0, 0, 0) == ST_OK                      # back to the whole frame
    assert set_node(h, cam, C.byref(d)) == ST_OK
    assert b.camera_set_window(h, cam, 16, 0, 64, 48) == ST_ERR_INVALID_ARGUMENT   # the node came first
    assert b.camera_set_window(h, cam, 0, 8, 64, 48) == ST_ERR_INVALID_ARGUMENT
    assert b.camera_set_rows(h, cam, 0, 24) == ST_ERR_INVALID_ARGUMENT
    assert b.camera_set_window(h, cam, 0, 0, 64, 48) == ST_OK                    # the whole frame is no tile
    assert set_node(h, cam, None) == ST_OK
    assert b.camera_set_window(h, cam, 16, 0, 64, 48) == ST_OK                   # off: windows work again
