"""CPU tests of the per-pixel AOV boundary (include/strolle_hip.h "per-pixel AOVs"): StAovTargets has the same layout in C and ctypes, the
plane element types of api.py are the header's, the entry point is exported, and its argument checks answer on a host-only engine."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from strolle_amd import Aov, Engine, StrolleError, scenes
from strolle_amd import api
from strolle_amd.api import load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_OK, ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE, ST_ERR_UNKNOWN_CAMERA = 0, 1, 2, 3

C_PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "strolle_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu\n", sizeof(StAovTargets), offsetof(StAovTargets, struct_size), offsetof(StAovTargets, _pad), offsetof(StAovTargets, planes));
    printf("%d %d %d %d %d %d %d\n", (int)ST_AOV_DEPTH, (int)ST_AOV_NORMAL, (int)ST_AOV_ALBEDO, (int)ST_AOV_MOTION, (int)ST_AOV_INSTANCE,
           (int)ST_AOV_TRIANGLE, (int)ST_AOV_COUNT);
    return 0;
}
"""


def test_layout_agrees_between_c_and_ctypes(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "layout.c"
    src.write_text(C_PROGRAM)
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    layout, kinds = [list(map(int, l.split())) for l in lines[:2]]
    assert layout == [56, 0, 4, 8]
    assert layout == [C.sizeof(api.StAovTargets), api.StAovTargets.struct_size.offset, api.StAovTargets._pad.offset, api.StAovTargets.planes.offset]
    assert kinds == [int(k) for k in Aov] + [api.AOV_COUNT]


def test_plane_element_types_match_the_header():
    # the element type each StAovKind comment of the header names
    want = {Aov.DEPTH: ("float32", 1), Aov.NORMAL: ("float32", 4), Aov.ALBEDO: ("float32", 4), Aov.MOTION: ("float32", 2),
            Aov.INSTANCE: ("uint64", 1), Aov.TRIANGLE: ("uint32", 1)}
    assert {k: (np.dtype(s).name, n) for k, (s, n) in api.AOV_ELEMENT.items()} == want
    header = open(os.path.join(ROOT, "include", "strolle_hip.h")).read()
    for k, (scalar, n) in want.items():
        tag = {"float32": "f32", "uint64": "u64", "uint32": "u32"}[scalar] + (f"x{n}" if n > 1 else "")
        line = next(l for l in header.splitlines() if f"ST_AOV_{k.name} = {int(k)}," in l)
        assert f"/* {tag}:" in line, line
    torch = pytest.importorskip("torch")
    planes = api.aov_planes((8, 4), device="cpu", fill=0)
    for k, t in planes.items():
        scalar, n = api.AOV_ELEMENT[k]
        assert t.element_size() == np.dtype(scalar).itemsize and t.numel() == 8 * 4 * n and t.is_contiguous()
        assert t.shape[:2] == (4, 8)
    assert planes[Aov.INSTANCE].dtype == torch.uint64 and planes[Aov.TRIANGLE].dtype == torch.uint32


def test_entry_point_is_exported():
    assert hasattr(load_library(), "st_camera_render_aovs")


@pytest.fixture()
def host_engine():
    e = Engine(device=-1)
    scenes.build_cornell(e)
    e.tick()
    yield e
    e.close()


def _targets(planes=None, struct_size=None):
    t = api.StAovTargets()
    t.struct_size = C.sizeof(api.StAovTargets) if struct_size is None else struct_size
    for k, v in (planes or {}).items():
        t.planes[int(k)] = v
    return t


def test_host_only_engine_has_no_device(host_engine):
    e = host_engine
    cam = e.create_camera(scenes.cornell_camera((32, 32)))
    buf = np.zeros(32 * 32, np.float32)
    assert e._b.camera_render_aovs(e._h, cam, C.byref(_targets({Aov.DEPTH: buf.ctypes.data})), None) == ST_ERR_NO_DEVICE
    with pytest.raises(StrolleError):
        e.render_aovs(cam, {Aov.DEPTH: buf.ctypes.data})


def test_argument_checks_come_before_the_device(host_engine):
    e = host_engine
    cam = e.create_camera(scenes.cornell_camera((32, 32)))
    buf = np.zeros(32 * 32 * 4, np.float32)
    ok = _targets({Aov.NORMAL: buf.ctypes.data})
    call = e._b.camera_render_aovs
    assert call(None, cam, C.byref(ok), None) == ST_ERR_INVALID_ARGUMENT                      # null engine
    assert call(e._h, cam, None, None) == ST_ERR_INVALID_ARGUMENT                             # null targets
    for bad in (0, 48, 55, 57, 64, 0xFFFFFFFF):                                               # wrong struct_size
        assert call(e._h, cam, C.byref(_targets({Aov.NORMAL: buf.ctypes.data}, bad)), None) == ST_ERR_INVALID_ARGUMENT
    assert call(e._h, cam, C.byref(_targets()), None) == ST_ERR_INVALID_ARGUMENT              # no plane requested
    assert call(e._h, cam + 1000, C.byref(ok), None) == ST_ERR_UNKNOWN_CAMERA                 # an unknown camera
    assert call(e._h, cam + 1000, C.byref(_targets()), None) == ST_ERR_INVALID_ARGUMENT       # the argument checks come first
    with pytest.raises(StrolleError):
        e.render_aovs(cam, {})
    with pytest.raises(StrolleError):
        e.render_aovs(cam + 1000, {Aov.NORMAL: buf.ctypes.data})
