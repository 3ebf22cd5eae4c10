"""CPU tests of the scene-query boundary (include/strolle_hip.h "scene queries"): the structs' layout is the same in C, ctypes and
numpy, the entry points are exported, and their argument checks answer on a host-only engine (no GPU is touched)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from strolle_amd import Engine, StrolleError, scenes
from strolle_amd import api
from strolle_amd.api import load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("st_scene_trace_rays", "st_scene_occluded", "st_camera_pick", "st_scene_trace_rays_host")
ST_OK, ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE, ST_ERR_UNKNOWN_CAMERA = 0, 1, 2, 3

C_PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "strolle_hip.h"
int main(void) {
    printf("%zu %zu\n", sizeof(StRay), sizeof(StRayHit));
    printf("%zu %zu %zu\n", offsetof(StRay, t_max), offsetof(StRay, direction), offsetof(StRay, _pad));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(StRayHit, t), offsetof(StRayHit, normal), offsetof(StRayHit, triangle),
           offsetof(StRayHit, uv), offsetof(StRayHit, barycentric), offsetof(StRayHit, instance), offsetof(StRayHit, hit), offsetof(StRayHit, _pad));
    printf("%d\n", (int)ST_RAY_COHERENT);
    return 0;
}
"""


def test_layouts_agree_between_c_ctypes_and_numpy(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "layout.c"
    src.write_text(C_PROGRAM)
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    sizes, ray_off, hit_off, coherent = [list(map(int, l.split())) for l in lines[:4]]
    assert sizes == [32, 64]
    assert sizes == [C.sizeof(api.StRay), C.sizeof(api.StRayHit)] == [api.RAY_DTYPE.itemsize, api.HIT_DTYPE.itemsize]
    assert ray_off == [api.StRay.t_max.offset, api.StRay.direction.offset, api.StRay._pad.offset]
    assert ray_off == [api.RAY_DTYPE.fields[f][1] for f in ("t_max", "direction", "_pad")]
    names = ("t", "normal", "triangle", "uv", "barycentric", "instance", "hit", "_pad")
    assert hit_off == [getattr(api.StRayHit, f).offset for f in names]
    assert hit_off == [api.HIT_DTYPE.fields[f][1] for f in names]
    assert coherent == [api.RAY_COHERENT]


def test_entry_points_are_exported():
    lib = load_library()
    assert [s for s in ENTRY_POINTS if not hasattr(lib, s)] == []


@pytest.fixture()
def host_engine():
    e = Engine(device=-1)
    scenes.build_cornell(e)
    e.tick()
    yield e
    e.close()


def _raw(e, name):
    return getattr(e._b, name)


def test_host_only_engine_has_no_device_for_any_query(host_engine):
    e = host_engine
    rays = np.zeros(4, api.RAY_DTYPE); hits = np.zeros(4, api.HIT_DTYPE); occ = np.zeros(4, np.uint32); px = np.zeros(8, np.uint32)
    cam = e.create_camera(scenes.cornell_camera((32, 32)))
    assert _raw(e, "scene_trace_rays")(e._h, rays.ctypes.data, 4, hits.ctypes.data, 0, None) == ST_ERR_NO_DEVICE
    assert _raw(e, "scene_occluded")(e._h, rays.ctypes.data, 4, occ.ctypes.data, None) == ST_ERR_NO_DEVICE
    assert _raw(e, "camera_pick")(e._h, cam, px.ctypes.data, 4, hits.ctypes.data, None) == ST_ERR_NO_DEVICE
    assert _raw(e, "scene_trace_rays_host")(e._h, rays.ctypes.data, 4, hits.ctypes.data) == ST_ERR_NO_DEVICE
    with pytest.raises(StrolleError):
        e.trace_rays_host(rays)
    with pytest.raises(StrolleError):
        e.trace_rays(rays.ctypes.data, 4, hits.ctypes.data)


def test_argument_checks_come_before_the_device(host_engine):
    e = host_engine
    rays = np.zeros(4, api.RAY_DTYPE); hits = np.zeros(4, api.HIT_DTYPE); px = np.zeros(8, np.uint32)
    cam = e.create_camera(scenes.cornell_camera((32, 32)))
    # count == 0: a no-op, null pointers included
    assert _raw(e, "scene_trace_rays")(e._h, None, 0, None, 0, None) == ST_OK
    assert _raw(e, "scene_trace_rays")(e._h, None, 0, None, api.RAY_COHERENT, None) == ST_OK
    assert _raw(e, "scene_occluded")(e._h, None, 0, None, None) == ST_OK
    assert _raw(e, "camera_pick")(e._h, cam, None, 0, None, None) == ST_OK
    assert _raw(e, "scene_trace_rays_host")(e._h, None, 0, None) == ST_OK
    assert e.trace_rays_host(np.zeros(0, api.RAY_DTYPE)).shape == (0,)
    # null pointers with count > 0
    assert _raw(e, "scene_trace_rays")(e._h, None, 4, hits.ctypes.data, 0, None) == ST_ERR_INVALID_ARGUMENT
    assert _raw(e, "scene_trace_rays")(e._h, rays.ctypes.data, 4, None, 0, None) == ST_ERR_INVALID_ARGUMENT
    assert _raw(e, "scene_occluded")(e._h, rays.ctypes.data, 4, None, None) == ST_ERR_INVALID_ARGUMENT
    assert _raw(e, "camera_pick")(e._h, cam, None, 4, hits.ctypes.data, None) == ST_ERR_INVALID_ARGUMENT
    assert _raw(e, "scene_trace_rays_host")(e._h, rays.ctypes.data, 4, None) == ST_ERR_INVALID_ARGUMENT
    assert _raw(e, "scene_trace_rays")(None, rays.ctypes.data, 4, hits.ctypes.data, 0, None) == ST_ERR_INVALID_ARGUMENT
    # unknown flag bits, whatever the count
    for bad in (2, 0x80000000, 3):
        assert _raw(e, "scene_trace_rays")(e._h, rays.ctypes.data, 4, hits.ctypes.data, bad, None) == ST_ERR_INVALID_ARGUMENT
        assert _raw(e, "scene_trace_rays")(e._h, None, 0, None, bad, None) == ST_ERR_INVALID_ARGUMENT
    # an unknown camera
    assert _raw(e, "camera_pick")(e._h, cam + 1000, px.ctypes.data, 4, hits.ctypes.data, None) == ST_ERR_UNKNOWN_CAMERA
