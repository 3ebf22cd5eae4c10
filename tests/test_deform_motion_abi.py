"""CPU tests of the deformation-motion boundary (include/strolle_hip.h "skinned meshes", st_engine_set_deformation_motion): the three
entry points are exported and declared in the Rust facade and in api.py, the switch round-trips on a host-only engine, and the numpy
restatement (tests/deform_ref.py) gives two hand-computed answers."""
import ctypes as C
import os
import re

import numpy as np

import deform_ref
from strolle_amd import Camera, Engine
from strolle_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE = 1, 2
SYMBOLS = ("st_engine_set_deformation_motion", "st_engine_get_deformation_motion", "st_debug_deformation")


def test_entry_points_are_exported_and_declared_everywhere():
    lib = api.load_library()
    header = open(os.path.join(ROOT, "include", "strolle_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "strolle-hip", "src", "ffi.rs")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(StEngine\*" % name, header), f"{name} is not declared in the header"
        assert re.search(r"pub fn %s\(" % name, ffi), f"{name} is not declared in the Rust binding"
    assert "fn set_deformation_motion" in open(os.path.join(ROOT, "rust", "strolle-hip", "src", "lib.rs")).read()
    for method in ("set_deformation_motion", "deformation_motion", "deformation_stats"):
        assert hasattr(Engine, method), method
    assert "Limitation: the velocity plane" not in header, "the header still states the limitation this switch lifts"


def test_switch_round_trips_on_a_host_only_engine():
    e = Engine(device=-1)
    try:
        assert e.deformation_motion is False, "deformation motion must be off by default"
        e.set_deformation_motion(True)
        assert e.deformation_motion is True
        e.tick()                                   # host work only: a host-only engine ticks with the switch on
        assert e.deformation_motion is True
        e.set_deformation_motion(False)
        assert e.deformation_motion is False
        assert e._b.engine_get_deformation_motion(e._h, None) == ST_ERR_INVALID_ARGUMENT
        n, b = C.c_uint64(), C.c_uint64()
        assert e._b.debug_deformation(e._h, C.byref(n), C.byref(b)) == ST_ERR_NO_DEVICE
        assert e._b.debug_deformation(e._h, None, C.byref(b)) == ST_ERR_INVALID_ARGUMENT
        assert e._b.debug_deformation(e._h, C.byref(n), None) == ST_ERR_INVALID_ARGUMENT
    finally:
        e.close()


def _translated(x, size=(100, 50)):
    t = np.eye(4, dtype=np.float32); t[0, 3] = x
    return Camera(size=size, transform=t, projection=np.eye(4, dtype=np.float32))


def test_reference_identity_cameras_that_differ_by_a_translation():
    """Identity projection: ndc = camera-space xy. Point (0.2, 0.4, 0): ndc (0.2, -0.4 after the flip) -> ((0.5 * 0.2 + 0.5) * 100,
    (0.5 * -0.4 + 0.5) * 50) = (60, 15). The previous camera stood 0.1 further along +x: the point is at camera-space x = 0.1 there ->
    (55, 15). A static point therefore moved by (+5, 0) pixels."""
    cam, prev = _translated(0.0), _translated(0.1)
    p = np.array([0.2, 0.4, 0.0])
    assert np.allclose(deform_ref.screen(cam, p), [60.0, 15.0], atol=1e-12)
    assert np.allclose(deform_ref.screen(prev, p), [55.0, 15.0], atol=1e-12)
    assert np.allclose(deform_ref.velocity(cam, prev, p, p), [5.0, 0.0], atol=1e-12)
    # below the 0.001 squared-length threshold the plane stores zero: 0.0004 px of camera-space x is 0.02 px
    assert np.array_equal(deform_ref.velocity(cam, _translated(0.0004), p, p), [0.0, 0.0])
    assert deform_ref.velocity(cam, _translated(0.0004), p, p, threshold=False)[0] > 0.0


def test_reference_triangle_whose_previous_corners_are_a_known_shift():
    """Triangle (0,0,0) (1,0,0) (0,1,0), hit at u = 0.25, v = 0.5: the point is (0.25, 0.5, 0) (all exactly representable). Its previous
    corners were 0.5 further along +x, and the previous transform lifted the instance by 2 along z: prev_point = (0.75, 0.5, 2)."""
    q = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    prev_q = q + np.array([0.5, 0, 0], np.float32)
    identity = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
    lifted = identity.copy(); lifted[2, 3] = 2.0
    assert np.array_equal(deform_ref.deformed_prev_point(q, 0.25, 0.5, identity), np.array([0.25, 0.5, 0.0], np.float32))
    got = deform_ref.deformed_prev_point(prev_q, 0.25, 0.5, lifted)
    assert got.dtype == np.float32 and np.array_equal(got, np.array([0.75, 0.5, 2.0], np.float32))
    # batched: two hits at once
    both = deform_ref.deformed_prev_point(np.stack([q, prev_q]), np.array([0.25, 0.25]), np.array([0.5, 0.5]), lifted)
    assert np.array_equal(both, np.array([[0.25, 0.5, 2.0], [0.75, 0.5, 2.0]], np.float32))
    # the rigid formula: a point of an instance that moved by +1 along x was 1 further back
    moved = identity.copy(); moved[0, 3] = 1.0
    assert np.allclose(deform_ref.rigid_prev_point(moved, identity, np.array([1.25, 0.5, 0.0])), [0.25, 0.5, 0.0], atol=1e-12)
    # with cameras from the first case: the corner shift alone is -0.5 in x = -25 px
    cam = _translated(0.0)
    vel = deform_ref.velocity(cam, cam, np.array([0.25, 0.5, 0.0]), deform_ref.deformed_prev_point(prev_q, 0.25, 0.5, identity))
    assert np.allclose(vel, [-25.0, 0.0], atol=1e-9)
