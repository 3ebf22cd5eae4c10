"""CPU tests of normal mapping (include/strolle_hip.h "normal mapping"): the boundary (entry points, the flag, the switch on a host-only engine), the
float32 restatement tests/normal_map_ref.py map_f32 at hand-worked cases, and the restatement against the float64 definition map_f64 over the cases of
tests/normal_map_cases.py — which is where the GPU tests' tolerances come from. No GPU is touched."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import normal_map_cases as nc
import normal_map_ref as nm
from strolle_amd import Engine, scenes
from strolle_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_OK, ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE = 0, 1, 2
SYMBOLS = ("st_engine_set_normal_mapping", "st_engine_get_normal_mapping")
F = np.float32


# ----------------------------------------------------------------------------- the boundary
def test_entry_points_and_the_flag_are_declared_everywhere():
    lib = api.load_library()
    header = open(os.path.join(ROOT, "include", "strolle_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "strolle-hip", "src", "ffi.rs")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(StEngine\*" % name, header), f"{name} is not declared in the header"
        assert re.search(r"pub fn %s\(" % name, ffi), f"{name} is not declared in the Rust binding"
    assert re.search(r"\bST_RAY_MAPPED_NORMAL\s*=\s*2\b", header), "ST_RAY_MAPPED_NORMAL = 2 is not in the header"
    assert re.search(r"pub const ST_RAY_MAPPED_NORMAL: u32 = 2;", ffi), "ST_RAY_MAPPED_NORMAL is not in the Rust binding"
    assert api.RAY_MAPPED_NORMAL == 2 and api.RAY_COHERENT == 1
    assert "fn set_normal_mapping" in open(os.path.join(ROOT, "rust", "strolle-hip", "src", "lib.rs")).read()
    for method in ("set_normal_mapping", "get_normal_mapping"):
        assert hasattr(Engine, method), method
    assert "normal mapping (NEW seam)" in header


def test_switch_round_trips_on_a_host_only_engine():
    e = Engine(device=-1)
    try:
        assert e.get_normal_mapping() is False, "normal mapping must be off by default"
        e.set_normal_mapping(True)
        assert e.get_normal_mapping() is True
        scenes.build_cornell(e)
        e.tick()                                   # only a flag: a host-only engine ticks with it on
        assert e.get_normal_mapping() is True
        e.set_normal_mapping(False)
        assert e.get_normal_mapping() is False
        on = C.c_int()
        assert e._b.engine_get_normal_mapping(e._h, None) == ST_ERR_INVALID_ARGUMENT
        assert e._b.engine_get_normal_mapping(None, C.byref(on)) == ST_ERR_INVALID_ARGUMENT
        assert e._b.engine_set_normal_mapping(None, 1) == ST_ERR_INVALID_ARGUMENT
    finally:
        e.close()


def test_unknown_flag_bits_are_still_errors_and_a_host_only_engine_does_not_know_the_flag():
    """(an engine with a device takes the flag: tests/test_gpu_normal_map.py)"""
    e = Engine(device=-1)
    try:
        scenes.build_cornell(e)
        e.tick()
        rays = np.zeros(4, api.RAY_DTYPE); hits = np.zeros(4, api.HIT_DTYPE)
        trace = e._b.scene_trace_rays
        assert trace(e._h, rays.ctypes.data, 4, hits.ctypes.data, api.RAY_COHERENT, None) == ST_ERR_NO_DEVICE   # a known bit gets past the argument checks
        for bad in (api.RAY_MAPPED_NORMAL, api.RAY_MAPPED_NORMAL | api.RAY_COHERENT, 4, 6, 0x80000000, 0x80000002):
            assert trace(e._h, rays.ctypes.data, 4, hits.ctypes.data, bad, None) == ST_ERR_INVALID_ARGUMENT
            assert trace(e._h, None, 0, None, bad, None) == ST_ERR_INVALID_ARGUMENT
    finally:
        e.close()


# ----------------------------------------------------------------------------- the restatement at hand-worked cases
# A quad in the xy-plane facing +z, u along +x, v along -y (glTF's v runs down the image): triangle (0,0,0) (1,0,0) (0,1,0) with uvs (0,0) (1,0) (0,-1).
E1, E2 = np.array([[1, 0, 0]], F), np.array([[0, 1, 0]], F)
UV0, UV1, UV2 = np.array([[0, 0]], F), np.array([[1, 0]], F), np.array([[0, -1]], F)
UP = np.array([[0, 0, 1]], F)
RECT = np.array([[0.0, 0.0, 1.0 / 8192.0, 1.0 / 256.0]], F)        # one texel at the atlas's origin
MID = np.array([[0.5, 0.5]], F)


def _atlas(texel):
    a = np.zeros((256, 8192, 4), np.uint8)
    a[0, 0, :3] = texel; a[0, 1, :3] = texel; a[1, 0, :3] = texel; a[1, 1, :3] = texel      # the clamp never leaves the texel's value
    a[:2, :2, 3] = 255
    return a


def _one(texel, n=UP, s=(1.0,), e1=E1, e2=E2, uv0=UV0, uv1=UV1, uv2=UV2, rect=RECT):
    out, mapped, _ = nm.map_f32(n, np.array(s, F), MID, e1, e2, uv0, uv1, uv2, rect, _atlas(texel))
    return out[0].astype(np.float64), bool(mapped[0])


def test_the_sign_convention_of_the_quad():
    x, mapped = _one((255, 128, 128))
    assert mapped and x[0] > 0.99 and abs(x[1]) < 0.01 and 0 < x[2] < 0.01, f"(255, 128, 128) must tilt the normal towards +x: {x}"
    y, mapped = _one((128, 255, 128))
    assert mapped and y[1] > 0.99 and abs(y[0]) < 0.01 and 0 < y[2] < 0.01, f"(128, 255, 128) must tilt the normal towards +y: {y}"
    for v in (x, y):
        assert abs(np.linalg.norm(v) - 1.0) < 1e-6


def test_the_neutral_texel_moves_the_normal_by_less_than_six_milliradians():
    z, mapped = _one((128, 128, 255))
    angle = np.arccos(np.clip(z[2], -1, 1))
    assert mapped and 0 < angle < 0.006, angle        # 128 / 255 is not one half: t = (0.0039, 0.0039, 1)


def test_a_mirrored_uv_layout_tilts_the_same_world_way():
    """u along -x: uvs (0,0) (-1,0) (0,-1). Pu = -x, so T = -x; the layout is mirrored, h = -1, and B stays +y... the texel's +x then means -x in the
    world (the image is seen mirrored) while its +y is unchanged — what a mirrored uv layout looks like with a correct handedness"""
    uv1 = np.array([[-1, 0]], F)
    # h: C = nf x T = z x (-x) = -y; Pv = -y; C . Pv = +1 > 0 -> h = -1, B = +y
    x, _ = _one((255, 128, 128), uv1=uv1)
    y, _ = _one((128, 255, 128), uv1=uv1)
    assert x[0] < -0.99, x
    assert y[1] > 0.99, y
    # v mirrored as well (v along +y: uvs (0,0) (-1,0) (0,1)): a rotation by 180 degrees, not a mirror: h = +1 and B = C = -y
    y2, _ = _one((128, 255, 128), uv1=uv1, uv2=np.array([[0, 1]], F))
    assert y2[1] < -0.99, y2


def test_a_mirrored_instance_transform():
    """the quad under diag(-1, 1, 1): its world edges are e1 = -x, e2 = +y, its front normal stays +z (the bake's inverse transpose) while the winding
    turns. uvs unchanged, so u now runs along -x in the world and the texel's +x must tilt towards world -x; +y stays +y."""
    e1 = np.array([[-1, 0, 0]], F)
    x, _ = _one((255, 128, 128), e1=e1)
    y, _ = _one((128, 255, 128), e1=e1)
    assert x[0] < -0.99 and y[1] > 0.99, (x, y)


def test_a_back_face_hit_is_exactly_the_negated_front_result():
    for texel in ((255, 128, 128), (128, 255, 128), (37, 201, 180), (128, 128, 255)):
        front, _, _ = nm.map_f32(UP, np.array([1.0], F), MID, E1, E2, UV0, UV1, UV2, RECT, _atlas(texel))
        back, _, _ = nm.map_f32(-UP, np.array([-1.0], F), MID, E1, E2, UV0, UV1, UV2, RECT, _atlas(texel))
        assert np.array_equal((-front).view(np.uint32), back.view(np.uint32)), texel


def test_degenerate_frames_return_the_input_bits():
    n = np.array([[0.6, 0.0, 0.8]], F)
    same = lambda out: np.array_equal(out.view(np.uint32), n.view(np.uint32))
    equal = np.array([[0.3, 0.6]], F)
    for uv0, uv1, uv2, what in ((equal, equal, equal, "all three uvs equal"), (UV0, np.array([[0.5, 0.5]], F), np.array([[1, 1]], F), "collinear uvs")):
        out, mapped, _ = nm.map_f32(n, np.array([1.0], F), MID, E1, E2, uv0, uv1, uv2, RECT, _atlas((255, 128, 128)))
        assert not mapped[0] and same(out), what
    # Pu parallel to n: the surface's u direction has no component in the tangent plane
    out, mapped, _ = nm.map_f32(np.array([[1, 0, 0]], F), np.array([1.0], F), MID, E1, E2, UV0, UV1, UV2, RECT, _atlas((255, 128, 128)))
    assert not mapped[0] and np.array_equal(out, np.array([[1, 0, 0]], F)), "Pu parallel to n"
    # no map
    out, mapped, _ = nm.map_f32(n, np.array([1.0], F), MID, E1, E2, UV0, UV1, UV2, np.zeros((1, 4), F), _atlas((255, 128, 128)))
    assert not mapped[0] and same(out), "a zero rectangle"
    # NaN inputs leave the bits alone too
    nan = np.array([[np.nan, 0, 1]], F)
    out, mapped, _ = nm.map_f32(nan, np.array([1.0], F), MID, E1, E2, UV0, UV1, UV2, RECT, _atlas((255, 128, 128)))
    assert not mapped[0] and np.array_equal(out.view(np.uint32), nan.view(np.uint32))


def test_a_texel_below_the_tangent_plane_is_flattened():
    low, _ = _one((255, 128, 0))
    flat, _ = _one((255, 128, 127))
    assert low[2] == 0.0 and flat[2] == 0.0, (low, flat)          # z byte below 128: t.z = max(2 m.z - 1, 0) = 0
    assert np.array_equal(low, flat), "every z byte below 128 gives the same normal"
    assert low[0] > 0.99
    up, _ = _one((255, 128, 129))
    assert up[2] > 0.0


def test_the_srgb_curve_is_never_applied():
    """byte 188 is 0.737 as byte / 255 and 0.503 through the sRGB curve: decoded linearly, (188, 128, 255) tilts by atan(0.474 / 1) = 0.443 rad"""
    v, _ = _one((188, 128, 255))
    assert abs(np.arctan2(v[0], v[2]) - np.arctan2(2 * 188 / 255 - 1, 1.0)) < 1e-3


# ----------------------------------------------------------------------------- the restatement against the definition
@pytest.mark.parametrize("case", nc.CASES)
def test_restatement_follows_the_definition_and_the_table_follows_the_measurement(case):
    m = nc.measure(case)
    print(f"{case}: {json.dumps(m)}")
    assert m["shares"]["excluded"] <= nc.CAPS["excluded"], f"{case}: {m['shares']['excluded']:.4f} of the rays are excluded"
    assert m["shares"]["compared_mapped"] >= nc.CAPS["compared_mapped"], f"{case}: only {m['shares']['compared_mapped']:.4f} of the rays are compared mapped hits"
    assert m["tolerance"] == nc.TOLERANCES[case], f"{case}: TOLERANCES holds {nc.TOLERANCES[case]}, the measurement gives {m['tolerance']}"


def test_the_profile_holds_the_measurement():
    with open(os.path.join(ROOT, "profiles", "normal_mapping.json")) as f:
        prof = json.load(f)
    for case in nc.CASES:
        assert prof["cpu"][case]["tolerance"] == nc.TOLERANCES[case], case
        assert prof["cpu"][case]["shares"]["excluded"] <= nc.CAPS["excluded"]
