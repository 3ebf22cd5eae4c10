"""CPU tests of the morph-target boundary (include/strolle_hip.h "morph targets"): the entry points exist in the library, the header and the
Rust binding, StMorphDelta has one layout everywhere, st_mesh_set_morph_targets checks its arguments on a host-only engine (where
st_instance_set_morph_weights is ST_ERR_NO_DEVICE), and the numpy restatement of the morph stage gives answers worked out by hand."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import morph_ref
from skin_ref import bind_store
from strolle_amd import Engine, Instance, Material, Mesh, StrolleError, scenes
from strolle_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE = 1, 2
SYMBOLS = ("st_mesh_set_morph_targets", "st_instance_set_morph_weights", "st_debug_morphing")

C_PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "strolle_hip.h"
int main(void) {
    printf("%zu %zu %zu\n", sizeof(StMorphDelta), offsetof(StMorphDelta, position), offsetof(StMorphDelta, normal));
    return 0;
}
"""


def test_morph_delta_is_24_bytes_in_c_ctypes_and_numpy(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "layout.c"
    src.write_text(C_PROGRAM)
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    layout = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert layout == [24, 0, 12]
    assert layout == [C.sizeof(api.StMorphDelta), api.StMorphDelta.position.offset, api.StMorphDelta.normal.offset]
    d = api.MORPH_DELTA_DTYPE
    assert [d.itemsize, d.fields["position"][1], d.fields["normal"][1]] == layout


def test_entry_points_are_exported_declared_and_bound():
    lib = api.load_library()
    header = open(os.path.join(ROOT, "include", "strolle_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "strolle-hip", "src", "ffi.rs")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert f"int {name}(StEngine* e" in header, f"{name} is not declared"
        assert f"pub fn {name}(e: *mut StEngine" in ffi, f"{name} is not bound in ffi.rs"
    assert "pub struct StMorphDelta" in ffi and "typedef struct StMorphDelta" in header


def _deltas(dp, dn):
    d = np.zeros((dp.shape[0], dp.shape[1] * 3), api.MORPH_DELTA_DTYPE)
    d["position"] = dp.reshape(dp.shape[0], -1, 3); d["normal"] = dn.reshape(dn.shape[0], -1, 3)
    return d


def _status(e, *args):
    return e._b.mesh_set_morph_targets(e._h, *args)


def test_set_morph_targets_error_matrix_on_a_host_only_engine():
    e = Engine(device=-1)
    mesh, _, _ = scenes.skinned_tube(2, 3, 4)
    e.insert_mesh(1, mesh)
    dp, dn = scenes.tube_morph_targets(mesh)
    n = 3 * len(mesh.positions)
    good = _deltas(dp, dn)
    assert _status(e, 1, good.ctypes.data, n, 3) == 0                              # a host-only engine accepts valid targets
    assert _status(e, 2, good.ctypes.data, n, 3) == ST_ERR_INVALID_ARGUMENT         # unknown mesh
    assert _status(e, 1, None, n, 3) == ST_ERR_INVALID_ARGUMENT                     # null pointer
    assert _status(e, 1, good.ctypes.data, n - 3, 3) == ST_ERR_INVALID_ARGUMENT     # wrong corner_count
    assert _status(e, 1, good.ctypes.data, n, 0) == ST_ERR_INVALID_ARGUMENT         # target_count outside 1..64
    many = _deltas(np.zeros((65, n // 3, 3, 3), np.float32), np.zeros((65, n // 3, 3, 3), np.float32))
    assert _status(e, 1, many.ctypes.data, n, 65) == ST_ERR_INVALID_ARGUMENT
    assert _status(e, 1, many.ctypes.data, n, 64) == 0                              # 64 targets
    assert _status(e, 1, good.ctypes.data, n, 1) == 0                               # 1 target
    for field in ("position", "normal"):
        for bad in (math.nan, math.inf, -math.inf):
            d = good.copy(); d[field][2, 7, 1] = bad                                # the last target, somewhere inside
            assert _status(e, 1, d.ctypes.data, n, 3) == ST_ERR_INVALID_ARGUMENT, (field, bad)
    e.set_morph_targets(1, dp, dn)
    with pytest.raises(StrolleError):
        e.set_morph_targets(1, dp[:, :-1], dn[:, :-1])
    with pytest.raises(StrolleError):
        e.set_morph_targets(1, dp, dn[:2])                                          # the two arrays differ in shape
    assert e.morphing_stats() == (0, 0, 0)                                          # nothing is on a device
    e.close()


def test_set_morph_weights_needs_a_device():
    e = Engine(device=-1)
    mesh, _, _ = scenes.skinned_tube(2, 3, 2)
    e.insert_mesh(1, mesh); e.set_morph_targets(1, *scenes.tube_morph_targets(mesh))
    e.insert_material(1, Material())
    e.insert_instance(1, Instance(1, 1, np.eye(4, dtype=np.float32)[:3]))
    w = np.float32([0.5, 0.0, 1.0])
    assert e._b.instance_set_morph_weights(e._h, 1, w.ctypes.data_as(C.POINTER(C.c_float)), 3) == ST_ERR_NO_DEVICE
    assert e._b.instance_set_morph_weights(e._h, 1, None, 0) == ST_ERR_NO_DEVICE
    e.close()


def test_targets_follow_the_mesh_through_insert_and_remove():
    """What a host-only engine shows of the lifecycle: targets are checked against the mesh as it is NOW, and go with it."""
    e = Engine(device=-1)
    small, _, _ = scenes.skinned_tube(2, 3, 2)
    large, _, _ = scenes.skinned_tube(3, 3, 2)
    e.insert_mesh(1, small)
    e.set_morph_targets(1, *scenes.tube_morph_targets(small))
    e.insert_mesh(1, large)                                                         # drops the targets made for the old triangles
    with pytest.raises(StrolleError):
        e.set_morph_targets(1, *scenes.tube_morph_targets(small))
    e.set_morph_targets(1, *scenes.tube_morph_targets(large))
    e.set_morph_targets(1, *scenes.tube_morph_targets(large))                       # replacing is allowed
    e.remove_mesh(1)
    with pytest.raises(StrolleError):
        e.set_morph_targets(1, *scenes.tube_morph_targets(large))
    e.tick()                                                                        # a host-only tick has nothing to morph
    e.close()


# ----------------------------------------------------------------------------- the restatement, against values worked out by hand
def _one_triangle():
    return Mesh(np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32), np.array([[[0, 0, 1], [0, 0, 1], [0, 0, 1]]], np.float32),
                np.array([[[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]]], np.float32))


def test_restatement_two_targets_by_hand():
    bind = bind_store(_one_triangle())
    dp = np.zeros((2, 1, 3, 3), np.float32); dn = np.zeros((2, 1, 3, 3), np.float32)
    dp[0, 0] = [[2, 4, 6], [0, 0, 0], [1, 1, 1]]; dp[1, 0] = [[0.5, 0, 0], [0.25, 0.25, 0.25], [0, 0, 0]]
    dn[0, 0] = [[6, 0, -2], [0, 0, 2], [0, 0, 0]]; dn[1, 0] = [[0, -2, 0], [0, 0, 0.5], [0, 0, 0]]
    out = morph_ref.morph(bind, dp, dn, [0.5, -2.0])
    # positions: base + 0.5 d0 - 2 d1, every step exact in float32
    assert np.array_equal(out[0, :9].reshape(3, 3), np.float32([[0, 2, 3], [0.5, -0.5, -0.5], [0.5, 1.5, 0.5]]))
    # normals: corner 0 (0,0,1) + (3,0,-1) + (0,4,0) = (3,4,0), length 5 -> each component x float32(1 / 5); corner 1 (0,0,1) + (0,0,1) - (0,0,1) = (0,0,1);
    # corner 2 has zero deltas: (0,0,1) x (1 / 1)
    fifth = np.float32(1.0) / np.float32(5.0)
    want = np.float32([[np.float32(3) * fifth, np.float32(4) * fifth, 0], [0, 0, 1], [0, 0, 1]])
    assert np.array_equal(out[0, 9:18].reshape(3, 3).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(out[0, 18:], bind[0, 18:])


def test_restatement_skips_zero_weights_and_keeps_a_negative_zero():
    mesh = _one_triangle()
    mesh.positions[0, 0, 0] = -0.0
    bind = bind_store(mesh)
    assert np.signbit(bind[0, 0])
    dp = np.zeros((2, 1, 3, 3), np.float32); dn = np.zeros((2, 1, 3, 3), np.float32)
    dp[0, 0, 0, 0] = 1.0       # weight 0: multiplied in, (-0) + 0 * 1 would be +0
    dp[1, 0, 0, 0] = -0.0      # weight 1: (-0) + 1 * (-0) = -0
    out = morph_ref.morph(bind, dp, dn, [0.0, 1.0])
    assert out[0, 0] == 0 and np.signbit(out[0, 0]), "the zero-weight target was multiplied in"
    assert morph_ref.active_targets([0.0, 1.0, -0.0, 2.0]) == [1, 3]


def test_restatement_cancelled_normal_falls_back_to_the_base_normal():
    bind = bind_store(_one_triangle())
    dp = np.zeros((1, 1, 3, 3), np.float32); dn = np.zeros((1, 1, 3, 3), np.float32)
    dn[0, 0, 1] = [0, 0, -1]                           # corner 1: (0,0,1) + 1 * (0,0,-1) has length 0
    dn[0, 0, 2] = [3.0e38, 3.0e38, 0]                  # corner 2: the squared length overflows: not finite
    out = morph_ref.morph(bind, dp, dn, [1.0])
    assert np.array_equal(out[0, 9:18].view(np.uint32), bind[0, 9:18].view(np.uint32))


def test_restatement_without_an_active_target_returns_the_base_bits():
    mesh, jt, wt = scenes.skinned_tube(4, 5, 3)
    bind = bind_store(mesh)
    bind[3, 2] = -0.0
    dp, dn = scenes.tube_morph_targets(mesh)
    assert morph_ref.morph(bind, dp, dn, [0.0, -0.0, 0.0]).tobytes() == bind.tobytes()
    # and the composition with an identity palette is the morph alone
    ident = np.tile(np.eye(4, dtype=np.float32)[:3], (3, 1, 1))
    j1 = np.zeros_like(jt); w1 = np.zeros_like(wt); w1[:, 0] = 1.0
    m = morph_ref.morph(bind, dp, dn, [0.5, 0.0, 1.5])
    both = morph_ref.morph_skin(bind, dp, dn, [0.5, 0.0, 1.5], j1, w1, ident)
    assert np.array_equal(both[:, :9], m[:, :9]) and np.allclose(both[:, 9:18], m[:, 9:18], atol=1e-6)


def test_tube_morph_targets_shapes():
    mesh, _, _ = scenes.skinned_tube(8, 6, 4)
    dp, dn = scenes.tube_morph_targets(mesh)
    n = len(mesh.positions)
    assert dp.shape == dn.shape == (3, n, 3, 3) and dp.dtype == dn.dtype == np.float32
    assert np.all(np.isfinite(dp)) and np.all(np.isfinite(dn)) and all(np.abs(dp[k]).max() > 0.05 for k in range(3))
    full = mesh.normals[None].astype(np.float64) + dn                               # at weight 1 each target's normals are unit
    assert np.allclose(np.linalg.norm(full, axis=-1), 1.0, atol=1e-5)
