"""CPU tests of the skinned-mesh boundary (include/strolle_hip.h "skinned meshes"): StSkinVertex has the same layout in C, ctypes and numpy,
st_mesh_set_skin checks its arguments on a host-only engine (where st_instance_set_pose is ST_ERR_NO_DEVICE), and the numpy restatement
of k_skin.hip gives the known answers."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from skin_ref import bind_store, palette12, skin
from strolle_amd import Engine, Instance, Material, Mesh, StrolleError, scenes
from strolle_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_ERR_INVALID_ARGUMENT, ST_ERR_NO_DEVICE = 1, 2

C_PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "strolle_hip.h"
int main(void) {
    printf("%zu %zu %zu\n", sizeof(StSkinVertex), offsetof(StSkinVertex, joints), offsetof(StSkinVertex, weights));
    return 0;
}
"""


def test_skin_vertex_layout_agrees_between_c_ctypes_and_numpy(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "layout.c"
    src.write_text(C_PROGRAM)
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    layout = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert layout == [24, 0, 8]
    assert layout == [C.sizeof(api.StSkinVertex), api.StSkinVertex.joints.offset, api.StSkinVertex.weights.offset]
    d = api.SKIN_VERTEX_DTYPE
    assert [d.itemsize, d.fields["joints"][1], d.fields["weights"][1]] == layout


def test_entry_points_are_exported():
    lib = api.load_library()
    for name in ("st_mesh_set_skin", "st_instance_set_pose", "st_debug_skinning", "st_debug_read_posed"):
        assert hasattr(lib, name), name


def _status(e, *args):
    return e._b.mesh_set_skin(e._h, *args)


def _corners(joints, weights):
    c = np.zeros(len(joints), api.SKIN_VERTEX_DTYPE)
    c["joints"] = joints; c["weights"] = weights
    return c


def test_set_skin_error_matrix_on_a_host_only_engine():
    e = Engine(device=-1)
    mesh, jt, wt = scenes.skinned_tube(2, 3, 4)
    e.insert_mesh(1, mesh)
    n = 3 * len(mesh.positions)
    good = _corners(jt, wt)
    assert _status(e, 1, good.ctypes.data, n, 4) == 0                            # a host-only engine accepts a valid skin
    assert _status(e, 2, good.ctypes.data, n, 4) == ST_ERR_INVALID_ARGUMENT       # unknown mesh
    assert _status(e, 1, None, n, 4) == ST_ERR_INVALID_ARGUMENT                   # null pointer
    assert _status(e, 1, good.ctypes.data, n - 3, 4) == ST_ERR_INVALID_ARGUMENT   # wrong corner_count
    assert _status(e, 1, good.ctypes.data, n, 0) == ST_ERR_INVALID_ARGUMENT       # joint_count outside 1..256
    assert _status(e, 1, good.ctypes.data, n, 257) == ST_ERR_INVALID_ARGUMENT
    assert _status(e, 1, good.ctypes.data, n, 3) == ST_ERR_INVALID_ARGUMENT       # joint index 3 >= joint_count
    big = np.zeros((n, 4), np.uint16); big[:, 0] = 255
    assert _status(e, 1, _corners(big, wt).ctypes.data, n, 256) == 0              # 256 joints, index 255
    for bad in (-1.0, math.nan, math.inf):
        w = wt.copy(); w[5, 2] = bad
        assert _status(e, 1, _corners(jt, w).ctypes.data, n, 4) == ST_ERR_INVALID_ARGUMENT, bad
    w = wt.copy(); w[7] = 0.0
    assert _status(e, 1, _corners(jt, w).ctypes.data, n, 4) == ST_ERR_INVALID_ARGUMENT   # an all-zero set
    e.set_skin(1, jt, wt, 4)
    with pytest.raises(StrolleError):
        e.set_skin(1, jt, wt, 2)
    e.close()


def test_set_pose_needs_a_device():
    e = Engine(device=-1)
    mesh, jt, wt = scenes.skinned_tube(2, 3, 2)
    e.insert_mesh(1, mesh); e.set_skin(1, jt, wt, 2)
    e.insert_material(1, Material())
    e.insert_instance(1, Instance(1, 1, np.eye(4, dtype=np.float32)[:3]))
    pose = palette12(scenes.bend_pose(2, 0.5))
    assert e._b.instance_set_pose(e._h, 1, pose.ctypes.data_as(C.POINTER(C.c_float)), 2) == ST_ERR_NO_DEVICE
    assert e._b.instance_set_pose(e._h, 1, None, 0) == ST_ERR_NO_DEVICE
    e.close()


def _one_triangle():
    return Mesh(np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32), np.array([[[0, 0, 1], [0.6, 0, 0.8], [0, 0.6, 0.8]]], np.float32),
                np.array([[[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]]], np.float32))


def test_restatement_identity_palette_returns_the_bind_bits():
    mesh, jt, wt = scenes.skinned_tube(8, 6, 5)
    bind = bind_store(mesh)
    j1 = np.zeros_like(jt); w1 = np.zeros_like(wt)
    rng = np.random.default_rng(3)
    j1[:, 0] = rng.integers(0, 5, len(jt)); w1[:, 0] = 1.0
    j1[:, 1:] = rng.integers(0, 5, (len(jt), 3))                                 # unused slots at weight 0 name any joint
    ident = np.tile(np.eye(4, dtype=np.float32)[:3], (5, 1, 1))
    posed = skin(bind, j1, w1, ident)
    assert posed.tobytes() == bind.tobytes()


def test_restatement_known_answers():
    bind = bind_store(_one_triangle())
    j = np.zeros((3, 4), np.uint16); w = np.zeros((3, 4), np.float32); w[:, 0] = 1.0
    # a translation moves the positions and keeps the normals
    t = np.eye(4, dtype=np.float32)[:3].copy(); t[:, 3] = (1.0, 2.0, 3.0)
    posed = skin(bind, j, w, t[None])
    assert np.array_equal(posed[0, :9].reshape(3, 3), bind[0, :9].reshape(3, 3) + np.float32([1, 2, 3]))
    assert np.array_equal(posed[0, 9:], bind[0, 9:])
    # a mirror (det < 0) flips x of positions and normals
    m = np.eye(4, dtype=np.float32)[:3].copy(); m[0, 0] = -1.0
    posed = skin(bind, j, w, m[None])
    assert np.array_equal(posed[0, 0:9:3], -bind[0, 0:9:3]) and np.array_equal(posed[0, 9:18:3], -bind[0, 9:18:3])
    # non-uniform scale: normals follow the inverse transpose, then are normalised
    s = np.diag(np.float32([2.0, 1.0, 1.0, 1.0]))[:3]
    posed = skin(bind, j, w, s[None])
    n = bind[0, 9:18].reshape(3, 3) * np.float32([0.5, 1, 1])
    n = n / np.linalg.norm(n.astype(np.float64), axis=1, keepdims=True)
    assert np.allclose(posed[0, 9:18].reshape(3, 3), n, atol=1e-6)
    # a singular blend keeps the bind normal; two half-weights of the same joint are that joint
    z = np.zeros((1, 3, 4), np.float32)
    assert np.array_equal(skin(bind, j, w, z)[0, 9:18], bind[0, 9:18])
    j2 = np.zeros((3, 4), np.uint16); w2 = np.zeros((3, 4), np.float32); w2[:, :2] = 0.5
    assert np.array_equal(skin(bind, j2, w2, t[None]), skin(bind, j, w, t[None]))
    # the blend: w0 J0 + w1 J1 of two translations is the weighted translation
    pair = np.stack([np.eye(4, dtype=np.float32)[:3], t]); j3 = j2.copy(); j3[:, 1] = 1; w3 = w2.copy(); w3[:, 0] = 0.75; w3[:, 1] = 0.25
    posed = skin(bind, j3, w3, pair)
    assert np.array_equal(posed[0, :9].reshape(3, 3), bind[0, :9].reshape(3, 3) + np.float32([0.25, 0.5, 0.75]))


def test_tube_and_bend_pose_shapes():
    mesh, jt, wt = scenes.skinned_tube(128, 32, 32)
    assert len(mesh.positions) == 8192 and jt.shape == (3 * 8192, 4) and wt.shape == (3 * 8192, 4)
    assert jt.max() < 32 and np.all(wt >= 0) and np.all(wt.sum(1) > 0) and np.allclose(wt.sum(1), 1.0)
    pose = scenes.bend_pose(32, 1.0, 0.5)
    assert pose.shape == (32, 3, 4) and pose.dtype == np.float32
    assert np.allclose(scenes.bend_pose(32, 0.0), np.tile(np.eye(4, dtype=np.float32)[:3], (32, 1, 1)), atol=1e-6)
