"""The decisions the scene's BVH owner takes (st_bvh_refresh.h SceneTree: plan, write, the accessors of derived state), held to a recording.

One fixed sequence of ABI calls (sequence(), below; tools/tree_trace.py prints it) goes through every tree decision of a tick in each refresh mode
0..4, on the two scenes that split the paths: scenes.build_random_soup(e, 700, seed=11), whose ~700 triangles do not fit LDS (compact, wide and
device-built streams), and scenes.build_cornell, which fits (none of them). After every step the eight counter and switch seams are read —
st_debug_bvh_refits, _bvh_device_refits, _device_builds, _device_tree_refits, _bvh_depth, _auto_tree, _bvh_refresh, and the mode set through
st_set_bvh_refresh — and compared with tests/golden/tree_decisions.json, which tests/golden/make_tree_decisions.py wrote with the library of
8f0148b ("Add colour grading"), the parent of the commit that gave the tree one owner: the "host" entries with a host-only engine, the "device"
entries on an MI355X. Integers are stored as they are, the leaf-run weight as a hex float. No frame is rendered, and the golden holds no hash of
a buffer: device-built data is compared between two libraries on one machine (tools/tree_trace.py), where a machine cannot make it flaky.

The second test runs the sequence on two engines: one reads every `what` of st_debug_read_scene after every tick, the other reads nothing until
the end. A debug read may bring derived state up to date (and rebuild the host's tree), but it must not change what a later read returns: the
final buffers, for every `what`, are equal byte for byte. Counters are not compared. READS_DIFFER names the `what`s left out because they
already differed with the parent's library. One did, and is not fixed here: under ST_BVH_REFIT (mode 1) on the device, the soup's live wide
nodes (what 16). A debug read of the wide topology (14, 15) leaves the tick's own topology void, so the next host refit collapses the tree
again, by the surface areas of the refitted boxes, where an engine nobody read keeps the collapse of its last rebuild. Both are valid wide
trees of the same binary tree; the leaf records (17) are equal."""
import hashlib
import json
import os

import numpy as np
import pytest

from strolle_amd import CameraMode, Engine, Instance, Material, Mesh, StrolleError, scenes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_decisions.json")
SCENES = ("soup", "cornell")
MODES = (0, 1, 2, 3, 4)
WHATS = (0, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17)   # the tree's cases of st_debug_read_scene
PROBE = 7000   # mesh, material and instance handle of the quad the sequence moves; PROBE + 1: the instance it spawns
READS_DIFFER = {("device", 1): (16,)}   # (half, mode) -> the `what`s whose final buffer depends on earlier reads: findings, see the docstring


def _quad(size):
    pos = np.array([[[0, 0, 0], [size, 0, 0], [size, size, 0]], [[0, 0, 0], [size, size, 0], [0, size, 0]]], np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (2, 3, 1))
    uv = pos[:, :, :2] / np.float32(size)
    return Mesh(pos, nrm, uv)


def _at(i):
    return np.array([[1, 0, 0, -0.5 + 0.05 * i], [0, 1, 0, 0.9], [0, 0, 1, 0.1 + 0.01 * i]], np.float32)


def build(e, scene):
    scenes.build_random_soup(e, 700, seed=11) if scene == "soup" else scenes.build_cornell(e)
    e.insert_material(PROBE, Material(base_color=(0.2, 0.7, 0.3, 1.0)))
    e.insert_mesh(PROBE, _quad(0.2))
    e.insert_instance(PROBE, Instance(PROBE, PROBE, _at(0)))


def seams(e, mode):
    rebuilds, refits = e.bvh_refits()
    depth, stack = e.bvh_depth()
    weight, first_on_device = e.auto_tree()
    prims, reused = e.bvh_refresh()
    return {"mode": mode, "rebuilds": rebuilds, "refits": refits, "device_refits": e.bvh_device_refits(), "device_builds": e.device_builds(),
            "device_tree_refits": e.device_tree_refits(), "depth": depth, "stack": stack, "leaf_run_weight": float(weight).hex(),
            "first_on_device": int(first_on_device), "primitives": prims, "reused": reused}


def read_all(e, order=WHATS):
    """what -> the buffer's bytes, or None where the library refuses (a host-only engine has no live copy)"""
    out = {}
    for what in order:
        try:
            out[what] = e.read_scene(what).tobytes()
        except StrolleError:
            out[what] = None
    return out


def sequence(e, scene, mode, stream=0):
    """The fixed sequence on a fresh engine: yields (step name, st_tick's status or None where the step ticks nothing) after every step."""
    def tick():
        try:
            e.tick(stream)
            return "ok"
        except StrolleError as err:   # (ST_ERR_BVH_TOO_DEEP is a status of a tick that did everything)
            return str(err).split(":")[0]
    e.set_bvh_refresh(mode)
    build(e, scene)
    yield "first", tick()
    yield "idle", tick()
    e.insert_instance(PROBE, Instance(PROBE, PROBE, _at(1)))
    yield "move", tick()
    e.insert_instance(PROBE + 1, Instance(PROBE, PROBE, _at(-3)))
    yield "spawn", tick()
    e.remove_instance(PROBE + 1)
    yield "despawn", tick()
    e.insert_material(PROBE, Material(base_color=(0.7, 0.2, 0.3, 1.0)))
    yield "material", tick()
    e.insert_mesh(PROBE, _quad(0.3)); e.insert_instance(PROBE, Instance(PROBE, PROBE, _at(2)))
    yield "mesh", tick()
    for i in range(16):   # crosses the limit of refits between two device builds
        e.insert_instance(PROBE, Instance(PROBE, PROBE, _at(3 + i)))
        yield f"move_{i + 1}", tick()
    cam = e.create_camera(scenes.camera_for((64, 48), (0.0, 1.0, 3.2), (0.0, 1.0, 0.0), CameraMode.BVH_HEATMAP))   # an observer of the contract stream
    yield "heatmap_on", tick()
    e.delete_camera(cam)
    yield "heatmap_off", tick()
    e.insert_instance(PROBE, Instance(PROBE, PROBE, _at(20)))
    yield "move_after_observer", tick()
    e.set_exact(True)
    yield "exact_on", tick()
    e.set_exact(False)
    yield "exact_off", tick()


def record(scene, mode, device, every_tick=False):
    """(the seams after every step, the buffers of the reads): a read of every `what` in ascending and then in descending order ends the sequence;
    every_tick reads them after every step too."""
    e = Engine(device=device)
    try:
        rows = []
        for name, status in sequence(e, scene, mode):
            if every_tick:
                read_all(e)
            rows.append(dict(step=name, status=status, **seams(e, mode)))
        up = read_all(e)
        rows.append(dict(step="reads_up", status=None, **seams(e, mode)))
        down = read_all(e, WHATS[::-1])
        rows.append(dict(step="reads_down", status=None, **seams(e, mode)))
        return rows, up, down
    finally:
        e.close()


def digest(buffers):
    return {what: (hashlib.sha256(b).hexdigest()[:16] if b is not None else None) for what, b in buffers.items()}


def _golden(half, scene, mode):
    with open(GOLDEN) as f:
        return json.load(f)[half][f"{scene}_{mode}"]


def _check_decisions(half, scene, mode, device):
    rows, _, _ = record(scene, mode, device)
    want = _golden(half, scene, mode)
    assert [r["step"] for r in rows] == [r["step"] for r in want]
    for got, expected in zip(rows, want):
        assert got == expected, f"{scene}, mode {mode}, step {got['step']}"


def _check_reads(half, scene, mode, device):
    _, _, quiet = record(scene, mode, device)
    _, _, read = record(scene, mode, device, every_tick=True)
    differ = [what for what in WHATS if quiet[what] != read[what]]   # (None: the library refused the read)
    print(f"{half} {scene} mode {mode}: final buffers that depend on earlier debug reads: {differ}")
    assert [what for what in differ if what not in READS_DIFFER.get((half, mode), ())] == []


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene", SCENES)
def test_tree_decisions_host_only(scene, mode):
    _check_decisions("host", scene, mode, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene", SCENES)
def test_tree_decisions_on_the_device(scene, mode):
    _check_decisions("device", scene, mode, 0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene", SCENES)
def test_debug_reads_do_not_change_later_reads_host_only(scene, mode):
    _check_reads("host", scene, mode, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene", SCENES)
def test_debug_reads_do_not_change_later_reads_on_the_device(scene, mode):
    _check_reads("device", scene, mode, 0)
