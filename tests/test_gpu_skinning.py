"""GPU tests of skinned meshes (include/strolle_hip.h "skinned meshes"; k_skin.hip, st_deform.cpp).

Engine A skins on the device: a skin per mesh, a pose per instance. Engine B is the same scene without skinning: every posed instance has a
mesh of its own into which B re-inserts A's read-back posed triangles each tick. What A renders, bakes and answers must be what B does."""
import ctypes as C

import numpy as np
import pytest
import torch

from skin_ref import bind_store, palette12, skin
from strolle_amd import Aov, Buffer, CameraMode, Engine, Instance, Material, Mesh, StrolleError, aov_planes, scenes
from strolle_amd.api import HIT_DTYPE, RAY_DTYPE

pytestmark = pytest.mark.gpu

REBUILD, REFIT, REFIT_DEVICE, AUTO = 0, 1, 2, 4
TUBE, TUBE_MAT, OWN_MESH = 7000, 7000, 8000
AGREE = 0.999   # tests/test_gpu_ray_query.py


def tube_xform(x, y, z, s=1.0):
    return np.array([[s, 0, 0, x], [0, s, 0, y], [0, 0, s, z]], np.float32)


def random_palette(rng, joints, mirrored=True):
    """Rotations, non-uniform scale, translations; one joint mirrored (det < 0)."""
    out = []
    for k in range(joints):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        m = np.zeros((3, 4))
        m[:, :3] = q @ np.diag(rng.uniform(0.5, 1.6, 3))
        if mirrored and k == joints // 2:
            m[:, 0] = -m[:, 0]
        m[:, 3] = rng.uniform(-0.5, 0.5, 3)
        out.append(m)
    return np.asarray(out, np.float32)


def random_skin(rng, n_corners, joints):
    """1-4 influences per corner, unused slots at weight 0 (naming any joint)."""
    jt = rng.integers(0, joints, (n_corners, 4)).astype(np.uint16)
    wt = rng.uniform(0.05, 1.0, (n_corners, 4)).astype(np.float32)
    used = rng.integers(1, 5, n_corners)
    wt[np.arange(4)[None, :] >= used[:, None]] = 0.0
    return jt, wt


def random_mesh(rng, n):
    pos = rng.uniform(-1, 1, (n, 3, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3, 3)); nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    return Mesh(pos, nrm.astype(np.float32), rng.uniform(0, 1, (n, 3, 2)).astype(np.float32))


def posed_mesh(e, inst, bind_mesh):
    """A's posed triangles of `inst` as a Mesh B can insert (tangents: the bind mesh's, which the host bake keeps)."""
    p = e.read_posed(inst)
    n = len(p)
    return Mesh(p[:, :9].reshape(n, 3, 3), p[:, 9:18].reshape(n, 3, 3), p[:, 18:].reshape(n, 3, 2), bind_mesh.tangents)


def skinning(e):
    return dict(zip(("launches", "triangles", "readbacks"), e.skinning_stats()))


def add_tubes(e, positions, mesh, jt, wt, joints, own_meshes=False):
    e.insert_material(TUBE_MAT, Material(base_color=(0.2, 0.7, 0.3, 1.0)))
    if own_meshes:
        for i in range(len(positions)):
            e.insert_mesh(OWN_MESH + i, mesh)
    else:
        e.insert_mesh(TUBE, mesh)
        e.set_skin(TUBE, jt, wt, joints)
    for i, p in enumerate(positions):
        e.insert_instance(TUBE + i, Instance(OWN_MESH + i if own_meshes else TUBE, TUBE_MAT, tube_xform(*p)))


def follow(a, b, ids, mesh):
    """B re-inserts A's posed triangles of every posed instance (and the instance, so that it is re-baked)."""
    for i, inst in enumerate(ids):
        b.insert_mesh(OWN_MESH + i, posed_mesh(a, inst, mesh))
        b.insert_instance(inst, Instance(OWN_MESH + i, TUBE_MAT, a._xf[inst]))


def remember(e, positions):
    e._xf = {TUBE + i: tube_xform(*p) for i, p in enumerate(positions)}


# ----------------------------------------------------------------------------- 1. kernel bits
def test_posed_bits_equal_numpy_in_fast_and_exact_engines():
    rng = np.random.default_rng(11)
    cases = [(1, 1), (63, 7), (64, 256), (65, 3), (127, 5), (128, 2), (129, 33), (10000, 64)]   # (a workgroup serves 128 triangles of one job)
    engines = {exact: Engine(device=0, exact=exact) for exact in (False, True)}
    try:
        expect = {}
        for e in engines.values():
            e.insert_material(1, Material())
        for k, (n, joints) in enumerate(cases):
            mesh = random_mesh(rng, n)
            jt, wt = random_skin(rng, 3 * n, joints)
            poses = [random_palette(rng, joints) for _ in range(2)]
            for e in engines.values():
                e.insert_mesh(100 + k, mesh); e.set_skin(100 + k, jt, wt, joints)
                for p in range(2):
                    e.insert_instance(1000 + 10 * k + p, Instance(100 + k, 1, tube_xform(3.0 * k, 0, 2.0 * p)))
                    e.set_pose(1000 + 10 * k + p, poses[p])
            for p in range(2):
                expect[1000 + 10 * k + p] = skin(bind_store(mesh), jt, wt, poses[p])
        for e in engines.values():
            e.tick()
            assert skinning(e)["launches"] == 1, "one launch covers every instance posed in a tick"
        for inst, want in expect.items():
            got = {exact: e.read_posed(inst) for exact, e in engines.items()}
            assert got[True].tobytes() == got[False].tobytes(), f"instance {inst}: fast and exact engines pose different bits"
            bad = np.flatnonzero(np.any(got[True].view(np.uint32) != want.view(np.uint32), axis=1))
            assert bad.size == 0, f"instance {inst}: {bad.size} triangles differ from the numpy restatement (first {bad[:5]})"
    finally:
        for e in engines.values():
            e.close()


# ----------------------------------------------------------------------------- 2. everything downstream, exact build
def frame_planes(e, cam, out):
    e.render_camera(cam, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    planes = {b: e.read_buffer(cam, b) for b in Buffer}
    planes["frame"] = out.cpu().numpy().copy()
    return planes


@pytest.mark.parametrize("mode_a,mode_b", [(REFIT_DEVICE, REFIT), (REBUILD, REBUILD)])
def test_downstream_bit_equal_to_reinserted_meshes(mode_a, mode_b):
    size = (64, 48)
    positions = [(-0.4, 0.0, 0.0), (0.4, 0.0, -0.3)]
    mesh, jt, wt = scenes.skinned_tube(24, 12, 6, length=1.2)
    a, b = Engine(device=0, exact=True), Engine(device=0, exact=True)
    try:
        for e, own in ((a, False), (b, True)):
            scenes.build_cornell(e); e.set_seed(3)
            e.set_bvh_refresh(mode_a if e is a else mode_b)
            add_tubes(e, positions, mesh, jt, wt, 6, own_meshes=own)
            remember(e, positions)
        a._xf = b._xf
        desc = scenes.cornell_camera(size, CameraMode.IMAGE)
        cams = [e.create_camera(desc) for e in (a, b)]
        outs = [torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        ids = [TUBE + i for i in range(len(positions))]
        for e in (a, b):
            e.tick()
        refits0 = b.bvh_refits()
        for step in range(12):
            for i, inst in enumerate(ids):
                a.set_pose(inst, scenes.bend_pose(6, 1.2, 0.4 * step + i, length=1.2))
            a.tick()
            follow(a, b, ids, mesh)
            b.tick()
            if step == 0 and mode_b == REFIT:
                assert b.bvh_refits()[1] > refits0[1], "engine B must refit (the comparison is device refit against host refit)"
            pa, pb = frame_planes(a, cams[0], outs[0]), frame_planes(b, cams[1], outs[1])
            for k in pa:
                assert pa[k].tobytes() == pb[k].tobytes(), f"step {step}: {getattr(k, 'name', k)} differs"
        for what in (0, 1):
            assert a.read_scene(what).tobytes() == b.read_scene(what).tobytes(), f"read_scene({what})"
        if mode_a == REFIT_DEVICE:
            assert skinning(a)["readbacks"] >= 1   # (the debug read above brought the host arrays up to date)
    finally:
        a.close(); b.close()


# ----------------------------------------------------------------------------- 3. the device path is really taken
DUNGEON_TUBES = [(-5.75 + 0.7 * (k % 4 - 1.5), 0.0, -19.0 - 0.9 * (k // 4)) for k in range(16)]


def tube_rays(rng, n, origin=(-5.75, 0.5, -16.8)):
    o = np.asarray(origin, np.float32)
    targets = np.asarray([DUNGEON_TUBES[k] for k in rng.integers(0, 16, n)], np.float32) + rng.uniform([-0.4, 0.0, -0.4], [0.4, 2.0, 0.4], (n, 3)).astype(np.float32)
    d = targets - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(n, RAY_DTYPE)
    rays["origin"] = o; rays["direction"] = d; rays["t_max"] = np.float32(3.0e38)
    return rays


def trace(e, rays, stream=None):
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    hits = torch.zeros((len(rays) * HIT_DTYPE.itemsize,), dtype=torch.uint8, device="cuda")
    e.trace_rays(d_rays.data_ptr(), len(rays), hits.data_ptr(), stream=(stream or torch.cuda.current_stream()).cuda_stream)
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(HIT_DTYPE)


def test_device_path_is_taken_and_queries_agree():
    mesh, jt, wt = scenes.skinned_tube(128, 32, 32)
    a, b = Engine(device=0), Engine(device=0)
    try:
        for e, own in ((a, False), (b, True)):
            scenes.build_dungeon(e)
            add_tubes(e, DUNGEON_TUBES, mesh, jt, wt, 32, own_meshes=own)
            remember(e, DUNGEON_TUBES)
            e.tick()
        ids = [TUBE + i for i in range(16)]
        rebuilds0, builds0, trefits0 = a.bvh_refits()[0], a.device_builds(), a.device_tree_refits()
        bakes = a.device_bakes()[0]
        for step in range(20):
            for i, inst in enumerate(ids):
                a.set_pose(inst, scenes.bend_pose(32, 1.5, 0.3 * step + i))
            a.tick()
            now = a.device_bakes()[0]
            assert now > bakes, f"step {step}: no device bake"
            bakes = now
            assert a.device_builds() + a.device_tree_refits() == builds0 + trefits0 + step + 1, f"step {step}: not a device build or device-tree refit"
        st = skinning(a)
        assert st["launches"] == 20 and st["readbacks"] == 0, st
        assert st["triangles"] == 20 * 16 * 8192
        assert a.bvh_refits()[0] == rebuilds0, "a host rebuild happened"
        follow(a, b, ids, mesh)
        b.tick()
        rays = tube_rays(np.random.default_rng(4), 4096)
        got, exp = trace(a, rays), trace(b, rays)
        agree = got["hit"] == exp["hit"]
        assert agree.mean() >= AGREE, agree.mean()
        same = (got["instance"] == exp["instance"]) | ~agree
        assert same.mean() >= AGREE and (got["instance"] >= TUBE).sum() > 1000
        assert skinning(a)["readbacks"] == 0
    finally:
        a.close(); b.close()


# ----------------------------------------------------------------------------- 4. host-path modes give the same result
@pytest.mark.parametrize("setup", ["exact_auto_small", "rebuild", "no_device_bake", "heatmap"])
def test_host_path_modes_match_reinserted_meshes(setup):
    mesh, jt, wt = scenes.skinned_tube(16, 8, 4, length=1.0)
    positions = [(-0.3, 0.0, 0.0), (0.3, 0.0, 0.0)]
    exact = setup != "heatmap"
    a, b = Engine(device=0, exact=exact), Engine(device=0, exact=exact)
    try:
        for e, own in ((a, False), (b, True)):
            if setup == "heatmap":
                scenes.build_dungeon(e)
                e.create_camera(scenes.dungeon_camera((32, 32), CameraMode.BVH_HEATMAP))
            else:
                scenes.build_cornell(e)
            if setup == "rebuild":
                e.set_bvh_refresh(REBUILD)
            if setup == "no_device_bake":
                e.set_bvh_refresh(REFIT_DEVICE); e.set_tuning(device_bake=0)
            add_tubes(e, positions, mesh, jt, wt, 4, own_meshes=own)
            remember(e, positions)
            e.tick()
        ids = [TUBE, TUBE + 1]
        for step in range(4):
            for i, inst in enumerate(ids):
                a.set_pose(inst, scenes.bend_pose(4, 1.0, step + i, length=1.0))
            a.tick()
            follow(a, b, ids, mesh)
            b.tick()
            for what in (0, 1):
                assert a.read_scene(what).tobytes() == b.read_scene(what).tobytes(), f"step {step}: read_scene({what})"
        assert skinning(a)["readbacks"] > 0
    finally:
        a.close(); b.close()


# ----------------------------------------------------------------------------- 5. picks and AOVs see the pose after its tick
def test_picks_and_aovs_see_the_pose_after_its_tick():
    size = (48, 48)
    mesh, jt, wt = scenes.skinned_tube(32, 12, 8, length=1.2)
    e = Engine(device=0)
    try:
        scenes.build_cornell(e)
        add_tubes(e, [(0.0, 0.0, 0.0)], mesh, jt, wt, 8)
        cam = e.create_camera(scenes.cornell_camera(size, CameraMode.REFERENCE, depth=0))
        out = torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda")
        px = np.stack(np.meshgrid(np.arange(size[0]), np.arange(size[1])), -1).reshape(-1, 2).astype(np.uint32)
        d_px = torch.from_numpy(px.reshape(-1).copy()).cuda()
        hits = torch.zeros((len(px) * HIT_DTYPE.itemsize,), dtype=torch.uint8, device="cuda")

        def look():
            e.render_camera(cam, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            e.pick(cam, d_px.data_ptr(), len(px), hits.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
            planes = aov_planes(size, kinds=(Aov.INSTANCE,))
            e.render_aovs(cam, planes)
            torch.cuda.synchronize()
            return hits.cpu().numpy().view(HIT_DTYPE).copy(), planes[Aov.INSTANCE].cpu().numpy().copy()

        e.tick()
        h0, a0 = look()
        e.set_pose(TUBE, scenes.bend_pose(8, 2.5, 1.5707963, length=1.2))
        h1, a1 = look()                                   # set, not ticked: nothing changes
        assert h1.tobytes() == h0.tobytes() and a1.tobytes() == a0.tobytes()
        e.tick()
        h2, a2 = look()
        new = (h2["instance"] == TUBE) & (h0["instance"] != TUBE)
        assert new.any(), "no pixel sees the bent tube after the pose's tick"
        assert np.all(h2["triangle"][new] < len(mesh.positions))
        assert np.any(a2.reshape(-1)[new] != a0.reshape(-1)[new]) and np.all(a2.reshape(-1)[new] == TUBE)
    finally:
        e.close()


# ----------------------------------------------------------------------------- 6. lifecycle
def test_lifecycle_and_errors():
    mesh, jt, wt = scenes.skinned_tube(8, 6, 4)
    bind = bind_store(mesh)
    e = Engine(device=0)
    try:
        scenes.build_cornell(e)
        add_tubes(e, [(0, 0, 0), (0.5, 0, 0)], mesh, jt, wt, 4)
        e.insert_mesh(1, mesh)   # a mesh without a skin
        e.insert_instance(50, Instance(1, TUBE_MAT, tube_xform(1, 0, 0)))
        e.tick()
        p1, p2 = scenes.bend_pose(4, 1.0, 0.2), scenes.bend_pose(4, -0.7, 1.1)
        # errors
        flat = palette12(p1).reshape(-1)
        ptr = flat.ctypes.data_as(C.POINTER(C.c_float))
        assert e._b.instance_set_pose(e._h, 999, ptr, 4) == 1          # unknown instance
        assert e._b.instance_set_pose(e._h, 50, ptr, 4) == 1           # mesh without a skin
        assert e._b.instance_set_pose(e._h, TUBE, ptr, 3) == 1         # joint_count differs from the skin's
        bad = flat.copy(); bad[5] = np.nan
        assert e._b.instance_set_pose(e._h, TUBE, bad.ctypes.data_as(C.POINTER(C.c_float)), 4) == 1
        bad[5] = np.inf
        assert e._b.instance_set_pose(e._h, TUBE, bad.ctypes.data_as(C.POINTER(C.c_float)), 4) == 1
        with pytest.raises(StrolleError):
            e.read_posed(TUBE)                                          # no pose yet
        # of two poses before one tick the last wins
        e.set_pose(TUBE, p1); e.set_pose(TUBE, p2); e.set_pose(TUBE + 1, p1)
        e.tick()
        assert e.read_posed(TUBE).tobytes() == skin(bind, jt, wt, p2).tobytes()
        assert skinning(e)["launches"] == 1
        # set_pose(None) restores the bind-pose triangles bit for bit
        tri0 = e.read_scene(1).copy()
        e.set_pose(TUBE + 1, None); e.tick()
        with pytest.raises(StrolleError):
            e.read_posed(TUBE + 1)
        ref = Engine(device=0)
        scenes.build_cornell(ref)
        add_tubes(ref, [(0, 0, 0), (0.5, 0, 0)], mesh, jt, wt, 4)
        ref.insert_mesh(1, mesh); ref.insert_instance(50, Instance(1, TUBE_MAT, tube_xform(1, 0, 0)))
        ref.set_pose(TUBE, p2); ref.tick()
        assert e.read_scene(1).tobytes() == ref.read_scene(1).tobytes(), "bind pose restored"
        assert e.read_scene(1).tobytes() != tri0.tobytes()
        ref.close()
        # an instance re-insert with the same mesh keeps its pose; with another mesh it drops it
        e.insert_instance(TUBE, Instance(TUBE, TUBE_MAT, tube_xform(0, 0.1, 0))); e.tick()
        assert e.read_posed(TUBE).tobytes() == skin(bind, jt, wt, p2).tobytes()
        # a mesh re-insert drops the skin and the poses
        e.set_pose(TUBE + 1, p1); e.tick()
        e.insert_mesh(TUBE, mesh); e.tick()
        for inst in (TUBE, TUBE + 1):
            with pytest.raises(StrolleError):
                e.read_posed(inst)
        with pytest.raises(StrolleError):
            e.set_pose(TUBE, p1)                                        # no skin any more
        e.set_skin(TUBE, jt, wt, 4)
        e.set_pose(TUBE, p1); e.set_pose(TUBE + 1, p2); e.tick()
        e.insert_instance(TUBE + 1, Instance(1, TUBE_MAT, tube_xform(0.5, 0, 0))); e.tick()
        with pytest.raises(StrolleError):
            e.read_posed(TUBE + 1)
        # removing an instance mid-animation
        for step in range(3):
            if step < 2:
                e.set_pose(TUBE, scenes.bend_pose(4, 0.5, step))
            if step == 1:
                e.remove_instance(TUBE)
            e.tick()
        with pytest.raises(StrolleError):
            e.read_posed(TUBE)
    finally:
        e.close()


def test_despawn_and_spawn_during_animation_under_auto():
    mesh, jt, wt = scenes.skinned_tube(64, 16, 8)
    a, b = Engine(device=0), Engine(device=0)
    try:
        for e, own in ((a, False), (b, True)):
            scenes.build_dungeon(e)
            add_tubes(e, DUNGEON_TUBES[:4], mesh, jt, wt, 8, own_meshes=own)
            remember(e, DUNGEON_TUBES[:4])
            e.tick()
        ids = [TUBE + i for i in range(4)]
        for step in range(6):
            if step == 2:
                for e in (a, b):
                    e.remove_instance(TUBE + 1)
                ids.remove(TUBE + 1)
            if step == 4:
                pos = DUNGEON_TUBES[5]
                for e, m in ((a, TUBE), (b, OWN_MESH + 9)):
                    if e is b:
                        e.insert_mesh(m, mesh)
                    e.insert_instance(TUBE + 9, Instance(m, TUBE_MAT, tube_xform(*pos)))
                a._xf[TUBE + 9] = tube_xform(*pos)
                ids.append(TUBE + 9)
            for i, inst in enumerate(ids):
                a.set_pose(inst, scenes.bend_pose(8, 1.0, step + i))
            a.tick()
            for i, inst in enumerate(ids):
                h = OWN_MESH + (9 if inst == TUBE + 9 else inst - TUBE)
                b.insert_mesh(h, posed_mesh(a, inst, mesh))
                b.insert_instance(inst, Instance(h, TUBE_MAT, a._xf[inst]))
            b.tick()
        assert a.read_scene(1).tobytes() == b.read_scene(1).tobytes()
    finally:
        a.close(); b.close()


# ----------------------------------------------------------------------------- 7. store growth
def test_store_growth_keeps_posed_triangles():
    """A bakes posed and moved instances on the device (ST_BVH_REFIT_DEVICE); C is the same engine with the host baking (device_bake = 0).
    New posed instances grow the posed store, new moving instances with new meshes grow the device mesh store; the device stream each bake
    patched and the host arrays stay equal, and the posed triangles stay numpy's."""
    mesh, jt, wt = scenes.skinned_tube(16, 8, 6)
    bind = bind_store(mesh)
    a, c = Engine(device=0, exact=True), Engine(device=0, exact=True)
    extra_meshes = [scenes.skinned_tube(4 * step, 8, 2, radius=0.1, length=0.5)[0] for step in range(1, 8)]   # 64 x step triangles each
    try:
        for e in (a, c):
            scenes.build_dungeon(e)
            e.set_bvh_refresh(REFIT_DEVICE)
            add_tubes(e, DUNGEON_TUBES[:3], mesh, jt, wt, 6)
            e.tick()
        c.set_tuning(device_bake=0)
        extra = []
        for step in range(8):
            n_posed = 3 + step
            if step >= 1:   # spawns: a posed instance to be (its pose comes two ticks later), a moving instance with a new mesh
                h = 9000 + step
                for e in (a, c):
                    e.insert_instance(TUBE + 2 + step, Instance(TUBE, TUBE_MAT, tube_xform(*DUNGEON_TUBES[(2 + step) % 16])))
                    e.insert_mesh(h, extra_meshes[step - 1])
                    e.insert_instance(h, Instance(h, TUBE_MAT, tube_xform(-5.0, 1.0, -25.0 - step)))
                    e.tick()
                extra.append(h)
            # two ticks of moves and poses: the first sends the copy the spawn did not write whole, the second is baked on the device — its
            # skin launch grows the posed store (the new instance's first pose), its bake appends the new mesh to the device mesh store
            for k in range(2):
                poses = {TUBE + i: scenes.bend_pose(6, 1.0, step + i + 0.5 * k) for i in range(n_posed - (1 if (step >= 1 and k == 0) else 0))}
                bakes = a.device_bakes()[0]
                for e in (a, c):
                    for h in extra:
                        e.insert_instance(h, Instance(h, TUBE_MAT, tube_xform(-5.0 + 0.1 * step + 0.05 * k, 1.0, -25.0 - h % 10)))
                    for inst, p in poses.items():
                        e.set_pose(inst, p)
                    e.tick()
                if k == 1:
                    assert a.device_bakes()[0] > bakes, f"step {step}: the tick was not baked on the device"
                for inst, p in poses.items():
                    assert a.read_posed(inst).tobytes() == skin(bind, jt, wt, p).tobytes(), f"step {step}.{k}: instance {inst}"
                assert a.read_scene(6).tobytes() == c.read_scene(6).tobytes(), f"step {step}.{k}: device streams differ"
        assert skinning(c)["readbacks"] > 0
        assert a.read_scene(1).tobytes() == c.read_scene(1).tobytes()
    finally:
        a.close(); c.close()


def test_pending_move_after_a_mesh_of_another_size():
    """An instance moved on the device stays pending for the other scene copy; its mesh is then re-inserted with another triangle count while
    it is left alone, and another instance moves. The pending bake must use the mesh version the instance was baked from (its slots' size)."""
    rng = np.random.default_rng(5)
    big, small = random_mesh(rng, 300), random_mesh(rng, 120)
    a, c = Engine(device=0, exact=True), Engine(device=0, exact=True)
    try:
        for e in (a, c):
            scenes.build_cornell(e)
            e.set_bvh_refresh(REFIT_DEVICE)
            e.insert_material(TUBE_MAT, Material())
            e.insert_mesh(1, big); e.insert_mesh(2, big)
            e.insert_instance(1, Instance(1, TUBE_MAT, tube_xform(0, 0.5, 0, 0.2)))
            e.insert_instance(2, Instance(2, TUBE_MAT, tube_xform(0.5, 0.5, 0, 0.2)))
            e.tick()
            for k in range(2):   # two moves: both scene copies hold the current tree, so the next moves are baked on the device
                e.insert_instance(2, Instance(2, TUBE_MAT, tube_xform(0.5, 0.5 + 0.01 * k, 0, 0.2)))
                e.tick()
        c.set_tuning(device_bake=0)
        bakes = a.device_bakes()[0]
        for e in (a, c):
            e.insert_instance(1, Instance(1, TUBE_MAT, tube_xform(0.1, 0.5, 0, 0.2)))   # X moves: one copy bakes it, the other keeps it pending
            e.tick()
            e.insert_mesh(1, small)                                                    # X's mesh changes size, X is left alone
            e.insert_instance(2, Instance(2, TUBE_MAT, tube_xform(0.6, 0.5, 0, 0.2)))  # Y moves: the other copy bakes Y and the pending X
            e.tick()
        assert a.device_bakes()[0] >= bakes + 2, "the moves must be baked on the device"
        assert a.read_scene(6).tobytes() == c.read_scene(6).tobytes(), "the device stream after the pending bake"
        for e in (a, c):
            e.insert_instance(1, Instance(1, TUBE_MAT, tube_xform(0.2, 0.5, 0, 0.2)))   # X is re-baked from its new mesh
            e.tick()
        assert a.read_scene(6).tobytes() == c.read_scene(6).tobytes()
        # (the host stream, not the host triangle array: X's old slots are dead now and keep whichever bake last wrote them, which the two
        # engines do differently — the device-baking engine's host copy of a device-moved instance is caught up only while it is live)
        assert a.read_scene(0).tobytes() == c.read_scene(0).tobytes()
    finally:
        a.close(); c.close()


# ----------------------------------------------------------------------------- 8. stream order
def test_tick_on_one_stream_query_on_another():
    mesh, jt, wt = scenes.skinned_tube(64, 16, 8)
    rays = tube_rays(np.random.default_rng(8), 1024)

    def run(sync):
        e = Engine(device=0)
        scenes.build_dungeon(e)
        add_tubes(e, DUNGEON_TUBES[:8], mesh, jt, wt, 8)
        cam = e.create_camera(scenes.dungeon_camera((64, 64), CameraMode.REFERENCE))
        e.tick()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        out = torch.zeros((64, 64, 4), dtype=torch.float32, device="cuda")
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        hits = [torch.zeros((len(rays) * HIT_DTYPE.itemsize,), dtype=torch.uint8, device="cuda") for _ in range(8)]
        torch.cuda.synchronize()
        for it in range(8):
            for i in range(8):
                e.set_pose(TUBE + i, scenes.bend_pose(8, 2.0, it + i))
            e.tick(s1.cuda_stream)
            if sync: torch.cuda.synchronize()
            e.trace_rays(d_rays.data_ptr(), len(rays), hits[it].data_ptr(), stream=s2.cuda_stream)
            if sync: torch.cuda.synchronize()
            e.render_camera(cam, out.data_ptr(), s2.cuda_stream)
            if sync: torch.cuda.synchronize()
        torch.cuda.synchronize()
        res = [h.cpu().numpy().view(HIT_DTYPE).copy() for h in hits]
        e.close()
        return res

    free, ordered = run(False), run(True)
    for it in range(8):
        assert free[it].tobytes() == ordered[it].tobytes(), f"iteration {it}: the query on another stream saw another pose"
    assert any(not np.array_equal(ordered[0]["t"], r["t"]) for r in ordered[1:]), "the poses changed nothing"
