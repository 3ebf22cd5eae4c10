"""GPU tests of morph targets (include/strolle_hip.h "morph targets"; k_skin.hip k_morph, st_deform.cpp).

Engine A morphs on the device: targets per mesh, weights per instance. The posed store's bits are tests/morph_ref.py's (and skin_ref's behind
it where the instance has a pose too); everything downstream is what a second engine gives in which the numpy-morphed triangles were
st_mesh_insert-ed; deformation motion follows tests/deform_ref.py's formula with the previous tick's posed positions."""
import ctypes as C

import numpy as np
import pytest
import torch

import morph_ref
import test_gpu_deform_motion as dm
from skin_ref import bind_store, skin
from strolle_amd import Aov, Buffer, CameraMode, Engine, Instance, Material, Mesh, StrolleError, aov_planes, scenes
from strolle_amd.api import HIT_DTYPE, RAY_DTYPE

pytestmark = pytest.mark.gpu

REBUILD, REFIT, REFIT_DEVICE, AUTO = 0, 1, 2, 4
TUBE, TUBE_MAT, OWN_MESH = 7000, 7000, 8000
JOINTS, LENGTH = 6, 1.2


def tube_xform(x, y, z, s=1.0):
    return np.array([[s, 0, 0, x], [0, s, 0, y], [0, 0, s, z]], np.float32)


def random_mesh(rng, n):
    pos = rng.uniform(-1, 1, (n, 3, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3, 3)); nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    return Mesh(pos, nrm.astype(np.float32), rng.uniform(0, 1, (n, 3, 2)).astype(np.float32))


def random_targets(rng, k, n):
    return rng.uniform(-0.3, 0.3, (k, n, 3, 3)).astype(np.float32), rng.uniform(-0.5, 0.5, (k, n, 3, 3)).astype(np.float32)


def weight_sets(rng, k):
    """Zeros among them, a negative weight, a weight above 1; with one target: each of the three in turn."""
    if k == 1:
        return [np.float32([-0.75]), np.float32([1.5]), np.float32([1.0])]
    a = rng.uniform(0.1, 1.0, k).astype(np.float32)
    a[rng.permutation(k)[: k // 3 + 1]] = 0.0
    nz = np.flatnonzero(a)
    a[nz[0]] = -0.6; a[nz[-1]] = 1.7
    b = rng.uniform(-1.0, 2.0, k).astype(np.float32)       # every target active
    return [a, b]


def morphing(e):
    return dict(zip(("ticks", "triangles", "bytes"), e.morphing_stats()))


def mesh_of(store, like):
    n = len(store)
    return Mesh(store[:, :9].reshape(n, 3, 3), store[:, 9:18].reshape(n, 3, 3), store[:, 18:].reshape(n, 3, 2), like.tangents)


def assert_bits(got, want, what):
    bad = np.flatnonzero(np.any(got.view(np.uint32) != want.view(np.uint32), axis=1))
    assert bad.size == 0, f"{what}: {bad.size} triangles differ from the numpy restatement (first {bad[:5]})"


def tube(segments=8, sides=6, joints=JOINTS):
    mesh, jt, wt = scenes.skinned_tube(segments, sides, joints, length=LENGTH)
    dp, dn = scenes.tube_morph_targets(mesh, length=LENGTH)
    return mesh, jt, wt, dp, dn


def tube_weights(step, i):
    return np.float32([0.6 * np.sin(0.9 * step + i), 0.0 if (step + i) % 3 == 0 else 0.8 * np.cos(0.7 * step + 2 * i), 1.3 * np.sin(0.5 * step + 1.0 + i) ** 2])


# ----------------------------------------------------------------------------- 1. kernel bits
def test_posed_bits_equal_numpy_in_fast_and_exact_engines():
    rng = np.random.default_rng(21)
    cases = [(1, 1), (127, 3), (128, 64), (129, 3), (300, 64), (300, 1)]   # (triangles, targets): a workgroup serves 128 triangles of one job
    engines = {exact: Engine(device=0, exact=exact) for exact in (False, True)}
    try:
        expect, total = {}, 0
        for e in engines.values():
            e.insert_material(1, Material())
        for c, (n, k) in enumerate(cases):
            mesh = random_mesh(rng, n)
            mesh.positions[0, 0, 0] = -0.0                                  # a sign bit a multiplied-in zero weight would flip
            dp, dn = random_targets(rng, k, n)
            dn[0, 0, 1] = -mesh.normals[0, 1]                                # a normal that cancels at weight 1 (the one-target cases have that set)
            sets = weight_sets(rng, k)
            for e in engines.values():
                e.insert_mesh(100 + c, mesh); e.set_morph_targets(100 + c, dp, dn)
                for p, w in enumerate(sets):
                    e.insert_instance(1000 + 10 * c + p, Instance(100 + c, 1, tube_xform(3.0 * c, 0, 2.0 * p)))
                    e.set_morph_weights(1000 + 10 * c + p, w)
            for p, w in enumerate(sets):
                expect[1000 + 10 * c + p] = morph_ref.morph(bind_store(mesh), dp, dn, w)
            total += n * len(sets)
        for e in engines.values():
            e.tick()
            st = morphing(e)
            assert st["ticks"] == 1 and st["triangles"] == total, st
            assert st["bytes"] == sum(k * ((n + 127) // 128 * 128) * 72 for n, k in cases), st
            assert e.skinning_stats()[:2] == (0, 0), "morph-only instances went through no skin stage"
        for inst, want in expect.items():
            got = {exact: e.read_posed(inst) for exact, e in engines.items()}
            assert got[True].tobytes() == got[False].tobytes(), f"instance {inst}: fast and exact engines morph different bits"
            assert_bits(got[True], want, f"instance {inst}")
    finally:
        for e in engines.values():
            e.close()


def test_morph_then_skin_bits_equal_numpy():
    mesh, jt, wt, dp, dn = tube(8, 6, 32)
    bind = bind_store(mesh)
    engines = {exact: Engine(device=0, exact=exact) for exact in (False, True)}
    try:
        w = [np.float32([0.5, -0.4, 1.2]), np.float32([0.0, 0.9, 0.0]), np.float32([0.0, 0.0, 0.0])]
        poses = [scenes.bend_pose(32, 1.5, 0.3 + i, length=LENGTH) for i in range(3)]
        for e in engines.values():
            e.insert_material(1, Material())
            e.insert_mesh(TUBE, mesh); e.set_skin(TUBE, jt, wt, 32); e.set_morph_targets(TUBE, dp, dn)
            for i in range(3):
                e.insert_instance(TUBE + i, Instance(TUBE, 1, tube_xform(i, 0, 0)))
                e.set_morph_weights(TUBE + i, w[i]); e.set_pose(TUBE + i, poses[i])
            e.tick()
            assert morphing(e)["triangles"] == 2 * len(bind) and e.skinning_stats()[:2] == (1, 3 * len(bind))
        for i in range(3):
            got = {exact: e.read_posed(TUBE + i) for exact, e in engines.items()}
            assert got[True].tobytes() == got[False].tobytes()
            assert_bits(got[True], morph_ref.morph_skin(bind, dp, dn, w[i], jt, wt, poses[i]), f"instance {i}")
        assert engines[True].read_posed(TUBE + 2).tobytes() == skin(bind, jt, wt, poses[2]).tobytes(), "no non-zero weight: skinned as without targets"
    finally:
        for e in engines.values():
            e.close()


def test_instances_share_a_morphed_mesh():
    rng = np.random.default_rng(5)
    mesh = random_mesh(rng, 129)
    dp, dn = random_targets(rng, 3, 129)
    bind = bind_store(mesh)
    e, ref = Engine(device=0, exact=True), Engine(device=0, exact=True)
    try:
        w = [np.float32([0.3, 0.0, -1.1]), np.float32([0.0, 2.0, 0.5])]
        for x in (e, ref):
            scenes.build_cornell(x)
            x.insert_material(TUBE_MAT, Material())
        e.insert_mesh(TUBE, mesh); e.set_morph_targets(TUBE, dp, dn)
        for i in range(3):
            e.insert_instance(TUBE + i, Instance(TUBE, TUBE_MAT, tube_xform(0.3 * i - 0.3, 0.5, 0, 0.2)))
            h = OWN_MESH + i
            ref.insert_mesh(h, mesh if i == 2 else mesh_of(morph_ref.morph(bind, dp, dn, w[i]), mesh))
            ref.insert_instance(TUBE + i, Instance(h, TUBE_MAT, tube_xform(0.3 * i - 0.3, 0.5, 0, 0.2)))
        e.set_morph_weights(TUBE, w[0]); e.set_morph_weights(TUBE + 1, w[1])
        e.tick(); ref.tick()
        for i in range(2):
            assert_bits(e.read_posed(TUBE + i), morph_ref.morph(bind, dp, dn, w[i]), f"instance {i}")
        with pytest.raises(StrolleError):
            e.read_posed(TUBE + 2)                                              # no weights: the base mesh, no posed region
        assert e.read_scene(1).tobytes() == ref.read_scene(1).tobytes(), "the third instance is not the base mesh bit for bit"
    finally:
        e.close(); ref.close()


# ----------------------------------------------------------------------------- 2. everything downstream, exact build
def add_tubes(e, positions, mesh, own_meshes=False, skin_of=None, targets=None):
    e.insert_material(TUBE_MAT, Material(base_color=(0.2, 0.7, 0.3, 1.0)))
    if own_meshes:
        for i in range(len(positions)):
            e.insert_mesh(OWN_MESH + i, mesh)
    else:
        e.insert_mesh(TUBE, mesh)
        if skin_of is not None:
            e.set_skin(TUBE, *skin_of)
        if targets is not None:
            e.set_morph_targets(TUBE, *targets)
    for i, p in enumerate(positions):
        e.insert_instance(TUBE + i, Instance(OWN_MESH + i if own_meshes else TUBE, TUBE_MAT, tube_xform(*p)))


def follow(b, positions, stores, mesh):
    """B re-inserts the numpy-deformed triangles of every instance (and the instance, so that it is re-baked)."""
    for i, store in enumerate(stores):
        b.insert_mesh(OWN_MESH + i, mesh_of(store, mesh))
        b.insert_instance(TUBE + i, Instance(OWN_MESH + i, TUBE_MAT, tube_xform(*positions[i])))


@pytest.mark.parametrize("mode_a,mode_b", [(REFIT_DEVICE, REFIT), (REBUILD, REBUILD)])
def test_downstream_bit_equal_to_reinserted_meshes(mode_a, mode_b):
    """Instance 0 morphs only, instance 1 morphs and is skinned."""
    size = (64, 48)
    positions = [(-0.4, 0.0, 0.0), (0.4, 0.0, -0.3)]
    mesh, jt, wt, dp, dn = tube(12, 8)
    bind = bind_store(mesh)
    a, b = Engine(device=0, exact=True), Engine(device=0, exact=True)
    try:
        for e, own in ((a, False), (b, True)):
            scenes.build_cornell(e); e.set_seed(3)
            e.set_bvh_refresh(mode_a if e is a else mode_b)
            add_tubes(e, positions, mesh, own_meshes=own, skin_of=(jt, wt, JOINTS), targets=(dp, dn))
        desc = scenes.cornell_camera(size, CameraMode.IMAGE)
        cams = [e.create_camera(desc) for e in (a, b)]
        outs = [dm.new_out(size) for _ in range(2)]
        for e in (a, b):
            e.tick()
        for step in range(6):
            w = [tube_weights(step, i) for i in range(2)]
            pose = scenes.bend_pose(JOINTS, 1.2, 0.4 * step, length=LENGTH)
            a.set_morph_weights(TUBE, w[0]); a.set_morph_weights(TUBE + 1, w[1]); a.set_pose(TUBE + 1, pose)
            a.tick()
            follow(b, positions, [morph_ref.morph(bind, dp, dn, w[0]), morph_ref.morph_skin(bind, dp, dn, w[1], jt, wt, pose)], mesh)
            b.tick()
            pa, pb = dm.frame_planes(a, cams[0], outs[0]), dm.frame_planes(b, cams[1], outs[1])
            dm.assert_planes_equal(pa, pb, f"step {step}")
        for what in (0, 1):
            assert a.read_scene(what).tobytes() == b.read_scene(what).tobytes(), f"read_scene({what})"
        if mode_a == REFIT_DEVICE:
            assert a.skinning_stats()[2] >= 1   # (the debug read above brought the host arrays up to date: the batched read-back)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("setup", ["exact_auto_small", "rebuild", "no_device_bake", "heatmap"])
def test_host_path_modes_match_reinserted_meshes(setup):
    mesh, jt, wt, dp, dn = tube(8, 6, 4)
    bind = bind_store(mesh)
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
            add_tubes(e, positions, mesh, own_meshes=own, skin_of=(jt, wt, 4), targets=(dp, dn))
            e.tick()
        for step in range(3):
            w = [tube_weights(step, i) for i in range(2)]
            pose = scenes.bend_pose(4, 1.0, step, length=LENGTH)
            a.set_morph_weights(TUBE, w[0]); a.set_morph_weights(TUBE + 1, w[1]); a.set_pose(TUBE + 1, pose)
            a.tick()
            follow(b, positions, [morph_ref.morph(bind, dp, dn, w[0]), morph_ref.morph_skin(bind, dp, dn, w[1], jt, wt, pose)], mesh)
            b.tick()
            for what in (0, 1):
                assert a.read_scene(what).tobytes() == b.read_scene(what).tobytes(), f"step {step}: read_scene({what})"
        assert a.skinning_stats()[2] > 0
    finally:
        a.close(); b.close()


# ----------------------------------------------------------------------------- 3. switching off
def test_zero_weights_are_no_weights():
    size = (64, 48)
    positions = [(-0.4, 0.0, 0.0), (0.4, 0.0, -0.3)]
    mesh, jt, wt, dp, dn = tube(12, 8)
    a, b = Engine(device=0, exact=True), Engine(device=0, exact=True)
    try:
        for e in (a, b):
            scenes.build_cornell(e); e.set_seed(3)
            add_tubes(e, positions, mesh, targets=(dp, dn))
        cams = [e.create_camera(scenes.cornell_camera(size, CameraMode.IMAGE)) for e in (a, b)]
        outs = [dm.new_out(size) for _ in range(2)]
        for step in range(3):
            for i in range(2):
                a.set_morph_weights(TUBE + i, np.float32([0.0, -0.0, 0.0]))     # all exactly zero: nothing to do
            for e in (a, b):
                e.tick()
            dm.assert_planes_equal(dm.frame_planes(a, cams[0], outs[0]), dm.frame_planes(b, cams[1], outs[1]), f"zero weights, frame {step}")
        assert morphing(a) == {"ticks": 0, "triangles": 0, "bytes": 0}
        with pytest.raises(StrolleError):
            a.read_posed(TUBE)
    finally:
        a.close(); b.close()


def test_weights_then_none_is_the_base_scene_again():
    """B inserts the numpy-morphed meshes while A has weights and the base mesh when A drops them: the same pictures all the way."""
    size = (64, 48)
    positions = [(-0.4, 0.0, 0.0), (0.4, 0.0, -0.3)]
    mesh, jt, wt, dp, dn = tube(12, 8)
    bind = bind_store(mesh)
    a, b = Engine(device=0, exact=True), Engine(device=0, exact=True)
    try:
        for e, own in ((a, False), (b, True)):
            scenes.build_cornell(e); e.set_seed(3)
            add_tubes(e, positions, mesh, own_meshes=own, targets=(dp, dn))
            e.tick()
        cams = [e.create_camera(scenes.cornell_camera(size, CameraMode.IMAGE)) for e in (a, b)]
        outs = [dm.new_out(size) for _ in range(2)]
        for cycle, off in enumerate((None, np.zeros(3, np.float32))):
            for step in range(2):
                w = [tube_weights(step + 1 + cycle, i) for i in range(2)]
                for i in range(2):
                    a.set_morph_weights(TUBE + i, w[i])
                follow(b, positions, [morph_ref.morph(bind, dp, dn, w[i]) for i in range(2)], mesh)
                a.tick(); b.tick()
                dm.assert_planes_equal(dm.frame_planes(a, cams[0], outs[0]), dm.frame_planes(b, cams[1], outs[1]), f"cycle {cycle}, morphed frame {step}")
            for i in range(2):
                a.set_morph_weights(TUBE + i, off)
            follow(b, positions, [bind, bind], mesh)
            a.tick(); b.tick()
            with pytest.raises(StrolleError):
                a.read_posed(TUBE)
            for step in range(2):
                dm.assert_planes_equal(dm.frame_planes(a, cams[0], outs[0]), dm.frame_planes(b, cams[1], outs[1]), f"cycle {cycle}, base frame {step}")
            for what in (0, 1):
                assert a.read_scene(what).tobytes() == b.read_scene(what).tobytes(), f"cycle {cycle}: read_scene({what})"
    finally:
        a.close(); b.close()


def test_dropped_weights_give_their_regions_back():
    """With deformation motion on an instance holds two regions. The posed store's size has no reader of its own; a store that outgrows its
    allocation computes every region again, previous ones included, and the triangle counter shows that: regions that did not go back to the
    free list would outgrow the first allocation (1.5 x four regions) in the second cycle."""
    mesh, jt, wt, dp, dn = tube(8, 6)
    n = len(mesh.positions)
    e = Engine(device=0)
    try:
        scenes.build_cornell(e)
        add_tubes(e, [(-0.4, 0.0, 0.0), (0.4, 0.0, -0.3)], mesh, targets=(dp, dn))
        e.set_deformation_motion(True)
        e.tick()
        steady = []
        for cycle in range(6):
            for step in range(3):
                before = morphing(e)["triangles"]
                for i in range(2):
                    e.set_morph_weights(TUBE + i, tube_weights(step + 1, i))
                e.tick()
                if cycle:
                    steady.append(morphing(e)["triangles"] - before)
            assert e.deformation_stats() == (2, 2 * n * 96)
            for i in range(2):
                e.set_morph_weights(TUBE + i, None if cycle % 2 == 0 else np.zeros(3, np.float32))
            e.tick()
            assert e.deformation_stats() == (0, 0), "the previous regions were not given back"
        assert set(steady) == {2 * n}, f"the posed store grew on repetition: {steady}"
        assert morphing(e)["bytes"] == 3 * ((n + 127) // 128 * 128) * 72
    finally:
        e.close()


# ----------------------------------------------------------------------------- 4. picks, queries and AOVs see the weights after their tick
def test_picks_queries_and_aovs_see_the_weights_after_their_tick():
    size = (48, 48)
    mesh, jt, wt, dp, dn = tube(16, 12)
    e = Engine(device=0)
    try:
        scenes.build_cornell(e)
        add_tubes(e, [(0.0, 0.0, 0.0)], mesh, targets=(dp, dn))
        cam = e.create_camera(scenes.cornell_camera(size, CameraMode.REFERENCE, depth=0))
        out = dm.new_out(size)
        px = np.stack(np.meshgrid(np.arange(size[0]), np.arange(size[1])), -1).reshape(-1, 2).astype(np.uint32)
        d_px = torch.from_numpy(px.reshape(-1).copy()).cuda()
        hits = torch.zeros((len(px) * HIT_DTYPE.itemsize,), dtype=torch.uint8, device="cuda")
        rays = np.zeros(256, RAY_DTYPE)
        rays["origin"] = np.float32([0.0, 0.6, 3.0]) + np.random.default_rng(2).uniform(-0.45, 0.45, (256, 3)).astype(np.float32) * np.float32([1, 1, 0])
        rays["direction"] = np.float32([0, 0, -1]); rays["t_max"] = np.float32(3.0e38)
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        ray_hits = torch.zeros((len(rays) * HIT_DTYPE.itemsize,), dtype=torch.uint8, device="cuda")

        def look():
            s = torch.cuda.current_stream().cuda_stream
            e.render_camera(cam, out.data_ptr(), s)
            e.pick(cam, d_px.data_ptr(), len(px), hits.data_ptr(), stream=s)
            e.trace_rays(d_rays.data_ptr(), len(rays), ray_hits.data_ptr(), stream=s)
            planes = aov_planes(size, kinds=(Aov.INSTANCE, Aov.DEPTH))
            e.render_aovs(cam, planes)
            torch.cuda.synchronize()
            return (hits.cpu().numpy().view(HIT_DTYPE).copy(), ray_hits.cpu().numpy().view(HIT_DTYPE).copy(),
                    planes[Aov.INSTANCE].cpu().numpy().copy(), planes[Aov.DEPTH].cpu().numpy().copy())

        e.tick()
        before = look()
        e.set_morph_weights(TUBE, np.float32([1.5, 0.0, 0.0]))      # the bulge
        unticked = look()                                           # set, not ticked: nothing changes
        for x, y in zip(before, unticked):
            assert x.tobytes() == y.tobytes()
        e.tick()
        after = look()
        new = (after[0]["instance"] == TUBE) & (before[0]["instance"] != TUBE)
        assert new.any(), "no pixel sees the bulged tube after the weights' tick"
        assert np.all(after[2].reshape(-1)[new] == TUBE) and np.any(after[3].reshape(-1)[new] != before[3].reshape(-1)[new])
        assert (after[1]["instance"] == TUBE).sum() > (before[1]["instance"] == TUBE).sum(), "the scene query does not see the bulge"
    finally:
        e.close()


# ----------------------------------------------------------------------------- 5. deformation motion
class MorphAnimation(dm.Animation):
    """dm.Animation with morph weights set every tick; `skinned`: the tubes are re-posed too (morph + skin)."""

    def __init__(self, e, size, skinned):
        super().__init__(e, size)
        self.skinned = skinned

    def advance(self, repose=None, stream=None, track=True, weights=True):
        if weights:
            for i, inst in enumerate(self.ids):
                self.e.set_morph_weights(inst, tube_weights(self.step, i) * np.float32(1.5))
        super().advance(repose=self.ids if (self.skinned and weights) else [], stream=stream, track=track)
        if track:
            self.reposed = [inst for inst in self.ids if inst in self.prev_posed and weights]


def build_motion(exact, skinned):
    e = dm.build(exact, True)
    e.set_morph_targets(TUBE, *scenes.tube_morph_targets(e._mesh, length=dm.LENGTH))
    return e


@pytest.mark.parametrize("skinned,exact", [(False, True), (False, False), (True, True), (True, False)], ids=["morph-exact", "morph-fast", "morph+skin-exact", "morph+skin-fast"])
def test_velocity_is_the_stated_formula(skinned, exact):
    e = build_motion(exact, skinned)
    try:
        anim = MorphAnimation(e, dm.SIZE, skinned)
        anim.advance(); anim.render()               # the first tick that deforms has no earlier positions (its frame: the test below)
        assert e.deformation_stats()[0] == 0
        n_tubes, tris = len(e._ids), len(e._mesh.positions)
        for step in range(3):
            anim.advance()
            n, nbytes = e.deformation_stats()
            assert n == n_tubes and nbytes == n_tubes * tris * 96, (n, nbytes)
            dm.check_velocity(anim, anim.render(), exact, f"tick {step}", min_median=1.0)
    finally:
        e.close()


def test_first_tick_and_return_to_base_show_the_rigid_formula():
    e, off = build_motion(True, False), build_motion(True, False)
    try:
        off.set_deformation_motion(False)
        anim, ref = MorphAnimation(e, dm.SIZE, False), MorphAnimation(off, dm.SIZE, False)
        for a in (anim, ref):
            a.advance()
        assert e.deformation_stats() == (0, 0)
        dm.assert_planes_equal(anim.render(), ref.render(), "the first tick that deforms")
        for a in (anim, ref):
            a.advance()
        assert e.deformation_stats()[0] == 2
        pa, pb = anim.render(), ref.render()
        assert pa[Buffer.VELOCITY_MAP].tobytes() != pb[Buffer.VELOCITY_MAP].tobytes()
        for a in (anim, ref):
            for inst in a.ids:
                a.e.set_morph_weights(inst, None)
            a.advance(weights=False)
        assert e.deformation_stats() == (0, 0)
        pa, pb = anim.render(), ref.render()
        # (the planes that depend on this tick's geometry and motion alone: colour history remembers the frame before)
        for plane in (Buffer.VELOCITY_MAP, Buffer.PRIM_GBUFFER_D0_A, Buffer.PRIM_GBUFFER_D0_B, Buffer.PRIM_GBUFFER_D1_A, Buffer.PRIM_GBUFFER_D1_B):
            assert pa[plane].tobytes() == pb[plane].tobytes(), f"the tick that returns to the base shape: {plane.name}"
    finally:
        e.close(); off.close()


def test_previous_regions_survive_posed_store_growth():
    e = build_motion(True, True)
    try:
        anim = MorphAnimation(e, dm.SIZE, True)
        anim.advance(); anim.render()
        anim.advance(); anim.render()
        n = len(e._mesh.positions)
        # six new deforming instances, out of sight: ten regions, more than the allocation holds (1.5 x what the last growth asked for, six at
        # the most) — the tick computes the two visible tubes' current AND previous regions again, which the triangle counter shows
        for k in range(6):
            e.insert_instance(TUBE + 10 + k, Instance(TUBE, TUBE_MAT, tube_xform(0.0, 5.0 + k, 0.0)))
            e.set_morph_weights(TUBE + 10 + k, tube_weights(k, 0))
        before = morphing(e)["triangles"]
        anim.advance()
        assert morphing(e)["triangles"] - before == (2 + 2 + 6) * n, "the posed store did not grow"
        assert e.deformation_stats()[0] == 2
        dm.check_velocity(anim, anim.render(), True, "the tick that grew the store", min_median=1.0)
    finally:
        e.close()


# ----------------------------------------------------------------------------- 6. lifecycle
def test_lifecycle_and_errors():
    mesh, jt, wt, dp, dn = tube(8, 6, 4)
    bind = bind_store(mesh)
    e = Engine(device=0)
    try:
        scenes.build_cornell(e)
        add_tubes(e, [(0, 0, 0), (0.5, 0, 0)], mesh, skin_of=(jt, wt, 4), targets=(dp, dn))
        e.insert_mesh(1, mesh)   # a mesh without targets
        e.insert_instance(50, Instance(1, TUBE_MAT, tube_xform(1, 0, 0)))
        e.tick()
        w1, w2, pose = np.float32([0.5, 0.0, -0.3]), np.float32([0.0, 1.4, 0.2]), scenes.bend_pose(4, 1.0, 0.2, length=LENGTH)

        def status(inst, w, n):
            return e._b.instance_set_morph_weights(e._h, inst, w.ctypes.data_as(C.POINTER(C.c_float)), n)

        assert status(999, w1, 3) == 1                                  # unknown instance
        assert status(50, w1, 3) == 1                                   # mesh without targets
        assert status(TUBE, w1, 2) == 1                                 # target_count differs from the mesh's
        for bad in (np.nan, np.inf):
            w = w1.copy(); w[1] = bad
            assert status(TUBE, w, 3) == 1
        with pytest.raises(StrolleError):
            e.read_posed(TUBE)
        # of two weight sets before one tick the last wins
        e.set_morph_weights(TUBE, w1); e.set_morph_weights(TUBE, w2); e.set_morph_weights(TUBE + 1, w1)
        e.tick()
        assert e.read_posed(TUBE).tobytes() == morph_ref.morph(bind, dp, dn, w2).tobytes()
        assert morphing(e)["ticks"] == 1
        # an instance re-insert with the same mesh keeps its weights; st_mesh_set_skin keeps them too (and drops poses)
        e.insert_instance(TUBE, Instance(TUBE, TUBE_MAT, tube_xform(0, 0.1, 0))); e.tick()
        assert e.read_posed(TUBE).tobytes() == morph_ref.morph(bind, dp, dn, w2).tobytes()
        e.set_pose(TUBE, pose); e.tick()
        assert e.read_posed(TUBE).tobytes() == morph_ref.morph_skin(bind, dp, dn, w2, jt, wt, pose).tobytes()
        e.set_skin(TUBE, jt, wt, 4); e.tick()
        assert e.read_posed(TUBE).tobytes() == morph_ref.morph(bind, dp, dn, w2).tobytes(), "st_mesh_set_skin keeps weights and drops the pose"
        # st_mesh_set_morph_targets replaces the targets, drops the weights and keeps poses
        e.set_pose(TUBE, pose); e.tick()
        e.set_morph_targets(TUBE, dp[:2], dn[:2]); e.tick()
        assert e.read_posed(TUBE).tobytes() == skin(bind, jt, wt, pose).tobytes(), "new targets drop the weights; the pose stays"
        with pytest.raises(StrolleError):
            e.read_posed(TUBE + 1)                                      # it had weights only
        with pytest.raises(StrolleError):
            e.set_morph_weights(TUBE, w1)                               # three weights, two targets
        e.set_morph_weights(TUBE, w1[:2]); e.set_morph_weights(TUBE + 1, w2[:2]); e.tick()
        assert e.read_posed(TUBE).tobytes() == morph_ref.morph_skin(bind, dp[:2], dn[:2], w1[:2], jt, wt, pose).tobytes()
        assert e.read_posed(TUBE + 1).tobytes() == morph_ref.morph(bind, dp[:2], dn[:2], w2[:2]).tobytes()
        # weights None with a pose: skinned as without targets; pose None with weights: the morph alone
        e.set_morph_weights(TUBE, None); e.tick()
        assert e.read_posed(TUBE).tobytes() == skin(bind, jt, wt, pose).tobytes()
        e.set_morph_weights(TUBE, w1[:2]); e.set_pose(TUBE, None); e.tick()
        assert e.read_posed(TUBE).tobytes() == morph_ref.morph(bind, dp[:2], dn[:2], w1[:2]).tobytes()
        # an instance re-insert with another mesh drops the weights
        e.insert_instance(TUBE + 1, Instance(1, TUBE_MAT, tube_xform(0.5, 0, 0))); e.tick()
        with pytest.raises(StrolleError):
            e.read_posed(TUBE + 1)
        # a mesh re-insert drops the targets and the weights
        e.insert_mesh(TUBE, mesh); e.tick()
        with pytest.raises(StrolleError):
            e.read_posed(TUBE)
        with pytest.raises(StrolleError):
            e.set_morph_weights(TUBE, w1[:2])                           # no targets any more
        assert morphing(e)["bytes"] == 0
        # st_mesh_remove drops the targets; st_instance_remove drops the weights
        e.set_morph_targets(TUBE, dp, dn)
        e.set_morph_weights(TUBE, w1); e.tick()
        e.remove_instance(TUBE); e.tick()
        with pytest.raises(StrolleError):
            e.read_posed(TUBE)
        e.insert_instance(TUBE, Instance(TUBE, TUBE_MAT, tube_xform(0, 0, 0))); e.tick()
        with pytest.raises(StrolleError):
            e.read_posed(TUBE)                                          # a new instance under the old id has no weights
        e.set_morph_weights(TUBE, w1); e.tick()
        e.remove_mesh(TUBE)
        assert morphing(e)["bytes"] == 0
        e.insert_mesh(TUBE, mesh)
        with pytest.raises(StrolleError):
            e.set_morph_weights(TUBE, w1)
        e.tick()
    finally:
        e.close()


# ----------------------------------------------------------------------------- 7. stream order
def test_tick_on_one_stream_query_on_another():
    mesh, jt, wt, dp, dn = tube(16, 12, 8)
    positions = [(-5.75 + 0.7 * (k % 4 - 1.5), 0.0, -19.0 - 0.9 * (k // 4)) for k in range(8)]
    rng = np.random.default_rng(8)
    o = np.float32([-5.75, 0.5, -16.8])
    targets = np.asarray([positions[k] for k in rng.integers(0, 8, 1024)], np.float32) + rng.uniform([-0.4, 0.0, -0.4], [0.4, LENGTH, 0.4], (1024, 3)).astype(np.float32)
    d = targets - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(1024, RAY_DTYPE)
    rays["origin"] = o; rays["direction"] = d; rays["t_max"] = np.float32(3.0e38)

    def run(sync):
        e = Engine(device=0)
        scenes.build_dungeon(e)
        add_tubes(e, positions, mesh, skin_of=(jt, wt, 8), targets=(dp, dn))
        cam = e.create_camera(scenes.dungeon_camera((64, 64), CameraMode.REFERENCE))
        e.tick()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        out = torch.zeros((64, 64, 4), dtype=torch.float32, device="cuda")
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        hits = [torch.zeros((len(rays) * HIT_DTYPE.itemsize,), dtype=torch.uint8, device="cuda") for _ in range(8)]
        torch.cuda.synchronize()
        for it in range(8):
            for i in range(8):
                e.set_morph_weights(TUBE + i, tube_weights(it, i) * np.float32(2.0))
                if i % 2:
                    e.set_pose(TUBE + i, scenes.bend_pose(8, 2.0, it + i, length=LENGTH))
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
        assert free[it].tobytes() == ordered[it].tobytes(), f"iteration {it}: the query on another stream saw other weights"
    assert any(not np.array_equal(ordered[0]["t"], r["t"]) for r in ordered[1:]), "the weights changed nothing"


# ----------------------------------------------------------------------------- 8. counters
def test_counters():
    mesh, jt, wt, dp, dn = tube(8, 6, 4)
    n = len(mesh.positions)
    e = Engine(device=0)
    try:
        scenes.build_cornell(e)
        add_tubes(e, [(0, 0, 0), (0.5, 0, 0)], mesh, skin_of=(jt, wt, 4), targets=(dp, dn))
        e.tick()
        assert morphing(e) == {"ticks": 0, "triangles": 0, "bytes": 0}
        e.set_morph_weights(TUBE, np.float32([0.0, 0.0, 0.0])); e.tick()
        assert morphing(e) == {"ticks": 0, "triangles": 0, "bytes": 0}, "no active target: no morph stage, nothing sent"
        # both instances deform once and return to the base shape: the posed store then has room for both regions, so that no later tick of
        # this test has to grow it (a store that grows computes every region again, which the counters rightly show)
        for i in range(2):
            e.set_morph_weights(TUBE + i, np.float32([0.3, 0.0, 0.0]))
        e.tick()
        assert morphing(e) == {"ticks": 1, "triangles": 2 * n, "bytes": 3 * ((n + 127) // 128 * 128) * 72}
        for i in range(2):
            e.set_morph_weights(TUBE + i, None)
        e.tick()
        assert e.skinning_stats()[:2] == (0, 0), "a morph-only instance is no skin stage"

        def counters():
            m = morphing(e)
            return np.array([m["ticks"], m["triangles"], *e.skinning_stats()[:2]], np.int64)

        def step(what):
            before = counters()
            e.tick()
            return tuple(int(x) for x in counters() - before), what

        assert step("nothing set")[0] == (0, 0, 0, 0)
        e.set_morph_weights(TUBE, np.float32([0.0, 0.7, 0.0]))
        assert step("a morph-only instance")[0] == (1, n, 0, 0)
        assert step("nothing changed: nothing runs")[0] == (0, 0, 0, 0)
        e.set_pose(TUBE + 1, scenes.bend_pose(4, 1.0, 0.0, length=LENGTH))
        assert step("a pose alone: k_skin")[0] == (0, 0, 1, n)
        e.set_pose(TUBE, scenes.bend_pose(4, 1.0, 1.0, length=LENGTH))
        assert step("morph + skin: one tick of each counter")[0] == (1, n, 1, n)
        e.set_morph_weights(TUBE, np.float32([0.0, 0.0, 0.0]))
        assert step("the pose stays, skinned by k_skin")[0] == (0, 0, 1, n)
        assert morphing(e)["bytes"] == 3 * ((n + 127) // 128 * 128) * 72
    finally:
        e.close()
