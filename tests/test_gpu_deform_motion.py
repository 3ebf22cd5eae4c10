"""GPU tests of deformation motion (include/strolle_hip.h "skinned meshes", st_engine_set_deformation_motion; st_traverse.h deform_prev_point).

Skinned tubes (scenes.skinned_tube / bend_pose) stand in the Cornell box, in the dungeon, or alone (a scene small enough to live in LDS) and
are re-posed every tick. With the switch off — the default — nothing changes; with it on, the velocity plane and ST_AOV_MOTION of the
pixels on a re-posed tube are the stated formula, evaluated by tests/deform_ref.py from st_camera_pick's (instance, triangle, barycentrics),
st_debug_read_posed of this tick and of the previous one, the camera descriptions and the instance transforms; and the reprojection map
lands on the surface point it came from more often than with the switch off."""
import json
import os

import numpy as np
import pytest
import torch

import deform_ref
from strolle_amd import Aov, Buffer, CameraMode, Engine, Instance, Light, Material, Sun, aov_planes, scenes
from strolle_amd.api import HIT_DTYPE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REBUILD, REFIT, REFIT_DEVICE, AUTO = 0, 1, 2, 4
TUBE, TUBE_MAT = 7000, 7000
JOINTS, LENGTH = 6, 1.2
AGREE = 0.999      # tests/test_gpu_ray_query.py: the share of fast-build picks that resolve a silhouette as the frame does
TOLERANCE = 1e-3   # px: the velocity map's tolerance (test_fast_whole_frames_with_light_and_camera_moving)
# the animation of test 3: chosen so that the median deformation velocity on tube pixels is above 3 px at SIZE (asserted from numpy there)
SIZE = (256, 192)
ANGLE, PHASE_STEP = 1.6, 0.7


def _tube_alone(e):
    """No scene but the tube: 32 triangles, a BVH stream that fits LDS (k_common.h scene_fits_lds) — the LDS_SCENE instantiations."""
    e.set_blue_noise(scenes.load_blue_noise())
    e.insert_light(1, Light.point((0.5, 1.5, 1.5), 0.15, (4.0,) * 3, 20.0))
    e.update_sun(Sun(azimuth=0.0, altitude=-1.0))


# scene: (builder, tube positions, tube (segments, sides), camera eye, camera target)
SCENES = {
    "cornell": (scenes.build_cornell, [(-0.4, 0.0, 0.0), (0.4, 0.0, -0.3)], (24, 12), (0.0, 1.0, 3.2), (0.0, 1.0, 0.0)),
    "dungeon": (scenes.build_dungeon, [(-6.1, 0.0, -19.0), (-5.4, 0.0, -19.0)], (24, 12), (-5.75, 0.5, -16.8), (-5.75, 0.5, -17.0)),
    "lds": (_tube_alone, [(0.0, 0.4, 0.0)], (4, 4), (0.0, 1.0, 3.2), (0.0, 1.0, 0.0)),
}
POSITIONS = SCENES["cornell"][1]
IDS = [TUBE, TUBE + 1]


def tube_xform(x, y, z):
    return np.array([[1, 0, 0, x], [0, 1, 0, y], [0, 0, 1, z]], np.float32)


def pose(step, i):
    return scenes.bend_pose(JOINTS, ANGLE, PHASE_STEP * step + i, length=LENGTH)


def build(exact, on, mode=None, tuning=None, scene="cornell"):
    e = Engine(device=0, exact=exact)
    builder, positions, (segments, sides), _, _ = SCENES[scene]
    builder(e); e.set_seed(3)
    if mode is not None:
        e.set_bvh_refresh(mode)
    if tuning:
        e.set_tuning(**tuning)
    e.keep_all_planes(True)
    mesh, jt, wt = scenes.skinned_tube(segments, sides, JOINTS, length=LENGTH)
    e.insert_material(TUBE_MAT, Material(base_color=(0.2, 0.7, 0.3, 1.0)))
    e.insert_mesh(TUBE, mesh); e.set_skin(TUBE, jt, wt, JOINTS)
    e._scene, e._ids, e._mesh = scene, [TUBE + i for i in range(len(positions))], mesh
    for inst, p in zip(e._ids, positions):
        e.insert_instance(inst, Instance(TUBE, TUBE_MAT, tube_xform(*p)))
    if on:
        e.set_deformation_motion(True)
    return e


def camera_at(step, size, moving=True, scene="cornell"):
    dx = 0.02 * step if moving else 0.0
    eye, target = SCENES[scene][3], SCENES[scene][4]
    return scenes.camera_for(size, (eye[0] + dx, eye[1] + 0.5 * dx, eye[2]), (target[0] + 0.5 * dx, target[1], target[2]), CameraMode.IMAGE)


def frame_planes(e, cam, out, stream=None):
    s = stream or torch.cuda.current_stream()
    e.render_camera(cam, out.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    planes = {b: e.read_buffer(cam, b) for b in Buffer}
    planes["frame"] = out.cpu().numpy().copy()
    return planes


def assert_planes_equal(pa, pb, what):
    for k in pa:
        assert pa[k].tobytes() == pb[k].tobytes(), f"{what}: {getattr(k, 'name', k)} differs"


def new_out(size):
    return torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda")


def pick_all(e, cam, size):
    w, h = size
    ys, xs = np.mgrid[0:h, 0:w]
    px = torch.from_numpy(np.stack([xs.ravel(), ys.ravel()], 1).astype(np.uint32).view(np.int32).copy()).cuda()
    hits = torch.zeros((w * h * HIT_DTYPE.itemsize,), dtype=torch.uint8, device="cuda")
    e.pick(cam, px.data_ptr(), w * h, hits.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(HIT_DTYPE).reshape(h, w)


def motion_aov(e, cam, size):
    planes = aov_planes(size, kinds=(Aov.MOTION,))
    e.render_aovs(cam, {Aov.MOTION: planes[Aov.MOTION]})
    torch.cuda.synchronize()
    return planes[Aov.MOTION].cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------- 1. off is today
def test_switch_off_changes_nothing():
    size = (64, 48)
    a, b = build(True, False), build(True, False)
    try:
        b.set_deformation_motion(True); b.set_deformation_motion(False)   # touched and put back before the first tick
        desc = scenes.cornell_camera(size, CameraMode.IMAGE)
        cams = [e.create_camera(desc) for e in (a, b)]
        outs = [new_out(size) for _ in range(2)]
        for e in (a, b):
            e.tick()
        for step in range(8):
            for e in (a, b):
                for i, inst in enumerate(IDS):
                    e.set_pose(inst, pose(step, i))
                e.tick()
            assert_planes_equal(frame_planes(a, cams[0], outs[0]), frame_planes(b, cams[1], outs[1]), f"step {step}")
            assert a.skinning_stats() == b.skinning_stats()
            assert a.deformation_stats() == (0, 0) and b.deformation_stats() == (0, 0)
    finally:
        a.close(); b.close()


# ----------------------------------------------------------------------------- 2. on, nothing deforming, is today
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
def test_switch_on_without_a_deformation_changes_nothing(exact):
    size = (64, 48)
    a, b = build(exact, False), build(exact, True)
    try:
        cams = [e.create_camera(camera_at(0, size)) for e in (a, b)]
        outs = [new_out(size) for _ in range(2)]
        for e in (a, b):
            for i, inst in enumerate(IDS):
                e.set_pose(inst, pose(0, i))   # the first pose of an instance has no earlier positions
            e.tick()
        assert b.deformation_stats() == (0, 0)
        assert_planes_equal(frame_planes(a, cams[0], outs[0]), frame_planes(b, cams[1], outs[1]), "the first posed tick")
        for step in range(1, 5):
            for e, cam in zip((a, b), cams):
                e.insert_instance(IDS[1], Instance(TUBE, TUBE_MAT, tube_xform(0.4 + 0.03 * step, 0.0, -0.3)))
                e.update_camera(cam, camera_at(step, size))
                e.tick()
            assert b.deformation_stats()[0] == 0
            assert_planes_equal(frame_planes(a, cams[0], outs[0]), frame_planes(b, cams[1], outs[1]), f"step {step}")
    finally:
        a.close(); b.close()


# ----------------------------------------------------------------------------- 3. the velocity is the stated formula
class Animation:
    """The scene's tubes re-posed every tick, the last one also moved by its transform, under a moving camera; keeps what deform_ref needs.
    track=False keeps nothing and never joins the device (the scheduling test's in-flight variant)."""

    def __init__(self, e, size, moving_camera=True):
        self.e, self.size, self.moving, self.scene, self.ids = e, size, moving_camera, e._scene, e._ids
        self.cam_desc = camera_at(0, size, moving_camera, self.scene)
        self.cam = e.create_camera(self.cam_desc)
        self.base = dict(zip(self.ids, SCENES[self.scene][1]))
        self.xf = {inst: tube_xform(*p) for inst, p in self.base.items()}
        self.prev_xf = dict(self.xf)
        self.posed, self.prev_posed = {}, {}
        self.prev_cam_desc = self.cam_desc
        self.step = 0
        self.out = new_out(size)

    def advance(self, repose=None, stream=None, track=True):
        e, s = self.e, self.step
        repose = self.ids if repose is None else repose
        for i, inst in enumerate(self.ids):
            if inst in repose:
                e.set_pose(inst, pose(s, i))
        mover = self.ids[-1]
        b = self.base[mover]
        x = tube_xform(b[0] + 0.03 * (s + 1), b[1], b[2])
        e.insert_instance(mover, Instance(TUBE, TUBE_MAT, x))
        self.prev_xf[mover] = self.xf[mover]; self.xf[mover] = x
        self.prev_cam_desc = self.cam_desc
        self.cam_desc = camera_at(s + 1, self.size, self.moving, self.scene)
        e.update_camera(self.cam, self.cam_desc)
        if stream is not None:
            e.tick(stream.cuda_stream)
        else:
            e.tick()
        self.step += 1
        if not track:
            return
        torch.cuda.synchronize()
        self.prev_posed = self.posed
        self.posed = {inst: e.read_posed(inst)[:, :9].reshape(-1, 3, 3).copy() for inst in self.ids if self.has_pose(inst)}
        self.reposed = [inst for inst in repose if inst in self.prev_posed]

    def has_pose(self, inst):
        try:
            self.e.read_posed(inst)
            return True
        except Exception:
            return False

    def render(self, stream=None):
        return frame_planes(self.e, self.cam, self.out, stream)

    def expected(self, picks):
        """deform_ref's velocity for every pixel the pick hits: (h, w, 2) float64, the mask of pixels on re-posed tubes, and the
        deformation term alone (what the rigid formula would miss) in pixels."""
        h, w = picks.shape
        want = np.zeros((h, w, 2)); tube = np.zeros((h, w), bool); deformation = np.zeros((h, w))
        hit = picks["hit"] == 1
        u, v = picks["barycentric"][..., 0], picks["barycentric"][..., 1]
        rest = hit.copy()
        for inst in self.ids:
            m = hit & (picks["instance"] == inst)
            rest &= ~m
            if not m.any():
                continue
            tri = picks["triangle"][m]
            if inst in self.posed:
                q = self.posed[inst][tri].astype(np.float64)
                uu, vv = u[m].astype(np.float64)[:, None], v[m].astype(np.float64)[:, None]
                obj = (1.0 - uu - vv) * q[:, 0] + uu * q[:, 1] + vv * q[:, 2]
                point = obj @ self.xf[inst][:, :3].astype(np.float64).T + self.xf[inst][:, 3]
            else:
                point = picks["point"][m].astype(np.float64)
            rigid = deform_ref.rigid_prev_point(self.xf[inst], self.prev_xf[inst], point)
            if inst in self.reposed:
                prev = deform_ref.deformed_prev_point(self.prev_posed[inst][tri], u[m], v[m], self.prev_xf[inst])
                tube[m] = True
                deformation[m] = np.linalg.norm(deform_ref.screen(self.prev_cam_desc, rigid) - deform_ref.screen(self.prev_cam_desc, prev), axis=-1)
            else:
                prev = rigid
            want[m] = deform_ref.velocity(self.cam_desc, self.prev_cam_desc, point, prev)
        point = picks["point"][rest].astype(np.float64)   # the box: static, unskinned
        want[rest] = deform_ref.velocity(self.cam_desc, self.prev_cam_desc, point, point)
        return want, tube, deformation, hit


def check_velocity(anim, planes, exact, what, min_median=3.0):
    e, size = anim.e, anim.size
    h, w = size[1], size[0]
    picks = pick_all(e, anim.cam, size)
    want, tube, deformation, hit = anim.expected(picks)
    vel = planes[Buffer.VELOCITY_MAP].reshape(h, w, 4)[..., :2]
    motion = motion_aov(e, anim.cam, size)
    assert tube.sum() > 500, f"{what}: only {int(tube.sum())} pixels on re-posed tubes"
    median = float(np.median(deformation[tube]))
    print(f"{what}: {int(tube.sum())} tube pixels, median expected deformation velocity {median:.2f} px")
    if min_median:
        assert median >= min_median, f"{what}: the median expected deformation velocity on tube pixels is {median:.2f} px: the signal is too small"
    err = np.abs(vel.astype(np.float64) - want).max(axis=-1)
    err_aov = np.abs(motion.astype(np.float64) - want).max(axis=-1)
    bad, bad_aov = err > TOLERANCE, err_aov > TOLERANCE
    print(f"{what}: worst error on tube pixels {err[tube].max():.3e} px (plane), {err_aov[tube].max():.3e} px (AOV); elsewhere {err[hit & ~tube].max(initial=0.0):.3e}")
    if exact:
        assert np.array_equal(bits(motion[hit]), bits(vel[hit])), f"{what}: ST_AOV_MOTION differs from the velocity plane"
        assert not bad[tube].any() and not bad_aov[tube].any(), f"{what}: {int(bad[tube].sum())} tube pixels off by more than {TOLERANCE} px (worst {err[tube].max():.4f})"
        assert not bad[hit & ~tube].any(), f"{what}: {int(bad[hit & ~tube].sum())} pixels off the re-posed tubes differ from the rigid formula"
    else:
        allowed = (1.0 - AGREE) * tube.sum()
        assert bad[tube].sum() <= allowed and bad_aov[tube].sum() <= allowed, f"{what}: {int(bad[tube].sum())} / {int(bad_aov[tube].sum())} of {int(tube.sum())} tube pixels off by more than {TOLERANCE} px"
        assert bad[hit & ~tube].sum() <= (1.0 - AGREE) * (hit & ~tube).sum()


@pytest.mark.parametrize("scene,exact", [("cornell", True), ("cornell", False), ("dungeon", True), ("dungeon", False), ("lds", True), ("lds", False)])
def test_velocity_is_the_stated_formula(scene, exact):
    """"lds": the tube alone, a scene that lives in LDS — the LDS_SCENE instantiations of k_prim_visibility and k_aov take the term."""
    e = build(exact, True, scene=scene)
    try:
        anim = Animation(e, SIZE)
        anim.advance(); anim.render()           # the first pose: no earlier positions
        assert e.deformation_stats()[0] == 0
        n_tubes, tris = len(e._ids), len(e._mesh.positions)
        for step in range(6):
            anim.advance()
            n, nbytes = e.deformation_stats()
            assert n == n_tubes and nbytes == n_tubes * tris * 96, (n, nbytes)
            check_velocity(anim, anim.render(), exact, f"{scene} tick {step}")
    finally:
        e.close()


def test_switch_turned_on_late_starts_with_the_next_reskin():
    """The tick after the switch is turned on only records the poses it skins (the header says so): that frame is the switch-off frame."""
    e, off = build(True, False), build(True, False)
    try:
        anim, ref = Animation(e, SIZE), Animation(off, SIZE)
        for _ in range(2):
            for a in (anim, ref):
                a.advance(); a.render()
        e.set_deformation_motion(True)
        assert_planes_equal(anim.render(), ref.render(), "a frame between the call and the tick")   # (takes effect at the next st_tick)
        for a in (anim, ref):
            a.advance()
        assert e.deformation_stats() == (0, 0)
        assert_planes_equal(anim.render(), ref.render(), "the first tick with the switch on")
        anim.advance()
        assert e.deformation_stats()[0] == 2
        check_velocity(anim, anim.render(), True, "the second tick with the switch on")
        e.set_deformation_motion(False)
        planes = anim.render()                     # still the tick's state: the term stays until the next st_tick
        check_velocity(anim, planes, True, "switched off, before the tick")
        anim.advance()
        assert e.deformation_stats() == (0, 0)
    finally:
        e.close(); off.close()


# ----------------------------------------------------------------------------- 4. reprojection follows the surface
def vertex_adjacency(mesh):
    """adj[a, b]: triangles a and b of the mesh are the same or share a vertex (positions compared after rounding to 1e-5)."""
    pos = np.round(np.asarray(mesh.positions, np.float64).reshape(-1, 3), 5)
    _, vid = np.unique(pos, axis=0, return_inverse=True)
    vid = vid.reshape(-1, 3)
    inc = np.zeros((len(vid), vid.max() + 1), np.int32)
    for c in range(3):
        inc[np.arange(len(vid)), vid[:, c]] = 1
    return (inc @ inc.T) > 0


def identity_aovs(e, cam, size):
    planes = aov_planes(size, kinds=(Aov.INSTANCE, Aov.TRIANGLE))
    e.render_aovs(cam, {k: planes[k] for k in (Aov.INSTANCE, Aov.TRIANGLE)})
    torch.cuda.synchronize()
    return planes[Aov.INSTANCE].cpu().numpy(), planes[Aov.TRIANGLE].cpu().numpy()


def reprojection_share(scene, on, ticks=7):
    e = build(False, on, scene=scene)
    try:
        w, h = SIZE
        anim = Animation(e, SIZE, moving_camera=False)
        adj = vertex_adjacency(e._mesh)
        prev, good, valid, tube_px = None, 0, 0, 0
        for step in range(ticks):
            anim.advance()
            planes = anim.render()
            inst, tri = identity_aovs(e, anim.cam, SIZE)
            if prev is not None and step >= 2:
                rp = planes[Buffer.REPROJECTION_MAP].reshape(h, w, 4)
                tube = np.isin(inst, e._ids)
                ok = tube & (rp[..., 2] > 0)
                px = np.clip(np.floor(rp[..., 0] + 0.5).astype(np.int64), 0, w - 1)[ok]
                py = np.clip(np.floor(rp[..., 1] + 0.5).astype(np.int64), 0, h - 1)[ok]
                p_inst, p_tri = prev[0][py, px], prev[1][py, px]
                same = p_inst == inst[ok]
                same[same] &= adj[tri[ok][same], np.minimum(p_tri[same], len(adj) - 1)]
                good += int(same.sum()); valid += int(ok.sum()); tube_px += int(tube.sum())
            prev = (inst, tri)
        return {"share": good / max(valid, 1), "valid": valid, "tube_pixels": tube_px}
    finally:
        e.close()


@pytest.mark.parametrize("scene", ["cornell", "dungeon"])
def test_reprojection_follows_the_surface(scene):
    """Of the tube pixels whose reprojection-map entry is valid, the share whose rounded previous position shows the same instance and the
    same triangle or one sharing a vertex with it in the previous frame's ST_AOV_INSTANCE / ST_AOV_TRIANGLE: higher with the switch on.
    Measured on one MI355X (fast build, 256x192, five compared ticks): see profiles/deform_motion.json "reprojection"."""
    on, off = reprojection_share(scene, True), reprojection_share(scene, False)
    print(f"{scene}: share on {on['share']:.4f} ({on['valid']} valid of {on['tube_pixels']}), off {off['share']:.4f} ({off['valid']} valid of {off['tube_pixels']})")
    path = os.path.join(ROOT, "profiles", "deform_motion.json")
    try:
        rec = json.load(open(path))
    except (OSError, ValueError):
        rec = {}
    rec.setdefault("reprojection", {})[scene] = {"size": list(SIZE), "on": on, "off": off}
    try:
        json.dump(rec, open(path, "w"), indent=1)
    except OSError:
        pass   # a read-only checkout still runs the assertion
    assert on["valid"] > 0 and off["tube_pixels"] > 0
    assert on["share"] > off["share"], f"{scene}: {on['share']:.4f} of the valid tube pixels land on their surface with the switch on, {off['share']:.4f} with it off"


# ----------------------------------------------------------------------------- 5. store growth and lifecycle
def test_store_growth_and_lifecycle():
    e, off = build(True, True), build(True, False)
    try:
        anim, ref = Animation(e, SIZE), Animation(off, SIZE)
        both = (anim, ref)
        tris = len(e._mesh.positions)

        def step(what, repose=None, check=True):
            for a in both:
                a.advance(repose=repose)
            pa, pb = anim.render(), ref.render()
            if check:
                check_velocity(anim, pa, True, what)
            return pa, pb

        step("first pose", check=False)
        for k in range(2):
            step(f"before growth {k}")
        # more posed instances than the posed store's headroom holds: the store is reallocated and every pose, current and previous, skinned again
        for a in both:
            for k in range(8):
                a.e.insert_instance(TUBE + 100 + k, Instance(TUBE, TUBE_MAT, tube_xform(-0.8 + 0.2 * k, 0.0, -0.8)))
                a.e.set_pose(TUBE + 100 + k, pose(k, 0))
        before = e.skinning_stats()[1]
        step("growth tick")
        assert e.skinning_stats()[1] - before == (10 + 2) * tris, "the store must have grown: ten poses and two previous regions skinned again"
        step("growth tick + 1")
        assert e.deformation_stats() == (2, 2 * tris * 96)

        def rigid_on(pa, pb, insts, what):
            picks = pick_all(e, anim.cam, SIZE)
            m = (picks["hit"] == 1) & np.isin(picks["instance"], insts)
            assert m.sum() > 200
            for k in pa:
                if k == "frame" or pa[k].size != SIZE[0] * SIZE[1] * 4:
                    continue
                va, vb = pa[k].reshape(SIZE[1], SIZE[0], 4), pb[k].reshape(SIZE[1], SIZE[0], 4)
                if k in (Buffer.VELOCITY_MAP, Buffer.REPROJECTION_MAP):
                    assert np.array_equal(bits(va[m]), bits(vb[m])), f"{what}: {k.name} differs from the switch-off frame on the instance"

        # (a) back to the bind pose: the pose and its previous positions go; that frame shows the rigid formula on the instance
        for a in both:
            a.e.set_pose(IDS[0], None)
        pa, pb = step("set_pose(None)", repose=[IDS[1]], check=False)
        assert e.deformation_stats()[0] == 1
        rigid_on(pa, pb, [IDS[0]], "after set_pose(None)")
        assert not np.array_equal(pa[Buffer.VELOCITY_MAP], pb[Buffer.VELOCITY_MAP]), "the tube that still deforms must differ from the switch-off frame"
        step("first pose again", check=False); step("the term returns after set_pose(None)")
        assert e.deformation_stats()[0] == 2
        # (b) an instance remove + insert drops that instance's pose only
        for a in both:
            a.e.remove_instance(IDS[0]); a.e.insert_instance(IDS[0], Instance(TUBE, TUBE_MAT, tube_xform(*POSITIONS[0])))
        pa, pb = step("remove + insert", check=False)
        assert e.deformation_stats()[0] == 1, "the re-inserted instance's first pose has no earlier positions; the other tube keeps its own"
        rigid_on(pa, pb, [IDS[0]], "after an instance remove + insert")
        step("the term returns after remove + insert")
        assert e.deformation_stats()[0] == 2
        # (c) a mesh re-insert drops the skin and every pose of it
        mesh, jt, wt = scenes.skinned_tube(24, 12, JOINTS, length=LENGTH)
        for a in both:
            a.e.insert_mesh(TUBE, mesh); a.e.set_skin(TUBE, jt, wt, JOINTS)
        pa, pb = step("mesh re-insert", check=False)
        assert e.deformation_stats()[0] == 0, "the first pose after a re-inserted mesh has no earlier positions"
        rigid_on(pa, pb, IDS, "after the mesh re-insert")   # (velocity and reprojection: the other planes carry the two engines' different histories)
        step("the term returns after the mesh re-insert")
        assert e.deformation_stats()[0] == 2
    finally:
        e.close(); off.close()


# ----------------------------------------------------------------------------- 6. scheduling
def velocity_planes(exact=False, mode=None, tuning=None, tick_stream=False, frames=1, ticks=4):
    e = build(exact, True, mode, tuning)
    try:
        anim = Animation(e, (128, 96))
        side = torch.cuda.Stream() if tick_stream else None
        got = []
        for step in range(ticks):
            anim.advance(stream=side)
            for _ in range(frames):
                planes = anim.render()
            got.append(planes[Buffer.VELOCITY_MAP].copy())
        assert e.deformation_stats()[0] == 2
        return got
    finally:
        e.close()


def test_scheduling_variants_give_the_same_velocity_plane():
    plain = velocity_planes()
    assert any(np.any(p != 0) for p in plain[1:])
    variants = {"REBUILD": dict(mode=REBUILD), "REFIT_DEVICE": dict(mode=REFIT_DEVICE), "AUTO": dict(mode=AUTO), "overlap off": dict(tuning=dict(overlap=0)),
                "tick on another stream": dict(tick_stream=True), "two frames per tick": dict(frames=2)}
    for name, kw in variants.items():
        got = velocity_planes(**kw)
        for step, (g, p) in enumerate(zip(got, plain)):
            assert g.tobytes() == p.tobytes(), f"{name}: the velocity plane of tick {step} differs from the plain run"


def final_planes(in_flight, ticks=10, size=(1920, 1080)):
    """`ticks` re-posed ticks with a frame each. in_flight: nothing joins the device in between — each set_pose + tick is enqueued on a side
    stream while the frame before it still runs on the render stream, so only the engine's own events order the skin launch behind the
    frames that read the regions it overwrites. Large frames, so that the host really is ahead."""
    e = build(False, True)
    try:
        anim = Animation(e, size)
        side, main = torch.cuda.Stream(), torch.cuda.current_stream()
        for step in range(ticks):
            anim.advance(stream=side if in_flight else None, track=False)
            if not in_flight:
                torch.cuda.synchronize()
            e.render_camera(anim.cam, anim.out.data_ptr(), main.cuda_stream)
            if not in_flight:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        planes = {b: e.read_buffer(anim.cam, b) for b in Buffer}
        planes["frame"] = anim.out.cpu().numpy().copy()
        return planes
    finally:
        e.close()


def test_frames_in_flight_are_ordered_by_the_engine_alone():
    assert_planes_equal(final_planes(True), final_planes(False), "ticks enqueued while frames are in flight")


def test_two_tiles_equal_the_single_engine():
    """Two st_dist_init_local ranks with the switch on. An Image frame's denoiser and resampling taps cross tile borders, so a composed
    Image frame gathered from apron-less tiles is not the single engine's at any commit; what deformation motion writes is per pixel. Each
    rank's velocity plane inside its own tile is the single engine's bit for bit, which is what is asserted, tick by tick, with the gather running."""
    size, world, ticks = (128, 96), 2, 4
    stream = torch.cuda.current_stream().cuda_stream

    def animate(e, cam, s):
        for i, inst in enumerate(IDS):
            e.set_pose(inst, pose(s, i))
        e.update_camera(cam, camera_at(s + 1, size))
        e.tick(stream)

    one = build(True, True)
    ranks = []
    try:
        cam = one.create_camera(camera_at(0, size))
        single = new_out(size)
        for r in range(world):
            e = build(True, True)
            c = e.create_camera(camera_at(0, size))
            e.dist_init_local(r, world, 7500 + world)
            owned, window = e.dist_set_partition(c, apron=0)
            ranks.append((e, c, torch.zeros_like(single), owned))
        full = torch.zeros_like(single)
        for s in range(ticks):
            animate(one, cam, s); one.render_camera(cam, single.data_ptr(), stream)
            for r in range(world - 1, -1, -1):   # in-process transport: rank 0 last
                e, c, out, _ = ranks[r]
                animate(e, c, s)
                e.render_camera(c, out.data_ptr(), stream)
                e.dist_gather(c, out.data_ptr(), full.data_ptr() if r == 0 else 0, stream)
            ranks[0][0].dist_wait(ranks[0][1], host=True)
            torch.cuda.synchronize()
            want = one.read_buffer(cam, Buffer.VELOCITY_MAP).reshape(size[1], size[0], 4)
            assert one.deformation_stats()[0] == (2 if s else 0)
            for e, c, _, (x0, y0, x1, y1) in ranks:
                got = e.read_buffer(c, Buffer.VELOCITY_MAP).reshape(size[1], size[0], 4)
                assert np.array_equal(bits(got[y0:y1, x0:x1]), bits(want[y0:y1, x0:x1])), f"tick {s}: a tile's velocity plane differs from the single engine's"
                assert e.deformation_stats()[0] == (2 if s else 0)
        assert np.any(want != 0)
    finally:
        for e, *_ in ranks:
            e.dist_shutdown(); e.close()
        one.close()
