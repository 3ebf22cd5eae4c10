"""Per-pixel AOVs on the GPU (include/strolle_hip.h "per-pixel AOVs"; k_aov.hip).

The exact build's AOVs are checked against what the frame itself stored (the G-buffer's depth, the velocity plane) and against
st_camera_pick of every pixel; the fast build against the exact build; every camera mode, a window, tiles of one frame, a second stream
and a subset of planes against the full single-engine AOVs."""

import numpy as np
import pytest
import torch

from strolle_amd import Aov, Buffer, CameraMode, Engine, Instance, Material, Mesh, aov_planes, scenes
from strolle_amd.api import HIT_DTYPE

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-3, 1e-5          # the fast build's tolerance gate (tests/test_gpu_fast_tolerance.py)
VELOCITY_ATOL_PX = 1e-3          # ... and its velocity gate in pixels (tests/test_gpu_fast_steady_state.py)
AGREE = 0.999                    # ties at shared edges (tests/test_gpu_ray_query.py)
FLT_MAX = np.float32(3.4028235e38)
SENTINEL = 12345                 # a value every plane type holds and no AOV of these scenes takes
ALL = tuple(Aov)

MESH, MATERIAL, MOVER = 7000, 7001, 7002


def _torus_xform(p, scale):
    return np.array([[scale, 0, 0, p[0]], [0, 0, -scale, p[1]], [0, scale, 0, p[2]]], np.float32)


# a torus of our own that moves every frame (instance motion in the velocity plane), and a camera that moves too
MOVING = {
    "cornell": (scenes.build_cornell, scenes.cornell_camera, (0.0, 1.0, 3.2), (0.0, 1.0, 0.0), (0.25, 0.8, 0.2), 0.25),
    "dungeon": (scenes.build_dungeon, scenes.dungeon_camera, (-5.75, 0.5, -16.8), (-5.75, 0.5, -17.0), (-5.75, 0.5, -17.8), 0.6),
}


def _add_mover(e, pos, scale):
    p, n, uv = scenes.bevy_torus()
    e.insert_mesh(MESH, Mesh(p, n, uv))
    e.insert_material(MATERIAL, Material(base_color=(0.8, 0.3, 0.2, 1.0)))
    e.insert_instance(MOVER, Instance(MESH, MATERIAL, _torus_xform(pos, scale)))


def _moving_frames(e, name, size, frames, mode=CameraMode.IMAGE, render=True):
    """A camera and `frames` ticks, each after a move of the torus and of the camera (and a render of it unless render=False)."""
    _, _, eye, target, pos, scale = MOVING[name]
    cam = e.create_camera(scenes.camera_for(size, eye, target, mode))
    pos = list(pos); eye = list(eye)
    out = torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda") if render else None
    for f in range(frames):
        pos[0] += 0.04; eye[0] += 0.02; eye[1] += 0.01
        e.insert_instance(MOVER, Instance(MESH, MATERIAL, _torus_xform(pos, scale)))
        e.update_camera(cam, scenes.camera_for(size, tuple(eye), (target[0] + 0.02 * (f + 1), target[1], target[2]), mode))
        e.tick()
        if render:
            e.render_camera(cam, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return cam


def run_aovs(e, cam, size, kinds=ALL, stream=None, planes=None):
    planes = planes if planes is not None else aov_planes(size, fill=SENTINEL)
    e.render_aovs(cam, {k: planes[k] for k in kinds}, stream=stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in planes.items()}


def pick_all(e, cam, size):
    w, h = size
    ys, xs = np.mgrid[0:h, 0:w]
    px = torch.from_numpy(np.stack([xs.ravel(), ys.ravel()], 1).astype(np.uint32).view(np.int32).copy()).cuda()
    hits = torch.zeros((w * h * HIT_DTYPE.itemsize,), dtype=torch.uint8, device="cuda")
    e.pick(cam, px.data_ptr(), w * h, hits.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(HIT_DTYPE).reshape(h, w)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_planes_equal(got, want, what, kinds=ALL):
    for k in kinds:
        g, x = got[k], want[k]
        same = g.view(np.uint8).tobytes() == x.view(np.uint8).tobytes()
        assert same, f"{what}: {k.name} differs"


def assert_sky_is_clean(a):
    sky = a[Aov.DEPTH] == FLT_MAX
    assert (~sky).mean() > 0.05, "the camera must see the scene"
    assert not a[Aov.NORMAL][sky].any() and not a[Aov.ALBEDO][sky].any() and not a[Aov.MOTION][sky].any()
    assert not a[Aov.INSTANCE][sky].any() and np.all(a[Aov.TRIANGLE][sky] == 0xFFFFFFFF)
    assert np.all(a[Aov.NORMAL][~sky][:, 3] == 0)


# ----------------------------------------------------------------------------- 1. the exact build against the frame's own planes and picks
@pytest.mark.parametrize("size", [(160, 96), (1920, 1080)], ids=["small", "1080p"])
@pytest.mark.parametrize("name", list(MOVING))
def test_exact_build_equals_the_frame_on_screen(name, size):
    w, h = size
    e = Engine(device=0, exact=True)
    try:
        MOVING[name][0](e)
        _add_mover(e, MOVING[name][4], MOVING[name][5])
        e.keep_all_planes(True)
        frames = 3
        cam = _moving_frames(e, name, size, frames)
        a = run_aovs(e, cam, size)
        assert_sky_is_clean(a)
        alt = frames % 2 == 1    # the camera's frame number is the tick's, and the engine's first frame is 1 (lib.rs:152): odd frames write the _B half
        d0 = e.read_buffer(cam, Buffer.PRIM_GBUFFER_D0_B if alt else Buffer.PRIM_GBUFFER_D0_A).reshape(h, w, 4)
        d1 = e.read_buffer(cam, Buffer.PRIM_GBUFFER_D1_B if alt else Buffer.PRIM_GBUFFER_D1_A).reshape(h, w, 4)
        vel = e.read_buffer(cam, Buffer.VELOCITY_MAP, strict=True).reshape(h, w, 4)
        hit = np.any(d0 != 0, axis=2)
        depth = a[Aov.DEPTH]
        assert np.array_equal(bits(depth[hit]), bits(d0[..., 0][hit])), f"depth differs on {int((bits(depth[hit]) != bits(d0[..., 0][hit])).sum())} pixels"
        assert np.array_equal(depth == FLT_MAX, ~hit)
        assert np.array_equal(bits(a[Aov.MOTION]), bits(vel[..., :2])), "motion differs from VELOCITY_MAP.xy"
        assert (a[Aov.INSTANCE] == MOVER).sum() > 50 and np.any(a[Aov.MOTION][a[Aov.INSTANCE] == MOVER] != 0)
        picks = pick_all(e, cam, size)
        assert np.array_equal(picks["hit"] == 1, hit)
        assert np.array_equal(bits(a[Aov.NORMAL][..., :3]), bits(picks["normal"]))
        assert np.array_equal(a[Aov.INSTANCE], picks["instance"])
        assert np.array_equal(a[Aov.TRIANGLE][hit], picks["triangle"][hit])
        # albedo: within one step of the G-buffer's gamma code (8 bits RGB, 6 bits alpha: st_math.h gbuffer_pack_base_color)
        code = d1[..., 3].view(np.uint32)[hit]
        want = np.stack([(code >> s) & 0xFF for s in (0, 8, 16, 24)], 1).astype(np.int64)
        g = np.clip(a[Aov.ALBEDO][hit].astype(np.float64), 0, None) ** (1 / 2.2)
        got = np.floor(np.clip(g, 0, 1) * np.array([255, 255, 255, 63])).astype(np.int64)
        assert np.abs(got - want).max() <= 1, f"albedo: gamma codes differ by {np.abs(got - want).max()}"
    finally:
        e.close()


# ----------------------------------------------------------------------------- 2. the fast build (device-built tree) against the exact build
SPAWN = 90001


@pytest.mark.parametrize("subdivide", [0, 2], ids=["dungeon", "dungeon208k"])
def test_fast_build_agrees_with_the_exact_build(subdivide):
    size = (1920, 1080)
    engines = [Engine(device=0, exact=True), Engine(device=0, exact=False)]
    try:
        cams = []
        for e in engines:
            scenes.build_dungeon(e, subdivide=subdivide)
            e.insert_material(SPAWN, Material(base_color=(0.8, 0.2, 0.2, 1.0)))
            cams.append(e.create_camera(scenes.dungeon_camera(size)))
            e.tick()
        builds0 = engines[1].device_builds()
        pos = [-5.75, 0.5, -17.8]
        for step in range(16):       # a spawn and 15 moves
            for e, cam in zip(engines, cams):
                e.insert_instance(SPAWN, Instance(5000, SPAWN, _torus_xform(pos, 0.6)))
                e.update_camera(cam, scenes.camera_for(size, (-5.75 + 0.01 * step, 0.5, -16.8), (-5.75, 0.5, -17.0)))
                e.tick()
            pos[0] += 0.05; pos[2] -= 0.02
        assert engines[1].device_builds() > builds0, "the spawn must be answered by a device LBVH build"
        mid = [run_aovs(e, cam, size) for e, cam in zip(engines, cams)]
        for e in engines:
            e.remove_instance(SPAWN)
            e.tick()
        end = [run_aovs(e, cam, size) for e, cam in zip(engines, cams)]
        assert (mid[0][Aov.INSTANCE] == SPAWN).sum() > 1000 and not (end[1][Aov.INSTANCE] == SPAWN).any()
        for what, (x, f) in (("after 15 moves", mid), ("after the despawn", end)):
            assert_sky_is_clean(f)
            ids = (f[Aov.INSTANCE] == x[Aov.INSTANCE]) & (f[Aov.TRIANGLE] == x[Aov.TRIANGLE])
            assert ids.mean() >= AGREE, f"{what}: ids agree on {ids.mean():.5f}"
            hit = ids & (x[Aov.DEPTH] < FLT_MAX)
            dx, df = x[Aov.DEPTH], f[Aov.DEPTH]
            close_d = np.where(x[Aov.DEPTH] < FLT_MAX, np.abs(df - dx) <= ATOL + RTOL * np.abs(dx), df == dx)
            assert close_d.mean() >= AGREE, f"{what}: depth agrees on {close_d.mean():.5f}"
            for k, atol in ((Aov.NORMAL, ATOL), (Aov.ALBEDO, ATOL), (Aov.MOTION, VELOCITY_ATOL_PX)):
                g, w = f[k][hit], x[k][hit]
                close = np.all(np.abs(g - w) <= atol + RTOL * np.abs(w), axis=1)
                assert close.mean() >= AGREE, f"{what}: {k.name} within the gate on {close.mean():.5f}"
    finally:
        for e in engines:
            e.close()


# ----------------------------------------------------------------------------- 3. every camera mode
def test_reference_and_heatmap_cameras_equal_an_image_camera():
    size = (320, 180)
    e = Engine(device=0)
    try:
        scenes.build_dungeon(e)
        cams = {m: e.create_camera(scenes.dungeon_camera(size, m)) for m in (CameraMode.IMAGE, CameraMode.REFERENCE, CameraMode.BVH_HEATMAP)}
        e.tick()
        out = torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda")
        for cam in cams.values():
            e.render_camera(cam, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        got = {m: run_aovs(e, cam, size) for m, cam in cams.items()}
        assert_sky_is_clean(got[CameraMode.IMAGE])
        for m in (CameraMode.REFERENCE, CameraMode.BVH_HEATMAP):
            assert_planes_equal(got[m], got[CameraMode.IMAGE], m.name)
    finally:
        e.close()


# ----------------------------------------------------------------------------- 4. windows and tiles
def test_window_leaves_the_rest_of_every_plane_untouched():
    size = (256, 144)
    e = Engine(device=0)
    try:
        scenes.build_dungeon(e)
        full_cam = e.create_camera(scenes.dungeon_camera(size))
        win_cam = e.create_camera(scenes.dungeon_camera(size))
        x0, y0, x1, y1 = 32, 21, 208, 117    # rows off the 8-pixel tile boundaries: the launch covers whole tiles, the window masks the rest
        e.set_camera_window(win_cam, x0, y0, x1, y1)
        e.tick()
        full, win = run_aovs(e, full_cam, size), run_aovs(e, win_cam, size)
        inside = np.zeros((size[1], size[0]), bool); inside[y0:y1, x0:x1] = True
        for k in ALL:
            assert np.array_equal(win[k][inside], full[k][inside]), k.name
            assert np.all(win[k][~inside] == SENTINEL), k.name
    finally:
        e.close()


@pytest.mark.parametrize("world", [2, 4])
def test_tiles_of_one_frame_assemble_into_the_single_engine_aovs(world):
    size = (272, 200)
    build, camera = scenes.build_dungeon, scenes.dungeon_camera
    single = Engine(device=0, exact=True)
    ranks = []
    try:
        build(single)
        cam = single.create_camera(camera(size))
        single.tick()
        want = run_aovs(single, cam, size)
        assembled = aov_planes(size, fill=SENTINEL)
        for r in range(world):
            e = Engine(device=0, exact=True)
            ranks.append(e)
            build(e)
            c = e.create_camera(camera(size))
            e.dist_init_local(r, world, 7100 + world)
            owned, window = e.dist_set_partition(c, apron=0)
            assert owned == window
            e.tick()
            mine = run_aovs(e, c, size)
            ox0, oy0, ox1, oy1 = owned
            outside = np.ones((size[1], size[0]), bool); outside[oy0:oy1, ox0:ox1] = False
            for k in ALL:
                assert np.all(mine[k][outside] == SENTINEL), f"rank {r}: {k.name} written outside its tile"
            run_aovs(e, c, size, planes=assembled)   # every rank writes its own tile of one set of planes
        got = {k: v.cpu().numpy() for k, v in assembled.items()}
        assert_planes_equal(got, want, f"{world} tiles vs one engine")
    finally:
        for e in ranks:
            e.close()
        single.close()


# ----------------------------------------------------------------------------- 5. ordering behind the tick's uploads
def test_aovs_on_another_stream_see_the_tick_before_them():
    size = (128, 96)

    def run(sync):
        e = Engine(device=0)
        scenes.build_dungeon(e)
        cam = e.create_camera(scenes.dungeon_camera(size))
        e.insert_material(SPAWN, Material(base_color=(0.8, 0.2, 0.2, 1.0)))
        e.tick()
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        planes = [aov_planes(size, (Aov.DEPTH, Aov.INSTANCE), fill=SENTINEL) for _ in range(10)]
        torch.cuda.synchronize()
        pos = [-5.75, 0.5, -17.8]
        for it in range(10):
            e.insert_instance(SPAWN, Instance(5000, SPAWN, _torus_xform(pos, 0.6)))
            pos[0] += 0.1
            e.tick(a.cuda_stream)
            if sync: torch.cuda.synchronize()
            e.render_aovs(cam, planes[it], stream=b)
            if sync: torch.cuda.synchronize()
        torch.cuda.synchronize()
        res = [{k: v.cpu().numpy() for k, v in p.items()} for p in planes]
        e.close()
        return res

    free, ordered = run(False), run(True)
    for it in range(10):
        assert (ordered[it][Aov.INSTANCE] == SPAWN).sum() > 100
        assert_planes_equal(free[it], ordered[it], f"iteration {it}: the AOVs on stream B saw another scene than the tick before them",
                            (Aov.DEPTH, Aov.INSTANCE))
    assert not np.array_equal(ordered[0][Aov.INSTANCE], ordered[-1][Aov.INSTANCE])


# ----------------------------------------------------------------------------- 6. a subset of the planes
def test_only_requested_planes_are_written():
    size = (200, 120)
    e = Engine(device=0)
    try:
        scenes.build_cornell(e)
        _add_mover(e, MOVING["cornell"][4], MOVING["cornell"][5])
        cam = _moving_frames(e, "cornell", size, 2)
        full = run_aovs(e, cam, size)
        assert_sky_is_clean(full)
        for subset in ((Aov.DEPTH, Aov.MOTION), (Aov.ALBEDO,), (Aov.INSTANCE, Aov.TRIANGLE), (Aov.NORMAL, Aov.TRIANGLE)):
            got = run_aovs(e, cam, size, kinds=subset)
            assert_planes_equal(got, full, f"subset {[k.name for k in subset]}", subset)
            for k in set(ALL) - set(subset):
                assert np.all(got[k] == SENTINEL), f"{k.name} was written though not requested ({[s.name for s in subset]})"
    finally:
        e.close()
