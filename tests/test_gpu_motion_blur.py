"""GPU tests of motion blur (include/strolle_hip.h "motion blur"; k_motion_blur.hip, st_motion_blur.cpp): st_motion_blur_process on
synthetic inputs against the numpy restatement (motion_blur_ref.py) bit for bit in both builds; properties that do not rest on the
restatement; whole frames with the blur on against the restatement fed the same frame rendered with the blur off and the velocity and
G-buffer planes read back; off is off; nothing else changes; pipelining across frames; lifecycle. Every test builds its own engines and
uses entry points the parent commit does not have.

Sizes: the tile is 32 x 32, the workgroup 32 x 8 and the radius at most 32, so 72 x 52 (neither a tile nor a workgroup multiple, 3 x 2
tiles), 64 x 64, 33 x 9 (a second tile one pixel wide) and 5 x 5 (one partial tile, where every tap clamps)."""
import numpy as np
import pytest
import torch

import bloom_ref
import display_ref
import motion_blur_ref as R
import output_chain as C
import post_ref
import test_gpu_deform_motion as deform
from output_chain import Out, _all_planes, _bits, _check, _engine, _image
from parity import assert_bits_equal
from strolle_amd import (Buffer, CameraMode, Engine, Instance, OutputFormat, PassBit, ResampleFilter, Tonemap, bloom_desc, display_desc,
                         motion_blur_desc, post_desc, scenes)

pytestmark = pytest.mark.gpu
SIZE = (72, 52)
SIZES = [(72, 52), (64, 64), (33, 9), (5, 5)]
F = np.float32


def _ref(key, make):
    return C._ref(__name__, key, make)


def _velocity(kind, w, h, seed=5):
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros((h, w, 2), np.float32)
    if kind == "uniform":
        return np.broadcast_to(np.array([37.0, -12.5], np.float32), (h, w, 2)).copy()
    by, bx = (h + 7) // 8, (w + 7) // 8   # random per 8 x 8 block: magnitudes 0 .. 200 px, a third of the blocks at rest
    mag = rng.random((by, bx)) * 200.0 * (rng.random((by, bx)) > 0.33)
    ang = rng.random((by, bx)) * 2 * np.pi
    v = np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1).astype(np.float32)
    v = np.repeat(np.repeat(v, 8, 0), 8, 1)[:h, :w].copy()
    if kind == "nan":
        n = max(2, w * h // 40)
        v[rng.integers(0, h, n), rng.integers(0, w, n), rng.integers(0, 2, n)] = np.nan
    return v


def _depth(w, h, seed=6):
    """two layers in 8 x 8 blocks, plus FLT_MAX (sky) in places"""
    rng = np.random.default_rng(seed)
    by, bx = (h + 7) // 8, (w + 7) // 8
    z = np.where(rng.random((by, bx)) < 0.5, 2.0, 9.0).astype(np.float32)
    z[rng.random((by, bx)) < 0.2] = R.FLT_MAX
    z = np.repeat(np.repeat(z, 8, 0), 8, 1)[:h, :w].copy()
    return np.where(z == R.FLT_MAX, z, z * (1.0 + 0.01 * rng.random((h, w)))).astype(np.float32)


def _process(e, d, color, vel, depth, fmt=0, display=None, stream=None):
    h, w = color.shape[:2]
    tc, tv, tz = torch.from_numpy(color).cuda(), torch.from_numpy(vel).cuda(), torch.from_numpy(depth).cuda()
    out = Out(fmt, (w, h), fill=0x5a)
    e.motion_blur_process(d, tc.data_ptr(), tv.data_ptr(), tz.data_ptr(), w, h, out.ptr(), fmt, display=display,
                          stream=stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.get()


def _restate(d, color, vel, depth, display=None, scale=None):
    c = R.motion_blur(color, vel, depth, d.shutter, d.samples, d.max_radius, d.depth_softness, d.flags)
    if display is None:
        return c
    return display_ref.transform(c[..., :3], int(display), scale)


# ---------------------------------------------------------------- 1. bit for bit against the restatement
DESCS = [dict(samples=2, jitter=False, max_radius=4.0, shutter=1.0), dict(samples=8, jitter=True, max_radius=0.0, shutter=0.5),
         dict(samples=32, jitter=True, max_radius=32.0, shutter=0.5, depth_softness=0.3), dict(samples=8, jitter=False, max_radius=4.0, shutter=0.25)]


@pytest.mark.parametrize("exact", [True, False])
def test_process_matches_the_restatement_on_synthetic_inputs(exact):
    e = Engine(device=0, exact=exact)
    moved = False
    with np.errstate(all="ignore"):
        for (w, h) in SIZES:
            img, z = _image(w, h), _depth(w, h)
            for kind in ("zero", "uniform", "blocks", "nan"):
                v = _velocity(kind, w, h)
                for i, kw in enumerate(DESCS):
                    d = motion_blur_desc(**kw)
                    want = _ref((w, h, kind, i), lambda: _restate(d, img, v, z))
                    got = _process(e, d, img, v, z)
                    _check(got, want, 0, f"{w}x{h} exact={exact} velocity={kind} desc={kw}")
                    moved |= kind != "zero" and not np.array_equal(_bits(got), _bits(img))
        assert moved, "the blur should change some pixel"
        # the four output formats, with and without a manual display of each operator
        w, h = SIZE
        img, z, v = _image(w, h), _depth(w, h), _velocity("blocks", w, h)
        d = motion_blur_desc(samples=8, shutter=0.5)
        for op in (None,) + tuple(Tonemap):
            disp = display_desc(tonemap=op, exposure_ev=-1.5) if op is not None else None
            want = _ref(("fmt", op), lambda: _restate(d, img, v, z, op, display_ref.manual_scale(-1.5) if op is not None else None))
            for fmt in range(4):
                _check(_process(e, d, img, v, z, fmt, disp), want, fmt, f"exact={exact} {op} fmt={fmt}")
    e.close()


# ---------------------------------------------------------------- 2. properties that do not rest on the restatement
@pytest.mark.parametrize("exact", [True, False])
def test_properties_of_the_filter(exact):
    e = Engine(device=0, exact=exact)
    w, h = SIZE
    z = _depth(w, h)
    # zero velocity: the output bits are the input bits, special values included
    for (sw, sh) in SIZES:
        img = _image(sw, sh)
        got = _process(e, motion_blur_desc(samples=8), img, _velocity("zero", sw, sh), _depth(sw, sh))
        assert np.array_equal(_bits(got), _bits(img)), (sw, sh)
    # a uniform finite colour under any velocity field comes back within (S + 1) 2^-24 <= 4e-6 relative: a weighted mean of at most 33 equal terms
    flat = np.broadcast_to(np.array([0.3, 2.5, 7.0, 1.0], np.float32), (h, w, 4)).copy()
    for kind in ("uniform", "blocks", "nan"):
        for samples in (2, 8, 32):
            got = _process(e, motion_blur_desc(samples=samples, shutter=1.0), flat, _velocity(kind, w, h), z)
            err = np.abs(got[..., :3].astype(np.float64) / flat[..., :3].astype(np.float64) - 1.0).max()
            print(f"uniform colour, velocity={kind} S={samples}: max relative error {err:.3g}")
            assert err <= 4e-6 and (got[..., 3] == 1).all(), (kind, samples, err)
    # a static pixel farther than R + 32 pixels (Chebyshev) from every moving pixel is untouched bit for bit. (Colours in [0, 65504]: such a
    # pixel may still lie in a tile next to a moving one, where it is c(X) 2 / 2, and c clamps what the rest path passes through.)
    ww, hh, rad = 130, 40, 16.0
    img = np.minimum(_image(ww, hh, seed=4, spoil=False), np.float32(60000.0))
    img[..., 3] = 1.0   # (the gather writes alpha 1)
    v = np.zeros((hh, ww, 2), np.float32)
    v[:, :10] = (100.0, 30.0)
    got = _process(e, motion_blur_desc(samples=8, shutter=1.0, max_radius=rad), img, v, np.full((hh, ww), 3.0, np.float32))
    far = 9 + int(rad) + 32 + 1
    assert np.array_equal(_bits(got[:, far:]), _bits(img[:, far:]))
    assert not np.array_equal(_bits(got[:, :10]), _bits(img[:, :10]))
    # a static near object over a fast far background: every tap's weight is exactly 0 on the object, which comes back as c(X)
    img = _image(w, h, seed=8)
    v = np.broadcast_to(np.array([150.0, 40.0], np.float32), (h, w, 2)).copy()
    zz = np.full((h, w), 50.0, np.float32)
    v[10:40, 20:50] = 0.0
    zz[10:40, 20:50] = 2.0
    for samples, jitter in ((2, False), (8, True), (32, True)):
        got = _process(e, motion_blur_desc(samples=samples, shutter=0.5, jitter=jitter), img, v, zz)
        want = bloom_ref.rgba(R.colour(img))
        assert np.array_equal(_bits(got[10:40, 20:50]), _bits(want[10:40, 20:50])), (samples, jitter)
        assert not np.array_equal(_bits(got[:10]), _bits(want[:10]))
    # one bright pixel under a uniform horizontal velocity: every other row is unchanged, and nothing beyond +-R of it changes even at |V| = 1000
    # (Unchanged bit for bit, not by luck of rounding: the background is 0.25, a power of two, so every product 0.25 w is exact and each
    # partial sum is 0.25 times the partial sum of the weights, rounded alike; sum / wsum is then (0.25 wsum) / wsum = 0.25 exactly.)
    for rad in (8.0, 32.0):
        ww, hh = 100, 20
        img = np.full((hh, ww, 4), 0.25, np.float32)
        img[..., 3] = 1.0
        img[11, 50, :3] = 1000.0
        v = np.broadcast_to(np.array([1000.0, 0.0], np.float32), (hh, ww, 2)).copy()
        got = _process(e, motion_blur_desc(samples=32, shutter=1.0, max_radius=rad), img, v, np.full((hh, ww), 3.0, np.float32))
        changed = _bits(got) != _bits(img)
        ys, xs = np.nonzero(changed.any(-1))
        assert len(xs) > 1 and (ys == 11).all() and (np.abs(xs - 50) <= rad).all(), (rad, ys, xs)
    e.close()


# ---------------------------------------------------------------- 3. whole frames
STEPS = (0.07, 0.05, 0.09, 0.06, 0.08, 0.05, 0.1, 0.055)   # the camera's sideways step in front of frame k + 1


def _eye(scene, k):
    base = (0.0, 1.0, 3.2) if scene == "cornell" else (-5.75, 0.5, -16.8)
    target = (0.0, 1.0, 0.0) if scene == "cornell" else (-5.75, 0.5, -17.0)
    dx = sum(STEPS[:k]) * (5.0 if scene == "cornell" else 1.0)   # a different step every frame, each a few pixels at 72 x 52
    return (base[0] + dx, base[1] + 0.4 * dx, base[2]), (target[0] + 0.3 * dx, target[1], target[2])


def _cam(scene, k, mode=CameraMode.IMAGE, denoise=True, size=SIZE):
    eye, target = _eye(scene, k)
    return scenes.camera_for(size, eye, target, mode, denoise)


TUBE_EYE, TUBE_TARGET = deform.SCENES["cornell"][3], deform.SCENES["cornell"][4]


def _advance_tubes(e, cam, step, mode, stream):
    """test_gpu_deform_motion's tubes re-posed (three of its steps at once: the frame is a quarter of its size), the last one also moved by its
    transform, under a static camera; one tick"""
    for i, inst in enumerate(e._ids):
        e.set_pose(inst, deform.pose(3 * step, i))
    x, y, z = deform.POSITIONS[-1]
    e.insert_instance(e._ids[-1], Instance(deform.TUBE, deform.TUBE_MAT, deform.tube_xform(x + 0.09 * (step + 1), y, z)))
    e.update_camera(cam, scenes.camera_for(SIZE, TUBE_EYE, TUBE_TARGET, mode))
    e.tick(stream)


class Planes:
    """the velocity map and the G-buffer of the frame just rendered, read back from a camera that blurs. Which of the two G-buffers the
    frame wrote is found by what changed since the last look (under a static camera the two are equal anyway)."""

    def __init__(self):
        self.prev = {}

    def read(self, e, cam, size=SIZE):
        v = e.read_buffer(cam, Buffer.VELOCITY_MAP)
        g = {b: e.read_buffer(cam, b) for b in (Buffer.PRIM_GBUFFER_D0_A, Buffer.PRIM_GBUFFER_D0_B)}
        changed = [b for b in g if b not in self.prev or not np.array_equal(_bits(self.prev[b]), _bits(g[b]))]
        if len(self.prev) == 0:   # the first frame: the other plane is still zero
            changed = [b for b in g if _bits(g[b]).any()]
        self.prev = g
        cur = g[changed[0]] if changed else g[Buffer.PRIM_GBUFFER_D0_A]
        assert len(changed) <= 1, "a frame writes one of the two G-buffers"
        w, h = size
        return v.reshape(h, w, 4)[..., :2].copy(), R.frame_depth(cur.reshape(h, w, 4)[..., 0])


FRAME_CASES = [
    # name, exact, scene, mode, what moves, display, bloom, post
    ("cornell_image_camera", False, "cornell", CameraMode.IMAGE, "camera", None, None, False),
    ("dungeon_image_camera_chain", False, "dungeon", CameraMode.IMAGE, "camera", dict(tonemap=Tonemap.ACES_FITTED, exposure_ev=0.5),
     dict(intensity=0.3, threshold=0.4, threshold_softness=0.5), True),
    ("dungeon_image_camera_auto", False, "dungeon", CameraMode.IMAGE, "camera", dict(tonemap=Tonemap.ACES_FITTED, auto_exposure=True, ev_min=-12.0, ev_max=8.0),
     None, False),
    ("cornell_di_diffuse_exact", True, "cornell", CameraMode.DI_DIFFUSE, "camera", dict(tonemap=Tonemap.ACES_FITTED, exposure_ev=0.0), None, False),
    ("cornell_gi_diffuse_tubes", False, "cornell", CameraMode.GI_DIFFUSE, "tubes", None, dict(intensity=0.25), False),
    ("cornell_image_tubes_exact", True, "cornell", CameraMode.IMAGE, "tubes", dict(tonemap=Tonemap.ACES_FITTED, auto_exposure=True, ev_min=-12.0, ev_max=8.0),
     dict(intensity=0.25), True),
]


@pytest.mark.parametrize("case", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_a_blurred_frame_equals_the_restatement_of_the_frame_without(case):
    name, exact, scene, mode, moves, display, bloom, with_post = case
    d = motion_blur_desc(shutter=1.0, samples=8)
    engines, cams = [], []
    for _ in range(2):   # a: plain; b: the blur and what follows it
        if moves == "tubes":   # test_gpu_deform_motion's re-posed tubes with deformation motion on: the previous-pose term is consumed
            e = deform.build(exact, True, scene=scene)
            e.keep_all_planes(False)
            cams.append(e.create_camera(scenes.camera_for(SIZE, TUBE_EYE, TUBE_TARGET, mode)))
        else:
            e = _engine(exact, scene)
            cams.append(e.create_camera(_cam(scene, 0, mode)))
        engines.append(e)
    (a, b), (ca, cb) = engines, cams
    b.set_motion_blur(cb, d)
    assert b.get_motion_blur(cb)[1]
    bd = bloom_desc(**bloom) if bloom else None
    if bd:
        b.set_bloom(cb, bd)
    if display:
        b.set_display(cb, **display)
    post = post_desc(fxaa=True, output_size=(108, 78), filter=ResampleFilter.CATMULL_ROM)
    if with_post:
        b.set_post(cb, post)
    planes, oa = Planes(), Out(0)
    changed = False
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(4):
        fmt = (0, 2, 1, 3)[k] if display else 0
        b.set_output_format(cb, OutputFormat(fmt))
        ob = Out(fmt, b.output_size(cb), fill=0x5a)
        scale = np.float32(b.exposure(cb)[0]) if display else None
        for e, cam, o in ((a, ca, oa), (b, cb, ob)):
            if moves == "tubes":
                _advance_tubes(e, cam, k, mode, stream)
            else:
                e.update_camera(cam, _cam(scene, k, mode)); e.tick(stream)
            e.render_camera(cam, o.ptr(), stream)
        torch.cuda.synchronize()
        plain, got = oa.get(), ob.get()
        assert not b.buffer_stale(cb, Buffer.VELOCITY_MAP)
        v, z = planes.read(b, cb)
        if k == 0:
            continue   # (the first frame has no previous camera: nothing moves yet)
        with np.errstate(all="ignore"):
            speed = np.hypot(v[..., 0], v[..., 1])
            print(f"{name} frame {k}: |V| max {np.nanmax(speed):.3f} px, {(speed >= 1.0).mean():.3f} of the pixels at 1 px or more")
            assert (speed >= 1.0).mean() > 0.005, f"{name}: the frame should hold moving pixels"
        ref = R.motion_blur(plain, v, z, d.shutter, d.samples, d.max_radius, d.depth_softness, d.flags)
        changed |= not np.array_equal(_bits(ref), _bits(plain))
        if bd:
            n, _, fac = b.bloom_plan(bd, *SIZE)
            ref = bloom_ref.rgba(bloom_ref.bloom(ref, fac, bd.flags, bd.threshold, bd.threshold_softness, bd.clamp))
        if display:
            ref = display_ref.transform(ref[..., :3], int(display["tonemap"]), scale)
        if with_post:
            ref = post_ref.process(ref, fxaa_on=True, out_size=(108, 78), flt=post_ref.CATMULL_ROM)
        _check(got, ref, fmt, f"{name} frame {k} fmt {fmt}")
        launches = b.last_launches()
        assert launches[-1] == PassBit.POST and sum(1 for x in launches if x & PassBit.POST) == 2, [hex(x) for x in launches]   # the pack launch, then the rest
    assert changed, "the blur should change some pixel"
    for e in engines:
        e.close()


# ---------------------------------------------------------------- 4. off is off
NODE = C.Node("set_motion_blur", "get_motion_blur", "the blur", "the camera moves: the blurred frame differs", (), dict(shutter=1.0),
              pipelined=dict(shutter=1.0, samples=8), recreated=dict(shutter=0.5))


@pytest.mark.parametrize("exact", [False, True])
def test_a_cleared_blur_renders_like_a_camera_that_never_had_one(exact):
    # five frames of this file's own camera path; a frame whose step is small need not differ; b's velocity map outlives the setting
    C.cleared_setting_renders_like_none(NODE, exact, camera=lambda k: _cam("cornell", k), frames=5, differs=False, unwritten_velocity=True)


@pytest.mark.parametrize("exact", [False, True])
def test_the_blur_over_a_static_scene_and_camera_changes_only_the_velocity_map(exact):
    a, b = _engine(exact, "dungeon"), _engine(exact, "dungeon")
    ca, cb = a.create_camera(_cam("dungeon", 0)), b.create_camera(_cam("dungeon", 0))
    b.set_motion_blur(cb, shutter=1.0, samples=32)
    for e, cam in ((a, ca), (b, cb)):
        e.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
        e.set_display(cam, tonemap=Tonemap.ACES_FITTED, auto_exposure=True, ev_min=-12.0, ev_max=8.0)
    oa, ob = Out(2), Out(2)
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(3):
        for e, cam, o in ((a, ca, oa), (b, cb, ob)):
            e.tick(stream); e.render_camera(cam, o.ptr(), stream)
        torch.cuda.synchronize()
        assert np.array_equal(oa.get(), ob.get()), (exact, k)
        assert not b.buffer_stale(cb, Buffer.VELOCITY_MAP)
        assert a.buffer_stale(ca, Buffer.VELOCITY_MAP) == (not exact), "the default frame of the fast build keeps the velocity in registers"
        assert not _bits(b.read_buffer(cb, Buffer.VELOCITY_MAP)).any(), "nothing moves"
        pa, pb = _all_planes(a, ca), _all_planes(b, cb)
        for buf in Buffer:
            if buf != Buffer.VELOCITY_MAP:
                assert a.buffer_stale(ca, buf) == b.buffer_stale(cb, buf), (k, buf)
                assert np.array_equal(_bits(pa[buf]), _bits(pb[buf])), (exact, k, buf)
        assert a.exposure(ca) == b.exposure(cb)
    a.close(); b.close()


# ---------------------------------------------------------------- 5. nothing else changes
def test_aovs_picks_and_the_exposure_do_not_depend_on_the_blur():
    # nothing moves in front of frame 0; the blur makes the frame keep its velocity map
    C.nothing_else_depends_on_the_setting(NODE, camera=lambda k: _cam("dungeon", k), differs_from=1, velocity_map=False)


@pytest.mark.parametrize("mode", [CameraMode.REFERENCE, CameraMode.BVH_HEATMAP])
def test_modes_without_a_velocity_map_skip_the_blur(mode):
    a, b = _engine(True), _engine(True)
    ca, cb = a.create_camera(_cam("cornell", 0, mode, False)), b.create_camera(_cam("cornell", 0, mode, False))
    b.set_motion_blur(cb, shutter=2.0)
    oa, ob = Out(0), Out(0)
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(2):
        for e, cam, o in ((a, ca, oa), (b, cb, ob)):
            e.update_camera(cam, _cam("cornell", k, mode, False)); e.tick(stream); e.render_camera(cam, o.ptr(), stream)
        torch.cuda.synchronize()
        assert_bits_equal(ob.get(), oa.get(), f"{mode.name} with the blur set, frame {k}")
        assert b.last_launches() == a.last_launches() and not any(l & PassBit.POST for l in b.last_launches())
    a.close(); b.close()


# ---------------------------------------------------------------- 6. pipelining
def test_frames_in_flight_read_their_own_velocities():
    C.frames_in_flight_read_their_own_inputs(NODE, camera=lambda k: _cam("dungeon", k))   # a different amount every frame: frame k + 1's velocities are not frame k's


# ---------------------------------------------------------------- 7. lifecycle
def test_updates_arithmetic_switches_two_cameras_and_teardown():
    a, b = _engine(False), _engine(False)
    d1, d2 = motion_blur_desc(shutter=1.0, samples=8), motion_blur_desc(shutter=2.0, samples=2, max_radius=8.0, jitter=False)
    stream = torch.cuda.current_stream().cuda_stream
    ca, cb, cb2 = a.create_camera(_cam("cornell", 0)), b.create_camera(_cam("cornell", 0)), b.create_camera(_cam("cornell", 0))
    b.set_motion_blur(cb, d1); b.set_motion_blur(cb2, d2)
    p1, p2 = Planes(), Planes()
    step = 0
    for size in (SIZE, (96, 80), (40, 24), SIZE):   # larger, smaller, back: the setting and the results stay
        if size == SIZE and step:
            for e in (a, b):
                e.set_exact(True); e.set_exact(False)   # ... and across an arithmetic switch
        for rep_ in range(2):
            oa, ob, ob2 = Out(0, size), Out(0, size), Out(0, size)
            for e, cam, o in ((a, ca, oa), (b, cb, ob)):
                e.update_camera(cam, _cam("cornell", step, size=size))
            b.update_camera(cb2, _cam("cornell", step, size=size))
            a.tick(stream); b.tick(stream)
            a.render_camera(ca, oa.ptr(), stream); b.render_camera(cb, ob.ptr(), stream); b.render_camera(cb2, ob2.ptr(), stream)
            torch.cuda.synchronize()
            assert b.get_motion_blur(cb)[1] and b.get_motion_blur(cb2)[0].samples == 2
            plain = oa.get()
            if rep_ == 0:   # (a resize starts the planes afresh: look once so that Planes knows them)
                p1, p2 = Planes(), Planes()
            for cam, o, d, p in ((cb, ob, d1, p1), (cb2, ob2, d2, p2)):
                v, z = p.read(b, cam, size)
                ref = R.motion_blur(plain, v, z, d.shutter, d.samples, d.max_radius, d.depth_softness, d.flags)
                _check(o.get(), ref, 0, f"size {size} step {step} samples {d.samples}")
            step += 1
    # process calls on two streams share the engine's planes: the engine orders them
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    ia, ib = _image(72, 52), _image(64, 64, seed=2)
    va, vb, za, zb = _velocity("blocks", 72, 52), _velocity("uniform", 64, 64), _depth(72, 52), _depth(64, 64)
    t = [torch.from_numpy(x).cuda() for x in (ia, va, za, ib, vb, zb)]
    oa, ob = Out(0, (72, 52)), Out(0, (64, 64))
    torch.cuda.synchronize()
    for _ in range(4):
        b.motion_blur_process(d1, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 72, 52, oa.ptr(), 0, stream=sa.cuda_stream)
        b.motion_blur_process(d2, t[3].data_ptr(), t[4].data_ptr(), t[5].data_ptr(), 64, 64, ob.ptr(), 0, stream=sb.cuda_stream)
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        _check(oa.get(), _restate(d1, ia, va, za), 0, "stream a")
        _check(ob.get(), _restate(d2, ib, vb, zb), 0, "stream b")
    # delete a camera with the blur on and a frame in flight; a new camera starts clean; destroy the engine with a blurred frame in flight
    C.teardown_with_the_setting_on(NODE, b, cb, _cam("cornell", 0))
    a.close(); b.close()
