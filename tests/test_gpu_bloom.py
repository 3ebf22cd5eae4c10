"""GPU tests of bloom (include/strolle_hip.h "bloom"; k_bloom.hip, st_bloom.cpp): st_bloom_process on synthetic HDR images against the
numpy restatement (bloom_ref.py, fed the factors st_bloom_plan reports) bit for bit in both builds; whole frames with bloom and a display
on against the restatement of the same frame rendered with both off; off is off; AOVs, picks, planes and the exposure do not change;
heatmap frames; scheduling; reallocation; lifecycle; tiles. Every test builds its own engines. All of them use entry points the parent
commit does not have.

The straightforward chain (one launch per level each way) ships; the fused tail (one single-workgroup launch for the last levels, k_bloom.hip
k_bloom_tail) measured slower and is off unless st_debug_set_bloom_tail turns it on. One test asserts that the two give equal bits."""
import numpy as np
import pytest
import torch

import bloom_ref as R
import display_ref
import output_chain as C
import post_ref
from output_chain import SIZE, Out, _camera, _check, _engine, _frame, _image
from parity import assert_bits_equal, bits_equal_mask
from strolle_amd import (Aov, Buffer, CameraMode, Engine, OutputFormat, PassBit, ResampleFilter, Tonemap, aov_planes, bloom_desc, display_desc,
                         post_desc)

pytestmark = pytest.mark.gpu
# SIZE (72 x 52) is not a multiple of the bloom tile (32 x 8); five levels fit (36x26 .. 3x2)


def _restate(e, d, frame, display=None, scale=None):
    """the restatement of `frame` (RGBA32F, display off, bloom off) through bloom `d` and the display (tonemap, scale): RGBA32F"""
    h, w = frame.shape[:2]
    n, _, fac = e.bloom_plan(d, w, h)
    assert n == len(R.plan_sizes(w, h, d.levels))
    c = R.bloom(frame, fac, d.flags, d.threshold, d.threshold_softness, d.clamp)
    if display is None:
        return R.rgba(c)
    return display_ref.transform(c, int(display), scale)


# ---------------------------------------------------------------- 1. synthetic images through st_bloom_process
SMALL = [(70, 45), (64, 48), (33, 21), (9, 7), (5, 5), (2, 7)]   # even, odd, non-square; 9 x 7 and 5 x 5 reduce the level count; 2 x 7 holds no level


def _ref(key, make):
    return C._ref(__name__, key, make)


def _process(e, d, img, src, fmt=0, display=None):
    h, w = img.shape[:2]
    out = Out(fmt, (w, h), fill=0x5a)
    e.bloom_process(d, src.data_ptr(), w, h, out.ptr(), fmt, display=display, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.get()


@pytest.mark.parametrize("exact", [True, False])
def test_bloom_process_matches_the_restatement_on_synthetic_images(exact):
    e = Engine(device=0, exact=exact)
    for (w, h) in SMALL:
        img = _image(w, h)
        src = torch.from_numpy(img).cuda()
        for flags in range(4):
            for thr in (0.0, 1.5):
                for levels in (1, 2, 6, 8):
                    d = bloom_desc(intensity=0.3 if not flags & 1 else 0.6, additive=bool(flags & 1), firefly_suppress=bool(flags & 2), levels=levels,
                                   low_frequency_boost=0.6, low_frequency_boost_curvature=0.9, high_pass_frequency=0.8, threshold=thr,
                                   threshold_softness=0.4, clamp=0.0 if levels != 2 else 50.0)
                    want = _ref((w, h, flags, thr, levels), lambda: _restate(e, d, img))
                    _check(_process(e, d, img, src), want, 0, f"{w}x{h} exact={exact} flags={flags} threshold={thr} levels={levels}")
    # the four output formats with a manual display of each operator
    w, h = 70, 45
    img = _image(w, h)
    src = torch.from_numpy(img).cuda()
    d = bloom_desc(intensity=0.25, levels=4, threshold=1.0, threshold_softness=0.5)
    for op in Tonemap:
        disp = display_desc(tonemap=op, exposure_ev=-1.5)
        want = _ref(("fmt", int(op)), lambda: _restate(e, d, img, op, display_ref.manual_scale(-1.5)))
        for fmt in range(4):
            _check(_process(e, d, img, src, fmt, disp), want, fmt, f"exact={exact} {op.name} fmt={fmt}")
    # 301 x 203: every level but the last spans several workgroups, both sides odd at several levels
    img = _image(301, 203, seed=5)
    src = torch.from_numpy(img).cuda()
    for flags, levels in ((0, 6), (3, 8)):
        d = bloom_desc(intensity=0.4, additive=bool(flags & 1), firefly_suppress=bool(flags & 2), levels=levels, threshold=2.0, threshold_softness=0.7)
        want = _ref(("mid", flags, levels), lambda: _restate(e, d, img))
        _check(_process(e, d, img, src), want, 0, f"301x203 exact={exact} flags={flags} levels={levels}")
    e.close()


@pytest.mark.parametrize("exact", [True, False])
def test_bloom_process_at_1080p(exact):
    e = Engine(device=0, exact=exact)
    img = _ref("1080p image", lambda: _image(1920, 1080, seed=3))
    src = torch.from_numpy(img).cuda()
    d = bloom_desc(intensity=0.15, firefly_suppress=True, levels=6, threshold=1.0, threshold_softness=0.5)
    assert e.bloom_plan(d, 1920, 1080)[1] == [(960, 540), (480, 270), (240, 135), (120, 68), (60, 34), (30, 17)]
    want = _ref("1080p", lambda: _restate(e, d, img, Tonemap.ACES_FITTED, display_ref.manual_scale(0.0)))
    _check(_process(e, d, img, src, 0, display_desc(tonemap=Tonemap.ACES_FITTED)), want, 0, f"1920x1080 exact={exact}")
    e.close()


def _tail_first(sizes, budget):
    """st_bloom.cpp bloom_tail_first: the first level the fused tail takes (len(sizes): none)"""
    t, used = len(sizes), 0
    while t > 1 and used + sizes[t - 1][0] * sizes[t - 1][1] * 12 <= budget:
        used += sizes[t - 1][0] * sizes[t - 1][1] * 12
        t -= 1
    return t


@pytest.mark.parametrize("exact", [True, False])
def test_the_fused_tail_and_the_straightforward_chain_give_equal_bits(exact):
    e = Engine(device=0, exact=exact)
    limit = e.set_bloom_tail(-1)
    assert limit >= 64 << 10, "a workgroup may always have 64 KiB of LDS"
    assert e.set_bloom_tail(0) == 0 and e.set_bloom_tail(4096) == 4096 and e.set_bloom_tail(1 << 30) == limit
    for (w, h), levels, flags in (((301, 203), 8, 3), ((70, 45), 6, 0), ((640, 360), 6, 2), ((1920, 1080), 6, 1), ((33, 21), 2, 0)):
        img = _ref(("tail image", w, h), lambda: _image(w, h, seed=9))
        src = torch.from_numpy(img).cuda()
        d = bloom_desc(intensity=0.35, additive=bool(flags & 1), firefly_suppress=bool(flags & 2), levels=levels, threshold=1.0, threshold_softness=0.5)
        sizes = e.bloom_plan(d, w, h)[1]
        assert _tail_first(sizes, limit) < len(sizes), "the device's budget puts at least the last level into the tail"
        e.set_bloom_tail(0)
        plain = _process(e, d, img, src)
        firsts = set()
        for budget in (-1, 64 << 10, 16 << 10, 2048):   # tails of several lengths, the longest the device allows down to the last level or two
            in_force = e.set_bloom_tail(budget)
            firsts.add(_tail_first(sizes, in_force))
            got = _process(e, d, img, src)
            assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)), (exact, w, h, levels, flags, budget)
        if len(sizes) > 3:
            assert len(firsts) > 1, "the budgets should cut the chain at different levels"
    e.close()
    # a camera's frames: an engine that runs the straightforward chain renders the bytes of one that runs the tail
    a, b = _engine(exact, "dungeon"), _engine(exact, "dungeon")
    assert a.set_bloom_tail(-1) > 0 and b.set_bloom_tail(0) == 0
    desc = _camera("dungeon", size=(200, 120))
    ca, cb = a.create_camera(desc), b.create_camera(desc)
    for eng, cam in ((a, ca), (b, cb)):
        eng.set_display(cam, tonemap=Tonemap.ACES_FITTED, auto_exposure=True, ev_min=-12.0, ev_max=8.0)
        eng.set_bloom(cam, intensity=0.3, firefly_suppress=True)
    oa, ob = Out(0, (200, 120)), Out(0, (200, 120))
    for k in range(3):
        x, y = _frame(a, ca, oa), _frame(b, cb, ob)
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (exact, k)
        assert a.last_launches() == b.last_launches()
    a.close(); b.close()


def test_bloom_process_on_two_streams_shares_the_pyramid_in_order_and_is_deterministic():
    e = Engine(device=0)
    a, b = _image(70, 45), _image(64, 48, seed=2)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    da, db = bloom_desc(intensity=0.3, levels=5), bloom_desc(intensity=0.5, additive=True, levels=3, threshold=1.0)
    oa, ob = Out(0, (70, 45)), Out(0, (64, 48))
    torch.cuda.synchronize()
    for _ in range(4):   # alternate without a host sync: the engine orders the users of its pyramid
        e.bloom_process(da, ta.data_ptr(), 70, 45, oa.ptr(), 0, stream=sa.cuda_stream)
        e.bloom_process(db, tb.data_ptr(), 64, 48, ob.ptr(), 0, stream=sb.cuda_stream)
    torch.cuda.synchronize()
    assert_bits_equal(oa.get(), _restate(e, da, a), "stream a")
    assert_bits_equal(ob.get(), _restate(e, db, b), "stream b")
    e.close()


# ---------------------------------------------------------------- 2. whole frames
NATURAL = dict(intensity=0.3, low_frequency_boost=0.7, low_frequency_boost_curvature=0.95, threshold=0.0)
FRAME_CASES = [
    # name, exact, scene, mode, denoise, depth, tuning, display, bloom
    ("image_fused_compose", False, "cornell", CameraMode.IMAGE, True, 0, None, dict(tonemap=Tonemap.ACES_FITTED, exposure_ev=0.5), NATURAL),
    ("image_fused_compose_dungeon", False, "dungeon", CameraMode.IMAGE, True, 0, None, dict(tonemap=Tonemap.REINHARD, exposure_ev=-1.0),
     dict(intensity=0.5, additive=True, firefly_suppress=True, threshold=0.6, threshold_softness=0.5, levels=3)),
    ("image_no_fuse_compose", False, "cornell", CameraMode.IMAGE, True, 0, dict(fuse_compose=0), dict(tonemap=Tonemap.PBR_NEUTRAL, exposure_ev=0.0), NATURAL),
    ("no_display", False, "cornell", CameraMode.IMAGE, True, 0, None, None, NATURAL),
    ("reference", False, "cornell", CameraMode.REFERENCE, False, 1, None, dict(tonemap=Tonemap.REINHARD_LUMINANCE, exposure_ev=1.0), NATURAL),
    ("display_auto", False, "dungeon", CameraMode.IMAGE, True, 0, None, dict(tonemap=Tonemap.PBR_NEUTRAL, auto_exposure=True, ev_min=-12.0, ev_max=8.0), NATURAL),
    ("display_auto_no_fuse_compose", False, "cornell", CameraMode.IMAGE, True, 0, dict(fuse_compose=0),
     dict(tonemap=Tonemap.ACES_FITTED, auto_exposure=True, ev_min=-12.0, ev_max=8.0), dict(intensity=0.2, firefly_suppress=True, levels=8)),
    ("exact", True, "cornell", CameraMode.IMAGE, True, 0, None, dict(tonemap=Tonemap.ACES_FITTED, exposure_ev=0.25), NATURAL),
    ("exact_dungeon_auto", True, "dungeon", CameraMode.IMAGE, False, 0, None, dict(tonemap=Tonemap.NONE, auto_exposure=True, ev_min=-12.0, ev_max=8.0),
     dict(intensity=0.4, additive=True, levels=2)),
]


@pytest.mark.parametrize("case", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_a_frame_with_bloom_equals_the_restatement_of_the_frame_without(case):
    name, exact, scene, mode, denoise, depth, tuning, display, bloom = case
    a, b, c = _engine(exact, scene), _engine(exact, scene), _engine(exact, scene)   # plain; bloom + display; display alone (for the exposure)
    desc = _camera(scene, mode, denoise, depth)
    ca, cb, cc = a.create_camera(desc), b.create_camera(desc), c.create_camera(desc)
    for e in (a, b, c):
        if tuning:
            e.set_tuning(**tuning)
    d = bloom_desc(**bloom)
    b.set_bloom(cb, d)
    if display:
        b.set_display(cb, **display)
        c.set_display(cc, **display)
    auto = bool(display and display.get("auto_exposure"))
    post = post_desc(fxaa=True, output_size=(108, 78), filter=ResampleFilter.CATMULL_ROM)
    oa, oc = Out(0), Out(0)
    changed = False
    for k in range(5):
        fmt = (0, 2, 1, 0, 3)[k]
        with_post = k >= 3   # FXAA and the resampler behind the bloom
        b.set_post(cb, post if with_post else None)
        b.set_output_format(cb, OutputFormat(fmt))
        ob = Out(fmt, b.output_size(cb), fill=0x5a)
        scale = np.float32(b.exposure(cb)[0]) if display else None
        plain = _frame(a, ca, oa)
        got = _frame(b, cb, ob)
        _frame(c, cc, oc)
        ref = _restate(b, d, plain, display["tonemap"] if display else None, scale)
        changed |= not bits_equal_mask(ref[..., :3], (display_ref.transform(plain, int(display["tonemap"]), scale) if display else plain)[..., :3]).all()
        if with_post:
            ref = post_ref.process(ref, fxaa_on=True, out_size=(108, 78), flt=post_ref.CATMULL_ROM)
        _check(got, ref, fmt, f"{name} frame {k} fmt {fmt} post {with_post}")
        if auto:   # the metering saw the composed frame before bloom: the same histogram and exposure as with the display alone
            assert np.array_equal(b.camera_histogram(cb), c.camera_histogram(cc)) and b.exposure(cb) == c.exposure(cc), k
        launches = b.last_launches()
        assert launches[-1] == PassBit.POST and sum(1 for x in launches if x & PassBit.POST) == 1, [hex(x) for x in launches]
    assert changed, "bloom should change some pixel"
    for e in (a, b, c):
        e.close()


# ---------------------------------------------------------------- 3. off is off
@pytest.mark.parametrize("exact", [False, True])
def test_a_cleared_bloom_renders_like_a_camera_that_never_had_one(exact):
    for fmt, display in ((0, None), (2, dict(tonemap=Tonemap.ACES_FITTED, auto_exposure=True))):
        a, b = _engine(exact), _engine(exact)
        desc = _camera()
        ca, cb = a.create_camera(desc), b.create_camera(desc)
        for e, cam in ((a, ca), (b, cb)):
            e.set_output_format(cam, OutputFormat(fmt))
            if display:
                e.set_display(cam, **display)
        b.set_bloom(cb, intensity=0.3)
        oa, ob = Out(fmt), Out(fmt)
        x, y = _frame(a, ca, oa), _frame(b, cb, ob)   # a bloomed frame, then off
        assert any(l & PassBit.POST for l in b.last_launches()) and not np.array_equal(x.view(np.uint8), y.view(np.uint8))
        b.set_bloom(cb, None)
        for k in range(3):
            x, y = _frame(a, ca, oa), _frame(b, cb, ob)
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (exact, fmt, k)
            assert b.last_launches() == a.last_launches() and not any(l & PassBit.POST for l in b.last_launches())
        a.close(); b.close()


# ---------------------------------------------------------------- 4. independence
def test_aovs_picks_planes_and_the_exposure_do_not_depend_on_bloom():
    a, b = _engine(True), _engine(True)
    desc = _camera()
    ca, cb = a.create_camera(desc), b.create_camera(desc)
    for e, cam in ((a, ca), (b, cb)):
        e.set_display(cam, tonemap=Tonemap.ACES_FITTED, auto_exposure=True, ev_min=-12.0, ev_max=8.0)
    b.set_bloom(cb, intensity=0.4, firefly_suppress=True, threshold=0.5, threshold_softness=0.5)
    oa, ob = Out(0), Out(0)
    pixels = torch.tensor([[0, 0], [36, 26], [71, 51], [10, 40], [60, 5]], dtype=torch.uint32, device="cuda:0")
    for k in range(3):
        _frame(a, ca, oa); _frame(b, cb, ob)
        pa, pb = aov_planes(SIZE, fill=0), aov_planes(SIZE, fill=0)
        a.render_aovs(ca, pa); b.render_aovs(cb, pb)
        ha, hb = torch.zeros(5 * 64, dtype=torch.uint8, device="cuda:0"), torch.zeros(5 * 64, dtype=torch.uint8, device="cuda:0")
        a.pick(ca, pixels.data_ptr(), 5, ha.data_ptr()); b.pick(cb, pixels.data_ptr(), 5, hb.data_ptr())
        torch.cuda.synchronize()
        for kind in Aov:
            assert np.array_equal(pa[kind].cpu().view(torch.uint8).numpy(), pb[kind].cpu().view(torch.uint8).numpy()), (k, kind)
        assert np.array_equal(ha.cpu().numpy(), hb.cpu().numpy()), k
        for buf in Buffer:
            assert np.array_equal(a.read_buffer(ca, buf).view(np.uint32), b.read_buffer(cb, buf).view(np.uint32)), (k, buf)
        ea, eb = a.exposure(ca), b.exposure(cb)
        assert ea == eb and np.isfinite(ea[1]), (k, ea, eb)
        assert np.array_equal(a.camera_histogram(ca), b.camera_histogram(cb))
    a.close(); b.close()


# ---------------------------------------------------------------- 5. heatmap frames
def test_heatmap_frames_skip_bloom():
    a, b = _engine(True), _engine(True)
    desc = _camera(mode=CameraMode.BVH_HEATMAP)
    ca, cb = a.create_camera(desc), b.create_camera(desc)
    b.set_bloom(cb, intensity=0.5)
    plain, got = _frame(a, ca, Out(0)), _frame(b, cb, Out(0))
    assert_bits_equal(got, plain, "heatmap with bloom set")
    assert b.last_launches() == a.last_launches() and not any(l & PassBit.POST for l in b.last_launches())
    a.close(); b.close()


# ---------------------------------------------------------------- 6. scheduling
def _run(exact, tuning=None, streams=1, frames=6, present=False):
    e = _engine(exact, "dungeon")
    if tuning:
        e.set_tuning(**tuning)
    cam = e.create_camera(_camera("dungeon"))
    e.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
    e.set_display(cam, tonemap=Tonemap.ACES_FITTED, auto_exposure=True, ev_min=-12.0, ev_max=8.0)
    e.set_bloom(cam, intensity=0.3, threshold=0.4, threshold_softness=0.5)
    e.set_post(cam, fxaa=True, output_size=(144, 104), filter=ResampleFilter.CATMULL_ROM)
    ss = [torch.cuda.Stream() for _ in range(streams)]
    outs = [Out(2, (144, 104)) for _ in range(streams)]   # one buffer per stream: two frames in flight never share one
    hosts = [torch.zeros(144 * 104 * 4, dtype=torch.uint8).pin_memory() for _ in range(streams)]
    got = []
    for k in range(frames):
        i = k % streams
        s = ss[i].cuda_stream
        e.tick(s)
        e.render_camera(cam, outs[i].ptr(), s)   # no host sync between frames
        if present:
            e.present_copy(cam, outs[i].ptr(), hosts[i].data_ptr(), hosts[i].numel(), s)
        if k % streams == streams - 1:
            if present:
                for j in range(streams):
                    assert e.present_ready(cam, hosts[j].data_ptr(), wait=True)
                got += [hosts[j].numpy().reshape(104, 144, 4).copy() for j in range(streams)]
            else:
                torch.cuda.synchronize()
                got += [outs[j].get() for j in range(streams)]
    torch.cuda.synchronize()
    e.close()
    return got


def test_two_runs_two_streams_overlap_and_the_present_path_give_the_same_frames():
    for exact in (True, False):
        base = _run(exact)
        for kw in (dict(), dict(streams=2), dict(streams=2, tuning=dict(overlap=0)), dict(present=True), dict(streams=2, present=True)):
            other = _run(exact, **kw)
            assert len(other) == len(base)
            for k, (x, y) in enumerate(zip(other, base)):
                assert np.array_equal(x, y), (exact, kw, k)


def test_a_pass_mask_without_post_skips_the_bloom_launches():
    e = _engine(True)
    cam = e.create_camera(_camera())
    e.set_bloom(cam, intensity=0.3)
    out = Out(0, fill=0x5a)
    e.set_pass_mask(0xFFFFFFFFFFFFFFFF & ~int(PassBit.POST))
    _frame(e, cam, out)
    assert (out.t.cpu().numpy() == 0x5a).all(), "the composing launch wrote the camera's plane, nothing wrote the caller's buffer"
    assert e.last_launches()[-1] == PassBit.POST, "the launch group is listed, executed or not"
    e.set_pass_mask(0xFFFFFFFFFFFFFFFF)
    got = _frame(e, cam, out)
    assert np.isfinite(got).all() and (got[..., 3] == 1).all()
    e.close()


# ---------------------------------------------------------------- 7. reallocation and lifecycle
def test_render_size_and_level_changes_camera_updates_and_teardown_with_bloom_on():
    a, b = _engine(False), _engine(False)
    desc = _camera()
    ca, cb = a.create_camera(desc), b.create_camera(desc)
    disp = dict(tonemap=Tonemap.REINHARD, exposure_ev=0.5)
    b.set_display(cb, **disp)
    scale = display_ref.manual_scale(0.5)
    size = SIZE
    # the level count changes between frames (the pyramid is made again), then the render size, then both go back: the engine has no
    # memory accounting of its own, so a stable, correct result (and the engine-cycle test below) stands for "no leak"
    for k, (levels, new_size) in enumerate([(6, None), (2, None), (8, None), (3, (96, 80)), (6, None), (1, SIZE), (6, None), (0, (40, 24))]):
        if new_size:
            size = new_size
            a.update_camera(ca, _camera(size=size)); b.update_camera(cb, _camera(size=size))
        d = bloom_desc(intensity=0.35, levels=levels, threshold=0.5, threshold_softness=0.3)
        b.set_bloom(cb, d)
        plain = _frame(a, ca, Out(0, size))
        _check(_frame(b, cb, Out(0, size)), _restate(b, d, plain, Tonemap.REINHARD, scale), 0, f"step {k}: levels {levels} at {size}")
    assert b.bloom_plan(d, 40, 24)[0] == 4, "40 x 24 holds four of the six default levels"
    a.update_camera(ca, desc); b.update_camera(cb, desc)
    for e in (a, b):                                                            # the setting survives an arithmetic switch
        e.set_exact(True); e.set_exact(False)
    assert b.bloom(cb)[1]
    plain = _frame(a, ca, Out(0))
    _check(_frame(b, cb, Out(0)), _restate(b, d, plain, Tonemap.REINHARD, scale), 0, "after an arithmetic switch")
    # delete a camera with bloom on and a frame in flight; a new camera starts clean; destroy the engine with bloom on and a frame in flight
    stream = torch.cuda.current_stream().cuda_stream
    keep = Out(0)
    b.tick(stream); b.render_camera(cb, keep.ptr(), stream)
    b.delete_camera(cb)
    c2 = b.create_camera(desc)
    assert not b.bloom(c2)[1]
    b.set_bloom(c2, intensity=0.2, additive=True)
    assert np.isfinite(_frame(b, c2, Out(0))).all()
    b.tick(stream); b.render_camera(c2, keep.ptr(), stream)
    a.close(); b.close()


def test_engine_cycles_with_bloom_give_all_their_device_memory_back():
    """Whole engines come and go with a blooming camera (HDR plane, pyramid, fence) and st_bloom_process's pyramid, frames left in flight, one
    change of the render size. After a warm-up cycle the device's free memory after every later cycle equals its value after the warm-up."""
    stream = torch.cuda.current_stream().cuda_stream
    out = Out(0, (96, 80))
    img = torch.from_numpy(_image(70, 45)).cuda()
    small, large = _camera(), _camera(size=(96, 80))

    def cycle():
        e = _engine(False)
        cam = e.create_camera(small)
        e.set_display(cam, tonemap=Tonemap.ACES_FITTED, auto_exposure=True)
        e.set_bloom(cam, intensity=0.3)
        for k in range(4):
            if k == 2:
                e.update_camera(cam, large)
            e.tick(stream)
            e.render_camera(cam, out.ptr(), stream)
        e.bloom_process(bloom_desc(intensity=0.3), img.data_ptr(), 70, 45, out.ptr(), 0, stream=stream)
        e.delete_camera(cam)
        e.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    free = [cycle() for _ in range(4)]
    print("free device memory after each cycle (the first is the warm-up):", free)
    assert free[1:] == [free[0]] * 3, f"free device memory after the warm-up cycle {free[0]}, after the later ones {free[1:]}"


# ---------------------------------------------------------------- 8. tiles
def test_gathered_tiles_through_bloom_process_equal_the_single_engine_frame():
    size, world = (272, 200), 4
    stream = torch.cuda.current_stream().cuda_stream
    desc = _camera("cornell", CameraMode.REFERENCE, False, 1, size)
    d = bloom_desc(intensity=0.3, firefly_suppress=True, threshold=0.5, threshold_softness=0.5)
    disp = display_desc(tonemap=Tonemap.ACES_FITTED, exposure_ev=1.0)
    post = post_desc(fxaa=True, output_size=(408, 300), filter=ResampleFilter.CATMULL_ROM)
    one = _engine(True)
    cam = one.create_camera(desc)
    one.set_display(cam, disp); one.set_bloom(cam, d); one.set_post(cam, post)
    one.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
    single = Out(2, (408, 300))
    for _ in range(3):
        one.update_camera(cam, desc); one.tick(stream); one.render_camera(cam, single.ptr(), stream)
    torch.cuda.synchronize()
    ranks = []
    for r in range(world):
        e = _engine(True)
        c = e.create_camera(desc)   # display and bloom off: the ranks render RGBA32F
        e.dist_init_local(r, world, 7500)
        e.dist_set_partition(c, apron=0)
        ranks.append((e, c, torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda:0")))
    full = torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda:0")
    for _ in range(3):
        for r in range(world - 1, -1, -1):   # in-process transport: rank 0 last
            e, c, out = ranks[r]
            e.update_camera(c, desc); e.tick(stream)
            e.render_camera(c, out.data_ptr(), stream)
            e.dist_gather(c, out.data_ptr(), full.data_ptr() if r == 0 else 0, stream)
    root, root_cam, _ = ranks[0]
    root.dist_wait(root_cam, host=True)
    torch.cuda.synchronize()
    mid, tiled = Out(0, size), Out(2, (408, 300))
    root.bloom_process(d, full.data_ptr(), size[0], size[1], mid.ptr(), 0, display=disp, stream=stream)   # the recipe for tiled frames: rank 0, on the gathered frame
    root.post_process(post, mid.ptr(), size[0], size[1], tiled.ptr(), 2, stream)
    torch.cuda.synchronize()
    assert np.array_equal(tiled.get(), single.get()), "4 gathered tiles through st_bloom_process and st_post_process vs one engine with bloom"
    # a window and bloom: refused in either order
    e, c, _ = ranks[1]
    with pytest.raises(Exception):
        e.set_bloom(c, d)
    e.set_camera_rows(c, 0, size[1])
    e.set_bloom(c, d)
    with pytest.raises(Exception):
        e.dist_set_partition(c, apron=0)
    for e, *_ in ranks:
        e.dist_shutdown(); e.close()
    one.close()
