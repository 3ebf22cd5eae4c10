"""GPU tests of output post-processing (include/strolle_hip.h "post-processing"; k_post.hip, st_post.cpp): st_post_process on synthetic
images against the numpy restatement (post_ref.py) bit for bit in both builds; whole frames with post-processing on against the
restatement of the same frame rendered with it off; off is off; AOVs, picks and planes do not change; heatmap frames; scheduling;
lifecycle; tiles. Every test builds its own engines. All of them use entry points the parent commit does not have."""
import ctypes as C

import numpy as np
import pytest
import torch

import post_ref as R
from output_chain import SIZE, Out, _camera, _check, _engine, _frame
from parity import assert_bits_equal, bits_equal_mask
from strolle_amd import (Aov, Buffer, CameraMode, Engine, Instance, Material, OutputFormat, PassBit, ResampleFilter, Tonemap, aov_planes, post_desc,
                         scenes)

pytestmark = pytest.mark.gpu
# SIZE (72 x 52) is not a multiple of the FXAA tile (64 x 8) or of the resampler's (64 x 4)


def _kw(d):
    return dict(fxaa_on=bool(d.flags & 1), out_size=(d.output_width, d.output_height) if d.output_width else None, flt=d.filter,
                edge_threshold=d.fxaa_edge_threshold, edge_threshold_min=d.fxaa_edge_threshold_min, subpixel=d.fxaa_subpixel)


# ---------------------------------------------------------------- 1. synthetic images through st_post_process
def _images():
    rng = np.random.default_rng(11)
    noise = np.exp(rng.standard_normal((45, 70, 4)) * 2.0).astype(np.float32)   # HDR: far above 1 in places
    noise[rng.random((45, 70)) < 0.03] *= -1.0
    for v, n in ((np.nan, 25), (np.inf, 25), (-np.inf, 10), (0.0, 20), (-0.0, 10)):
        noise[rng.integers(0, 45, n), rng.integers(0, 70, n), rng.integers(0, 3, n)] = v
    ldr = rng.random((33, 129, 4)).astype(np.float32)                            # display-referred noise: most pixels are "edges"
    s1, _ = R.half_plane(130, 37, 1 / 8, 11.3)
    s2, _ = R.half_plane(130, 37, -2.5, 160.0)
    slanted = np.stack([0.1 + 0.8 * s1, 0.9 - 0.7 * s2 * s1, 0.2 + 0.6 * s2, np.ones_like(s1)], -1).astype(np.float32)
    lines = np.full((9, 65, 4), 0.05, np.float32)
    lines[4, :, :3] = (0.9, 0.8, 0.1)
    lines[:, 20, :3] = (0.2, 0.9, 0.9)
    ys, xs = np.mgrid[0:9, 0:65]
    lines[(xs - 2 * ys) % 23 == 0] = 1.0
    return {"hdr_noise": noise, "ldr_noise": ldr, "slanted": slanted, "thin_lines": lines}


def _ratios(w, h):
    return {"1:1": (w, h), "2x": (2 * w, 2 * h), "1.5x": (w * 3 // 2, h * 3 // 2), "3:2 non-uniform": (3 * w, 2 * h), "0.5x": (w // 2, h // 2)}


@pytest.mark.parametrize("exact", [True, False])
def test_post_process_matches_the_restatement_on_synthetic_images(exact):
    e = Engine(device=0, exact=exact)
    stream = torch.cuda.current_stream().cuda_stream
    for name, img in _images().items():
        h, w = img.shape[:2]
        src = torch.from_numpy(img).cuda()
        thresholds = [(0.0, 0.0, 0.75)] + ([(0.08, 0.02, 1.0), (0.3, 0.1, 0.0)] if name == "slanted" else [])
        for fxaa in (False, True):
            for et, etm, sub in (thresholds if fxaa else thresholds[:1]):
                base = R.fxaa(img, et, etm, sub) if fxaa else None
                for rname, (ow, oh) in _ratios(w, h).items():
                    for flt in ResampleFilter:
                        ref = base if base is not None else np.concatenate([img[..., :3], np.ones((h, w, 1), np.float32)], -1)
                        if (ow, oh) != (w, h):
                            ref = R.resample(ref, ow, oh, int(flt))
                        d = post_desc(fxaa=fxaa, output_size=(ow, oh), filter=flt, fxaa_edge_threshold=et, fxaa_edge_threshold_min=etm, fxaa_subpixel=sub)
                        for fmt in range(4):
                            out = Out(fmt, (ow, oh), fill=0x5a)
                            e.post_process(d, src.data_ptr(), w, h, out.ptr(), fmt, stream)
                            torch.cuda.synchronize()
                            _check(out.get(), ref, fmt, f"{name} exact={exact} fxaa={fxaa} {et, etm, sub} {rname} {flt.name} fmt={fmt}")
        # a desc that asks for nothing is a format-converting copy (alpha written as 1)
        out = Out(0, (w, h))
        e.post_process(post_desc(), src.data_ptr(), w, h, out.ptr(), 0, stream)
        torch.cuda.synchronize()
        assert bits_equal_mask(out.get()[..., :3], img[..., :3]).all() and (out.get()[..., 3] == 1).all()
    e.close()


def test_post_process_on_two_streams_shares_the_intermediate_plane_in_order():
    e = Engine(device=0)
    imgs = _images()
    a, b = imgs["slanted"], imgs["ldr_noise"]
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    da = post_desc(fxaa=True, output_size=(260, 74), filter=ResampleFilter.CATMULL_ROM)
    db = post_desc(fxaa=True, output_size=(64, 50), filter=ResampleFilter.BILINEAR)
    oa, ob = Out(0, (260, 74)), Out(0, (64, 50))
    torch.cuda.synchronize()
    for _ in range(4):   # alternate without a host sync: the engine orders the users of its intermediate plane
        e.post_process(da, ta.data_ptr(), a.shape[1], a.shape[0], oa.ptr(), 0, sa.cuda_stream)
        e.post_process(db, tb.data_ptr(), b.shape[1], b.shape[0], ob.ptr(), 0, sb.cuda_stream)
    torch.cuda.synchronize()
    assert_bits_equal(oa.get(), R.process(a, **_kw(da)), "stream a")
    assert_bits_equal(ob.get(), R.process(b, **_kw(db)), "stream b")
    e.close()


# ---------------------------------------------------------------- 2. whole frames
FRAME_CASES = [
    # name, exact, scene, mode, denoise, depth, tuning, display
    ("image_fused_compose", False, "cornell", CameraMode.IMAGE, True, 0, None, None),
    ("image_fused_compose_dungeon", False, "dungeon", CameraMode.IMAGE, True, 0, None, dict(tonemap=Tonemap.ACES_FITTED, exposure_ev=-1.0)),
    ("image_no_fuse_compose", False, "cornell", CameraMode.IMAGE, True, 0, dict(fuse_compose=0), None),
    ("reference", False, "cornell", CameraMode.REFERENCE, False, 1, None, None),
    ("display_manual", False, "dungeon", CameraMode.IMAGE, True, 0, None, dict(tonemap=Tonemap.REINHARD, exposure_ev=0.5)),
    ("display_auto", False, "dungeon", CameraMode.IMAGE, True, 0, None, dict(tonemap=Tonemap.PBR_NEUTRAL, auto_exposure=True, ev_min=-12.0, ev_max=8.0)),
    ("exact", True, "cornell", CameraMode.IMAGE, True, 0, None, dict(tonemap=Tonemap.ACES_FITTED, exposure_ev=0.25)),
    ("exact_dungeon_no_denoise", True, "dungeon", CameraMode.IMAGE, False, 0, None, None),
]


@pytest.mark.parametrize("case", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_a_frame_with_post_equals_the_restatement_of_the_frame_without(case):
    name, exact, scene, mode, denoise, depth, tuning, display = case
    a, b = _engine(exact, scene), _engine(exact, scene)
    desc = _camera(scene, mode, denoise, depth)
    ca, cb = a.create_camera(desc), b.create_camera(desc)
    for e, c in ((a, ca), (b, cb)):
        if tuning:
            e.set_tuning(**tuning)
        if display:
            e.set_display(c, **display)
    oa = Out(0)
    descs = [post_desc(fxaa=True), post_desc(fxaa=True, output_size=(144, 104), filter=ResampleFilter.CATMULL_ROM),
             post_desc(output_size=(108, 78), filter=ResampleFilter.BILINEAR), post_desc(fxaa=True, output_size=(36, 26), filter=ResampleFilter.NEAREST)]
    moved = 0
    for k in range(8):
        d, fmt = descs[k % 4], (0, 2, 1, 3, 0, 0, 0, 2)[k]
        b.set_post(cb, d)
        b.set_output_format(cb, OutputFormat(fmt))
        assert b.output_size(cb) == ((d.output_width, d.output_height) if d.output_width else SIZE)
        ob = Out(fmt, b.output_size(cb), fill=0x5a)
        plain = _frame(a, ca, oa)
        got = _frame(b, cb, ob)
        ref = R.process(plain, **_kw(d))
        _check(got, ref, fmt, f"{name} frame {k} fmt {fmt}")
        if k == 0:
            moved = int((~bits_equal_mask(ref[..., :3], plain[..., :3])).any(-1).sum())
        if display and display.get("auto_exposure"):   # the metering saw the render-size composed frame, as without post-processing
            assert np.array_equal(a.camera_histogram(ca), b.camera_histogram(cb)) and a.exposure(ca) == b.exposure(cb), k
        launches = b.last_launches()
        assert launches[-1] == PassBit.POST and sum(1 for x in launches if x & PassBit.POST) == 1, [hex(x) for x in launches]
    assert moved > 0, "FXAA should move some pixel of the first frame"
    a.close(); b.close()


# ---------------------------------------------------------------- 3. off is off
@pytest.mark.parametrize("exact", [False, True])
def test_a_cleared_post_and_a_desc_that_asks_nothing_render_like_none(exact):
    for fmt in range(4):
        a, b, c = _engine(exact), _engine(exact), _engine(exact)
        desc = _camera()
        cams = [e.create_camera(desc) for e in (a, b, c)]
        for e, cam in zip((a, b, c), cams):
            e.set_output_format(cam, OutputFormat(fmt))
        b.set_post(cams[1], fxaa=True, output_size=(100, 60))
        big = Out(fmt, (100, 60))
        _frame(b, cams[1], big)   # a post-processed frame, then off
        _frame(a, cams[0], Out(fmt)); _frame(c, cams[2], Out(fmt))
        b.set_post(cams[1], None)
        c.set_post(cams[2], post_desc(output_size=SIZE, filter=ResampleFilter.CATMULL_ROM))   # no flag, output size = render size
        assert b.output_size(cams[1]) == SIZE and c.output_size(cams[2]) == SIZE
        outs = [Out(fmt) for _ in range(3)]
        for k in range(3):
            x, y, z = (_frame(e, cam, o) for e, cam, o in zip((a, b, c), cams, outs))
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)) and np.array_equal(x.view(np.uint8), z.view(np.uint8)), (exact, fmt, k)
            assert b.last_launches() == a.last_launches() == c.last_launches()
            assert not any(l & PassBit.POST for l in b.last_launches())
        for e in (a, b, c):
            e.close()


# ---------------------------------------------------------------- 4. independence
def test_aovs_picks_and_planes_do_not_depend_on_post():
    a, b = _engine(True), _engine(True)
    desc = _camera()
    ca, cb = a.create_camera(desc), b.create_camera(desc)
    b.set_post(cb, fxaa=True, output_size=(216, 156), filter=ResampleFilter.BILINEAR)
    oa, ob = Out(0), Out(0, (216, 156))
    pixels = torch.tensor([[0, 0], [36, 26], [71, 51], [10, 40], [60, 5]], dtype=torch.uint32, device="cuda:0")   # render-size coordinates
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
        for buf in (Buffer.PRIM_GBUFFER_D0_A, Buffer.DI_DIFF_CURR_COLORS, Buffer.GI_DIFF_CURR_COLORS, Buffer.VELOCITY_MAP, Buffer.GI_RESERVOIRS_1):
            assert np.array_equal(a.read_buffer(ca, buf).view(np.uint32), b.read_buffer(cb, buf).view(np.uint32)), (k, buf)
    a.close(); b.close()


# ---------------------------------------------------------------- 5. heatmap frames
def test_heatmap_frames_are_resampled_but_not_anti_aliased():
    a, b = _engine(True), _engine(True)
    desc = _camera(mode=CameraMode.BVH_HEATMAP)
    ca, cb = a.create_camera(desc), b.create_camera(desc)
    oa = Out(0)
    plain = _frame(a, ca, oa)
    b.set_post(cb, fxaa=True)                                   # FXAA alone on false colour: nothing to do, no launch
    got = _frame(b, cb, Out(0))
    assert_bits_equal(got, plain, "heatmap with FXAA only")
    assert not any(l & PassBit.POST for l in b.last_launches())
    d = post_desc(fxaa=True, output_size=(144, 104), filter=ResampleFilter.BILINEAR)
    b.set_post(cb, d)
    got = _frame(b, cb, Out(0, (144, 104)))
    assert_bits_equal(got, R.resample(plain, 144, 104, R.BILINEAR), "heatmap resampled, not anti-aliased")
    assert not bits_equal_mask(R.process(plain, **_kw(d)), got).all(), "FXAA would have changed the heatmap"
    a.close(); b.close()


# ---------------------------------------------------------------- 6. scheduling
def _run(exact, tuning=None, streams=1, frames=6, present=False):
    e = _engine(exact, "dungeon")
    if tuning:
        e.set_tuning(**tuning)
    cam = e.create_camera(_camera("dungeon"))
    e.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
    e.set_display(cam, tonemap=Tonemap.ACES_FITTED, exposure_ev=-0.5)
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


def test_streams_overlap_and_the_present_path_give_the_same_frames():
    for exact in (True, False):
        base = _run(exact)
        for kw in (dict(streams=2), dict(tuning=dict(overlap=0)), dict(streams=2, tuning=dict(overlap=0)), dict(present=True), dict(streams=2, present=True)):
            other = _run(exact, **kw)
            assert len(other) == len(base)
            for k, (x, y) in enumerate(zip(other, base)):
                assert np.array_equal(x, y), (exact, kw, k)


def test_a_pass_mask_without_post_skips_the_post_launches():
    e = _engine(True)
    cam = e.create_camera(_camera())
    e.set_post(cam, fxaa=True, output_size=(144, 104))
    out = Out(0, (144, 104), fill=0x5a)
    e.set_pass_mask(0xFFFFFFFFFFFFFFFF & ~int(PassBit.POST))
    _frame(e, cam, out)
    assert (out.t.cpu().numpy() == 0x5a).all(), "the composing launch wrote the camera's plane, nothing wrote the caller's buffer"
    assert e.last_launches()[-1] == PassBit.POST, "the launch group is listed, executed or not"
    e.set_pass_mask(0xFFFFFFFFFFFFFFFF)
    got = _frame(e, cam, out)
    assert np.isfinite(got).all() and (got[..., 3] == 1).all()
    e.close()


# ---------------------------------------------------------------- 7. lifecycle
def test_output_size_changes_camera_updates_and_teardown_with_post_on():
    a, b = _engine(False), _engine(False)
    desc = _camera()
    ca, cb = a.create_camera(desc), b.create_camera(desc)
    oa = Out(0)
    for k, size in enumerate([(144, 104), (90, 65), (36, 26), (144, 104)]):   # the output size changes between frames
        d = post_desc(fxaa=True, output_size=size, filter=ResampleFilter.BILINEAR)
        b.set_post(cb, d)
        _check(_frame(b, cb, Out(0, size)), R.process(_frame(a, ca, oa), **_kw(d)), 0, f"output size {size}")
    for e in (a, b):                                                            # the setting survives an arithmetic switch
        e.set_exact(True); e.set_exact(False)
    _check(_frame(b, cb, Out(0, (144, 104))), R.process(_frame(a, ca, oa), **_kw(d)), 0, "after an arithmetic switch")
    big = _camera(size=(96, 80))                                                # another render size: the explicit output size is kept
    a.update_camera(ca, big); b.update_camera(cb, big)
    assert b.output_size(cb) == (144, 104)
    oa2 = Out(0, (96, 80))
    _check(_frame(b, cb, Out(0, (144, 104))), R.process(_frame(a, ca, oa2), **_kw(d)), 0, "after a resize")
    b.set_post(cb, fxaa=True)                                                   # ... and without one the output follows the render size
    d2 = post_desc(fxaa=True)
    _check(_frame(b, cb, Out(0, (96, 80))), R.process(_frame(a, ca, oa2), **_kw(d2)), 0, "FXAA at the new render size")
    # delete a camera with post-processing on and a frame in flight; a new camera starts clean; destroy the engine with post-processing on
    stream = torch.cuda.current_stream().cuda_stream
    keep = Out(0, (96, 80))
    b.tick(stream); b.render_camera(cb, keep.ptr(), stream)
    b.delete_camera(cb)
    c2 = b.create_camera(desc)
    assert not b.post(c2)[1] and b.output_size(c2) == SIZE
    b.set_post(c2, fxaa=True, output_size=(144, 104), filter=ResampleFilter.CATMULL_ROM)
    got = _frame(b, c2, Out(0, (144, 104)))
    assert np.isfinite(got).all()
    b.tick(stream); b.render_camera(c2, Out(0, (144, 104)).ptr(), stream)
    a.close(); b.close()


def test_engine_cycles_give_all_their_device_memory_back():
    """Whole engines come and go, each with every kind of device resource the host engine owns: Cornell, an environment map, a camera with an
    auto-exposure display and FXAA + resize, one skinned instance re-posed every tick with deformation motion on, a few frames at a small size
    left in flight, one change of the camera's size, st_camera_delete, st_engine_destroy. The output tensors are allocated once. After a
    warm-up cycle (code objects, the runtime's own pools) the device's free memory after every later cycle EQUALS its value after the warm-up
    cycle: an allocation, event or stream that teardown forgets shows up as a figure that shrinks from cycle to cycle.
    The commit before the owning types (teardown by enumeration) returned to the same value in this very test, five cycles out of five, so
    "equal" is what is asserted, not "does not grow"."""
    stream = torch.cuda.current_stream().cuda_stream
    outs = [Out(0, (144, 104)), Out(0, (144, 104))]
    env = np.random.default_rng(5).random((16, 32, 3)).astype(np.float32) + 0.05
    mesh, joints, weights = scenes.skinned_tube(8, 6, 4, length=1.2)
    small, large = _camera(), _camera(size=(96, 80))

    def cycle():
        e = _engine(False)
        e.set_environment(env, intensity=0.8)
        e.insert_material(7000, Material(base_color=(0.2, 0.7, 0.3, 1.0)))
        e.insert_mesh(7000, mesh); e.set_skin(7000, joints, weights, 4)
        e.insert_instance(7000, Instance(7000, 7000, np.array([[1, 0, 0, -0.4], [0, 1, 0, 0.0], [0, 0, 1, 0.0]], np.float32)))
        e.set_deformation_motion(True)
        cam = e.create_camera(small)
        e.set_display(cam, tonemap=Tonemap.ACES_FITTED, auto_exposure=True)
        e.set_post(cam, fxaa=True, output_size=(144, 104))
        for k in range(6):
            if k == 3:
                e.update_camera(cam, large)
            e.set_pose(7000, scenes.bend_pose(4, 1.6, 0.7 * k, length=1.2))
            e.tick(stream)
            e.render_camera(cam, outs[k & 1].ptr(), stream)
        assert e.deformation_stats()[0] == 1, "the last tick left the instance a previous pose"
        e.delete_camera(cam)
        e.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    free = [cycle() for _ in range(5)]
    print("free device memory after each cycle (the first is the warm-up):", free)
    assert np.isfinite(outs[0].get()).all() and np.isfinite(outs[1].get()).all()
    assert free[1:] == [free[0]] * 4, f"free device memory after the warm-up cycle {free[0]}, after the later ones {free[1:]}"


# ---------------------------------------------------------------- 8. tiles
def test_gathered_tiles_through_post_process_equal_the_single_engine_frame():
    size, world = (272, 200), 4
    stream = torch.cuda.current_stream().cuda_stream
    desc = _camera("cornell", CameraMode.REFERENCE, False, 1, size)
    d = post_desc(fxaa=True, output_size=(408, 300), filter=ResampleFilter.CATMULL_ROM)
    one = _engine(True)
    cam = one.create_camera(desc)
    one.set_display(cam, tonemap=Tonemap.ACES_FITTED, exposure_ev=1.0)
    one.set_post(cam, d)
    one.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
    single = Out(2, (408, 300))
    for _ in range(3):
        one.update_camera(cam, desc); one.tick(stream); one.render_camera(cam, single.ptr(), stream)
    torch.cuda.synchronize()
    ranks = []
    for r in range(world):
        e = _engine(True)
        c = e.create_camera(desc)
        e.set_display(c, tonemap=Tonemap.ACES_FITTED, exposure_ev=1.0)   # manual exposure works with tiles; post-processing does not
        e.dist_init_local(r, world, 7400)
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
    tiled = Out(2, (408, 300))
    root.post_process(d, full.data_ptr(), size[0], size[1], tiled.ptr(), 2, stream)   # the recipe for tiled frames: rank 0, on the gathered frame
    torch.cuda.synchronize()
    assert np.array_equal(tiled.get(), single.get()), "4 gathered tiles through st_post_process vs one engine with post-processing"
    # a window and post-processing: refused in either order
    e, c, _ = ranks[1]
    with pytest.raises(Exception):
        e.set_post(c, d)
    e.set_camera_rows(c, 0, size[1])
    e.set_post(c, d)
    with pytest.raises(Exception):
        e.dist_set_partition(c, apron=0)
    for e, *_ in ranks:
        e.dist_shutdown(); e.close()
    one.close()
