"""GPU tests of the upscale stage (include/strolle_hip.h "upscaling"; k_upscale.hip, st_upscale.cpp): st_upscale_process over the matrix of
tests/upscale_cases.py against the numpy restatement (upscale_ref.py) bit for bit in both builds and within the recorded tolerance of its
float64 definition; properties that do not rest on the restatement; whole frames with the stage on against the restatement of the same
frame rendered without it; off is off; nothing else depends on the setting; heatmap, reference and orthographic frames; gathered tiles;
frames in flight; lifecycle. Every test builds its own engines. All of them use entry points the parent commit does not have."""
import numpy as np
import pytest
import torch

import post_ref
import upscale_cases as K
import upscale_ref as U
from output_chain import SIZE, Node, Out, _bits, _camera, _check, _engine, _frame, _orthographic, _ref, nothing_else_depends_on_the_setting
from parity import assert_bits_equal, bits_equal_mask
from strolle_amd import CameraMode, Engine, OutputFormat, PassBit, ResampleFilter, Tonemap, scenes, upscale_desc
from test_upscale_abi import recorded

pytestmark = pytest.mark.gpu
BIG = (144, 104)   # SIZE (72 x 52) doubled; neither is a multiple of the kernels' 64 x 4 tile


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _process(e, img, out_size, sharpness, denoise, fmt=0):
    h, w = img.shape[:2]
    size = tuple(out_size) if out_size else (w, h)
    src = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    out = Out(fmt, size, fill=0x5a)
    e.upscale_process(upscale_desc(output_size=out_size, sharpness=sharpness, denoise=denoise), src.data_ptr(), w, h, out.ptr(), fmt, _stream())
    torch.cuda.synchronize()
    return out.get()


# ---------------------------------------------------------------- 1. the matrix through st_upscale_process
def _case_ref(case):
    """(the restatement's result, the definition's, the pixels left out of the float64 comparison), computed once for both builds"""
    name, size, _oname, osize, sharp, den = case
    return _ref(__name__, case, lambda: K.f64_comparison(K.source(name, size), osize, sharp, den, recorded()["r2_margin"]))


@pytest.mark.parametrize("exact", [True, False])
def test_upscale_process_matches_the_restatement_and_the_definition_over_the_matrix(exact):
    e = Engine(device=0, exact=exact)
    tol = recorded()["tolerance"]
    off, channels, worst = 0, 0, 0.0
    for case in K.cases():
        name, size, oname, osize, sharp, den = case
        img = K.source(name, size)
        ref, want64, skip = _case_ref(case)
        what = f"{name} {size} -> {oname} {osize} sharpness {sharp} limiter {den} exact={exact}"
        got = _process(e, img, osize, sharp, den, 0)
        assert_bits_equal(got, ref, what)
        assert np.isfinite(got).all() and (got[..., 3] == 1).all(), what   # every pixel written (the buffer was filled with 0x5a), finite, alpha 1
        assert skip.mean() <= 0.01, what
        worst = max(worst, K.deviation(got, want64, skip))
        assert worst <= tol, (what, worst, tol)
        for fmt in (1, 2, 3):
            got = _process(e, img, osize, sharp, den, fmt)
            want = post_ref.to_format(ref, fmt)
            if fmt == 1:
                assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), what
            else:   # tests/test_gpu_display.py's criterion, the share of exact channels taken over the whole matrix (a case may be one pixel)
                d = np.abs(got[..., :3].astype(np.int32) - want[..., :3].astype(np.int32))
                assert d.max() <= 1 and (got[..., 3] == 255).all(), (what, fmt)
                off += int((d != 0).sum()); channels += d.size
    print(f"exact={exact}: worst deviation from the definition {worst:.3e} (tolerance {tol:.3e}); {off} of {channels} 8-bit channels off by one")
    assert off <= 0.001 * channels
    e.close()


def test_a_desc_that_asks_for_neither_step_copies_the_image():
    e = Engine(device=0)
    img = K.source("spoiled", (37, 23))
    for d in (dict(out_size=None), dict(out_size=(37, 23))):
        got = _process(e, img, d["out_size"], 0.0, True)
        assert bits_equal_mask(got[..., :3], img[..., :3]).all() and (got[..., 3] == 1).all()
    _check(_process(e, img, None, 0.0, False, 2), U.process(img), 2, "the copy into RGBA8 sRGB")
    e.close()


# ---------------------------------------------------------------- 2. properties that do not rest on the restatement
@pytest.mark.parametrize("exact", [True, False])
def test_properties_of_the_two_steps(exact):
    e = Engine(device=0, exact=exact)
    tol = recorded()["tolerance"]
    # a constant image is unchanged by the upscaler and stays within the tolerance under the sharpening step
    for v in (0.0, 1.0, 0.3, 0.7071):
        img = np.full((23, 37, 4), v, np.float32)
        for size in ((37, 23), (38, 24), (56, 35), (74, 46), (111, 69)):
            if size != (37, 23):
                assert (_process(e, img, size, 0.0, False)[..., :3] == np.float32(v)).all(), (v, size)
            for den in (False, True):
                got = _process(e, img, size, 1.0, den)
                assert np.abs(got[..., :3].astype(np.float64) - np.float64(np.float32(v))).max() <= tol, (v, size, den)
    # the upscaler's output lies within the min / max of its four nearest texels (of the clamped colour), every pixel written and finite
    for name in ("noise", "spoiled", "slanted"):
        img = K.source(name, (72, 52))
        unit = U.unit(img)
        for size in ((73, 53), (96, 70), (144, 104), (216, 156), (144, 52)):
            got = _process(e, img, size, 0.0, False)
            assert np.isfinite(got).all() and (got[..., 3] == 1).all(), (name, size)
            ix, _, _ = post_ref.axis_resample(72, size[0])
            iy, _, _ = post_ref.axis_resample(52, size[1])
            x0, x1, y0, y1 = np.clip(ix, 0, 71)[None, :], np.clip(ix + 1, 0, 71)[None, :], np.clip(iy, 0, 51)[:, None], np.clip(iy + 1, 0, 51)[:, None]
            four = np.stack([unit[y0, x0], unit[y0, x1], unit[y1, x0], unit[y1, x1]])
            assert (got[..., :3] >= four.min(0)).all() and (got[..., :3] <= four.max(0)).all(), (name, size)
    # a blurred checker's Laplacian energy grows with sharpness
    ys, xs = np.mgrid[0:52, 0:72]
    checker = np.where(((xs // 4) + (ys // 4)) % 2 == 0, 0.75, 0.25).astype(np.float64)
    for _ in range(2):
        p = np.pad(checker, 1, mode="edge")
        checker = (4 * p[1:-1, 1:-1] + p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:]) / 8
    blurred = K.grey(checker)

    def laplacian_energy(a):
        a = a[..., 0].astype(np.float64)
        return float(((4 * a[1:-1, 1:-1] - a[:-2, 1:-1] - a[2:, 1:-1] - a[1:-1, :-2] - a[1:-1, 2:]) ** 2).sum())

    for size in (None, BIG):
        energy = [laplacian_energy(_process(e, blurred, size, s, False)) for s in (0.0, 0.25, 0.5, 1.0)]
        assert all(a < b for a, b in zip(energy, energy[1:])), (size, energy)
    # the noise limiter lowers the amplification of per-pixel noise on a flat field
    rng = np.random.default_rng(3)
    noisy = K.grey(0.5 + 0.05 * rng.standard_normal((52, 72)))

    def noise_rms(a):
        return float(np.sqrt(np.mean((a[..., 0].astype(np.float64) - 0.5) ** 2)))

    plain, limited, before = noise_rms(_process(e, noisy, None, 1.0, False)), noise_rms(_process(e, noisy, None, 1.0, True)), noise_rms(noisy)
    print(f"exact={exact}: per-pixel noise {before:.5f} -> {plain:.5f} sharpened, {limited:.5f} with the limiter")
    assert before < limited < plain
    e.close()


# ---------------------------------------------------------------- 2b. both steps in one launch (st_debug_set_upscale_fused)
@pytest.mark.parametrize("exact", [True, False])
def test_the_fused_launch_matches_the_restatement_and_the_two_launches_over_the_matrix(exact):
    e = Engine(device=0, exact=exact)
    ran = 0
    for case in K.cases():
        name, size, oname, osize, sharp, den = case
        if osize == size or sharp == 0.0:
            continue   # one step alone is never fused
        img = K.source(name, size)
        ref, _want64, _skip = _case_ref(case)
        e.set_upscale_fused(0)
        two = [_process(e, img, osize, sharp, den, fmt) for fmt in range(4)]
        for tile in (1, 2, 3):   # 64 x 8, 32 x 32, 64 x 16 output pixels per workgroup: the matrix's widths 63 .. 65 and 129 and its heights cross all three
            e.set_upscale_fused(tile)
            what = f"{name} {size} -> {oname} {osize} sharpness {sharp} limiter {den} exact={exact} tile {tile}"
            for fmt in range(4):
                got = _process(e, img, osize, sharp, den, fmt)
                assert np.array_equal(got.view(np.uint8), two[fmt].view(np.uint8)), (what, fmt)   # fused equals two launches, every byte of every format
            assert_bits_equal(_process(e, img, osize, sharp, den, 0), ref, what)
        ran += 1
    assert ran >= 40
    e.close()


def test_frames_through_the_fused_launch_equal_frames_through_the_two():
    outs = {}
    for tile in (0, 1, 2, 3):
        e = _engine(False, "dungeon")
        e.profile_enable(1)
        e.set_upscale_fused(tile)
        cam = e.create_camera(_camera("dungeon"))
        e.set_display(cam, tonemap=Tonemap.ACES_FITTED, exposure_ev=-1.0)
        e.set_post(cam, fxaa=True)
        e.set_upscale(cam, output_size=(145, 103), sharpness=0.5, denoise=True)
        outs[tile] = [_frame(e, cam, Out(2, (145, 103), fill=0x5a)) for _ in range(3)]
        names = {p["name"]: p["launches"] for p in e.profile_read()}
        assert (names.get("upscale+sharpen"), names.get("upscale"), names.get("sharpen")) == ((None, 3, 3) if tile == 0 else (3, None, None)), (tile, names)
        e.set_upscale(cam, sharpness=0.5)   # one step alone: the knob does not matter
        _frame(e, cam, Out(2))
        assert {p["name"]: p["launches"] for p in e.profile_read()}.get("sharpen") == 1
        e.close()
    for tile in (1, 2, 3):
        for k in range(3):
            assert np.array_equal(outs[tile][k], outs[0][k]), (tile, k)


def test_upscale_process_on_two_streams_shares_the_intermediate_plane_in_order():
    e = Engine(device=0)
    a, b = K.source("slanted", (72, 52)), K.source("noise", (37, 23))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    da, db = upscale_desc(output_size=(216, 156), sharpness=1.0, denoise=True), upscale_desc(output_size=(56, 35), sharpness=0.25)
    oa, ob = Out(0, (216, 156)), Out(0, (56, 35))
    torch.cuda.synchronize()
    for _ in range(4):   # alternate without a host sync: the engine orders the users of its plane between the two steps
        e.upscale_process(da, ta.data_ptr(), 72, 52, oa.ptr(), 0, sa.cuda_stream)
        e.upscale_process(db, tb.data_ptr(), 37, 23, ob.ptr(), 0, sb.cuda_stream)
    torch.cuda.synchronize()
    assert_bits_equal(oa.get(), U.process(a, (216, 156), 1.0, True), "stream a")
    assert_bits_equal(ob.get(), U.process(b, (56, 35), 0.25, False), "stream b")
    e.close()


# ---------------------------------------------------------------- 3. whole frames
FRAME_SIZE, FRAME_OUT = (64, 48), (128, 96)
UPSTREAM = dict(set_bloom=dict(intensity=0.2), set_color_grading=dict(contrast=1.1, saturation=1.05, slope=(1.05, 1.0, 0.95)), set_post=dict(fxaa=True))
FRAME_CASES = [
    # name, exact, scene, display
    ("cornell_manual", False, "cornell", dict(tonemap=Tonemap.ACES_FITTED, exposure_ev=0.5)),
    ("dungeon_manual", False, "dungeon", dict(tonemap=Tonemap.ACES_FITTED, exposure_ev=-1.0)),
    ("dungeon_auto", False, "dungeon", dict(tonemap=Tonemap.ACES_FITTED, auto_exposure=True, ev_min=-12.0, ev_max=8.0)),
    ("cornell_auto_exact", True, "cornell", dict(tonemap=Tonemap.ACES_FITTED, auto_exposure=True, ev_min=-12.0, ev_max=8.0)),
    ("dungeon_manual_exact", True, "dungeon", dict(tonemap=Tonemap.ACES_FITTED, exposure_ev=-1.0)),
]
FRAME_DESCS = [dict(output_size=FRAME_OUT, sharpness=0.5, denoise=True), dict(output_size=FRAME_OUT), dict(sharpness=1.0), dict(output_size=(96, 72), sharpness=0.25)]


@pytest.mark.parametrize("case", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_a_frame_with_the_stage_equals_the_restatement_of_the_frame_without(case):
    name, exact, scene, display = case
    a, b = _engine(exact, scene), _engine(exact, scene)
    desc = _camera(scene, size=FRAME_SIZE)
    ca, cb = a.create_camera(desc), b.create_camera(desc)
    for e, c in ((a, ca), (b, cb)):
        e.set_display(c, **display)
        for setter, kw in UPSTREAM.items():
            getattr(e, setter)(c, **kw)
    oa = Out(0, FRAME_SIZE)
    for k in range(4):
        d, fmt = FRAME_DESCS[k], (0, 2, 1, 0)[k]
        b.set_upscale(cb, **d)
        b.set_output_format(cb, OutputFormat(fmt))
        size = d.get("output_size", FRAME_SIZE)
        assert b.output_size(cb) == size
        ob = Out(fmt, size, fill=0x5a)
        plain = _frame(a, ca, oa)     # bloom, ACES, grading and FXAA, at the render size
        got = _frame(b, cb, ob)
        ref = U.process(plain, d.get("output_size"), d.get("sharpness", 0.0), d.get("denoise", False))
        _check(got, ref, fmt, f"{name} frame {k} fmt {fmt}")
        if k == 0:
            assert not bits_equal_mask(ref, U.process(plain, FRAME_OUT)).all(), "the sharpening step should move some pixel"
        if display.get("auto_exposure"):   # the metering saw the render-size composed frame, as without the stage
            assert np.array_equal(a.camera_histogram(ca), b.camera_histogram(cb)) and a.exposure(ca) == b.exposure(cb), k
        launches = b.last_launches()
        assert launches[-1] == PassBit.POST and sum(1 for x in launches if x & PassBit.POST) == 1, [hex(x) for x in launches]
    a.close(); b.close()


def test_a_one_pixel_frame():
    a, b = _engine(True), _engine(True)
    desc = _camera(size=(1, 1))
    ca, cb = a.create_camera(desc), b.create_camera(desc)
    b.set_upscale(cb, output_size=(3, 2), sharpness=1.0, denoise=True)
    plain, got = _frame(a, ca, Out(0, (1, 1))), _frame(b, cb, Out(0, (3, 2), fill=0x5a))
    assert_bits_equal(got, U.process(plain, (3, 2), 1.0, True), "1 x 1 -> 3 x 2")
    b.set_upscale(cb, output_size=(3, 2))
    up = _frame(b, cb, Out(0, (3, 2), fill=0x5a))
    assert (up[..., :3] == U.unit(plain)[0, 0]).all()   # one texel: the upscaler writes its clamped colour into every output pixel
    a.close(); b.close()


# ---------------------------------------------------------------- 4. off is off
@pytest.mark.parametrize("exact", [False, True])
def test_a_cleared_stage_and_a_desc_that_asks_nothing_render_like_none(exact):
    for fmt in (0, 2):
        a, b, c = _engine(exact), _engine(exact), _engine(exact)
        desc = _camera()
        cams = [e.create_camera(desc) for e in (a, b, c)]
        for e, cam in zip((a, b, c), cams):
            e.set_output_format(cam, OutputFormat(fmt))
            e.set_post(cam, fxaa=True)
        b.set_upscale(cams[1], output_size=BIG, sharpness=0.5)
        _frame(b, cams[1], Out(fmt, BIG))   # a frame through the stage, then off
        _frame(a, cams[0], Out(fmt)); _frame(c, cams[2], Out(fmt))
        b.set_upscale(cams[1], None)
        c.set_upscale(cams[2], upscale_desc(output_size=SIZE, sharpness=0.0, denoise=True))   # the render size and no sharpening
        assert b.output_size(cams[1]) == SIZE and c.output_size(cams[2]) == SIZE
        outs = [Out(fmt) for _ in range(3)]
        for k in range(8):
            if k == 4:
                c.set_upscale(cams[2], upscale_desc())   # 0, 0 and no sharpening
            x, y, z = (_frame(e, cam, o) for e, cam, o in zip((a, b, c), cams, outs))
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)) and np.array_equal(x.view(np.uint8), z.view(np.uint8)), (exact, fmt, k)
            assert b.last_launches() == a.last_launches() == c.last_launches()
        for e in (a, b, c):
            e.close()


def test_profile_slots_without_the_stage_are_the_parents():
    e = _engine(False)
    e.profile_enable(1)
    cam = e.create_camera(_camera())
    e.set_post(cam, fxaa=True, output_size=BIG, filter=ResampleFilter.CATMULL_ROM)
    _frame(e, cam, Out(0, BIG))
    names = {p["name"]: p["launches"] for p in e.profile_read()}
    assert names.get("post_fxaa") == 1 and names.get("post_resample") == 1 and not names.get("upscale") and not names.get("sharpen"), names
    e.close()


# ---------------------------------------------------------------- 5. independence
NODE = Node("set_upscale", "upscale", "upscaling", "the sharpened frame differs", ("sharpen",), dict(sharpness=1.0, denoise=True))


def test_aovs_picks_planes_and_exposure_do_not_depend_on_the_stage():
    nothing_else_depends_on_the_setting(NODE)   # (the helper's buffers are render size: the sharpening step alone)
    a, b = _engine(True), _engine(True)         # ... and with the upscaler: planes and exposure
    desc = _camera()
    ca, cb = a.create_camera(desc), b.create_camera(desc)
    for e, c in ((a, ca), (b, cb)):
        e.set_display(c, tonemap=Tonemap.ACES_FITTED, auto_exposure=True, ev_min=-12.0, ev_max=8.0)
    b.set_upscale(cb, output_size=BIG, sharpness=0.5, denoise=True)
    oa, ob = Out(0), Out(0, BIG)
    from strolle_amd import Buffer
    for k in range(3):
        _frame(a, ca, oa); _frame(b, cb, ob)
        for buf in Buffer:
            assert a.buffer_stale(ca, buf) == b.buffer_stale(cb, buf), (k, buf)
            assert np.array_equal(_bits(a.read_buffer(ca, buf)), _bits(b.read_buffer(cb, buf))), (k, buf)
        assert a.exposure(ca) == b.exposure(cb) and np.array_equal(a.camera_histogram(ca), b.camera_histogram(cb)), k
    a.close(); b.close()


# ---------------------------------------------------------------- 6. the frames that skip the stage, and those that do not
def test_heatmap_frames_are_resized_by_nearest_and_not_sharpened():
    a, b = _engine(True), _engine(True)
    desc = _camera(mode=CameraMode.BVH_HEATMAP)
    ca, cb = a.create_camera(desc), b.create_camera(desc)
    plain = _frame(a, ca, Out(0))
    b.set_upscale(cb, sharpness=1.0)                            # sharpening alone on false colour: nothing to do, no launch
    assert_bits_equal(_frame(b, cb, Out(0)), plain, "heatmap with sharpening only")
    assert not any(l & PassBit.POST for l in b.last_launches())
    b.set_upscale(cb, output_size=BIG, sharpness=1.0, denoise=True)
    assert b.output_size(cb) == BIG
    got = _frame(b, cb, Out(0, BIG, fill=0x5a))
    assert_bits_equal(got, post_ref.resample(plain, BIG[0], BIG[1], post_ref.NEAREST), "heatmap brought to the output size by NEAREST")
    assert not bits_equal_mask(U.process(plain, BIG, 1.0, True), got).all(), "the stage would have changed the heatmap"
    a.close(); b.close()


@pytest.mark.parametrize("what", ["reference", "orthographic"])
def test_reference_and_orthographic_frames_go_through_the_stage(what):
    a, b = _engine(True), _engine(True)
    desc = scenes.cornell_camera(SIZE, CameraMode.REFERENCE, denoise=False, depth=1) if what == "reference" else _orthographic(SIZE)
    ca, cb = a.create_camera(desc), b.create_camera(desc)
    b.set_upscale(cb, output_size=BIG, sharpness=0.5, denoise=True)
    for k in range(2):
        plain, got = _frame(a, ca, Out(0)), _frame(b, cb, Out(0, BIG, fill=0x5a))
        ref = U.process(plain, BIG, 0.5, True)
        assert_bits_equal(got, ref, f"{what} frame {k}")
        assert not bits_equal_mask(ref, post_ref.resample(plain, BIG[0], BIG[1], post_ref.CATMULL_ROM)).all()
    a.close(); b.close()


# ---------------------------------------------------------------- 7. tiles
@pytest.mark.parametrize("world", [2, 4])
def test_gathered_tiles_through_upscale_process_equal_the_single_engine_frame(world):
    size, big = (272, 200), (408, 300)
    stream = _stream()
    desc = _camera("cornell", CameraMode.REFERENCE, False, 1, size)
    d = upscale_desc(output_size=big, sharpness=0.5, denoise=True)
    one = _engine(True)
    cam = one.create_camera(desc)
    one.set_display(cam, tonemap=Tonemap.ACES_FITTED, exposure_ev=1.0)
    one.set_upscale(cam, d)
    one.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
    single = Out(2, big)
    for _ in range(2):
        one.update_camera(cam, desc); one.tick(stream); one.render_camera(cam, single.ptr(), stream)
    torch.cuda.synchronize()
    ranks = []
    for r in range(world):
        e = _engine(True)
        c = e.create_camera(desc)
        e.set_display(c, tonemap=Tonemap.ACES_FITTED, exposure_ev=1.0)   # manual exposure works with tiles; the upscale stage does not
        e.dist_init_local(r, world, 7500 + world)
        e.dist_set_partition(c, apron=0)
        ranks.append((e, c, torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda:0")))
    full = torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda:0")
    for _ in range(2):
        for r in range(world - 1, -1, -1):   # in-process transport: rank 0 last
            e, c, out = ranks[r]
            e.update_camera(c, desc); e.tick(stream)
            e.render_camera(c, out.data_ptr(), stream)
            e.dist_gather(c, out.data_ptr(), full.data_ptr() if r == 0 else 0, stream)
    root, root_cam, _ = ranks[0]
    root.dist_wait(root_cam, host=True)
    torch.cuda.synchronize()
    tiled = Out(2, big)
    root.upscale_process(d, full.data_ptr(), size[0], size[1], tiled.ptr(), 2, stream)   # the recipe for tiled frames: rank 0, on the gathered frame
    torch.cuda.synchronize()
    assert np.array_equal(tiled.get(), single.get()), f"{world} gathered tiles through st_upscale_process vs one engine with the stage"
    e, c, _ = ranks[1]   # a window and the stage: refused in either order
    with pytest.raises(Exception):
        e.set_upscale(c, d)
    e.set_camera_rows(c, 0, size[1])
    e.set_upscale(c, d)
    with pytest.raises(Exception):
        e.dist_set_partition(c, apron=0)
    for e, *_ in ranks:
        e.dist_shutdown(); e.close()
    one.close()


# ---------------------------------------------------------------- 8. frames in flight
def _run(sync, streams=1, profiling=False, frames=8, schedule=None):
    """`frames` moving dungeon frames through ACES, FXAA and the stage into RGBA8 sRGB, a host sync after every frame or none, round robin
    over `streams` streams. `schedule`: frame -> the stage's keywords (None: off) set in front of that frame."""
    from output_chain import _dungeon4
    e = _engine(False, "dungeon")
    if profiling:
        e.profile_enable(1)
    cam = e.create_camera(_dungeon4(0))
    e.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
    e.set_display(cam, tonemap=Tonemap.ACES_FITTED, exposure_ev=0.5)
    e.set_post(cam, fxaa=True)
    e.set_upscale(cam, output_size=BIG, sharpness=0.5, denoise=True)
    ss = [torch.cuda.Stream() for _ in range(streams)]
    outs = [Out(2, (216, 156)) for _ in range(frames)]   # the largest size of any schedule; a frame writes the first w * h pixels of its own
    sizes = []
    torch.cuda.synchronize()
    for k in range(frames):
        s = ss[k % streams].cuda_stream
        if schedule and k in schedule:
            if schedule[k] is None:
                e.set_upscale(cam, None)
            else:
                e.set_upscale(cam, **schedule[k])
        sizes.append(e.output_size(cam))
        e.update_camera(cam, _dungeon4(k))
        e.tick(s)
        e.render_camera(cam, outs[k].ptr(), s)
        if sync:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    got = [o.t.cpu().numpy()[:w * h * 4].reshape(h, w, 4).copy() for o, (w, h) in zip(outs, sizes)]
    names = {p["name"]: p["launches"] for p in e.profile_read()} if profiling else None
    e.close()
    return got, names


def test_frames_in_flight_read_their_own_inputs():
    base, _ = _run(True)
    assert any(not np.array_equal(base[k], base[k + 1]) for k in range(7)) and base[0].shape == (BIG[1], BIG[0], 4)
    for kw in (dict(), dict(streams=2), dict(profiling=True)):
        for sync in ((False,) if not kw else (True, False)):
            other, names = _run(sync, **kw)
            for k, (x, y) in enumerate(zip(other, base)):
                assert np.array_equal(x, y), (kw, sync, k)
            if names is not None:
                assert names["upscale"] == 8 and names["sharpen"] == 8 and names["post_fxaa"] == 8 and not names.get("post_resample"), names


def test_the_output_size_changed_and_the_stage_switched_off_between_frames_in_flight():
    schedule = {1: dict(output_size=(216, 156), sharpness=0.5), 2: dict(output_size=(108, 78)), 3: None, 4: dict(sharpness=1.0, denoise=True),
                5: dict(output_size=BIG, sharpness=0.25, denoise=True), 6: None, 7: dict(output_size=(216, 156), sharpness=1.0)}
    base, _ = _run(True, schedule=schedule)
    assert [b.shape[:2] for b in base] == [(104, 144), (156, 216), (78, 108), (52, 72), (52, 72), (104, 144), (52, 72), (156, 216)]
    for streams in (1, 2):
        other, _ = _run(False, streams=streams, schedule=schedule)
        for k, (x, y) in enumerate(zip(other, base)):
            assert np.array_equal(x, y), (streams, k)


# ---------------------------------------------------------------- 9. lifecycle
def test_camera_updates_and_teardown_with_the_stage_on():
    a, b = _engine(False), _engine(False)
    desc = _camera()
    ca, cb = a.create_camera(desc), b.create_camera(desc)
    d = dict(output_size=BIG, sharpness=0.5, denoise=True)
    b.set_upscale(cb, **d)
    for e in (a, b):                                                            # the setting survives an arithmetic switch
        e.set_exact(True); e.set_exact(False)
    _check(_frame(b, cb, Out(0, BIG)), U.process(_frame(a, ca, Out(0)), BIG, 0.5, True), 0, "after an arithmetic switch")
    big = _camera(size=(96, 80))                                                # another render size: the output size is kept
    a.update_camera(ca, big); b.update_camera(cb, big)
    assert b.output_size(cb) == BIG
    _check(_frame(b, cb, Out(0, BIG)), U.process(_frame(a, ca, Out(0, (96, 80))), BIG, 0.5, True), 0, "after a resize")
    with pytest.raises(Exception):                                              # larger than the output: refused, and the camera renders as before
        b.update_camera(cb, _camera(size=(160, 104)))
    _check(_frame(b, cb, Out(0, BIG)), U.process(_frame(a, ca, Out(0, (96, 80))), BIG, 0.5, True), 0, "after a refused resize")
    # delete a camera with the stage on and a frame in flight; a new camera starts clean; destroy the engine with planes live
    stream = _stream()
    keep = Out(0, BIG)
    b.tick(stream); b.render_camera(cb, keep.ptr(), stream)
    b.delete_camera(cb)
    c2 = b.create_camera(desc)
    assert not b.upscale(c2)[1] and b.output_size(c2) == SIZE
    b.set_upscale(c2, **d)
    assert np.isfinite(_frame(b, c2, Out(0, BIG))).all()
    b.tick(stream); b.render_camera(c2, keep.ptr(), stream)
    src, dst = torch.zeros((52, 72, 4), device="cuda:0"), Out(0, BIG)
    b.upscale_process(upscale_desc(**d), src.data_ptr(), 72, 52, dst.ptr(), 0, stream)   # the engine's own plane, live too
    a.close(); b.close()
