"""GPU tests of the lens effects (include/strolle_hip.h "lens effects"; k_lens.hip, st_lens.cpp): st_lens_process on the synthetic input
matrix (lens_cases.py) against the numpy restatement (lens_ref.lens_f32) bit for bit in both builds, and within the recorded tolerance
of the float64 definition; properties that do not rest on the restatement; whole frames with the node on against the restatement fed the
same frame rendered without it; the whole output chain against the eight process calls; off is off; nothing else changes; the frames that
skip it and the frames that do not; auto-exposure; ST_LENS_GRAIN_ANIMATE; frames in flight; lifecycle; the launch list. Every test builds
its own engines and uses entry points the parent commit does not have.

Sizes: the workgroup is 32 x 8 pixels and a wave 32 x 2, so 72 x 52 (partial groups both ways), widths 63, 64, 65 and 129 astride their
edges, 5 x 5 and 1 x 1."""
import json
import os

import numpy as np
import pytest
import torch

import display_ref
import lens_cases as K
import lens_ref as R
import output_chain as C
from output_chain import Depth, Out, _bits, _check, _engine, _moving, _orthographic, _proj, _scene_camera, _xf
from parity import assert_bits_equal
from strolle_amd import (Buffer, CameraMode, Engine, OutputFormat, PassBit, ResampleFilter, Tonemap, bloom_desc, color_grading_desc, display_desc, dof_desc, fog_desc, lens_desc,
                         lens_plan, light_shafts_desc, motion_blur_desc, post_desc, scenes, upscale_desc)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = K.SIZE
F = np.float32
# every step (the shared bodies set the node by keywords)
LENS = dict(k1=-0.2, k2=0.03, fit=True, fringe=0.03, fringe_taps=4, vignette_intensity=0.6, vignette_falloff=1.5, grain_intensity=0.25, grain_size=2, grain_seed=12345)
NODE = C.Node("set_lens", "get_lens", "lens effects", "the frame through the lens differs", ("lens",), LENS, pipelined=dict(LENS, grain_animate=True))
EV = K.EV


def _ref(key, make):
    return C._ref(__name__, key, make)


def _process(e, d, img, fmt=0, display=None, stream=None, dst=None):
    h, w = img.shape[:2]
    tc = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    out = dst if dst is not None else Out(fmt, (w, h), fill=0x5a)
    e.lens_process(d, tc.data_ptr(), w, h, out.ptr(), fmt, display=display, stream=stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.get()


def _restate(d, img, op=None, ev=EV, frame=0, force_gather=False):
    """lens_f32 with the library's own plan (st_lens_plan; tests/test_lens_abi.py holds it to numpy)"""
    h, w = img.shape[:2]
    return R.lens_f32(img, d, R.plan_of(lens_plan(d, w, h)), op, display_ref.manual_scale(ev), frame=frame, force_gather=force_gather)


def _disp(op, ev=EV):
    return display_desc(tonemap=op, exposure_ev=ev) if op is not None else None


# ---------------------------------------------------------------- 1. bit for bit against the restatement
@pytest.mark.parametrize("exact", [True, False])
def test_process_matches_the_restatement_on_synthetic_inputs(exact):
    e = Engine(device=0, exact=exact)
    changed = 0
    for name, size, kind, kw, op in K.cases():
        d = K.build(kw)
        img = K.image(size, True, kind)
        want = _ref(name, lambda: _restate(d, img, op))
        got = _process(e, d, img, 0, _disp(op))
        _check(got, want, 0, f"{name} exact={exact}")
        changed += int((~(_bits(got) == _bits(img)).all(-1)).sum())
    assert changed > 50000, changed
    # the four output formats, without a display and with a manual ACES one, through both instantiations
    img = K.image((65, 17), True)
    for what, kw in (("gather", dict(K.ALL, fringe_taps=7, fit=True)), ("pointwise", dict(K.STEPS["vignette"], **K.STEPS["grain"]))):
        d = K.build(kw)
        for op in (None, Tonemap.ACES_FITTED):
            want = _ref(("fmt", what, op), lambda: _restate(d, img, op, -1.5))
            for fmt in range(4):
                _check(_process(e, d, img, fmt, _disp(op, -1.5)), want, fmt, f"exact={exact} {what} {op} fmt={fmt}")
    e.close()


@pytest.mark.parametrize("exact", [True, False])
def test_both_builds_stay_within_the_recorded_tolerance_of_the_definition(exact):
    """unspoiled inputs, every pixel and channel, in front of the display transform: rel <= 4 a + 4 b spread with the restatement's own
    constants a and b (profiles/lens.json), in the measure of tests/test_lens_abi.py restatement_vs_definition"""
    ta, tb = K.tolerance()
    e = Engine(device=0, exact=exact)
    worst = 0.0
    for name, size, kind, kw, _op in K.cases():
        d = K.build(kw)
        img = K.image(size, False, kind)
        want, spread = _ref(("f64", name), lambda: R.lens_f64(img, d, spread=True))
        got = _process(e, d, img, 0)
        assert np.isfinite(got).all(), name
        den = np.maximum(1.0, np.abs(want))
        over = np.abs(got[..., :3].astype(np.float64) - want) / den - (ta + tb * spread / den)
        worst = max(worst, float(over.max()))
        print(f"{name} exact={exact}: worst rel {float((np.abs(got[..., :3].astype(np.float64) - want) / den).max()):.3e}, over the bound by {float(over.max()):.3e}")
        assert over.max() <= 0, (name, exact, float(over.max()))
    e.close()


# ---------------------------------------------------------------- 2. properties that do not rest on the restatement
@pytest.mark.parametrize("exact", [True, False])
def test_properties_of_the_lens(exact):
    e = Engine(device=0, exact=exact)
    other = Engine(device=0, exact=not exact)
    aces = _disp(Tonemap.ACES_FITTED)
    everything = K.build(dict(K.ALL, fringe_taps=16, fit=True))
    for (w, h) in K.SIZES:
        img = K.image((w, h), True)
        clean = K.image((w, h), False)
        # a neutral descriptor is a copy through the display and the format: without a display the pixel's own four words, alpha, NaN and all
        for disp, op in ((None, None), (aces, Tonemap.ACES_FITTED)):
            through = img if op is None else display_ref.transform(img[..., :3], int(op), display_ref.manual_scale(EV))
            for fmt in range(4):
                got = _process(e, lens_desc(fringe_taps=5, grain_size=3, vignette_falloff=2.0), img, fmt, disp)
                if op is None and fmt == 0:
                    assert np.array_equal(_bits(got), _bits(img)), (w, h)
                else:
                    _check(got, through, fmt, f"{w}x{h} neutral fmt={fmt}")
        # a constant image under distortion + fringe is that constant: three single-channel taps of weight 1 exactly, more taps within the
        # weights' rounding (n half-ulps in their sum, one per product and per sum)
        const = np.broadcast_to(np.array([0.75, 3.0, 1000.0, 0.2], np.float32), (h, w, 4)).copy()
        for n in (3, 16):
            got = _process(e, lens_desc(k1=0.15, k2=0.05, scale=0.9, fringe=0.1, fringe_taps=n), const, 0)
            err = np.abs(got[..., :3].astype(np.float64) / const[..., :3] - 1.0).max()
            assert (err == 0 if n == 3 else err <= 2 * n * 2.0 ** -24) and (got[..., 3] == 1).all(), (w, h, n, err)
        # no NaN from finite input, with everything on
        for op in (Tonemap.ACES_FITTED, Tonemap.NONE, None):
            assert np.isfinite(_process(e, everything, clean, 0, _disp(op))).all(), (w, h, op)
        # the pointwise and the gather instantiation agree on a descriptor without taps (the debug seam forces the gather)
        for kw in (K.STEPS["vignette"], K.STEPS["grain"], dict(K.STEPS["vignette"], vignette_round=True, **K.STEPS["grain"])):
            d = lens_desc(**kw)
            pointwise = _process(e, d, img, 0, aces)
            e.set_lens_gather(True)
            gathered = _process(e, d, img, 0, aces)
            e.set_lens_gather(False)
            assert_bits_equal(gathered, pointwise, f"{w}x{h} {sorted(kw)}: the gather against the pointwise instantiation")
        # the two builds give the same bits
        assert_bits_equal(_process(other, everything, img, 0, aces), _process(e, everything, img, 0, aces), f"{w}x{h}: fast against exact")
    # the vignette darkens towards the corner and leaves the centre. Barrel distortion with ST_LENS_FIT of an image that is 1 everywhere but
    # 1000 on its outermost ring: the vertical axis binds (20.5 / (20 f(0.296)) = 1.10 against 30.5 / (30 f(0.666)) = 1.20), so the top
    # edge's midpoint reads the frame's very edge, the ring, and the side edge's midpoint reads 2.5 pixels inside it
    flat = np.ones((41, 61, 4), np.float32)
    v = _process(e, lens_desc(vignette_intensity=1.0, vignette_falloff=2.0), flat, 0)[..., 0]
    assert v[20, 30] == 1.0 and v[0, 0] < 0.2 and v[0, 0] == v[40, 60] == v[0, 60] == v[40, 0] and (np.diff(v[20, 30:]) < 0).all()
    ring = flat.copy(); ring[0, :, :3] = ring[-1, :, :3] = 1000.0; ring[:, 0, :3] = ring[:, -1, :3] = 1000.0
    g = _process(e, lens_desc(k1=-0.25, k2=0.03, fit=True), ring, 0)[..., 0]
    assert g.max() <= 1000.0 and g[20, 30] == 1.0 and g[0, 30] == 1000.0 and g[40, 30] == 1000.0 and g[20, 0] == 1.0 and g[20, 60] == 1.0
    e.close(); other.close()


# ---------------------------------------------------------------- 3. whole frames
FRAME_CASES = [("cornell_fast", False, "cornell"), ("cornell_exact", True, "cornell"), ("dungeon_fast", False, "dungeon"), ("dungeon_exact", True, "dungeon")]
GRADE = dict(temperature=0.2, contrast=1.2, saturation=0.8, slope=(1.1, 0.9, 1.2), dither=True)


@pytest.mark.parametrize("case", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_a_frame_through_the_lens_equals_the_restatement_of_the_frame_without(case):
    """a: no display, no lens, RGBA32F; b: ACES and every step of the lens. Then both with bloom in front (a blooms without a display),
    then b with colour grading, FXAA and the upscaler behind it: the lens writes the grade's plane, and the frame is
    st_color_grading_process, st_post_process and st_upscale_process over st_lens_process of the plain frame."""
    name, exact, scene = case
    a, b = _engine(exact, scene), _engine(exact, scene)
    cam = _scene_camera(scene, SIZE)
    ca, cb = a.create_camera(cam), b.create_camera(cam)
    disp = _disp(Tonemap.ACES_FITTED)
    d = lens_desc(**LENS)
    b.set_lens(cb, d)
    b.set_display(cb, disp)
    assert b.get_lens(cb)[1]
    oa, ob = Out(0), Out(0, fill=0x5a)
    stream = torch.cuda.current_stream().cuda_stream
    bd = bloom_desc(intensity=0.3, threshold=0.4, threshold_softness=0.5)
    gd, post, up = color_grading_desc(**GRADE), post_desc(fxaa=True), upscale_desc(output_size=(108, 78), sharpness=0.5)
    for k in range(5):
        if k == 2:
            a.set_bloom(ca, bd); b.set_bloom(cb, bd)
        if k == 4:
            b.set_color_grading(cb, gd); b.set_post(cb, post); b.set_upscale(cb, up); b.set_output_format(cb, OutputFormat.RGBA8_UNORM_SRGB)
            ob = Out(2, (108, 78), fill=0x5a)
        for e, c, o in ((a, ca, oa), (b, cb, ob)):
            e.tick(stream); e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        plain, got = oa.get(), ob.get()
        if k < 4:
            ref = _restate(d, plain, Tonemap.ACES_FITTED)
            assert not np.array_equal(_bits(ref), _bits(plain))
            _check(got, ref, 0, f"{name} frame {k}")
            launches = b.last_launches()
            assert launches[-1] == PassBit.POST and sum(1 for x in launches if x & PassBit.POST) == 1, [hex(x) for x in launches]
        else:
            lensed, graded, smooth, want = Out(0), Out(0), Out(0), Out(2, (108, 78), fill=0xa5)
            _process(b, d, plain, 0, None, dst=lensed)
            assert_bits_equal(lensed.get(), _restate(d, plain, None), f"{name}: the process call")
            b.color_grading_process(gd, lensed.ptr(), SIZE[0], SIZE[1], graded.ptr(), 0, display=disp, stream=stream)
            b.post_process(post, graded.ptr(), SIZE[0], SIZE[1], smooth.ptr(), 0, stream=stream)
            b.upscale_process(up, smooth.ptr(), SIZE[0], SIZE[1], want.ptr(), 2, stream)
            torch.cuda.synchronize()
            assert np.array_equal(got, want.get()), (name, np.abs(got.astype(int) - want.get().astype(int)).max())
    a.close(); b.close()


@pytest.mark.parametrize("exact,scene", [(False, "dungeon"), (True, "cornell")])
def test_the_whole_chain_equals_the_eight_process_calls(exact, scene):
    """fog, light shafts, depth of field, motion blur, bloom, the lens, the grade around ACES and FXAA (with a resample) in one frame
    against st_fog_process, st_light_shafts_process, st_dof_process, st_motion_blur_process, st_bloom_process, st_lens_process (the three
    of them without a display: the grade applies it), st_color_grading_process and st_post_process over the plain frame's colour, the
    velocity map and the G-buffer depth"""
    a, b = _engine(exact, scene), _engine(exact, scene)
    ca, cb = a.create_camera(_moving(scene, 0)), b.create_camera(_moving(scene, 0))
    fd = fog_desc(color=(0.5, 0.6, 0.7, 0.9), density=0.12, height_falloff=0.25, height_reference=0.5)
    sd = light_shafts_desc(steps=8, divisor=2, **C.MEDIUM, **C.SUN)
    dd = dof_desc(samples=32, autofocus=(0.5, 0.5), sensor_height=0.5, focal_distance=3.0)
    md, bd = motion_blur_desc(shutter=1.0, samples=8), bloom_desc(intensity=0.3, threshold=0.4, threshold_softness=0.5)
    ld, gd = lens_desc(**LENS), color_grading_desc(**GRADE)
    disp = _disp(Tonemap.ACES_FITTED)
    post = post_desc(fxaa=True, output_size=(108, 78), filter=ResampleFilter.CATMULL_ROM)
    b.set_fog(cb, fd); b.set_light_shafts(cb, sd); b.set_dof(cb, dd); b.set_motion_blur(cb, md); b.set_bloom(cb, bd); b.set_lens(cb, ld); b.set_color_grading(cb, gd)
    b.set_display(cb, disp); b.set_post(cb, post)
    b.set_output_format(cb, OutputFormat.RGBA8_UNORM_SRGB)
    oa, ob, depth = Out(0), Out(2, (108, 78), fill=0x5a), Depth()
    stream = torch.cuda.current_stream().cuda_stream
    w, h = SIZE
    for k in range(3):
        for e, c, o in ((a, ca, oa), (b, cb, ob)):
            e.update_camera(c, _moving(scene, k)); e.tick(stream); e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        z = depth.read(b, cb, SIZE)
        v = b.read_buffer(cb, Buffer.VELOCITY_MAP).reshape(h, w, 4)[..., :2].copy()
        if k == 0:
            continue   # (the first frame has no previous camera)
        tz, tv = torch.from_numpy(z).cuda(), torch.from_numpy(v).cuda()
        s0, s1, s2, s3, s4, s5, s6, want = Out(0), Out(0), Out(0), Out(0), Out(0), Out(0), Out(0), Out(2, (108, 78), fill=0xa5)
        cam = _moving(scene, k)
        b.fog_process(fd, _xf(cam), _proj(cam), oa.ptr(), tz.data_ptr(), w, h, s0.ptr(), 0, stream=stream)
        b.light_shafts_process(sd, _xf(cam), _proj(cam), s0.ptr(), tz.data_ptr(), w, h, s1.ptr(), 0, stream=stream)
        b.dof_process(dd, _proj(cam), s1.ptr(), tz.data_ptr(), w, h, s2.ptr(), 0, stream=stream)
        b.motion_blur_process(md, s2.ptr(), tv.data_ptr(), tz.data_ptr(), w, h, s3.ptr(), 0, stream=stream)
        b.bloom_process(bd, s3.ptr(), w, h, s4.ptr(), 0, stream=stream)
        b.lens_process(ld, s4.ptr(), w, h, s5.ptr(), 0, stream=stream)
        b.color_grading_process(gd, s5.ptr(), w, h, s6.ptr(), 0, display=disp, stream=stream)
        b.post_process(post, s6.ptr(), w, h, want.ptr(), 2, stream=stream)
        torch.cuda.synchronize()
        assert not np.array_equal(_bits(s5.get()), _bits(s4.get()))
        assert np.array_equal(ob.get(), want.get()), (exact, scene, k, np.abs(ob.get().astype(int) - want.get().astype(int)).max())
        launches = b.last_launches()
        assert launches[-1] == PassBit.POST and sum(1 for x in launches if x & PassBit.POST) == 2, [hex(x) for x in launches]   # the two pack launches, then the rest
    a.close(); b.close()


# ---------------------------------------------------------------- 4. off is off; nothing else changes
@pytest.mark.parametrize("exact", [False, True])
def test_a_cleared_setting_renders_like_a_camera_that_never_had_one(exact):
    C.cleared_setting_renders_like_none(NODE, exact, frames=8)


def test_aovs_picks_planes_and_the_exposure_do_not_depend_on_the_setting():
    C.nothing_else_depends_on_the_setting(NODE)


@pytest.mark.parametrize("exact", [False, True])
def test_a_neutral_descriptor_renders_what_off_renders(exact):
    """on, but every step neutral: the bytes of the camera without the setting, in RGBA32F without a display and in RGBA8 sRGB through
    ACES, alone and with bloom in front; the node's one launch is a copy through the display and the format"""
    a, b = _engine(exact), _engine(exact)
    ca, cb = a.create_camera(C._cornell(0)), b.create_camera(C._cornell(0))
    b.set_lens(cb, lens_desc(fringe_taps=9, grain_size=4, grain_seed=3))
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(6):
        if k == 2:
            for e, c in ((a, ca), (b, cb)):
                e.set_display(c, tonemap=Tonemap.ACES_FITTED, exposure_ev=0.5); e.set_output_format(c, OutputFormat.RGBA8_UNORM_SRGB)
        if k == 4:
            for e, c in ((a, ca), (b, cb)):
                e.set_bloom(c, intensity=0.3, threshold=0.4, threshold_softness=0.5)
        oa, ob = (Out(0), Out(0, fill=0x5a)) if k < 2 else (Out(2), Out(2, fill=0x5a))
        for e, c, o in ((a, ca, oa), (b, cb, ob)):
            e.update_camera(c, C._cornell(k)); e.tick(stream); e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(oa.get()) if k < 2 else oa.get(), _bits(ob.get()) if k < 2 else ob.get()), (exact, k)
        if k < 4:
            assert b.last_launches() == a.last_launches() + [int(PassBit.POST)]
    a.close(); b.close()


# ---------------------------------------------------------------- 5. the frames that skip it, and the frames that do not
def test_heatmap_frames_skip_the_lens():
    C.frames_that_skip(NODE, "heatmap", (64, 48))


@pytest.mark.parametrize("what", ["reference", "orthographic"])
def test_reference_and_orthographic_frames_pass_through_the_lens(what):
    """nothing in the node depends on a G-buffer or on the projection"""
    size = (64, 48)
    a, b = _engine(True), _engine(True)
    cam = scenes.cornell_camera(size, CameraMode.REFERENCE, denoise=False, depth=1) if what == "reference" else _orthographic(size)
    ca, cb = a.create_camera(cam), b.create_camera(cam)
    d = lens_desc(**LENS)
    b.set_lens(cb, d)
    oa, ob = Out(0, size), Out(0, size)
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(2):
        for e, c, o in ((a, ca, oa), (b, cb, ob)):
            e.tick(stream); e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        plain = oa.get()
        assert _bits(plain).any()
        _check(ob.get(), _restate(d, plain, None), 0, f"{what} frame {k}")
        assert not np.array_equal(_bits(ob.get()), _bits(plain))
        assert b.last_launches() == a.last_launches() + [int(PassBit.POST)]
    a.close(); b.close()


def test_auto_exposure_stores_with_the_scale_of_the_frame_before():
    """the meter reads the composed frame in the composing launch; the lens's display transform takes the scale the previous frame's
    finalize left, as every node's last store does"""
    a, b = _engine(False, "dungeon"), _engine(False, "dungeon")
    ca, cb = a.create_camera(C._dungeon(0)), b.create_camera(C._dungeon(0))
    b.set_display(cb, tonemap=Tonemap.ACES_FITTED, auto_exposure=True, ev_min=-12.0, ev_max=8.0)
    d = lens_desc(**LENS)
    b.set_lens(cb, d)
    oa, ob = Out(0), Out(0)
    stream = torch.cuda.current_stream().cuda_stream
    scales = []
    for k in range(4):
        scale = b.exposure(cb)[0] if k else None     # what frame k - 1 left
        for e, c, o in ((a, ca, oa), (b, cb, ob)):
            e.update_camera(c, C._dungeon(k)); e.tick(stream); e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        if k:
            ref = R.lens_f32(oa.get(), d, R.plan_of(lens_plan(d, *SIZE)), Tonemap.ACES_FITTED, F(scale))
            _check(ob.get(), ref, 0, f"auto-exposure frame {k}")
            scales.append(float(scale))
    assert len(set(scales)) > 1, scales   # the exposure adapts while the camera moves
    a.close(); b.close()


# ---------------------------------------------------------------- 6. ST_LENS_GRAIN_ANIMATE
def test_animated_grain_follows_the_frame_counter():
    """a: plain frames; b: grain with ST_LENS_GRAIN_ANIMATE; c: the same grain without the flag. Frame k of b is the restatement of a's
    frame at seed + the camera's frame counter — so two consecutive frames differ by their grain pattern, beyond what the renderer's own
    frames differ — and no other counter gives it; c's pattern is the same every frame."""
    kw = dict(grain_intensity=0.5, grain_size=2, grain_seed=0xfffffffe)     # (the sum wraps)
    da, dc = lens_desc(grain_animate=True, **kw), lens_desc(**kw)
    engines = [_engine(False) for _ in range(3)]
    cams = [e.create_camera(C._cornell(0)) for e in engines]
    engines[1].set_lens(cams[1], da); engines[2].set_lens(cams[2], dc)
    outs = [Out(0), Out(0), Out(0)]
    stream = torch.cuda.current_stream().cuda_stream
    etas = []
    for k in range(3):
        for e, c, o in zip(engines, cams, outs):
            e.tick(stream); e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        plain, animated, still = (o.get() for o in outs)
        frame = engines[1].world()[1] - 1                                   # the counter the tick gave the camera
        _check(animated, _restate(da, plain, None, frame=frame), 0, f"animated grain, frame {k}")
        assert not np.array_equal(_bits(animated), _bits(_restate(da, plain, None, frame=frame + 1)))
        _check(still, _restate(dc, plain, None, frame=frame), 0, f"still grain, frame {k}")
        assert_bits_equal(_restate(dc, plain, None, frame=0), _restate(dc, plain, None, frame=frame), "without the flag the counter does not matter")
        etas.append(R.grain_eta(*np.meshgrid(np.arange(SIZE[0]), np.arange(SIZE[1])), 2, R.seed_of(da, frame)))
    assert not np.array_equal(etas[0], etas[1]) and not np.array_equal(etas[1], etas[2])
    for e in engines:
        e.close()


# ---------------------------------------------------------------- 7. pipelining
def test_frames_in_flight_read_their_own_inputs():
    C.frames_in_flight_read_their_own_inputs(NODE)


def test_the_setting_changed_and_switched_off_between_frames_in_flight():
    """eight dungeon frames without a host sync on two streams: the descriptor changes in front of frames 2 and 4 (pointwise, then a
    16-tap gather), goes off in front of frame 5 and comes back in front of frame 6 — the frames of the run that syncs after every frame"""
    schedule = {0: LENS, 2: dict(vignette_intensity=0.8, vignette_falloff=2.0), 4: dict(k1=0.15, k2=0.05, scale=0.8, fringe=0.1, fringe_taps=16), 5: None, 6: dict(LENS, grain_animate=True)}

    def run(sync, streams):
        e = _engine(False, "dungeon")
        cam = e.create_camera(C._dungeon4(0))
        e.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
        e.set_display(cam, tonemap=Tonemap.ACES_FITTED, exposure_ev=0.5)
        ss = [torch.cuda.Stream() for _ in range(streams)]
        outs = [Out(2) for _ in range(8)]
        torch.cuda.synchronize()
        for k in range(8):
            s = ss[k % streams].cuda_stream
            if k in schedule:
                NODE.set(e, cam, schedule[k])
            e.update_camera(cam, C._dungeon4(k)); e.tick(s); e.render_camera(cam, outs[k].ptr(), s)
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        got = [o.get() for o in outs]
        e.close()
        return got

    base = run(True, 1)
    for k, (x, y) in enumerate(zip(run(False, 2), base)):
        assert np.array_equal(x, y), k


# ---------------------------------------------------------------- 8. lifecycle
def test_resizes_toggles_arithmetic_switches_tiny_frames_and_teardown():
    a, b = _engine(False), _engine(False)
    stream = torch.cuda.current_stream().cuda_stream
    ca, cb = a.create_camera(scenes.cornell_camera(SIZE)), b.create_camera(scenes.cornell_camera(SIZE))
    d = lens_desc(**LENS)
    b.set_lens(cb, d)
    step = 0
    for size in (SIZE, (96, 80), (8, 8), (1, 1), SIZE):   # larger, tiny, back: the setting and the results stay (the plan follows the size)
        if size == SIZE and step:
            for e in (a, b):
                e.set_exact(True); e.set_exact(False)   # ... and across an arithmetic switch
        cam = scenes.cornell_camera(size)
        for e, c in ((a, ca), (b, cb)):
            e.update_camera(c, cam)
        for rep_ in range(2):
            if rep_ == 1 and size == (96, 80):
                b.set_lens(cb, None); b.set_lens(cb, d)   # a toggle between two frames
            oa, ob = Out(0, size), Out(0, size)
            a.tick(stream); b.tick(stream)
            a.render_camera(ca, oa.ptr(), stream); b.render_camera(cb, ob.ptr(), stream)
            torch.cuda.synchronize()
            assert b.get_lens(cb)[1] and b.get_lens(cb)[0].k1 == F(LENS["k1"])
            _check(ob.get(), _restate(d, oa.get(), None), 0, f"size {size} step {step}")
            step += 1
    # delete a camera with the setting on and a frame in flight; a new camera starts clean; destroy the engine with such a frame in flight
    C.teardown_with_the_setting_on(NODE, b, cb)
    a.close(); b.close()


# ---------------------------------------------------------------- 9. the launch list
def test_a_frame_through_the_lens_adds_one_post_launch_named_lens():
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "render_launches.json")))["default"]
    stream = torch.cuda.current_stream().cuda_stream
    for lensed in (False, True):
        for profiled in (False, True):
            e = Engine(device=0)
            scenes.build_cornell(e)
            e.set_seed(7)
            cam = e.create_camera(scenes.cornell_camera((64, 48)))
            if lensed:
                e.set_lens(cam, **LENS)
            if profiled:
                e.profile_enable(1 | 8)
            out = torch.zeros((48, 64, 4), dtype=torch.float32, device="cuda:0")
            for frame in range(1, 7):
                e.tick(stream)
                e.render_camera(cam, out.data_ptr(), stream)
                torch.cuda.synchronize()
                if profiled:
                    got = {p["name"]: p["launches"] for p in e.profile_read(reset=True) if p["launches"]}
                    want = dict(golden["profiled"][frame - 1][1], **({"lens": 1} if lensed else {}))
                else:
                    got, want = e.last_launches(), golden["full"][frame - 1][1] + ([int(PassBit.POST)] if lensed else [])
                assert got == want, (lensed, profiled, frame, got, want)
            e.close()
