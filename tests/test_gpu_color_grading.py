"""GPU tests of colour grading (include/strolle_hip.h "colour grading"; k_grade.hip, st_grade.cpp): st_color_grading_process on the synthetic
input matrix (grade_cases.py) against the numpy restatement (grade_ref.grade_f32) bit for bit in both builds, and within the recorded
tolerance of the float64 definition; properties that do not rest on the restatement; whole frames with grading on against the restatement
fed the same frame rendered without it; the whole output chain against the seven process calls; off is off; nothing else changes; the
frames that skip it and the frames that do not; auto-exposure; tiles; a table replaced and removed with frames in flight; lifecycle; the
launch list. Every test builds its own engines and uses entry points the parent commit does not have.

Sizes: the workgroup is 32 x 8 pixels, so 72 x 52 (partial groups both ways), 33 x 9, 5 x 5 and 1 x 1; LUT sides 2, 3, 17 and 33."""
import json
import os

import numpy as np
import pytest
import torch

import display_ref
import grade_cases as K
import grade_ref as R
import output_chain as C
from output_chain import Depth, Out, _bits, _check, _engine, _moving, _orthographic, _proj, _scene_camera, _xf
from parity import assert_bits_equal
from strolle_amd import (Buffer, CameraMode, Engine, LutDomain, OutputFormat, PassBit, ResampleFilter, Tonemap, bloom_desc, color_grading_desc, color_grading_plan,
                         display_desc, dof_desc, fog_desc, light_shafts_desc, motion_blur_desc, post_desc, scenes)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = K.SIZE
F = np.float32
# every step but the table (the shared bodies set the node by keywords); LOOK adds a table by handle
GRADE = dict(temperature=0.35, tint=-0.2, contrast=1.3, saturation=0.6, slope=(1.1, 0.9, 1.2), offset=(0.02, -0.03, 0.0), power=(1.2, 1.0, 0.8), cdl_saturation=1.25,
             dither=True)
LUT_ID = 41
NODE = C.Node("set_color_grading", "get_color_grading", "colour grading", "the graded frame differs", ("color_grading",), GRADE)
EV = K.EV


def _ref(key, make):
    return C._ref(__name__, key, make)


def _lut_device(table):
    """a table as the device holds it: one float4 per texel, red fastest"""
    t = np.concatenate([table.reshape(-1, 3), np.ones((table.shape[0] ** 3, 1), np.float32)], -1)
    return torch.from_numpy(np.ascontiguousarray(t)).cuda()


def _process(e, d, img, fmt=0, display=None, table=None, stream=None, dst=None):
    h, w = img.shape[:2]
    tc = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    tl = _lut_device(table) if table is not None else None
    out = dst if dst is not None else Out(fmt, (w, h), fill=0x5a)
    e.color_grading_process(d, tc.data_ptr(), w, h, out.ptr(), fmt, display=display, lut_ptr=tl.data_ptr() if tl is not None else 0,
                            lut_size=table.shape[0] if table is not None else 0, stream=stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.get()


def _restate(d, img, op=None, ev=EV, table=None, origin=(0, 0)):
    """grade_f32 with the library's own matrix (st_color_grading_plan)"""
    return R.grade_f32(img, d, op, display_ref.manual_scale(ev), lut=table, M=color_grading_plan(d)[1], origin=origin)


def _disp(op, ev=EV):
    return display_desc(tonemap=op, exposure_ev=ev) if op is not None else None


# ---------------------------------------------------------------- 1. bit for bit against the restatement
@pytest.mark.parametrize("exact", [True, False])
def test_process_matches_the_restatement_on_synthetic_inputs(exact):
    e = Engine(device=0, exact=exact)
    changed = 0
    for name, size, kw, op in K.cases():
        d, table = K.build(kw)
        img = K.image(size, spoil=True)
        want = _ref(name, lambda: _restate(d, img, op, table=table))
        got = _process(e, d, img, 0, _disp(op), table)
        _check(got, want, 0, f"{name} exact={exact}")
        changed += int((~(_bits(got) == _bits(img)).all(-1)).sum())
    assert changed > 50000, changed
    # the four output formats, without a display and with a manual ACES one
    d, table = K.build(K.ALL)
    img = K.image((33, 9), spoil=True)
    for op in (None, Tonemap.ACES_FITTED):
        want = _ref(("fmt", op), lambda: _restate(d, img, op, -1.5, table))
        for fmt in range(4):
            _check(_process(e, d, img, fmt, _disp(op, -1.5), table), want, fmt, f"exact={exact} {op} fmt={fmt}")
    e.close()


@pytest.mark.parametrize("exact", [True, False])
def test_both_builds_stay_within_the_recorded_tolerance_of_the_definition(exact):
    """unspoiled inputs, every pixel: the bound is 4 x the restatement's own worst deviation (profiles/grading.json), in the same measure"""
    bound = 4.0 * json.load(open(os.path.join(ROOT, "profiles", "grading.json")))["restatement_vs_definition"]["worst"]
    e = Engine(device=0, exact=exact)
    worst = 0.0
    for name, size, kw, op in K.cases():
        d, table = K.build(kw)
        img = K.image(size, spoil=False)
        want = _ref(("f64", name), lambda: R.grade_f64(img, d, op, display_ref.manual_scale(EV), lut=table))
        got = _process(e, d, img, 0, _disp(op), table)
        assert np.isfinite(got).all(), name
        err = np.abs(got[..., :3].astype(np.float64) - want).max(-1) / np.maximum(1.0, np.abs(want).max(-1))
        worst = max(worst, float(err.max()))
        assert err.max() <= bound, (name, exact, float(err.max()), bound)
    print(f"exact={exact}: worst deviation from the definition {worst:.3e}, bound {bound:.3e}")
    e.close()


# ---------------------------------------------------------------- 2. properties that do not rest on the restatement
def _srgb8(e, d, img, table=None, display=None):
    return _process(e, d, img, int(OutputFormat.RGBA8_UNORM_SRGB), display, table)


@pytest.mark.parametrize("exact", [True, False])
def test_properties_of_the_grade(exact):
    e = Engine(device=0, exact=exact)
    other = Engine(device=0, exact=not exact)
    aces = _disp(Tonemap.ACES_FITTED)
    for (w, h) in K.SIZES:
        img = K.image((w, h), spoil=True)
        clean = K.image((w, h), spoil=False)
        # a neutral descriptor is a copy through the display and the format: without a display the pixel's own four words, alpha, NaN and all
        for disp, op in ((None, None), (aces, Tonemap.ACES_FITTED)):
            through = img if op is None else display_ref.transform(img[..., :3], int(op), display_ref.manual_scale(EV))
            for fmt in range(4):
                got = _process(e, color_grading_desc(lut=5), img, fmt, disp)   # (the process call does not consult the handle)
                if op is None and fmt == 0:
                    assert np.array_equal(_bits(got), _bits(img)), (w, h)
                else:
                    _check(got, through, fmt, f"{w}x{h} neutral fmt={fmt}")
        # a constant table gives that constant, whatever the input, in both domains
        const = K.lut("constant", 3)
        for kw in (dict(), dict(lut_domain=LutDomain.LOG2, lut_ev_min=-8.0, lut_ev_max=8.0)):
            got = _process(e, color_grading_desc(lut=1, **kw), img, 0, aces, const)
            # (four weights that sum to 1 before rounding: four products and three sums below 1, half an ulp of 1 each at the most)
            assert np.abs(got.astype(np.float64) - np.array([0.25, 0.5, 0.75, 1.0])).max() <= 4 * 2.0 ** -24 and (got[..., 3] == 1).all(), (w, h, kw)
        # an identity table at side 2 equals no table within the tolerance
        bound = 4.0 * json.load(open(os.path.join(ROOT, "profiles", "grading.json")))["restatement_vs_definition"]["worst"]
        a = _process(e, color_grading_desc(lut=1), clean, 0, aces, K.lut("identity", 2))
        b = _process(e, color_grading_desc(), clean, 0, aces)
        assert np.abs(a.astype(np.float64) - b).max() <= bound, (w, h)
        # no NaN from finite input, with everything on
        d, table = K.build(K.ALL)
        for op in (Tonemap.ACES_FITTED, Tonemap.NONE, None):
            assert np.isfinite(_process(e, d, clean, 0, _disp(op), table)).all(), (w, h, op)
        # dither moves an encoded channel by one 8-bit step at the most
        plain8 = _srgb8(e, color_grading_desc(), clean, display=aces)
        dith8 = _srgb8(e, color_grading_desc(dither=True), clean, display=aces)
        assert np.abs(plain8.astype(int) - dith8.astype(int)).max() <= 1, (w, h)
        # the two builds give the same bits
        assert_bits_equal(_process(other, d, img, 0, aces, table), _process(e, d, img, 0, aces, table), f"{w}x{h}: fast against exact")
    # a 64-pixel dark ramp over 8 rows in RGBA8: its few levels meet in hard edges; dithered, rows differ from each other around them
    ramp = np.zeros((8, 64, 4), np.float32)
    ramp[..., :3] = np.linspace(0.0008, 0.0016, 64, dtype=np.float32)[None, :, None]
    ramp[..., 3] = 1.0
    plain8 = _srgb8(e, color_grading_desc(), ramp)[..., 0].astype(int)
    dith8 = _srgb8(e, color_grading_desc(dither=True), ramp)[..., 0].astype(int)
    assert np.abs(plain8 - dith8).max() <= 1
    assert (plain8 == plain8[0]).all() and len(np.unique(plain8)) <= 4                      # bands: every row the same few steps
    transitions = lambda a: int((np.diff(a, axis=1) != 0).sum())   # noqa: E731
    assert transitions(dith8) > transitions(plain8) and not (dith8 == dith8[0]).all(), (transitions(plain8), transitions(dith8))
    assert abs(dith8.mean() - plain8.mean()) < 0.5                                           # ... around the same mean
    e.close(); other.close()


# ---------------------------------------------------------------- 3. whole frames
def _look(e, cam, table=None, **more):
    """everything on, with a table by handle; the descriptor"""
    table = K.lut("random", 17) if table is None else table
    e.insert_lut(LUT_ID, table)
    d = color_grading_desc(lut=LUT_ID, **dict(GRADE, **more))
    e.set_color_grading(cam, d)
    return d, table


FRAME_CASES = [("cornell_fast", False, "cornell"), ("cornell_exact", True, "cornell"), ("dungeon_fast", False, "dungeon"), ("dungeon_exact", True, "dungeon")]


@pytest.mark.parametrize("case", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_a_graded_frame_equals_the_restatement_of_the_frame_without(case):
    """a: no display, no grading, RGBA32F; b: ACES and the whole grade. Then both with bloom in front (a blooms without a display), then b
    with FXAA and a resample behind it: the grade writes the post plane, and the frame is st_post_process over the graded plane."""
    name, exact, scene = case
    a, b = _engine(exact, scene), _engine(exact, scene)
    cam = _scene_camera(scene, SIZE)
    ca, cb = a.create_camera(cam), b.create_camera(cam)
    disp = _disp(Tonemap.ACES_FITTED)
    d, table = _look(b, cb)
    b.set_display(cb, disp)
    assert b.get_color_grading(cb)[1]
    oa, ob = Out(0), Out(0, fill=0x5a)
    stream = torch.cuda.current_stream().cuda_stream
    bd = bloom_desc(intensity=0.3, threshold=0.4, threshold_softness=0.5)
    post = post_desc(fxaa=True, output_size=(108, 78), filter=ResampleFilter.CATMULL_ROM)
    for k in range(5):
        if k == 2:
            a.set_bloom(ca, bd); b.set_bloom(cb, bd)
        if k == 4:
            b.set_post(cb, post); b.set_output_format(cb, OutputFormat.RGBA8_UNORM_SRGB)
            ob = Out(2, (108, 78), fill=0x5a)
        for e, c, o in ((a, ca, oa), (b, cb, ob)):
            e.tick(stream); e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        plain, got = oa.get(), ob.get()
        ref = _restate(d, plain, Tonemap.ACES_FITTED, table=table)
        assert not np.array_equal(_bits(ref), _bits(plain))
        if k < 4:
            _check(got, ref, 0, f"{name} frame {k}")
            launches = b.last_launches()
            assert launches[-1] == PassBit.POST and sum(1 for x in launches if x & PassBit.POST) == 1, [hex(x) for x in launches]
        else:
            graded, want = Out(0), Out(2, (108, 78), fill=0xa5)
            _process(b, d, plain, 0, disp, table, dst=graded)
            assert_bits_equal(graded.get(), ref, f"{name}: the process call")
            b.post_process(post, graded.ptr(), SIZE[0], SIZE[1], want.ptr(), 2, stream=stream)
            torch.cuda.synchronize()
            assert np.array_equal(got, want.get()), (name, np.abs(got.astype(int) - want.get().astype(int)).max())
    a.close(); b.close()


@pytest.mark.parametrize("exact,scene", [(False, "dungeon"), (True, "cornell")])
def test_the_whole_chain_equals_the_seven_process_calls(exact, scene):
    """fog, light shafts, depth of field, motion blur, bloom, the grade around ACES and FXAA (with a resample) in one frame against
    st_fog_process, st_light_shafts_process, st_dof_process, st_motion_blur_process, st_bloom_process (no display: the grade applies it),
    st_color_grading_process and st_post_process over the plain frame's colour, the velocity map and the G-buffer depth"""
    a, b = _engine(exact, scene), _engine(exact, scene)
    ca, cb = a.create_camera(_moving(scene, 0)), b.create_camera(_moving(scene, 0))
    fd = fog_desc(color=(0.5, 0.6, 0.7, 0.9), density=0.12, height_falloff=0.25, height_reference=0.5)
    sd = light_shafts_desc(steps=8, divisor=2, **C.MEDIUM, **C.SUN)
    dd = dof_desc(samples=32, autofocus=(0.5, 0.5), sensor_height=0.5, focal_distance=3.0)
    md, bd = motion_blur_desc(shutter=1.0, samples=8), bloom_desc(intensity=0.3, threshold=0.4, threshold_softness=0.5)
    disp = _disp(Tonemap.ACES_FITTED)
    post = post_desc(fxaa=True, output_size=(108, 78), filter=ResampleFilter.CATMULL_ROM)
    gd, table = _look(b, cb)
    b.set_fog(cb, fd); b.set_light_shafts(cb, sd); b.set_dof(cb, dd); b.set_motion_blur(cb, md); b.set_bloom(cb, bd); b.set_display(cb, disp); b.set_post(cb, post)
    b.set_output_format(cb, OutputFormat.RGBA8_UNORM_SRGB)
    oa, ob, depth = Out(0), Out(2, (108, 78), fill=0x5a), Depth()
    stream = torch.cuda.current_stream().cuda_stream
    tl = _lut_device(table)
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
        s0, s1, s2, s3, s4, s5, want = Out(0), Out(0), Out(0), Out(0), Out(0), Out(0), Out(2, (108, 78), fill=0xa5)
        cam = _moving(scene, k)
        b.fog_process(fd, _xf(cam), _proj(cam), oa.ptr(), tz.data_ptr(), w, h, s0.ptr(), 0, stream=stream)
        b.light_shafts_process(sd, _xf(cam), _proj(cam), s0.ptr(), tz.data_ptr(), w, h, s1.ptr(), 0, stream=stream)
        b.dof_process(dd, _proj(cam), s1.ptr(), tz.data_ptr(), w, h, s2.ptr(), 0, stream=stream)
        b.motion_blur_process(md, s2.ptr(), tv.data_ptr(), tz.data_ptr(), w, h, s3.ptr(), 0, stream=stream)
        b.bloom_process(bd, s3.ptr(), w, h, s4.ptr(), 0, stream=stream)
        b.color_grading_process(gd, s4.ptr(), w, h, s5.ptr(), 0, display=disp, lut_ptr=tl.data_ptr(), lut_size=table.shape[0], stream=stream)
        b.post_process(post, s5.ptr(), w, h, want.ptr(), 2, stream=stream)
        torch.cuda.synchronize()
        assert not np.array_equal(_bits(s5.get()), _bits(s4.get()))
        assert np.array_equal(ob.get(), want.get()), (exact, scene, k, np.abs(ob.get().astype(int) - want.get().astype(int)).max())
        launches = b.last_launches()
        assert launches[-1] == PassBit.POST and sum(1 for x in launches if x & PassBit.POST) == 2, [hex(x) for x in launches]   # the two pack launches, then the rest
    a.close(); b.close()


# ---------------------------------------------------------------- 4. off is off; nothing else changes
@pytest.mark.parametrize("exact", [False, True])
def test_a_cleared_setting_renders_like_a_camera_that_never_had_one(exact):
    C.cleared_setting_renders_like_none(NODE, exact)


def test_aovs_picks_planes_and_the_exposure_do_not_depend_on_the_setting():
    C.nothing_else_depends_on_the_setting(NODE)


@pytest.mark.parametrize("exact", [False, True])
def test_a_neutral_descriptor_renders_what_off_renders(exact):
    """on, but every step neutral (and a handle that names no table): the bytes of the camera without the setting, in RGBA32F without a
    display and in RGBA8 sRGB through ACES; the node's one launch is a copy through the display and the format"""
    a, b = _engine(exact), _engine(exact)
    ca, cb = a.create_camera(C._cornell(0)), b.create_camera(C._cornell(0))
    b.set_color_grading(cb, color_grading_desc(lut=LUT_ID + 7))
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(4):
        if k == 2:
            for e, c in ((a, ca), (b, cb)):
                e.set_display(c, tonemap=Tonemap.ACES_FITTED, exposure_ev=0.5); e.set_output_format(c, OutputFormat.RGBA8_UNORM_SRGB)
        oa, ob = (Out(0), Out(0, fill=0x5a)) if k < 2 else (Out(2), Out(2, fill=0x5a))
        for e, c, o in ((a, ca, oa), (b, cb, ob)):
            e.update_camera(c, C._cornell(k)); e.tick(stream); e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(oa.get()) if k < 2 else oa.get(), _bits(ob.get()) if k < 2 else ob.get()), (exact, k)
        assert b.last_launches() == a.last_launches() + [int(PassBit.POST)]
    a.close(); b.close()


# ---------------------------------------------------------------- 5. the frames that skip it, and the frames that do not
def test_heatmap_frames_skip_the_grade():
    C.frames_that_skip(NODE, "heatmap", (64, 48))


@pytest.mark.parametrize("what", ["reference", "orthographic"])
def test_reference_and_orthographic_frames_are_graded(what):
    """nothing in the grade depends on a G-buffer or on the projection"""
    size = (64, 48)
    a, b = _engine(True), _engine(True)
    cam = scenes.cornell_camera(size, CameraMode.REFERENCE, denoise=False, depth=1) if what == "reference" else _orthographic(size)
    ca, cb = a.create_camera(cam), b.create_camera(cam)
    d, table = _look(b, cb)
    oa, ob = Out(0, size), Out(0, size)
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(2):
        for e, c, o in ((a, ca, oa), (b, cb, ob)):
            e.tick(stream); e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        plain = oa.get()
        assert _bits(plain).any()
        _check(ob.get(), _restate(d, plain, None, table=table), 0, f"{what} frame {k}")
        assert not np.array_equal(_bits(ob.get()), _bits(plain))
        assert b.last_launches() == a.last_launches() + [int(PassBit.POST)]
    a.close(); b.close()


def test_auto_exposure_grades_with_the_scale_of_the_frame_before():
    """the meter reads the composed frame in the composing launch; the grade's display transform takes the scale the previous frame's
    finalize left, as every node's last store does"""
    a, b = _engine(False, "dungeon"), _engine(False, "dungeon")
    ca, cb = a.create_camera(C._dungeon(0)), b.create_camera(C._dungeon(0))
    auto = dict(tonemap=Tonemap.ACES_FITTED, auto_exposure=True, ev_min=-12.0, ev_max=8.0)
    b.set_display(cb, **auto)
    d, table = _look(b, cb)
    oa, ob = Out(0), Out(0)
    stream = torch.cuda.current_stream().cuda_stream
    scales = []
    for k in range(4):
        scale = b.exposure(cb)[0] if k else None     # what frame k - 1 left
        for e, c, o in ((a, ca, oa), (b, cb, ob)):
            e.update_camera(c, C._dungeon(k)); e.tick(stream); e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        if k:
            ref = R.grade_f32(oa.get(), d, Tonemap.ACES_FITTED, F(scale), lut=table, M=color_grading_plan(d)[1])
            _check(ob.get(), ref, 0, f"auto-exposure frame {k}")
            scales.append(float(scale))
    assert len(set(scales)) > 1, scales   # the exposure adapts while the camera moves
    a.close(); b.close()


# ---------------------------------------------------------------- 6. tiles
def _tiles(world, scene, grade, disp, size, group, frames=3):
    """`world` engines on one device render their windows and st_dist_gather assembles them on rank 0: the gathered frame"""
    stream = torch.cuda.current_stream().cuda_stream
    desc = scenes.cornell_camera(size)
    ranks = []
    for r in range(world):
        e = Engine(device=0, exact=True)
        if scene:
            scenes.build_cornell(e)
        else:
            e.set_blue_noise(scenes.load_blue_noise())
        e.set_seed(7)
        c = e.create_camera(desc)
        if grade is not None:
            e.insert_lut(LUT_ID, grade[1])
        if r % 2 == 0 and grade is not None:
            e.set_color_grading(c, grade[0])            # the grade, then the tile
        e.dist_init_local(r, world, group)
        owned, window = e.dist_set_partition(c, apron=0)
        if r % 2 == 1 and grade is not None:
            e.set_color_grading(c, grade[0])            # the tile, then the grade
        if disp is not None:
            e.set_display(c, disp)
        ranks.append((e, c, torch.full((size[1], size[0], 4), 7.0, dtype=torch.float32, device="cuda:0"), owned))
    full = torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda:0")
    for _ in range(frames):
        for r in range(world - 1, -1, -1):   # in-process transport: rank 0 last
            e, c, out, _ = ranks[r]
            e.tick(stream)
            e.render_camera(c, out.data_ptr(), stream)
            e.dist_gather(c, out.data_ptr(), full.data_ptr() if r == 0 else 0, stream)
    ranks[0][0].dist_wait(ranks[0][1], host=True)
    torch.cuda.synchronize()
    for e, c, out, (x0, y0, x1, y1) in ranks:
        o = out.cpu().numpy()
        outside = np.ones((size[1], size[0]), bool); outside[y0:y1, x0:x1] = False
        assert (o[outside] == 7.0).all(), "a rank wrote outside its window"
    got = full.cpu().numpy()
    for e, *_ in ranks:
        e.dist_shutdown(); e.close()
    return got


@pytest.mark.parametrize("world", [2, 4])
def test_graded_tiles_gather_to_the_graded_frame(world):
    """Cornell 64 x 48, the whole grade (dither and a table included) and a manual ACES display, as 2 and 4 windows gathered on one device.
    An Image frame's resampling and denoiser taps cross tile borders, so a composed Image frame gathered from tiles is not the single
    engine's at any commit, with or without grading (tests/test_gpu_fog.py says so too). What the grade adds is per pixel in frame
    coordinates, and that is held bit for bit: the gathered graded tiles are st_color_grading_process over the gathered tiles rendered
    without it — dither's pattern does not restart at a tile's corner. A frame without geometry has no such taps: there the gathered graded
    tiles are the single engine's graded frame bit for bit."""
    size = (64, 48)
    table = K.lut("random", 17)
    d = color_grading_desc(lut=LUT_ID, **GRADE)
    disp = display_desc(Tonemap.ACES_FITTED, exposure_ev=1.25)
    plain = _tiles(world, True, None, None, size, 7700 + world)
    got = _tiles(world, True, (d, table), disp, size, 7710 + world)
    one = Engine(device=0, exact=True)
    want = _process(one, d, plain, 0, disp, table)
    assert_bits_equal(got, want, f"{world} graded tiles against st_color_grading_process over the gathered plain tiles")
    assert not np.array_equal(_bits(got), _bits(plain))
    sky = _tiles(world, False, (d, table), disp, size, 7720 + world)
    one.set_blue_noise(scenes.load_blue_noise()); one.set_seed(7)
    c = one.create_camera(scenes.cornell_camera(size))
    one.insert_lut(LUT_ID, table)
    one.set_color_grading(c, d); one.set_display(c, disp)
    single = Out(0, size)
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        one.tick(stream); one.render_camera(c, single.ptr(), stream)
    torch.cuda.synchronize()
    assert_bits_equal(sky, single.get(), f"{world} graded sky tiles against one engine")
    one.close()


# ---------------------------------------------------------------- 7. pipelining: a table replaced and removed with frames in flight
def _pipeline(sync_every_frame, streams=1, profiling=False, frames=8):
    """dungeon frames through RGBA8 sRGB and ACES with the whole grade; the table is replaced in front of frame 3 and removed in front of
    frame 6 (each edit takes effect at that frame's tick): (the frames, the launches per profile slot when profiling)"""
    e = _engine(False, "dungeon")
    if profiling:
        e.profile_enable(1)   # per-kernel timing: the serial schedule
    cam = e.create_camera(C._dungeon4(0))
    e.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
    e.set_display(cam, tonemap=Tonemap.ACES_FITTED, exposure_ev=0.5)
    _look(e, cam, table=K.lut("random", 33))
    ss = [torch.cuda.Stream() for _ in range(streams)]
    outs = [Out(2) for _ in range(frames)]
    torch.cuda.synchronize()
    for k in range(frames):
        s = ss[k % streams].cuda_stream
        if k == 3:
            e.insert_lut(LUT_ID, K.lut("random", 17, seed=9))
        if k == 6:
            e.remove_lut(LUT_ID)
        e.update_camera(cam, C._dungeon4(k))
        e.tick(s)
        e.render_camera(cam, outs[k].ptr(), s)
        if sync_every_frame:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    got = [o.get() for o in outs]
    names = {p["name"]: p["launches"] for p in e.profile_read()} if profiling else None
    e.close()
    return got, names


def test_a_table_replaced_or_removed_with_frames_in_flight_serves_the_frames_that_read_it():
    base, _ = _pipeline(True)
    # the edits show: the same view with each of the three states of the table differs
    e = _engine(False, "dungeon")
    cam = e.create_camera(C._dungeon4(0))
    e.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
    e.set_display(cam, tonemap=Tonemap.ACES_FITTED, exposure_ev=0.5)
    d, _t = _look(e, cam, table=K.lut("random", 33))
    stills = []
    for edit in (lambda: None, lambda: e.insert_lut(LUT_ID, K.lut("random", 17, seed=9)), lambda: e.remove_lut(LUT_ID)):
        edit()
        o = Out(2)
        stills.append(C._frame(e, cam, o))
    e.close()
    assert not np.array_equal(stills[0], stills[1]) and not np.array_equal(stills[1], stills[2]) and not np.array_equal(stills[0], stills[2])
    for kw in (dict(), dict(streams=2), dict(profiling=True)):
        for sync in ((False,) if not kw else (True, False)):
            other, names = _pipeline(sync, **kw)
            for k, (x, y) in enumerate(zip(other, base)):
                assert np.array_equal(x, y), (kw, sync, k)
            if names is not None:
                assert names["color_grading"] == 8, names


def test_frames_in_flight_read_their_own_inputs():
    C.frames_in_flight_read_their_own_inputs(NODE)


# ---------------------------------------------------------------- 8. lifecycle
def test_resizes_toggles_arithmetic_switches_tiny_frames_and_teardown():
    a, b = _engine(False), _engine(False)
    stream = torch.cuda.current_stream().cuda_stream
    ca, cb = a.create_camera(scenes.cornell_camera(SIZE)), b.create_camera(scenes.cornell_camera(SIZE))
    d, table = _look(b, cb)
    step = 0
    for size in (SIZE, (96, 80), (8, 8), (1, 1), SIZE):   # larger, tiny, back: the setting, the table and the results stay
        if size == SIZE and step:
            for e in (a, b):
                e.set_exact(True); e.set_exact(False)   # ... and across an arithmetic switch
        cam = scenes.cornell_camera(size)
        for e, c in ((a, ca), (b, cb)):
            e.update_camera(c, cam)
        for rep_ in range(2):
            if rep_ == 1 and size == (96, 80):
                b.set_color_grading(cb, None); b.set_color_grading(cb, d)   # a toggle between two frames
            oa, ob = Out(0, size), Out(0, size)
            a.tick(stream); b.tick(stream)
            a.render_camera(ca, oa.ptr(), stream); b.render_camera(cb, ob.ptr(), stream)
            torch.cuda.synchronize()
            assert b.get_color_grading(cb)[1] and b.get_color_grading(cb)[0].contrast == F(GRADE["contrast"])
            _check(ob.get(), _restate(d, oa.get(), None, table=table), 0, f"size {size} step {step}")
            step += 1
    # a handle that names no table: the step is skipped, the rest runs
    b.update_camera(cb, scenes.cornell_camera(SIZE)); a.update_camera(ca, scenes.cornell_camera(SIZE))
    b.set_color_grading(cb, color_grading_desc(lut=LUT_ID + 1, **GRADE))
    oa, ob = Out(0), Out(0)
    a.tick(stream); b.tick(stream)
    a.render_camera(ca, oa.ptr(), stream); b.render_camera(cb, ob.ptr(), stream)
    torch.cuda.synchronize()
    _check(ob.get(), _restate(color_grading_desc(**GRADE), oa.get(), None), 0, "a handle without a table")
    b.set_color_grading(cb, d)
    # delete a camera with the setting on and a frame in flight; a new camera starts clean; destroy the engine with a graded frame in flight
    C.teardown_with_the_setting_on(NODE, b, cb)
    a.close(); b.close()


# ---------------------------------------------------------------- 9. the launch list
def test_a_graded_frame_adds_one_post_launch_named_color_grading():
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "render_launches.json")))["default"]
    stream = torch.cuda.current_stream().cuda_stream
    for graded in (False, True):
        for profiled in (False, True):
            e = Engine(device=0)
            scenes.build_cornell(e)
            e.set_seed(7)
            cam = e.create_camera(scenes.cornell_camera((64, 48)))
            if graded:
                _look(e, cam)
            if profiled:
                e.profile_enable(1 | 8)
            out = torch.zeros((48, 64, 4), dtype=torch.float32, device="cuda:0")
            for frame in range(1, 7):
                e.tick(stream)
                e.render_camera(cam, out.data_ptr(), stream)
                torch.cuda.synchronize()
                if profiled:
                    got = {p["name"]: p["launches"] for p in e.profile_read(reset=True) if p["launches"]}
                    want = dict(golden["profiled"][frame - 1][1], **({"color_grading": 1} if graded else {}))
                else:
                    got, want = e.last_launches(), golden["full"][frame - 1][1] + ([int(PassBit.POST)] if graded else [])
                assert got == want, (graded, profiled, frame, got, want)
            e.close()
