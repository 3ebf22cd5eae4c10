"""GPU tests of light shafts (include/strolle_hip.h "light shafts"; k_shafts.hip, st_shafts.cpp).

st_light_shafts_process on the synthetic matrix (shafts_cases.py) over both slat scenes against the numpy restatement (shafts_ref.shafts_f32)
bit for bit: the exact build with the CHECKER's occlusion (independent of the engine's walk), the fast build with visibility from its own
st_scene_occluded on the restatement's rays (the ray-for-ray test that the march's walk is the query's) and within the profile's tolerance
of the float64 definition on non-ambiguous pixels. `slats` (34 triangles) takes the scene-in-LDS instantiation, `slats600` (546) and the
dungeon the 16-bit stack slots, the 208 k-triangle dungeon in the exact build the 32-bit ones. Then properties that do not rest on the
restatement, whole frames against the restatement of the same frame without the setting (with the ray count), the whole chain against the
six process calls, ST_SHAFTS_FOLLOW_SUN across a tick, a light removed between frames, off is off, nothing else changes, the frames that
skip the node, pipelining, lifecycle. Every test uses entry points the parent commit does not have.

Sizes: 72 x 52, 41 x 23, 9 x 9, 5 x 5, 1 x 1: partial 8 x 8-cell tiles, more than one workgroup, odd sizes for the partial cells of divisor 2."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

import display_ref
import shafts_cases as K
import shafts_ref as R
from geometry_extremes import oracle_trace
from oracle_binding import OracleEngine
import output_chain as C
from output_chain import MEDIUM, SUN, Depth, Out, _bits, _check, _engine, _moving, _proj, _scene_camera, _xf
from strolle_amd import (Buffer, Engine, Light, OutputFormat, PassBit, ResampleFilter, Sun, Tonemap, bloom_desc, display_desc, dof_desc, fog_desc,
                         light_shafts_desc, motion_blur_desc, post_desc, scenes)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (72, 52)
F = np.float32
CORNELL_LIGHTS = {1: Light.point((math.sin(0.0) / 2.0, 1.5, math.cos(0.0) / 2.0), 0.15, (50.0 / (4.0 * math.pi),) * 3, 20.0)}
DUNGEON_LIGHTS = {1 + i: Light.point(p, 0.15, (5000.0 / (4.0 * math.pi),) * 3, 35.0)
                  for i, p in enumerate([(-3.0, 0.75, -23.0), (-23.5, 0.75, -31.0), (1.25, 0.75, -10.5), (-3.15, 0.75, 1.25), (-3.25, 0.75, 20.25), (13.25, 0.75, -28.25)])}
SCENE_LIGHTS = {"cornell": CORNELL_LIGHTS, "dungeon": DUNGEON_LIGHTS}


def _tool():
    spec = importlib.util.spec_from_file_location("shafts_bench", os.path.join(ROOT, "tools", "shafts_bench.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def _ref(key, make):
    return C._ref(__name__, key, make)


def _own_occlusion(e):
    """visibility from the engine's own st_scene_occluded"""
    def occluded(rays):
        r = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8)).cuda()
        out = torch.full((len(rays),), 7, dtype=torch.int32, device="cuda:0")
        e.occluded(r.data_ptr(), len(rays), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert ((o == 0) | (o == 1)).all()
        return o == 1
    return occluded


def _process(e, d, color, depth, M, P, fmt=0, display=None, stream=None):
    h, w = color.shape[:2]
    tc, tz = torch.from_numpy(color).cuda(), torch.from_numpy(depth).cuda()
    out = Out(fmt, (w, h), fill=0x5a)
    e.light_shafts_process(d, M, P, tc.data_ptr(), tz.data_ptr(), w, h, out.ptr(), fmt, display=display,
                           stream=stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.get()


def _slats(exact, scene):
    e = Engine(device=0, exact=exact)
    K.build_slats(e, K.SCENES[scene])
    e.set_seed(7)
    e.tick(torch.cuda.current_stream().cuda_stream)
    return e


def _checker(scene):
    def make():
        o = OracleEngine()
        K.build_slats(o, K.SCENES[scene]); o.tick()
        return o
    return _ref(("checker", scene), make)


# ---------------------------------------------------------------- 1. bit for bit against the restatement
@pytest.mark.parametrize("scene", list(K.SCENES))
def test_the_exact_build_matches_the_restatement_with_the_checkers_occlusion(scene):
    e = _slats(True, scene)
    orac = _checker(scene)
    changed = kept = 0
    for name, size, kind, d in K.cases():
        img, z, M, P = K.inputs(size, kind)
        want, n = _ref(("probe", scene, name), lambda: R.shafts_f32(img, z, M, P, d, K.table_lights(d), lambda r: oracle_trace(orac, r)[4]))
        got = _process(e, d, img, z, M, P)
        print(f"{scene} {name}: {n} shadow rays")
        _check(got, want, 0, f"{scene} {name}")
        same = (_bits(got) == _bits(img)).all(-1)
        changed += int((~same).sum()); kept += int(same.sum())
    assert changed > 4000 and kept > 20, (changed, kept)
    # the four output formats, without a display and with a manual ACES one
    name, size, kind, d = K.cases()[0]
    img, z, M, P = K.inputs(size, kind)
    plain, _ = C._REFS[__name__, ("probe", scene, name)]
    for op in (None, Tonemap.ACES_FITTED):
        disp = display_desc(tonemap=op, exposure_ev=-1.5) if op is not None else None
        want = plain if op is None else display_ref.transform(plain[..., :3], int(op), display_ref.manual_scale(-1.5))
        for fmt in range(4):
            _check(_process(e, d, img, z, M, P, fmt, disp), want, fmt, f"{scene} {op} fmt={fmt}")
    e.close()


@pytest.mark.parametrize("scene", list(K.SCENES))
def test_the_fast_build_walks_what_its_own_query_walks(scene):
    """bit for bit with visibility from its own st_scene_occluded on the restatement's rays; and, on `slats`, within the profile's tolerance of
    the float64 definition wherever no cell is ambiguous"""
    e = _slats(False, scene)
    with open(os.path.join(ROOT, "profiles", "light_shafts.json")) as f:
        prof = json.load(f)["reference"][scene]
    tool = _tool()
    for name, size, kind, d in K.cases():
        img, z, M, P = K.inputs(size, kind)
        want, n = R.shafts_f32(img, z, M, P, d, K.table_lights(d), _own_occlusion(e))
        got = _process(e, d, img, z, M, P)
        _check(got, want, 0, f"{scene} {name}")
        if scene == "slats":
            c = _ref(("definition", scene), lambda: tool.reference_scene(scene))["cases"][name]
            sure = tool.pixel_cell_margin(c) >= prof["threshold"]
            dev = tool.deviation(got, c["want"])
            print(f"{name}: worst deviation from the definition {np.nanmax(np.where(sure[..., None], dev, 0), initial=0.0):.3g} on {int(sure.sum())} pixels, tolerance {prof['tolerance']:.3g}")
            assert not (np.nan_to_num(dev[sure]) > prof["tolerance"]).any(), name
    e.close()


def _dungeon_inputs(size, cam):
    w, h = size
    img = np.full((h, w, 4), 0.25, np.float32); img[..., 3] = 1.0
    z = K.depth("plane", w, h) * F(0.5)
    return img, z, _xf(cam), _proj(cam)


@pytest.mark.parametrize("case", [("dungeon_fast_wide_16", False, 0, (41, 23)), ("dungeon_exact_16", True, 0, (9, 9)), ("dungeon208k_exact_32", True, 2, (9, 9))], ids=lambda c: c[0])
def test_the_dungeons_walk_what_their_own_query_walks(case):
    """the wide stream with 16-bit slots (fast), the contract stream with 16-bit slots, and — 208 k triangles, more than 65,536 stream entries —
    32-bit slots: st_light_shafts_process bit for bit with visibility from the same engine's st_scene_occluded"""
    name, exact, subdivide, size = case
    e = Engine(device=0, exact=exact)
    scenes.build_dungeon(e, subdivide=subdivide)
    e.set_seed(7)
    e.tick(torch.cuda.current_stream().cuda_stream)
    if subdivide:
        assert len(e.read_scene(1)) // 36 > 200000
    cam = scenes.dungeon_camera(size)
    d = light_shafts_desc(steps=8, divisor=2, lights=(1, 3), **MEDIUM, **SUN)
    img, z, M, P = _dungeon_inputs(size, cam)
    lights = [R.table_light(DUNGEON_LIGHTS[h]) for h in (1, 3)]
    det = {}
    want, n = R.shafts_f32(img, z, M, P, d, lights, _own_occlusion(e), details=det)
    lit = sum(int((~x[4]).sum()) for x in det["log"])
    assert 0 < lit < n, "both lit and shadowed samples"
    _check(_process(e, d, img, z, M, P), want, 0, name)
    e.close()


# ---------------------------------------------------------------- 2. properties that do not rest on the restatement
@pytest.mark.parametrize("exact", [True, False])
def test_properties_of_the_shafts(exact):
    e = _slats(exact, "slats600")
    for size in K.SIZES:
        img, z, M, P = K.inputs(size, "odd")
        # nothing to add: density 0, no lights and no sun, intensity 0, albedo 0 — the input's own bits on every pixel
        for kw in (dict(K.BASE, density=0.0, **K.SUN), dict(K.BASE), dict(K.BASE, lights=(K.MISSING,)), dict(K.BASE, intensity=0.0, lights=(K.POINT,), **K.SUN),
                   dict(K.BASE, scatter=(0.0, 0.0, 0.0), **K.SUN)):
            for div in (1, 2):
                got = _process(e, light_shafts_desc(steps=4, divisor=div, **kw), img, z, M, P)
                assert np.array_equal(_bits(got), _bits(img)), (size, kw, div)
        # no finite input produces NaN; pixels without a distance keep their bits; the alpha is the pixel's own
        clean = np.abs(np.nan_to_num(img, nan=1.0, posinf=2.0, neginf=-2.0))
        for div in (1, 2):
            got = _process(e, light_shafts_desc(steps=4, divisor=div, lights=(K.POINT, K.SPOT), light_extinction=True, **K.BASE, **K.SUN), clean, z, M, P)
            assert np.isfinite(got).all(), (size, div)
            through = ~(z > 0)
            assert np.array_equal(_bits(got[through]), _bits(clean[through])) and np.array_equal(_bits(got[..., 3]), _bits(clean[..., 3])), (size, div)
            assert (got[..., :3] >= np.minimum(clean[..., :3], 65504.0)).all(), "light is only added"
    e.close()
    # an occluder-free scene: the closed form sigma_s E (1 - e^(-sigma d)) / (4 pi sigma) within the stratified bound, every pixel, g = 0
    e = Engine(device=0, exact=exact)
    e.set_blue_noise(scenes.load_blue_noise()); e.tick(torch.cuda.current_stream().cuda_stream)
    w, h = 41, 23
    black = np.zeros((h, w, 4), np.float32)
    for steps, dist, sigma in ((16, 6.0, 0.2), (64, 20.0, 0.05)):
        d = light_shafts_desc(steps=steps, divisor=1, density=sigma, anisotropy=0.0, max_distance=100.0, intensity=1.0, scatter=(1.0, 0.6, 0.2), sun_color=(5.0, 5.0, 5.0))
        got = _process(e, d, black, np.full((h, w), dist, np.float32), K.transform((w, h)), K.projection((w, h)))
        s = float(F(sigma))
        for i, alb in enumerate((1.0, float(F(0.6)), float(F(0.2)))):
            exact_value = alb * 5.0 * (1 - math.exp(-s * dist)) / (4 * math.pi)
            bound = alb * 5.0 / (4 * math.pi) * s * (s * dist * dist / (2 * steps)) + 1e-5 * exact_value   # (+ float32's rounding of the sum)
            assert np.abs(got[..., i].astype(np.float64) - exact_value).max() <= bound, (steps, i)
    e.close()


def test_a_pixel_behind_a_slat_is_darker_than_its_lit_neighbour():
    """a camera 2 m behind the wall, at the height of a slat's edge (z = -3.2), looks away from it along -x over a depth of 0.3 m; the sun
    alone, low, through the wall along +x: the samples of the columns on one side of the centre lie behind the slat (z in [-3.55, -3.2]) and
    receive nothing, those on the other side lie behind the gap and are lit"""
    e = _slats(False, "slats")
    w, h = 72, 9
    cam = scenes.camera_for((w, h), (1.0, 1.0, -3.2), (-5.0, 1.0, -3.2))
    d = light_shafts_desc(steps=8, divisor=1, density=0.3, anisotropy=0.0, max_distance=50.0, intensity=1.0, scatter=(1.0, 1.0, 1.0), sun_color=(5.0, 5.0, 5.0),
                          sun_direction=(1.0, 0.4, 0.0))
    black = np.zeros((h, w, 4), np.float32)
    row = _process(e, d, black, np.full((h, w), 0.3, np.float32), _xf(cam), _proj(cam))[h // 2, :, 0]
    dark, lit = sorted((float(row[30]), float(row[41])))
    assert dark == 0.0 and lit > 0.01, (row[30], row[41])
    assert (row[20:31] == row[30]).all() or (row[20:31] > 0).all() == (row[30] > 0)   # the whole side is of one kind
    e.close()


# ---------------------------------------------------------------- 3. whole frames
FRAME_CASES = [("cornell_fast", False, "cornell", 2, 8), ("cornell_exact", True, "cornell", 1, 4), ("dungeon_fast", False, "dungeon", 2, 8), ("dungeon_exact", True, "dungeon", 2, 4)]


def _frame_desc(scene, divisor, steps, **more):
    return light_shafts_desc(steps=steps, divisor=divisor, lights=(1,) if scene == "cornell" else (3, 1), **dict(MEDIUM, **SUN, **more))


NODE = C.Node("set_light_shafts", "get_light_shafts", "shafts", "the frame with shafts differs", ("shafts_march", "shafts_apply"), _frame_desc("cornell", 2, 8),
              independent=_frame_desc("dungeon", 2, 8), pipelined=_frame_desc("dungeon", 2, 8), recreated=_frame_desc("cornell", 2, 4), counts_rays=True)


@pytest.mark.parametrize("case", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_a_frame_with_shafts_equals_the_restatement_of_the_frame_without(case):
    name, exact, scene, divisor, steps = case
    d = _frame_desc(scene, divisor, steps)
    a, b = _engine(exact, scene), _engine(exact, scene)
    cam = _scene_camera(scene, SIZE)
    ca, cb = a.create_camera(cam), b.create_camera(cam)
    b.set_light_shafts(cb, d)
    assert b.get_light_shafts(cb)[1]
    lights = [R.table_light(SCENE_LIGHTS[scene][int(d.lights[i])]) for i in range(d.light_count)]
    oa, ob, depth = Out(0), Out(0, fill=0x5a), Depth()
    stream = torch.cuda.current_stream().cuda_stream
    changed = False
    for k in range(3):
        for e, c, o in ((a, ca, oa), (b, cb, ob)):
            e.ray_count(c, reset=True)
            e.tick(stream); e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        plain, got = oa.get(), ob.get()
        ref, n = R.shafts_f32(plain, depth.read(b, cb, SIZE), _xf(cam), _proj(cam), d, lights, _own_occlusion(b))
        changed |= not np.array_equal(_bits(ref), _bits(plain))
        _check(got, ref, 0, f"{name} frame {k}")
        assert n > 0 and b.ray_count(cb) - a.ray_count(ca) == n, (name, k, n, b.ray_count(cb), a.ray_count(ca))
        launches = b.last_launches()
        assert launches[-1] == PassBit.POST and sum(1 for x in launches if x & PassBit.POST) == 1, [hex(x) for x in launches]
    assert changed, "the shafts should change some pixel"
    a.close(); b.close()


def test_a_cornell_frame_in_the_exact_build_with_the_checkers_occlusion():
    d = _frame_desc("cornell", 2, 4)
    a, b, orac = _engine(True), _engine(True), OracleEngine()
    scenes.build_cornell(orac); orac.tick()
    cam = _scene_camera("cornell", SIZE)
    ca, cb = a.create_camera(cam), b.create_camera(cam)
    b.set_light_shafts(cb, d)
    oa, ob, depth = Out(0), Out(0, fill=0x5a), Depth()
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(2):
        for e, c, o in ((a, ca, oa), (b, cb, ob)):
            e.tick(stream); e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        ref, n = R.shafts_f32(oa.get(), depth.read(b, cb, SIZE), _xf(cam), _proj(cam), d, [R.table_light(CORNELL_LIGHTS[1])], lambda r: oracle_trace(orac, r)[4])
        _check(ob.get(), ref, 0, f"frame {k}")
    a.close(); b.close(); orac.close()


@pytest.mark.parametrize("exact,scene", [(False, "dungeon"), (True, "cornell")])
def test_the_whole_chain_equals_the_six_process_calls(exact, scene):
    """fog, light shafts, depth of field, motion blur, bloom, ACES and FXAA (with a resample) in one frame against st_fog_process,
    st_light_shafts_process, st_dof_process, st_motion_blur_process, st_bloom_process and st_post_process over the plain frame's colour"""
    a, b = _engine(exact, scene), _engine(exact, scene)
    ca, cb = a.create_camera(_moving(scene, 0)), b.create_camera(_moving(scene, 0))
    fd = fog_desc(color=(0.5, 0.6, 0.7, 0.9), density=0.12, height_falloff=0.25, height_reference=0.5)
    sd = _frame_desc(scene, 2, 8)
    dd = dof_desc(samples=32, autofocus=(0.5, 0.5), sensor_height=0.5, focal_distance=3.0)
    md, bd = motion_blur_desc(shutter=1.0, samples=8), bloom_desc(intensity=0.3, threshold=0.4, threshold_softness=0.5)
    disp = display_desc(tonemap=Tonemap.ACES_FITTED, exposure_ev=0.5)
    post = post_desc(fxaa=True, output_size=(108, 78), filter=ResampleFilter.CATMULL_ROM)
    b.set_fog(cb, fd); b.set_light_shafts(cb, sd); b.set_dof(cb, dd); b.set_motion_blur(cb, md); b.set_bloom(cb, bd); b.set_display(cb, disp); b.set_post(cb, post)
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
            continue
        tz, tv = torch.from_numpy(z).cuda(), torch.from_numpy(v).cuda()
        s0, s1, s2, s3, s4, want = Out(0), Out(0), Out(0), Out(0), Out(0), Out(2, (108, 78), fill=0xa5)
        cam = _moving(scene, k)
        b.fog_process(fd, _xf(cam), _proj(cam), oa.ptr(), tz.data_ptr(), w, h, s0.ptr(), 0, stream=stream)
        b.light_shafts_process(sd, _xf(cam), _proj(cam), s0.ptr(), tz.data_ptr(), w, h, s1.ptr(), 0, stream=stream)
        b.dof_process(dd, _proj(cam), s1.ptr(), tz.data_ptr(), w, h, s2.ptr(), 0, stream=stream)
        b.motion_blur_process(md, s2.ptr(), tv.data_ptr(), tz.data_ptr(), w, h, s3.ptr(), 0, stream=stream)
        b.bloom_process(bd, s3.ptr(), w, h, s4.ptr(), 0, display=disp, stream=stream)
        b.post_process(post, s4.ptr(), w, h, want.ptr(), 2, stream=stream)
        torch.cuda.synchronize()
        assert not np.array_equal(_bits(s0.get()), _bits(oa.get())) and not np.array_equal(_bits(s1.get()), _bits(s0.get()))
        assert np.array_equal(ob.get(), want.get()), (exact, scene, k, np.abs(ob.get().astype(int) - want.get().astype(int)).max())
        launches = b.last_launches()
        assert launches[-1] == PassBit.POST and sum(1 for x in launches if x & PassBit.POST) == 2, [hex(x) for x in launches]   # the two pack launches, then the rest
    a.close(); b.close()


def test_follow_sun_takes_the_direction_of_the_last_tick_and_a_removed_light_drops_out():
    first, second = Sun(azimuth=0.6, altitude=0.5), Sun(azimuth=0.0, altitude=0.0)   # the second: (0, 0, -1) exactly
    d = light_shafts_desc(steps=4, divisor=2, lights=(50,), follow_sun=True, sun_color=(6.0, 5.0, 4.0), sun_direction=(0.0, 0.0, 0.0), **MEDIUM)
    a, b = _engine(False, "dungeon"), _engine(False, "dungeon")
    torch_light = Light.point((-5.75, 1.0, -19.0), 0.1, (200.0, 150.0, 100.0), 20.0)   # in the open, 2.2 m in front of the camera; the table's last slot
    for e in (a, b):
        e.insert_light(50, torch_light)
    cam = _scene_camera("dungeon", SIZE)
    ca, cb = a.create_camera(cam), b.create_camera(cam)
    b.set_light_shafts(cb, d)
    oa, ob, depth = Out(0), Out(0), Depth()
    stream = torch.cuda.current_stream().cuda_stream
    south = np.array([0, 0, -1], np.float32)

    def frame(tick):
        for e, c, o in ((a, ca, oa), (b, cb, ob)):
            if tick:
                e.tick(stream)
            e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        return oa.get(), ob.get(), depth.read(b, cb, SIZE)

    def restate(plain, z, sun, lights):
        return R.shafts_f32(plain, z, _xf(cam), _proj(cam), d, lights, _own_occlusion(b), sun=sun)[0]

    l3 = [R.table_light(torch_light)]
    frame(True); frame(True)
    for e in (a, b):
        e.update_sun(second)
    plain, got, z = frame(False)     # not before the next tick
    assert not np.array_equal(_bits(restate(plain, z, south, l3)), _bits(got)) and not np.array_equal(_bits(plain), _bits(got))
    plain, got, z = frame(True)      # after it
    _check(got, restate(plain, z, south, l3), 0, "the sun of the last tick")
    # light 1 goes: light 50 moves to another slot of the table and stays; then light 50 goes: its handle is skipped, no error
    for e in (a, b):
        e.remove_light(1)
    plain, got, z = frame(True)
    _check(got, restate(plain, z, south, l3), 0, "another light removed")
    for e in (a, b):
        e.remove_light(50)
    plain, got, z = frame(False)     # the table of the last tick still holds it
    _check(got, restate(plain, z, south, l3), 0, "removed, not yet ticked")
    plain, got, z = frame(True)
    want = restate(plain, z, south, [])
    _check(got, want, 0, "the handle names no light")
    assert not np.array_equal(_bits(want), _bits(restate(plain, z, south, l3)))
    a.close(); b.close()


# ---------------------------------------------------------------- 4. off is off; nothing else changes
@pytest.mark.parametrize("exact", [False, True])
def test_a_cleared_setting_renders_like_a_camera_that_never_had_one(exact):
    C.cleared_setting_renders_like_none(NODE, exact)


def test_aovs_picks_planes_and_the_exposure_do_not_depend_on_the_setting():
    C.nothing_else_depends_on_the_setting(NODE)


@pytest.mark.parametrize("what", ["reference", "heatmap", "orthographic"])
def test_frames_that_skip_the_shafts(what):
    C.frames_that_skip(NODE, what, (64, 48))


# ---------------------------------------------------------------- 5. pipelining
def test_frames_in_flight_read_their_own_depths():
    C.frames_in_flight_read_their_own_inputs(NODE)


# ---------------------------------------------------------------- 6. lifecycle
def test_resizes_toggles_arithmetic_switches_tiny_frames_and_teardown():
    a, b = _engine(False), _engine(False)
    d = _frame_desc("cornell", 2, 4)
    lights = [R.table_light(CORNELL_LIGHTS[1])]
    stream = torch.cuda.current_stream().cuda_stream
    ca, cb = a.create_camera(scenes.cornell_camera(SIZE)), b.create_camera(scenes.cornell_camera(SIZE))
    b.set_light_shafts(cb, d)
    step = 0
    for size in (SIZE, (96, 80), (9, 9), (1, 1), SIZE):   # larger, tiny, back: the setting and the results stay
        if size == SIZE and step:
            for e in (a, b):
                e.set_exact(True); e.set_exact(False)   # ... and across an arithmetic switch
        cam = scenes.cornell_camera(size)
        for e, c in ((a, ca), (b, cb)):
            e.update_camera(c, cam)
        p = Depth()
        for rep_ in range(2):
            if rep_ == 1 and size == (96, 80):
                b.set_light_shafts(cb, None); b.set_light_shafts(cb, d)   # a toggle between two frames
            oa, ob = Out(0, size), Out(0, size)
            a.tick(stream); b.tick(stream)
            a.render_camera(ca, oa.ptr(), stream); b.render_camera(cb, ob.ptr(), stream)
            torch.cuda.synchronize()
            assert b.get_light_shafts(cb)[1] and b.get_light_shafts(cb)[0].steps == 4
            ref, _ = R.shafts_f32(oa.get(), p.read(b, cb, size), _xf(cam), _proj(cam), d, lights, _own_occlusion(b))
            _check(ob.get(), ref, 0, f"size {size} step {step}")
            step += 1
    # delete a camera with the setting on and a frame in flight; a new camera starts clean; destroy the engine with such a frame in flight
    C.teardown_with_the_setting_on(NODE, b, cb)
    a.close(); b.close()
