"""GPU tests of fog (include/strolle_hip.h "fog"; k_fog.hip, st_fog.cpp): st_fog_process on the synthetic input matrix (fog_cases.py)
against the numpy restatement (fog_ref.fog_f32) bit for bit in both builds; properties that do not rest on the restatement; whole frames
with fog on against the restatement fed the same frame rendered without it and the G-buffer depth read back; the whole output chain against
the five process calls; off is off; nothing else changes; the frames that skip it; tiles; pipelining across frames; lifecycle. Every test
builds its own engines and uses entry points the parent commit does not have.

Sizes: the workgroup is 32 x 8 pixels, so 72 x 52 (partial groups both ways), 33 x 21, 64 x 8 (exactly the groups), 5 x 5 and 1 x 1."""
import numpy as np
import pytest
import torch

import display_ref
import fog_cases as K
import fog_ref as R
import output_chain as C
from output_chain import Depth, Out, _bits, _check, _engine, _moving, _proj, _scene_camera, _xf
from parity import assert_bits_equal
from strolle_amd import (Buffer, Engine, FogFalloff, OutputFormat, PassBit, ResampleFilter, Sun, Tonemap, bloom_desc, display_desc, dof_desc,
                         fog_desc, motion_blur_desc, post_desc, scenes)

pytestmark = pytest.mark.gpu
SIZE = K.SIZE
F = np.float32
FOG = dict(falloff=FogFalloff.EXPONENTIAL, color=(0.5, 0.6, 0.7, 0.9), density=0.12, height_falloff=0.25, height_reference=0.5, sky_distance=60.0,
           light_color=(1.0, 0.7, 0.0), light_exponent=8.0, light_direction=(0.3, 0.5, -0.8))
NODE = C.Node("set_fog", "get_fog", "fog", "the fogged frame differs", ("fog",), FOG)


def _ref(key, make):
    return C._ref(__name__, key, make)


def _process(e, d, color, depth, M, P, fmt=0, display=None, stream=None):
    h, w = color.shape[:2]
    tc, tz = torch.from_numpy(color).cuda(), torch.from_numpy(depth).cuda()
    out = Out(fmt, (w, h), fill=0x5a)
    e.fog_process(d, M, P, tc.data_ptr(), tz.data_ptr(), w, h, out.ptr(), fmt, display=display,
                  stream=stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.get()


def _restate(d, color, depth, M, P, display=None, scale=None, sun=None):
    c = R.fog_f32(color, depth, M, P, d, sun=sun)
    if display is None:
        return c
    return display_ref.transform(c[..., :3], int(display), scale)


# ---------------------------------------------------------------- 1. bit for bit against the restatement
@pytest.mark.parametrize("exact", [True, False])
def test_process_matches_the_restatement_on_synthetic_inputs(exact):
    e = Engine(device=0, exact=exact)
    changed = kept = 0
    for name, size, kind, t, d in K.cases():
        img, z, M, P = K.inputs(size, kind, t)
        want = _ref(name, lambda: _restate(d, img, z, M, P))
        got = _process(e, d, img, z, M, P)
        _check(got, want, 0, f"{name} exact={exact}")
        same = (_bits(got) == _bits(img)).all(-1)
        changed += int((~same).sum()); kept += int(same.sum())
    assert changed > 50000 and kept > 5000, (changed, kept)
    # the four output formats, without a display and with a manual ACES one
    name, size, kind, t, d = next(c for c in K.cases() if c[0] == "f1h0l1s1-blocks-low")
    img, z, M, P = K.inputs(size, kind, t)
    for op in (None, Tonemap.ACES_FITTED):
        disp = display_desc(tonemap=op, exposure_ev=-1.5) if op is not None else None
        want = _ref(("fmt", op), lambda: _restate(d, img, z, M, P, op, display_ref.manual_scale(-1.5) if op is not None else None))
        for fmt in range(4):
            _check(_process(e, d, img, z, M, P, fmt, disp), want, fmt, f"exact={exact} {op} fmt={fmt}")
    # a projection with a lens shift and a mirrored x axis
    shifted = P.copy(); shifted[0] = -shifted[0]; shifted[8] = 0.2; shifted[9] = -0.1
    _check(_process(e, d, img, z, M, shifted), _ref("shifted", lambda: _restate(d, img, z, M, shifted)), 0, f"exact={exact} shifted projection")
    e.close()


# ---------------------------------------------------------------- 2. properties that do not rest on the restatement
@pytest.mark.parametrize("exact", [True, False])
def test_properties_of_the_fog(exact):
    e = Engine(device=0, exact=exact)
    other = Engine(device=0, exact=not exact)
    for (w, h) in K.SIZES:
        img, z, M, P = K.inputs((w, h), "blocks", "rolled")
        # nothing to add: alpha 0, density 0, a linear ramp that starts beyond every depth — the input's own bits on every pixel
        for kw in (dict(FOG, color=(0.5, 0.6, 0.7, 0.0)), dict(FOG, density=0.0), dict(FOG, falloff=FogFalloff.LINEAR, start=500.0, end=600.0, height_falloff=0.0),
                   dict(falloff=FogFalloff.ATMOSPHERIC, sky_distance=5.0)):
            got = _process(e, fog_desc(**kw), img, z, M, P)
            assert np.array_equal(_bits(got), _bits(img)), (w, h, kw)
        # without ST_FOG_SKY sky pixels (and every depth that is not > 0) keep their bits, the others do not all keep theirs
        plain = {k: v for k, v in FOG.items() if k != "sky_distance"}
        got = _process(e, fog_desc(**plain), img, z, M, P)
        through = ~(z > 0) | (z >= R.FLT_MAX)
        assert np.array_equal(_bits(got[through]), _bits(img[through])), (w, h)
        fogged = ~through & (z > 1e-3)   # (an optical depth below half an ulp of 1 leaves the factors 0)
        assert not fogged.any() or not np.array_equal(_bits(got[fogged]), _bits(img[fogged])), (w, h)
        # a = 1 and g = 1 (d >> 1 / density): the fog colour's bits, alpha 1, wherever there is a distance
        got = _process(e, fog_desc(FogFalloff.EXPONENTIAL, color=(0.5, 0.25, 2.0, 1.0), density=1e6, sky_distance=1.0), img, z, M, P)
        hit = (z > 1e-3)
        assert np.array_equal(_bits(got[hit]), _bits(np.broadcast_to(np.array([0.5, 0.25, 2.0, 1.0], np.float32), got[hit].shape))), (w, h)
        # the two builds give the same bits
        d = fog_desc(**FOG)
        assert_bits_equal(_process(other, d, img, z, M, P), _process(e, d, img, z, M, P), f"{w}x{h}: fast against exact")
    # along the scan line through the optical axis of a level camera dy is 0 for every pixel: g does not decrease with D (black under white fog: out = g)
    w, h = 64, 9
    black = np.zeros((h, w, 4), np.float32); black[..., 3] = 1.0
    z = np.broadcast_to(np.geomspace(0.05, 400.0, w).astype(np.float32), (h, w)).copy()
    for f in range(4):
        for hf in (0.0, 0.2):
            kw = dict(K.FALLOFF[f]); kw.update(color=(1.0, 1.0, 1.0, 1.0), height_falloff=hf, height_reference=1.0)
            got = _process(e, fog_desc(**kw), black, z, K.transform(position=(0.0, 3.0, 0.0)), K.projection(w, h))
            g = got[4, :, :3]
            assert (np.diff(g, axis=0) >= 0).all() and g[-1].max() > g[0].max(), (f, hf)
    e.close(); other.close()


# ---------------------------------------------------------------- 3. whole frames
FRAME_CASES = [("cornell_fast", False, "cornell"), ("cornell_exact", True, "cornell"), ("dungeon_fast", False, "dungeon"), ("dungeon_exact", True, "dungeon")]


@pytest.mark.parametrize("case", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_a_fogged_frame_equals_the_restatement_of_the_frame_without(case):
    name, exact, scene = case
    d = fog_desc(**FOG)
    a, b = _engine(exact, scene), _engine(exact, scene)
    cam = _scene_camera(scene, SIZE)
    ca, cb = a.create_camera(cam), b.create_camera(cam)
    b.set_fog(cb, d)
    assert b.get_fog(cb)[1]
    oa, ob, depth = Out(0), Out(0, fill=0x5a), Depth()
    stream = torch.cuda.current_stream().cuda_stream
    changed = False
    for k in range(3):
        for e, c, o in ((a, ca, oa), (b, cb, ob)):
            e.tick(stream); e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        plain, got = oa.get(), ob.get()
        ref = _restate(d, plain, depth.read(b, cb, SIZE), _xf(cam), _proj(cam))
        changed |= not np.array_equal(_bits(ref), _bits(plain))
        _check(got, ref, 0, f"{name} frame {k}")
        launches = b.last_launches()
        assert launches[-1] == PassBit.POST and sum(1 for x in launches if x & PassBit.POST) == 1, [hex(x) for x in launches]
    assert changed, "fog should change some pixel"
    a.close(); b.close()


@pytest.mark.parametrize("exact,scene", [(False, "dungeon"), (True, "cornell")])
def test_the_whole_chain_equals_the_five_process_calls(exact, scene):
    """fog, depth of field, motion blur, bloom, ACES and FXAA (with a resample) in one frame against st_fog_process, st_dof_process,
    st_motion_blur_process, st_bloom_process and st_post_process over the plain frame's colour, the velocity map and the G-buffer depth"""
    a, b = _engine(exact, scene), _engine(exact, scene)
    ca, cb = a.create_camera(_moving(scene, 0)), b.create_camera(_moving(scene, 0))
    fd = fog_desc(**FOG)
    dd = dof_desc(samples=32, autofocus=(0.5, 0.5), sensor_height=0.5, focal_distance=3.0)
    md, bd = motion_blur_desc(shutter=1.0, samples=8), bloom_desc(intensity=0.3, threshold=0.4, threshold_softness=0.5)
    disp = display_desc(tonemap=Tonemap.ACES_FITTED, exposure_ev=0.5)
    post = post_desc(fxaa=True, output_size=(108, 78), filter=ResampleFilter.CATMULL_ROM)
    b.set_fog(cb, fd); b.set_dof(cb, dd); b.set_motion_blur(cb, md); b.set_bloom(cb, bd); b.set_display(cb, disp); b.set_post(cb, post)
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
        s0, s1, s2, s3, want = Out(0), Out(0), Out(0), Out(0), Out(2, (108, 78), fill=0xa5)
        cam = _moving(scene, k)
        b.fog_process(fd, _xf(cam), _proj(cam), oa.ptr(), tz.data_ptr(), w, h, s0.ptr(), 0, stream=stream)
        b.dof_process(dd, _proj(cam), s0.ptr(), tz.data_ptr(), w, h, s1.ptr(), 0, stream=stream)
        b.motion_blur_process(md, s1.ptr(), tv.data_ptr(), tz.data_ptr(), w, h, s2.ptr(), 0, stream=stream)
        b.bloom_process(bd, s2.ptr(), w, h, s3.ptr(), 0, display=disp, stream=stream)
        b.post_process(post, s3.ptr(), w, h, want.ptr(), 2, stream=stream)
        torch.cuda.synchronize()
        assert not np.array_equal(_bits(s0.get()), _bits(oa.get())) and not np.array_equal(_bits(s1.get()), _bits(s0.get()))
        assert np.array_equal(ob.get(), want.get()), (exact, scene, k, np.abs(ob.get().astype(int) - want.get().astype(int)).max())
        launches = b.last_launches()
        assert launches[-1] == PassBit.POST and sum(1 for x in launches if x & PassBit.POST) == 2, [hex(x) for x in launches]   # the two pack launches, then the rest
    a.close(); b.close()


def _sun_direction(sun):
    """World::sun_dir in float32; the library's own sine and cosine may differ from numpy's in the last bit"""
    sa, ca, sz, cz = np.sin(F(sun.altitude)), np.cos(F(sun.altitude)), np.sin(F(sun.azimuth)), np.cos(F(sun.azimuth))
    return np.array([ca * sz, sa, -(ca * cz)], np.float32)


def _matches_some_rounding(got, plain, z, cam, d, sun):
    """`got` is the restatement under `sun` with each component at most one ulp away"""
    for dx in (0, -1, 1):
        for dy in (0, -1, 1):
            for dz in (0, -1, 1):
                s = sun.copy()
                for i, step in enumerate((dx, dy, dz)):
                    if step:
                        s[i] = np.nextafter(s[i], F(np.inf) * step)
                if np.array_equal(_bits(_restate(d, plain, z, _xf(cam), _proj(cam), sun=s)), _bits(got)):
                    return True
    return False


def test_follow_sun_takes_the_direction_of_the_last_tick():
    first, second = Sun(azimuth=0.6, altitude=0.5), Sun(azimuth=0.0, altitude=0.0)   # the second: (0, 0, -1) exactly
    d = fog_desc(**dict(FOG, follow_sun=True, light_direction=(0.0, 0.0, 0.0)))
    a, b = _engine(False, "dungeon"), _engine(False, "dungeon")
    cam = _scene_camera("dungeon", SIZE)
    ca, cb = a.create_camera(cam), b.create_camera(cam)
    b.set_fog(cb, d)
    oa, ob, depth = Out(0), Out(0), Depth()
    stream = torch.cuda.current_stream().cuda_stream

    def frame(tick):
        for e, c, o in ((a, ca, oa), (b, cb, ob)):
            if tick:
                e.tick(stream)
            e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        return oa.get(), ob.get(), depth.read(b, cb, SIZE)

    frame(True)
    plain, got, z = frame(True)      # (a static camera: from the second frame on both G-buffers hold these depths)
    assert _matches_some_rounding(got, plain, z, cam, d, _sun_direction(first))
    for e in (a, b):
        e.update_sun(second)
    plain, got, z = frame(False)     # not before the next tick
    assert _matches_some_rounding(got, plain, z, cam, d, _sun_direction(first))
    assert not np.array_equal(_bits(_restate(d, plain, z, _xf(cam), _proj(cam), sun=np.array([0, 0, -1], np.float32))), _bits(got))
    plain, got, z = frame(True)      # after it
    _check(got, _restate(d, plain, z, _xf(cam), _proj(cam), sun=np.array([0, 0, -1], np.float32)), 0, "the sun of the last tick")
    a.close(); b.close()


# ---------------------------------------------------------------- 4. off is off; nothing else changes
@pytest.mark.parametrize("exact", [False, True])
def test_a_cleared_setting_renders_like_a_camera_that_never_had_one(exact):
    C.cleared_setting_renders_like_none(NODE, exact)


def test_aovs_picks_planes_and_the_exposure_do_not_depend_on_the_setting():
    C.nothing_else_depends_on_the_setting(NODE)


# ---------------------------------------------------------------- 5. the frames that skip it
@pytest.mark.parametrize("what", ["reference", "heatmap", "orthographic"])
def test_frames_that_skip_fog(what):
    C.frames_that_skip(NODE, what, (64, 48))


# ---------------------------------------------------------------- 6. tiles
def _tiles(world, scene, fog, disp, size, group, frames=3):
    """`world` engines on one device render their windows and st_dist_gather assembles them on rank 0: (the gathered frame, rank r's
    G-buffer depth inside its own tile assembled into one plane)"""
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
        if r % 2 == 0 and fog is not None:
            e.set_fog(c, fog)                       # fog, then the tile
        e.dist_init_local(r, world, group)
        owned, window = e.dist_set_partition(c, apron=0)
        if r % 2 == 1 and fog is not None:
            e.set_fog(c, fog)                       # the tile, then fog
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
    z = np.zeros((size[1], size[0]), np.float32)
    for e, c, out, (x0, y0, x1, y1) in ranks:
        g = e.read_buffer(c, Buffer.PRIM_GBUFFER_D0_A).reshape(size[1], size[0], 4)[..., 0]   # a static camera: either parity
        z[y0:y1, x0:x1] = R.frame_depth(g)[y0:y1, x0:x1]
        # only the pixels inside the window are written
        o = out.cpu().numpy()
        outside = np.ones((size[1], size[0]), bool); outside[y0:y1, x0:x1] = False
        assert (o[outside] == 7.0).all(), "a rank wrote outside its window"
    got = full.cpu().numpy()
    for e, *_ in ranks:
        e.dist_shutdown(); e.close()
    return got, z


@pytest.mark.parametrize("world", [2, 4])
def test_fogged_tiles_gather_to_the_fogged_frame(world):
    """Cornell 64 x 48, fog and a manual ACES display, as 2 and 4 windows gathered on one device. An Image frame's resampling and denoiser
    taps cross tile borders, so a composed Image frame gathered from tiles is not the single engine's at any commit, with or without fog
    (tests/test_gpu_deform_motion.py says so too; the existing tile tests compare Reference frames, which skip fog). What fog adds is per
    pixel, and that is held bit for bit: the gathered fogged tiles are st_fog_process, with the whole frame's camera, over the gathered
    tiles rendered without fog and the tiles' own depths — which also needs every pixel's ray taken at its absolute coordinates. A frame
    without geometry has no such taps: there the gathered fogged tiles are the single engine's fogged frame bit for bit."""
    size = (64, 48)
    d = fog_desc(**FOG)
    disp = display_desc(Tonemap.ACES_FITTED, exposure_ev=1.25)
    cam = scenes.cornell_camera(size)
    plain, z = _tiles(world, True, None, None, size, 7600 + world)
    got, z2 = _tiles(world, True, d, disp, size, 7610 + world)
    assert np.array_equal(_bits(z), _bits(z2))
    one = Engine(device=0, exact=True)
    want = _process(one, d, plain, z, _xf(cam), _proj(cam), 0, disp)
    assert_bits_equal(got, want, f"{world} fogged tiles against st_fog_process over the gathered plain tiles")
    assert not np.array_equal(_bits(got), _bits(plain))
    # sky only: the single engine's fogged frame, literally
    sky, _ = _tiles(world, False, d, disp, size, 7620 + world)
    one.set_blue_noise(scenes.load_blue_noise()); one.set_seed(7)
    c = one.create_camera(cam)
    one.set_fog(c, d); one.set_display(c, disp)
    single = Out(0, size)
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        one.tick(stream); one.render_camera(c, single.ptr(), stream)
    torch.cuda.synchronize()
    assert_bits_equal(sky, single.get(), f"{world} fogged sky tiles against one engine")
    rows = single.get()[:, 0, :3]
    assert not np.array_equal(rows[0], rows[-1]), "the fogged sky depends on the ray's height"
    one.close()


# ---------------------------------------------------------------- 7. pipelining
def test_frames_in_flight_read_their_own_depths():
    C.frames_in_flight_read_their_own_inputs(NODE)


# ---------------------------------------------------------------- 8. lifecycle
def test_resizes_toggles_arithmetic_switches_tiny_frames_and_teardown():
    a, b = _engine(False), _engine(False)
    d = fog_desc(**FOG)
    stream = torch.cuda.current_stream().cuda_stream
    ca, cb = a.create_camera(scenes.cornell_camera(SIZE)), b.create_camera(scenes.cornell_camera(SIZE))
    b.set_fog(cb, d)
    step = 0
    for size in (SIZE, (96, 80), (8, 8), (1, 1), SIZE):   # larger, tiny, back: the setting and the results stay
        if size == SIZE and step:
            for e in (a, b):
                e.set_exact(True); e.set_exact(False)   # ... and across an arithmetic switch
        cam = scenes.cornell_camera(size)
        for e, c in ((a, ca), (b, cb)):
            e.update_camera(c, cam)
        p = Depth()
        for rep_ in range(2):
            if rep_ == 1 and size == (96, 80):
                b.set_fog(cb, None); b.set_fog(cb, d)   # a toggle between two frames
            oa, ob = Out(0, size), Out(0, size)
            a.tick(stream); b.tick(stream)
            a.render_camera(ca, oa.ptr(), stream); b.render_camera(cb, ob.ptr(), stream)
            torch.cuda.synchronize()
            assert b.get_fog(cb)[1] and b.get_fog(cb)[0].density == F(FOG["density"])
            _check(ob.get(), _restate(d, oa.get(), p.read(b, cb, size), _xf(cam), _proj(cam)), 0, f"size {size} step {step}")
            step += 1
    # delete a camera with the setting on and a frame in flight; a new camera starts clean; destroy the engine with a fogged frame in flight
    C.teardown_with_the_setting_on(NODE, b, cb)
    a.close(); b.close()
