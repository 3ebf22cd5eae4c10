"""GPU tests of depth of field (include/strolle_hip.h "depth of field"; k_dof.hip, st_dof.cpp): st_dof_process on synthetic inputs against
the numpy restatement (dof_ref.py) bit for bit in both builds; properties that do not rest on the restatement; whole frames with depth of
field on against the restatement fed the same frame rendered without it and the G-buffer depth read back; the whole output chain against
the four process calls; off is off; nothing else changes; the frames that skip it; pipelining across frames; lifecycle. Every test builds
its own engines and uses entry points the parent commit does not have.

Sizes: the tile is 32 x 32, the workgroup 32 x 8 and the radius at most 32, so 72 x 52 (neither a tile nor a workgroup multiple, 3 x 2
tiles with partial ones), 33 x 21 (a second tile one pixel wide), 32 x 32 (exactly one tile) and 5 x 5 (one partial tile, where every tap
clamps)."""
import numpy as np
import pytest
import torch

import display_ref
import dof_ref as R
import output_chain as C
from output_chain import Depth, Out, _bits, _check, _engine, _image, _moving, _proj, _scene_camera
from strolle_amd import (Buffer, Engine, OutputFormat, PassBit, ResampleFilter, Tonemap, bloom_desc, display_desc, dof_desc,
                         dof_plan, motion_blur_desc, post_desc, scenes)

pytestmark = pytest.mark.gpu
SIZE = (72, 52)
SIZES = [(72, 52), (33, 21), (32, 32), (5, 5)]
F = np.float32
nan, inf = float("nan"), float("inf")


def _ref(key, make):
    return C._ref(__name__, key, make)


def _projection(w, h):
    return _proj(scenes.cornell_camera((w, h)))   # 45 degrees: P[5] = 2.414


# A lens that blurs at these sizes: a 0.5 m sensor at f/1 focused at 3 m. At 45 degrees f = 0.60 m, and at H = 52 K = 18.9 px m, A = 7.9 px.
LENS = dict(focal_distance=3.0, sensor_height=0.5, aperture_f_stops=1.0)
AUTO = dict(samples=32, autofocus=(0.5, 0.5), sensor_height=0.5, focal_distance=3.0)
NODE = C.Node("set_dof", "get_dof", "depth of field", "the focused frame differs", ("dof_pack", "dof_neighbour", "dof_gather"), AUTO,
              cleared=dict(samples=4, **LENS), skipped=dict(samples=4, autofocus=(0.5, 0.5), **LENS), recreated=LENS)


# ---------------------------------------------------------------- synthetic inputs
def _depth(kind, w, h, seed=6):
    """distances along the rays"""
    rng = np.random.default_rng(seed)
    if kind == "focus":      # everything on the focal plane, to within what the planar factor rounds (|coc| far below 0.5)
        x, y = np.meshgrid(np.arange(w), np.arange(h))
        P = _projection(w, h)
        ax, ay = ((x + 0.5) * 2 / w - 1) / P[0], ((y + 0.5) * 2 / h - 1) / P[5]
        return (3.0 * np.sqrt(ax * ax + ay * ay + 1)).astype(np.float32)
    if kind == "edge":       # near on the left, far on the right
        d = np.full((h, w), 1.2, np.float32); d[:, w // 2:] = 12.0
        return d
    if kind == "ramp":       # through the focal plane
        return np.broadcast_to(np.linspace(1.0, 9.0, w, dtype=np.float32), (h, w)).copy()
    if kind == "sky":        # FLT_MAX beside geometry at the focal distance and in front of it
        d = np.full((h, w), 3.1, np.float32); d[: h // 2, w // 3:] = R.FLT_MAX; d[h // 2:, : w // 4] = 1.5
        return d
    if kind == "corner":     # one near-field pixel in the corner of a tile inside an in-focus frame: the neighbour maximum crosses a tile corner
        d = _depth("focus", w, h)
        d[min(31, h - 1), min(31, w - 1)] = 0.9
        return d
    by, bx = (h + 7) // 8, (w + 7) // 8   # "blocks": three layers in 8 x 8 blocks with noise, sky, and depths no frame holds
    z = rng.choice(np.array([1.1, 3.0, 20.0], np.float32), (by, bx))
    z[rng.random((by, bx)) < 0.15] = R.FLT_MAX
    z = np.repeat(np.repeat(z, 8, 0), 8, 1)[:h, :w].copy()
    z = np.where(z == R.FLT_MAX, z, z * (1.0 + 0.01 * rng.random((h, w)))).astype(np.float32)
    n = max(1, w * h // 200)
    for v in (nan, inf, -inf, 0.0, -2.0, 1e-30):
        z[rng.integers(0, h, n), rng.integers(0, w, n)] = v
    return z


KINDS = ("focus", "edge", "ramp", "sky", "corner", "blocks")


def _process(e, d, color, depth, proj, fmt=0, display=None, stream=None):
    h, w = color.shape[:2]
    tc, tz = torch.from_numpy(color).cuda(), torch.from_numpy(depth).cuda()
    out = Out(fmt, (w, h), fill=0x5a)
    e.dof_process(d, proj, tc.data_ptr(), tz.data_ptr(), w, h, out.ptr(), fmt, display=display,
                  stream=stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.get()


def _restate(d, color, depth, proj, display=None, scale=None, details=None):
    h, w = color.shape[:2]
    n, _, taps = dof_plan(d, w, h)
    with np.errstate(all="ignore"):
        c = R.dof_desc(color, depth, proj, taps, d, details)
    if display is None:
        return c
    return display_ref.transform(c[..., :3], int(display), scale)


# ---------------------------------------------------------------- 1. bit for bit against the restatement
DESCS = [dict(samples=4, max_radius=4.0, **LENS), dict(samples=32, max_radius=0.0, **LENS), dict(samples=64, max_radius=32.0, focal_distance=3.0, sensor_height=0.5, aperture_f_stops=0.25),
         dict(samples=0, max_radius=4.0, autofocus=(0.3, 0.6), **LENS), dict(samples=4, autofocus=(0.99, 0.01), **LENS), dict(samples=32, planar_depth=True, **LENS),
         dict(samples=4, planar_depth=True, autofocus=(0.5, 0.5), max_radius=4.0, **LENS)]


@pytest.mark.parametrize("exact", [True, False])
def test_process_matches_the_restatement_on_synthetic_inputs(exact):
    e = Engine(device=0, exact=exact)
    blurred = focused_on_sky = focused_on_hit = False
    for (w, h) in SIZES:
        img, proj = _image(w, h), _projection(w, h)
        for kind in KINDS:
            z = _depth(kind, w, h)
            for i, kw in enumerate(DESCS):
                if (w, h) != SIZE and i in (1, 2) and kind not in ("ramp", "corner"):
                    continue   # the long tap counts on every field at the full size, on two fields at the others
                d = dof_desc(**kw)
                det = {}
                want = _ref((w, h, kind, i), lambda: (_restate(d, img, z, proj, details=det), det.get("s")))
                got = _process(e, d, img, z, proj)
                _check(got, want[0], 0, f"{w}x{h} exact={exact} depth={kind} desc={kw}")
                blurred |= kind != "focus" and not np.array_equal(_bits(got), _bits(img))
                if "autofocus" in kw:
                    focused_on_sky |= kind == "sky" and want[1] == F(3.0)
                    focused_on_hit |= want[1] != F(3.0)
    assert blurred and focused_on_sky and focused_on_hit, (blurred, focused_on_sky, focused_on_hit)
    # the four output formats, with and without a manual display of each operator
    w, h = SIZE
    img, z, proj = _image(w, h), _depth("blocks", w, h), _projection(w, h)
    d = dof_desc(samples=32, **LENS)
    for op in (None,) + tuple(Tonemap):
        disp = display_desc(tonemap=op, exposure_ev=-1.5) if op is not None else None
        want = _ref(("fmt", op), lambda: _restate(d, img, z, proj, op, display_ref.manual_scale(-1.5) if op is not None else None))
        for fmt in range(4):
            _check(_process(e, d, img, z, proj, fmt, disp), want, fmt, f"exact={exact} {op} fmt={fmt}")
    # a projection with a lens shift and a mirrored x axis
    shifted = proj.copy(); shifted[0] = -shifted[0]; shifted[8] = 0.2; shifted[9] = -0.1
    _check(_process(e, d, img, z, shifted), _ref("shifted", lambda: _restate(d, img, z, shifted)), 0, f"exact={exact} shifted projection")
    e.close()


# ---------------------------------------------------------------- 2. properties that do not rest on the restatement
@pytest.mark.parametrize("exact", [True, False])
def test_properties_of_the_filter(exact):
    e = Engine(device=0, exact=exact)
    w, h = SIZE
    proj = _projection(w, h)
    # an all-in-focus frame returns the input's own bits, NaN and alpha included
    for (sw, sh) in SIZES:
        img = _image(sw, sh)
        for kw in (dict(samples=32, **LENS), dict(samples=4, planar_depth=True, **LENS)):
            z = np.full((sh, sw), 3.0, np.float32) if "planar_depth" in kw else _depth("focus", sw, sh)
            got = _process(e, dof_desc(**kw), img, z, _projection(sw, sh))
            assert np.array_equal(_bits(got), _bits(img)), (sw, sh, kw)
    # a constant colour of 1.0 or 0.5 under any depth field stays exactly constant: sum = v wsum at every step, with the same roundings
    for v in (1.0, 0.5):
        flat = np.full((h, w, 4), v, np.float32); flat[..., 3] = 1.0
        for kind in KINDS:
            for samples in (4, 64):
                got = _process(e, dof_desc(samples=samples, **LENS), flat, _depth(kind, w, h), proj)
                assert np.array_equal(_bits(got), _bits(flat)), (v, kind, samples)
    # an in-focus pixel in front of a blurred background keeps its own bits
    img = _image(w, h, seed=8)
    zz = np.full((h, w), 40.0, np.float32)
    zz[10:40, 20:50] = 3.0
    d = dof_desc(samples=32, planar_depth=True, **LENS)
    got = _process(e, d, img, zz, proj)
    assert np.array_equal(_bits(got[10:40, 20:50]), _bits(img[10:40, 20:50]))
    assert not np.array_equal(_bits(got[:10]), _bits(img[:10])), "the background is blurred"
    # pixels beside a near-field blob change, pixels farther from it than its radius (here |coc| = R = 6) and a texel's diagonal do not
    ww, hh = 96, 40
    img = np.full((hh, ww, 4), 0.25, np.float32); img[..., 3] = 1.0
    zz = np.full((hh, ww), 3.0, np.float32)
    zz[18:22, 30:34] = 0.7
    img[18:22, 30:34, :3] = 50.0
    got = _process(e, dof_desc(samples=64, planar_depth=True, max_radius=6.0, **LENS), img, zz, _projection(ww, hh))
    changed = (_bits(got) != _bits(img)).any(-1)
    ys, xs = np.nonzero(changed)
    ring = int(changed[17:23, 29:35].sum()) - int(changed[18:22, 30:34].sum())   # the 20 pixels that touch the blob
    assert ring >= 10, ring
    dist = np.maximum(np.maximum(30 - xs, xs - 33), 0) ** 2 + np.maximum(np.maximum(18 - ys, ys - 21), 0) ** 2
    assert (np.sqrt(dist) <= 6.0 + 0.5 + np.sqrt(2.0)).all(), np.sqrt(dist).max()
    assert np.array_equal(_bits(got[:, 64:]), _bits(img[:, 64:]))   # (gathered with r_g = 6 too, the blob's tile is next door, but every weight is 0)
    e.close()


# ---------------------------------------------------------------- 3. whole frames
CORNELL, DUNGEON = (64, 48), (72, 48)
FRAME_CASES = [
    # name, exact, scene, size, keep all planes, lens
    ("cornell_fused_lean", False, "cornell", CORNELL, False, dict(samples=32, **LENS)),
    ("cornell_fused_all_planes_autofocus", False, "cornell", CORNELL, True, dict(samples=4, autofocus=(0.5, 0.5), sensor_height=0.5, focal_distance=10.0)),
    ("cornell_exact_autofocus", True, "cornell", CORNELL, False, dict(samples=32, autofocus=(0.5, 0.5), sensor_height=0.5, focal_distance=10.0)),
    ("dungeon_fused_lean_autofocus", False, "dungeon", DUNGEON, False, dict(samples=64, autofocus=(0.5, 0.5), sensor_height=0.5, focal_distance=10.0)),
    ("dungeon_exact", True, "dungeon", DUNGEON, False, dict(samples=32, max_radius=8.0, focal_distance=1.0, sensor_height=0.5)),
]


@pytest.mark.parametrize("case", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_a_focused_frame_equals_the_restatement_of_the_frame_without(case):
    name, exact, scene, size, keep, lens = case
    d = dof_desc(**lens)
    a, b = _engine(exact, scene), _engine(exact, scene)
    for e in (a, b):
        e.keep_all_planes(keep)
    cam = _scene_camera(scene, size)
    ca, cb = a.create_camera(cam), b.create_camera(cam)
    b.set_dof(cb, d)
    assert b.get_dof(cb)[1]
    oa, ob, depth = Out(0, size), Out(0, size, fill=0x5a), Depth()
    stream = torch.cuda.current_stream().cuda_stream
    changed = False
    for k in range(3):
        for e, c, o in ((a, ca, oa), (b, cb, ob)):
            e.tick(stream); e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        plain, got = oa.get(), ob.get()
        z = depth.read(b, cb, size)
        det = {}
        ref = _restate(d, plain, z, _proj(cam), details=det)
        print(f"{name} frame {k}: s = {det['s']:.3f} m, A = {det['A']:.2f} px, |coc| max {np.abs(det['coc']).max():.2f}, {(np.abs(det['coc']) >= 0.5).mean():.3f} of the pixels blurred, "
              f"near-field tiles {int((det['tiles'] > 0).sum())}")
        if "autofocus" in lens:
            assert det["s"] != F(lens["focal_distance"]), "the centre of these frames is geometry"
        changed |= not np.array_equal(_bits(ref), _bits(plain))
        _check(got, ref, 0, f"{name} frame {k}")
        launches = b.last_launches()
        assert launches[-1] == PassBit.POST and sum(1 for x in launches if x & PassBit.POST) == 2, [hex(x) for x in launches]   # the pack launch, then the rest
    assert changed, "depth of field should change some pixel"
    a.close(); b.close()


# ---------------------------------------------------------------- 4. the chain
@pytest.mark.parametrize("exact,scene", [(False, "dungeon"), (True, "cornell")])
def test_the_whole_chain_equals_the_four_process_calls(exact, scene):
    """depth of field, motion blur, bloom, ACES and FXAA (with a resample) in one frame against st_dof_process, st_motion_blur_process,
    st_bloom_process and st_post_process over the plain frame's colour, the velocity map and the G-buffer depth"""
    a, b = _engine(exact, scene), _engine(exact, scene)
    ca, cb = a.create_camera(_moving(scene, 0)), b.create_camera(_moving(scene, 0))
    dd = dof_desc(samples=32, autofocus=(0.5, 0.5), sensor_height=0.5, focal_distance=3.0)
    md, bd = motion_blur_desc(shutter=1.0, samples=8), bloom_desc(intensity=0.3, threshold=0.4, threshold_softness=0.5)
    disp = display_desc(tonemap=Tonemap.ACES_FITTED, exposure_ev=0.5)
    post = post_desc(fxaa=True, output_size=(108, 78), filter=ResampleFilter.CATMULL_ROM)
    b.set_dof(cb, dd); b.set_motion_blur(cb, md); b.set_bloom(cb, bd); b.set_display(cb, disp); b.set_post(cb, post)
    b.set_output_format(cb, OutputFormat.RGBA8_UNORM_SRGB)
    oa, ob, depth = Out(0), Out(2, (108, 78), fill=0x5a), Depth()
    stream = torch.cuda.current_stream().cuda_stream
    w, h = SIZE
    for k in range(3):
        for e, c, o in ((a, ca, oa), (b, cb, ob)):
            e.update_camera(c, _moving(scene, k)); e.tick(stream); e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        z = depth.read(b, cb, SIZE)
        assert not b.buffer_stale(cb, Buffer.VELOCITY_MAP)
        v = b.read_buffer(cb, Buffer.VELOCITY_MAP).reshape(h, w, 4)[..., :2].copy()
        if k == 0:
            continue   # (the first frame has no previous camera)
        tz, tv = torch.from_numpy(z).cuda(), torch.from_numpy(v).cuda()
        s1, s2, s3, want = Out(0), Out(0), Out(0), Out(2, (108, 78), fill=0xa5)
        b.dof_process(dd, _proj(_moving(scene, k)), oa.ptr(), tz.data_ptr(), w, h, s1.ptr(), 0, stream=stream)
        b.motion_blur_process(md, s1.ptr(), tv.data_ptr(), tz.data_ptr(), w, h, s2.ptr(), 0, stream=stream)
        b.bloom_process(bd, s2.ptr(), w, h, s3.ptr(), 0, display=disp, stream=stream)
        b.post_process(post, s3.ptr(), w, h, want.ptr(), 2, stream=stream)
        torch.cuda.synchronize()
        assert not np.array_equal(_bits(s1.get()), _bits(oa.get())) and not np.array_equal(_bits(s2.get()), _bits(s1.get()))
        assert np.array_equal(ob.get(), want.get()), (exact, scene, k, np.abs(ob.get().astype(int) - want.get().astype(int)).max())
        launches = b.last_launches()
        assert launches[-1] == PassBit.POST and sum(1 for x in launches if x & PassBit.POST) == 2, [hex(x) for x in launches]
    a.close(); b.close()


# ---------------------------------------------------------------- 5. off is off; nothing else changes
@pytest.mark.parametrize("exact", [False, True])
def test_a_cleared_setting_renders_like_a_camera_that_never_had_one(exact):
    C.cleared_setting_renders_like_none(NODE, exact)


def test_aovs_picks_planes_and_the_exposure_do_not_depend_on_the_setting():
    C.nothing_else_depends_on_the_setting(NODE)


@pytest.mark.parametrize("what", ["reference", "heatmap", "orthographic"])
def test_frames_that_skip_depth_of_field(what):
    C.frames_that_skip(NODE, what, CORNELL)


# ---------------------------------------------------------------- 6. pipelining
def test_frames_in_flight_read_their_own_depths():
    C.frames_in_flight_read_their_own_inputs(NODE)


# ---------------------------------------------------------------- 7. lifecycle
def test_resizes_toggles_arithmetic_switches_two_cameras_and_teardown():
    a, b = _engine(False), _engine(False)
    d1, d2 = dof_desc(samples=32, **LENS), dof_desc(samples=4, max_radius=8.0, autofocus=(0.4, 0.6), sensor_height=0.5, focal_distance=2.0)
    stream = torch.cuda.current_stream().cuda_stream
    ca, cb, cb2 = (e.create_camera(scenes.cornell_camera(SIZE)) for e in (a, b, b))
    b.set_dof(cb, d1); b.set_dof(cb2, d2)
    step = 0
    for size in (SIZE, (96, 80), (40, 24), SIZE):   # larger, smaller, back: the setting and the results stay
        if size == SIZE and step:
            for e in (a, b):
                e.set_exact(True); e.set_exact(False)   # ... and across an arithmetic switch
        cam = scenes.cornell_camera(size)
        for e, c in ((a, ca), (b, cb), (b, cb2)):
            e.update_camera(c, cam)
        p1, p2 = Depth(), Depth()
        for rep_ in range(2):
            if rep_ == 1 and size == (96, 80):
                b.set_dof(cb, None); b.set_dof(cb, d1)   # a toggle between two frames
            oa, ob, ob2 = Out(0, size), Out(0, size), Out(0, size)
            a.tick(stream); b.tick(stream)
            a.render_camera(ca, oa.ptr(), stream); b.render_camera(cb, ob.ptr(), stream); b.render_camera(cb2, ob2.ptr(), stream)
            torch.cuda.synchronize()
            assert b.get_dof(cb)[1] and b.get_dof(cb2)[0].samples == 4
            plain = oa.get()
            for c, o, d, p in ((cb, ob, d1, p1), (cb2, ob2, d2, p2)):
                ref = _restate(d, plain, p.read(b, c, size), _proj(cam))
                _check(o.get(), ref, 0, f"size {size} step {step} samples {d.samples}")
            step += 1
    # process calls on two streams share the engine's planes: the engine orders them
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    ia, ib = _image(72, 52), _image(33, 21, seed=2)
    za, zb, pa, pb = _depth("blocks", 72, 52), _depth("ramp", 33, 21), _projection(72, 52), _projection(33, 21)
    t = [torch.from_numpy(x).cuda() for x in (ia, za, ib, zb)]
    oa, ob = Out(0, (72, 52)), Out(0, (33, 21))
    torch.cuda.synchronize()
    for _ in range(4):
        b.dof_process(d1, pa, t[0].data_ptr(), t[1].data_ptr(), 72, 52, oa.ptr(), 0, stream=sa.cuda_stream)
        b.dof_process(d2, pb, t[2].data_ptr(), t[3].data_ptr(), 33, 21, ob.ptr(), 0, stream=sb.cuda_stream)
    torch.cuda.synchronize()
    _check(oa.get(), _restate(d1, ia, za, pa), 0, "stream a")
    _check(ob.get(), _restate(d2, ib, zb, pb), 0, "stream b")
    # delete a camera with the setting on and a frame in flight; a new camera starts clean; destroy the engine with a focused frame in flight
    b.update_camera(cb, scenes.cornell_camera(SIZE))
    C.teardown_with_the_setting_on(NODE, b, cb)
    a.close(); b.close()
