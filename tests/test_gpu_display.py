"""GPU tests of camera display transforms (include/strolle_hip.h "display transforms"; st_passes.h display_transform, k_display.hip): a
cleared display is today's output; every operator against the numpy restatement (display_ref.py) of the same engine's HDR frame; the
metering histogram, metered EV and one frame of lag; a known answer under a uniform environment map; the adaptation's steps; scheduling
switches, streams and determinism; tiles; lifecycle. Every test builds its own engines."""
import math

import numpy as np
import pytest
import torch

import display_ref as R
from output_chain import Out as _Out, _engine, _frame
from parity import assert_bits_equal
from strolle_amd import CameraMode, OutputFormat, Tonemap, display_desc, scenes

pytestmark = pytest.mark.gpu
SIZE = (64, 48)
AWAY = ((0.0, 1.0, 3.2), (0.0, 1.0, 10.0))   # from the Cornell camera's eye, looking away from the box: every pixel is sky
MODES = [("image_denoise", CameraMode.IMAGE, True, 0), ("image", CameraMode.IMAGE, False, 0), ("di_diffuse", CameraMode.DI_DIFFUSE, True, 0),
         ("reference", CameraMode.REFERENCE, False, 1)]


def _camera(scene, mode=CameraMode.IMAGE, denoise=True, depth=0, size=SIZE):
    return (scenes.cornell_camera if scene == "cornell" else scenes.dungeon_camera)(size, mode, denoise=denoise, depth=depth)


def Out(fmt, size=SIZE):
    return _Out(fmt, size)


def _check(got, hdr, op, s, fmt, exact, what):
    """`got` (the display engine's output in format `fmt`) against display_ref of the same frame's HDR colour"""
    ref = R.transform(hdr, op, s)
    if fmt == 0:
        if exact:
            assert_bits_equal(got, ref, what)
        else:
            ok = np.isclose(got, ref, rtol=1e-6, atol=1e-7, equal_nan=True)
            assert ok.all(), f"{what}: {np.count_nonzero(~ok)} channels beyond 1e-6"
    elif fmt == 1:
        ref16 = ref.astype(np.float16)
        if exact:
            assert np.array_equal(got.view(np.uint16), ref16.view(np.uint16)), what
        else:
            ok = np.isclose(got.astype(np.float32), ref16.astype(np.float32), rtol=2e-3, atol=1e-7, equal_nan=True)
            assert ok.all(), f"{what}: {np.count_nonzero(~ok)} half channels beyond one ulp"
    else:
        want = R.srgb8(ref[..., :3])
        rgb = got[..., :3].astype(np.int32) if fmt == 2 else got[..., 2::-1].astype(np.int32)
        d = np.abs(rgb - want)
        assert d.max() <= 1, f"{what}: 8-bit channel off by {d.max()}"
        assert (d == 0).mean() >= 0.999, f"{what}: only {(d == 0).mean():.5f} of the 8-bit channels exact"
        assert (got[..., 3] == 255).all(), what


# ---------------------------------------------------------------- 1. off is today
@pytest.mark.parametrize("exact", [False, True])
def test_a_cleared_display_renders_like_none(exact):
    for fmt in range(4):
        a, b = _engine(exact), _engine(exact)
        desc = _camera("cornell")
        ca, cb = a.create_camera(desc), b.create_camera(desc)
        a.set_output_format(ca, OutputFormat(fmt)); b.set_output_format(cb, OutputFormat(fmt))
        b.set_display(cb, tonemap=Tonemap.ACES_FITTED, exposure_ev=1.0, auto_exposure=True)
        oa, ob = Out(fmt), Out(fmt)
        _frame(b, cb, ob)                     # a metered frame, then off
        _frame(a, ca, oa)
        b.set_display(cb, None)
        for k in range(3):
            x, y = _frame(a, ca, oa), _frame(b, cb, ob)
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (exact, fmt, k)
        assert b.exposure(cb)[0] == 1.0 and math.isnan(b.exposure(cb)[1])
        a.close(); b.close()


# ---------------------------------------------------------------- 2. manual operators against display_ref
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("scene", ["cornell", "dungeon"])
def test_manual_operators_match_the_reference(exact, scene):
    evs = (0.0, -1.0, 1.5, 3.0)
    for name, mode, denoise, depth in MODES:
        a, b = _engine(exact, scene), _engine(exact, scene)
        desc = _camera(scene, mode, denoise, depth)
        ca, cb = a.create_camera(desc), b.create_camera(desc)
        oa = Out(0)
        outs = {f: Out(f) for f in range(4)}
        for i in range(20):   # every operator in every format, the camera's history accumulating as usual
            op, fmt, ev = i % 5, (i // 5) % 4, evs[i % 4]
            b.set_output_format(cb, OutputFormat(fmt))
            b.set_display(cb, tonemap=Tonemap(op), exposure_ev=ev)
            hdr = _frame(a, ca, oa)
            got = _frame(b, cb, outs[fmt])
            _check(got, hdr, op, R.manual_scale(ev), fmt, exact, f"{scene} {name} exact={exact} op={op} fmt={fmt} ev={ev} frame {i}")
        if scene == "dungeon" and name == "image_denoise":
            assert (hdr[..., :3] > 1.0).any(), "the sun-lit dungeon should exceed 1 somewhere"
        a.close(); b.close()


# ---------------------------------------------------------------- 3. metering
def _edge_pixels(hdr, ev_min, ev_max, tol=1e-5):
    ly = R.log2_y(hdr)
    t = (ly - ev_min) * (R.BINS / (ev_max - ev_min))
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero(np.isfinite(t) & (np.abs(t - np.round(t)) * (ev_max - ev_min) / R.BINS < tol)))


@pytest.mark.parametrize("scene", ["cornell", "dungeon"])
def test_metering_matches_numpy_with_one_frame_of_lag(scene):
    lo_ev, hi_ev, comp = -10.0, 6.0, 0.5
    a, b = _engine(True, scene), _engine(True, scene)
    desc = _camera(scene)
    ca, cb = a.create_camera(desc), b.create_camera(desc)
    b.set_display(cb, tonemap=Tonemap.ACES_FITTED, exposure_ev=comp, auto_exposure=True, ev_min=lo_ev, ev_max=hi_ev, low_fraction=0.2,
                  high_fraction=0.95, max_ev_step_up=0.25, max_ev_step_down=0.5)
    oa, ob = Out(0), Out(0)
    s = R.manual_scale(comp)                       # the first frame: adapted = log2 0.18
    adapted, primed = None, False
    for k in range(6):
        hdr = _frame(a, ca, oa)
        got = _frame(b, cb, ob)
        _check(got, hdr, R.ACES_FITTED, s, 0, True, f"{scene} frame {k} at the previous frame's scale")
        hist = b.camera_histogram(cb).astype(np.int64)
        want = R.histogram(hdr, lo_ev, hi_ev)
        assert hist.sum() == SIZE[0] * SIZE[1]
        moved = int(np.abs(hist - want).sum()) // 2
        assert moved <= _edge_pixels(hdr, lo_ev, hi_ev), f"{scene} frame {k}: {moved} pixels in other bins than numpy's"
        scale, metered, adapted_dev = b.exposure(cb)
        m = R.metered_ev(want, 0.2, 0.95, lo_ev, hi_ev)
        assert abs(metered - m) < 1e-4, (k, metered, m)
        assert metered == R.metered_ev(hist, 0.2, 0.95, lo_ev, hi_ev)
        adapted = R.adapt(adapted if primed else 0.0, metered, primed, 0.25, 0.5)
        primed = True
        assert adapted_dev == adapted, (k, adapted_dev, adapted)
        assert scale == pytest.approx(float(R.auto_scale(comp, adapted)), rel=1e-6)
        s = np.float32(scale)
    a.close(); b.close()


# ---------------------------------------------------------------- 4. known answer, 5. adaptation
def _sky_engines(L, intensity=1.0):
    m = np.ones((16, 32, 3), np.float32) * np.asarray(L, np.float32)
    es = []
    for _ in range(2):
        e = _engine(True)
        e.set_environment(m, intensity=intensity)
        es.append(e)
    desc = scenes.camera_for(SIZE, AWAY[0], AWAY[1], CameraMode.IMAGE)
    return es, m, desc


@pytest.mark.parametrize("op", list(Tonemap))
def test_known_answer_under_a_uniform_map(op):
    L = (0.7, 0.5, 0.3)
    c = np.asarray(L, np.float32) / np.float32(math.pi)   # a sky pixel composes its direct colour: the radiance over pi
    y = float(R.luma(c[0], c[1], c[2]))
    lo_ev, hi_ev, comp = -8.0, 8.0, -0.5
    t = (math.log2(y) - lo_ev) * 4
    assert 0.1 < t - math.floor(t) < 0.9, "L's luminance sits well inside its bin"
    centre = lo_ev + (math.floor(t) + 0.5) * 0.25
    (a, b), m, desc = _sky_engines(L)
    ca, cb = a.create_camera(desc), b.create_camera(desc)
    b.set_display(cb, tonemap=op, exposure_ev=comp, auto_exposure=True, ev_min=lo_ev, ev_max=hi_ev, low_fraction=0.0, high_fraction=1.0)
    oa, ob = Out(0), Out(0)
    for k in range(3):
        hdr = _frame(a, ca, oa)
        got = _frame(b, cb, ob)
        assert np.allclose(hdr[..., :3], c, rtol=1e-6), "every pixel is the map's radiance (over pi)"
        hist = b.camera_histogram(cb)
        assert hist.max() == SIZE[0] * SIZE[1] and hist.argmax() == int((centre - lo_ev) / 0.25), list(np.nonzero(hist)[0])
        scale, metered, adapted = b.exposure(cb)
        assert metered == np.float32(centre) and adapted == np.float32(centre)
        want = 0.18 * 2.0 ** (comp - centre)
        assert scale == pytest.approx(want, rel=1e-6)
        if k > 0:
            _check(got, hdr, int(op), prev, 0, True, f"op {op} frame {k}")
        prev = np.float32(scale)
    a.close(); b.close()


@pytest.mark.parametrize("step", [0.0, 0.75])
def test_adaptation_steps_towards_a_brighter_map(step):
    L, lo_ev, hi_ev = (0.2, 0.2, 0.2), -8.0, 8.0
    (b, _), m, desc = _sky_engines(L)
    _.close()
    cb = b.create_camera(desc)
    b.set_display(cb, tonemap=Tonemap.REINHARD, auto_exposure=True, ev_min=lo_ev, ev_max=hi_ev, low_fraction=0.0, high_fraction=1.0,
                  max_ev_step_up=step, max_ev_step_down=step)
    ob = Out(0)
    seq = []
    for k in range(14):
        if k == 3:
            b.set_environment(m, intensity=16.0)
        _frame(b, cb, ob)
        seq.append(b.exposure(cb))
    met = [x[1] for x in seq]
    assert met[0] == met[2] and met[3] == np.float32(met[2] + 4.0), met   # 16 x = 4 EV = 16 bins of 0.25
    adapted = np.float32(met[2])
    for k in range(3, 14):
        adapted = R.adapt(adapted, met[k], True, step, step)
        assert seq[k][2] == adapted, (k, seq[k][2], adapted)
    if step == 0.0:
        assert seq[3][2] == met[3]
    else:
        assert seq[3][2] == np.float32(met[2] + step) and seq[-1][2] == met[3]
    b.close()


# ---------------------------------------------------------------- 6. scheduling and determinism
def _auto_run(exact, tuning=None, keep_all=None, streams=1, frames=6, scene="dungeon"):
    e = _engine(exact, scene)
    if tuning:
        e.set_tuning(**tuning)
    if keep_all is not None:
        e.keep_all_planes(keep_all)
    desc = _camera(scene)
    cam = e.create_camera(desc)
    e.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
    e.set_display(cam, tonemap=Tonemap.PBR_NEUTRAL, exposure_ev=0.25, auto_exposure=True, ev_min=-12.0, ev_max=8.0, max_ev_step_up=0.5,
                  max_ev_step_down=0.5)
    ss = [torch.cuda.Stream() for _ in range(streams)]
    out = Out(2)
    frames_out, expo = [], []
    for k in range(frames):
        s = ss[k % streams].cuda_stream
        e.tick(s)
        e.render_camera(cam, out.ptr(), s)   # no host sync between frames: the engine orders the camera's frames
        if k % 2 == 1:
            torch.cuda.synchronize()
            frames_out.append(out.get())
            expo.append(e.exposure(cam))
    e.close()
    return frames_out, expo


def test_scheduling_switches_and_streams_give_the_same_exposure_and_pixels():
    base = _auto_run(True)
    for kw in (dict(tuning=dict(overlap=0)), dict(tuning=dict(fuse=0)), dict(streams=2), dict(streams=3, tuning=dict(overlap=0))):
        other = _auto_run(True, **kw)
        assert [tuple(map(float, x)) for x in other[1]] == [tuple(map(float, x)) for x in base[1]], kw
        for x, y in zip(other[0], base[0]):
            assert np.array_equal(x, y), kw
    f1, f2 = _auto_run(False), _auto_run(False, streams=2)
    assert [tuple(map(float, x)) for x in f1[1]] == [tuple(map(float, x)) for x in f2[1]]
    for x, y in zip(f1[0], f2[0]):
        assert np.array_equal(x, y), "two fast-build runs"
    lean, full = _auto_run(False, keep_all=False), _auto_run(False, keep_all=True)
    assert [tuple(map(float, x)) for x in lean[1]] == [tuple(map(float, x)) for x in full[1]]
    for x, y in zip(lean[0], full[0]):
        assert np.array_equal(x, y), "lean frame against every plane kept"


# ---------------------------------------------------------------- 7. tiles
@pytest.mark.parametrize("world", [2, 4])
def test_manual_tiles_gather_to_the_single_frame(world):
    size = (272, 200)
    stream = torch.cuda.current_stream().cuda_stream
    disp = display_desc(Tonemap.ACES_FITTED, exposure_ev=1.25)
    desc = _camera("cornell", CameraMode.REFERENCE, False, 1, size)
    one = _engine(True)
    cam = one.create_camera(desc)
    one.set_display(cam, disp)
    single = torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda:0")
    for _ in range(3):
        one.update_camera(cam, desc); one.tick(stream); one.render_camera(cam, single.data_ptr(), stream)
    torch.cuda.synchronize()
    ranks = []
    for r in range(world):
        e = _engine(True)
        c = e.create_camera(desc)
        e.set_display(c, disp)
        e.dist_init_local(r, world, 7300 + world)
        e.dist_set_partition(c, apron=0)
        ranks.append((e, c, torch.zeros_like(single)))
    full = torch.zeros_like(single)
    for _ in range(3):
        for r in range(world - 1, -1, -1):   # in-process transport: rank 0 last
            e, c, out = ranks[r]
            e.update_camera(c, desc); e.tick(stream)
            e.render_camera(c, out.data_ptr(), stream)
            e.dist_gather(c, out.data_ptr(), full.data_ptr() if r == 0 else 0, stream)
    ranks[0][0].dist_wait(ranks[0][1], host=True)
    torch.cuda.synchronize()
    assert_bits_equal(full.cpu().numpy(), single.cpu().numpy(), f"{world} display tiles vs one engine")
    # auto together with a window: refused in either order
    e, c, _ = ranks[1]
    with pytest.raises(Exception):
        e.set_display(c, tonemap=Tonemap.ACES_FITTED, auto_exposure=True)
    e.set_camera_rows(c, 0, size[1])   # back to the whole frame
    e.set_display(c, tonemap=Tonemap.ACES_FITTED, auto_exposure=True)
    with pytest.raises(Exception):
        e.dist_set_partition(c, apron=0)
    for e, *_ in ranks:
        e.dist_shutdown(); e.close()
    one.close()


# ---------------------------------------------------------------- 8. lifecycle
def test_display_survives_arithmetic_and_camera_updates_and_reaches_present_copies():
    a, b = _engine(True), _engine(True)
    desc = _camera("cornell")
    ca, cb = a.create_camera(desc), b.create_camera(desc)
    b.set_display(cb, tonemap=Tonemap.REINHARD_LUMINANCE, exposure_ev=0.75)
    s = R.manual_scale(0.75)
    oa, ob = Out(0), Out(0)
    _check(_frame(b, cb, ob), _frame(a, ca, oa), R.REINHARD_LUMINANCE, s, 0, True, "before")
    for e in (a, b):
        e.set_exact(False); e.set_exact(True)
    _check(_frame(b, cb, ob), _frame(a, ca, oa), R.REINHARD_LUMINANCE, s, 0, True, "after an arithmetic switch")
    big = _camera("cornell", size=(80, 64))
    a.update_camera(ca, big); b.update_camera(cb, big)
    oa2, ob2 = Out(0, (80, 64)), Out(0, (80, 64))
    _check(_frame(b, cb, ob2), _frame(a, ca, oa2), R.REINHARD_LUMINANCE, s, 0, True, "after a resize")
    # present copies carry the transformed pixels
    host = torch.zeros(80 * 64 * 16, dtype=torch.uint8).pin_memory()
    stream = torch.cuda.current_stream().cuda_stream
    b.tick(stream); b.render_camera(cb, ob2.ptr(), stream)
    b.present_copy(cb, ob2.ptr(), host.data_ptr(), host.numel(), stream)
    assert b.present_ready(cb, host.data_ptr(), wait=True)
    torch.cuda.synchronize()
    assert np.array_equal(host.numpy(), ob2.t.cpu().numpy())
    # a camera with auto-exposure can be deleted, also with frames in flight
    b.set_display(cb, tonemap=Tonemap.ACES_FITTED, auto_exposure=True)
    b.tick(stream); b.render_camera(cb, ob2.ptr(), stream)
    b.delete_camera(cb)
    c2 = b.create_camera(desc)
    b.set_display(c2, tonemap=Tonemap.ACES_FITTED, auto_exposure=True)
    _frame(b, c2, ob)
    assert np.isfinite(b.exposure(c2)[1])
    a.close(); b.close()
