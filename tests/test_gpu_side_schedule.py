"""StTuning::side_start (include/strolle_hip.h; st_render.cpp two_streams / denoise): where the NEXT frame's side-stream work may start —
behind this frame's DI passes (0), or also behind the a-trous launch of strides 1+2 (1), stride 4 (2) or stride 8 (3). Only waits move, so
every value renders the bits of the serial schedule (overlap = 0): the composed frame at every frame, and after the last frame the
reservoir and denoiser planes, in both builds — also with motion blur (its pack launch sits in front of ev_prim_ok and reads the
single-buffered velocity map), with an auto-exposure display, when two-stream and serial frames alternate, when the value changes every
frame, and with two cameras on one engine.

Cornell at 64 x 48 and 72 x 48 (8 and 9 tile columns: the fused spatial launches need an even count, so the two sizes take different
launch lists), 12 frames = two 6-frame GI cycles. The frames of a run are enqueued without a host synchronisation in between — each into
an output buffer of its own — so that frame N + 1's side stream really runs beside frame N. One serial run per (size, build, variant) is
the reference of every test that needs it."""
import math

import numpy as np
import pytest
import torch

from output_chain import Out, _bits, _engine
from strolle_amd import Buffer, CameraMode, Tonemap, scenes

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (72, 48)]
FRAMES = 12
PLANES = [b for b in Buffer if b.name.startswith(("DI_RESERVOIRS_", "GI_RESERVOIRS_", "DI_DIFF_", "GI_DIFF_"))]
SERIAL = dict(overlap=0)
_serial = {}


def _cam(size, k, moving):
    """Cornell's camera in front of frame k; `moving`: on a slow orbit around the box (every pixel has a velocity)"""
    if not moving:
        return scenes.cornell_camera(size, CameraMode.IMAGE)
    a = 0.04 * k
    return scenes.camera_for(size, (3.2 * math.sin(a), 1.0, 3.2 * math.cos(a)), (0.0, 1.0, 0.0), CameraMode.IMAGE)


def _setup(e, cam, variant):
    if variant == "blur":
        e.set_motion_blur(cam, shutter=1.0, samples=8)
    if variant == "auto":
        e.set_display(cam, tonemap=Tonemap.ACES_FITTED, auto_exposure=True, ev_min=-12.0, ev_max=8.0)


def _run(exact, variant, sizes, schedule):
    """FRAMES frames of one engine with one camera per entry of `sizes`, rendered in that order after every tick. schedule(k) -> (StTuning
    fields, profile flags) in front of frame k. Returns per camera {"frames": [composed frame] * FRAMES, "planes": {plane: bits}, "exposure"}."""
    e = _engine(exact)
    moving = variant == "blur"
    cams = [e.create_camera(_cam(size, 0, moving)) for size in sizes]
    for cam in cams:
        _setup(e, cam, variant)
    outs = [[Out(0, size) for _ in range(FRAMES)] for size in sizes]
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(FRAMES):
        fields, profile = schedule(k)
        e.set_tuning(**fields); e.profile_enable(profile)
        for cam, size in zip(cams, sizes):
            e.update_camera(cam, _cam(size, k, moving))
        e.tick(stream)
        for cam, o in zip(cams, outs):
            e.render_camera(cam, o[k].ptr(), stream)
    torch.cuda.synchronize()
    e.profile_enable(0)
    got = [{"frames": [_bits(x.get()) for x in o], "planes": {b: _bits(e.read_buffer(cam, b)) for b in PLANES}, "exposure": e.exposure(cam) if variant == "auto" else None}
           for cam, o in zip(cams, outs)]
    e.close()
    return got


def _reference(exact, variant, size):
    key = (exact, variant, size)
    if key not in _serial:
        _serial[key] = _run(exact, variant, [size], lambda k: (SERIAL, 0))[0]
        frames = _serial[key]["frames"]
        assert all(f.any() for f in frames), "an empty frame"
        assert any(not np.array_equal(frames[0], f) for f in frames[1:]), "twelve equal frames: nothing accumulates"
    return _serial[key]


def _same(got, want, what):
    for k, (g, w) in enumerate(zip(got["frames"], want["frames"])):
        assert np.array_equal(g, w), f"{what}: the composed frame {k + 1} differs from the serial run's in {int((g != w).sum())} lanes"
    for b in PLANES:
        assert np.array_equal(got["planes"][b], want["planes"][b]), f"{what}: {b.name} differs from the serial run's after frame {FRAMES}"
    assert got["exposure"] == want["exposure"], what


@pytest.mark.parametrize("variant", ["plain", "blur", "auto"])
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_every_start_point_renders_the_serial_schedules_bits(size, exact, variant):
    want = _reference(exact, variant, size)
    for start in range(4):
        got = _run(exact, variant, [size], lambda k: (dict(overlap=1, side_start=start), 0))[0]
        _same(got, want, f"{size} exact={exact} {variant} side_start={start}")


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_two_stream_and_serial_frames_alternate(size, exact):
    """per-kernel profiling makes a frame serial: on and off every third frame, at every start point"""
    want = _reference(exact, "plain", size)
    for start in range(1, 4):
        got = _run(exact, "plain", [size], lambda k: (dict(overlap=1, side_start=start), (k // 3) % 2))[0]
        _same(got, want, f"{size} exact={exact} side_start={start}, profiled every other three frames")


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_the_start_point_changes_every_frame(size, exact):
    want = _reference(exact, "plain", size)
    for first in range(2):
        got = _run(exact, "plain", [size], lambda k: (dict(overlap=1, side_start=(3 * k + first) % 4), 0))[0]
        _same(got, want, f"{size} exact={exact} side_start=(3k + {first}) % 4")


@pytest.mark.parametrize("exact", [False, True])
def test_two_cameras_of_one_engine_each_render_their_single_camera_run(exact):
    """each camera has its own side stream and events: rendered one after the other behind every tick, neither waits for — nor overtakes — the other's frames"""
    for start in range(4):
        got = _run(exact, "plain", SIZES, lambda k: (dict(overlap=1, side_start=start), 0))
        for size, g in zip(SIZES, got):
            _same(g, _reference(exact, "plain", size), f"two cameras, {size} exact={exact} side_start={start}")

