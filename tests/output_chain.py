"""What the GPU tests of the output chain share (test_gpu_fog, _shafts, _dof, _motion_blur, _bloom, _post, _display, _output_chain): the
engines, cameras and output buffers they build, the comparison against a restatement, and the test bodies that every node of the chain
repeats — off is off, nothing else depends on the setting, the frames that skip the node, frames in flight, teardown. A body is a function
of a `Node` record; the test function that calls it stays in the node's own file under its own name. Where a node's copy really differs
(motion blur's velocity map, its own camera path) the difference is an argument. A plain module: no fixtures, no pytest settings."""
from dataclasses import dataclass

import numpy as np
import torch

import post_ref
from parity import assert_bits_equal
from ref_num import frame_depth
from strolle_amd import Aov, Buffer, Camera, CameraMode, Engine, OutputFormat, PassBit, Sun, Tonemap, aov_planes, scenes

SIZE = (72, 52)   # no multiple of any tile of the chain: 32 x 8 workgroups, 32 x 32 tiles, FXAA's 64 x 8, the resampler's 64 x 4
BPP = {0: 16, 1: 8, 2: 4, 3: 4}
# the medium and the sun of the frames with light shafts: tests/test_gpu_shafts.py and the routing test of tests/test_gpu_output_chain.py
MEDIUM = dict(density=0.08, anisotropy=0.6, max_distance=30.0, intensity=1.5, scatter=(0.9, 0.8, 0.6))
SUN = dict(sun_color=(6.0, 5.0, 4.0), sun_direction=(0.35, 0.8, 0.3))


# ---------------------------------------------------------------- engines, cameras, buffers
def _engine(exact, scene="cornell"):
    e = Engine(device=0, exact=exact)
    if scene == "cornell":
        scenes.build_cornell(e)
    else:
        scenes.build_dungeon(e)
        e.update_sun(Sun(azimuth=0.6, altitude=0.5))   # the sun up: lit areas far above 1
    e.set_seed(7)
    return e


def _camera(scene="cornell", mode=CameraMode.IMAGE, denoise=True, depth=0, size=SIZE):
    return (scenes.cornell_camera if scene == "cornell" else scenes.dungeon_camera)(size, mode, denoise=denoise, depth=depth)


def _scene_camera(scene, size, mode=CameraMode.IMAGE, denoise=True):
    return (scenes.cornell_camera if scene == "cornell" else scenes.dungeon_camera)(size, mode, denoise=denoise)


MOVES = (0.07, 0.05, 0.09, 0.06)


def _moving(scene, k, size=SIZE, mode=CameraMode.IMAGE):
    """the camera in front of frame k: it steps sideways by MOVES[k - 1]"""
    base, target = ((0.0, 1.0, 3.2), (0.0, 1.0, 0.0)) if scene == "cornell" else ((-5.75, 0.5, -16.8), (-5.75, 0.5, -17.0))
    dx = sum(MOVES[:k]) * (5.0 if scene == "cornell" else 1.0)
    return scenes.camera_for(size, (base[0] + dx, base[1] + 0.4 * dx, base[2]), (target[0] + 0.3 * dx, target[1], target[2]), mode, True)


def _orthographic(size):
    cam = scenes.cornell_camera(size)
    cam.projection = np.array([[0.8, 0, 0, 0], [0, 0.8, 0, 0], [0, 0, 0.01, 1.0], [0, 0, 0, 1.0]], np.float32)   # [15] = 1: no perspective ray, no focal length to derive
    return cam


class Out:
    """a device output buffer of one format"""

    def __init__(self, fmt=0, size=SIZE, fill=0):
        self.fmt, self.size = int(fmt), size
        self.t = torch.full((size[1] * size[0] * BPP[self.fmt],), fill, dtype=torch.uint8, device="cuda:0")

    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        a = self.t.cpu().numpy()
        w, h = self.size
        if self.fmt == 0:
            return a.view(np.float32).reshape(h, w, 4).copy()
        if self.fmt == 1:
            return a.view(np.float16).reshape(h, w, 4).copy()
        return a.reshape(h, w, 4).copy()


def _frame(e, cam, out, stream=None):
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    e.tick(s)
    e.render_camera(cam, out.ptr(), s)
    torch.cuda.synchronize()
    return out.get()


def _check(got, ref32, fmt, what):
    """`got` in format `fmt` against the restatement's float32 result: RGBA32F bit for bit (NaN payloads aside), RGBA16F bit for bit its
    round-to-nearest-even, the 8-bit formats by tests/test_gpu_display.py's criterion (within 1, 99.9 % exact, alpha 255)"""
    want = post_ref.to_format(ref32, fmt)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if fmt == 0:
        assert_bits_equal(got, want, what)
    elif fmt == 1:
        ok = (got.view(np.uint16) == want.view(np.uint16)) | (np.isnan(got) & np.isnan(want))
        assert ok.all(), f"{what}: {np.count_nonzero(~ok)} half channels differ"
    else:
        d = np.abs(got[..., :3].astype(np.int32) - want[..., :3].astype(np.int32))
        assert d.max() <= 1, f"{what}: 8-bit channel off by {d.max()}"
        assert (d == 0).mean() >= 0.999, f"{what}: only {(d == 0).mean():.5f} of the 8-bit channels exact"
        assert (got[..., 3] == 255).all(), what


def _image(w, h, seed=11, spoil=True):
    rng = np.random.default_rng(seed)
    img = np.exp(rng.standard_normal((h, w, 4)) * 2.0).astype(np.float32)   # HDR: far above 1 in places
    img[rng.random((h, w)) < 0.01] *= 300.0                                  # fireflies
    if spoil:
        img[rng.random((h, w)) < 0.03] *= -1.0
        n = max(1, w * h // 150)
        for v in (np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30):
            img[rng.integers(0, h, n), rng.integers(0, w, n), rng.integers(0, 3, n)] = v
    return img


_REFS = {}


def _ref(module, key, make):
    """a restatement's result, computed once and shared by the two builds: one cache, keyed by the test module and its own key"""
    if (module, key) not in _REFS:
        _REFS[module, key] = make()
    return _REFS[module, key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _proj(cam: Camera):
    """the 16 floats of a camera's projection, column major"""
    return np.asarray(cam.projection, np.float32).T.reshape(-1).copy()


def _xf(cam):
    """the 16 floats of a camera's transform, column major"""
    return np.asarray(cam.transform, np.float32).T.reshape(-1).copy()


def _all_planes(e, cam):
    return {b: e.read_buffer(cam, b) for b in Buffer}


class Depth:
    """D of the frame just rendered: PRIM_GBUFFER_D0.x of the frame's parity. Which of the two G-buffers the frame wrote is found by what
    changed since the last look (under a static camera the two are equal anyway)."""

    def __init__(self):
        self.prev = {}

    def read(self, e, cam, size):
        g = {b: e.read_buffer(cam, b) for b in (Buffer.PRIM_GBUFFER_D0_A, Buffer.PRIM_GBUFFER_D0_B)}
        changed = [b for b in g if b not in self.prev or not np.array_equal(_bits(self.prev[b]), _bits(g[b]))]
        if len(self.prev) == 0:   # the first frame: the other plane is still zero
            changed = [b for b in g if _bits(g[b]).any()]
        self.prev = g
        assert len(changed) <= 1, "a frame writes one of the two G-buffers"
        cur = g[changed[0]] if changed else g[Buffer.PRIM_GBUFFER_D0_A]
        w, h = size
        return frame_depth(cur.reshape(h, w, 4)[..., 0])


# ---------------------------------------------------------------- a node of the chain, as its tests see it
@dataclass(frozen=True)
class Node:
    """`settings` and the per-test settings are a dict of the setter's keyword arguments or a descriptor; a per-test one left None is `settings`"""
    setter: str                 # Engine.set_fog, ...
    getter: str
    noun: str                   # "fog": "... with fog set, frame 0"
    differs: str                # "the fogged frame differs"
    slots: tuple                # the profile slots of the node; each is launched once per frame
    settings: object
    cleared: object = None      # ... of cleared_setting_renders_like_none
    independent: object = None  # ... of nothing_else_depends_on_the_setting
    skipped: object = None      # ... of frames_that_skip
    pipelined: object = None    # ... of pipeline
    recreated: object = None    # ... of the new camera in teardown_with_the_setting_on
    counts_rays: bool = False   # the node traces: a frame that skips it counts the rays of a frame without it

    def set(self, e, cam, s):
        if isinstance(s, dict):
            getattr(e, self.setter)(cam, **s)
        else:
            getattr(e, self.setter)(cam, s)   # a descriptor, or None to clear

    def get(self, e, cam):
        return getattr(e, self.getter)(cam)

    def of(self, test):
        s = getattr(self, test)
        return self.settings if s is None else s


def _cornell(k):
    return _moving("cornell", k)


def _dungeon(k):
    return _moving("dungeon", k)


def _dungeon4(k):
    return _moving("dungeon", k % 4)   # another view every frame: frame k + 2's depths are not frame k's


def cleared_setting_renders_like_none(node, exact, camera=_cornell, frames=4, differs=True, unwritten_velocity=False):
    """Two frames with the setting, then cleared: from then on the bytes, launches and planes of an engine that never had it.
    `differs`: the frames with the setting are also held to differ. `unwritten_velocity`: a velocity map that is stale in both engines is
    not compared (motion blur: b's still holds what its last blurred frame kept)."""
    a, b = _engine(exact), _engine(exact)
    ca, cb = a.create_camera(camera(0)), b.create_camera(camera(0))
    node.set(b, cb, node.of("cleared"))
    oa, ob = Out(0), Out(0)
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(frames):
        if k == 2:
            node.set(b, cb, None)
        for e, cam, o in ((a, ca, oa), (b, cb, ob)):
            e.update_camera(cam, camera(k)); e.tick(stream); e.render_camera(cam, o.ptr(), stream)
        torch.cuda.synchronize()
        if k < 2:
            assert any(l & PassBit.POST for l in b.last_launches())
            if differs:
                assert not np.array_equal(_bits(oa.get()), _bits(ob.get()))
            continue
        assert np.array_equal(_bits(oa.get()), _bits(ob.get())), (exact, k)
        assert b.last_launches() == a.last_launches() and not any(l & PassBit.POST for l in b.last_launches())
        pa, pb = _all_planes(a, ca), _all_planes(b, cb)
        for buf in Buffer:
            assert a.buffer_stale(ca, buf) == b.buffer_stale(cb, buf), (k, buf)
            if unwritten_velocity and buf == Buffer.VELOCITY_MAP and a.buffer_stale(ca, buf):
                continue
            assert np.array_equal(_bits(pa[buf]), _bits(pb[buf])), (exact, k, buf)
    a.close(); b.close()


def nothing_else_depends_on_the_setting(node, camera=_dungeon, differs_from=0, velocity_map=True):
    """AOVs, picks, planes, the exposure and the histogram of a camera with the setting are those of one without, while the frames differ
    (from frame `differs_from` on). `velocity_map` False: that plane is not compared (motion blur makes the frame keep it)."""
    a, b = _engine(False, "dungeon"), _engine(False, "dungeon")
    ca, cb = a.create_camera(camera(0)), b.create_camera(camera(0))
    for e, cam in ((a, ca), (b, cb)):
        e.set_display(cam, tonemap=Tonemap.ACES_FITTED, auto_exposure=True, ev_min=-12.0, ev_max=8.0)
    node.set(b, cb, node.of("independent"))
    oa, ob = Out(0), Out(0)
    pixels = torch.tensor([[0, 0], [36, 26], [71, 51], [10, 40], [60, 5]], dtype=torch.uint32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(3):
        for e, cam, o in ((a, ca, oa), (b, cb, ob)):
            e.update_camera(cam, camera(k)); e.tick(stream); e.render_camera(cam, o.ptr(), stream)
        pa, pb = aov_planes(SIZE, fill=0), aov_planes(SIZE, fill=0)
        a.render_aovs(ca, pa); b.render_aovs(cb, pb)
        ha, hb = torch.zeros(5 * 64, dtype=torch.uint8, device="cuda:0"), torch.zeros(5 * 64, dtype=torch.uint8, device="cuda:0")
        a.pick(ca, pixels.data_ptr(), 5, ha.data_ptr()); b.pick(cb, pixels.data_ptr(), 5, hb.data_ptr())
        torch.cuda.synchronize()
        if k >= differs_from:
            assert not np.array_equal(_bits(oa.get()), _bits(ob.get())), node.differs
        for kind in Aov:
            assert np.array_equal(pa[kind].cpu().view(torch.uint8).numpy(), pb[kind].cpu().view(torch.uint8).numpy()), (k, kind)
        assert np.array_equal(ha.cpu().numpy(), hb.cpu().numpy()), k
        for buf in Buffer:
            if velocity_map or buf != Buffer.VELOCITY_MAP:
                assert a.buffer_stale(ca, buf) == b.buffer_stale(cb, buf), (k, buf)
                assert np.array_equal(_bits(a.read_buffer(ca, buf)), _bits(b.read_buffer(cb, buf))), (k, buf)
        ea, eb = a.exposure(ca), b.exposure(cb)
        assert ea == eb and np.isfinite(ea[1]), (k, ea, eb)
        assert np.array_equal(a.camera_histogram(ca), b.camera_histogram(cb))
    a.close(); b.close()


def frames_that_skip(node, what, size):
    """Reference, heatmap and orthographic frames with the setting on: the bits and launches of the frame without it"""
    a, b = _engine(True), _engine(True)
    cam = {"reference": lambda: scenes.cornell_camera(size, CameraMode.REFERENCE, denoise=False, depth=1),
           "heatmap": lambda: scenes.cornell_camera(size, CameraMode.BVH_HEATMAP, denoise=False), "orthographic": lambda: _orthographic(size)}[what]()
    ca, cb = a.create_camera(cam), b.create_camera(cam)
    node.set(b, cb, node.of("skipped"))
    oa, ob = Out(0, size), Out(0, size)
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(2):
        for e, c, o in ((a, ca, oa), (b, cb, ob)):
            if node.counts_rays:
                e.ray_count(c, reset=True)
            e.tick(stream); e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        assert_bits_equal(ob.get(), oa.get(), f"{what} with {node.noun} set, frame {k}")
        assert _bits(oa.get()).any()
        assert b.last_launches() == a.last_launches() and not any(l & PassBit.POST for l in b.last_launches())
        if node.counts_rays:
            assert a.ray_count(ca) == b.ray_count(cb)
    a.close(); b.close()


def pipeline(node, sync_every_frame, streams=1, profiling=False, frames=8, camera=_dungeon4):
    """`frames` dungeon frames through RGBA8 sRGB and ACES with the setting on, a host sync after every frame or none, round robin over
    `streams` streams: (the frames, the launches per profile slot when profiling)"""
    e = _engine(False, "dungeon")
    if profiling:
        e.profile_enable(1)   # per-kernel timing: the serial schedule
    cam = e.create_camera(camera(0))
    e.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
    e.set_display(cam, tonemap=Tonemap.ACES_FITTED, exposure_ev=0.5)
    node.set(e, cam, node.of("pipelined"))
    ss = [torch.cuda.Stream() for _ in range(streams)]
    outs = [Out(2) for _ in range(frames)]
    torch.cuda.synchronize()
    for k in range(frames):
        s = ss[k % streams].cuda_stream
        e.update_camera(cam, camera(k))
        e.tick(s)
        e.render_camera(cam, outs[k].ptr(), s)
        if sync_every_frame:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    got = [o.get() for o in outs]
    names = {p["name"]: p["launches"] for p in e.profile_read()} if profiling else None
    e.close()
    return got, names


def frames_in_flight_read_their_own_inputs(node, camera=_dungeon4):
    """Without a host sync, on two streams and under the profiler's serial schedule: the frames of the run that syncs after every frame"""
    base, _ = pipeline(node, True, camera=camera)
    assert any(not np.array_equal(base[k], base[k + 1]) for k in range(7))
    for kw in (dict(), dict(streams=2), dict(profiling=True)):
        for sync in ((False,) if not kw else (True, False)):
            other, names = pipeline(node, sync, camera=camera, **kw)
            for k, (x, y) in enumerate(zip(other, base)):
                assert np.array_equal(x, y), (kw, sync, k)
            if names is not None:   # the node's slots report themselves
                for slot in node.slots:
                    assert names[slot] == 8, names


def teardown_with_the_setting_on(node, engine, camera, desc=None):
    """Delete `camera` with the setting on and a frame in flight; a new camera starts clean; leave the engine with such a frame in flight
    (the caller closes it)"""
    desc = desc if desc is not None else scenes.cornell_camera(SIZE)
    stream = torch.cuda.current_stream().cuda_stream
    keep = Out(0)
    engine.tick(stream); engine.render_camera(camera, keep.ptr(), stream)
    engine.delete_camera(camera)
    c3 = engine.create_camera(desc)
    assert not node.get(engine, c3)[1]
    node.set(engine, c3, node.of("recreated"))
    engine.tick(stream); engine.render_camera(c3, keep.ptr(), stream)
    torch.cuda.synchronize()
    assert np.isfinite(keep.get()).all()
    engine.tick(stream); engine.render_camera(c3, keep.ptr(), stream)
