"""GPU test of the routing of the HDR output chain (st_render.cpp: fog, light shafts, depth of field, motion blur, bloom, in that order):
every one of the 32 subsets of the five nodes, bit for bit against the stateless calls of the nodes that are on.

One pair of engines, fast build, dungeon, 64 x 48, a camera that moves every frame. Engine A is plain; engine B carries the settings. After a
warm-up frame, per subset: exactly those nodes are set on B, both render one frame, and B's output must hold the bits of st_fog_process,
st_light_shafts_process, st_dof_process, st_motion_blur_process and st_bloom_process — those of the subset, chained in that order — over A's
output with B's G-buffer depth and velocity map. The intermediate calls write RGBA32F without a display, the last one the camera's format
through the camera's display. Once with an RGBA32F target and no display, once with RGBA8 sRGB through ACES. (An empty subset under ACES has
no call to compare with: it is held to the display's restatement by tests/test_gpu_display.py's criterion.)

Toggling a node leaves the temporal state alone (each node's "planes do not depend on the setting" test), so one pair serves every subset.
The other tests hold each stateless call to its float64 definition; this one ties every routing of the chain to those calls."""
import itertools

import numpy as np
import pytest
import torch

import display_ref
from output_chain import MEDIUM, SUN, Depth, Out, _bits, _check, _engine, _moving, _proj, _xf
from strolle_amd import Buffer, OutputFormat, Tonemap, bloom_desc, display_desc, dof_desc, fog_desc, light_shafts_desc, motion_blur_desc

pytestmark = pytest.mark.gpu
SIZE = (64, 48)
SCENE = "dungeon"
NODES = ("fog", "shafts", "dof", "mblur", "bloom")   # chain order
SUBSETS = [s for n in range(len(NODES) + 1) for s in itertools.combinations(NODES, n)]
DESCS = dict(fog=fog_desc(color=(0.5, 0.6, 0.7, 0.9), density=0.12, height_falloff=0.25, height_reference=0.5),
             shafts=light_shafts_desc(steps=8, divisor=2, lights=(3, 1), **dict(MEDIUM, **SUN)),
             dof=dof_desc(samples=32, autofocus=(0.5, 0.5), sensor_height=0.5, focal_distance=3.0),
             mblur=motion_blur_desc(shutter=1.0, samples=8),
             bloom=bloom_desc(intensity=0.3, threshold=0.4, threshold_softness=0.5))
SETTERS = dict(fog="set_fog", shafts="set_light_shafts", dof="set_dof", mblur="set_motion_blur", bloom="set_bloom")
ACES = display_desc(tonemap=Tonemap.ACES_FITTED, exposure_ev=0.5)


class Pair:
    def __init__(self):
        self.a, self.b = _engine(False, SCENE), _engine(False, SCENE)
        self.ca, self.cb = self.a.create_camera(_moving(SCENE, 0, SIZE)), self.b.create_camera(_moving(SCENE, 0, SIZE))
        self.oa, self.depth, self.k = Out(0, SIZE), Depth(), 0
        self.frame(Out(0, SIZE))   # warm-up

    def frame(self, ob):
        """one frame of both engines at the next camera position: (the camera, A's colour, B's depth)"""
        stream = torch.cuda.current_stream().cuda_stream
        cam = _moving(SCENE, self.k % 4, SIZE)
        self.k += 1
        for e, c, o in ((self.a, self.ca, self.oa), (self.b, self.cb, ob)):
            e.update_camera(c, cam); e.tick(stream); e.render_camera(c, o.ptr(), stream)
        torch.cuda.synchronize()
        return cam, self.depth.read(self.b, self.cb, SIZE)

    def close(self):
        self.a.close(); self.b.close()


@pytest.fixture(scope="module")
def pair():
    p = Pair()
    yield p
    p.close()


def _chained(p, on, cam, z, fmt, display):
    """the stateless calls of the nodes in `on`, in chain order, over A's output: the last one in `fmt` through `display`"""
    w, h = SIZE
    b, stream = p.b, torch.cuda.current_stream().cuda_stream
    tz = torch.from_numpy(z).cuda()
    tv = torch.from_numpy(b.read_buffer(p.cb, Buffer.VELOCITY_MAP).reshape(h, w, 4)[..., :2].copy()).cuda() if "mblur" in on else None
    M, P = _xf(cam), _proj(cam)
    src = p.oa
    for node in on:
        last = node == on[-1]
        dst = Out(fmt if last else 0, SIZE, fill=0xa5)
        kw = dict(display=display if last else None, stream=stream)
        f = dst.fmt
        if node == "fog":
            b.fog_process(DESCS[node], M, P, src.ptr(), tz.data_ptr(), w, h, dst.ptr(), f, **kw)
        elif node == "shafts":
            b.light_shafts_process(DESCS[node], M, P, src.ptr(), tz.data_ptr(), w, h, dst.ptr(), f, **kw)
        elif node == "dof":
            b.dof_process(DESCS[node], P, src.ptr(), tz.data_ptr(), w, h, dst.ptr(), f, **kw)
        elif node == "mblur":
            b.motion_blur_process(DESCS[node], src.ptr(), tv.data_ptr(), tz.data_ptr(), w, h, dst.ptr(), f, **kw)
        else:
            b.bloom_process(DESCS[node], src.ptr(), w, h, dst.ptr(), f, **kw)
        src = dst
    torch.cuda.synchronize()
    return src.get()


@pytest.mark.parametrize("target", ["rgba32f", "aces_rgba8_srgb"])
def test_every_subset_of_the_chain_equals_the_process_calls_of_its_nodes(pair, target):
    p = pair
    fmt, display = (0, None) if target == "rgba32f" else (int(OutputFormat.RGBA8_UNORM_SRGB), ACES)
    p.b.set_display(p.cb, display)
    p.b.set_output_format(p.cb, OutputFormat(fmt))
    differs = 0
    for on in SUBSETS:
        for node in NODES:
            getattr(p.b, SETTERS[node])(p.cb, DESCS[node] if node in on else None)
        ob = Out(fmt, SIZE, fill=0x5a)
        cam, z = p.frame(ob)
        got, plain = ob.get(), p.oa.get()
        if not on and display is not None:
            _check(got, display_ref.transform(plain[..., :3], int(display.tonemap), display_ref.manual_scale(display.exposure_ev)), fmt, f"{target}: no node")
            continue
        want = _chained(p, on, cam, z, fmt, display) if on else plain
        same = np.array_equal(got, want) if fmt else np.array_equal(_bits(got), _bits(want))
        assert same, (target, on, int(np.count_nonzero(got != want)))
        if on and not fmt:
            differs += not np.array_equal(_bits(got), _bits(plain))
    assert fmt or differs == len(SUBSETS) - 1, "every node changes the frame"
