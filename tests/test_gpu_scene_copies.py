"""The tick's device copies (strolle_amd/csrc/st_copies.h) under edits with frames in flight: the scene's and the lights' pairs, a replaced and a
cleared environment map, a replaced and a removed look-up table — on one stream, on two streams that alternate per frame (the readers' streams are
then mixed: a writer and a retirement join the device) and with the tick on one stream and the render on another. Cornell, fast build,
Image{denoise}, 64 x 48, colour grading with a side-5 table, a 16 x 8 map, RGBA32F into one buffer per frame; twelve frames, each edit in front of
its frame's tick. Every variant equals, bit for bit, the run that joins the device after every frame."""
import os

import numpy as np
import pytest
import torch

import grade_cases as K
from output_chain import Out, _engine
from strolle_amd import Instance, Light, Material, scenes

pytestmark = pytest.mark.gpu
SIZE, FRAMES, LUT_ID = (64, 48), 12, 41
EDITED = range(2, 11)   # the frames with an edit in front (_edit)


def _edit(e, k, box):
    sky = lambda seed: (np.random.default_rng(seed).random((8, 16, 3)) * 4.0).astype(np.float32)
    at = lambda dx: np.concatenate([box[:, :3], box[:, 3:] + np.float32([[dx], [0.0], [0.0]])], 1)
    lamp = lambda x: e.insert_light(1, Light.point((x, 1.5, 0.5), 0.15, (4.0,) * 3, 20.0))
    if k == 0:
        e.insert_lut(LUT_ID, K.lut("random", 5)); e.set_environment(sky(1))
    if k == 2: e.insert_instance(7, Instance(7, 7, at(0.3)))                      # an instance re-inserted with a new transform
    if k == 3: lamp(0.4)                                                          # a point light moved
    if k == 4: e.insert_material(6, Material(base_color=(0.1, 0.2, 0.9, 1.0)))    # a material's base colour
    if k == 5: e.set_environment(sky(2))                                          # the map replaced
    if k == 6: lamp(-0.4)
    if k == 7: e.insert_lut(LUT_ID, K.lut("random", 5, seed=9))                   # the table replaced
    if k == 8: e.insert_instance(50, Instance(7, 4, at(-0.5)))                    # an instance spawned
    if k == 9: e.clear_environment()
    if k == 10: e.remove_lut(LUT_ID)


def _run(variant):
    """the twelve frames of one variant; close() comes with the last frames still in flight (the base run has joined them)"""
    box = np.load(os.path.join(scenes.ASSETS, "cornell.npz"))["xform_6"].reshape(4, 3).T.astype(np.float32)
    e = _engine(False)
    cam = e.create_camera(scenes.cornell_camera(SIZE))
    e.set_color_grading(cam, lut=LUT_ID, contrast=1.3, saturation=0.6)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    outs = [Out(0, SIZE) for _ in range(FRAMES)]
    torch.cuda.synchronize()
    for k in range(FRAMES):
        tick, render = {"base": (a, a), "one": (a, a), "alternating": ((a, b)[k % 2],) * 2, "split": (a, b)}[variant]
        _edit(e, k, box)
        e.tick(tick.cuda_stream)
        e.render_camera(cam, outs[k].ptr(), render.cuda_stream)
        if variant == "base":
            torch.cuda.synchronize()
    e.close()
    torch.cuda.synchronize()
    return [o.get() for o in outs]


@pytest.fixture(scope="module")
def base():
    return _run("base")


def test_the_edits_show(base):
    for k in EDITED:
        assert np.isfinite(base[k]).all() and not np.array_equal(base[k - 1], base[k]), k


@pytest.mark.parametrize("variant", ["one", "alternating", "split"])
def test_edits_with_frames_in_flight_bit_exact(base, variant):
    for k, (got, want) in enumerate(zip(_run(variant), base)):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (variant, k)
