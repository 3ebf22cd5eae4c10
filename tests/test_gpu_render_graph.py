"""GPU test of the frame's pass graph (st_render.cpp Engine::render): which launch groups a frame considers, in which order, and how often
each kernel is launched, for one factor at a time around the default on the Cornell scene — against tests/golden/render_launches.json,
which tests/golden/make_render_launches.py wrote. Two commits wrote its entries: every case outside CHAIN_CASES with the library as it was
before Engine::render was split into phases (the parent of "Split Engine::render into phases; one owner for output scratch planes"), the
CHAIN_CASES — motion blur, depth of field, fog and light shafts did not exist then — with the library of abb0108 ("Add light shafts"),
the parent of the commit that put the HDR output chain into one node table.

Per configuration and per frame 1..6 (one cycle: both parities, the tracing frames `frame % 6 < 4` and the validation frames):
  full      last_launches() and the status of st_render_camera with every pass enabled
  mask0     the same with pass mask 0: every launch group is listed, none runs, and the frame is not a whole graph — the other half of
            every switch that asks for one
  profiled  a serial frame under profile_enable(1 | 8): launches per kernel name (last_launches merges consecutive equal groups)
  bytes     (CHAIN_CASES only) the algorithmic bytes per kernel name of that profiled frame: what each launch is credited, host arithmetic
            on integer-valued doubles, so it compares exactly
The test compares whichever recordings a case's golden entry holds. Each of the three engines is fresh and renders frames 1..6; an engine is closed before the next one is made. A render that returns a HIP error fails
its case, and every later case fails without touching the device.

Not a case: a bloom descriptor whose plan holds no level at this size — st_bloom_plan keeps a level while both sides of its mip are at
least 2, so 64 x 48 always holds five and the descriptor cannot ask for none."""
import json
import os

import pytest
import torch

from strolle_amd import (CameraMode, Engine, ResampleFilter, Tonemap, bloom_desc, display_desc, dof_desc, fog_desc, light_shafts_desc, motion_blur_desc, post_desc,
                         scenes)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_launches.json")
FRAMES = 6
EVEN, ODD = (64, 48), (72, 48)   # eight / nine tile columns
ST_ERR_HIP = 5
TUNING_FLIPS = ("overlap", "fuse", "fuse_di_head", "fuse_spatial", "fuse_wavelet", "fuse_compose", "fuse_gi_sampling", "fuse_gi_reprojection",
                "fuse_gi_validation", "preview_both", "variance_in_reproject", "lean_frame", "alias_gi_history", "di_head_on_main")


def _cases():
    """name -> what differs from the default (64 x 48, fast, IMAGE, denoise, an output buffer, Cornell, default tuning, no output chain)"""
    c = {"default": {}, "odd_tiles": dict(size=ODD), "odd_tiles_fuse_spatial_0": dict(size=ODD, tuning=dict(fuse_spatial=0)), "exact": dict(exact=True)}
    c["mode_di_diffuse"] = dict(mode=CameraMode.DI_DIFFUSE)
    c["mode_gi_diffuse"] = dict(mode=CameraMode.GI_DIFFUSE)
    c["mode_reference_depth_2"] = dict(mode=CameraMode.REFERENCE, depth=2)
    c["mode_bvh_heatmap"] = dict(mode=CameraMode.BVH_HEATMAP)
    c["denoise_0"] = dict(denoise=False)
    c["no_output"] = dict(out=False)
    c["no_instances"] = dict(scene=False)
    for field in TUNING_FLIPS:
        c["flip_" + field] = dict(flip=field)
    c["display_auto"] = dict(display=dict(tonemap=Tonemap.ACES_FITTED, auto_exposure=True))
    c["post_fxaa"] = dict(post=dict(fxaa=True))
    c["post_fxaa_96x72"] = dict(post=dict(fxaa=True, output_size=(96, 72), filter=ResampleFilter.BILINEAR))
    c["post_resize_96x72"] = dict(post=dict(output_size=(96, 72), filter=ResampleFilter.BILINEAR))
    c["bloom"] = dict(bloom=dict())
    c["display_post_bloom"] = dict(display=dict(tonemap=Tonemap.ACES_FITTED, auto_exposure=True), post=dict(fxaa=True, output_size=(96, 72)), bloom=dict())
    c["bloom_tail"] = dict(bloom=dict(), bloom_tail=-1)
    return c


# the HDR nodes in chain order: the case's key, the setter, the descriptor
CHAIN = (("fog", "set_fog", lambda: fog_desc(density=0.1, height_falloff=0.25)),
         ("shafts", "set_light_shafts", lambda: light_shafts_desc(steps=4, lights=(1,), sun_color=(1.0, 1.0, 1.0), sun_direction=(0.35, 0.8, 0.3))),
         ("dof", "set_dof", lambda: dof_desc(focal_distance=3.0, sensor_height=0.5)),
         ("mblur", "set_motion_blur", lambda: motion_blur_desc()),
         ("bloom", "set_bloom", lambda: bloom_desc()))


def _chain_cases():
    """the output chain: each later node alone (bloom alone is above), all five, all five under a display, FXAA and a resize, the subsets in
    which a node's target skips the nodes that are off, and all five in the frames that differ in what runs around the chain"""
    nodes = lambda *names: {n: True for n in names}   # noqa: E731
    every = nodes("fog", "shafts", "dof", "mblur", "bloom")
    c = {"chain_" + n: nodes(n) for n in ("mblur", "dof", "fog", "shafts")}
    c["chain_all"] = dict(every)
    c["chain_all_display_post"] = dict(every, display=dict(tonemap=Tonemap.ACES_FITTED, auto_exposure=True), post=dict(fxaa=True, output_size=(96, 72)))
    c["chain_fog_bloom"] = nodes("fog", "bloom")
    c["chain_shafts_mblur"] = nodes("shafts", "mblur")
    c["chain_dof_bloom"] = nodes("dof", "bloom")
    c["chain_fog_dof"] = nodes("fog", "dof")
    for name in ("mode_reference_depth_2", "mode_bvh_heatmap", "no_output", "denoise_0", "flip_overlap"):
        c["chain_all_" + name] = dict(every, **CASES[name])
    return c


CASES = _cases()
CHAIN_CASES = _chain_cases()
CASES.update(CHAIN_CASES)
_hip_error = []   # the first render that returned a HIP error: nothing is started after it


def make_engine(case, lib_engine=Engine):
    """(engine, camera, output tensor or None) of a case; the caller closes the engine"""
    e = lib_engine(device=0, exact=bool(case.get("exact", False)))
    if case.get("scene", True):
        scenes.build_cornell(e)
    else:
        e.set_blue_noise(scenes.load_blue_noise())
    e.set_seed(7)
    if "flip" in case:
        e.set_tuning(**{case["flip"]: 0 if getattr(e.tuning(), case["flip"]) else 1})
    if "tuning" in case:
        e.set_tuning(**case["tuning"])
    size = case.get("size", EVEN)
    cam = e.create_camera(scenes.cornell_camera(size, case.get("mode", CameraMode.IMAGE), denoise=case.get("denoise", True), depth=case.get("depth", 0)))
    if "display" in case:
        e.set_display(cam, display_desc(**case["display"]))
    if "post" in case:
        e.set_post(cam, post_desc(**case["post"]))
    if "bloom" in case and case["bloom"] is not True:
        e.set_bloom(cam, bloom_desc(**case["bloom"]))
    for key, setter, desc in CHAIN:
        if case.get(key) is True:
            getattr(e, setter)(cam, desc())
    if "bloom_tail" in case:
        e.set_bloom_tail(case["bloom_tail"])
    out = None
    if case.get("out", True):
        w, h = e.output_size(cam)
        out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    return e, cam, out


def _frames(name, case, what):
    """frames 1..6 of a fresh engine: per frame (status, last_launches) — `what` = "profiled": (status, {kernel: launches}), and beside
    them (status, {kernel: algorithmic bytes})"""
    e, cam, out = make_engine(case)
    rows, credited = [], []
    try:
        if what == "mask0":
            e.set_pass_mask(0)
        if what == "profiled":
            e.profile_enable(1 | 8)
        stream = torch.cuda.current_stream().cuda_stream
        for frame in range(1, FRAMES + 1):
            e.tick(stream)
            status = e._b.render_camera(e._h, cam, out.data_ptr() if out is not None else 0, stream)   # the status itself, not an exception
            if status == ST_ERR_HIP:
                _hip_error.append(f"{name} / {what} / frame {frame}: {e._b.last_error().decode(errors='replace')}")
                pytest.fail(_hip_error[0])
            torch.cuda.synchronize()
            if what == "profiled":
                prof = [p for p in e.profile_read(reset=True) if p["launches"]]
                rows.append([status, {p["name"]: p["launches"] for p in prof}])
                credited.append([status, {p["name"]: p["algorithmic_bytes"] for p in prof}])
            else:
                rows.append([status, e.last_launches()])
    finally:
        e.close()
    return rows, credited


def record(name):
    case = CASES[name]
    rec = {what: _frames(name, case, what)[0] for what in ("full", "mask0")}
    rec["profiled"], credited = _frames(name, case, "profiled")
    if name in CHAIN_CASES:
        rec["bytes"] = credited
    return rec


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_a_frame_considers_and_launches_what_it_did_before_the_split(name, golden):
    assert not _hip_error, f"not started: an earlier render returned a HIP error ({_hip_error[0]})"
    got = json.loads(json.dumps(record(name)))   # (as JSON holds it: lists, string keys)
    want = golden[name]
    assert set(want) >= {"full", "mask0", "profiled"} and set(want) <= set(got), sorted(want)
    for what in want:
        for frame in range(FRAMES):
            assert got[what][frame] == want[what][frame], f"{name}: {what}, frame {frame + 1}"
