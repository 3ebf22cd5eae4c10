"""Both builds against the CPU oracle at odd, tiny and tall frame shapes.

The pass graph is built from frame geometry: a wave owns an 8x8 tile and a block four tiles in a row (st_device.h tile_for_block), the
half-resolution passes count tiles of 16 pixels and drop the last 8-pixel tile column when the tile-column count is odd (k_common.h
tile_window, st_render.cpp even_tiles — which alone switches the fused spatial launch, kLeanGiRes2 and skip_dead_scratch), the LDS-staged
a-trous passes work on 32x16 blocks with viewport-clipped halos (k_denoise.hip wavelet_stage / wavelet_block), and both tilings are re-dealt
to XCDs in chunks of 256 pixel rows (tile_map / tile_map_denoise). The other modules stay on regular shapes; here are the shapes where each
of those structures has a remainder:

  1x1, 7x5, 8x8 ... at or below one tile: the half-resolution passes get NO workgroup, as the reference's own `(size + 7) / 8 / (2, 1)`
                    gives them none — the composed frame is all zero, and the product owes exactly those zeros
  9x9, 17x9 ....... two and three tile columns; column 16 of 17x9 lies in the dropped half-resolution column
  41x23 ........... 6 tile columns: even, not a multiple of 4 — the last block has two idle waves
  72x40 ........... 9 tile columns (odd)
  197x101 ......... 25 tile columns, clipped by 5 pixels both ways; 7x7 a-trous blocks, the last ones clipped
  41x296, 72x296 .. 37 tile rows = one full 32-row chunk plus 5; 19 a-trous block rows = one full chunk of 16 plus 3; groups_x 2 and 3

EXACT build: every float plane, the composed frame and the ray count equal the oracle's bit for bit after each of 8 frames (every GI
schedule). FAST build (what ships): the oracle's state in, one launch or one whole unmasked frame out (test_gpu_fast_steady_state._run),
held to
  1. status and finiteness — every render returns OK, every compared lane is finite where the oracle's is (but for the (NaN, NaN) the
     reference's own octahedral code makes of a zero normal, which every empty GI reservoir of the oracle holds: a pixel that flipped to
     such a record is an outlier under 3 and 4);
  2. coverage — the output tensor is filled with a NaN pattern the renderer cannot produce before each unmasked frame, none is left;
  3. STRUCTURE — a condition, not a measurement: a flipped discrete choice is an isolated pixel (for filtered planes a small cluster
     around one), a geometry fault fills a region. The per-pixel outlier mask (any lane of the pixel outside RTOL / ATOL) covers at most
     half of any region of `regions()`;
  4. the pinned fractions (BAD_FRACTION launch by launch, _check_whole_rows for whole frames) at the shapes of about the pixel count
     those were calibrated at.
The camera stands INSIDE the Cornell box (inside_camera): cornell.rs's own sees sky beside the box in wide frames, and edge tiles full of sky
test nothing; one exact case looks up at the ceiling instead (ceiling_camera says why). test_oracle_preconditions (CPU) asserts on the oracle alone that every shape used here has a surface in
every pixel and light in every region.

Measured on one MI355X (profiles/frame_shapes.json): launch by launch at most 1.5e-4 of a plane's lanes outside the tolerance (gate 2e-3), after a
whole frame 3.0e-4 on discrete planes (2e-3) and 2.2e-3 on filtered ones (5e-3), PSNR >= 74.5 dB (70); the outlier mask never covered more than
0.08 of a region (0.5). No shape had to grow. The lean frame did fail here at first: on odd tracing frames kLeanGiRes2 left the last pixel of
every other row of an odd-width frame (9x9, 41x23, 197x101) with a stale GI_RESERVOIRS_2 record (st_render.cpp `kLeanGiRes2`).
"""
import json
import math

import numpy as np
import pytest

from oracle_binding import OracleEngine
from parity import assert_bits_equal
from strolle_amd import Buffer, CameraMode, Engine, Light, scenes
from test_gpu_fast_steady_state import FILTERED, _check_whole_rows, _run, inside_camera
from test_gpu_fast_tolerance import ATOL, BAD_FRACTION, REPORT_ONLY, RTOL
from test_gpu_parity import ALL_FLOAT_BUFFERS, _torch

gpu = pytest.mark.gpu
FRAMES = 8   # every GI schedule of the 6-frame cycle, and the first frame of the next
SEED = 11

BUILD = {"cornell": scenes.build_cornell, "dungeon": scenes.build_dungeon,
         "soup": lambda e: scenes.build_random_soup(e, 1500, seed=2, n_lights=5)}


def ceiling_camera(size, mode=CameraMode.IMAGE, denoise=True, depth=0):
    """Under the Cornell box's ceiling, looking up: the ceiling fills the frame, so the left and the right frame edge show one plane at the same
    depth (red wall's bounce light on one side, the green wall's on the other). Under inside_camera they show the box's furniture and its side
    walls, whose depths and normals make the a-trous edge-stopping weights reject a texel staged from the wrong side of the frame; here such a
    texel passes them, so a halo that is not clipped to the viewport changes the filtered colours."""
    return scenes.camera_for(size, (0.0, 1.2, 0.2), (0.0, 2.0, 0.199), mode, denoise, depth)


BUILD["cornell_ceiling"] = scenes.build_cornell
CAMERA = {"cornell": inside_camera, "dungeon": scenes.dungeon_camera, "soup": inside_camera, "cornell_ceiling": ceiling_camera}

NO_HALF_RES = [(1, 1), (7, 5), (8, 8)]   # width <= 8: the half-resolution passes have no workgroup
CORNELL_SHAPES = NO_HALF_RES + [(9, 9), (17, 9), (41, 23), (72, 40), (197, 101), (41, 296), (72, 296)]
EXACT_CASES = [("cornell", s) for s in CORNELL_SHAPES] + [("dungeon", (197, 101)), ("dungeon", (41, 23)), ("soup", (41, 23)),
                                                               ("cornell_ceiling", (197, 101))]


# ---- regions -------------------------------------------------------------------------------------------------------------------------

def tile_grid(w, h):
    """8x8 tiles, one per wave (st_device.h tile_for_block)"""
    return (w + 7) // 8, (h + 7) // 8


def block_grid(w, h):
    """32x16 blocks of the LDS-staged a-trous passes (k_denoise.hip wavelet_block)"""
    return (w + 31) // 32, (h + 15) // 16


def _spans(n, step, join_clipped):
    """[(start, end)] of `step`-sized pieces of 0..n; with join_clipped a shorter last piece is joined to its inner neighbour"""
    edges = list(range(0, n, step)) + [n]
    spans = list(zip(edges[:-1], edges[1:]))
    if join_clipped and len(spans) > 1 and spans[-1][1] - spans[-1][0] < step:
        spans[-2:] = [(spans[-2][0], n)]
    return spans


def regions(w, h):
    """{class: [(name, x0, y0, x1, y1)]} — the pieces of a w x h frame one geometry fault would fill:
      tiles ..... every 8x8 tile, clipped to the frame
      blocks .... every 32x16 a-trous block, a clipped one joined to its inner neighbour (a filter footprint spreads one flip over a few pixels:
                  a 5-pixel-wide block of its own could be half covered by one)
      bands ..... the full-height columns 16 * (tiles_x // 2) .. w - 1 the half-resolution passes do not own when tiles_x is odd or the last tile
                  is clipped, and the full-width clipped tile row
      borders ... the first and last row and column
    A frame of fewer than 256 pixels (four tiles, one block's width) is ONE region."""
    if w * h < 256:
        return {"frame": [("frame", 0, 0, w, h)]}
    tiles_x = tile_grid(w, h)[0]
    out = {"tiles": [(f"tile {x0 // 8},{y0 // 8}", x0, y0, x1, y1) for y0, y1 in _spans(h, 8, False) for x0, x1 in _spans(w, 8, False)],
           "blocks": [(f"block {x0 // 32},{y0 // 16}", x0, y0, x1, y1) for y0, y1 in _spans(h, 16, True) for x0, x1 in _spans(w, 32, True)],
           "bands": [],
           "borders": [("first row", 0, 0, w, 1), ("last row", 0, h - 1, w, h), ("first column", 0, 0, 1, h), ("last column", w - 1, 0, w, h)]}
    if (tiles_x % 2 or w % 8) and 16 * (tiles_x // 2) < w:
        out["bands"].append(("columns past the last whole 16-pixel tile", 16 * (tiles_x // 2), 0, w, h))
    if h % 8:
        out["bands"].append(("clipped tile row", 0, 8 * (h // 8), w, h))
    return out


COARSE = ("blocks", "bands", "borders", "frame")   # what applies to filtered planes and the composed frame after a whole frame


def worst_region(mask, classes=None):
    """(share, class, name) of the region of `mask` ([h, w] bool) with the largest share of set pixels"""
    h, w = mask.shape
    worst = (0.0, None, None)
    for cls, regs in regions(w, h).items():
        if classes is not None and cls not in classes:
            continue
        for name, x0, y0, x1, y1 in regs:
            share = float(mask[y0:y1, x0:x1].mean())
            if share > worst[0]:
                worst = (share, cls, name)
    return worst


# ---- the oracle, once per case ---------------------------------------------------------------------------------------------------------

def _orbit(size, frame):
    """camera of the motion cases: 0.02 rad per frame about the look-at point, on the inside camera's radius"""
    a = 0.02 * frame
    return scenes.camera_for(size, (0.9 * math.sin(a), 1.0, 0.9 * math.cos(a)), (0.0, 1.0, 0.0))


def _moving_light(frame):
    """the light of test_gpu_parity.test_moving_camera_and_light_bit_exact"""
    t = 0.05 * frame
    return Light.point((math.sin(t) / 2.0, 1.5, math.cos(t) / 2.0), 0.15, (50.0 / (4 * math.pi),) * 3, 20.0)


def _drive(e, cam, scene, size, mode, denoise, motion, frame):
    desc = _orbit(size, frame) if motion else CAMERA[scene](size, mode, denoise=denoise)
    if motion:
        e.insert_light(1, _moving_light(frame))
    e.update_camera(cam, desc)
    e.tick()


_oracle = {}


def oracle_frames(scene, size, mode=CameraMode.IMAGE, denoise=True, motion=False):
    """[(planes, composed frame, ray count)] after each of FRAMES frames; computed once per case and left unchanged"""
    key = (scene, size, int(mode), denoise, motion)
    if key not in _oracle:
        o = OracleEngine()
        BUILD[scene](o); o.set_seed(SEED)
        cam = o.create_camera(CAMERA[scene](size, mode, denoise=denoise))
        rows = []
        for frame in range(FRAMES):
            _drive(o, cam, scene, size, mode, denoise, motion, frame)
            ref = np.array(o.render_camera(cam), copy=True)
            planes = {b: o.read_buffer(cam, b) for b in ALL_FLOAT_BUFFERS}
            for a in list(planes.values()) + [ref]:
                a.setflags(write=False)
            rows.append((planes, ref, o.ray_count(cam)))
        o.close()
        _oracle[key] = rows
    return _oracle[key]


def _exact_against_oracle(scene, size, mode=CameraMode.IMAGE, denoise=True, motion=False, tuning=None):
    """The exact build, frame by frame: all float planes, the composed frame and the ray count equal the oracle's bits."""
    torch = _torch()
    want = oracle_frames(scene, size, mode, denoise, motion)
    prod = Engine(device=0, exact=True)
    assert prod.exact
    if tuning:
        prod.set_tuning(**tuning)
        t = prod.tuning()
        assert all(getattr(t, k) == v for k, v in tuning.items()), "set_tuning did not take"
    BUILD[scene](prod); prod.set_seed(SEED)
    cam = prod.create_camera(CAMERA[scene](size, mode, denoise=denoise))
    out = torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda:0")
    for frame, (planes, ref, rays) in enumerate(want):
        _drive(prod, cam, scene, size, mode, denoise, motion, frame)
        prod.render_camera(cam, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for b in ALL_FLOAT_BUFFERS:
            assert_bits_equal(prod.read_buffer(cam, b), planes[b], f"{scene} {size[0]}x{size[1]} frame {frame} buffer {b.name}")
        assert_bits_equal(out.cpu().numpy(), ref, f"{scene} {size[0]}x{size[1]} composed frame {frame}")
        assert prod.ray_count(cam) == rays, f"{scene} {size[0]}x{size[1]} frame {frame}: ray count {prod.ray_count(cam)}, the oracle's {rays}"
    prod.close()


# ---- CPU: what the GPU tests rest on ------------------------------------------------------------------------------------------------------

def test_region_builder():
    assert tile_grid(197, 101) == (25, 13) and block_grid(197, 101) == (7, 7)
    r = regions(197, 101)
    assert len(r["tiles"]) == 25 * 13
    assert r["tiles"][24][1:] == (192, 0, 197, 8) and r["tiles"][-1][1:] == (192, 96, 197, 101)          # the last ones 5 wide / 5 high
    assert len(r["blocks"]) == 6 * 6 and r["blocks"][5][1:] == (160, 0, 197, 16) and r["blocks"][-1][1:] == (160, 80, 197, 101)   # 7x7, the clipped ones joined inwards
    assert [b[1:] for b in r["bands"]] == [(192, 0, 197, 101), (0, 96, 197, 101)]
    assert [b[1:] for b in r["borders"]] == [(0, 0, 197, 1), (0, 100, 197, 101), (0, 0, 1, 101), (196, 0, 197, 101)]
    covered = np.zeros((101, 197), np.int32)
    for cls in ("tiles", "blocks"):
        for _, x0, y0, x1, y1 in r[cls]:
            covered[y0:y1, x0:x1] += 1
    assert (covered == 2).all()                                                                           # each a partition of the frame
    assert regions(8, 8) == {"frame": [("frame", 0, 0, 8, 8)]} and list(regions(17, 9)) == ["frame"]
    r = regions(72, 40)       # 9 tile columns: the half-resolution passes own 4 tiles of 16
    assert [b[1:] for b in r["bands"]] == [(64, 0, 72, 40)] and len(r["blocks"]) == 2 * 2 and r["blocks"][1][1:] == (32, 0, 72, 16)
    r = regions(41, 296)      # 6 tile columns (even), the last clipped to 1 pixel: 3 tiles of 16 reach past the frame, no column is left over
    assert r["bands"] == [] and len(r["blocks"]) == 1 * 18 and len(r["tiles"]) == 6 * 37
    assert [b[1:] for b in regions(41, 23)["bands"]] == [(0, 16, 41, 23)]
    m = np.zeros((101, 197), bool); m[96:, 192:] = True
    assert worst_region(m) == (1.0, "tiles", "tile 24,12") and worst_region(m, COARSE)[0] == pytest.approx(5 / 101)   # the 5-wide band, and the last column


@pytest.mark.parametrize("scene,size", EXACT_CASES, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_oracle_preconditions(scene, size):
    """The oracle alone, Image{denoise}, after 7 frames: the surface is present in every pixel; for widths above 8 at least 0.99 of the
    composed pixels are lit, with lit pixels in every region; for widths of 8 or less NONE is (no half-resolution workgroup).
    The random soup cannot cover a frame (measured: 0.890 of 41x23 has a surface, 0.884 is lit): it is held to light in every region only."""
    planes, ref, _ = oracle_frames(scene, size)[6]
    w, h = size
    surface = planes[Buffer.PRIM_SURFACE_MAP_A].reshape(h, w, 4)[..., 2] != 0
    lit = (ref[..., :3] > 0).any(axis=-1)
    if scene != "soup":
        assert surface.all(), f"{1.0 - surface.mean():.3f} of the pixels see no surface"
    if w <= 8:
        assert not ref[..., :3].any(), "the reference gives its half-resolution passes a workgroup at this width after all"
        return
    if scene != "soup":
        assert lit.mean() >= 0.99, f"lit fraction {lit.mean():.3f}"
    for cls, regs in regions(w, h).items():
        for name, x0, y0, x1, y1 in regs:
            assert lit[y0:y1, x0:x1].any(), f"{cls} {name}: no lit pixel"
            assert scene == "soup" or surface[y0:y1, x0:x1].all()


# ---- exact build: bits ----------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("scene,size", EXACT_CASES, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_exact_build_every_plane_every_frame(scene, size):
    _exact_against_oracle(scene, size)


@gpu
@pytest.mark.parametrize("size", [(197, 101), (72, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_build_under_motion(size):
    """The camera orbits the look-at point by 0.02 rad per frame and the light moves: reprojected positions cross the clipped edges."""
    _exact_against_oracle("cornell", size, motion=True)


@gpu
@pytest.mark.parametrize("size", [(72, 296), (41, 296)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("tile_map_denoise", [0, 1, 2])
@pytest.mark.parametrize("tile_map", [0, 1, 2])
def test_exact_build_every_workgroup_mapping(tile_map, tile_map_denoise, size):
    """Taller than one 256-row chunk with a tile-column count that is no multiple of 4: the chunk remap of mode 2 is live (a full chunk and a
    ragged tail), which it is on no other small frame of the suite."""
    _exact_against_oracle("cornell", size, tuning={"tile_map": tile_map, "tile_map_denoise": tile_map_denoise})


@gpu
@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("mode", [CameraMode.GI_DIFFUSE, CameraMode.DI_SPECULAR], ids=lambda m: m.name)
def test_exact_build_partial_modes_odd_tile_columns(mode, denoise):
    _exact_against_oracle("cornell", (72, 40), mode=mode, denoise=denoise)


# ---- fast build: structure -------------------------------------------------------------------------------------------------------------------

# engine frame numbers; f % 6 < 4 is a tracing frame (even f samples, odd f resamples spatially), else validation
PLAN = {7: "launches", 8: "launches", 9: "whole", 10: "whole", 11: "launches", 12: "whole", 13: "whole_keep"}
PLAN_TINY = {f: "whole" for f in range(1, 9)}
PLAN_TINY_KEEP = {f: "whole_keep" for f in range(1, 9)}
UNWRITTEN = 0x7FD5A5C3   # a quiet NaN with a payload: arithmetic yields the default NaN (payload 0), and the renderer copies no NaN from its inputs
STATISTICAL = [("cornell_inside", (197, 101), "host"), ("cornell_inside", (72, 296), "host"), ("dungeon", (197, 101), "host"), ("dungeon", (197, 101), "device")]
TINY = [(1, 1), (8, 8), (9, 9), (17, 9), (41, 23), (72, 40)]


def _check_structure(rep, what, size):
    """assertions 1-3 of the module's docstring on one _run(..., masks=True, fill_bits=UNWRITTEN) report"""
    assert rep["compared"] > 0, "nothing compared"
    shares = {}
    for frame, lanes in rep["unwritten"]:
        assert lanes == 0, f"{what} frame {frame}: {lanes} lanes of the output tensor were not written"
    for r in rep["masks"]:
        where = f"{what} frame {r['frame']} {r['launch'] or r['kind']}: {r['plane']}"
        assert r["nonfinite_lanes"] == 0, f"{where}: {r['nonfinite_lanes']} lanes not finite where the oracle's are\n{r['diagnose']}"
        coarse = r["launch"] is None and (r["plane"] == "composed frame" or r["plane"] in {b.name for b in FILTERED})
        share, cls, name = worst_region(r["mask"], COARSE if coarse else None)
        key = ("filtered, whole frame" if coarse else "launch by launch" if r["launch"] else "discrete, whole frame")
        shares[key] = max(shares.get(key, 0.0), share)
        assert share <= 0.5, f"{where}: {share:.2f} of {cls} '{name}' outside rtol {RTOL} / atol {ATOL} — a region, not isolated flips\n{r['diagnose']}"
    print("largest region share per plane class:", json.dumps({what: shares}))   # (profiles/frame_shapes.json holds a run's figures)


@gpu
@pytest.mark.parametrize("scene,size,tree", STATISTICAL, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_fast_build_launches_and_whole_frames(scene, size, tree):
    """Launch by launch on one frame of each GI schedule, whole lean frames of each, one frame with every plane kept: structure, and the
    pinned fractions (about the pixel count BAD_FRACTION was calibrated at; measured figures in profiles/frame_shapes.json)."""
    rep = _run(scene, size, PLAN, tree=tree, masks=True, fill_bits=UNWRITTEN)
    what = f"{scene} {size[0]}x{size[1]} {tree} tree"
    if tree == "device":
        assert rep["tree"]["device_builds"] >= 1, "the first tree was not built on the device"
    assert {r["frame"] for r in rep["launches"]} <= {7, 8, 11}
    assert {(r["frame"], r["kind"]) for r in rep["whole"]} == {(9, "whole"), (10, "whole"), (12, "whole"), (13, "whole_keep")}
    _check_structure(rep, what, size)
    for r in rep["launches"]:
        assert REPORT_ONLY or r["bad_fraction"] <= BAD_FRACTION, f"{what} frame {r['frame']} launch {r['launch']}: plane {r['plane']}: {r['bad_fraction']:.2e} of the lanes outside rtol {RTOL} / atol {ATOL}"
    _check_whole_rows(rep["whole"], what)


@gpu
@pytest.mark.parametrize("plan", [PLAN_TINY, PLAN_TINY_KEEP], ids=["lean", "keep_all_planes"])
@pytest.mark.parametrize("size", TINY, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fast_build_tiny_whole_frames(size, plan):
    """Whole unmasked frames 1..8 from the oracle's state at one pixel, one tile, two and three tile columns, an idle-wave block and an odd
    tile-column count: too few pixels for a fraction, so structure only. At widths <= 8 the composed frame is the reference's zeros."""
    rep = _run("cornell_inside", size, plan, masks=True, fill_bits=UNWRITTEN)
    assert {r["frame"] for r in rep["whole"]} == set(plan)
    _check_structure(rep, f"cornell_inside {size[0]}x{size[1]} {'keep' if plan is PLAN_TINY_KEEP else 'lean'}", size)
