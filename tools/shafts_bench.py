#!/usr/bin/env python3
"""Light shafts (include/strolle_hip.h "light shafts"; k_shafts.hip): the reference side's figures and the cost. Every run MERGES into --out.

  --reference           CPU only: the restatement (tests/shafts_ref.py shafts_f32) with visibility from the checker's occlusion probe
                        against the float64 definition with brute-force visibility (shafts_f64), on both slat scenes over the GPU test's
                        case matrix (tests/shafts_cases.py). Fixes the ambiguity threshold (the smallest margin above every shadow ray the
                        probe and brute force decide differently, never below 16 float32 roundings) and the tolerance (4 x the worst
                        deviation on non-ambiguous pixels), and reports the shares of ambiguous and of mixed (lit and shadowed) cells.
  (default)             ms per frame of Cornell and the dungeon at 1920x1080 Image{denoise} into RGBA8 sRGB with ACES, fast build, interleaved
                        twice: off, sun, sun + two lights, divisor 1 against 2, steps 8 / 16 / 32, and the whole chain behind it.
  --yardstick           the march against the project's own walk: st_light_shafts_process (march + apply) and st_scene_occluded over the
                        identical ray set (the restatement's rays uploaded as StRay records) in the same run, dungeon, 1080p depth from a frame.
  --kernel-stats        one `rocprofv3 --kernel-trace --stats` child run of its own (no counters) on the serial schedule: the two launches' times.
  --profile-child       what that run wraps.
  --abab PARENT         A B B A (three times) of bench.py with the feature off: PARENT/bench.py (the parent commit, built) against this tree's.

  python tools/shafts_bench.py [--out profiles/light_shafts.json] [--reference | --yardstick | --kernel-stats | --profile-child | --abab DIR]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))   # (the tests load this file by its path)

from chain_bench import BLOOM, BLUR, DOF, FOG, FRAMES, HD, WARMUP, abab, camera, kernel_stats, merge, run_frames  # noqa: E402

PROFILE = os.path.join(ROOT, "profiles", "light_shafts.json")
THRESHOLD_FLOOR = 16 * 2.0 ** -24
MEDIUM = dict(density=0.05, anisotropy=0.6, max_distance=40.0, intensity=1.0, scatter=(0.9, 0.9, 0.9))
SUN = dict(sun_color=(4.0, 3.5, 3.0), sun_direction=(0.3, 0.8, 0.2))
CHAIN = dict(set_fog=FOG, set_dof=DOF, set_motion_blur=BLUR, set_bloom=BLOOM, set_post=dict(fxaa=True))
# name: (desc keywords or None, lights taken from the scene, the chain behind it)
VARIANTS = {
    "off": (None, 0, False),
    "sun_d2_s16": (dict(steps=16, divisor=2, **MEDIUM, **SUN), 0, False),
    "sun_2lights_d2_s16": (dict(steps=16, divisor=2, **MEDIUM, **SUN), 2, False),
    "sun_d1_s16": (dict(steps=16, divisor=1, **MEDIUM, **SUN), 0, False),
    "sun_d2_s8": (dict(steps=8, divisor=2, **MEDIUM, **SUN), 0, False),
    "sun_d2_s32": (dict(steps=32, divisor=2, **MEDIUM, **SUN), 0, False),
    "sun_2lights_d2_s16_fog_dof_motion_blur_bloom_fxaa": (dict(steps=16, divisor=2, **MEDIUM, **SUN), 2, True),
}
SCENE_LIGHTS = {"cornell": (1,), "dungeon": (1, 3)}


def round_up(x, digits=3):
    """x rounded up to `digits` significant digits: a committed figure that a re-measurement reproduces exactly"""
    if x == 0:
        return 0.0
    from math import ceil, floor, log10
    q = 10.0 ** (floor(log10(abs(x))) - digits + 1)
    return float("%.*g" % (digits, ceil(x / q) * q))


# ---------------------------------------------------------------- the reference side (CPU)
_reference = {}


def reference_scene(scene):
    """every case of the matrix on one slat scene: the restatement with the probe's visibility, the definition, the margins; computed once"""
    if scene in _reference:
        return _reference[scene]
    import shafts_cases as K
    import shafts_ref as R
    import walk_ref
    from geometry_extremes import oracle_trace
    from oracle_binding import OracleEngine
    orac = OracleEngine()
    out = {}
    try:
        K.build_slats(orac, K.SCENES[scene]); orac.tick()
        tris = orac.read_scene(1).copy()
        recs = walk_ref.records(tris)
        for name, size, kind, d in K.cases():
            img, z, M, P = K.inputs(size, kind)
            lights = K.table_lights(d)
            det = {}
            got, n_rays = R.shafts_f32(img, z, M, P, d, lights, lambda r: oracle_trace(orac, r)[4], details=det)
            want, pix_margin = R.shafts_f64(img, z, M, P, d, lights, tris)
            ch, cw = det["cells"].shape[:2]
            cell_margin = np.full(ch * cw, np.inf); lit = np.zeros(ch * cw, bool); dark = np.zeros(ch * cw, bool)
            worst_disagreement = 0.0
            for cells, k, li, rays, occ in det["log"]:
                a = walk_ref.trace(*recs, rays)
                np.minimum.at(cell_margin, cells, a.decision_margin)
                lit[cells[~occ]] = True; dark[cells[occ]] = True
                bad = a.occluded != occ
                if bad.any():
                    worst_disagreement = max(worst_disagreement, float(a.decision_margin[bad].max()))
            out[name] = dict(got=got, want=want, pix_margin=pix_margin, cell_margin=cell_margin.reshape(ch, cw), live=det["live"], mixed=(lit & dark).reshape(ch, cw),
                             changed=det["changed"], rays=n_rays, worst_disagreement=worst_disagreement, divisor=int(d.divisor), depth=z, desc=d)
    finally:
        orac.close()
    _reference[scene] = dict(cases=out, triangles=int(len(recs[0])))
    return _reference[scene]


def pixel_cell_margin(c):
    """per pixel, the smallest margin of the cells its S is made of (both statements' rays)"""
    m, div = c["cell_margin"], c["divisor"]
    h, w = c["depth"].shape
    if div == 1:
        pm = m.copy()
    else:
        ch, cw = m.shape
        pad = np.pad(m, 1, mode="edge")
        nb = np.minimum.reduce([pad[dy:dy + ch, dx:dx + cw] for dy in range(3) for dx in range(3)])   # the bilinear footprint lies within the 3 x 3 cells around the pixel's own
        pm = np.repeat(np.repeat(nb, 2, 0), 2, 1)[:h, :w]
    return np.minimum(pm, c["pix_margin"])


def deviation(got, want):
    """|restatement - definition| / max(1, |definition|) per channel, NaN where either is not finite (inputs hold NaN and infinities)"""
    with np.errstate(all="ignore"):
        g, w = got[..., :3].astype(np.float64), want
        dev = np.abs(g - w) / np.maximum(1.0, np.abs(w))
    return np.where(np.isfinite(g) & np.isfinite(w), dev, np.nan)


def measure_reference(scene):
    ref = reference_scene(scene)
    worst = max([THRESHOLD_FLOOR] + [c["worst_disagreement"] for c in ref["cases"].values()])
    thr = round_up(float(np.nextafter(worst, np.inf))) if worst > THRESHOLD_FLOOR else THRESHOLD_FLOOR
    live = amb = mixed = 0
    worst_dev, where = 0.0, None
    for name, c in ref["cases"].items():
        live += int(c["live"].sum()); amb += int((c["live"] & (c["cell_margin"] < thr)).sum()); mixed += int((c["live"] & c["mixed"]).sum())
        sure = pixel_cell_margin(c) >= thr
        dev = deviation(c["got"], c["want"])[sure]
        if dev.size and np.nanmax(dev, initial=0.0) > worst_dev:
            worst_dev, where = float(np.nanmax(dev)), name
    return dict(triangles=ref["triangles"], threshold=thr, tolerance=round_up(4.0 * worst_dev), worst_deviation=float("%.3e" % worst_dev), worst_case=where,
                ambiguous_cell_share=round(amb / max(live, 1), 5), mixed_cell_share=round(mixed / max(live, 1), 5), cells=live,
                shadow_rays=int(sum(c["rays"] for c in ref["cases"].values())), probe_disagreements_worst_margin=float("%.3e" % worst))


# ---------------------------------------------------------------- the cost (GPU)
def frames_ms(scene, shafts, n_lights, chain, **kw):
    settings = dict(set_light_shafts=dict(shafts, lights=SCENE_LIGHTS[scene][:n_lights]) if shafts else None, **(CHAIN if chain else {}))
    return run_frames(scene, settings, moving=chain, **kw)


def yardstick():
    """the march against st_scene_occluded over the same rays, dungeon at 1080p, sun only, divisor 2, 16 steps"""
    import torch
    import shafts_ref as R
    from strolle_amd import Buffer, Engine, light_shafts_desc, scenes
    from strolle_amd.api import RAY_DTYPE
    e = Engine(device=0)
    scenes.build_dungeon(e); e.set_seed(7)
    cam_desc = camera("dungeon", 0, False)
    cam = e.create_camera(cam_desc)
    w, h = HD
    out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    e.tick(s); e.render_camera(cam, out.data_ptr(), s); torch.cuda.synchronize()
    g0 = e.read_buffer(cam, Buffer.PRIM_GBUFFER_D0_A).reshape(h, w, 4)[..., 0]
    z = np.where(g0 == 0, np.finfo(np.float32).max, g0).astype(np.float32)
    d = light_shafts_desc(steps=16, divisor=2, **MEDIUM, **SUN)
    M = np.asarray(cam_desc.transform, np.float32).T.reshape(-1); P = np.asarray(cam_desc.projection, np.float32).T.reshape(-1)
    det = {}
    R.march_f32(z, M, P, d, [], lambda r: np.zeros(len(r), bool), details=det)   # which rays are cast does not depend on what they hit
    rays = np.concatenate([x[3] for x in det["log"]]).astype(RAY_DTYPE)
    tr, tz, tc = torch.from_numpy(rays.view(np.uint8)).cuda(), torch.from_numpy(z).cuda(), out
    occ = torch.zeros(len(rays), dtype=torch.int32, device="cuda:0")
    dst = torch.zeros_like(out)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    series = {"march_plus_apply_ms": [], "scene_occluded_ms": []}
    for rep in range(6):   # interleaved; the first pair warms up
        for key, call in (("march_plus_apply_ms", lambda: e.light_shafts_process(d, M, P, tc.data_ptr(), tz.data_ptr(), w, h, dst.data_ptr(), 0, stream=s)),
                          ("scene_occluded_ms", lambda: e.occluded(tr.data_ptr(), len(rays), occ.data_ptr(), s))):
            torch.cuda.synchronize(); ev[0].record(); call(); ev[1].record(); torch.cuda.synchronize()
            if rep:
                series[key].append(round(ev[0].elapsed_time(ev[1]), 4))
    e.close()
    return {"yardstick_dungeon_1080p_sun_d2_s16": {"rays": int(len(rays)), **series, "note": "the query also moves 36 B a ray through HBM; the process call includes the apply launch"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=PROFILE)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--yardstick", action="store_true")
    ap.add_argument("--profile-child", action="store_true")
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--abab")
    args = ap.parse_args()
    if args.reference:
        import shafts_cases as K
        merge(args.out, {"reference": {scene: measure_reference(scene) for scene in K.SCENES},
                         "reference_note": "threshold: a cell is ambiguous when any of its shadow rays has walk_ref's decision_margin below it. tolerance: 4 x the worst "
                                           "|shafts_f32 (probe visibility) - shafts_f64 (brute force)| / max(1, |shafts_f64|) over the pixels none of whose cells is ambiguous."})
        return
    import torch  # noqa: F401  (before the library: torch's bundled HIP runtime has to be the first one loaded)
    if args.abab:   # A B B A three times: neither side always runs second
        merge(args.out, abab(args.abab, "shafts_off", order=("parent", "this", "this", "parent") * 3, order_note="parent this this parent, three times"))
        return
    if args.yardstick:
        merge(args.out, yardstick())
        return
    if args.profile_child:
        shafts, n, _ = VARIANTS["sun_2lights_d2_s16"]
        frames_ms("dungeon", shafts, n, False, frames=30, warmup=10, serial=True)
        return
    if args.kernel_stats:
        out = kernel_stats(__file__, ["--profile-child"], {"k_shafts_march": None, "k_shafts_apply": None}, None, "shafts")
        merge(args.out, {"kernel_stats_dungeon_1080p_sun_2lights_d2_s16_serial_schedule": out})
        return
    rec = {"render_size": list(HD), "mode": "Image{denoise}", "format": "RGBA8_UNORM_SRGB", "display": "ACES_FITTED", "build": "fast", "frames": FRAMES, "warmup": WARMUP,
           "medium": {k: list(v) if isinstance(v, tuple) else v for k, v in {**MEDIUM, **SUN}.items()}}
    for scene in ("cornell", "dungeon"):
        rec[scene + "_ms_per_frame"] = {}
        for _ in range(2):   # interleaved twice: the spread of one box
            for name, (shafts, n, chain) in VARIANTS.items():
                rec[scene + "_ms_per_frame"].setdefault(name, []).append(round(frames_ms(scene, shafts, n, chain), 4))
    merge(args.out, rec)


if __name__ == "__main__":
    main()
