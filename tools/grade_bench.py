#!/usr/bin/env python3
"""Cost of colour grading (include/strolle_hip.h "colour grading"; k_grade.hip) in the default (fast) build. Every run MERGES its figures
into --out.

  (default)  (a) ms per frame of Cornell and the dungeon at 1920x1080 Image{denoise} into RGBA8 sRGB with ACES: grading off, stage A + the
             CDL, + a 33^3 table, + dither, and the whole chain (fog, depth of field, motion blur, bloom, the grade, FXAA under a moving
             camera) — FRAMES frames after WARMUP, events around the whole run on one stream, interleaved twice;
             (b) the copy ceiling (st_debug_copy_bandwidth) and the launch's compulsory bytes (st_grade.cpp grade_step).
  --restatement         CPU only: the worst deviation of the numpy restatement from the float64 definition over the tests' input matrix
                        (tests/test_color_grading_abi.py restatement_vs_definition), the figure the tests' bound is four times of.
  --kernel-stats        one `rocprofv3 --kernel-trace --stats` child run of its own (no counters), on the serial schedule (a launch's time is
                        its own): the grade launch per dispatch against bytes / copy ceiling for each variant, table sides 17, 33 and 65, and
                        the fog launch — the yardstick: it moves the same bytes — re-measured in the same run.
  --profile-child       what that run wraps.
  --abab PARENT         A B A B A B of bench.py (the headline and the dungeon at 1080p): PARENT/bench.py (the parent commit, built) against this tree's.

  python tools/grade_bench.py [--out profiles/grading.json] [--restatement | --kernel-stats | --profile-child | --abab DIR]
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # grade_ref.py, grade_cases.py, test_color_grading_abi.py: the restatement's deviation

from chain_bench import BLOOM, BLUR, DOF, FOG, FRAMES, HD, WARMUP, abab, camera, dispatch_record, dispatch_us, kernel_trace, merge  # noqa: E402

A_CDL = dict(temperature=0.2, tint=-0.1, contrast=1.15, saturation=1.1, slope=(1.05, 1.0, 0.95), offset=(0.01, 0.0, -0.01), power=(1.1, 1.0, 0.9), cdl_saturation=0.95)
LUT_ID = 9
# name: (descriptor keywords or None, table side or 0, the rest of the chain under a moving camera)
VARIANTS = {"off": (None, 0, False), "a_cdl": (A_CDL, 0, False), "a_cdl_lut33": (A_CDL, 33, False), "a_cdl_lut33_dither": (dict(A_CDL, dither=True), 33, False),
            "dither_only": (dict(dither=True), 0, False), "fog_dof_motion_blur_bloom_grade_fxaa": (dict(A_CDL, dither=True), 33, True)}
CHAIN = dict(set_fog=FOG, set_dof=DOF, set_motion_blur=BLUR, set_bloom=BLOOM, set_post=dict(fxaa=True))
# the child run's sequence: (descriptor keywords, table side); then fog alone
CHILD = [("a_cdl", A_CDL, 0), ("dither_only", dict(dither=True), 0), ("a_cdl_dither_lut17", dict(A_CDL, dither=True), 17), ("a_cdl_dither_lut33", dict(A_CDL, dither=True), 33),
         ("a_cdl_dither_lut65", dict(A_CDL, dither=True), 65)]
CHILD_FRAMES, CHILD_WARMUP = 30, 10


def table(n):
    """a smooth, non-trivial look: a per-channel curve with some cross-talk"""
    import numpy as np
    g = np.linspace(0.0, 1.0, n)
    b, gg, r = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([r ** 0.9 * 0.95 + 0.05 * gg, gg ** 1.1, 0.9 * b + 0.1 * r * gg], -1).astype(np.float32)


def frames_ms(scene, grade, side, chain, frames=FRAMES, warmup=WARMUP, serial=False, fog_only=False):
    """chain_bench.run_frames with a table inserted in front of the first tick (a table needs the engine: not a camera setter)"""
    import torch
    from strolle_amd import Engine, OutputFormat, Tonemap, scenes
    e = Engine(device=0)
    if serial:
        e.set_tuning(overlap=0)
    (scenes.build_cornell if scene == "cornell" else scenes.build_dungeon)(e)
    e.set_seed(7)
    cam = e.create_camera(camera(scene, 0, chain))
    e.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
    e.set_display(cam, tonemap=Tonemap.ACES_FITTED)
    if chain:
        for setter, s in CHAIN.items():
            getattr(e, setter)(cam, **s)
    if fog_only:
        e.set_fog(cam, **FOG)
    if side:
        e.insert_lut(LUT_ID, table(side))
    if grade is not None:
        e.set_color_grading(cam, lut=LUT_ID if side else 0, **grade)
    w, h = e.output_size(cam)
    out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in range(warmup + frames):
        if k == warmup:
            torch.cuda.synchronize(); a.record(s)
        if chain:
            e.update_camera(cam, camera(scene, k, True))
        e.tick(s.cuda_stream)
        e.render_camera(cam, out.data_ptr(), s.cuda_stream)
    b.record(s); torch.cuda.synchronize()
    e.close()
    return a.elapsed_time(b) / frames


def launch_bytes(w, h, out_bytes=4):
    return {"k_grade": w * h * (16 + out_bytes), "k_fog": w * h * (20 + out_bytes)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grading.json"))
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--profile-child", action="store_true")
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--abab")
    args = ap.parse_args()
    if args.restatement:
        import grade_cases
        from test_color_grading_abi import restatement_vs_definition
        worst, where, pixels = restatement_vs_definition()
        merge(args.out, {"restatement_vs_definition": {"worst": float("%.3e" % worst), "case": where, "pixels": pixels, "cases": len(grade_cases.cases()),
                                                       "metric": "max |grade_f32 - grade_f64| / max(1, the definition's largest channel of the pixel), unspoiled inputs, every pixel"}})
        return
    import torch  # noqa: F401  (before the library: torch's bundled HIP runtime has to be the first one loaded)
    if args.abab:
        merge(args.out, abab(args.abab, "grading_off", order=("parent", "this") * 3, order_note="parent this, three times"))   # three rounds: two leave the spread to one pair
        return
    if args.profile_child:   # the dungeon on the serial schedule: each grade variant in CHILD's order, then fog alone
        for _name, grade, side in CHILD:
            frames_ms("dungeon", grade, side, False, frames=CHILD_FRAMES, warmup=CHILD_WARMUP, serial=True)
        frames_ms("dungeon", None, 0, False, frames=CHILD_FRAMES, warmup=CHILD_WARMUP, serial=True, fog_only=True)
        return
    if args.kernel_stats:
        ceiling = json.load(open(args.out))["copy_ceiling_gb_s"]
        rows, _ = kernel_trace(__file__, ["--profile-child"], "grading")
        nbytes = launch_bytes(*HD)
        grade_us, per = dispatch_us(rows, "k_grade"), CHILD_FRAMES + CHILD_WARMUP
        assert len(grade_us) == per * len(CHILD), (len(grade_us), per, len(CHILD))
        out, med = {}, {}
        for i, (name, _grade, _side) in enumerate(CHILD):   # the variants ran one after the other: the dispatches in start order, warm-up left out
            out["k_grade " + name], med[name] = dispatch_record(grade_us[i * per + CHILD_WARMUP:(i + 1) * per], nbytes["k_grade"], ceiling)
        out["k_fog"], fog = dispatch_record(dispatch_us(rows, "k_fog")[CHILD_WARMUP:], nbytes["k_fog"], ceiling)
        out["grade_over_fog"] = {name: round(m / fog, 3) for name, m in med.items()}
        out["lut_side_17_33_65_us"] = [out["k_grade a_cdl_dither_lut%d" % n]["median_us"] for n in (17, 33, 65)]
        merge(args.out, {"kernel_stats_dungeon_1080p_serial_schedule": out})
        return
    from strolle_amd import Engine
    rec = {"render_size": list(HD), "mode": "Image{denoise}", "format": "RGBA8_UNORM_SRGB", "display": "ACES_FITTED", "build": "fast", "frames": FRAMES, "warmup": WARMUP,
           "a_cdl": {k: list(v) if isinstance(v, tuple) else v for k, v in A_CDL.items()}, "lut": "a smooth 33^3 table in the UNIT domain at strength 1",
           "chain": "fog, depth of field (f/0.25, 32 samples, autofocus), motion blur (shutter 0.5, 8 samples) under a moving camera, bloom (0.15, six levels), the grade and FXAA"}
    for scene in ("cornell", "dungeon"):
        rec[scene + "_ms_per_frame"] = {}
        for _ in range(2):   # interleaved twice: the spread of one box
            for name, (grade, side, chain) in VARIANTS.items():
                rec[scene + "_ms_per_frame"].setdefault(name, []).append(round(frames_ms(scene, grade, side, chain), 4))
    e = Engine(device=0)
    rec["copy_ceiling_gb_s"] = round(float(e.copy_bandwidth()), 1)
    e.close()
    rec["launch_compulsory_bytes"] = launch_bytes(*HD)["k_grade"]
    merge(args.out, rec)


if __name__ == "__main__":
    main()
