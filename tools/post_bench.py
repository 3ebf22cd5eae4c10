#!/usr/bin/env python3
"""Cost of output post-processing (include/strolle_hip.h "post-processing"; k_post.hip) in the default (fast) build, and what it buys.

  (a) ms per frame of Cornell and the dungeon at 1920x1080 Image{denoise} into RGBA8 sRGB: post-processing off, FXAA only, FXAA +
      Catmull-Rom to 3840x2160 (FRAMES frames after WARMUP, events around the whole run on one stream, interleaved twice);
  (b) the dungeon rendered at 1920x1080 and upscaled to 3840x2160 (Catmull-Rom, with and without FXAA) against the dungeon rendered
      natively at 3840x2160, in the same run;
  (c) the bytes each post launch moves (every source texel read once, every output pixel written once) and, with --kernel-stats, the
      kernels' own times from a separate `rocprofv3 --kernel-trace --stats` run of `--profile-child`, as a fraction of the measured copy
      ceiling (st_debug_copy_bandwidth);
  (d) the CPU-side property of the restatement: a slanted edge's error against its analytic coverage before and after FXAA.

  python tools/post_bench.py [--out profiles/post.json] [--profile-child] [--kernel-stats FILE]
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from strolle_amd import CameraMode, Engine, OutputFormat, ResampleFilter, scenes

WARMUP, FRAMES, HD, UHD = 20, 120, (1920, 1080), (3840, 2160)
VARIANTS = {"off": None, "fxaa": dict(fxaa=True), "fxaa_catmull_rom_2160p": dict(fxaa=True, output_size=UHD, filter=ResampleFilter.CATMULL_ROM),
            "catmull_rom_2160p": dict(output_size=UHD, filter=ResampleFilter.CATMULL_ROM)}


def frame_ms(scene, post, size=HD, frames=FRAMES):
    e = Engine(device=0)
    (scenes.build_cornell if scene == "cornell" else scenes.build_dungeon)(e)
    e.set_seed(7)
    cam = e.create_camera((scenes.cornell_camera if scene == "cornell" else scenes.dungeon_camera)(size, CameraMode.IMAGE))
    e.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
    if post is not None:
        e.set_post(cam, **post)
    w, h = e.output_size(cam)
    out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in range(WARMUP + frames):
        if k == WARMUP:
            torch.cuda.synchronize(); a.record(s)
        e.tick(s.cuda_stream)
        e.render_camera(cam, out.data_ptr(), s.cuda_stream)
    b.record(s); torch.cuda.synchronize()
    e.close()
    return a.elapsed_time(b) / frames


def launch_bytes():
    """compulsory bytes of the launches of the timed variants (st_post.cpp post_plan): RGBA32F in; RGBA32F between the two, RGBA8 out"""
    n, m = HD[0] * HD[1], UHD[0] * UHD[1]
    return {"k_post_fxaa (1080p -> RGBA8)": n * (16 + 4), "k_post_fxaa (1080p -> RGBA32F plane)": n * (16 + 16), "k_post_resample<2> (1080p -> 2160p RGBA8)": n * 16 + m * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "post.json"))
    ap.add_argument("--profile-child", action="store_true", help="Cornell and dungeon frames of every variant, 40 each (the rocprofv3 run)")
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel stats of a --profile-child run: adds the post kernels' times to --out")
    args = ap.parse_args()
    if args.kernel_stats:
        rec = json.load(open(args.out))
        if args.kernel_stats.endswith(".db"):
            import sqlite3
            rows = {}
            for name, d in sqlite3.connect(args.kernel_stats).execute("select name, duration from kernels"):
                rows.setdefault(name, []).append(d)
            rows = {k: (float(np.mean(v)) / 1e3, len(v)) for k, v in rows.items()}
        else:
            with open(args.kernel_stats) as f:
                rows = {r["Name"]: (float(r["AverageNs"]) / 1e3, int(r["Calls"])) for r in csv.DictReader(f)}
        rec["kernels_us"] = {k: {"us": round(us, 2), "calls": n} for k, (us, n) in sorted(rows.items()) if "k_post" in k}
        json.dump(rec, open(args.out, "w"), indent=1)
        print(json.dumps(rec["kernels_us"], indent=1))
        return
    if args.profile_child:
        for scene in ("cornell", "dungeon"):
            for name in ("fxaa", "fxaa_catmull_rom_2160p"):
                frame_ms(scene, VARIANTS[name], frames=40)
        return
    rec = {"render_size": list(HD), "mode": "Image{denoise}", "format": "RGBA8_UNORM_SRGB", "build": "fast", "frames": FRAMES, "warmup": WARMUP,
           "variants": {k: (None if v is None else {kk: (int(vv) if isinstance(vv, ResampleFilter) else vv) for kk, vv in v.items()}) for k, v in VARIANTS.items()}}
    for scene in ("cornell", "dungeon"):
        rec[scene] = {}
        for _ in range(2):   # interleaved twice: the spread of one box
            for name in ("off", "fxaa", "fxaa_catmull_rom_2160p"):
                rec[scene].setdefault(name, []).append(round(frame_ms(scene, VARIANTS[name]), 4))
    buys = rec["dungeon_2160p_output_ms"] = {}
    for _ in range(2):
        buys.setdefault("native_2160p", []).append(round(frame_ms("dungeon", None, size=UHD, frames=60), 4))
        buys.setdefault("1080p_catmull_rom", []).append(round(frame_ms("dungeon", VARIANTS["catmull_rom_2160p"]), 4))
        buys.setdefault("1080p_fxaa_catmull_rom", []).append(round(frame_ms("dungeon", VARIANTS["fxaa_catmull_rom_2160p"]), 4))
    e = Engine(device=0)
    rec["copy_ceiling_gb_s"] = round(float(e.copy_bandwidth()), 1)
    e.close()
    rec["launch_bytes"] = launch_bytes()
    from test_post_abi import SLOPES, slanted_edge_errors   # the float32 restatement's own figures (CPU)
    rec["restatement_slanted_edge_mean_abs_error"] = {k: dict(zip(("before", "after"), (round(v, 6) for v in slanted_edge_errors(*SLOPES[k])))) for k in SLOPES}
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
