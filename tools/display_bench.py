#!/usr/bin/env python3
"""Cost of camera display transforms (include/strolle_hip.h "display transforms"; st_passes.h display_transform, k_display.hip) in the
default (fast) build.

  (a) ms per frame of Cornell and the dungeon at 1920x1080 Image{denoise} into RGBA8 sRGB: the display off, ACES with manual exposure and
      ACES with auto-exposure (FRAMES frames after WARMUP, events around the whole run on one stream, interleaved twice);
  (b) the composing launch (k_denoise_wavelet_far<true, ...>: the fast build's last a-trous pass with composition) and the finalize kernel
      come from a separate `rocprofv3 --kernel-trace --stats` run of `--profile-child`; `--kernel-stats <kernel_stats.csv or rocpd .db>`
      adds their times to the JSON.

  python tools/display_bench.py [--out profiles/display.json] [--profile-child] [--kernel-stats FILE]
"""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

from strolle_amd import CameraMode, Engine, OutputFormat, Tonemap, scenes

WARMUP, FRAMES, SIZE = 20, 120, (1920, 1080)
VARIANTS = {"off": None, "aces_manual": dict(tonemap=Tonemap.ACES_FITTED, exposure_ev=0.5),
            "aces_auto": dict(tonemap=Tonemap.ACES_FITTED, auto_exposure=True, ev_min=-12.0, ev_max=8.0, max_ev_step_up=0.1, max_ev_step_down=0.1)}


def frame_ms(scene, display, frames=FRAMES):
    e = Engine(device=0)
    (scenes.build_cornell if scene == "cornell" else scenes.build_dungeon)(e)
    e.set_seed(7)
    cam = e.create_camera((scenes.cornell_camera if scene == "cornell" else scenes.dungeon_camera)(SIZE, CameraMode.IMAGE))
    e.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
    if display is not None:
        e.set_display(cam, **display)
    out = torch.zeros((SIZE[1], SIZE[0], 4), dtype=torch.uint8, device="cuda:0")
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "display.json"))
    ap.add_argument("--profile-child", action="store_true", help="Cornell and dungeon frames of every variant, 40 each (the rocprofv3 run)")
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel stats of a --profile-child run: adds the composing and finalize kernels' times to --out")
    args = ap.parse_args()
    if args.kernel_stats:
        rec = json.load(open(args.out))
        rows = {}
        if args.kernel_stats.endswith(".db"):
            import sqlite3
            for name, d in sqlite3.connect(args.kernel_stats).execute("select name, duration from kernels"):
                rows.setdefault(name, []).append(d)
            rows = {k: (float(np.mean(v)) / 1e3, len(v)) for k, v in rows.items()}
        else:
            with open(args.kernel_stats) as f:
                rows = {r["Name"]: (float(r["AverageNs"]) / 1e3, int(r["Calls"])) for r in csv.DictReader(f)}
        rec["kernels_us"] = {k: {"us": round(us, 2), "calls": n} for k, (us, n) in sorted(rows.items())
                             if "k_denoise_wavelet_far" in k or "k_display" in k or "k_composition" in k}
        json.dump(rec, open(args.out, "w"), indent=1)
        print(json.dumps(rec["kernels_us"], indent=1))
        return
    if args.profile_child:   # the variants' composing kernels are told apart by their template arguments: <true, false> off, <true, true> on
        for scene in ("cornell", "dungeon"):
            for d in VARIANTS.values():
                frame_ms(scene, d, frames=40)
        return
    rec = {"size": list(SIZE), "mode": "Image{denoise}", "format": "RGBA8_UNORM_SRGB", "build": "fast", "frames": FRAMES, "warmup": WARMUP,
           "variants": {k: (None if v is None else {kk: (int(vv) if isinstance(vv, Tonemap) else vv) for kk, vv in v.items()}) for k, v in VARIANTS.items()}}
    for scene in ("cornell", "dungeon"):
        rec[scene] = {}
        for _ in range(2):   # interleaved twice: the spread of one box
            for name, d in VARIANTS.items():
                rec[scene].setdefault(name, []).append(round(frame_ms(scene, d), 4))
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
