#!/usr/bin/env python3
"""Cost of motion blur (include/strolle_hip.h "motion blur"; k_motion_blur.hip) in the default (fast) build. Every run MERGES its figures into --out.

  (default)  (a) ms per frame of Cornell and the dungeon at 1920x1080 Image{denoise} into RGBA8 sRGB with ACES: blur off (static and moving
             camera), blur on under a camera that moves every frame, blur on under a static camera (pack, neighbour and the rest-path copy),
             and blur + bloom + FXAA under the moving camera (FRAMES frames after WARMUP, events around the whole run on one stream,
             interleaved twice);
             (b) the copy ceiling (st_debug_copy_bandwidth) and the three launches' compulsory bytes (st_motion_blur.cpp mblur_steps).
  --kernel-stats        one `rocprofv3 --kernel-trace --stats` child run of its own (no counters): the three launches' times per dispatch under
                        the moving and the static camera, on the two-stream schedule (sharing the chip with the side stream) and on the
                        serial one (alone; also as a plain RGBA32F copy), against bytes / copy ceiling, and the moving gather's time per tap.
  --profile-child       what that run wraps.
  --abab PARENT         A B A B of bench.py (the headline and the dungeon at 1080p): PARENT/bench.py (the parent commit, built) against this tree's.

  python tools/motion_blur_bench.py [--out profiles/motion_blur.json] [--kernel-stats | --profile-child | --abab DIR]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (before the library: torch's bundled HIP runtime has to be the first one loaded)

WARMUP, FRAMES, HD = 20, 120, (1920, 1080)
BLUR = dict(shutter=0.5, samples=8)
BLOOM = dict(intensity=0.15, levels=6)
# name: (blur, moving camera, bloom + FXAA)
VARIANTS = {"off_static": (False, False, False), "off_moving": (False, True, False), "blur_moving": (True, True, False), "blur_static": (True, False, False),
            "blur_bloom_fxaa_moving": (True, True, True)}
# the engines of --profile-child: the two-stream schedule (a launch shares the chip with the side stream's), then the serial one (its time is its own)
SEGMENTS = ("moving_camera", "static_camera", "moving_camera_serial_schedule", "static_camera_serial_schedule", "static_camera_serial_schedule_rgba32f_no_display")
EYES = {"cornell": ((0.0, 1.0, 3.2), (0.0, 1.0, 0.0)), "dungeon": ((-5.75, 0.5, -16.8), (-5.75, 0.5, -17.0))}


def merge(path, rec):
    old = json.load(open(path)) if os.path.exists(path) else {}
    old.update(rec)
    json.dump(old, open(path, "w"), indent=1)
    print(json.dumps(rec, indent=1))


def camera(scene, k, moving):
    """the scene's camera, swaying a few centimetres a frame when it moves (tens of pixels of velocity at 1080p on near walls)"""
    import math
    from strolle_amd import CameraMode, scenes
    (ex, ey, ez), (tx, ty, tz) = EYES[scene]
    dx = 0.25 * math.sin(0.35 * k) if moving else 0.0
    return scenes.camera_for(HD, (ex + dx, ey + 0.3 * dx, ez), (tx + 0.5 * dx, ty, tz), CameraMode.IMAGE)


def run_frames(scene, blur, moving, chain, frames=FRAMES, warmup=WARMUP, serial=False, plain=False):
    import torch
    from strolle_amd import Engine, OutputFormat, Tonemap, scenes
    e = Engine(device=0)
    if serial:
        e.set_tuning(overlap=0)   # one stream: a launch's time is its own, not that of a launch sharing the chip with the side stream's
    (scenes.build_cornell if scene == "cornell" else scenes.build_dungeon)(e)
    e.set_seed(7)
    cam = e.create_camera(camera(scene, 0, moving))
    if not plain:   # (plain: RGBA32F with no display transform: the gather at rest is a 16-B copy)
        e.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
        e.set_display(cam, tonemap=Tonemap.ACES_FITTED)
    if blur:
        e.set_motion_blur(cam, **BLUR)
    if chain:
        e.set_bloom(cam, **BLOOM)
        e.set_post(cam, fxaa=True)
    w, h = e.output_size(cam)
    out = torch.zeros((h, w, 16 if plain else 4), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in range(warmup + frames):
        if k == warmup:
            torch.cuda.synchronize(); a.record(s)
        if moving:
            e.update_camera(cam, camera(scene, k, True))
        e.tick(s.cuda_stream)
        e.render_camera(cam, out.data_ptr(), s.cuda_stream)
    b.record(s); torch.cuda.synchronize()
    moving_tiles = None
    if blur:   # tiles of the last frame whose neighbourhood moves: the pixels the gather taps for
        from strolle_amd import Buffer
        import numpy as np
        v = e.read_buffer(cam, Buffer.VELOCITY_MAP).reshape(h, w, 4)[..., :2].astype(np.float64) * (0.5 * BLUR["shutter"])
        r = np.hypot(v[..., 0], v[..., 1])
        ty, tx = (h + 31) // 32, (w + 31) // 32
        t = np.zeros((ty + 2, tx + 2), bool)
        pad = np.zeros((ty * 32, tx * 32)); pad[:h, :w] = r
        t[1:-1, 1:-1] = pad.reshape(ty, 32, tx, 32).max((1, 3)) >= 0.5
        n = np.zeros((ty, tx), bool)
        for dy in range(3):
            for dx in range(3):
                n |= t[dy:dy + ty, dx:dx + tx]
        moving_tiles = int(n.sum())
    e.close()
    return a.elapsed_time(b) / frames, moving_tiles


def launch_bytes(w, h, out_bytes=4):
    tiles = ((w + 31) // 32) * ((h + 31) // 32)
    return {"k_mblur_pack": w * h * 40 + tiles * 16, "k_mblur_neighbour": tiles * 32, "k_mblur_gather": w * h * (16 + out_bytes) + tiles * 16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_blur.json"))
    ap.add_argument("--profile-child", action="store_true")
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--abab")
    args = ap.parse_args()
    if args.abab:
        rec = {}
        for key, extra in (("bench_py_headline", []), ("bench_py_dungeon_1080p", ["--scene", "dungeon"])):
            series = {"parent": [], "this": []}
            for _ in range(2):
                for name, root in (("parent", args.abab), ("this", ROOT)):
                    r = subprocess.run([sys.executable, os.path.join(os.path.abspath(root), "bench.py"), "--gpus", "1", "--steps", "60", "--warmup", "15", "--no-extras", "--no-cpu-baseline"] + extra,
                                       cwd=os.path.abspath(root), capture_output=True, text=True, check=True, timeout=300)
                    series[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"])
            mean = {k: sum(v) / len(v) for k, v in series.items()}
            rec[key + "_blur_off_abab_ms_per_step"] = {"order": "parent this parent this", **series, "mean_difference": round(mean["this"] - mean["parent"], 5),
                                                      "parent_spread": round(max(series["parent"]) - min(series["parent"]), 5)}
        merge(args.out, rec)
        return
    if args.profile_child:   # the dungeon, 30 frames each: SEGMENTS below, in this order
        run_frames("dungeon", True, True, False, frames=30, warmup=10)
        run_frames("dungeon", True, False, False, frames=30, warmup=10)
        run_frames("dungeon", True, True, False, frames=30, warmup=10, serial=True)
        run_frames("dungeon", True, False, False, frames=30, warmup=10, serial=True)
        run_frames("dungeon", True, False, False, frames=30, warmup=10, serial=True, plain=True)
        return
    if args.kernel_stats:
        old = json.load(open(args.out))
        ceiling, tiles_moving = old["copy_ceiling_gb_s"], old["dungeon_moving_tiles_last_frame"]
        with tempfile.TemporaryDirectory() as tmp:
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "mblur", "--", sys.executable, os.path.abspath(__file__), "--profile-child"],
                           check=True, timeout=600)
            trace = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)[0]
            with open(trace) as f:
                rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
        nbytes = launch_bytes(*HD)
        out = {}
        for kernel in nbytes:
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
            n = len(us) // len(SEGMENTS)   # every engine of the child dispatched each kernel as often
            for i, name in enumerate(SEGMENTS):
                part = us[i * n:(i + 1) * n]
                if name.endswith("rgba32f_no_display") and kernel == "k_mblur_gather":
                    rec_bytes = HD[0] * HD[1] * 32 + 2040 * 16
                else:
                    rec_bytes = nbytes[kernel]
                med = sorted(part)[len(part) // 2]
                rec = {"median_us": round(med, 2), "dispatches": len(part), "compulsory_bytes": rec_bytes, "bytes_over_copy_ceiling_us": round(rec_bytes / (ceiling * 1e3), 2),
                       "time_over_that": round(med / (rec_bytes / (ceiling * 1e3)), 2)}
                if kernel == "k_mblur_gather" and name.startswith("moving") and tiles_moving:
                    rec["ns_per_tap"] = round(med * 1e3 / (tiles_moving * 1024 * BLUR["samples"]), 4)
                    rec["pixels_in_moving_tiles_x_samples"] = tiles_moving * 1024 * BLUR["samples"]
                out.setdefault(kernel, {})[name] = rec
        merge(args.out, {"kernel_stats_dungeon_1080p": out})
        return
    from strolle_amd import Engine
    rec = {"render_size": list(HD), "mode": "Image{denoise}", "format": "RGBA8_UNORM_SRGB", "display": "ACES_FITTED", "build": "fast", "frames": FRAMES,
           "warmup": WARMUP, "blur": BLUR, "chain": "bloom (0.15, six levels) + FXAA behind the blur"}
    for scene in ("cornell", "dungeon"):
        rec[scene + "_ms_per_frame"] = {}
        for _ in range(2):   # interleaved twice: the spread of one box
            for name, (blur, moving, chain) in VARIANTS.items():
                ms, tiles = run_frames(scene, blur, moving, chain)
                rec[scene + "_ms_per_frame"].setdefault(name, []).append(round(ms, 4))
                if name == "blur_moving":
                    rec[scene + "_moving_tiles_last_frame"] = tiles
    e = Engine(device=0)
    rec["copy_ceiling_gb_s"] = round(float(e.copy_bandwidth()), 1)
    e.close()
    rec["tiles"] = ((HD[0] + 31) // 32) * ((HD[1] + 31) // 32)
    rec["launch_compulsory_bytes"] = launch_bytes(*HD)
    merge(args.out, rec)


if __name__ == "__main__":
    main()
