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
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (before the library: torch's bundled HIP runtime has to be the first one loaded)

from chain_bench import BLOOM, BLUR, FRAMES, HD, WARMUP, abab, dispatch_record, dispatch_us, kernel_trace, merge, moving_tiles, run_frames  # noqa: E402

# name: (blur, moving camera, bloom + FXAA)
VARIANTS = {"off_static": (False, False, False), "off_moving": (False, True, False), "blur_moving": (True, True, False), "blur_static": (True, False, False),
            "blur_bloom_fxaa_moving": (True, True, True)}
# the engines of --profile-child: the two-stream schedule (a launch shares the chip with the side stream's), then the serial one (its time is its own)
SEGMENTS = ("moving_camera", "static_camera", "moving_camera_serial_schedule", "static_camera_serial_schedule", "static_camera_serial_schedule_rgba32f_no_display")


def frames_ms(scene, blur, moving, chain, plain=False, **kw):
    """(ms per frame, the moving tiles of the last frame when the blur is on); plain: RGBA32F with no display transform, where the gather at
    rest is a 16-B copy"""
    settings = dict(set_motion_blur=BLUR if blur else None, **(dict(set_bloom=BLOOM, set_post=dict(fxaa=True)) if chain else {}))
    return run_frames(scene, settings, moving=moving, fmt=None if plain else "RGBA8_UNORM_SRGB",
                      after=lambda e, cam, size: moving_tiles(e, cam, size, BLUR["shutter"]) if blur else None, **kw)


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
        merge(args.out, abab(args.abab, "blur_off"))
        return
    if args.profile_child:   # the dungeon, 30 frames each: SEGMENTS below, in this order
        frames_ms("dungeon", True, True, False, frames=30, warmup=10)
        frames_ms("dungeon", True, False, False, frames=30, warmup=10)
        frames_ms("dungeon", True, True, False, frames=30, warmup=10, serial=True)
        frames_ms("dungeon", True, False, False, frames=30, warmup=10, serial=True)
        frames_ms("dungeon", True, False, False, frames=30, warmup=10, serial=True, plain=True)
        return
    if args.kernel_stats:
        old = json.load(open(args.out))
        ceiling, tiles_moving = old["copy_ceiling_gb_s"], old["dungeon_moving_tiles_last_frame"]
        rows, _ = kernel_trace(__file__, ["--profile-child"], "mblur")
        nbytes = launch_bytes(*HD)
        out = {}
        for kernel in nbytes:
            us = dispatch_us(rows, kernel)
            n = len(us) // len(SEGMENTS)   # every engine of the child dispatched each kernel as often
            for i, name in enumerate(SEGMENTS):
                part = us[i * n:(i + 1) * n]
                if name.endswith("rgba32f_no_display") and kernel == "k_mblur_gather":
                    rec_bytes = HD[0] * HD[1] * 32 + 2040 * 16
                else:
                    rec_bytes = nbytes[kernel]
                rec, med = dispatch_record(part, rec_bytes, ceiling)
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
                ms, tiles = frames_ms(scene, blur, moving, chain)
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
