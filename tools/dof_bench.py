#!/usr/bin/env python3
"""Cost of depth of field (include/strolle_hip.h "depth of field"; k_dof.hip) in the default (fast) build. Every run MERGES its figures into --out.

  (default)  (a) ms per frame of Cornell and the dungeon at 1920x1080 Image{denoise} into RGBA8 sRGB with ACES: depth of field off, on and
             focused on the centre of the frame (mid-scene), on with everything in focus (pack, neighbour and the copy path of the gather),
             and on together with motion blur, bloom and FXAA (FRAMES frames after WARMUP, events around the whole run on one stream,
             interleaved twice);
             (b) the copy ceiling (st_debug_copy_bandwidth), the three launches' compulsory bytes (st_dof.cpp dof_steps) and the number of
             pixels of the last frame that go through the tap loop.
  --kernel-stats        one `rocprofv3 --kernel-trace --stats` child run of its own (no counters), on the serial schedule (a launch's time is
                        its own): the three launches' times per dispatch focused mid-scene and with everything in focus, against bytes /
                        copy ceiling, the gather's time per tap, and the motion-blur gather's time per tap re-measured in the same run.
  --profile-child       what that run wraps.
  --abab PARENT         A B A B of bench.py (the headline and the dungeon at 1080p): PARENT/bench.py (the parent commit, built) against this tree's.

  python tools/dof_bench.py [--out profiles/dof.json] [--kernel-stats | --profile-child | --abab DIR]
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # dof_ref.py: which pixels the last frame blurs

import torch  # noqa: E402,F401  (before the library: torch's bundled HIP runtime has to be the first one loaded)

from chain_bench import BLOOM, BLUR, DOF, FRAMES, HD, WARMUP, abab, camera, dispatch_record, dispatch_us, kernel_trace, merge, moving_tiles, run_frames  # noqa: E402

SHARP = dict(samples=32, aperture_f_stops=1000.0, autofocus=(0.5, 0.5))   # |coc| < 0.5 everywhere: the copy path
# name: (depth of field, motion blur + bloom + FXAA under a moving camera)
VARIANTS = {"off": (None, False), "dof_mid_scene": (DOF, False), "dof_all_in_focus": (SHARP, False), "dof_motion_blur_bloom_fxaa": (DOF, True)}
SEGMENTS = ("dof_mid_scene", "dof_all_in_focus", "motion_blur_moving_camera")


def blurred_pixels(e, cam, desc, scene):
    """pixels of the last frame that run the tap loop (r_g >= 0.5), from the G-buffer's depth and the restatement's steps 0 to 5"""
    import numpy as np
    import dof_ref as R
    from strolle_amd import Buffer
    w, h = HD
    planes = [e.read_buffer(cam, b).reshape(h, w, 4)[..., 0] for b in (Buffer.PRIM_GBUFFER_D0_A, Buffer.PRIM_GBUFFER_D0_B)]   # a static camera: either parity
    proj = np.asarray(camera(scene, 0, False).projection, np.float32).T.reshape(-1)
    f, K = R.constants(proj, h, desc.aperture_f_stops, desc.sensor_height)
    z = R.planar(R.frame_depth(planes[0]), proj)
    s, A = R.focus(z, f, K, desc.focal_distance, desc.flags, desc.focus_x, desc.focus_y)
    coc = R.pack(z, s, A, desc.max_radius)
    n = np.repeat(np.repeat(R.neighbour_max(R.tile_max(coc)), 32, 0), 32, 1)[:h, :w]
    return int((np.maximum(np.abs(coc), n) >= 0.5).sum()), float(s), float(A)


def frames_ms(scene, dof, chain, blur_only=False, **kw):
    """(ms per frame; under a static camera what blurred_pixels says of the last frame, with blur_only the moving tiles of it)"""
    from strolle_amd import dof_desc
    desc = dof_desc(**dof) if dof else None
    moving = chain or blur_only
    settings = dict(set_dof=desc, set_motion_blur=BLUR if moving else None, **(dict(set_bloom=BLOOM, set_post=dict(fxaa=True)) if chain else {}))

    def after(e, cam, size):
        if desc is not None and not moving:
            return blurred_pixels(e, cam, desc, scene)
        return moving_tiles(e, cam, size, BLUR["shutter"]) if blur_only else None

    return run_frames(scene, settings, moving=moving, after=after, **kw)


def launch_bytes(w, h, out_bytes=4):
    tiles = ((w + 31) // 32) * ((h + 31) // 32)
    return {"k_dof_pack": w * h * 12 + tiles * 4, "k_dof_neighbour": tiles * 8, "k_dof_gather": w * h * (24 + out_bytes) + tiles * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dof.json"))
    ap.add_argument("--profile-child", action="store_true")
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--abab")
    args = ap.parse_args()
    if args.abab:
        merge(args.out, abab(args.abab, "dof_off"))
        return
    if args.profile_child:   # the dungeon on the serial schedule, 30 frames each: SEGMENTS, in this order
        _, mid = frames_ms("dungeon", DOF, False, frames=30, warmup=10, serial=True)
        frames_ms("dungeon", SHARP, False, frames=30, warmup=10, serial=True)
        _, tiles = frames_ms("dungeon", None, False, frames=30, warmup=10, serial=True, blur_only=True)
        print("CHILD " + json.dumps({"dof_blurred_pixels": mid[0], "mblur_moving_tiles": tiles}))
        return
    if args.kernel_stats:
        old = json.load(open(args.out))
        ceiling = old["copy_ceiling_gb_s"]
        rows, stdout = kernel_trace(__file__, ["--profile-child"], "dof")
        child = json.loads([ln for ln in stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])
        nbytes = launch_bytes(*HD)
        out = {}
        for kernel in nbytes:
            us = dispatch_us(rows, kernel)
            n = len(us) // 2   # the two depth-of-field engines of the child dispatched each kernel as often
            for i, name in enumerate(SEGMENTS[:2]):
                part = us[i * n:(i + 1) * n]
                rec, med = dispatch_record(part, nbytes[kernel], ceiling)
                if kernel == "k_dof_gather" and name == "dof_mid_scene" and child["dof_blurred_pixels"]:
                    taps = child["dof_blurred_pixels"] * DOF["samples"]
                    rec["blurred_pixels_x_samples"] = taps
                    rec["ps_per_tap"] = round(med * 1e6 / taps, 3)
                out.setdefault(kernel, {})[name] = rec
        us = dispatch_us(rows, "k_mblur_gather")
        if us and child["mblur_moving_tiles"]:
            med, taps = sorted(us)[len(us) // 2], child["mblur_moving_tiles"] * 1024 * BLUR["samples"]
            out["k_mblur_gather"] = {"motion_blur_moving_camera": {"median_us": round(med, 2), "dispatches": len(us), "pixels_in_moving_tiles_x_samples": taps, "ps_per_tap": round(med * 1e6 / taps, 3)}}
        merge(args.out, {"kernel_stats_dungeon_1080p_serial_schedule": out})
        return
    from strolle_amd import Engine
    rec = {"render_size": list(HD), "mode": "Image{denoise}", "format": "RGBA8_UNORM_SRGB", "display": "ACES_FITTED", "build": "fast", "frames": FRAMES,
           "warmup": WARMUP, "dof": {k: list(v) if isinstance(v, tuple) else v for k, v in DOF.items()}, "all_in_focus": "the same lens at f/1000",
           "chain": "motion blur (shutter 0.5, 8 samples) under a moving camera + bloom (0.15, six levels) + FXAA behind depth of field"}
    for scene in ("cornell", "dungeon"):
        rec[scene + "_ms_per_frame"] = {}
        for _ in range(2):   # interleaved twice: the spread of one box
            for name, (dof, chain) in VARIANTS.items():
                ms, extra = frames_ms(scene, dof, chain)
                rec[scene + "_ms_per_frame"].setdefault(name, []).append(round(ms, 4))
                if extra is not None:
                    rec[scene + "_" + name + "_last_frame"] = {"pixels_through_the_tap_loop": extra[0], "focus_distance_m": round(extra[1], 4), "A_px": round(extra[2], 3)}
    e = Engine(device=0)
    rec["copy_ceiling_gb_s"] = round(float(e.copy_bandwidth()), 1)
    e.close()
    rec["tiles"] = ((HD[0] + 31) // 32) * ((HD[1] + 31) // 32)
    rec["launch_compulsory_bytes"] = launch_bytes(*HD)
    merge(args.out, rec)


if __name__ == "__main__":
    main()
