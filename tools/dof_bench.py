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
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # dof_ref.py: which pixels the last frame blurs

import torch  # noqa: E402,F401  (before the library: torch's bundled HIP runtime has to be the first one loaded)

WARMUP, FRAMES, HD = 20, 120, (1920, 1080)
# a Super 35 sensor at 45 degrees is a 22.5 mm lens; f/0.25 opens it far enough that A is about 20 px at 1080p and 3 m
DOF = dict(samples=32, aperture_f_stops=0.25, autofocus=(0.5, 0.5))
SHARP = dict(samples=32, aperture_f_stops=1000.0, autofocus=(0.5, 0.5))   # |coc| < 0.5 everywhere: the copy path
BLUR = dict(shutter=0.5, samples=8)
BLOOM = dict(intensity=0.15, levels=6)
# name: (depth of field, motion blur + bloom + FXAA under a moving camera)
VARIANTS = {"off": (None, False), "dof_mid_scene": (DOF, False), "dof_all_in_focus": (SHARP, False), "dof_motion_blur_bloom_fxaa": (DOF, True)}
SEGMENTS = ("dof_mid_scene", "dof_all_in_focus", "motion_blur_moving_camera")
EYES = {"cornell": ((0.0, 1.0, 3.2), (0.0, 1.0, 0.0)), "dungeon": ((-5.75, 0.5, -16.8), (-5.75, 0.5, -17.0))}


def merge(path, rec):
    old = json.load(open(path)) if os.path.exists(path) else {}
    old.update(rec)
    json.dump(old, open(path, "w"), indent=1)
    print(json.dumps(rec, indent=1))


def camera(scene, k, moving):
    import math
    from strolle_amd import CameraMode, scenes
    (ex, ey, ez), (tx, ty, tz) = EYES[scene]
    dx = 0.25 * math.sin(0.35 * k) if moving else 0.0
    return scenes.camera_for(HD, (ex + dx, ey + 0.3 * dx, ez), (tx + 0.5 * dx, ty, tz), CameraMode.IMAGE)


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


def run_frames(scene, dof, chain, frames=FRAMES, warmup=WARMUP, serial=False, blur_only=False):
    import torch
    from strolle_amd import Engine, OutputFormat, Tonemap, dof_desc, scenes
    e = Engine(device=0)
    if serial:
        e.set_tuning(overlap=0)   # one stream: a launch's time is its own, not that of a launch sharing the chip with the side stream's
    (scenes.build_cornell if scene == "cornell" else scenes.build_dungeon)(e)
    e.set_seed(7)
    moving = chain or blur_only
    cam = e.create_camera(camera(scene, 0, moving))
    e.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
    e.set_display(cam, tonemap=Tonemap.ACES_FITTED)
    desc = dof_desc(**dof) if dof else None
    if desc is not None:
        e.set_dof(cam, desc)
    if chain or blur_only:
        e.set_motion_blur(cam, **BLUR)
    if chain:
        e.set_bloom(cam, **BLOOM)
        e.set_post(cam, fxaa=True)
    w, h = e.output_size(cam)
    out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
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
    extra = None
    if desc is not None and not moving:
        extra = blurred_pixels(e, cam, desc, scene)
    elif blur_only:   # tiles of the last frame whose neighbourhood moves: the pixels the motion-blur gather taps for (tools/motion_blur_bench.py)
        import numpy as np
        from strolle_amd import Buffer
        v = e.read_buffer(cam, Buffer.VELOCITY_MAP).reshape(h, w, 4)[..., :2].astype(np.float64) * (0.5 * BLUR["shutter"])
        ty, tx = (h + 31) // 32, (w + 31) // 32
        pad = np.zeros((ty * 32, tx * 32)); pad[:h, :w] = np.hypot(v[..., 0], v[..., 1])
        t = np.zeros((ty + 2, tx + 2), bool)
        t[1:-1, 1:-1] = pad.reshape(ty, 32, tx, 32).max((1, 3)) >= 0.5
        n = np.zeros((ty, tx), bool)
        for dy in range(3):
            for dx in range(3):
                n |= t[dy:dy + ty, dx:dx + tx]
        extra = int(n.sum())
    e.close()
    return a.elapsed_time(b) / frames, extra


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
        rec = {}
        for key, extra in (("bench_py_headline", []), ("bench_py_dungeon_1080p", ["--scene", "dungeon"])):
            series = {"parent": [], "this": []}
            for _ in range(2):
                for name, root in (("parent", args.abab), ("this", ROOT)):
                    r = subprocess.run([sys.executable, os.path.join(os.path.abspath(root), "bench.py"), "--gpus", "1", "--steps", "60", "--warmup", "15", "--no-extras", "--no-cpu-baseline"] + extra,
                                       cwd=os.path.abspath(root), capture_output=True, text=True, check=True, timeout=300)
                    series[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"])
            mean = {k: sum(v) / len(v) for k, v in series.items()}
            rec[key + "_dof_off_abab_ms_per_step"] = {"order": "parent this parent this", **series, "mean_difference": round(mean["this"] - mean["parent"], 5),
                                                     "parent_spread": round(max(series["parent"]) - min(series["parent"]), 5)}
        merge(args.out, rec)
        return
    if args.profile_child:   # the dungeon on the serial schedule, 30 frames each: SEGMENTS, in this order
        _, mid = run_frames("dungeon", DOF, False, frames=30, warmup=10, serial=True)
        run_frames("dungeon", SHARP, False, frames=30, warmup=10, serial=True)
        _, tiles = run_frames("dungeon", None, False, frames=30, warmup=10, serial=True, blur_only=True)
        print("CHILD " + json.dumps({"dof_blurred_pixels": mid[0], "mblur_moving_tiles": tiles}))
        return
    if args.kernel_stats:
        old = json.load(open(args.out))
        ceiling = old["copy_ceiling_gb_s"]
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "dof", "--", sys.executable, os.path.abspath(__file__), "--profile-child"],
                               check=True, timeout=600, capture_output=True, text=True)
            child = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])
            trace = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)[0]
            with open(trace) as f:
                rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
        nbytes = launch_bytes(*HD)
        out = {}
        for kernel in nbytes:
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
            n = len(us) // 2   # the two depth-of-field engines of the child dispatched each kernel as often
            for i, name in enumerate(SEGMENTS[:2]):
                part = us[i * n:(i + 1) * n]
                med = sorted(part)[len(part) // 2]
                rec = {"median_us": round(med, 2), "dispatches": len(part), "compulsory_bytes": nbytes[kernel], "bytes_over_copy_ceiling_us": round(nbytes[kernel] / (ceiling * 1e3), 2),
                       "time_over_that": round(med / (nbytes[kernel] / (ceiling * 1e3)), 2)}
                if kernel == "k_dof_gather" and name == "dof_mid_scene" and child["dof_blurred_pixels"]:
                    taps = child["dof_blurred_pixels"] * DOF["samples"]
                    rec["blurred_pixels_x_samples"] = taps
                    rec["ps_per_tap"] = round(med * 1e6 / taps, 3)
                out.setdefault(kernel, {})[name] = rec
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "k_mblur_gather" in r["Kernel_Name"]]
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
                ms, extra = run_frames(scene, dof, chain)
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
