#!/usr/bin/env python3
"""Cost of fog (include/strolle_hip.h "fog"; k_fog.hip) in the default (fast) build. Every run MERGES its figures into --out.

  (default)  (a) ms per frame of Cornell and the dungeon at 1920x1080 Image{denoise} into RGBA8 sRGB with ACES: fog off, on (exponential +
             height + the light lobe), on with ST_FOG_SKY, and on with depth of field, motion blur, bloom and FXAA behind it (FRAMES frames
             after WARMUP, events around the whole run on one stream, interleaved twice);
             (b) the copy ceiling (st_debug_copy_bandwidth) and the launch's compulsory bytes (st_fog.cpp fog_step).
  --restatement         CPU only: the worst deviation of the numpy restatement from the float64 definition over the tests' input matrix
                        (tests/test_fog_abi.py restatement_vs_definition), the figure that test's bound is four times of.
  --kernel-stats        one `rocprofv3 --kernel-trace --stats` child run of its own (no counters), on the serial schedule (a launch's time is
                        its own): the fog launch's time per dispatch against bytes / copy ceiling, and depth of field's all-in-focus copy
                        path (k_dof_gather at f/1000, which moves the same colour bytes) re-measured in the same run.
  --profile-child       what that run wraps.
  --abab PARENT         A B A B of bench.py (the headline and the dungeon at 1080p): PARENT/bench.py (the parent commit, built) against this tree's.

  python tools/fog_bench.py [--out profiles/fog.json] [--restatement | --kernel-stats | --profile-child | --abab DIR]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))   # fog_ref.py, fog_cases.py, test_fog_abi.py: the restatement's deviation

WARMUP, FRAMES, HD = 20, 120, (1920, 1080)
FOG = dict(falloff=1, color=(0.55, 0.62, 0.7, 1.0), density=0.06, height_falloff=0.3, height_reference=0.0, light_color=(1.0, 0.8, 0.5), light_exponent=8.0,
           light_direction=(0.3, 0.5, -0.8))
FOG_SKY = dict(FOG, sky_distance=200.0)
DOF = dict(samples=32, aperture_f_stops=0.25, autofocus=(0.5, 0.5))
SHARP = dict(samples=32, aperture_f_stops=1000.0, autofocus=(0.5, 0.5))   # |coc| < 0.5 everywhere: depth of field's copy path
BLUR = dict(shutter=0.5, samples=8)
BLOOM = dict(intensity=0.15, levels=6)
# name: (fog, depth of field + motion blur + bloom + FXAA under a moving camera)
VARIANTS = {"off": (None, False), "fog": (FOG, False), "fog_sky": (FOG_SKY, False), "fog_dof_motion_blur_bloom_fxaa": (FOG, True)}
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


def run_frames(scene, fog, chain, frames=FRAMES, warmup=WARMUP, serial=False, dof=None):
    import torch
    from strolle_amd import Engine, OutputFormat, Tonemap, scenes
    e = Engine(device=0)
    if serial:
        e.set_tuning(overlap=0)   # one stream: a launch's time is its own, not that of a launch sharing the chip with the side stream's
    (scenes.build_cornell if scene == "cornell" else scenes.build_dungeon)(e)
    e.set_seed(7)
    cam = e.create_camera(camera(scene, 0, chain))
    e.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
    e.set_display(cam, tonemap=Tonemap.ACES_FITTED)
    if fog:
        e.set_fog(cam, **fog)
    if dof:
        e.set_dof(cam, **dof)
    if chain:
        e.set_dof(cam, **DOF)
        e.set_motion_blur(cam, **BLUR)
        e.set_bloom(cam, **BLOOM)
        e.set_post(cam, fxaa=True)
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
    return {"k_fog": w * h * (20 + out_bytes), "k_dof_gather": w * h * (24 + out_bytes) + ((w + 31) // 32) * ((h + 31) // 32) * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fog.json"))
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--profile-child", action="store_true")
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--abab")
    args = ap.parse_args()
    if args.restatement:
        import fog_cases
        from test_fog_abi import restatement_vs_definition
        worst, where, pixels = restatement_vs_definition()
        merge(args.out, {"restatement_vs_definition": {"worst": float("%.3e" % worst), "case": where, "pixels": pixels, "cases": len(fog_cases.cases()),
                                                       "metric": "max |fog_f32 - fog_f64| / (max c' + max F), finite-depth pixels"}})
        return
    import torch  # noqa: F401  (before the library: torch's bundled HIP runtime has to be the first one loaded)
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
            rec[key + "_fog_off_abab_ms_per_step"] = {"order": "parent this parent this", **series, "mean_difference": round(mean["this"] - mean["parent"], 5),
                                                     "parent_spread": round(max(series["parent"]) - min(series["parent"]), 5)}
        merge(args.out, rec)
        return
    if args.profile_child:   # the dungeon on the serial schedule, 30 frames each: fog, then depth of field with everything in focus
        run_frames("dungeon", FOG_SKY, False, frames=30, warmup=10, serial=True)
        run_frames("dungeon", None, False, frames=30, warmup=10, serial=True, dof=SHARP)
        return
    if args.kernel_stats:
        ceiling = json.load(open(args.out))["copy_ceiling_gb_s"]
        with tempfile.TemporaryDirectory() as tmp:
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "fog", "--", sys.executable, os.path.abspath(__file__), "--profile-child"],
                           check=True, timeout=600, capture_output=True, text=True)
            trace = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)[0]
            with open(trace) as f:
                rows = list(csv.DictReader(f))
        out = {}
        for kernel, nbytes in launch_bytes(*HD).items():
            us = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"])
            if not us:
                continue
            med = us[len(us) // 2]
            out[kernel] = {"median_us": round(med, 2), "dispatches": len(us), "compulsory_bytes": nbytes, "bytes_over_copy_ceiling_us": round(nbytes / (ceiling * 1e3), 2),
                           "time_over_that": round(med / (nbytes / (ceiling * 1e3)), 2)}
        merge(args.out, {"kernel_stats_dungeon_1080p_serial_schedule": out})
        return
    from strolle_amd import Engine
    rec = {"render_size": list(HD), "mode": "Image{denoise}", "format": "RGBA8_UNORM_SRGB", "display": "ACES_FITTED", "build": "fast", "frames": FRAMES, "warmup": WARMUP,
           "fog": {k: list(v) if isinstance(v, tuple) else v for k, v in FOG.items()}, "fog_sky": "the same with ST_FOG_SKY at 200 m",
           "chain": "depth of field (f/0.25, 32 samples, autofocus), motion blur (shutter 0.5, 8 samples) under a moving camera, bloom (0.15, six levels) and FXAA behind the fog"}
    for scene in ("cornell", "dungeon"):
        rec[scene + "_ms_per_frame"] = {}
        for _ in range(2):   # interleaved twice: the spread of one box
            for name, (fog, chain) in VARIANTS.items():
                rec[scene + "_ms_per_frame"].setdefault(name, []).append(round(run_frames(scene, fog, chain), 4))
    e = Engine(device=0)
    rec["copy_ceiling_gb_s"] = round(float(e.copy_bandwidth()), 1)
    e.close()
    rec["launch_compulsory_bytes"] = launch_bytes(*HD)["k_fog"]
    merge(args.out, rec)


if __name__ == "__main__":
    main()
