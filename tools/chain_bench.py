"""What the bench tools of the output chain share (fog_bench, shafts_bench, dof_bench, motion_blur_bench, bloom_bench, post_bench,
display_bench): merging a record into a profile, the 1080p camera that sways when it moves, timing frames with a set of camera settings
on, the A B A B of bench.py against a built parent tree, and the `rocprofv3 --kernel-trace --stats` child run with the median per kernel
against bytes over the copy ceiling. A library: each tool keeps its variants table, its launch_bytes, what only it measures, and main()."""
import csv
import glob
import json
import math
import os
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
WARMUP, FRAMES, HD = 20, 120, (1920, 1080)
EYES = {"cornell": ((0.0, 1.0, 3.2), (0.0, 1.0, 0.0)), "dungeon": ((-5.75, 0.5, -16.8), (-5.75, 0.5, -17.0))}
# the other nodes as the tools switch them on behind (or in front of) the one they measure
FOG = dict(falloff=1, color=(0.55, 0.62, 0.7, 1.0), density=0.06)
DOF = dict(samples=32, aperture_f_stops=0.25, autofocus=(0.5, 0.5))   # a Super 35 sensor at 45 degrees is a 22.5 mm lens; f/0.25: A is about 20 px at 1080p and 3 m
BLUR = dict(shutter=0.5, samples=8)
BLOOM = dict(intensity=0.15, levels=6)
BENCH_PY_SETS = (("bench_py_headline", []), ("bench_py_dungeon_1080p", ["--scene", "dungeon"]))


def merge(path, rec):
    old = json.load(open(path)) if os.path.exists(path) else {}
    old.update(rec)
    json.dump(old, open(path, "w"), indent=1)
    print(json.dumps(rec, indent=1))


def camera(scene, k, moving):
    """the scene's camera, swaying a few centimetres a frame when it moves (tens of pixels of velocity at 1080p on near walls)"""
    from strolle_amd import CameraMode, scenes
    (ex, ey, ez), (tx, ty, tz) = EYES[scene]
    dx = 0.25 * math.sin(0.35 * k) if moving else 0.0
    return scenes.camera_for(HD, (ex + dx, ey + 0.3 * dx, ez), (tx + 0.5 * dx, ty, tz), CameraMode.IMAGE)


def run_frames(scene, settings, moving=False, frames=FRAMES, warmup=WARMUP, serial=False, fmt="RGBA8_UNORM_SRGB", display="ACES_FITTED", after=None):
    """ms per frame of `scene` at 1080p Image{denoise}: events around `frames` frames after `warmup` on one stream. `settings` maps a
    camera setter's name to its keyword arguments or to a descriptor, applied in that order; None values are left out. `fmt` None: RGBA32F
    and no display. `after(e, cam, (w, h))` looks at the engine behind the last frame; with it the result is (ms, what it returns)."""
    import torch
    from strolle_amd import Engine, OutputFormat, Tonemap, scenes
    e = Engine(device=0)
    if serial:
        e.set_tuning(overlap=0)   # one stream: a launch's time is its own, not that of a launch sharing the chip with the side stream's
    (scenes.build_cornell if scene == "cornell" else scenes.build_dungeon)(e)
    e.set_seed(7)
    cam = e.create_camera(camera(scene, 0, moving))
    if fmt is not None:
        e.set_output_format(cam, OutputFormat[fmt])
        e.set_display(cam, tonemap=Tonemap[display])
    for setter, s in settings.items():
        if isinstance(s, dict):
            getattr(e, setter)(cam, **s)
        elif s is not None:
            getattr(e, setter)(cam, s)
    w, h = e.output_size(cam)
    out = torch.zeros((h, w, 16 if fmt is None else 4), dtype=torch.uint8, device="cuda:0")
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
    extra = after(e, cam, (w, h)) if after else None
    e.close()
    ms = a.elapsed_time(b) / frames
    return (ms, extra) if after else ms


def moving_tiles(e, cam, size, shutter):
    """32 x 32 tiles of the last frame whose 3 x 3 neighbourhood moves by half a pixel or more: the pixels the motion-blur gather taps for"""
    import numpy as np
    from strolle_amd import Buffer
    w, h = size
    v = e.read_buffer(cam, Buffer.VELOCITY_MAP).reshape(h, w, 4)[..., :2].astype(np.float64) * (0.5 * shutter)
    ty, tx = (h + 31) // 32, (w + 31) // 32
    pad = np.zeros((ty * 32, tx * 32)); pad[:h, :w] = np.hypot(v[..., 0], v[..., 1])
    t = np.zeros((ty + 2, tx + 2), bool)
    t[1:-1, 1:-1] = pad.reshape(ty, 32, tx, 32).max((1, 3)) >= 0.5
    n = np.zeros((ty, tx), bool)
    for dy in range(3):
        for dx in range(3):
            n |= t[dy:dy + ty, dx:dx + tx]
    return int(n.sum())


def abab(parent, key_prefix, extra_arg_sets=BENCH_PY_SETS, flags=("--no-extras", "--no-cpu-baseline"), order=("parent", "this") * 2, order_note="parent this parent this"):
    """bench.py of the built tree `parent` against this tree's, in `order`, once per (key, extra arguments) of `extra_arg_sets`:
    {key + "_" + key_prefix + "_abab_ms_per_step": both series, the difference of their means and the parent's spread}"""
    roots = {"parent": os.path.abspath(parent), "this": ROOT}
    rec = {}
    for key, extra in extra_arg_sets:
        series = {"parent": [], "this": []}
        for name in order:
            r = subprocess.run([sys.executable, os.path.join(roots[name], "bench.py"), "--gpus", "1", "--steps", "60", "--warmup", "15"] + list(flags) + list(extra),
                               cwd=roots[name], capture_output=True, text=True, check=True, timeout=300)
            series[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"])
        mean = {k: sum(v) / len(v) for k, v in series.items()}
        rec["%s_%s_abab_ms_per_step" % (key, key_prefix)] = {"order": order_note, **series, "mean_difference": round(mean["this"] - mean["parent"], 5),
                                                             "parent_spread": round(max(series["parent"]) - min(series["parent"]), 5)}
    return rec


def kernel_trace(script, child_args=("--profile-child",), name="chain"):
    """One `rocprofv3 --kernel-trace --stats` run (no counters) of `script child_args`: (the trace's rows in start order, the child's stdout)"""
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", name, "--", sys.executable, os.path.abspath(script)] + list(child_args),
                           check=True, timeout=600, capture_output=True, text=True)
        trace = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)[0]
        with open(trace) as f:
            rows = sorted(csv.DictReader(f), key=lambda row: int(row["Start_Timestamp"]))
    return rows, r.stdout


def dispatch_us(rows, kernel):
    """the microseconds of every dispatch whose kernel name contains `kernel`, in start order"""
    return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]


def dispatch_record(us, nbytes=None, ceiling=None):
    """the median of `us` and, given a launch's compulsory bytes and the copy ceiling in GB/s, the time those bytes take at the ceiling"""
    med = sorted(us)[len(us) // 2]
    rec = {"median_us": round(med, 2), "dispatches": len(us)}
    if nbytes is not None:
        floor = nbytes / (ceiling * 1e3)
        rec.update({"compulsory_bytes": nbytes, "bytes_over_copy_ceiling_us": round(floor, 2), "time_over_that": round(med / floor, 2)})
    return rec, med


def kernel_stats(script, child_args, launch_bytes, ceiling, name="chain"):
    """the child run's record per kernel of `launch_bytes` ({kernel: compulsory bytes, or None}); kernels that never ran are left out"""
    rows, _ = kernel_trace(script, child_args, name)
    out = {}
    for kernel, nbytes in launch_bytes.items():
        us = dispatch_us(rows, kernel)
        if us:
            out[kernel] = dispatch_record(us, nbytes, ceiling)[0]
    return out
