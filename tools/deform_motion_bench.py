#!/usr/bin/env python3
"""Cost of deformation motion (include/strolle_hip.h "skinned meshes", st_engine_set_deformation_motion) in the default (fast) build.

Scene: the dungeon + tools/skin_bench.py's 16 tubes of 8,192 triangles and 32 joints, every tube re-posed every tick, one 1920x1080
Image{denoise} frame per tick. Four runs in one process order, switch off / on / off / on, each a fresh engine:
  ms per frame (events around st_render_camera), st_tick's host ms and the device ms of the tick's work (events around st_tick on the tick's
  stream), medians over TICKS ticks after WARMUP; previous_bytes from st_debug_deformation.
The gate: st_tick gains no host wait. Its host time with the switch on (the larger of the two runs) must stay within the spread the two
switch-off runs show around their own figures: on <= max(off) + |off_1 - off_2|. The tool exits 1 when it does not.
`--profile` adds prim_visibility's kernel time from one `rocprofv3 --kernel-trace --stats` child run of each setting (`--child off|on`).
Keys other than this tool's in --out (the tests' reprojection shares, the A/B record against the parent commit) are kept.

  python tools/deform_motion_bench.py [--out profiles/deform_motion.json] [--profile] [--size 1920x1080]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np
import torch

from strolle_amd import CameraMode, Engine, Instance, Material, scenes

WARMUP, TICKS = 8, 40
TUBES, SEGMENTS, SIDES, JOINTS = 16, 128, 32, 32
POSITIONS = [(-5.75 + 0.7 * (k % 4 - 1.5), 0.0, -19.0 - 0.9 * (k // 4)) for k in range(TUBES)]


def xform(p):
    return np.array([[1, 0, 0, p[0]], [0, 1, 0, p[1]], [0, 0, 1, p[2]]], np.float32)


def run(on, size, mesh, jt, wt, ticks=TICKS):
    e = Engine(device=0)
    scenes.build_dungeon(e)
    e.insert_material(7000, Material(base_color=(0.2, 0.7, 0.3, 1.0)))
    e.insert_mesh(7000, mesh); e.set_skin(7000, jt, wt, JOINTS)
    for k, p in enumerate(POSITIONS):
        e.insert_instance(7000 + k, Instance(7000, 7000, xform(p)))
    e.set_deformation_motion(on)
    cam = e.create_camera(scenes.dungeon_camera(size, CameraMode.IMAGE))
    out = torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    e.tick(s.cuda_stream); torch.cuda.synchronize()
    host, kept = [], []
    for t in range(WARMUP + ticks):
        poses = [scenes.bend_pose(JOINTS, 1.5, 0.1 * t + k) for k in range(TUBES)]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        for k in range(TUBES):
            e.set_pose(7000 + k, poses[k])
        ev[0].record(s)
        t1 = time.perf_counter()
        e.tick(s.cuda_stream)          # (the previous frame may still be in flight: nothing here joins the device)
        t2 = time.perf_counter()
        ev[1].record(s)
        ev[2].record(s)
        e.render_camera(cam, out.data_ptr(), s.cuda_stream)
        ev[3].record(s)
        if t >= WARMUP:
            host.append((t2 - t1) * 1e3); kept.append(ev)
        if t % 4 == 3:
            ev[3].synchronize()        # the host stays at most a few frames ahead (an application presents)
    torch.cuda.synchronize()
    dev = [ev[0].elapsed_time(ev[1]) for ev in kept]; frame = [ev[2].elapsed_time(ev[3]) for ev in kept]
    with_previous, previous_bytes = e.deformation_stats()
    e.close()
    med = lambda v: round(float(np.median(v)), 4)
    return {"switch": "on" if on else "off", "ms_per_frame": med(frame), "tick_host_ms": med(host), "tick_device_ms": med(dev),
            "instances_with_previous": with_previous, "previous_bytes": previous_bytes}


def prim_visibility_us(setting, size):
    """One rocprofv3 --kernel-trace --stats run of a child of this tool: the mean time of k_prim_visibility's dispatches."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
               sys.executable, os.path.abspath(__file__), "--child", setting, "--size", "%dx%d" % size]
        subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                rows = [r for r in csv.DictReader(f) if "k_prim_visibility" in r["Name"]]
            if rows:
                calls = sum(int(r["Calls"]) for r in rows)
                return {"us": round(sum(float(r["TotalDurationNs"]) for r in rows) / calls / 1e3, 2), "calls": calls}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deform_motion.json"))
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--profile", action="store_true", help="add prim_visibility's kernel time from a rocprofv3 child run of each setting")
    ap.add_argument("--child", choices=("off", "on"), help="one short run of one setting and nothing else (what rocprofv3 wraps)")
    args = ap.parse_args()
    size = tuple(int(v) for v in args.size.split("x"))
    mesh, jt, wt = scenes.skinned_tube(SEGMENTS, SIDES, JOINTS)
    if args.child:
        run(args.child == "on", size, mesh, jt, wt, ticks=12)
        return 0
    runs = [run(on, size, mesh, jt, wt) for on in (False, True, False, True)]
    off = [r["tick_host_ms"] for r in runs if r["switch"] == "off"]
    on = [r["tick_host_ms"] for r in runs if r["switch"] == "on"]
    spread = abs(off[0] - off[1])
    gate = {"off_ms": off, "on_ms": on, "aa_spread_ms": round(spread, 4), "bound_ms": round(max(off) + spread, 4), "pass": bool(max(on) <= max(off) + spread)}
    rec = {}
    if os.path.exists(args.out):
        try:
            rec = json.load(open(args.out))
        except ValueError:
            rec = {}
    rec["cost_when_on"] = {"scene": "dungeon_13k + 16 tubes re-posed every tick", "size": list(size), "triangles_posed_per_tick": TUBES * len(mesh.positions),
                           "ticks": TICKS, "warmup": WARMUP, "build": "fast", "runs": runs, "tick_host_gate": gate}
    if args.profile:
        rec["cost_when_on"]["prim_visibility"] = {s: prim_visibility_us(s, size) for s in ("off", "on")}
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec["cost_when_on"]))
    return 0 if gate["pass"] else 1


if __name__ == "__main__":
    sys.exit(main())
