#!/usr/bin/env python3
"""Cost of morph targets per tick (include/strolle_hip.h "morph targets"; k_skin.hip k_morph) in the default (fast) build, default tuning.

Scene: tools/skin_bench.py's — the dungeon + 16 tubes of 8,192 triangles — with 64 morph targets on the tube mesh, every tube re-weighted
every tick. Four cases: 8 or 64 active targets, morph only or morph + a 32-joint pose. For each case, interleaved tick by tick in one process:
  (a) the device path: st_instance_set_morph_weights (and st_instance_set_pose) for each tube, then st_tick — host ms of st_tick and device
      ms of the tick's work (events on the tick's stream right before and after st_tick);
  (b) what an application does without it: the morph (and linear blend skinning) in numpy, st_mesh_insert + st_instance_insert of every
      tube, then st_tick — host ms of all of that, device ms as in (a).
Medians over TICKS ticks after WARMUP. Each case's kernel time comes from one `rocprofv3 --kernel-trace --stats` child process of its own
(`--child CASE`: path (a) alone), started before this process touches the device. Compulsory bytes per launch and triangle: base 96 B +
output 96 B + 72 B per active target + 72 B of skin corners; their rate is put against st_debug_copy_bandwidth.

  python tools/morph_bench.py [--out profiles/morphing.json] [--no-kernel-times]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

WARMUP, TICKS = 5, 30
TUBES, SEGMENTS, SIDES, JOINTS, TARGETS = 16, 128, 32, 32, 64
POSITIONS = [(-5.75 + 0.7 * (k % 4 - 1.5), 0.0, -19.0 - 0.9 * (k // 4)) for k in range(TUBES)]
CASES = {"morph_8": (8, False), "morph_64": (64, False), "morph_skin_8": (8, True), "morph_skin_64": (64, True)}


def xform(p):
    return np.array([[1, 0, 0, p[0]], [0, 1, 0, p[1]], [0, 0, 1, p[2]]], np.float32)


def tube_with_targets():
    from strolle_amd import scenes
    mesh, jt, wt = scenes.skinned_tube(SEGMENTS, SIDES, JOINTS)
    dp3, dn3 = scenes.tube_morph_targets(mesh)
    rng = np.random.default_rng(64)
    n = len(mesh.positions)
    dp = rng.uniform(-0.01, 0.01, (TARGETS, n, 3, 3)).astype(np.float32); dn = rng.uniform(-0.05, 0.05, (TARGETS, n, 3, 3)).astype(np.float32)
    dp[:3], dn[:3] = dp3, dn3
    return mesh, jt, wt, dp, dn


def weights(t, k, active):
    w = np.zeros(TARGETS, np.float32)
    idx = np.arange(active) * (TARGETS // active)
    w[idx] = (0.2 + 0.5 * np.abs(np.sin(0.1 * t + k + 0.37 * idx))).astype(np.float32) / np.float32(active ** 0.5)
    return w


def numpy_morph(mesh, dp, dn, w):
    from strolle_amd import Mesh
    act = np.flatnonzero(w)
    p = mesh.positions + np.tensordot(w[act], dp[act], 1)
    nrm = mesh.normals + np.tensordot(w[act], dn[act], 1)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    return Mesh(p.astype(np.float32), nrm.astype(np.float32), mesh.uvs, mesh.tangents)


def build(device_path, mesh, jt, wt, dp, dn, skinned):
    from strolle_amd import Engine, Instance, Material, scenes
    e = Engine(device=0)
    scenes.build_dungeon(e)
    e.insert_material(7000, Material(base_color=(0.2, 0.7, 0.3, 1.0)))
    if device_path:
        e.insert_mesh(7000, mesh); e.set_morph_targets(7000, dp, dn)
        if skinned:
            e.set_skin(7000, jt, wt, JOINTS)
    for k, p in enumerate(POSITIONS):
        if not device_path:
            e.insert_mesh(8000 + k, mesh)
        e.insert_instance(7000 + k, Instance(7000 if device_path else 8000 + k, 7000, xform(p)))
    return e


def run_case(active, skinned, data, device_only=False, ticks=TICKS):
    import torch
    from skin_bench import numpy_lbs
    from strolle_amd import Instance, scenes
    mesh, jt, wt, dp, dn = data
    engines = {"device": build(True, *data, skinned)}
    if not device_only:
        engines["host_numpy_and_mesh_insert"] = build(False, *data, skinned)
    s = torch.cuda.Stream()
    for e in engines.values():
        e.tick(s.cuda_stream)
    torch.cuda.synchronize()
    host = {k: [] for k in engines}; dev = {k: [] for k in engines}
    for t in range(WARMUP + ticks):
        ws = [weights(t, k, active) for k in range(TUBES)]
        poses = [scenes.bend_pose(JOINTS, 1.5, 0.1 * t + k) for k in range(TUBES)] if skinned else None
        for name, e in engines.items():   # interleaved: both paths see the same box state
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(TUBES):
                if name == "device":
                    e.set_morph_weights(7000 + k, ws[k])
                    if skinned:
                        e.set_pose(7000 + k, poses[k])
                else:
                    m = numpy_morph(mesh, dp, dn, ws[k])
                    e.insert_mesh(8000 + k, numpy_lbs(m, jt, wt, poses[k]) if skinned else m)
                    e.insert_instance(7000 + k, Instance(8000 + k, 7000, xform(POSITIONS[k])))
            t1 = time.perf_counter()
            a.record(s)
            e.tick(s.cuda_stream)
            t2 = time.perf_counter()
            b.record(s)
            torch.cuda.synchronize()
            if t >= WARMUP:
                host[name].append(((t2 - t1) if name == "device" else (t2 - t0)) * 1e3)
                dev[name].append(a.elapsed_time(b))
    out = {k: {"host_ms": round(float(np.median(host[k])), 4), "device_ms": round(float(np.median(dev[k])), 4)} for k in engines}
    out["device"]["morphing_stats"] = list(engines["device"].morphing_stats()); out["device"]["skinning_stats"] = list(engines["device"].skinning_stats())
    gbps = engines["device"].copy_bandwidth()
    for e in engines.values():
        e.close()
    return out, gbps


def kernel_time(case):
    """One rocprofv3 child for the case: (median-free) average ns and calls of k_morph from its kernel_stats.csv; None where rocprofv3 is missing."""
    tool = shutil.which("rocprofv3")
    if tool is None:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [tool, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", case]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit(f"the rocprofv3 child of {case} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    if "k_morph" in row["Name"]:
                        return {"us": round(float(row["AverageNs"]) / 1e3, 2), "calls": int(row["Calls"])}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morphing.json"))
    ap.add_argument("--no-kernel-times", action="store_true", help="skip the rocprofv3 child processes")
    ap.add_argument("--child", choices=sorted(CASES), help="path (a) of one case alone (what the rocprofv3 child runs)")
    args = ap.parse_args()
    if args.child:
        active, skinned = CASES[args.child]
        run_case(active, skinned, tube_with_targets(), device_only=True, ticks=10)
        return
    kernels = {} if args.no_kernel_times else {c: kernel_time(c) for c in CASES}   # (before this process opens the device)
    data = tube_with_targets()
    tris = TUBES * len(data[0].positions)
    rec = {"scene": "dungeon_13k + 16 tubes", "triangles_morphed_per_tick": tris, "targets": TARGETS, "joints": JOINTS, "ticks": TICKS, "warmup": WARMUP,
           "build": "fast", "cases": {}}
    for case, (active, skinned) in CASES.items():
        res, gbps = run_case(active, skinned, data)
        rec["copy_ceiling_gb_per_s"] = round(gbps, 1)
        res["tick_ratio_host_over_device"] = round(res["host_numpy_and_mesh_insert"]["host_ms"] / res["device"]["host_ms"], 2)
        moved = tris * (96 + 96 + 72 * active + (72 if skinned else 0))
        res["compulsory_bytes_per_launch"] = moved
        if kernels.get(case):
            k = dict(kernels[case]); k["gb_per_s"] = round(moved / k["us"] / 1e3, 1); k["share_of_copy_ceiling"] = round(k["gb_per_s"] / gbps, 3)
            res["k_morph"] = k
        rec["cases"][case] = res
        print(case, json.dumps(res), flush=True)
    json.dump(rec, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
