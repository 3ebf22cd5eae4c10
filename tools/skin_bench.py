#!/usr/bin/env python3
"""Cost of skinned meshes per tick (include/strolle_hip.h "skinned meshes"; k_skin.hip) in the default (fast) build, default tuning.

Scene: the dungeon (13 k triangles) + 16 tubes of 8,192 triangles and 32 joints (scenes.skinned_tube), every tube re-posed every tick.
  (a) the new path: st_instance_set_pose for each tube, then st_tick — host ms of st_tick, and device ms of the tick's work (events recorded
      on the tick's stream right before and after st_tick: the skin, bake and tree work of the tick is ordered before the second event);
  (b) the way without skinning, on the same box in the same run: linear blend skinning in numpy on the host, then st_mesh_insert + st_instance_insert
      of every tube, then st_tick — host ms of all of that (numpy included), device ms of st_tick's work as in (a).
Medians over TICKS ticks after WARMUP. The skin kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of
`--only-new`; `--kernel-stats <kernel_stats.csv or rocpd .db>` puts its figure and its bytes / us against st_debug_copy_bandwidth into the JSON.

  python tools/skin_bench.py [--out profiles/skinning.json] [--only-new] [--kernel-stats FILE]
"""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

from strolle_amd import Engine, Instance, Material, Mesh, scenes

WARMUP, TICKS = 5, 40
TUBES, SEGMENTS, SIDES, JOINTS = 16, 128, 32, 32
POSITIONS = [(-5.75 + 0.7 * (k % 4 - 1.5), 0.0, -19.0 - 0.9 * (k // 4)) for k in range(TUBES)]


def xform(p):
    return np.array([[1, 0, 0, p[0]], [0, 1, 0, p[1]], [0, 0, 1, p[2]]], np.float32)


def numpy_lbs(mesh, jt, wt, pose):
    """Linear blend skinning of positions and normals on the host (what an application does without st_instance_set_pose)."""
    n = len(mesh.positions)
    M = np.einsum("ck,ckij->cij", wt, pose[jt.astype(np.int64)])            # (3n, 3, 4)
    p = np.einsum("cij,cj->ci", M[:, :, :3], mesh.positions.reshape(-1, 3)) + M[:, :, 3]
    nrm = np.einsum("cij,cj->ci", np.linalg.inv(M[:, :, :3]).transpose(0, 2, 1), mesh.normals.reshape(-1, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return Mesh(p.reshape(n, 3, 3), nrm.reshape(n, 3, 3), mesh.uvs, mesh.tangents)


def run(new_path, mesh, jt, wt):
    e = Engine(device=0)
    scenes.build_dungeon(e)
    e.insert_material(7000, Material(base_color=(0.2, 0.7, 0.3, 1.0)))
    if new_path:
        e.insert_mesh(7000, mesh); e.set_skin(7000, jt, wt, JOINTS)
    for k, p in enumerate(POSITIONS):
        if not new_path:
            e.insert_mesh(8000 + k, mesh)
        e.insert_instance(7000 + k, Instance(7000 if new_path else 8000 + k, 7000, xform(p)))
    s = torch.cuda.Stream()
    e.tick(s.cuda_stream); torch.cuda.synchronize()
    host, dev = [], []
    for t in range(WARMUP + TICKS):
        poses = [scenes.bend_pose(JOINTS, 1.5, 0.1 * t + k) for k in range(TUBES)]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(TUBES):
            if new_path:
                e.set_pose(7000 + k, poses[k])
            else:
                e.insert_mesh(8000 + k, numpy_lbs(mesh, jt, wt, poses[k]))
                e.insert_instance(7000 + k, Instance(8000 + k, 7000, xform(POSITIONS[k])))
        t1 = time.perf_counter()
        a.record(s)   # (after the host's own work of the tick: the device interval holds the tick's device work only)
        e.tick(s.cuda_stream)
        t2 = time.perf_counter()
        b.record(s)
        torch.cuda.synchronize()
        if t >= WARMUP:
            host.append(((t2 - t1) if new_path else (t2 - t0)) * 1e3)
            dev.append(a.elapsed_time(b))
    stats = e.skinning_stats()
    gbps = e.copy_bandwidth()
    e.close()
    return {"host_ms": round(float(np.median(host)), 4), "device_ms": round(float(np.median(dev)), 4), "skinning_stats": list(stats)}, gbps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "skinning.json"))
    ap.add_argument("--only-new", action="store_true", help="path (a) only (the rocprofv3 run)")
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel_stats.csv of an --only-new run: adds the skin kernel's time to --out")
    args = ap.parse_args()
    mesh, jt, wt = scenes.skinned_tube(SEGMENTS, SIDES, JOINTS)
    tris = TUBES * len(mesh.positions)
    if args.kernel_stats:
        rec = json.load(open(args.out))
        if args.kernel_stats.endswith(".db"):   # rocprofv3's default output (rocpd SQLite): the median dispatch
            import sqlite3
            d = [r[0] for r in sqlite3.connect(args.kernel_stats).execute("select duration from kernels where name like '%k_skin%'")]
            us, calls = float(np.median(d)) / 1e3, len(d)
        else:                                   # --output-format csv: kernel_stats.csv
            with open(args.kernel_stats) as f:
                row = next(r for r in csv.DictReader(f) if "k_skin" in r["Name"])
            us, calls = float(row["AverageNs"]) / 1e3, int(row["Calls"])
        moved = tris * (96 + 72 + 96)   # per triangle: bind pose read, skin read, posed triangles written
        rec["skin_kernel"] = {"us": round(us, 2), "calls": calls, "bytes": moved, "gb_per_s": round(moved / us / 1e3, 1),
                              "share_of_copy_ceiling": round(moved / us / 1e3 / rec["copy_ceiling_gb_per_s"], 3)}
        json.dump(rec, open(args.out, "w"), indent=1)
        print(json.dumps(rec["skin_kernel"]))
        return
    new, gbps = run(True, mesh, jt, wt)
    rec = {"scene": "dungeon_13k + 16 tubes", "triangles_posed_per_tick": tris, "joints": JOINTS, "ticks": TICKS, "warmup": WARMUP, "build": "fast",
           "new_path": new, "copy_ceiling_gb_per_s": round(gbps, 1)}
    if not args.only_new:
        rec["host_lbs_and_mesh_insert"], _ = run(False, mesh, jt, wt)
        json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
