#!/usr/bin/env python3
"""Cost of environment lighting (include/strolle_hip.h "environment lighting"; k_env.hip, k_gi.hip) in the default (fast) build.

  (a) ms per frame of Cornell and the dungeon at 1920x1080 Image{denoise}: the atmosphere, a 2048x1024 map with importance sampling, and the
      same map with ST_ENV_UNIFORM_SAMPLING (FRAMES frames after WARMUP, events around the whole run on one stream);
  (b) what setting a map costs at the tick that uploads it (host wall time of st_tick, synchronised, minus a tick that uploads nothing):
      2048x1024 and 8192x4096, from host memory and from device memory;
  (c) the GI sampling kernels' own times come from a separate `rocprofv3 --kernel-trace --stats` run of `--profile-child`;
      `--kernel-stats <kernel_stats.csv or rocpd .db>` adds them to the JSON.

  python tools/env_bench.py [--out profiles/environment.json] [--profile-child] [--only-upload] [--kernel-stats FILE]
"""
import argparse
import csv
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

from strolle_amd import CameraMode, Engine, scenes

WARMUP, FRAMES, SIZE = 20, 120, (1920, 1080)


def studio_map(h, w):
    """a sun-like disc of 2e4 over ~0.05 % of the sphere, 35 degrees up, on a dim sky gradient"""
    v = (np.arange(h, dtype=np.float32) + 0.5) / h
    u = (np.arange(w, dtype=np.float32) + 0.5) / w
    th, ph = math.pi * v[:, None], 2 * math.pi * (u[None, :] - 0.5)
    c = np.array([0.3, 0.57, 0.76], np.float32); c /= np.linalg.norm(c)
    cosang = np.sin(th) * np.sin(ph) * c[0] + np.cos(th) * c[1] - np.sin(th) * np.cos(ph) * c[2]
    sky = (0.1 + 0.4 * np.clip(np.cos(th), 0, 1)) * np.ones_like(ph)
    m = np.stack([sky * 0.6, sky * 0.8, sky], -1).astype(np.float32)
    m[cosang >= 1 - 1e-3] = 2e4
    return m


def frame_ms(scene, env, uniform=False, frames=FRAMES):
    e = Engine(device=0)
    (scenes.build_cornell if scene == "cornell" else scenes.build_dungeon)(e)
    e.set_seed(7)
    if env is not None:
        e.set_environment(env, uniform=uniform)
    cam = e.create_camera((scenes.cornell_camera if scene == "cornell" else scenes.dungeon_camera)(SIZE, CameraMode.IMAGE))
    out = torch.zeros((SIZE[1], SIZE[0], 4), dtype=torch.float32, device="cuda:0")
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


def upload_ms(h, w, device):
    e = Engine(device=0)
    scenes.build_cornell(e)
    e.tick(); torch.cuda.synchronize()
    m = studio_map(h, w)
    src = torch.from_numpy(m).cuda() if device else m
    torch.cuda.synchronize()
    idle = []
    for _ in range(5):   # ticks that upload nothing
        t0 = time.perf_counter(); e.tick(); torch.cuda.synchronize(); idle.append(time.perf_counter() - t0)
    idle = float(np.median(idle))
    t0 = time.perf_counter()
    e.set_environment(src)
    t1 = time.perf_counter()
    e.tick(); torch.cuda.synchronize()
    t2 = time.perf_counter()
    e.close()
    return {"set_call_ms": round((t1 - t0) * 1e3, 3), "tick_ms": round((t2 - t1 - idle) * 1e3, 3)}


def upload_all():
    return {f"{w}x{h}_{'device' if d else 'host'}": upload_ms(h, w, d) for (w, h) in ((2048, 1024), (8192, 4096)) for d in (False, True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "environment.json"))
    ap.add_argument("--profile-child", action="store_true", help="Cornell frames with the map and importance sampling only (the rocprofv3 run)")
    ap.add_argument("--only-upload", action="store_true", help="(b) only, into an existing --out")
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel stats of a --profile-child run: adds the GI sampling kernels' times to --out")
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
        rec["kernels_us"] = {k: {"us": round(us, 2), "calls": n} for k, (us, n) in sorted(rows.items()) if "k_gi_sampling" in k or "k_di_resolving" in k or "k_env" in k}
        json.dump(rec, open(args.out, "w"), indent=1)
        print(json.dumps(rec["kernels_us"], indent=1))
        return
    if args.profile_child:   # 2 x 60 frames: the atmosphere first, then the map (the kernels' names tell them apart: the map's are the <.., true, ..> instances)
        frame_ms("cornell", None, frames=60)
        frame_ms("cornell", studio_map(1024, 2048), frames=60)
        return
    if args.only_upload:
        rec = json.load(open(args.out))
        rec["set_environment"] = upload_all()
        json.dump(rec, open(args.out, "w"), indent=1)
        print(json.dumps(rec["set_environment"], indent=1))
        return
    env = studio_map(1024, 2048)
    rec = {"size": list(SIZE), "mode": "Image{denoise}", "build": "fast", "frames": FRAMES, "warmup": WARMUP, "map": "2048x1024, disc of 2e4 over 0.05 % of the sphere"}
    for scene in ("cornell", "dungeon"):
        rec[scene] = {}
        for _ in range(2):   # interleaved twice: the spread of one box
            for name, m, uni in (("atmosphere", None, False), ("map_is", env, False), ("map_uniform", env, True)):
                rec[scene].setdefault(name, []).append(round(frame_ms(scene, m, uni), 4))
    rec["set_environment"] = upload_all()
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
