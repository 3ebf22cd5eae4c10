#!/usr/bin/env python3
"""Cost of the per-pixel AOV launch (include/strolle_hip.h "per-pixel AOVs"; k_aov.hip) in the default (fast) build: one JSON line per case.

Scenes: Cornell, the 13 k-triangle dungeon, BASELINE config 3's 208 k-triangle dungeon (subdivide = 2), each through its benchmark camera
at 1920 x 1080 after one rendered frame. Planes: all six, and DEPTH + MOTION only (what a temporal upscaler asks for).
Timing: device events around 20 launches after 5 warm-up launches on one stream; ms per launch.

  python tools/aov_bench.py [--out profiles/aov.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

from strolle_amd import Aov, Engine, aov_planes, scenes

WARMUP, LAUNCHES = 5, 20
SIZE = (1920, 1080)


def time_launches(launch):
    s = torch.cuda.current_stream()
    for _ in range(WARMUP):
        launch(s.cuda_stream)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(s)
    for _ in range(LAUNCHES):
        launch(s.cuda_stream)
    stop.record(s)
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / LAUNCHES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    lines = []
    cases = (("cornell", scenes.build_cornell, scenes.cornell_camera),
             ("dungeon_13k", scenes.build_dungeon, scenes.dungeon_camera),
             ("dungeon_208k_config3", lambda e: scenes.build_dungeon(e, subdivide=2), scenes.dungeon_camera))
    for name, build, camera in cases:
        e = Engine(device=0)
        build(e)
        cam = e.create_camera(camera(SIZE))
        e.tick()
        out = torch.zeros((SIZE[1], SIZE[0], 4), dtype=torch.float32, device="cuda")
        e.render_camera(cam, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        planes = aov_planes(SIZE, fill=0)
        for label, kinds in (("all", tuple(Aov)), ("depth_motion", (Aov.DEPTH, Aov.MOTION))):
            want = {k: planes[k] for k in kinds}
            ms = time_launches(lambda s: e.render_aovs(cam, want, stream=s))
            store_bytes = sum(planes[k].element_size() * planes[k].numel() for k in kinds)
            hit = float((planes[Aov.DEPTH] < 3.0e38).float().mean())
            line = {"scene": name, "size": list(SIZE), "planes": label, "ms": round(ms, 4), "store_bytes": store_bytes,
                    "store_gb_per_s": round(store_bytes / (ms * 1e-3) / 1e9, 1), "hit_fraction": round(hit, 4),
                    "launches": LAUNCHES, "warmup": WARMUP, "build": "fast"}
            print(json.dumps(line), flush=True)
            lines.append(line)
        e.close()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
