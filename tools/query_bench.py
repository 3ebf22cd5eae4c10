#!/usr/bin/env python3
"""Throughput of the scene queries (include/strolle_hip.h "scene queries"; k_query.hip) in the default (fast) build: one JSON line per case.

Scenes: Cornell, the 13 k-triangle dungeon, BASELINE config 3's 208 k-triangle dungeon (subdivide = 2). Rays per scene:
  incoherent   1 M rays, origins uniform in the scene's box, directions uniform on the sphere, unbounded
  camera       the 1920 x 1080 camera rays of the scene's benchmark camera (2.07 M), ordered by 8 x 8 tiles (64 consecutive rays = one tile)
  camera_coherent  the same rays with ST_RAY_COHERENT (one packet per wave)
  occlusion    1 M rays of the incoherent set, t_max = a quarter of the box's diagonal
Timing: device events around 20 launches after 5 warm-up launches on one stream; ms per launch and Grays/s.

  python tools/query_bench.py [--out profiles/ray_query.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

from strolle_amd import Engine, scenes
from strolle_amd.api import HIT_DTYPE, RAY_DTYPE

WARMUP, LAUNCHES = 5, 20


def camera_rays_tiled(desc):
    """Camera::ray of every pixel (float64 unprojection, rounded to f32: timing only needs camera-like rays), tile-major in 8 x 8 tiles."""
    c = desc.to_c(); w, h = desc.size
    transform = np.array(c.transform[:], np.float64).reshape(4, 4).T
    projection = np.array(c.projection[:], np.float64).reshape(4, 4).T
    ndc_to_world = transform @ np.linalg.inv(projection)
    ty, tx, py, px = np.meshgrid(np.arange((h + 7) // 8), np.arange((w + 7) // 8), np.arange(8), np.arange(8), indexing="ij")
    x, y = (tx * 8 + px).ravel(), (ty * 8 + py).ravel()
    keep = (x < w) & (y < h)
    x, y = x[keep], y[keep]
    ndc = np.stack([(x + 0.5) * 2.0 / w - 1.0, -((y + 0.5) * 2.0 / h - 1.0)], 1)

    def unproject(z):
        p = np.concatenate([ndc, np.full((len(x), 1), z), np.ones((len(x), 1))], 1) @ ndc_to_world.T
        return p[:, :3] / p[:, 3:]
    near, far = unproject(1.0), unproject(float(np.finfo(np.float32).eps))
    d = far - near; d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros(len(x), RAY_DTYPE)
    r["origin"] = near; r["direction"] = d; r["t_max"] = np.inf
    return r


def incoherent_rays(lo, hi, n, rng, t_max=np.inf):
    r = np.zeros(n, RAY_DTYPE)
    r["origin"] = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    r["direction"] = d; r["t_max"] = t_max
    return r


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
    rng = np.random.default_rng(1)
    for name, build, camera in cases:
        e = Engine(device=0)
        build(e)
        e.tick()
        torch.cuda.synchronize()
        tris = e.read_scene(1).view(np.float32).reshape(-1, 9, 4)[:, [0, 3, 6], :3].reshape(-1, 3)
        lo, hi = tris.min(0), tris.max(0)
        diag = float(np.linalg.norm(hi - lo))
        sets = {"incoherent": incoherent_rays(lo, hi, 1 << 20, rng), "camera": camera_rays_tiled(camera((1920, 1080))),
                "occlusion": incoherent_rays(lo, hi, 1 << 20, rng, t_max=0.25 * diag)}
        dev = {k: torch.from_numpy(v.view(np.uint8).copy()).cuda() for k, v in sets.items()}
        n_max = max(len(v) for v in sets.values())
        hits = torch.empty(n_max * HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        occ = torch.empty(n_max, dtype=torch.int32, device="cuda")
        runs = (("incoherent", "incoherent", lambda s: e.trace_rays(dev["incoherent"].data_ptr(), len(sets["incoherent"]), hits.data_ptr(), stream=s)),
                ("camera", "camera", lambda s: e.trace_rays(dev["camera"].data_ptr(), len(sets["camera"]), hits.data_ptr(), stream=s)),
                ("camera_coherent", "camera", lambda s: e.trace_rays(dev["camera"].data_ptr(), len(sets["camera"]), hits.data_ptr(), coherent=True, stream=s)),
                ("occlusion", "occlusion", lambda s: e.occluded(dev["occlusion"].data_ptr(), len(sets["occlusion"]), occ.data_ptr(), stream=s)))
        for label, key, launch in runs:
            ms = time_launches(launch)
            n = len(sets[key])
            line = {"scene": name, "triangles": int(len(tris) // 3), "rays": label, "count": n, "ms": round(ms, 4),
                    "grays_per_s": round(n / (ms * 1e-3) / 1e9, 3), "launches": LAUNCHES, "warmup": WARMUP, "build": "fast"}
            if label == "camera":
                h = np.empty(len(sets["camera"]), HIT_DTYPE)
                h.view(np.uint8)[:] = hits[: h.nbytes].cpu().numpy()
                line["hit_fraction"] = round(float(h["hit"].mean()), 4)
            print(json.dumps(line), flush=True)
            lines.append(line)
        e.close()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
