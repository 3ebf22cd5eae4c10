#!/usr/bin/env python3
"""Host time of st_render_camera per frame with all five HDR nodes of the output chain on (fog, light shafts, depth of field, motion blur,
bloom), on the Cornell scene at 64 x 48 and at 1920 x 1080: one JSON line. The device is idle before every timed call, so the figure is
what the call itself spends enqueueing the frame. STROLLE_HIP_LIB selects another build of the library (same-box A/B of two commits).

    python tools/output_chain_host_cost.py [frames]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

from strolle_amd import CameraMode, Engine, bloom_desc, dof_desc, fog_desc, light_shafts_desc, motion_blur_desc, scenes
from strolle_amd.api import LIB_PATH, library_build_commit

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 300
result = {"library": os.environ.get("STROLLE_HIP_LIB", "the tree's"), "commit": library_build_commit(LIB_PATH), "frames": frames, "unit": "us per st_render_camera call"}
stream = torch.cuda.current_stream().cuda_stream
for size in ((64, 48), (1920, 1080)):
    e = Engine(device=0)
    scenes.build_cornell(e); e.set_seed(7)
    desc = scenes.cornell_camera(size, CameraMode.IMAGE)
    cam = e.create_camera(desc)
    e.set_fog(cam, fog_desc(density=0.1, height_falloff=0.25))
    e.set_light_shafts(cam, light_shafts_desc(steps=4, lights=(1,), sun_color=(1.0, 1.0, 1.0), sun_direction=(0.35, 0.8, 0.3)))
    e.set_dof(cam, dof_desc(focal_distance=3.0, sensor_height=0.5))
    e.set_motion_blur(cam, motion_blur_desc())
    e.set_bloom(cam, bloom_desc())
    out = torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda:0")
    times = []
    for k in range(24 + frames):
        e.update_camera(cam, desc); e.tick(stream)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.render_camera(cam, out.data_ptr(), stream)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        if k >= 24:
            times.append((t1 - t0) * 1e6)
    times.sort()
    result[f"{size[0]}x{size[1]}"] = {"median": round(statistics.median(times), 2), "p10": round(times[len(times) // 10], 2), "p90": round(times[len(times) * 9 // 10], 2),
                                      "mean": round(statistics.fmean(times), 2)}
    e.close()
print(json.dumps(result), flush=True)
