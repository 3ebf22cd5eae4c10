#!/usr/bin/env python3
"""Normal mapping (include/strolle_hip.h "normal mapping") in numbers, merged into profiles/normal_mapping.json; keys of other sections are kept.

  (default)            dungeon and Cornell at 1920x1080, Image{denoise}, the default (fast) build, a synthetic 512 x 512 bump map on EVERY material; fresh
                       engines in the order off on off on, ms per frame from events around FRAMES frames after WARMUP; and the dungeon under
                       ST_BVH_REBUILD with one torus moved every tick, ms per tick + frame                                      -> "frames"
  --kernel-stats       prim_visibility's time with the switch off and on, from one `rocprofv3 --kernel-trace --stats` child run  -> "prim_visibility"
  --abab PARENT        bench.py of the built parent tree against this tree's, parent this parent this (tools/chain_bench.py abab) -> "*_abab_ms_per_step",
                       judged by the spread of the parent's own runs
  --cpu                no GPU: the restatement against the definition (tests/normal_map_cases.py measure)                      -> "cpu"
  --resources PARENT   no GPU: hipcc's kernel-resource-usage remarks of every k_prim_visibility, k_aov and k_query_* instantiation, both arithmetic
                       builds, the parent tree's sources against this tree's                                                   -> "resource_usage"
  --gpu-tests LOG      the worst deviations a `pytest -s tests/test_gpu_normal_map.py` log reports                              -> "gpu"

  python tools/normal_map_bench.py [--out profiles/normal_mapping.json] [--kernel-stats] [--abab ../parent]"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import chain_bench as cb

MAP_HANDLE, MAP_SIZE = 9000, 512
KERNELS = ("k_trace", "k_aov", "k_query")
BUILD_FLAGS = {"exact": ["-ffp-contract=off", "-DST_KNS=exact"], "fast": ["-ffp-contract=fast-honor-pragmas", "-DST_KNS=fast", "-DST_FAST_MATH=1"]}


def bump_map(size=MAP_SIZE):
    """a tangent-space map of overlapping sine bumps: the normal of the height field h(x, y), encoded the glTF way"""
    y, x = np.mgrid[0:size, 0:size] / size
    two_pi = 2.0 * np.pi
    dx = 0.35 * np.cos(two_pi * 8 * x) * np.cos(two_pi * 3 * y) + 0.2 * np.cos(two_pi * 31 * x)
    dy = -0.35 * np.sin(two_pi * 8 * x) * np.sin(two_pi * 3 * y) + 0.2 * np.cos(two_pi * 23 * y)
    n = np.stack([-dx, -dy, np.ones_like(dx)], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    rgba = np.full((size, size, 4), 255, np.uint8)
    rgba[..., :3] = np.round((0.5 * n + 0.5) * 255.0)
    return rgba


class EveryMaterialMapped:
    """the engine, as a scene builder sees it: every material it is handed gets the bump map"""

    def __init__(self, e):
        self._e = e
        e.insert_image(MAP_HANDLE, bump_map())

    def __getattr__(self, name):
        return getattr(self._e, name)

    def insert_material(self, handle, material):
        material.normal_map_texture = MAP_HANDLE
        self._e.insert_material(handle, material)


def run(scene, on, frames=cb.FRAMES, warmup=cb.WARMUP, moving=False):
    """moving: ST_BVH_REBUILD and one torus re-inserted at another height before every tick — the tree is the host's every tick, so every tick's copy of the
    scene gets its hit-test records with the tick's upload while the switch is on (st_tick.cpp upload_scene)"""
    import torch
    from strolle_amd import Engine, Instance, scenes
    e = Engine(device=0)
    if moving:
        e.set_bvh_refresh(0)
    (scenes.build_cornell if scene == "cornell" else scenes.build_dungeon)(EveryMaterialMapped(e))
    e.set_seed(7)
    e.set_normal_mapping(on)
    cam = e.create_camera(cb.camera(scene, 0, False))
    w, h = cb.HD
    out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    s = torch.cuda.Stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in range(warmup + frames):
        if k == warmup:
            torch.cuda.synchronize(); a.record(s)
        if moving:
            t = scenes.DUNGEON_TORI[0]
            c1, s1 = np.cos(1.0), np.sin(1.0)
            x = np.array([[0.5 * c1, -0.5 * s1, 0.0, t[0]], [0.5 * s1, 0.5 * c1, 0.0, t[1] + 0.05 * np.sin(0.3 * k)], [0.0, 0.0, 0.5, t[2]]], np.float32)
            e.insert_instance(5001, Instance(5000, 5001, x))
        e.tick(s.cuda_stream)
        e.render_camera(cam, out.data_ptr(), s.cuda_stream)
    b.record(s); torch.cuda.synchronize()
    e.close()
    return a.elapsed_time(b) / frames


def frames_record():
    rec = {}
    for scene in ("dungeon", "cornell"):
        series = {"off": [], "on": []}
        for setting in ("off", "on", "off", "on"):
            series[setting].append(round(run(scene, setting == "on"), 4))
        rec[scene] = {"size": list(cb.HD), "mode": "Image{denoise}", "build": "fast", "frames": cb.FRAMES, "warmup": cb.WARMUP, "order": "off on off on",
                      "map": f"{MAP_SIZE} x {MAP_SIZE} on every material", "ms_per_frame": series,
                      "on_minus_off": round(sum(series["on"]) / 2 - sum(series["off"]) / 2, 4), "off_spread": round(abs(series["off"][0] - series["off"][1]), 4)}
    # a moving scene over a host tree: wall time per tick + frame, the host's rebuild included (the same in both settings)
    series = {"off": [], "on": []}
    for setting in ("off", "on", "off", "on"):
        series[setting].append(round(run("dungeon", setting == "on", frames=60, warmup=10, moving=True), 4))
    rec["dungeon_moving_rebuild"] = {"size": list(cb.HD), "mode": "Image{denoise}", "build": "fast", "refresh": "ST_BVH_REBUILD, one torus moved every tick", "frames": 60, "warmup": 10,
                                     "order": "off on off on", "ms_per_tick_and_frame": series, "on_minus_off": round(sum(series["on"]) / 2 - sum(series["off"]) / 2, 4),
                                     "off_spread": round(abs(series["off"][0] - series["off"][1]), 4)}
    return rec


def kernel_stats():
    out = {}
    for scene in ("dungeon", "cornell"):
        rows, _ = cb.kernel_trace(__file__, ("--profile-child", scene), name="normal_map")
        us = cb.dispatch_us(rows, "k_prim_visibility")
        half = len(us) // 2                      # the child renders its frames with the switch off, then as many with it on
        steady = lambda v: v[len(v) // 4:]       # (the first quarter of each half warms up)
        out[scene] = {"off": cb.dispatch_record(steady(us[:half]))[0], "on": cb.dispatch_record(steady(us[half:]))[0]}
    return out


def profile_child(scene, frames=40):
    import torch
    from strolle_amd import Engine, scenes
    e = Engine(device=0)
    (scenes.build_cornell if scene == "cornell" else scenes.build_dungeon)(EveryMaterialMapped(e))
    e.set_seed(7)
    cam = e.create_camera(cb.camera(scene, 0, False))
    out = torch.zeros((cb.HD[1], cb.HD[0], 4), dtype=torch.float32, device="cuda:0")
    for on in (False, True):
        e.set_normal_mapping(on)
        for _ in range(frames):
            e.tick(); e.render_camera(cam, out.data_ptr(), 0)
        torch.cuda.synchronize()
    e.close()


# ----------------------------------------------------------------------------- no GPU
def resource_usage(parent):
    """{kernel instantiation: {"parent": {...}, "this": {...}}} from hipcc -Rpass-analysis=kernel-resource-usage (device pass only, nothing is kept)"""
    def remarks(tree, kernel, build):
        src = os.path.join(tree, "strolle_amd", "csrc")
        cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-fno-slp-vectorize"] + BUILD_FLAGS[build] + \
              ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", kernel + ".hip", "-o", os.devnull]
        text = subprocess.run(cmd, cwd=src, capture_output=True, text=True, check=True).stderr
        rows, cur = {}, None
        for line in text.splitlines():
            m = re.search(r"remark: .*Function Name: (\S+)", line)
            if m:
                name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
                cur = re.sub(r"^void st::", "", re.sub(r"\(.*", "", name)); rows[cur] = {}
                continue
            m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
            if m and cur:
                rows[cur][m.group(1).split(" [")[0]] = int(m.group(2))
        return {k: v for k, v in rows.items() if re.search(r"k_prim_visibility|k_aov|k_query", k)}

    table = {}
    for kernel in KERNELS:
        for build in BUILD_FLAGS:
            old, new = remarks(os.path.abspath(parent), kernel, build), remarks(ROOT, kernel, build)
            for name in new:
                table[name] = {"parent": old.get(name), "this": new[name]}
    worse = [k for k, v in table.items() if v["parent"] and (v["this"]["ScratchSize"] > v["parent"]["ScratchSize"] or v["this"]["Occupancy"] < v["parent"]["Occupancy"])]
    return {"flags": "Makefile BASE + the build's, --cuda-device-only, gfx950", "gained_scratch_or_lost_an_occupancy_step": worse, "kernels": table}


def cpu_record():
    import normal_map_cases as nc
    return {case: nc.measure(case) for case in nc.CASES}


def gpu_record(log):
    """{what: {"worst_angle_rad": ..., "deviation_over_tolerance": ...}} from the lines check_function prints"""
    out = {}
    for line in open(log):
        line = line.strip().lstrip(".")                 # (pytest's progress dots share the line)
        m = re.match(r"(.+?): (\d+) rays compared with the definition, worst angle (\S+) rad, worst deviation / tolerance (\S+);", line.strip())
        if m:
            out[m.group(1)] = {"rays": int(m.group(2)), "worst_angle_rad": float(m.group(3)), "deviation_over_tolerance": float(m.group(4))}
        m = re.match(r"(.+? default): (\d+) pixels, frame outputs against the flagged query, worst deviation / tolerance (\{.*\})", line.strip())
        if m:
            out[m.group(1) + " frame"] = {"pixels": int(m.group(2)), "deviation_over_twice_the_tolerance": json.loads(m.group(3).replace("'", '"'))}
        m = re.match(r"relative left - right luminance.*", line.strip())
        if m:
            out["lit quad"] = line.strip()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normal_mapping.json"))
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--abab", metavar="PARENT")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--resources", metavar="PARENT")
    ap.add_argument("--gpu-tests", metavar="LOG")
    ap.add_argument("--profile-child", metavar="SCENE", help="what --kernel-stats wraps in rocprofv3: frames with the switch off, then on, and nothing else")
    args = ap.parse_args()
    if args.profile_child:
        profile_child(args.profile_child)
        return 0
    rec = {}
    if args.cpu:
        rec["cpu"] = cpu_record()
    if args.resources:
        rec["resource_usage"] = resource_usage(args.resources)
    if args.gpu_tests:
        rec["gpu"] = gpu_record(args.gpu_tests)
    if not (args.cpu or args.resources or args.gpu_tests):
        rec["frames"] = frames_record()
        if args.kernel_stats:
            rec["prim_visibility"] = kernel_stats()
        if args.abab:
            rec.update(cb.abab(args.abab, "normal_mapping"))
    cb.merge(args.out, rec)
    return 0


if __name__ == "__main__":
    sys.exit(main())
