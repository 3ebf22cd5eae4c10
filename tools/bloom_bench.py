#!/usr/bin/env python3
"""Cost of bloom (include/strolle_hip.h "bloom"; k_bloom.hip) in the default (fast) build. Every run MERGES its figures into --out.

  (default)  (a) ms per frame of Cornell and the dungeon at 1920x1080 Image{denoise} into RGBA8 sRGB with ACES: bloom off, on (the straightforward chain,
             the default), on with the fused tail, and off / on with FXAA + Catmull-Rom to 3840x2160 behind it (FRAMES frames after WARMUP,
             events around the whole run on one stream, interleaved twice);
             (b) the bloom chain alone (st_bloom_process on a 1080p image, back to back): launches and microseconds per chain for the
             straightforward chain and for each tail budget - the comparison that decides which chain ships;
             (c) the copy ceiling (st_debug_copy_bandwidth) and each launch's compulsory bytes (st_bloom.cpp bloom_steps).
  --profile-child       what `rocprofv3 --kernel-trace` wraps (no counters in that run): 40 chains with the tail, 40 without.
  --kernel-trace FILE   rocprofv3's kernel trace of that child (csv): each bloom launch's own time per dispatch, grouped by kernel and grid
                        size (= level), its bytes, its share of the copy ceiling, and the chain's summed kernel time.
  --abab PARENT         A B A B of bench.py at 1080p: PARENT/bench.py (the parent commit, built) against this tree's, both series.

  python tools/bloom_bench.py [--out profiles/bloom.json] [--profile-child | --kernel-trace FILE | --abab DIR]
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (before the library: torch's bundled HIP runtime has to be the first one loaded)

from chain_bench import BLOOM, FRAMES, HD, WARMUP, abab, merge  # noqa: E402

UHD = (3840, 2160)
# name: (bloom, post, tail budget: -1 the device's, 0 the straightforward chain)
VARIANTS = {"off": (False, False, 0), "bloom": (True, False, 0), "bloom_fused_tail": (True, False, -1), "post": (False, True, 0), "bloom_post": (True, True, 0)}


def frame_ms(scene, bloom, post, tail, frames=FRAMES):
    import torch
    from strolle_amd import CameraMode, Engine, OutputFormat, ResampleFilter, Tonemap, scenes
    e = Engine(device=0)
    (scenes.build_cornell if scene == "cornell" else scenes.build_dungeon)(e)
    e.set_seed(7)
    e.set_bloom_tail(tail)
    cam = e.create_camera((scenes.cornell_camera if scene == "cornell" else scenes.dungeon_camera)(HD, CameraMode.IMAGE))
    e.set_output_format(cam, OutputFormat.RGBA8_UNORM_SRGB)
    e.set_display(cam, tonemap=Tonemap.ACES_FITTED)
    if bloom:
        e.set_bloom(cam, **BLOOM)
    if post:
        e.set_post(cam, fxaa=True, output_size=UHD, filter=ResampleFilter.CATMULL_ROM)
    w, h = e.output_size(cam)
    out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
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


def tail_first(sizes, budget):
    """st_bloom.cpp bloom_tail_first"""
    t, used = len(sizes), 0
    while t > 1 and used + sizes[t - 1][0] * sizes[t - 1][1] * 12 <= budget:
        used += sizes[t - 1][0] * sizes[t - 1][1] * 12
        t -= 1
    return t


def launches(sizes, budget):
    """[(kernel, grid size in threads, label, compulsory bytes)] of one chain at 1080p into RGBA8 (st_bloom.cpp bloom_steps)"""
    blocks = lambda w, h: ((w + 31) // 32) * ((h + 7) // 8) * 256
    L, T, out, src = len(sizes), tail_first(sizes, budget), [], HD
    for k in range(T):
        w, h = sizes[k]
        out.append(("k_bloom_down<true>" if k == 0 else "k_bloom_down<false>", blocks(w, h), f"down {k} ({src[0]}x{src[1]} -> {w}x{h})", (src[0] * src[1] + w * h) * 16))
        src = (w, h)
    if T < L:
        bw, bh = sizes[T - 1]
        out.append(("k_bloom_tail", 1024, f"tail levels {T}..{L - 1} (from and into {bw}x{bh})", bw * bh * 48))
    for k in range(T - 1, 0, -1):
        (sw, sh), (dw, dh) = sizes[k], sizes[k - 1]
        out.append(("k_bloom_up<false>", blocks(dw, dh), f"up {k} ({sw}x{sh} -> {dw}x{dh})", sw * sh * 16 + dw * dh * 32))
    out.append(("k_bloom_up<true>", blocks(*HD), f"composite ({sizes[0][0]}x{sizes[0][1]} -> {HD[0]}x{HD[1]} RGBA8)", sizes[0][0] * sizes[0][1] * 16 + HD[0] * HD[1] * 20))
    return out


def chain(e, tail, n, img=None):
    """n bloom chains over a 1080p image back to back; returns (us per chain, the budget in force)"""
    import torch
    from strolle_amd import Tonemap, bloom_desc, display_desc
    in_force = e.set_bloom_tail(tail)
    img = img if img is not None else torch.rand((HD[1], HD[0], 4), device="cuda:0") * 4.0
    out = torch.zeros((HD[1], HD[0], 4), dtype=torch.uint8, device="cuda:0")
    d, disp = bloom_desc(**BLOOM), display_desc(tonemap=Tonemap.ACES_FITTED)
    s = torch.cuda.Stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in range(20 + n):
        if k == 20:
            torch.cuda.synchronize(); a.record(s)
        e.bloom_process(d, img.data_ptr(), HD[0], HD[1], out.data_ptr(), 2, display=disp, stream=s.cuda_stream)
    b.record(s); torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n, in_force


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bloom.json"))
    ap.add_argument("--profile-child", action="store_true")
    ap.add_argument("--kernel-trace")
    ap.add_argument("--abab")
    ap.add_argument("--chains-only", action="store_true", help="only (b) and (c)")
    args = ap.parse_args()
    if args.abab:
        merge(args.out, abab(args.abab, "bloom_off", (("bench_py_1080p", []),), flags=()))
        return
    from strolle_amd import Engine, bloom_desc
    if args.profile_child:
        e = Engine(device=0)
        for tail in (-1, 0):
            chain(e, tail, 20)
        e.close()
        return
    e = Engine(device=-1)   # the plan is host arithmetic
    sizes = e.bloom_plan(bloom_desc(**BLOOM), *HD)[1]
    e.close()
    if args.kernel_trace:
        rec = json.load(open(args.out))
        ceiling, limit = rec["copy_ceiling_gb_s"], rec["tail_lds_bytes_in_force"]
        with open(args.kernel_trace) as f:
            rows = list(csv.DictReader(f))
        gkey = next(k for k in rows[0] if k.lower() in ("grid_size_x", "grid_size"))
        times = {}
        for r in rows:
            if "k_bloom" in r["Kernel_Name"]:
                times.setdefault((r["Kernel_Name"], int(r[gkey])), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        out = {}
        for cname, budget in (("fused_tail", limit), ("straightforward", 0)):
            per, total = {}, 0.0
            for kernel, grid, label, nbytes in launches(sizes, budget):
                hit = [v for (kn, g), v in times.items() if g == grid and kernel.split("<")[0] in kn]   # (kernel, grid size) names the level
                us = sorted(hit[0])[len(hit[0]) // 2] if hit else None
                per[label] = {"kernel": kernel, "median_us": None if us is None else round(us, 2), "dispatches": len(hit[0]) if hit else 0, "bytes": nbytes,
                              "share_of_copy_ceiling": None if us is None else round(nbytes / (us * 1e-6) / (ceiling * 1e9), 3)}
                total += us or 0.0
            out[cname] = {"launches": len(per), "sum_of_kernel_us": round(total, 2), "per_launch": per}
        merge(args.out, {"kernel_trace": out})
        return
    rec = {"render_size": list(HD), "mode": "Image{denoise}", "format": "RGBA8_UNORM_SRGB", "display": "ACES_FITTED", "build": "fast", "frames": FRAMES,
           "warmup": WARMUP, "bloom": BLOOM, "post": "FXAA + Catmull-Rom to 3840x2160"}
    for scene in (() if args.chains_only else ("cornell", "dungeon")):
        rec[scene + "_ms_per_frame"] = {}
        for _ in range(2):   # interleaved twice: the spread of one box
            for name, (bloom, post, tail) in VARIANTS.items():
                rec[scene + "_ms_per_frame"].setdefault(name, []).append(round(frame_ms(scene, bloom, post, tail), 4))
    e = Engine(device=0)
    rec["copy_ceiling_gb_s"] = round(float(e.copy_bandwidth()), 1)
    rec["tail_lds_bytes_in_force"] = e.set_bloom_tail(-1)
    chains = rec["chain_alone_1080p_six_levels"] = {}
    for _ in range(2):
        for name, tail in (("straightforward", 0), ("tail_64KiB", 64 << 10), ("tail_device_limit", -1)):
            us, in_force = chain(e, tail, 300)
            c = chains.setdefault(name, {"lds_budget": in_force, "first_tail_level": tail_first(sizes, in_force), "launches": len(launches(sizes, in_force)), "us_per_chain": []})
            c["us_per_chain"].append(round(us, 2))
    e.close()
    rec["launch_bytes_default_chain"] = {label: b for _, _, label, b in launches(sizes, rec["tail_lds_bytes_in_force"])}
    merge(args.out, rec)


if __name__ == "__main__":
    main()
