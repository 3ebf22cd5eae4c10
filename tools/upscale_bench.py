#!/usr/bin/env python3
"""Cost of the upscale stage (include/strolle_hip.h "upscaling"; k_upscale.hip) in the default (fast) build. Every run MERGES its figures
into --out.

  (default)  (a) ms per frame of Cornell and the dungeon at 1920x1080 Image{denoise} into RGBA8 sRGB with ACES: the stage off, the upscaler to
             3840x2160 alone, upscale + sharpen as two launches and as one (three tile shapes), sharpen alone, FXAA in front of upscale + sharpen, and the Catmull-Rom resampler to the
             same size — the reference cost, measured in the same run — FRAMES frames after WARMUP, events around the whole run on one
             stream, interleaved twice;
             (b) the copy ceiling (st_debug_copy_bandwidth) and the launches' compulsory bytes (st_upscale.cpp upscale_plan).
  --restatement         CPU only: the worst deviation of the numpy restatement from its float64 definition over the tests' matrix
                        (tests/test_upscale_abi.py restatement_vs_definition), the tolerance (four times that) and the r2 margin the GPU
                        test reads, the smallest weight sum seen, and the slanted-edge RMS errors against Catmull-Rom's.
  --kernel-stats        one `rocprofv3 --kernel-trace --stats` child run of its own (no counters), on the serial schedule: each kernel per
                        dispatch against bytes / copy ceiling, the fused launch's three tile shapes against the two launches' sum, the
                        Catmull-Rom resampler re-measured in the same run.
  --profile-child       what that run wraps.
  --abab PARENT         A B A B A B of bench.py (the headline and the dungeon at 1080p): PARENT/bench.py (the parent commit, built) against
                        this tree's, the stage off.

  python tools/upscale_bench.py [--out profiles/upscale.json] [--restatement | --kernel-stats | --profile-child | --abab DIR]
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # upscale_ref.py, upscale_cases.py, test_upscale_abi.py: the restatement's deviation

from chain_bench import FRAMES, HD, WARMUP, abab, kernel_stats, merge, run_frames  # noqa: E402

UHD = (3840, 2160)
# name: the camera setters of the variant
VARIANTS = {"off": {}, "upscale_2160p": dict(set_upscale=dict(output_size=UHD)), "upscale_sharpen_2160p": dict(set_upscale=dict(output_size=UHD, sharpness=0.5, denoise=True)),
            "sharpen_1080p": dict(set_upscale=dict(sharpness=0.5, denoise=True)),
            "fxaa_upscale_sharpen_2160p": dict(set_post=dict(fxaa=True), set_upscale=dict(output_size=UHD, sharpness=0.5, denoise=True)),
            "catmull_rom_2160p": dict(set_post=dict(output_size=UHD, filter=2)), "fxaa_catmull_rom_2160p": dict(set_post=dict(fxaa=True, output_size=UHD, filter=2))}
FUSED = {"upscale_sharpen_2160p_fused_64x8": 1, "upscale_sharpen_2160p_fused_32x32": 2, "upscale_sharpen_2160p_fused_64x16": 3}   # ST_UPSCALE_FUSED (st_debug_set_upscale_fused)
VARIANTS.update({k: VARIANTS["upscale_sharpen_2160p"] for k in FUSED})
CHILD = ("upscale_2160p", "upscale_sharpen_2160p", "sharpen_1080p", "catmull_rom_2160p") + tuple(FUSED)
CHILD_FRAMES, CHILD_WARMUP = 30, 10


def frames(scene, name, **kw):
    """chain_bench.run_frames of a variant, the fused ones with their tile in the environment the engine reads at creation"""
    os.environ["ST_UPSCALE_FUSED"] = str(FUSED.get(name, 0))
    try:
        return run_frames(scene, VARIANTS[name], **kw)
    finally:
        del os.environ["ST_UPSCALE_FUSED"]


def launch_bytes():
    """compulsory bytes of the timed launches (st_upscale.cpp upscale_plan, st_post.cpp post_plan): RGBA32F in, RGBA8 out, RGBA32F between the two steps.
    The keys are substrings of the kernels' names; k_upscale runs with both destinations, so its record is split by the child's order instead."""
    n, m = HD[0] * HD[1], UHD[0] * UHD[1]
    return {"k_upscale (1080p -> 2160p RGBA8)": n * 16 + m * 4, "k_upscale (1080p -> 2160p RGBA32F plane)": n * 16 + m * 16, "k_sharpen (2160p plane -> RGBA8)": m * (16 + 4),
            "k_sharpen (1080p -> RGBA8)": n * (16 + 4), "k_post_resample<2> (1080p -> 2160p RGBA8)": n * 16 + m * 4,
            "k_upscale_sharpen (1080p -> 2160p RGBA8)": n * 16 + m * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upscale.json"))
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--profile-child", action="store_true")
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--abab")
    args = ap.parse_args()
    if args.restatement:
        import upscale_cases as K
        from test_upscale_abi import r2_margin, restatement_vs_definition
        import upscale_ref as U
        worst_r2 = float("%.3e" % r2_margin()[0])
        margin = 4.0 * worst_r2 * U.R2_MIN
        r = restatement_vs_definition(margin)
        r["worst"] = float("%.3e" % r["worst"])
        r.update(tolerance=4.0 * r["worst"], worst_r2_deviation=worst_r2, r2_margin=margin,
                 metric="max |process_f32 - process_f64| per channel, every pixel but those whose float64 r2 lies within r2_margin of 1/32768; "
                        "worst_r2_deviation is relative to max(r2, 1/32768), r2_margin = 4 x that x 1/32768")
        edges = {"%g degrees %s" % (a, n): dict(zip(("upscale_rms", "catmull_rom_rms", "ratio"), (lambda u, c: (round(u, 5), round(c, 5), round(u / c, 3)))(*K.edge_rms(a, q))))
                 for a in K.EDGE_ANGLES + K.EDGE_AXIS_ANGLES for n, q in K.EDGE_RATIOS.items()}
        merge(args.out, {"restatement_vs_definition": r, "slanted_edge_rms_against_coverage": edges})
        return
    import torch  # noqa: F401  (before the library: torch's bundled HIP runtime has to be the first one loaded)
    if args.abab:
        merge(args.out, abab(args.abab, "upscale_off", order=("parent", "this") * 3, order_note="parent this, three times"))
        return
    if args.profile_child:   # the dungeon on the serial schedule, each variant of CHILD in order
        for name in CHILD:
            frames("dungeon", name, frames=CHILD_FRAMES, warmup=CHILD_WARMUP, serial=True)
        return
    if args.kernel_stats:
        from chain_bench import dispatch_record, dispatch_us, kernel_trace
        ceiling = json.load(open(args.out))["copy_ceiling_gb_s"]
        rows, _ = kernel_trace(__file__, ["--profile-child"], "upscale")
        nb, per = launch_bytes(), CHILD_FRAMES + CHILD_WARMUP
        fu = dispatch_us(rows, "k_upscale_sharpen")
        up = dispatch_us([r for r in rows if "k_upscale_sharpen" not in r["Kernel_Name"]], "k_upscale")
        sh, rs = dispatch_us(rows, "k_sharpen"), dispatch_us(rows, "k_post_resample")
        assert len(up) == 2 * per and len(sh) == 2 * per and len(rs) == per and len(fu) == len(FUSED) * per, (len(up), len(sh), len(rs), len(fu))
        out = {}   # the variants ran one after the other: the dispatches in start order, warm-up left out
        for key, us in (("k_upscale (1080p -> 2160p RGBA8)", up[CHILD_WARMUP:per]), ("k_upscale (1080p -> 2160p RGBA32F plane)", up[per + CHILD_WARMUP:]),
                        ("k_sharpen (2160p plane -> RGBA8)", sh[CHILD_WARMUP:per]), ("k_sharpen (1080p -> RGBA8)", sh[per + CHILD_WARMUP:]),
                        ("k_post_resample<2> (1080p -> 2160p RGBA8)", rs[CHILD_WARMUP:])):
            out[key] = dispatch_record(us, nb[key], ceiling)[0]
        for i, name in enumerate(FUSED):
            out["k_upscale_sharpen " + name.rsplit("_", 1)[1]] = dispatch_record(fu[i * per + CHILD_WARMUP:(i + 1) * per], nb["k_upscale_sharpen (1080p -> 2160p RGBA8)"], ceiling)[0]
        two = sorted(a + b for a, b in zip(up[per + CHILD_WARMUP:], sh[CHILD_WARMUP:per]))   # the two launches of one frame, frame by frame
        out["two_launch_upscale_sharpen_frame_sum_us"] = {"median": round(two[len(two) // 2], 2), "min": round(two[0], 2), "max": round(two[-1], 2)}
        best = min(FUSED, key=lambda n: out["k_upscale_sharpen " + n.rsplit("_", 1)[1]]["median_us"])
        best_us, spread = out["k_upscale_sharpen " + best.rsplit("_", 1)[1]]["median_us"], round(two[-1] - two[0], 2)
        out["fused_against_two_launches"] = {"best_tile": best.rsplit("_", 1)[1], "best_us": best_us, "two_launch_us": round(two[len(two) // 2], 2), "two_launch_spread_us": spread,
                                             "frames_launch_the_fused_form": bool(two[len(two) // 2] - best_us > spread)}
        out["two_launch_upscale_sharpen_us"] = round(out["k_upscale (1080p -> 2160p RGBA32F plane)"]["median_us"] + out["k_sharpen (2160p plane -> RGBA8)"]["median_us"], 2)
        merge(args.out, {"kernel_stats_dungeon_1080p_serial_schedule": out})
        return
    from strolle_amd import Engine
    rec = {"render_size": list(HD), "output_size": list(UHD), "mode": "Image{denoise}", "format": "RGBA8_UNORM_SRGB", "display": "ACES_FITTED", "build": "fast",
           "frames": FRAMES, "warmup": WARMUP, "variants": VARIANTS}
    for scene in ("cornell", "dungeon"):
        rec[scene + "_ms_per_frame"] = {}
        for _ in range(2):   # interleaved twice: the spread of one box
            for name, settings in VARIANTS.items():
                rec[scene + "_ms_per_frame"].setdefault(name, []).append(round(frames(scene, name), 4))
    e = Engine(device=0)
    rec["copy_ceiling_gb_s"] = round(float(e.copy_bandwidth()), 1)
    e.close()
    rec["launch_compulsory_bytes"] = launch_bytes()
    merge(args.out, rec)


if __name__ == "__main__":
    main()
