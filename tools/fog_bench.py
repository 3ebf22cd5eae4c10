#!/usr/bin/env python3
"""Cost of fog (include/strolle_hip.h "fog"; k_fog.hip) in the default (fast) build. Every run MERGES its figures into --out.

  (default)  (a) ms per frame of Cornell and the dungeon at 1920x1080 Image{denoise} into RGBA8 sRGB with ACES: fog off, on (exponential +
             height + the light lobe), on with ST_FOG_SKY, and on with depth of field, motion blur, bloom and FXAA behind it (FRAMES frames
             after WARMUP, events around the whole run on one stream, interleaved twice);
             (b) the copy ceiling (st_debug_copy_bandwidth) and the launch's compulsory bytes (st_fog.cpp fog_step).
  --restatement         CPU only: the worst deviation of the numpy restatement from the float64 definition over the tests' input matrix
                        (tests/test_fog_abi.py restatement_vs_definition), the figure that test's bound is four times of.
  --kernel-stats        one `rocprofv3 --kernel-trace --stats` child run of its own (no counters), on the serial schedule (a launch's time is
                        its own): the fog launch's time per dispatch against bytes / copy ceiling, and depth of field's all-in-focus copy
                        path (k_dof_gather at f/1000, which moves the same colour bytes) re-measured in the same run.
  --profile-child       what that run wraps.
  --abab PARENT         A B A B of bench.py (the headline and the dungeon at 1080p): PARENT/bench.py (the parent commit, built) against this tree's.

  python tools/fog_bench.py [--out profiles/fog.json] [--restatement | --kernel-stats | --profile-child | --abab DIR]
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # fog_ref.py, fog_cases.py, test_fog_abi.py: the restatement's deviation

from chain_bench import BLOOM, BLUR, DOF, FRAMES, HD, WARMUP, abab, kernel_stats, merge, run_frames  # noqa: E402

FOG = dict(falloff=1, color=(0.55, 0.62, 0.7, 1.0), density=0.06, height_falloff=0.3, height_reference=0.0, light_color=(1.0, 0.8, 0.5), light_exponent=8.0,
           light_direction=(0.3, 0.5, -0.8))
FOG_SKY = dict(FOG, sky_distance=200.0)
SHARP = dict(samples=32, aperture_f_stops=1000.0, autofocus=(0.5, 0.5))   # |coc| < 0.5 everywhere: depth of field's copy path
# name: (fog, depth of field + motion blur + bloom + FXAA under a moving camera)
VARIANTS = {"off": (None, False), "fog": (FOG, False), "fog_sky": (FOG_SKY, False), "fog_dof_motion_blur_bloom_fxaa": (FOG, True)}
CHAIN = dict(set_dof=DOF, set_motion_blur=BLUR, set_bloom=BLOOM, set_post=dict(fxaa=True))


def frames_ms(scene, fog, chain, **kw):
    return run_frames(scene, dict(set_fog=fog, **(CHAIN if chain else {})), moving=chain, **kw)


def launch_bytes(w, h, out_bytes=4):
    return {"k_fog": w * h * (20 + out_bytes), "k_dof_gather": w * h * (24 + out_bytes) + ((w + 31) // 32) * ((h + 31) // 32) * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fog.json"))
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--profile-child", action="store_true")
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--abab")
    args = ap.parse_args()
    if args.restatement:
        import fog_cases
        from test_fog_abi import restatement_vs_definition
        worst, where, pixels = restatement_vs_definition()
        merge(args.out, {"restatement_vs_definition": {"worst": float("%.3e" % worst), "case": where, "pixels": pixels, "cases": len(fog_cases.cases()),
                                                       "metric": "max |fog_f32 - fog_f64| / (max c' + max F), finite-depth pixels"}})
        return
    import torch  # noqa: F401  (before the library: torch's bundled HIP runtime has to be the first one loaded)
    if args.abab:
        merge(args.out, abab(args.abab, "fog_off"))
        return
    if args.profile_child:   # the dungeon on the serial schedule, 30 frames each: fog, then depth of field with everything in focus
        frames_ms("dungeon", FOG_SKY, False, frames=30, warmup=10, serial=True)
        run_frames("dungeon", dict(set_dof=SHARP), frames=30, warmup=10, serial=True)
        return
    if args.kernel_stats:
        ceiling = json.load(open(args.out))["copy_ceiling_gb_s"]
        out = kernel_stats(__file__, ["--profile-child"], launch_bytes(*HD), ceiling, "fog")
        merge(args.out, {"kernel_stats_dungeon_1080p_serial_schedule": out})
        return
    from strolle_amd import Engine
    rec = {"render_size": list(HD), "mode": "Image{denoise}", "format": "RGBA8_UNORM_SRGB", "display": "ACES_FITTED", "build": "fast", "frames": FRAMES, "warmup": WARMUP,
           "fog": {k: list(v) if isinstance(v, tuple) else v for k, v in FOG.items()}, "fog_sky": "the same with ST_FOG_SKY at 200 m",
           "chain": "depth of field (f/0.25, 32 samples, autofocus), motion blur (shutter 0.5, 8 samples) under a moving camera, bloom (0.15, six levels) and FXAA behind the fog"}
    for scene in ("cornell", "dungeon"):
        rec[scene + "_ms_per_frame"] = {}
        for _ in range(2):   # interleaved twice: the spread of one box
            for name, (fog, chain) in VARIANTS.items():
                rec[scene + "_ms_per_frame"].setdefault(name, []).append(round(frames_ms(scene, fog, chain), 4))
    e = Engine(device=0)
    rec["copy_ceiling_gb_s"] = round(float(e.copy_bandwidth()), 1)
    e.close()
    rec["launch_compulsory_bytes"] = launch_bytes(*HD)["k_fog"]
    merge(args.out, rec)


if __name__ == "__main__":
    main()
