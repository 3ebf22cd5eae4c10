#!/usr/bin/env python3
"""Cost of the lens effects (include/strolle_hip.h "lens effects"; k_lens.hip) in the default (fast) build. Every run MERGES its figures
into --out.

  (default)  (a) ms per frame of Cornell and the dungeon at 1920x1080 Image{denoise} into RGBA8 sRGB with ACES: the node off, vignette +
             grain only (the pointwise instantiation), distortion, distortion + a 3-tap fringe, distortion + a 16-tap fringe, and the whole
             chain (fog, depth of field, motion blur, bloom, the lens, FXAA under a moving camera) — FRAMES frames after WARMUP, events
             around the whole run on one stream, interleaved twice;
             (b) the copy ceiling (st_debug_copy_bandwidth) and the launch's compulsory bytes (st_lens.cpp lens_step).
  --restatement         CPU only: the two constants of the tolerance between the numpy restatement and the float64 definition over the
                        tests' input matrix (tests/test_lens_abi.py restatement_vs_definition): a, the worst relative deviation where no
                        tap's texels differ, and b, the worst excess over a per unit of tap spread. The tests' bound is four times each.
  --resources           CPU only: hipcc's kernel-resource-usage remarks for k_lens.hip in both builds (VGPRs, spills, scratch, occupancy).
  --kernel-stats        one `rocprofv3 --kernel-trace --stats` child run of its own (no counters), on the serial schedule (a launch's time is
                        its own): the lens launch per dispatch against bytes / copy ceiling for each variant, its time per tap, the
                        pointwise instantiation against the fog launch — the yardstick: it moves the same bytes — and the gather against
                        the motion-blur gather's time per tap, both re-measured in the same run.
  --profile-child       what that run wraps.
  --abab PARENT         A B A B A B of bench.py (the headline and the dungeon at 1080p): PARENT/bench.py (the parent commit, built) against this tree's.

  python tools/lens_bench.py [--out profiles/lens.json] [--restatement | --resources | --kernel-stats | --profile-child | --abab DIR]
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # lens_ref.py, lens_cases.py, test_lens_abi.py: the restatement's deviation

from chain_bench import BLOOM, BLUR, DOF, FOG, FRAMES, HD, WARMUP, abab, dispatch_record, dispatch_us, kernel_trace, merge, run_frames  # noqa: E402

POINTWISE = dict(vignette_intensity=0.5, vignette_falloff=1.5, grain_intensity=0.1, grain_size=2, grain_seed=1, grain_animate=True)
BARREL = dict(k1=-0.15, k2=0.02, fit=True)
# name: (the lens keywords or None, the rest of the chain under a moving camera)
VARIANTS = {"off": (None, False), "vignette_grain": (POINTWISE, False), "distortion": (BARREL, False), "distortion_fringe3": (dict(BARREL, fringe=0.02, fringe_taps=3), False),
            "distortion_fringe16": (dict(BARREL, fringe=0.02, fringe_taps=16), False),
            "fog_dof_motion_blur_bloom_lens_fxaa": (dict(BARREL, fringe=0.02, fringe_taps=3, **POINTWISE), True)}
# the child run's sequence: (name, lens keywords, taps); then fog alone and motion blur alone
CHILD = [("vignette_grain", POINTWISE, 0), ("distortion", BARREL, 1), ("distortion_fringe3", dict(BARREL, fringe=0.02, fringe_taps=3), 3),
         ("distortion_fringe16", dict(BARREL, fringe=0.02, fringe_taps=16), 16)]
CHILD_FRAMES, CHILD_WARMUP = 30, 10


def settings(lens, chain):
    s = dict(set_fog=FOG, set_dof=DOF, set_motion_blur=BLUR, set_bloom=BLOOM) if chain else {}
    s["set_lens"] = lens
    if chain:
        s["set_post"] = dict(fxaa=True)
    return s


def launch_bytes(w, h, out_bytes=4):
    return {"k_lens": w * h * (16 + out_bytes), "k_fog": w * h * (20 + out_bytes)}


def resources():
    """hipcc's kernel-resource-usage remarks for k_lens.hip, per build and instantiation"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "strolle_amd", "csrc")
    builds = {"exact": ["-ffp-contract=off", "-DST_KNS=exact"], "fast": ["-ffp-contract=fast-honor-pragmas", "-DST_KNS=fast", "-DST_FAST_MATH=1"]}
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "Occupancy [waves/SIMD]": "occupancy_waves_per_simd",
            "SGPRs Spill": "sgpr_spills", "VGPRs Spill": "vgpr_spills", "LDS Size [bytes/block]": "lds_bytes_per_block"}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for build, flags in builds.items():
            r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-fno-slp-vectorize"] + flags +
                               ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "k_lens.hip"), "-o", os.path.join(tmp, "k_lens.o")],
                               cwd=csrc, capture_output=True, text=True, check=True)
            name = None
            for line in r.stderr.splitlines():
                m = re.search(r"remark: (?:.*?:\d+:\d+: )?\s*(.+?): (\S+) \[-Rpass-analysis", line)
                if not m:
                    continue
                if m.group(1) == "Function Name":
                    name = "%s %s" % (build, "gather" if "ILb1E" in m.group(2) else "pointwise")
                    out[name] = {}
                elif name and m.group(1) in keys:
                    out[name][keys[m.group(1)]] = int(m.group(2))
    for rec in out.values():
        assert rec["vgpr_spills"] == 0 and rec["sgpr_spills"] == 0 and rec["scratch_bytes_per_lane"] == 0, out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens.json"))
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--profile-child", action="store_true")
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--abab")
    args = ap.parse_args()
    if args.restatement:
        import lens_cases
        from test_lens_abi import restatement_vs_definition
        a, b, where_a, where_b, pixels = restatement_vs_definition()
        merge(args.out, {"restatement_vs_definition": {
            "a": float("%.3e" % a), "b": float("%.3e" % b), "case_a": where_a, "case_b": where_b, "pixels": pixels, "cases": len(lens_cases.cases()),
            "metric": "per pixel and channel, in front of the display transform, unspoiled inputs, every pixel: rel = |lens_f32 - lens_f64| / max(1, |lens_f64|) and "
                      "spread = lens_f64's tap spread / max(1, |lens_f64|); a = max rel where spread == 0; b = max (rel - a) / spread where spread > 0; "
                      "the tests hold rel <= 4 a + 4 b spread"}})
        return
    if args.resources:
        merge(args.out, {"hipcc_resource_usage_k_lens": resources()})
        return
    import torch  # noqa: F401  (before the library: torch's bundled HIP runtime has to be the first one loaded)
    if args.abab:
        merge(args.out, abab(args.abab, "lens_off", order=("parent", "this") * 3, order_note="parent this, three times"))   # three rounds: two leave the spread to one pair
        return
    if args.profile_child:   # the dungeon on the serial schedule: each lens variant in CHILD's order, then fog alone, then motion blur alone (a moving camera)
        for _name, lens, _taps in CHILD:
            run_frames("dungeon", settings(lens, False), frames=CHILD_FRAMES, warmup=CHILD_WARMUP, serial=True)
        run_frames("dungeon", dict(set_fog=FOG), frames=CHILD_FRAMES, warmup=CHILD_WARMUP, serial=True)
        run_frames("dungeon", dict(set_motion_blur=BLUR), moving=True, frames=CHILD_FRAMES, warmup=CHILD_WARMUP, serial=True)
        return
    if args.kernel_stats:
        ceiling = json.load(open(args.out))["copy_ceiling_gb_s"]
        rows, _ = kernel_trace(__file__, ["--profile-child"], "lens")
        nbytes = launch_bytes(*HD)
        lens_us, per = dispatch_us(rows, "k_lens"), CHILD_FRAMES + CHILD_WARMUP
        assert len(lens_us) == per * len(CHILD), (len(lens_us), per, len(CHILD))
        out, med = {}, {}
        for i, (name, _lens, _taps) in enumerate(CHILD):   # the variants ran one after the other: the dispatches in start order, warm-up left out
            out["k_lens " + name], med[name] = dispatch_record(lens_us[i * per + CHILD_WARMUP:(i + 1) * per], nbytes["k_lens"], ceiling)
        out["k_fog"], fog = dispatch_record(dispatch_us(rows, "k_fog")[CHILD_WARMUP:], nbytes["k_fog"], ceiling)
        blur_us = dispatch_us(rows, "k_mblur_gather")[CHILD_WARMUP:]
        out["pointwise_over_fog"] = round(med["vignette_grain"] / fog, 3)
        out["us_per_tap"] = {name: round(med[name] / taps, 2) for name, _lens, taps in CHILD if taps}
        out["us_per_extra_tap_3_to_16"] = round((med["distortion_fringe16"] - med["distortion_fringe3"]) / 13.0, 2)
        if blur_us:
            out["k_mblur_gather"], blur = dispatch_record(blur_us)
            out["motion_blur_us_per_tap"] = {"samples": BLUR["samples"], "us_per_tap": round(blur / BLUR["samples"], 2),
                                             "note": "one point-sampled 16-B texel and one 8-B (r, Z) read per tap, on the tiles that move only; a lens tap is four 16-B texels on every pixel"}
        merge(args.out, {"kernel_stats_dungeon_1080p_serial_schedule": out})
        return
    from strolle_amd import Engine
    rec = {"render_size": list(HD), "mode": "Image{denoise}", "format": "RGBA8_UNORM_SRGB", "display": "ACES_FITTED", "build": "fast", "frames": FRAMES, "warmup": WARMUP,
           "variants": {k: v[0] for k, v in VARIANTS.items()},
           "chain": "fog, depth of field (f/0.25, 32 samples, autofocus), motion blur (shutter 0.5, 8 samples) under a moving camera, bloom (0.15, six levels), the lens and FXAA"}
    for scene in ("cornell", "dungeon"):
        rec[scene + "_ms_per_frame"] = {}
        for _ in range(2):   # interleaved twice: the spread of one box
            for name, (lens, chain) in VARIANTS.items():
                rec[scene + "_ms_per_frame"].setdefault(name, []).append(round(run_frames(scene, settings(lens, chain), moving=chain), 4))
    e = Engine(device=0)
    rec["copy_ceiling_gb_s"] = round(float(e.copy_bandwidth()), 1)
    e.close()
    rec["launch_compulsory_bytes"] = launch_bytes(*HD)["k_lens"]
    merge(args.out, rec)


if __name__ == "__main__":
    main()
