#!/usr/bin/env python3
"""profiles/surface_attributes.json and the TOLERANCES table of tests/surface_families.py.

    tools/surface_attributes_profile.py                 measure every case on the CPU oracle (tests/surface_families.py measure): shares under each cap,
                                                        the oracle's worst deviation from the float64 definition per quantity, the fitted texture model
                                                        (a, b) and FACTOR x each as the tolerance; prints the TOLERANCES table to paste
    tools/surface_attributes_profile.py --gpu DIR       merge what tests/test_gpu_surface_attributes.py left in DIR (ST_SURFACE_DUMP=DIR): per case and
                                                        build the worst observed deviation as a fraction of its tolerance
    tools/surface_attributes_profile.py --note KEY FILE merge a JSON file under KEY (the broken-oracle experiments, findings)"""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def _load(path):
    if os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    return {}


def main():
    import surface_families as sf
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu"); ap.add_argument("--note", nargs=2)
    args = ap.parse_args()
    prof = _load(sf.PROFILE)
    if args.gpu:
        runs = prof.setdefault("gpu", {})
        for path in sorted(glob.glob(os.path.join(args.gpu, "*.json"))):
            with open(path) as f:
                d = json.load(f)
            runs.setdefault(d["case"], {})[d["config"]] = d["observed"]
    elif args.note:
        with open(args.note[1]) as f:
            prof[args.note[0]] = json.load(f)
    else:
        prof["factor"] = sf.FACTOR; prof["ambiguous_below_margin"] = sf.AMBIGUOUS; prof["caps"] = sf.CAPS
        prof["units"] = dict(barycentric="absolute", t="relative", point="relative to |origin| + |point|", depth="relative to |origin| + |point|",
                             normal="radians", uv="relative to max(1, |uv|)", motion="pixels", texture_a="relative to the material's factor",
                             texture_b="per unit of slope x delta, delta = 2^-24 (atlas coordinate + |uv| x image size) texels")
        prof["cases"] = {c: sf.measure(c) for c in sf.CASES}
        print("TOLERANCES = {")
        for c in sf.CASES:
            print(f"    {c!r}: {prof['cases'][c]['tolerance']!r},")
        print("}")
    with open(sf.PROFILE, "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True); f.write("\n")


if __name__ == "__main__":
    main()
