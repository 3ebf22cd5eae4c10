#!/usr/bin/env python3
"""Writes profiles/geometry_extremes.json: per family and size of tests/geometry_extremes.py, the ambiguity threshold and the t tolerance the GPU
tests use, both measured on the CPU against the oracle (the reference side), never against a HIP build.

    python tools/geometry_extremes_profile.py                  measure on the CPU, keep the GPU figures already in the file
    python tools/geometry_extremes_profile.py --gpu DIR        merge the observations tests/test_gpu_geometry_extremes.py left in DIR
                                                               (ST_GEOMETRY_EXTREMES_DUMP=DIR): worst t deviation, stack overflows

threshold    the smallest margin (tests/walk_ref.py) above every ray on which the oracle and the float64 restatement disagree on hit / miss, winning
             slot or occlusion, and never below THRESHOLD_FLOOR: a barycentric coordinate within 16 float32 roundings of an edge is not decided by
             float32 arithmetic, whichever way one scene's rays happened to fall.
t_tolerance  4 x the largest relative deviation of the oracle's t from the float64 t over non-ambiguous common hits (4: at most three contractions of
             the fast build's arithmetic, one rounding each, on top of the oracle's own), and never below 4 float32 roundings."""
import argparse
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import geometry_extremes as gx   # noqa: E402

THRESHOLD_FLOOR = 16 * 2.0 ** -24
TOLERANCE_FLOOR = 4 * 2.0 ** -24


def round_up(x, digits=2):
    """x rounded up to `digits` significant digits (so the committed figure is not a 17-digit float, and never below what was measured)"""
    if x == 0:
        return 0.0
    e = int(np.floor(np.log10(x))) - (digits - 1)
    return float(np.ceil(x / 10.0 ** e) * 10.0 ** e)


def disagreements(case, family):
    """per ray: (the oracle and the restatement decide hit / miss or occlusion differently, they name different triangles)"""
    ref = case["ref"]; hit, t, slot, point, occ = case["oracle"]
    decision = (hit != ref.hit) | (occ != ref.occluded)
    both = hit & ref.hit
    other = np.zeros(len(hit), bool)
    other[both] = ~gx.same_triangle(case["triangles"], slot[both], ref.slot[both])
    return decision, other


def measure(family, n):
    """both scenes the GPU tests trace: as built, and after the refit configuration's move. threshold / t_tolerance: the larger of the two"""
    a, b = measure_scene(family, n, False), measure_scene(family, n, True)
    for k in ("threshold", "t_tolerance"):
        a[k] = max(a[k], b[k])
    for r, moved in ((a, False), (b, True)):       # the shares at the threshold the tests use
        r["ambiguous_share"], r["hit_share"] = (round(x, 5) for x in shares(gx.oracle_case(family, n, moved), family, a["threshold"]))
    a["moved"] = {k: b[k] for k in ("ambiguous_share", "hit_share", "oracle_disagreements", "oracle_worst_t_deviation", "oracle_worst_point_deviation_over_extent", "extent")}
    return a


def shares(case, family, thr):
    """(ambiguous share, share of non-ambiguous hits) of a case's rays at threshold `thr`"""
    ref = case["ref"]
    amb = ref.decision_margin < thr if family in gx.TIED else ref.margin < thr
    return float(amb.mean()), float((ref.hit & ~amb).mean())


def measure_scene(family, n, moved):
    case = gx.oracle_case(family, n, moved)
    ref = case["ref"]; hit, t, slot, point, occ = case["oracle"]
    decision, other = disagreements(case, family)
    worst = max([THRESHOLD_FLOOR] + ref.decision_margin[decision].tolist() + ref.margin[other].tolist())
    thr = round_up(float(np.nextafter(worst, np.inf))) if worst > THRESHOLD_FLOOR else THRESHOLD_FLOOR
    amb = ref.decision_margin < thr if family in gx.TIED else ref.margin < thr
    sure = hit & ref.hit & ~amb
    dev = np.abs(t[sure].astype(np.float64) - ref.t[sure]) / ref.t[sure]
    pdev = np.abs(point[sure].astype(np.float64) - ref.point[sure]).max(axis=1) if sure.any() else np.zeros(0)
    out = dict(triangles=int(len(case["triangles"]) // 36), reaches=gx.FAMILIES[family][1], threshold=thr,
               t_tolerance=round_up(max(TOLERANCE_FLOOR, 4.0 * float(dev.max()) if len(dev) else 0.0)),
               ambiguous_share=round(float(amb.mean()), 5), hit_share=round(float((ref.hit & ~amb).mean()), 5),
               oracle_disagreements=dict(decision=int(decision.sum()), slot=int(other.sum())),
               oracle_worst_t_deviation=float(dev.max()) if len(dev) else 0.0,
               oracle_worst_point_deviation_over_extent=float(pdev.max() / case["extent"]) if len(pdev) else 0.0,
               extent=case["extent"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", help="directory of observations left by the GPU tests")
    ap.add_argument("--out", default=gx.PROFILE)
    args = ap.parse_args()
    old = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = json.load(f)
    cases = {}
    for family, n in gx.CASES:
        key = gx.case_key(family, n)
        cases[key] = measure(family, n)
        if "gpu" in old.get("cases", {}).get(key, {}):
            cases[key]["gpu"] = old["cases"][key]["gpu"]
        print(key, {k: cases[key][k] for k in ("threshold", "t_tolerance", "ambiguous_share", "hit_share", "oracle_disagreements")})
    if args.gpu:
        for path in sorted(glob.glob(os.path.join(args.gpu, "*.json"))):
            with open(path) as f:
                obs = json.load(f)
            cases[obs["case"]].setdefault("gpu", {})[obs["config"]] = obs["observed"]
    doc = {k: v for k, v in old.items() if k != "cases"}
    doc.setdefault("about", "Ray walks and tree builders against a tree-free float64 brute force at geometric extremes (tests/walk_ref.py, "
                            "tests/geometry_extremes.py). threshold / t_tolerance / shares: measured on the CPU against the oracle by "
                            "tools/geometry_extremes_profile.py; gpu: what tests/test_gpu_geometry_extremes.py observed on one MI355X.")
    doc["cases"] = cases
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
