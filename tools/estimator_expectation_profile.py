#!/usr/bin/env python3
"""CPU: the oracle's long-run means against the closed form of tests/light_ref.py.

    python tools/estimator_expectation_profile.py [--jobs N] [--only case:mode ...]

Per (case, mode) of tests/light_cases.py: 16 oracle seeds x (64 warm-up + 1,000 averaged) frames, per-pixel means in float64; the frame sum and every
8x8-block sum per channel over the non-ambiguous pixels. Two files come out:

    tests/golden/estimator_expectation.npz   per row and statistic: the oracle's sum over the 16 seeds, over the first 8 alone (what the exact build
                                             has to reproduce bit for bit) and the per-seed standard deviation sigma_seed of the deviation
    profiles/estimator_expectation.json      what a reader wants: the allowance b and where it came from, each case's shares, per row the frame
                                             sums' deviation and standard error and the blocks' range

A deviation is (sum - definition) / definition (light_cases.denominators); the definition is recomputed wherever it is needed, never stored.
--gpu FILE, --mutations FILE and --parent TEXT write sections measured elsewhere into the JSON; a re-measurement carries them over.
"""
import argparse
import json
import multiprocessing
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")          # 48x32 frames: one thread per engine, engines side by side
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import light_cases as lc  # noqa: E402

B_FLOOR = 0.002
ONE_LINE = ("rows", "tests", "caught_by")          # lists under these keys are written one compact entry per line


def dump(doc, path):
    """indented JSON; the long tables one entry per line"""
    def enc(v, depth, key=None):
        pad = " " * depth
        if isinstance(v, dict):
            return "{\n" + ",\n".join(f"{pad} {json.dumps(k)}: {enc(x, depth + 1, k)}" for k, x in v.items()) + f"\n{pad}}}"
        if isinstance(v, list) and key in ONE_LINE:
            return "[\n" + ",\n".join(f"{pad} {json.dumps(x)}" for x in v) + f"\n{pad}]"
        if isinstance(v, list) and v and isinstance(v[0], dict):
            return "[\n" + ",\n".join(f"{pad} {enc(x, depth + 1)}" for x in v) + f"\n{pad}]"
        return json.dumps(v)
    with open(path, "w") as f:
        f.write(enc(doc, 0) + "\n")


def _one(job):
    case, mode, seed = job
    return job, lc.oracle_mean(lc.ALL_CASES[case], mode, seed)


def measure(case: str, mode: str, means: dict):
    """(sum over 16 seeds, sum over the first 8, sigma_seed) of one row from its 16 per-seed means"""
    exp = lc.expectation(case, lc.DEFINED_BY.get(mode, mode))
    per_seed = np.array([lc.deviations(means[s], exp)[0] for s in lc.SEEDS16])
    return (lc.deviations(lc.pooled([means[s] for s in lc.SEEDS16]), exp)[1], lc.deviations(lc.pooled([means[s] for s in lc.SEEDS8]), exp)[1],
            per_seed.std(axis=0, ddof=1))


def summary(case: str, mode: str, rec, b: float):
    dev, sigma = lc.recorded_deviation(case, mode, rec), rec["sigma_seed"]
    with np.errstate(all="ignore"):
        z = np.where(sigma > 0, np.abs(dev) / (sigma / 4.0), 0.0)
    r4 = lambda a: [round(float(x), 5) for x in a]
    return {"case": case, "mode": mode, "frame_deviation": r4(dev[:3]), "frame_standard_error": r4(sigma[:3] / 4.0),
            "block_deviation_range": r4([dev[3:].min(), dev[3:].max()]), "block_max_z": round(float(z[3:].max()), 1),
            "worst_excess_over_4se_plus_b": round(float(np.max(np.abs(dev) - (sigma + b))), 5)}


def allowance(recs):
    """b: twice the largest |r_o - 1| over the frame sums of the diffuse, Reference and Image rows that lie beyond 3 standard errors; 0.002 if none does"""
    worst, where = 0.0, None
    for (case, mode), rec in recs.items():
        if mode not in ("DI_DIFFUSE", "REFERENCE", "IMAGE"):
            continue
        dev = lc.recorded_deviation(case, mode, rec)
        for k in range(3):
            d, se = abs(dev[k]), rec["sigma_seed"][k] / 4.0
            if d > 3.0 * se and d > worst:
                worst, where = float(d), f"{case} {mode} frame {'RGB'[k]}"
    return (2.0 * worst, where) if where else (B_FLOOR, None)


def merge(args):
    """--gpu / --mutations / --parent: sections measured elsewhere, written into the existing JSON"""
    doc = json.load(open(lc.PROFILE))
    if args.gpu:
        rows = [json.loads(line) for line in open(args.gpu) if line.strip()]
        fast = [r for r in rows if r["test"] != "exact"]
        short = lambda r: ({"test": r["test"], "case": r["case"], "mode": r["mode"], "seconds": r["seconds"]} |
                           ({"differing": r["differing"]} if r["test"] == "exact" else
                            {"worst": r["worst"], "in_tolerances": round(r["worst_in_tolerances"], 3), "spread_in_bounds": round(r["worst_spread_in_bounds"], 3)}))
        doc["gpu"] = {"what": "tests/test_gpu_estimator_expectation.py on one MI355X (ST_ESTIMATOR_REPORT): per test the worst statistic in units of its "
                              "tolerance (1 = the bound), the widest per-seed spread in units of 2 sigma_seed, and the test's seconds",
                      "worst_in_tolerances": round(max(r["worst_in_tolerances"] for r in fast), 3),
                      "worst_spread_in_bounds": round(max(r["worst_spread_in_bounds"] for r in fast), 3),
                      "exact_sums_differing": sum(r["differing"] for r in rows if r["test"] == "exact"),
                      "seconds_total": round(sum(r["seconds"] for r in rows), 1), "seconds_slowest": max(r["seconds"] for r in rows), "tests": [short(r) for r in rows]}
    if args.mutations:
        doc["mutations"] = json.load(open(args.mutations))
    if args.parent:
        doc["failed_at_the_parent_commit"] = args.parent
    dump(doc, lc.PROFILE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--only", nargs="*", default=None, help="case:mode rows to re-measure; the others are kept from the existing files")
    ap.add_argument("--gpu", help="the ST_ESTIMATOR_REPORT file of a GPU run: becomes the section \"gpu\"; nothing is re-measured")
    ap.add_argument("--mutations", help="a JSON file with the table of deliberately broken oracles: becomes the section \"mutations\"")
    ap.add_argument("--parent", help="what failed at the parent commit, in words")
    args = ap.parse_args()
    if args.gpu or args.mutations or args.parent:
        return merge(args)
    old = json.load(open(lc.PROFILE)) if os.path.exists(lc.PROFILE) else {}
    pairs = [(c, m) for c, m in lc.MATRIX if args.only is None or f"{c}:{m}" in args.only]
    t0 = time.time()
    means = {}
    with multiprocessing.get_context("fork").Pool(args.jobs) as pool:
        for (c, m, s), mean in pool.imap_unordered(_one, [(c, m, s) for c, m in pairs for s in lc.SEEDS16]):
            means.setdefault((c, m), {})[s] = mean
    recs = {}
    for c, m in lc.MATRIX:
        recs[(c, m)] = dict(zip(("sum_16", "sum_8", "sigma_seed"), measure(c, m, means[(c, m)]))) if (c, m) in means else lc.recorded(c, m)
    np.savez_compressed(lc.RECORDED, **{f"{c}:{m}:{k}": v for (c, m), rec in recs.items() for k, v in rec.items()})
    b, b_from = allowance(recs)
    doc = {"what": "tests/light_cases.py on the CPU oracle against tests/light_ref.py: per (case, mode) 16 seeds x (64 warm-up + 1,000 averaged) frames; "
                   "statistics are the frame sum and the 8x8-block sums per channel over the non-ambiguous pixels, as deviations from the definition "
                   "(ratio - 1; absolute in units of an average block where the definition is 0). The per-statistic sums and sigma_seed are in "
                   "tests/golden/estimator_expectation.npz",
           "warmup": lc.WARMUP, "frames": lc.FRAMES, "seeds_16": list(lc.SEEDS16), "seeds_8": list(lc.SEEDS8),
           "b": b, "b_from": b_from or "no frame sum of a diffuse, Reference or Image row lies beyond 3 standard errors: the floor of 0.002",
           "oracle_held": old.get("oracle_held", {}),
           "specular_blocks": "DI_SPECULAR block sums are held to the definition like every other statistic: with the representative point, the intensity "
                              "and the quantised G-buffer material of tests/light_ref.py the oracle's blocks stay within 4 standard errors + b of the "
                              "closed form (test_light_ref.py test_profile_invariants), so no row is listed under oracle_held",
           "shares": {c: lc.shares(lc.expectation(c, "DI_DIFFUSE")) for c in lc.ALL_CASES},
           "rows": [summary(c, m, rec, b) for (c, m), rec in recs.items()], "cpu_seconds": round(time.time() - t0, 1)}
    for key in ("mutations", "gpu", "failed_at_the_parent_commit"):
        if key in old:
            doc[key] = old[key]
    dump(doc, lc.PROFILE)
    print(f"b = {b:.5f} ({b_from}); {len(recs)} rows in {time.time() - t0:.0f} s -> {lc.PROFILE}, {lc.RECORDED}")
    for r in doc["rows"]:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
