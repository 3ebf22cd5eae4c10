#!/usr/bin/env python3
"""Reduces what tools/gpu_side_schedule.sh left under its OUT_ROOT to profiles/side_schedule.json: per start point (StTuning::side_start) the
timeline shares and the mean duration of every kernel in the traced frames, this library's headline per start point, and the parent / head
bench calls with the issue's criteria (noise of a call = the spread of its two same-library results; the headline has to gain more than
three times that, nothing else may lose more than it). Runs anywhere.
  python tools/side_schedule_report.py OUT_ROOT [--notes notes.json] > profiles/side_schedule.json"""
import argparse, glob, json, os, re

METRICS = ("ms_per_step", "ms_per_step_moving", "ms_per_step_geometry_moving", "ms_per_step_with_present")


def last_line(path):
    return json.loads(open(path).read().strip().splitlines()[-1])


def timeline(path):
    durations, frames = {}, 0
    shares, per_frame, kernel_sum = {}, None, None
    for line in open(path):
        m = re.match(r"q\d+\s+[\d.]+ us\s+\+\s*([\d.]+)\s+(.*?)\s*\|", line)
        if m:
            name = re.sub(r"<.*", "", m.group(2))
            name = m.group(2).strip() if name in ("denoise_wavelet_far", "denoise_wavelet_lds") else name   # stride 8 / stride 16 + composition differ by their arguments
            durations.setdefault(name, []).append(float(m.group(1)))
            frames += name == "prim_visibility"
        m = re.match(r"(\d+) frames, ([\d.]+) us per frame by the trace; sum of kernel durations ([\d.]+)", line)
        if m:
            per_frame, kernel_sum = float(m.group(2)), float(m.group(3))
        m = re.match(r"\s+(\d) kernel\(s\) in flight:\s+([\d.]+) %", line)
        if m:
            shares[{"0": "idle", "1": "one_kernel", "2": "two_kernels", "3": "three_kernels"}[m.group(1)]] = float(m.group(2))
    return {"frames": frames, "us_per_frame_by_the_trace": per_frame, "sum_of_kernel_durations_us_per_frame": kernel_sum, "share_percent": shares,
            "mean_us_per_launch": {k: round(sum(v) / len(v), 1) for k, v in sorted(durations.items())}}


def ab_call(d):
    res = {}
    for scene in ("cornell", "dungeon"):
        runs = {lib: [last_line(p) for p in sorted(glob.glob(os.path.join(d, f"{scene}_{lib}_r*.json")))] for lib in ("parent", "head")}
        if not runs["parent"]:
            continue
        res[scene] = {}
        for m in METRICS:
            if m not in runs["parent"][0]:
                continue
            p, h = [r[m] for r in runs["parent"]], [r[m] for r in runs["head"]]
            spread = round(max(max(p) - min(p), max(h) - min(h)), 4)
            diff = round(sum(h) / len(h) - sum(p) / len(p), 5)
            row = {"parent": p, "head": h, "parent_mean": round(sum(p) / len(p), 5), "head_mean": round(sum(h) / len(h), 5), "spread": spread, "head_minus_parent": diff}
            if m == "ms_per_step" and scene == "cornell":
                row["gain_exceeds_three_spreads"] = -diff > 3 * spread
            else:
                row["not_above_parent_by_more_than_spread"] = diff <= spread
            res[scene][m] = row
        # a figure the schedule cannot move: the kernels' durations summed over a SERIAL (profiled) frame — it tells which state a process's kernels ran in
        res[scene]["serial_kernel_sum_ms"] = {lib: [r.get("gpu_kernel_ms_per_frame") for r in runs[lib]] for lib in runs}
        res[scene]["build_stamp"] = {lib: sorted({str(r.get("build_stamp")) for r in runs[lib]}) for lib in runs}
    return res


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("out_root", help="the OUT_ROOT tools/gpu_side_schedule.sh wrote to"); ap.add_argument("--notes", default=None)
    a = ap.parse_args()
    OUT = os.path.abspath(a.out_root)
    rep = {"timelines": {}, "headline_per_start_point": {}, "parent_head_calls": {}, "control": {}}
    for p in sorted(glob.glob(os.path.join(OUT, "side_timeline", "*", "timeline.txt"))):
        scene, v = os.path.basename(os.path.dirname(p)).rsplit("_", 1)
        rep["timelines"].setdefault(scene, {})[f"side_start_{v}"] = timeline(p)
    for p in sorted(glob.glob(os.path.join(OUT, "side_choose", "*.json"))):
        scene, v, _ = os.path.basename(p)[:-5].split("_")
        rep["headline_per_start_point"].setdefault(scene, {}).setdefault(f"side_start_{v}", []).append(last_line(p)["ms_per_step"])
    for d in sorted(glob.glob(os.path.join(OUT, "side_ab_*"))):
        rep["parent_head_calls"][os.path.basename(d)[len("side_ab_"):]] = ab_call(d)
    for p in sorted(glob.glob(os.path.join(OUT, "side_control", "*.json"))):
        lib = os.path.basename(p).split("_")[1]
        r = last_line(p)
        for m in METRICS + ("gpu_kernel_ms_per_frame",):
            rep["control"].setdefault(lib, {}).setdefault(m, []).append(r.get(m))
    if a.notes:
        rep = {**json.load(open(a.notes)), **rep}
    print(json.dumps(rep, indent=1))


if __name__ == "__main__":
    main()
