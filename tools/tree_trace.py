"""One fixed sequence of ABI calls through every tree decision of st_tick, for comparing two builds of the library (STROLLE_HIP_LIB picks the
library): the sequence of tests/test_tree_decisions.py — in each refresh mode 0..4 the first tick, a tick without changes, a move, a spawn, a
despawn, a material edit, a mesh re-insert, sixteen moves in a row, a heatmap camera created and deleted, exact arithmetic and back, then a debug
read of every `what` in ascending and in descending order — on the random soup of 700 triangles (above the LDS limit: compact, wide and
device-built streams) and on Cornell (fits LDS). No frame is rendered.

It prints one line per step: the counter and switch seams, and at the read steps a SHA-256 (16 hex digits) of every st_debug_read_scene buffer
that answers; then the same sequence again with every `what` read — and hashed — after every tick. Two libraries agree when the two outputs are
identical text. --device -1 runs the host-only engine (plans none, host_rebuild, host_refit); the default device 0 all six plans.

    python tools/tree_trace.py [--device N] > trace.txt
    rocprofv3 --hip-trace --stats --output-format csv -d DIR -- python tools/tree_trace.py      # then tools/ownership_trace.py --summarize DIR: the per-API call counts"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.device >= 0:
        import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    import test_tree_decisions as T
    from strolle_amd import Engine

    def line(scene, mode, reads, step, status, seams, hashes):
        counters = " ".join(f"{k}={v}" for k, v in seams.items() if k != "mode")
        buffers = "" if hashes is None else " | " + " ".join(f"{what}:{h or '-'}" for what, h in hashes.items())
        print(f"{scene} mode={mode} reads={reads} {step} status={status} {counters}{buffers}", flush=True)

    for scene in T.SCENES:
        for mode in T.MODES:
            for reads in ("end", "every_tick"):
                e = Engine(device=args.device)
                for step, status in T.sequence(e, scene, mode):
                    hashes = T.digest(T.read_all(e)) if reads == "every_tick" else None
                    line(scene, mode, reads, step, status, T.seams(e, mode), hashes)
                for step, order in (("reads_up", T.WHATS), ("reads_down", T.WHATS[::-1])):
                    hashes = T.digest(T.read_all(e, order))
                    line(scene, mode, reads, step, None, T.seams(e, mode), hashes)
                e.close()


if __name__ == "__main__":
    main()
