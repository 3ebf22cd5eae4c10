#!/usr/bin/env python3
"""Regenerates tests/golden/render_launches.json on a machine with the GPU (run from the repo root, after build()):

    python tests/golden/make_render_launches.py [--only CASE [CASE ...]]

For every case of tests/test_gpu_render_graph.py (one factor at a time around the default, on the Cornell scene) and each of frames 1..6
it records what the library that is loaded does: the launch groups st_debug_last_launches lists and st_render_camera's status with every
pass enabled and with pass mask 0, the launches per kernel of a serial profiled frame and, for the output-chain cases, the bytes credited
per kernel. --only records the named cases alone and merges them into the file; every other entry stays as it is, byte for byte. The
test's docstring says which commit wrote which entries; regenerate an entry only with a commit whose pass graph is meant to change, and say so."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (one HIP runtime per process: torch's first)
import test_gpu_render_graph as T  # noqa: E402


def main():
    args = sys.argv[1:]
    only = None
    if "--only" in args:
        only = args[args.index("--only") + 1:]
        args = args[:args.index("--only")]
        unknown = [n for n in only if n not in T.CASES]
        if not only or unknown:
            sys.exit(f"--only takes case names of tests/test_gpu_render_graph.py; unknown: {unknown}")
    out = args[0] if args else T.GOLDEN
    result = {}
    if only is not None:
        with open(T.GOLDEN) as f:
            result = json.load(f)
    for name in (only if only is not None else T.CASES):
        result[name] = T.record(name)
        print(name, "ok", flush=True)
    with open(out, "w") as f:   # one line per case and recording
        f.write("{\n" + ",\n".join(json.dumps(name) + ": {\n" + ",\n".join(f"  {json.dumps(what)}: {json.dumps(rows, separators=(',', ':'))}" for what, rows in rec.items()) + "\n }"
                                     for name, rec in result.items()) + "\n}\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
