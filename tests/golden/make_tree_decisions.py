#!/usr/bin/env python3
"""Regenerates one half of tests/golden/tree_decisions.json with the library that is loaded (run from the repo root, after build(); STROLLE_HIP_LIB
picks another build of the library):

    python tests/golden/make_tree_decisions.py host      # a host-only engine: any machine
    python tests/golden/make_tree_decisions.py device    # on a machine with the GPU

For each scene and refresh mode of tests/test_tree_decisions.py it records the counter and switch seams after every step of the test's sequence.
The other half stays as it is, byte for byte. The test's docstring says which commit wrote the file; regenerate it only with a commit whose tree
decisions are meant to change, and say so."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    half = sys.argv[1] if len(sys.argv) > 1 else ""
    if half not in ("host", "device"):
        sys.exit("usage: make_tree_decisions.py host|device [OUT]")
    if half == "device":
        import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    import test_tree_decisions as T
    out = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN
    result = {"host": {}, "device": {}}
    if os.path.exists(T.GOLDEN):
        with open(T.GOLDEN) as f:
            result.update(json.load(f))
    result[half] = {f"{scene}_{mode}": T.record(scene, mode, -1 if half == "host" else 0)[0] for scene in T.SCENES for mode in T.MODES}
    with open(out, "w") as f:   # one line per step
        f.write("{\n" + ",\n".join(json.dumps(h) + ": {\n" + ",\n".join(f" {json.dumps(case)}: [\n" + ",\n".join("  " + json.dumps(row, separators=(",", ":")) for row in rows) + "\n ]"
                                                                       for case, rows in result[h].items()) + "\n}" for h in ("host", "device")) + "\n}\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
