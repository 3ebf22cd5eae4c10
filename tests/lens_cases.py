"""The input matrix of the lens-effects tests (tests/test_gpu_lens.py on the GPU; tests/test_lens_abi.py holds the restatement to the
float64 definition over the same matrix): images and descriptors.

Sizes: the workgroup is 32 x 8 pixels and a wave 32 x 2, so 72 x 52 (partial groups both ways), widths 63, 64, 65 and 129 astride the
wave's and the workgroup's edges, 5 x 5 (smaller than any tile) and 1 x 1 (u = v = 0: no radius at all)."""
import itertools
import json
import os

import numpy as np

from output_chain import _image
from strolle_amd import Tonemap, lens_desc

SIZE = (72, 52)
SIZES = [(72, 52), (63, 10), (64, 9), (65, 17), (129, 5), (5, 5), (1, 1)]
EV = 0.5   # the manual exposure of every case with a display

STEPS = {
    "distortion": dict(k1=-0.2, k2=0.03),
    "fringe": dict(fringe=0.03, fringe_taps=3),
    "vignette": dict(vignette_intensity=0.6, vignette_falloff=1.5),
    "grain": dict(grain_intensity=0.25, grain_size=2, grain_seed=12345),
}
ALL = {k: v for s in STEPS.values() for k, v in s.items()}
COEFFICIENTS = {"barrel": dict(k1=-0.2, k2=0.03), "pincushion": dict(k1=0.15, k2=0.05), "mixed": dict(k1=-0.25, k2=0.03), "mixed2": dict(k1=0.2, k2=-0.06)}
KINDS = ("noise", "edge", "checker", "ramp")


def image(size, spoil, kind="noise", seed=11):
    """(h, w, 4) float32: HDR noise with fireflies, a slanted edge (0 against 8), a one-pixel checker (0.1 against 5) or a ramp over both
    axes; `spoil` adds negatives, NaN, infinities, zeros of both signs and values beyond 65504"""
    w, h = size
    if kind == "noise":
        return _image(w, h, seed=seed + w, spoil=spoil)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    if kind == "edge":
        v = np.where(y - 0.5 * h > 0.37 * (x - 0.5 * w), 8.0, 0.0)
        rgb = np.stack([v, v, v], -1)
    elif kind == "checker":
        v = np.where((x + y) % 2 == 0, 5.0, 0.1)
        rgb = np.stack([v, 0.5 * v, 2.0 * v], -1)
    else:
        rgb = np.stack([x / max(w - 1, 1) * 4.0, y / max(h - 1, 1) * 2.0, (x + y) / max(w + h - 2, 1) * 100.0], -1)
    img = np.concatenate([rgb, np.full((h, w, 1), 0.5)], -1).astype(np.float32)
    if spoil:
        rng = np.random.default_rng(seed + w + 7 * h)
        n = max(1, w * h // 150)
        for bad in (np.nan, np.inf, -np.inf, -3.0, -0.0, 1e30, 70000.0):
            img[rng.integers(0, h, n), rng.integers(0, w, n), rng.integers(0, 3, n)] = bad
    return img


def cases():
    """(name, size, image kind, keyword arguments of lens_desc, the display's operator or None)"""
    out = []
    aces = Tonemap.ACES_FITTED
    for name, kw in STEPS.items():                                         # each step alone
        out.append((name, SIZE, "noise", dict(kw), aces))
    for a, b in itertools.combinations(STEPS, 2):                          # pairwise
        out.append((f"{a}+{b}", SIZE, "noise", dict(STEPS[a], **STEPS[b]), aces))
    for k, size in enumerate(SIZES):                                       # everything, every size, the image kinds in turn
        out.append((f"all-{size[0]}x{size[1]}", size, KINDS[k % 4], dict(ALL, fit=(k % 2 == 0), vignette_round=(k % 2 == 1)), aces))
    sizes = itertools.cycle([(63, 10), (64, 9), (65, 17), (129, 5)])
    for (cname, co), scale, fit in itertools.product(COEFFICIENTS.items(), (0.5, 1.0, 2.0), (False, True)):   # coefficients x scale x fit
        if cname == "mixed2" and scale != 1.0:
            continue
        out.append((f"{cname}-scale{scale}-{'fit' if fit else 'nofit'}", next(sizes), "noise", dict(co, scale=scale, fit=fit), None))
    out.append(("scale-only-2", (65, 17), "ramp", dict(scale=2.0), None))
    out.append(("fit-only", (64, 9), "noise", dict(fit=True), None))                                # the identity under the fit: W / (W - 1), the border pixels' centres go to the frame's edge
    for taps, kind in zip((3, 4, 7, 16), KINDS[1:] + KINDS[:1]):                                   # tap counts, with and without distortion
        out.append((f"fringe-{taps}-taps", (65, 17), kind, dict(fringe=0.05, fringe_taps=taps), aces))
        out.append((f"fringe-{taps}-taps-barrel-fit", (129, 5), kind, dict(COEFFICIENTS["barrel"], fringe=0.1, fringe_taps=taps, fit=True), Tonemap.NONE))
    for rnd in (False, True):                                                                       # both vignette shapes
        out.append((f"vignette-{'round' if rnd else 'ellipse'}", (129, 5), "ramp", dict(vignette_intensity=1.0, vignette_falloff=3.0, vignette_round=rnd), None))
    for gs in (1, 3, 8):                                                                            # grain sizes
        out.append((f"grain-size-{gs}", (65, 17), "ramp", dict(grain_intensity=0.9, grain_size=gs, grain_seed=0xfffffff0 + gs), Tonemap.REINHARD))
    for kind in KINDS:                                                                              # every input, everything on
        out.append((f"all-{kind}", (63, 10), kind, dict(ALL, fringe_taps=4), aces))
    out.append(("neutral", (33, 9), "noise", dict(), aces))
    return out


def tolerance():
    """(a, b) of the bound rel <= a + b spread between a float32 result and the float64 definition: four times the restatement's own two
    constants, measured on the CPU and recorded in profiles/lens.json (tools/lens_bench.py --restatement)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rec = json.load(open(os.path.join(root, "profiles", "lens.json")))["restatement_vs_definition"]
    return 4.0 * rec["a"], 4.0 * rec["b"]


def build(kw):
    return lens_desc(**kw)
