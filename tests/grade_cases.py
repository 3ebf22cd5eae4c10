"""The input matrix of the colour-grading tests (tests/test_gpu_color_grading.py on the GPU; tests/test_color_grading_abi.py holds the
restatement to the float64 definition over the same matrix): images, look-up tables, descriptors.

Sizes: the workgroup is 32 x 8 pixels, so 72 x 52 (partial groups both ways), 33 x 9 (a second group one pixel wide and one row high),
5 x 5 and 1 x 1. LUT sides 2 (one cell: every pixel in it, every high corner the table's last texel), 3, 17 and 33."""
import itertools

import numpy as np

from output_chain import _image
from strolle_amd import LutDomain, Tonemap, color_grading_desc

SIZE = (72, 52)
SIZES = [(72, 52), (33, 9), (5, 5), (1, 1)]
LUT_SIDES = (2, 3, 17, 33)

STEPS = {
    "wb": dict(temperature=0.35, tint=-0.2),
    "contrast": dict(contrast=1.3),
    "sat": dict(saturation=0.6),
    "cdl": dict(slope=(1.1, 0.9, 1.2), offset=(0.02, -0.03, 0.0), power=(1.2, 1.0, 0.8), cdl_saturation=1.25),
    "lut": dict(lut=("random", 17)),
    "dither": dict(dither=True),
}
ALL = {k: v for s in STEPS.values() for k, v in s.items()}
EV = 0.5   # the manual exposure of every case with a display


def lut(kind, n, seed=5):
    """(n, n, n, 3) float32 indexed [b, g, r]: the identity, a constant, or random values that leave [0, 1] on both sides"""
    if kind == "identity":
        g = np.arange(n, dtype=np.float64) / (n - 1)
        b, gg, r = np.meshgrid(g, g, g, indexing="ij")
        return np.stack([r, gg, b], -1).astype(np.float32)
    if kind == "constant":
        return np.broadcast_to(np.array([0.25, 0.5, 0.75], np.float32), (n, n, n, 3)).copy()
    rng = np.random.default_rng(seed + n)
    return (rng.random((n, n, n, 3)) * 1.2 - 0.1).astype(np.float32)


def image(size, spoil, seed=11):
    return _image(size[0], size[1], seed=seed + size[0], spoil=spoil)


def cases():
    """(name, size, keyword arguments of color_grading_desc with `lut` a (kind, side) pair or absent, the display's operator or None)"""
    out = []
    aces = Tonemap.ACES_FITTED
    for name, kw in STEPS.items():                                         # each step alone
        out.append((name, SIZE, dict(kw), aces))
    for a, b in itertools.combinations(STEPS, 2):                          # pairwise
        out.append((f"{a}+{b}", SIZE, dict(STEPS[a], **STEPS[b]), aces))
    for size in SIZES:                                                     # everything, every size
        out.append((f"all-{size[0]}x{size[1]}", size, dict(ALL), aces))
    for op in (None, Tonemap.NONE, Tonemap.REINHARD, Tonemap.REINHARD_LUMINANCE, Tonemap.PBR_NEUTRAL):   # every operator, and no display
        out.append((f"all-op-{'off' if op is None else op.name}", (33, 9), dict(ALL), op))
    for n in LUT_SIDES:                                                    # both domains, every side, random and identity tables
        out.append((f"lut-unit-random-{n}", (33, 9), dict(lut=("random", n)), aces))
        out.append((f"lut-unit-identity-{n}", (33, 9), dict(lut=("identity", n)), aces))
        out.append((f"lut-log2-random-{n}", (33, 9), dict(lut=("random", n), lut_domain=LutDomain.LOG2, lut_ev_min=-9.0, lut_ev_max=5.0), Tonemap.NONE))
    out.append(("lut-log2-stage-a", SIZE, dict(STEPS["wb"], contrast=1.2, lut=("random", 33), lut_domain=LutDomain.LOG2, lut_ev_min=-12.0, lut_ev_max=4.0, dither=True), Tonemap.NONE))
    for strength in (0.0, 0.5, 1.0):
        out.append((f"lut-strength-{strength}", (33, 9), dict(lut=("random", 3), lut_strength=strength), aces))
    out.append(("neutral", (33, 9), dict(), aces))
    return out


def build(kw):
    """(the descriptor with a placeholder handle, the table or None)"""
    kw = dict(kw)
    spec = kw.pop("lut", None)
    table = lut(*spec) if spec is not None else None
    return color_grading_desc(lut=1 if table is not None else 0, **kw), table
