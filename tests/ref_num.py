"""What the numpy restatements of the output chain (fog_ref, shafts_ref, dof_ref, motion_blur_ref, bloom_ref, post_ref) share: the header's
min, max and clamp01 with the post-processing section's NaN rule, the colour clamp, and the depth of a frame. Both operands are taken to
float32 before they are compared, so a Python or float64 operand is rounded once, as the kernels' float constants are."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
COLOUR_CLAMP = 65504.0


def min2(a, b):
    """the header's min: a when a < b or b is NaN, else b"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.where((a < b) | (b != b), a, b).astype(np.float32)


def max2(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.where((a > b) | (b != b), a, b).astype(np.float32)


def clamp01(x):
    return min2(max2(x, F(0)), F(1))


def frame_depth(g0x):
    """D of a frame: PRIM_GBUFFER_D0.x with 0 (sky) read as FLT_MAX"""
    g0x = np.asarray(g0x, np.float32)
    return np.where(g0x == 0, FLT_MAX, g0x).astype(np.float32)


def colour(c):
    """the first three channels held to [0, 65504]"""
    return min2(max2(np.asarray(c, np.float32)[..., :3], F(0)), F(COLOUR_CLAMP))
