"""numpy restatements for the environment-lighting tests (include/strolle_hip.h "environment lighting"): a Radiance .hdr writer (flat and
new-style run-length scanlines), the RGBE conversion m * 2^(e - 136), and the map's look-up (st_device.h env_eval)."""
import math

import numpy as np


def rgbe_to_float(rgbe: np.ndarray) -> np.ndarray:
    """(..., 4) uint8 -> (..., 3) float32: m * 2^(e - 136), e == 0 -> 0 (exact in float64, one rounding to float32)."""
    m = rgbe[..., :3].astype(np.float64)
    e = rgbe[..., 3:4].astype(np.int64)
    out = m * np.ldexp(1.0, e - 136)
    return np.where(e == 0, 0.0, out).astype(np.float32)


def _rle_channel(v: np.ndarray) -> bytes:
    out, i, n = bytearray(), 0, len(v)
    while i < n:
        run = 1
        while i + run < n and run < 127 and v[i + run] == v[i]:
            run += 1
        if run >= 3:
            out += bytes([128 + run, int(v[i])]); i += run
            continue
        j = i   # a literal up to the next run of 3 (or 128 bytes)
        while j < n and j - i < 128 and not (j + 2 < n and v[j] == v[j + 1] == v[j + 2]):
            j += 1
        out += bytes([j - i]) + bytes(int(x) for x in v[i:j]); i = j
    return bytes(out)


def write_hdr(rgbe: np.ndarray, rle: bool = True, magic: str = "#?RADIANCE", extra_header=("EXPOSURE=1.5",),
              fmt: str = "32-bit_rle_rgbe", resolution: str = None) -> bytes:
    """(H, W, 4) uint8 RGBE -> .hdr bytes. rle: new-style runs per scanline where the format allows it (8 <= W < 32768)."""
    h, w, _ = rgbe.shape
    head = [magic, "# written by tests/env_ref.py"] + list(extra_header) + [f"FORMAT={fmt}", ""]
    out = bytearray(("\n".join(head) + "\n" + (resolution or f"-Y {h} +X {w}") + "\n").encode())
    for y in range(h):
        if rle and 8 <= w < 32768:
            out += bytes([2, 2, w >> 8, w & 255])
            for c in range(4):
                out += _rle_channel(rgbe[y, :, c])
        else:
            out += rgbe[y].tobytes()
    return bytes(out)


def random_rgbe(rng, h, w, runs=True) -> np.ndarray:
    """RGBE texels with exponents over the whole range (0 included) and, with runs, long constant stretches; no (1, 1, 1, x) texels
    (old-style run markers)."""
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    px[..., 3] = rng.choice(np.array([0, 1, 9, 100, 127, 128, 129, 140, 200, 255], np.uint8), (h, w))
    if runs:
        for y in range(h):
            a = int(rng.integers(0, w)); b = min(w, a + int(rng.integers(3, 200)))
            px[y, a:b] = px[y, a]
    flat = (px[..., 0] == 1) & (px[..., 1] == 1) & (px[..., 2] == 1)
    px[flat, 0] = 2
    return px


def env_uv(d: np.ndarray):
    u = 0.5 + np.arctan2(d[:, 0], -d[:, 2]) / (2.0 * math.pi)
    v = np.arccos(np.clip(d[:, 1], -1.0, 1.0)) / math.pi
    return u, v


def env_local(dirs: np.ndarray, yaw: float) -> np.ndarray:
    """the world direction rotated by -yaw about +Y"""
    c, s = math.cos(yaw), math.sin(yaw)
    x, y, z = dirs[:, 0], dirs[:, 1], dirs[:, 2]
    return np.stack([c * x - s * z, y, s * x + c * z], axis=1)


def env_eval(texels: np.ndarray, dirs: np.ndarray, yaw: float = 0.0, intensity: float = 1.0) -> np.ndarray:
    """bilinear at texel centres, wrapping in u and clamping in v (float64)"""
    t = texels[..., :3].astype(np.float64)
    h, w, _ = t.shape
    u, v = env_uv(env_local(dirs.astype(np.float64), yaw))
    fx, fy = u * w - 0.5, v * h - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0)[:, None], (fy - y0)[:, None]
    x0 = x0.astype(np.int64); y0 = y0.astype(np.int64)
    xa, xb = x0 % w, (x0 + 1) % w
    ya, yb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    top = t[ya, xa] + (t[ya, xb] - t[ya, xa]) * tx
    bot = t[yb, xa] + (t[yb, xb] - t[yb, xa]) * tx
    return (top + (bot - top) * ty) * intensity


def smooth_map(h: int, w: int) -> np.ndarray:
    """a positive map of low frequencies (neighbouring texels differ little: float32 look-ups agree with float64 ones to ~1e-6)"""
    v = (np.arange(h)[:, None] + 0.5) / h
    u = (np.arange(w)[None, :] + 0.5) / w
    base = 1.0 + 0.5 * np.sin(2 * math.pi * u) * np.cos(math.pi * v) + 0.25 * np.cos(4 * math.pi * u + 1.0)
    return np.stack([base, 0.5 + 0.3 * base * v, 2.0 - base * 0.5], axis=-1).astype(np.float32)


def uniform_sphere(rng, n: int) -> np.ndarray:
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
