"""Bit-exact comparison helpers (test infrastructure)."""
import numpy as np


def bits_equal_mask(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Element-wise: identical bit patterns, or both NaN (NaN payload/sign is not part of the contract:
    x86 produces the negative default NaN for 0/0, gfx950 the positive one)."""
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.dtype == np.float32:
        return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return a == b


def assert_bits_equal(got: np.ndarray, want: np.ndarray, what: str = ""):
    m = bits_equal_mask(got, want)
    if not m.all():
        bad = np.argwhere(~m)
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {m.size} elements differ; first at {first}: got {got[first]!r} want {want[first]!r}")


def psnr(a: np.ndarray, b: np.ndarray, peak: float = 1.0) -> float:
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return float("inf") if mse == 0 else 10.0 * np.log10(peak * peak / mse)


def scene_fingerprint(engine, n_triangles: int) -> dict:
    """sha256 digests of a ticked engine's scene as the host holds it: the triangles (world space; rows sorted, so the order the
    tree keeps them in does not enter), the lights and the materials. tests/golden/scene_fingerprints.json holds those of the
    benchmark scenes as the glTF loader reads the original files."""
    import hashlib
    tri = engine.read_scene(1)
    assert n_triangles > 0 and tri.size % n_triangles == 0, (tri.size, n_triangles)
    rows = np.ascontiguousarray(tri.view(np.uint32).reshape(n_triangles, -1))
    rows = rows[np.lexsort(rows.T[::-1])]
    return {"triangles": int(n_triangles), "triangle_words": int(rows.shape[1]),
            "triangles_sha256": hashlib.sha256(rows.tobytes()).hexdigest(),
            "lights_sha256": hashlib.sha256(engine.read_scene(2).tobytes()).hexdigest(),
            "materials_sha256": hashlib.sha256(engine.read_scene(3).tobytes()).hexdigest()}
