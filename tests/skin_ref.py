"""numpy float32 restatement of k_skin.hip (include/strolle_hip.h "skinned meshes"): linear blend skinning with the kernel's operations in
the kernel's order, so that the device's posed triangles can be compared bit for bit (st_math.h rules 1-2: +, -, *, /, sqrt only, no FMA)."""
import numpy as np


def bind_store(mesh) -> np.ndarray:
    """A Mesh in the device mesh store's layout: (n, 24) float32 — positions 9, normals 9, uvs 6."""
    n = len(mesh.positions)
    return np.concatenate([mesh.positions.reshape(n, 9), mesh.normals.reshape(n, 9), mesh.uvs.reshape(n, 6)], 1).astype(np.float32)


def palette12(matrices) -> np.ndarray:
    """(J, 3, 4) matrices (Instance.transform style) -> (J, 12) float32 in Affine3A column order: x, y, z, t (what Engine.set_pose sends)."""
    m = np.asarray(matrices, np.float32).reshape(-1, 3, 4)
    return np.ascontiguousarray(m.transpose(0, 2, 1).reshape(-1, 12))


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0], a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def skin(bind: np.ndarray, joints, weights, matrices) -> np.ndarray:
    """Posed triangles, (n, 24) float32, of `bind` (bind_store) under the palette `matrices` ((J, 3, 4)), corners' joints / weights (3n, 4)."""
    bind = np.asarray(bind, np.float32).reshape(-1, 24)
    n = len(bind)
    pal = palette12(matrices)
    J = np.asarray(joints, np.int64).reshape(n, 3, 4)
    W = np.asarray(weights, np.float32).reshape(n, 3, 4)
    f32 = np.float32
    with np.errstate(all="ignore"):
        M = W[..., 0, None] * pal[J[..., 0]]                                       # ((w0 J0 + w1 J1) + w2 J2) + w3 J3, per element
        for s in range(1, 4):
            M = M + W[..., s, None] * pal[J[..., s]]
        ax, ay, az, at = M[..., 0:3], M[..., 3:6], M[..., 6:9], M[..., 9:12]
        q = bind[:, 0:9].reshape(n, 3, 3)
        p = ((ax * q[..., 0:1] + ay * q[..., 1:2]) + az * q[..., 2:3]) + at        # Affine3A::transform_point3
        nn = bind[:, 9:18].reshape(n, 3, 3)
        c0, c1, c2 = _cross(ay, az), _cross(az, ax), _cross(ax, ay)
        det = _dot(az, c2)[..., None]
        acc = (c0 / det) * nn[..., 0:1]
        acc = acc + (c1 / det) * nn[..., 1:2]
        acc = acc + (c2 / det) * nn[..., 2:3]
        length = np.sqrt(_dot(acc, acc))[..., None]
        nrm = acc * (f32(1.0) / length)                                            # st_math.h normalize (exact build)
        nrm = np.where(det == 0, nn, nrm)
    out = np.empty((n, 24), np.float32)
    out[:, 0:9] = p.reshape(n, 9)
    out[:, 9:18] = nrm.reshape(n, 9)
    out[:, 18:24] = bind[:, 18:24]
    return out
