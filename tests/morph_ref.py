"""numpy float32 restatement of k_skin.hip's k_morph (include/strolle_hip.h "morph targets"): the morph stage with the kernel's operations in
the kernel's order, and its composition with the skin stage (skin_ref.skin), so that the device's posed triangles can be compared bit for
bit (st_math.h rules 1-2: +, -, *, / and sqrt only, no FMA)."""
import numpy as np

import skin_ref


def active_targets(weights):
    """The indices of the weights that are not exactly 0, ascending: the targets that take part."""
    w = np.asarray(weights, np.float32).reshape(-1)
    return [k for k in range(len(w)) if w[k] != 0]


def morph(bind: np.ndarray, position_deltas, normal_deltas, weights) -> np.ndarray:
    """Morphed triangles, (n, 24) float32, of `bind` (skin_ref.bind_store) under `weights` ((K,)) of the targets' deltas ((K, n, 3, 3) each)."""
    bind = np.asarray(bind, np.float32).reshape(-1, 24)
    n = len(bind)
    dp = np.asarray(position_deltas, np.float32).reshape(-1, n, 9)
    dn = np.asarray(normal_deltas, np.float32).reshape(-1, n, 9)
    w = np.asarray(weights, np.float32).reshape(-1)
    assert len(w) == len(dp) == len(dn)
    act = active_targets(w)
    out = bind.copy()
    if not act:
        return out                                                              # the base triangle, bit for bit
    f32 = np.float32
    with np.errstate(all="ignore"):
        p = bind[:, 0:9].copy(); nn = bind[:, 9:18].copy()
        for k in act:                                                           # x = x + w[k] * d[k], left to right; zero weights are skipped
            p = p + w[k] * dp[k]
            nn = nn + w[k] * dn[k]
        v = nn.reshape(n, 3, 3)
        length = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])[..., None]   # st_math.h dot, length
        unit = v * (f32(1.0) / length)                                          # st_math.h normalize (exact build)
        keep = (length == 0) | ~np.isfinite(length)
        nrm = np.where(keep, bind[:, 9:18].reshape(n, 3, 3), unit)
    out[:, 0:9] = p
    out[:, 9:18] = nrm.reshape(n, 9)
    return out


def morph_skin(bind, position_deltas, normal_deltas, weights, joints, corner_weights, matrices) -> np.ndarray:
    """Morph, then skin: the morphed positions and normals replace the bind pose at the input of the skin stage."""
    return skin_ref.skin(morph(bind, position_deltas, normal_deltas, weights), joints, corner_weights, matrices)
