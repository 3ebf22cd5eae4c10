"""Numpy restatement of deformation motion (include/strolle_hip.h "skinned meshes"; strolle_amd/csrc/st_traverse.h deform_prev_point).

The deformation term is restated in float32, one rounding per operation, in the kernel's order:
    w          = (1 - u) - v
    o          = ((q0 * w) + (q1 * u)) + (q2 * v)            per component; q0..q2: the triangle's PREVIOUS posed object-space positions
    prev_point = ((x * o.x + y * o.y) + z * o.z) + t          x, y, z, t: the columns of the instance's previous transform
The screen projection (camera.rs world_to_clip / clip_to_screen) is evaluated in float64 from the camera DESCRIPTION — projection x
inverse(transform) — so that an expected velocity rests on nothing the engine computed; the tests compare within the velocity map's
1e-3 px tolerance, four orders of magnitude above float32 rounding at these image sizes."""
import numpy as np

f32 = np.float32
THRESHOLD = 0.001   # squared length below which the velocity plane stores 0 (prim_raster.rs)


def affine_point32(xform, p):
    """glam Affine3A::transform_point3 in float32: xform (3, 4) [axes | translation] in maths layout, p (..., 3)."""
    m = np.asarray(xform, f32)
    p = np.asarray(p, f32)
    x, y, z, t = m[:, 0], m[:, 1], m[:, 2], m[:, 3]
    return ((x * p[..., 0:1] + y * p[..., 1:2]) + z * p[..., 2:3]) + t


def deformed_prev_point(q_prev, u, v, prev_xform):
    """q_prev (..., 3 corners, 3) previous posed object-space positions of the hit triangles, (u, v) Triangle::hit's barycentrics."""
    q = np.asarray(q_prev, f32)
    u = np.asarray(u, f32)[..., None]; v = np.asarray(v, f32)[..., None]
    w = (f32(1.0) - u) - v
    o = ((q[..., 0, :] * w) + (q[..., 1, :] * u)) + (q[..., 2, :] * v)
    return affine_point32(prev_xform, o)


def rigid_prev_point(xform, prev_xform, point):
    """prim_raster.rs:21-27: prev_xform x inverse(xform) x point (float64: the rigid formula's own bits are not this module's subject)."""
    def m4(a):
        m = np.eye(4); m[:3, :] = np.asarray(a, np.float64); return m
    p = np.concatenate([np.asarray(point, np.float64), np.ones(np.shape(point)[:-1] + (1,))], -1)
    return (p @ (m4(prev_xform) @ np.linalg.inv(m4(xform))).T)[..., :3]


def screen(camera, point):
    """Pixel position of a world-space point under a strolle_amd.Camera description (projection x inverse(transform); y flipped)."""
    pv = np.asarray(camera.projection, np.float64) @ np.linalg.inv(np.asarray(camera.transform, np.float64))
    p = np.concatenate([np.asarray(point, np.float64), np.ones(np.shape(point)[:-1] + (1,))], -1)
    clip = p @ pv.T
    ndc = clip[..., :2] / clip[..., 3:4]
    ndc = ndc * np.array([1.0, -1.0])
    return (0.5 * ndc + 0.5) * np.array([float(camera.size[0]), float(camera.size[1])])


def velocity(camera, prev_camera, point, prev_point, threshold=True):
    """screen(camera, point) - screen(prev_camera, prev_point), zero where its squared length is below 0.001."""
    vel = screen(camera, point) - screen(prev_camera, prev_point)
    if threshold:
        vel = np.where(np.sum(vel * vel, -1, keepdims=True) >= THRESHOLD, vel, 0.0)
    return vel
