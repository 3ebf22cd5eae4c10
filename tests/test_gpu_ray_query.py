"""Scene queries on the GPU (include/strolle_hip.h "scene queries"; k_query.hip) against the CPU oracle's one-ray probe (or_probe_trace).

The oracle's closest hit of the UNBOUNDED ray, kept where distance < t_max, is exactly the bounded closest hit; its any-hit probe with
len = t_max is the occlusion answer (out[0] < len). Rays with t_max <= 0 or NaN and all-zero directions are misses on both sides without
any special case in the checker."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle_binding import OracleEngine, oracle_lib
from strolle_amd import Buffer, CameraMode, Engine, Instance, Material, Mesh, scenes
from strolle_amd.api import HIT_DTYPE, RAY_DTYPE

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-3, 1e-5          # the fast build's tolerance gate (tests/test_gpu_fast_tolerance.py)
FLT_MAX = np.float32(3.4028235e38)
# Fast build, default tuning: the wide walk tests leaves with the contract's exact Triangle::hit, so a triangle both walks find carries the same t
# bits. What remains are rays whose two candidates tie at a shared edge (either triangle is a correct answer) and grazing box tests where the fast
# slab test and the contract's differ by an ulp: a handful per 10^4 rays.
AGREE = 0.999

_lib = oracle_lib()
_lib.or_probe_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p]
_lib.or_probe_camera_ray.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]


# ----------------------------------------------------------------------------- rays
def make_rays(origins, dirs, t_max):
    r = np.zeros(len(origins), RAY_DTYPE)
    r["origin"] = origins; r["direction"] = dirs; r["t_max"] = t_max
    return r


def camera_rays(desc, n, rng):
    c = desc.to_c(); w, h = desc.size
    xs, ys = rng.integers(0, w, n), rng.integers(0, h, n)
    out = np.zeros((n, 6), np.float32)
    for i in range(n):
        _lib.or_probe_camera_ray(C.byref(c), int(xs[i]), int(ys[i]), out[i].ctypes.data)
    return out[:, :3], out[:, 3:]


def scene_box(orac):
    tris = orac.read_scene(1).view(np.float32).reshape(-1, 9, 4)[:, [0, 3, 6], :3].reshape(-1, 3)
    return tris.min(0), tris.max(0)


def t_max_mix(n, rng, scale):
    """unbounded (inf, FLT_MAX) and bounded t_max, with the degenerate ones (0, negative, NaN) among them"""
    t = rng.uniform(0.05, 1.0, n).astype(np.float32) * np.float32(scale)
    k = rng.integers(0, 10, n)
    t[k < 3] = np.inf
    t[k == 3] = FLT_MAX
    t[k == 4] = rng.choice(np.array([0.0, -1.0, np.nan], np.float32), int((k == 4).sum()))
    return t


def incoherent_rays(orac, n, rng, bounded=True):
    lo, hi = scene_box(orac)
    ext = hi - lo
    o = rng.uniform(lo - 0.2 * ext, hi + 0.2 * ext, (n, 3)).astype(np.float32)   # some outside the scene's box
    d = rng.normal(size=(n, 3)).astype(np.float32) * rng.uniform(0.25, 4.0, (n, 1)).astype(np.float32)   # not normalised
    k = rng.integers(0, 20, n)
    for axis in range(3):   # axis-parallel directions: two components zero (inv_dir of +-inf)
        sel = k == axis
        keep = d[sel, axis].copy(); d[sel] = 0.0; d[sel, axis] = keep
    d[k == 3] = 0.0        # all-zero directions: misses
    t = t_max_mix(n, rng, float(np.linalg.norm(ext))) if bounded else np.full(n, np.inf, np.float32)
    return make_rays(o, d, t)


def query_set(orac, cam_desc, n, seed):
    rng = np.random.default_rng(seed)
    o, d = camera_rays(cam_desc, n, rng)
    lo, hi = scene_box(orac)
    cam = make_rays(o, d, t_max_mix(n, rng, float(np.linalg.norm(hi - lo))))
    return cam, incoherent_rays(orac, n, rng)


# ----------------------------------------------------------------------------- the oracle's answers
def oracle_closest(orac, rays):
    n = len(rays)
    out = np.zeros((n, 11), np.float32)
    for i in range(n):
        _lib.or_probe_trace(orac._h, rays["origin"][i].ctypes.data, rays["direction"][i].ctypes.data, 0.0, 0, out[i].ctypes.data)
    hit = (out[:, 0] < FLT_MAX) & (out[:, 0] < rays["t_max"])   # a miss is distance = FLT_MAX (which is < an infinite t_max); NaN t_max: False
    exp = np.zeros(n, HIT_DTYPE)
    exp["hit"] = hit
    exp["t"] = np.where(hit, out[:, 0], FLT_MAX)
    exp["point"][hit] = out[hit, 1:4]; exp["normal"][hit] = out[hit, 4:7]; exp["uv"][hit] = out[hit, 7:9]
    return exp


def oracle_occluded(orac, rays):
    n = len(rays)
    out = np.zeros(11, np.float32)
    occ = np.zeros(n, bool)
    for i in range(n):
        ln = rays["t_max"][i]
        _lib.or_probe_trace(orac._h, rays["origin"][i].ctypes.data, rays["direction"][i].ctypes.data, ln, 1, out.ctypes.data)
        occ[i] = out[0] < ln
    return occ


# ----------------------------------------------------------------------------- the product's answers
def _dev(a: np.ndarray):
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


def _stream(s=None):
    return (s or torch.cuda.current_stream()).cuda_stream


def gpu_trace(e, rays, coherent=False):
    d_rays = _dev(rays)
    d_hits = torch.full((len(rays) * HIT_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device="cuda")
    e.trace_rays(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), coherent=coherent, stream=_stream())
    torch.cuda.synchronize()
    return d_hits.cpu().numpy().view(HIT_DTYPE)


def gpu_occluded(e, rays):
    d_rays = _dev(rays)
    d_out = torch.full((len(rays),), 7, dtype=torch.int32, device="cuda")
    e.occluded(d_rays.data_ptr(), len(rays), d_out.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    assert set(np.unique(out)) <= {0, 1}
    return out == 1


def gpu_pick(e, cam, pixels):
    d_px = _dev(np.ascontiguousarray(pixels, np.uint32).reshape(-1))
    d_hits = torch.zeros((len(pixels) * HIT_DTYPE.itemsize,), dtype=torch.uint8, device="cuda")
    e.pick(cam, d_px.data_ptr(), len(pixels), d_hits.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    return d_hits.cpu().numpy().view(HIT_DTYPE)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_misses_are_clean(got):
    m = got["hit"] == 0
    assert set(np.unique(got["hit"])) <= {0, 1}
    assert np.all(got["t"][m] == FLT_MAX)
    for f in ("point", "normal", "uv", "barycentric"):
        assert not np.any(got[f][m])
    assert not np.any(got["triangle"][m]) and not np.any(got["instance"][m])


def assert_exact(got, exp, what):
    assert_misses_are_clean(got)
    assert np.array_equal(got["hit"], exp["hit"]), f"{what}: {int((got['hit'] != exp['hit']).sum())} hit / miss disagreements"
    for f in ("t", "point", "normal", "uv"):
        bad = np.any(bits(got[f]).reshape(len(got), -1) != bits(exp[f]).reshape(len(got), -1), axis=1)
        assert not bad.any(), f"{what}: {f} differs on {int(bad.sum())} rays (first: {np.flatnonzero(bad)[:5]})"


def assert_within_gate(got, exp, what):
    assert_misses_are_clean(got)
    agree = got["hit"] == exp["hit"]
    assert agree.mean() >= AGREE, f"{what}: hit / miss agree on {agree.mean():.5f}"
    both = (got["hit"] == 1) & (exp["hit"] == 1)
    assert both.sum() > 0.1 * len(got), f"{what}: too few hits to say anything ({int(both.sum())})"
    same_t = bits(got["t"][both]) == bits(exp["t"][both])
    assert same_t.mean() >= AGREE, f"{what}: t bit-identical on {same_t.mean():.5f} of the common hits"
    keep = both.copy(); keep[both] = same_t   # attributes of the same triangle
    for f in ("point", "normal", "uv"):
        g, x = got[f][keep], exp[f][keep]
        close = np.all(np.abs(g - x) <= ATOL + RTOL * np.abs(x), axis=1)
        assert close.mean() >= AGREE, f"{what}: {f} within the gate on {close.mean():.5f}"


# ----------------------------------------------------------------------------- scenes
def _pair(build, exact):
    prod, orac = Engine(device=0, exact=exact), OracleEngine()
    for e in (prod, orac):
        build(e)
        e.tick()
    return prod, orac


SCENES = {
    "cornell": (scenes.build_cornell, scenes.cornell_camera((320, 240))),
    "dungeon": (scenes.build_dungeon, scenes.dungeon_camera((320, 180))),
    "blend_soup": (lambda e: scenes.build_random_soup(e, 3000, seed=3, blend_fraction=0.5), scenes.camera_for((320, 240), (0.0, 0.3, 3.0), (0.0, 0.0, 0.0))),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_exact_build_is_bit_identical_to_the_oracle(name):
    build, cam_desc = SCENES[name]
    prod, orac = _pair(build, True)
    try:
        for kind, rays in zip(("camera", "incoherent"), query_set(orac, cam_desc, 8192, seed=11)):
            exp = oracle_closest(orac, rays)
            assert exp["hit"].mean() > 0.1, f"{name} {kind}: the rays must hit something"
            assert_exact(gpu_trace(prod, rays), exp, f"{name} {kind}")
            assert np.array_equal(gpu_occluded(prod, rays), oracle_occluded(orac, rays)), f"{name} {kind}: occlusion"
    finally:
        prod.close(); orac.close()


@pytest.mark.parametrize("subdivide", [0, 2])
def test_fast_build_within_the_gate(subdivide):
    prod, orac = _pair(lambda e: scenes.build_dungeon(e, subdivide=subdivide), False)
    try:
        assert not prod.exact
        cam_rays, inc_rays = query_set(orac, scenes.dungeon_camera((320, 180)), 8192, seed=23 + subdivide)
        for kind, rays in (("camera", cam_rays), ("incoherent", inc_rays)):
            got = gpu_trace(prod, rays)
            assert_within_gate(got, oracle_closest(orac, rays), f"dungeon/{subdivide} {kind}")
            occ = gpu_occluded(prod, rays) == oracle_occluded(orac, rays)
            assert occ.mean() >= AGREE, f"dungeon/{subdivide} {kind}: occlusion agrees on {occ.mean():.5f}"
        plain, packet = gpu_trace(prod, cam_rays), gpu_trace(prod, cam_rays, coherent=True)
        assert np.array_equal(plain["hit"], packet["hit"]) and np.array_equal(bits(plain["t"]), bits(packet["t"])), "ST_RAY_COHERENT changed the answer"
    finally:
        prod.close(); orac.close()


SPAWN = 90001


def _torus_at(x, y, z, scale=0.6):
    return np.array([[scale, 0, 0, x], [0, 0, -scale, y], [0, scale, 0, z]], np.float32)   # standing up, facing the dungeon camera


def _rays_at(point, n, rng, origin=(-5.75, 0.5, -16.8)):
    o = np.tile(np.asarray(origin, np.float32), (n, 1))
    target = np.asarray(point, np.float32) + rng.uniform(-0.8, 0.8, (n, 3)).astype(np.float32)
    return make_rays(o, target - o, np.full(n, np.inf, np.float32))


def test_device_built_tree_follows_spawn_moves_and_despawn():
    prod, orac = _pair(scenes.build_dungeon, False)
    try:
        rng = np.random.default_rng(5)
        base_rays = np.concatenate(query_set(orac, scenes.dungeon_camera((320, 180)), 1024, seed=31))
        for e in (prod, orac):
            e.insert_material(SPAWN, Material(base_color=(0.8, 0.2, 0.2, 1.0)))
        builds0 = prod.device_builds()
        pos = [-5.75, 0.5, -17.8]
        for step in range(16):
            inst = Instance(5000, SPAWN, _torus_at(*pos))
            for e in (prod, orac):
                e.insert_instance(SPAWN, inst)
                e.tick()
            if step == 0:
                assert prod.device_builds() > builds0, "the spawn must be answered by a device LBVH build"
            rays = np.concatenate([base_rays, _rays_at(pos, 512, rng)])
            got = gpu_trace(prod, rays)
            assert_within_gate(got, oracle_closest(orac, rays), f"step {step}")
            assert (got["instance"] == SPAWN).sum() > 100, f"step {step}: the spawned instance is not hit"
            pos[0] += 0.05; pos[2] -= 0.02
        for e in (prod, orac):
            e.remove_instance(SPAWN)
            e.tick()
        rays = np.concatenate([base_rays, _rays_at(pos, 512, rng)])
        got = gpu_trace(prod, rays)
        assert not (got["instance"] == SPAWN).any(), "a despawned instance was hit"
        assert_within_gate(got, oracle_closest(orac, rays), "after despawn")
    finally:
        prod.close(); orac.close()


def test_hits_identify_instance_and_mesh_triangle():
    rng = np.random.default_rng(9)
    n_tri = 400
    c = rng.uniform(-1, 1, (n_tri, 1, 3)).astype(np.float32)
    pos = (c + rng.uniform(-0.2, 0.2, (n_tri, 3, 3))).astype(np.float32)
    nrm = np.cross(pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.repeat(nrm[:, None], 3, 1).astype(np.float32)
    uv = rng.uniform(0, 1, (n_tri, 3, 2)).astype(np.float32)
    xforms = {}
    e = Engine(device=0)
    try:
        e.set_blue_noise(scenes.load_blue_noise())
        e.insert_material(1, Material(base_color=(0.5, 0.5, 0.5, 1.0)))
        e.insert_mesh(7, Mesh(pos, nrm, uv))
        for k, h in enumerate((101, 202, 303, 404)):
            a = 0.7 * k
            rot = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], np.float32) * np.float32(0.5 + 0.25 * k)
            x = np.concatenate([rot, np.array([[3.0 * k], [0.2 * k], [0.0]], np.float32)], 1).astype(np.float32)
            xforms[h] = x
            e.insert_instance(h, Instance(7, 1, x))
        e.tick()
        o = np.tile(np.array([4.5, 0.5, 8.0], np.float32), (8192, 1))
        target = rng.uniform([-1.5, -1.2, -1.5], [10.5, 1.8, 1.5], (8192, 3)).astype(np.float32)
        got = gpu_trace(e, make_rays(o, target - o, np.full(8192, np.inf, np.float32)))
        hit = got["hit"] == 1
        assert hit.mean() > 0.15
        seen = set()
        for r in np.flatnonzero(hit):
            h = int(got["instance"][r]); t = int(got["triangle"][r])
            assert h in xforms and 0 <= t < n_tri, (h, t)
            seen.add(h)
            x = xforms[h].astype(np.float64)
            p = pos[t].astype(np.float64) @ x[:, :3].T + x[:, 3]
            u, v = got["barycentric"][r].astype(np.float64)
            want = (1 - u - v) * p[0] + u * p[1] + v * p[2]
            assert np.allclose(got["point"][r], want, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(want).max())), (r, got["point"][r], want)
            # closest_resolve: the interpolated normal, turned by the sign of 1/det (the side of the triangle the ray came from)
            d = (target[r] - o[r]).astype(np.float64)
            det = np.dot(p[1] - p[0], np.cross(d, p[2] - p[0]))
            n_world = np.linalg.inv(x[:, :3]).T @ nrm[t, 0].astype(np.float64)
            assert np.sign(np.dot(got["normal"][r], n_world)) == np.sign(det), r
        assert seen == set(xforms), f"every instance of the shared mesh must be hit: {seen}"
    finally:
        e.close()


@pytest.mark.parametrize("exact", [True, False])
def test_picks_equal_the_frame_on_screen(exact):
    size = (256, 144)
    e = Engine(device=0, exact=exact)
    try:
        scenes.build_dungeon(e)
        desc = scenes.dungeon_camera(size, CameraMode.REFERENCE, depth=0)
        cam = e.create_camera(desc)
        e.tick()
        out = torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda")

        def frame():
            e.render_camera(cam, out.data_ptr(), _stream())
            torch.cuda.synchronize()
            return e.read_buffer(cam, Buffer.REF_HITS).reshape(size[1], size[0], -1).copy()

        rng = np.random.default_rng(3)
        px = np.stack([rng.integers(0, size[0], 4096), rng.integers(0, size[1], 4096)], 1).astype(np.uint32)
        outside = np.array([[size[0], 0], [0, size[1]], [size[0] + 7, size[1] + 3], [0xFFFFFFFF, 5]], np.uint32)

        def check(got, hits, what):
            ref = hits[px[:, 1], px[:, 0]]
            want_hit = np.any(ref[:, :3] != 0, axis=1)   # hit.rs: a zero point is a miss
            assert np.array_equal(got["hit"] == 1, want_hit), what
            for f, sl in (("point", slice(0, 3)), ("uv", slice(6, 8))):
                g, x = got[f][want_hit], ref[want_hit, sl]
                if exact:
                    assert np.array_equal(bits(g), bits(x)), f"{what}: {f}"
                else:
                    assert np.all(np.abs(g - x) <= ATOL + RTOL * np.abs(x)), f"{what}: {f}"

        hits0 = frame()
        check(gpu_pick(e, cam, px), hits0, "first frame")
        miss = gpu_pick(e, cam, outside)
        assert not miss["hit"].any(); assert_misses_are_clean(miss)
        moved = scenes.camera_for(size, (-5.0, 0.7, -15.0), (-6.0, 0.5, -18.0), CameraMode.REFERENCE, depth=0)
        e.update_camera(cam, moved)
        check(gpu_pick(e, cam, px), hits0, "after update, before render: the frame on screen")
        hits1 = frame()
        assert not np.array_equal(hits0, hits1)
        check(gpu_pick(e, cam, px), hits1, "after the render")
    finally:
        e.close()


def test_queries_on_another_stream_follow_the_ticks():
    rays = None
    size = (64, 64)

    def run(sync):
        e = Engine(device=0)
        scenes.build_dungeon(e)
        cam = e.create_camera(scenes.dungeon_camera(size, CameraMode.REFERENCE, depth=0))
        e.insert_material(SPAWN, Material(base_color=(0.8, 0.2, 0.2, 1.0)))
        e.tick()
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        out = torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda")
        d_rays = _dev(rays)
        hits = [torch.zeros((len(rays) * HIT_DTYPE.itemsize,), dtype=torch.uint8, device="cuda") for _ in range(20)]
        torch.cuda.synchronize()
        pos = [-5.75, 0.5, -17.8]
        for it in range(20):
            if it % 5 == 0:
                e.insert_instance(SPAWN + it, Instance(5000, SPAWN, _torus_at(*pos)))   # a spawn
            else:
                e.insert_instance(SPAWN + it - it % 5, Instance(5000, SPAWN, _torus_at(*pos)))   # a move
            pos[0] += 0.1
            e.tick(a.cuda_stream)
            if sync: torch.cuda.synchronize()
            e.trace_rays(d_rays.data_ptr(), len(rays), hits[it].data_ptr(), stream=b.cuda_stream)
            if sync: torch.cuda.synchronize()
            e.render_camera(cam, out.data_ptr(), a.cuda_stream)
            if sync: torch.cuda.synchronize()
        torch.cuda.synchronize()
        res = [h.cpu().numpy().view(HIT_DTYPE).copy() for h in hits]
        e.close()
        return res

    rng = np.random.default_rng(17)
    rays = np.concatenate([_rays_at((-5.75 + 0.1 * k, 0.5, -17.8), 128, rng) for k in range(20)])
    free, ordered = run(False), run(True)
    for it in range(20):
        assert free[it].tobytes() == ordered[it].tobytes(), f"iteration {it}: the query on stream B saw another scene than the tick before it"
    assert any((r["instance"] >= SPAWN).any() for r in ordered)

    empty = Engine(device=0)
    try:
        empty.tick()
        got = gpu_trace(empty, rays[:256])
        assert not got["hit"].any(); assert_misses_are_clean(got)
    finally:
        empty.close()


def test_host_call_equals_the_device_call():
    prod, orac = _pair(scenes.build_dungeon, False)
    try:
        rays = np.concatenate(query_set(orac, scenes.dungeon_camera((320, 180)), 4096, seed=41))
        dev = gpu_trace(prod, rays)
        host = prod.trace_rays_host(rays)
        assert host.dtype == HIT_DTYPE and host.tobytes() == dev.tobytes()
        assert prod.trace_rays_host(rays[:100]).tobytes() == dev[:100].tobytes()   # the engine's buffers, reused smaller
    finally:
        prod.close(); orac.close()


# ----------------------------------------------------------------------------- the alpha test, over every stream
# Two layers of ALPHA_GRID x ALPHA_GRID unit quads (z = 0 and z = -1), AlphaMode::Blend, all on ONE 32 x 32 texture whose alpha is a checkerboard of 0 / 255 in
# 8 x 8-texel blocks (4 x 4 blocks per quad). Rays cross a layer only at "safe points": 2.5 / 5.5 texels into a block, so the four bilinear taps
# lie in one block (alpha exactly 0 or 1), at least 2.5 texels (0.078 of a quad) from every quad edge and 3 texels off the quad's diagonal. The
# answer of every ray is therefore decided — by the geometry below, in float64 — and each walk owes the same triangle and the same occlusion bit.
ALPHA_GRID, ALPHA_BLOCK, ALPHA_TEXELS = 12, 8, 32
ALPHA_LAYER_SHIFT = ((0.0, 0.0), (0.5, 0.125))      # layer 1 lies (0.5, 0.125) beside layer 0: a ray along ALPHA_COHERENT_DIR arrives one block to the left
ALPHA_COHERENT_DIR = np.array([0.25, 0.125, -1.0])
ALPHA_CONFIGS = {"exact": (True, {}), "default": (False, {}), "no_packets": (False, {"primary_packets": 0}), "no_wide": (False, {"wide_bvh": 0}),
                 "no_compact": (False, {"compact_bvh": 0}), "no_anyhit_fast": (False, {"anyhit_fast": 0})}


def _build_alpha_layers(e):
    e.set_blue_noise(scenes.load_blue_noise())
    tex = np.full((ALPHA_TEXELS, ALPHA_TEXELS, 4), 200, np.uint8)
    ty, tx = np.mgrid[0:ALPHA_TEXELS, 0:ALPHA_TEXELS]
    tex[..., 3] = np.where((tx // ALPHA_BLOCK + ty // ALPHA_BLOCK) % 2 == 0, 255, 0)
    e.insert_image(900, tex, srgb=True)
    e.insert_material(1, Material(base_color=(1.0, 1.0, 1.0, 1.0), base_color_texture=900, alpha_mode=1))
    pos, uv = [], []
    for layer, (sx, sy) in enumerate(ALPHA_LAYER_SHIFT):
        for j in range(ALPHA_GRID):
            for i in range(ALPHA_GRID):
                x0, y0, z = i - ALPHA_GRID / 2 + sx, j - ALPHA_GRID / 2 + sy, -float(layer)
                p00, p10, p11, p01 = (x0, y0, z), (x0 + 1, y0, z), (x0 + 1, y0 + 1, z), (x0, y0 + 1, z)
                pos += [[p00, p10, p11], [p00, p11, p01]]          # triangle 2 q: u > v (below the diagonal), 2 q + 1: above it
                uv += [[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]]
    pos = np.asarray(pos, np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (len(pos), 3, 1))
    e.insert_mesh(7, Mesh(pos, nrm, np.asarray(uv, np.float32)))
    e.insert_instance(77, Instance(7, 1, np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)))
    return len(pos)


def _safe_points(layer, rng, n=None):
    """world positions of safe points on `layer`: one per block in raster order (n = None), or n random ones"""
    if n is None:
        j, i, by, bx = [a.reshape(-1) for a in np.mgrid[0:ALPHA_GRID, 0:ALPHA_GRID, 0:4, 0:4]]   # a run of 64 consecutive rays: four neighbouring quads
    else:
        i, j, bx, by = (rng.integers(0, ALPHA_GRID, n), rng.integers(0, ALPHA_GRID, n), rng.integers(0, 4, n), rng.integers(0, 4, n))
    sx, sy = ALPHA_LAYER_SHIFT[layer]
    x = i - ALPHA_GRID / 2 + sx + (ALPHA_BLOCK * bx + 2.5) / ALPHA_TEXELS
    y = j - ALPHA_GRID / 2 + sy + (ALPHA_BLOCK * by + 5.5) / ALPHA_TEXELS
    return np.stack([x, y, np.full(len(x), -float(layer))], 1)


def _alpha_expected(rays):
    """(hit, triangle, occluded) of every ray, from the construction alone"""
    o, d, t_max = rays["origin"].astype(np.float64), rays["direction"].astype(np.float64), rays["t_max"].astype(np.float64)
    best_t = np.full(len(rays), np.inf); best_tri = np.zeros(len(rays), np.uint32)
    for layer, (sx, sy) in enumerate(ALPHA_LAYER_SHIFT):
        t = (-float(layer) - o[:, 2]) / d[:, 2]
        lx, ly = o[:, 0] + t * d[:, 0] + ALPHA_GRID / 2 - sx, o[:, 1] + t * d[:, 1] + ALPHA_GRID / 2 - sy
        inside = (t > 0) & (lx > 0) & (lx < ALPHA_GRID) & (ly > 0) & (ly < ALPHA_GRID)
        i, j = np.floor(lx), np.floor(ly)
        u, v = (lx - i) * ALPHA_TEXELS, (ly - j) * ALPHA_TEXELS                                # texel coordinates inside the quad
        margin = np.minimum.reduce([u % ALPHA_BLOCK - 0.5, ALPHA_BLOCK - 0.5 - u % ALPHA_BLOCK, v % ALPHA_BLOCK - 0.5, ALPHA_BLOCK - 0.5 - v % ALPHA_BLOCK, np.abs(u - v)])
        outside = np.maximum.reduce([-lx, lx - ALPHA_GRID, -ly, ly - ALPHA_GRID])
        assert np.all(np.where(inside, margin, outside * ALPHA_TEXELS) > 1.0), "a ray of this test leaves the safe points"
        opaque = inside & ((u // ALPHA_BLOCK + v // ALPHA_BLOCK) % 2 == 0)
        tri = (2 * (layer * ALPHA_GRID * ALPHA_GRID + j * ALPHA_GRID + i) + (v > u)).astype(np.int64)
        closer = opaque & (t < best_t)
        best_t[closer] = t[closer]; best_tri[closer] = tri[closer]
    hit = best_t < t_max
    assert np.all(np.abs(best_t[np.isfinite(best_t)] / t_max[np.isfinite(best_t)] - 1.0) > 0.05), "a t_max of this test is too close to a hit"
    return hit, np.where(hit, best_tri, 0), hit


@pytest.fixture(scope="module")
def alpha_rays():
    rng = np.random.default_rng(29)
    p0 = _safe_points(0, rng)                                    # coherent: parallel rays through every block of layer 0, in raster order
    coherent = (p0 - 2.0 * ALPHA_COHERENT_DIR, np.tile(ALPHA_COHERENT_DIR, (len(p0), 1)))
    a, b = _safe_points(0, rng, len(p0)), _safe_points(1, rng, len(p0))   # incoherent: through a random safe point of each layer, either way
    flip = rng.integers(0, 2, len(p0)).astype(bool)[:, None]
    a, b = np.where(flip, b, a), np.where(flip, a, b)
    s = rng.uniform(0.5, 2.0, (len(p0), 1))
    incoherent = (a - s * (b - a), (b - a) * rng.uniform(0.5, 2.0, (len(p0), 1)))
    sets = {}
    for name, (o, d) in (("coherent", coherent), ("incoherent", incoherent)):
        o32, d32 = o.astype(np.float32), d.astype(np.float32)
        t1 = (a if name == "incoherent" else p0)[:, 2] - o32[:, 2]; t1 = t1 / d32[:, 2]   # the ray parameter at its first layer ...
        t2 = t1 + np.abs(1.0 / d32[:, 2])                                                 # ... and at its second
        k = rng.integers(0, 4, len(o32))
        t_max = np.select([k == 0, k == 1, k == 2], [0.5 * t1, 0.5 * (t1 + t2), 1.5 * t2], np.inf).astype(np.float32)
        rays = make_rays(o32, d32, t_max)
        sets[name] = (rays,) + _alpha_expected(rays)
    for name, (_, hit, tri, _) in sets.items():
        assert 0.2 < hit.mean() < 0.8 and len(np.unique(tri[hit] // (2 * ALPHA_GRID * ALPHA_GRID))) == 2, f"{name}: both layers and the holes must be met"
    return sets


@pytest.mark.parametrize("config", list(ALPHA_CONFIGS))
def test_alpha_test_decides_the_same_in_every_walk(config, alpha_rays):
    """The alpha test (AlphaMode::Blend: a hit counts where the base colour's alpha is 1) through st_scene_trace_rays and st_scene_occluded, in the
    exact build and over each stream of the fast build: contract, compact, wide, and the wide stream's packets (ST_RAY_COHERENT)."""
    exact, tuning = ALPHA_CONFIGS[config]
    e = Engine(device=0, exact=exact)
    try:
        if tuning:
            e.set_tuning(**tuning)
        n_tri = _build_alpha_layers(e)
        e.tick()
        assert 4 * (2 * n_tri - 1) > 448, "the stream must not fit the LDS scene copy (kLdsSceneTexels), or no compact / wide stream is built"
        for name, (rays, hit, tri, occ) in alpha_rays.items():
            for coherent in (False, True):
                got = gpu_trace(e, rays, coherent=coherent)
                what = f"{config} {name} coherent={coherent}"
                assert_misses_are_clean(got)
                assert np.array_equal(got["hit"] == 1, hit), f"{what}: {int(((got['hit'] == 1) != hit).sum())} hit / miss disagreements"
                assert np.array_equal(got["triangle"], tri), f"{what}: {int((got['triangle'] != tri).sum())} rays found another triangle"
                assert np.all(got["instance"][hit] == 77)
            assert np.array_equal(gpu_occluded(e, rays), occ), f"{config} {name}: occlusion"
    finally:
        e.close()
