"""Hit attributes, texture sampling, material channels and motion vectors of both builds against their float64 definition (tests/surface_ref.py: from
the arrays handed to the API, no read_scene record, no atlas rectangle, no tree), for every case of tests/surface_families.py, through three surfaces:

  st_scene_trace_rays, with and without ST_RAY_COHERENT: instance and mesh triangle identical on every non-ambiguous ray; barycentrics, t, point, normal
      (as an angle) and uv within the case's tolerance
  st_camera_render_aovs, all six planes per pixel: DEPTH, NORMAL, ALBEDO (the only unquantised view of the texture path: held to the texture model
      a + b x slope x delta per pixel), MOTION, INSTANCE, TRIANGLE
  one Image frame with keep_all_planes: the decoded G-buffer within one code of the definition's quantised roughness, metallic and base colour, emissive,
      depth and normal within tolerance, the velocity plane equal to ST_AOV_MOTION bit for bit

The tolerances are surface_families.TOLERANCES: 4 x the ORACLE's own worst deviation from the definition, measured on the CPU by tests/test_surface_ref.py
and never on a HIP build. The exact build additionally equals the oracle bit for bit wherever the oracle has the value (or_probe_surface_rays, its
G-buffer and velocity planes) — on all rays, ambiguous, border and undefined ones included.

Measured on one MI355X (profiles/surface_attributes.json): no case of either build used more than 0.36 of a tolerance (the oracle itself uses 0.25); the
fast build's default and primary_packets=0 runs stay within 0.29 (the G-buffer's normal on the per-face quads), wide_bvh=0 reaches 0.36 (the G-buffer's depth on
the icospheres). What the parent commit failed
is in the profile's `findings`: in the fast build ST_AOV_DEPTH and ST_AOV_MOTION were an ulp off the frame's own planes for scenes outside LDS.

ST_SURFACE_DUMP=<directory>: every case leaves what it observed there (tools/surface_attributes_profile.py --gpu merges it into the profile)."""
import faulthandler
import json
import os

import numpy as np
import pytest
import torch

import surface_families as sf
import surface_ref as sr
from strolle_amd import Aov, Engine, aov_planes
from test_gpu_ray_query import _stream, assert_misses_are_clean, bits, gpu_trace

pytestmark = pytest.mark.gpu

CONFIGS = {
    "exact": dict(exact=True),
    "default": dict(exact=False),
    "no_wide": dict(exact=False, tuning=dict(wide_bvh=0)),
    "no_packets": dict(exact=False, tuning=dict(primary_packets=0)),
}
REBUILD = dict(exact=False, refresh=0)              # ST_BVH_REBUILD; the others run under the library's default, ST_BVH_AUTO
DEVICE_IMAGES = ("placement_device_static", "placement_device_dynamic")
CASES = [(c, k) for c in sf.CASES for k in CONFIGS] + [("transforms_moved", "rebuild")] + [(c, k) for c in DEVICE_IMAGES for k in ("exact", "default")]
FLT_MAX = np.float32(3.4028235e38)
CASE_SECONDS = 120


@pytest.fixture(autouse=True)
def _time_limit():
    """every case under a limit of its own: a case that hangs ends the run with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(CASE_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _table_case(case):
    return "placement_first" if case in DEVICE_IMAGES else case


def _device_images(dynamic, keep):
    """the case's images as device-resident ones, rows 64 B further apart than a row is long"""
    def insert(e, images):
        for h, px in images.items():
            ih, iw = px.shape[:2]
            pitch = iw * 4 + 64
            buf = torch.zeros((ih, pitch), dtype=torch.uint8, device="cuda")
            buf[:, :iw * 4] = torch.from_numpy(px.reshape(ih, iw * 4)).cuda()
            torch.cuda.synchronize()
            keep.append(buf)
            e.insert_device_image(h, buf.data_ptr(), iw, ih, row_pitch_bytes=pitch, dynamic=dynamic)
    return insert


class Run:
    """a case driven through its frames on an engine (every frame rendered), with the planes of the last one"""

    def __init__(self, case, exact, tuning=None, refresh=None):
        self.case, self.keep = case, []
        self.e = e = Engine(device=0, exact=exact)
        if tuning:
            e.set_tuning(**tuning)
        if refresh is not None:
            e.set_bvh_refresh(refresh)
        e.keep_all_planes(True)
        images = _device_images(case.endswith("dynamic"), self.keep) if case in DEVICE_IMAGES else None
        driven = "placement_first" if case in DEVICE_IMAGES else case
        w, h = sf.SIZE
        self.out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        self.ticks = 0
        for self.frame, self.cam in sf.drive(e, driven, images=images):
            self.ticks += 1
            e.render_camera(self.cam, self.out.data_ptr(), _stream())
            torch.cuda.synchronize()
        self.scene = self.frame.scene
        self.rects = {k: e.image_rect(k) for k in self.scene.images}

    def planes(self):
        d0, d1, vel = sf._gbuffer(self.e, self.cam, self.ticks)
        planes = aov_planes(sf.SIZE, fill=12345)
        self.e.render_aovs(self.cam, planes, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        return d0, d1, vel, {k: v.cpu().numpy() for k, v in planes.items()}

    def close(self):
        self.e.close()


def _oracle(case):
    """the oracle's side: tests/surface_families.py oracle_case, driven like Run (every frame rendered)"""
    return sf.oracle_case(_table_case(case))


def _dump(case, config, observed):
    d = os.environ.get("ST_SURFACE_DUMP")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, f"{case}_{config}.json"), "w") as f:
            json.dump(dict(case=case, config=config, observed=observed), f)


def _identity(what, scene, surf, hit, instance, triangle):
    """hit / miss, the instance handle and the mesh triangle equal the definition's on every non-ambiguous ray"""
    sure = surf.ans.margin >= sf.AMBIGUOUS
    bad = sure & (hit != surf.ans.hit)
    assert not bad.any(), f"{what}: {int(bad.sum())} non-ambiguous rays decide hit / miss differently (first rows {np.flatnonzero(bad)[:5]})"
    both = sure & hit
    handles = np.array([h for h, _, _, _, _ in scene.instances], np.uint64)[np.where(both, surf.instance, 0)]
    bad = both & ((instance != handles) | (triangle.astype(np.int64) != surf.triangle))
    assert not bad.any(), f"{what}: {int(bad.sum())} non-ambiguous rays name another instance or triangle (first rows {np.flatnonzero(bad)[:5]})"


def _check_rays(what, run, c, tol, got, rows):
    """one st_scene_trace_rays answer against the definition; returns {quantity: worst deviation / tolerance}"""
    surf, rays = c["surf"], c["rays"]
    assert_misses_are_clean(got)
    full = np.zeros(len(rays), got.dtype); full[rows] = got
    mask = np.zeros(len(rays), bool); mask[rows] = True
    hit = full["hit"] == 1
    _identity(what, run.scene, _take(surf, mask), hit[mask], full["instance"][mask], full["triangle"][mask])
    keep = sf.compared(surf) & mask & hit
    r = sf.judge_geometry(surf, rays, tol, {k: full[k] for k in ("barycentric", "t", "point", "normal", "uv")}, keep)
    print(f"{what}: {int(keep.sum())} rays compared, worst deviation / tolerance {r}")
    assert all(v <= 1.0 for v in r.values()), f"{what}: outside the tolerance: {r}"
    return r


def _take(surf, mask):
    """the rows `mask` of a Surface, for _identity"""
    class View:
        pass
    v = View(); v.ans = View()
    v.ans.margin, v.ans.hit = surf.ans.margin[mask], surf.ans.hit[mask]
    v.instance, v.triangle = surf.instance[mask], surf.triangle[mask]
    return v


@pytest.mark.parametrize("case,config", CASES, ids=[f"{c}-{k}" for c, k in CASES])
def test_surface_attributes_equal_the_definition(case, config):
    opts = REBUILD if config == "rebuild" else CONFIGS[config]
    c = _oracle(case)
    tol = sf.TOLERANCES[_table_case(case)]
    run = Run(case, **opts)
    try:
        e, what = run.e, f"{case} {config}"
        if case == "placement_far":
            assert all(x >= 7168 and y >= 1024 and y + h <= 1536 for x, y, w, h in run.rects.values()), run.rects
        if case == "transforms_moved" and config == "default":
            assert e.device_bakes()[0] >= 1, "the second frame must come from the device bake"
        observed = {}
        # ---- 1. the scene queries
        rays, surf = c["rays"], c["surf"]
        plain = gpu_trace(e, rays)
        packet = gpu_trace(e, rays[:sf.N_BUNDLE], coherent=True)
        observed["trace_rays"] = _check_rays(f"{what} trace_rays", run, c, tol, plain, np.arange(len(rays)))
        observed["coherent"] = _check_rays(f"{what} coherent bundle", run, c, tol, packet, np.arange(sf.N_BUNDLE))
        # ---- 2. the AOVs and the frame's own planes, per pixel
        d0, d1, vel, a = run.planes()
        psurf, pixels = c["psurf"], c["pixels"]
        depth = a[Aov.DEPTH].reshape(-1)
        hit = depth != FLT_MAX
        _identity(f"{what} AOVs", run.scene, psurf, hit, a[Aov.INSTANCE].reshape(-1), a[Aov.TRIANGLE].reshape(-1))
        sky = ~hit
        assert not a[Aov.NORMAL].reshape(-1, 4)[sky].any() and not a[Aov.ALBEDO].reshape(-1, 4)[sky].any() and not a[Aov.MOTION].reshape(-1, 2)[sky].any()
        assert not a[Aov.INSTANCE].reshape(-1)[sky].any() and np.all(a[Aov.TRIANGLE].reshape(-1)[sky] == 0xFFFFFFFF)
        pk = sf.compared(psurf) & hit
        assert pk.mean() >= 0.1, "the camera must see the scene"
        r = sf.judge_geometry(psurf, pixels, dict(normal=tol["normal"], depth=tol["depth"]), dict(normal=a[Aov.NORMAL].reshape(-1, 4)[:, :3], depth=depth), pk)
        r["albedo"] = sf.judge_channels(run.scene, psurf, run.rects, tol, a[Aov.ALBEDO].reshape(-1, 4), pk)
        mvel, mamb = c["motion"]
        r["motion"] = sf.ratio(np.abs(a[Aov.MOTION].reshape(-1, 2).astype(np.float64) - mvel)[pk & ~mamb], tol["motion"])
        print(f"{what} AOVs: {int(pk.sum())} pixels compared, worst deviation / tolerance {r}")
        assert all(v <= 1.0 for v in r.values()), f"{what} AOVs: outside the tolerance: {r}"
        observed["aovs"] = r
        assert np.array_equal(bits(vel[:, :2]), bits(a[Aov.MOTION].reshape(-1, 2))), f"{what}: the velocity plane differs from ST_AOV_MOTION"
        if case == "motion_static":
            assert not vel.any(), "nothing moved: every pixel's velocity is exactly 0"
        # ---- 3. the G-buffer of the frame on screen
        g = sr.decode_gbuffer(d0, d1)
        assert np.array_equal(np.any(d0 != 0, axis=1), hit)
        assert np.array_equal(bits(depth[hit]), bits(d0[:, 0][hit])), f"{what}: ST_AOV_DEPTH differs from the G-buffer's depth"
        r = {"gbuffer_" + k: v for k, v in sf.judge_geometry(psurf, pixels, dict(normal=tol["gbuffer_normal"], depth=tol["gbuffer_depth"]),
                                                             dict(normal=g["normal"], depth=g["depth"]), pk).items()}
        r["gbuffer_emissive"] = sf.judge_channels(run.scene, psurf, run.rects, tol, g["emissive"], pk, first=4)
        codes = sf.judge_codes(run.scene, psurf, run.rects, tol, g, pk)
        print(f"{what} G-buffer: worst deviation / tolerance {r}, codes outside one code of the definition's {codes}")
        assert all(v <= 1.0 for v in r.values()), f"{what} G-buffer: outside the tolerance: {r}"
        assert max(codes.values()) == 0, f"{what}: the G-buffer's quantised fields are {codes} codes outside one code of the definition's"
        observed["gbuffer"] = r
        # ---- 4. the exact build equals the oracle bit for bit wherever the oracle has the value
        if opts["exact"]:
            probe = sf.probe_fields(c["probe"])
            ohit = probe["t"] < FLT_MAX
            assert np.array_equal(plain["hit"] == 1, ohit), f"{what}: hit / miss differs from the oracle"
            for f in ("t", "point", "normal", "uv", "barycentric"):
                same = np.all(bits(plain[f]).reshape(len(rays), -1)[ohit] == bits(np.ascontiguousarray(probe[f])).reshape(len(rays), -1)[ohit], axis=1)
                assert same.all(), f"{what}: {f} differs from the oracle on {int((~same).sum())} rays (first {np.flatnonzero(~same)[:5]})"
            assert np.array_equal(bits(packet["t"]), bits(plain["t"][:sf.N_BUNDLE])) and np.array_equal(bits(packet["normal"]), bits(plain["normal"][:sf.N_BUNDLE]))
            assert np.array_equal(bits(d0), bits(c["d0"])) and np.array_equal(bits(d1), bits(c["d1"])), f"{what}: the G-buffer differs from the oracle's"
            assert np.array_equal(bits(vel[:, :2]), bits(c["velocity"])), f"{what}: the velocity plane differs from the oracle's"
            pp = sf.probe_fields(c["pixel_probe"])
            assert np.array_equal(bits(a[Aov.ALBEDO].reshape(-1, 4)[hit]), bits(np.ascontiguousarray(pp["base_color"][hit]))), f"{what}: ALBEDO differs from the oracle's base colour"
            assert np.array_equal(bits(a[Aov.NORMAL].reshape(-1, 4)[:, :3][hit]), bits(np.ascontiguousarray(pp["normal"][hit])))
            assert np.array_equal(bits(depth[hit]), bits(np.ascontiguousarray(pp["depth"][hit])))
        _dump(case, config, observed)
    finally:
        run.close()


def test_undefined_normals_are_the_same_non_finite_rays_in_both_builds():
    """flat_degenerate's cancelling and all-zero vertex normals: nothing is owed on those rays but that the fast build and the exact build (which equals the
    oracle bit for bit, above) agree on WHICH of them are non-finite"""
    c = _oracle("flat_degenerate")
    und = c["surf"].undefined
    assert und.sum() > 100
    answers = []
    for config in ("exact", "default", "no_wide"):
        run = Run("flat_degenerate", **CONFIGS[config])
        try:
            answers.append(gpu_trace(run.e, c["rays"]))
        finally:
            run.close()
    finite = [np.all(np.isfinite(g["normal"]), axis=1) for g in answers]
    assert (~finite[0][und]).sum() > 10, "the all-zero normals normalise to NaN in the contract (glam normalize)"
    for f, config in zip(finite[1:], ("default", "no_wide")):
        assert np.array_equal(f[und], finite[0][und]), f"{config}: {int((f[und] != finite[0][und]).sum())} undefined rays are finite in one build and not in the other"
        assert np.all(f[~und]), f"{config}: a defined normal is not finite"


@pytest.mark.parametrize("config", ["exact", "default"])
def test_the_atlas_histories_give_the_same_pixels(config):
    """placement: first into an empty atlas, far out in a tall one, between live neighbours over stale texels, as a static and as a dynamic device-resident
    image — the non-border samples of ALBEDO and of the ray queries' uv agree within the two histories' tolerances"""
    histories = [f"placement_{h}" for h in sf.HISTORIES] + list(DEVICE_IMAGES)
    c = _oracle("placement_first")
    psurf = c["psurf"]
    albedo, allowed = {}, {}
    for case in histories:
        run = Run(case, **CONFIGS[config])
        try:
            _, _, _, a = run.planes()
            albedo[case] = a[Aov.ALBEDO].reshape(-1, 4).astype(np.float64)
            allowed[case] = sf.channel_tolerance(sf.TOLERANCES[_table_case(case)], psurf, sf.texel_delta(run.scene, psurf, run.rects))[:, :4]
        finally:
            run.close()
    keep = sf.compared(psurf)
    worst = {}
    for case in histories[1:]:
        worst[case] = sf.ratio(np.abs(albedo[case] - albedo[histories[0]])[keep], (allowed[case] + allowed[histories[0]])[keep])
    print(f"{config}: first against the other histories, worst difference / the two tolerances: {worst}")
    assert all(v <= 1.0 for v in worst.values()), worst
    _dump("placement_histories", config, worst)
