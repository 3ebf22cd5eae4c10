"""Normal mapping (include/strolle_hip.h "normal mapping") on the GPU, both builds, over the cases of tests/normal_map_cases.py.

  the function   st_scene_trace_rays with ST_RAY_MAPPED_NORMAL against the float32 restatement normal_map_ref.map_f32, fed the SAME engine's unflagged
                 normal and uv, read_scene's records and rectangles and the image bytes: identical bits. Against the float64 definition map_f64:
                 within normal_map_cases.TOLERANCES, which the CPU measured. Every other StRayHit field: identical with and without the flag.
  the frame      with the switch on, the G-buffer's octahedral code, the surface map, ST_AOV_NORMAL and st_camera_pick against the flagged query over
                 the camera's own rays
  off is off     the switch on without a mapped material, and the switch off with mapped materials: every plane, the composed frame, the ray count,
                 the six AOVs and the launch list are an untouched engine's bit for bit, over 8 frames; a removed image returns the frame to unmapped bits
  what moves     moved instances under every refresh mode, the device-built tree, a re-posed skinned tube and a morphed one: the flagged query follows
                 the restatement on the re-read records
  properties     unit length, no NaN, the ray's side of the tangent plane; a lit quad whose map tilts one half towards the light is brighter there
  scheduling     the switch toggled with eight frames in flight on one and on two streams; 2 and 4 tiles; destroy with the switch on

The decoded-surface plane `sn` is not readable through st_camera_read_buffer; the kernel writes normal_decode of the very code the surface map and the
G-buffer hold, and those two are compared."""
import faulthandler

import numpy as np
import pytest
import torch

import normal_map_cases as nc
import surface_families as sf
import surface_ref as sr
from strolle_amd import Aov, Buffer, Engine, Instance, Light, Material, Mesh, Sun, aov_planes, scenes
from strolle_amd.api import HIT_DTYPE
from test_gpu_ray_query import _dev, _stream, bits, gpu_pick

pytestmark = pytest.mark.gpu

BUILDS = {"exact": True, "default": False}
CASE_SECONDS = 120
F = np.float32


@pytest.fixture(autouse=True)
def _time_limit():
    """every case under a limit of its own: a case that hangs ends the run with a traceback instead of holding the device"""
    faulthandler.dump_traceback_later(CASE_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def trace(e, rays, mapped=False, coherent=False):
    d_rays = _dev(rays)
    d_hits = torch.full((len(rays) * HIT_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device="cuda")
    e.trace_rays(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), coherent=coherent, stream=_stream(), mapped_normal=mapped)
    torch.cuda.synchronize()
    return d_hits.cpu().numpy().view(HIT_DTYPE)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_but_normal(a, b, what):
    for f in HIT_DTYPE.names:
        if f != "normal":
            assert np.array_equal(raw(a[f]), raw(b[f])), f"{what}: StRayHit.{f} differs between the flagged and the unflagged call"


def slots_of(scene, hits):
    """the winning triangle slot of every hit (0 on a miss)"""
    first = nc.first_slots(scene)
    table = np.zeros(int(max(first) + 1), np.int64)
    for h, v in first.items():
        table[h] = v
    hit = hits["hit"] == 1
    return np.where(hit, table[np.where(hit, hits["instance"], 0).astype(np.int64)] + hits["triangle"].astype(np.int64), 0)


def restated(e, scene, rays, plain, rects=None):
    """map_f32 on what engine e itself reports: (n' float32 [n,3], mapped [n], border [n])"""
    rects = rects or {h: e.image_rect(h) for h in scene.images}
    return nc.restate(scene, rays, plain["hit"] == 1, np.ascontiguousarray(plain["normal"]), np.ascontiguousarray(plain["uv"]), slots_of(scene, plain),
                      e.read_scene(1), e.read_scene(3), rects)


def assert_bits(got, want, rows, what):
    bad = rows & np.any(bits(got) != bits(want), axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {int(rows.sum())} normals differ in bits from the restatement (first rows {np.flatnonzero(bad)[:5]}: " \
                          f"{got[bad][:2]} against {want[bad][:2]})"


def check_function(e, case, what, coherent=False):
    """the flagged query against the restatement (bits) and against the definition (tolerance); returns the worst deviation / tolerance"""
    c = nc.reference(case)
    scene, rays, surf, mapped = c["scene"], c["rays"], c["surf"], c["mapped"]
    plain, flagged = trace(e, rays, coherent=coherent), trace(e, rays, mapped=True, coherent=coherent)
    same_but_normal(plain, flagged, what)
    hit = plain["hit"] == 1
    want, was_mapped, border = restated(e, scene, rays, plain)
    assert_bits(flagged["normal"], want, hit & ~border, what)
    # a material without a map, and every degenerate layout: the two calls agree in every bit
    untouched = hit & ~was_mapped
    assert np.array_equal(bits(flagged["normal"][untouched]), bits(plain["normal"][untouched])), f"{what}: an unmapped hit's normal changed"
    assert (hit & was_mapped & np.any(bits(flagged["normal"]) != bits(plain["normal"]), axis=1)).sum() >= 0.1 * len(rays), f"{what}: the map changed too few normals"
    keep = nc.compared(surf, mapped) & hit
    dev = sf.angle(flagged["normal"][keep], mapped.normal[keep])
    allowed = nc.allowed(case, scene, surf, mapped, {h: e.image_rect(h) for h in scene.images})[keep]
    r = sf.ratio(dev, allowed)
    print(f"{what}: {int(keep.sum())} rays compared with the definition, worst angle {dev.max(initial=0.0):.3e} rad, worst deviation / tolerance {r:.3f}; "
          f"{int((hit & ~border).sum())} rays bit-equal to the restatement, {int((hit & border).sum())} border samples left out")
    assert r <= 1.0, f"{what}: outside the tolerance: {r}"
    # properties that do not rest on the restatement
    n = flagged["normal"][hit].astype(np.float64)
    defined = np.all(np.isfinite(plain["normal"][hit]), axis=1)
    assert np.all(np.isfinite(n[defined])), f"{what}: a mapped normal is not finite"
    assert np.abs(np.linalg.norm(n[defined], axis=1) - 1.0).max() <= 1e-6, f"{what}: a mapped normal is not of unit length"
    side = np.einsum("ij,ij->i", n, plain["normal"][hit].astype(np.float64))
    assert np.all(side[defined] >= -1e-6), f"{what}: a mapped normal points to the far side of the tangent plane"
    return r


def engine_for(case, exact, on=False, refresh=None, images=None, tuning=None):
    e = Engine(device=0, exact=exact)
    if tuning:
        e.set_tuning(**tuning)
    if refresh is not None:
        e.set_bvh_refresh(refresh)
    e.keep_all_planes(True)
    if on:
        e.set_normal_mapping(True)
    cam = nc.drive(e, case, images=images)
    return e, cam


# ----------------------------------------------------------------------------- the function
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("case", nc.CASES)
def test_the_flagged_query_is_the_restatement_bit_for_bit(case, build):
    e, _ = engine_for(case, BUILDS[build])
    try:
        assert e.get_normal_mapping() is False                     # the flag does not ask the switch
        check_function(e, case, f"{case} {build}")
    finally:
        e.close()


@pytest.mark.parametrize("build", BUILDS)
def test_coherent_rays_and_the_switch_change_nothing_of_the_flagged_query(build):
    e, _ = engine_for("transforms", BUILDS[build], on=True)
    try:
        rays = nc.reference("transforms")["rays"]
        a = trace(e, rays, mapped=True)
        check_function(e, "transforms", f"transforms {build} ST_RAY_COHERENT", coherent=True)   # (the packet walk may pick the other of two tied triangles: held on its own answers)
        if BUILDS[build]:                                                                      # the exact build walks the contract stream either way
            assert np.array_equal(raw(a), raw(trace(e, rays, mapped=True, coherent=True)))
        e.set_normal_mapping(False)
        assert np.array_equal(raw(a), raw(trace(e, rays, mapped=True))), "the engine's switch changed a flagged query"
    finally:
        e.close()


def test_a_dynamic_device_image_is_a_map():
    keep = []

    def insert(e, images):
        for h, px in images.items():
            ih, iw = px.shape[:2]
            pitch = iw * 4 + 64
            buf = torch.zeros((ih, pitch), dtype=torch.uint8, device="cuda")
            buf[:, :iw * 4] = torch.from_numpy(px.reshape(ih, iw * 4)).cuda()
            torch.cuda.synchronize()
            keep.append(buf)
            e.insert_device_image(h, buf.data_ptr(), iw, ih, row_pitch_bytes=pitch, dynamic=True)

    e, _ = engine_for("texel_grid", False, images=insert)
    try:
        check_function(e, "texel_grid", "texel_grid default, dynamic device images")
    finally:
        e.close()


# ----------------------------------------------------------------------------- the frame
def encode32(n):
    """st_traverse.h normal_encode_exact (= st_device.h normal_encode without contraction or a reciprocal) in float32"""
    n = np.ascontiguousarray(n, F)
    s = (np.abs(n[:, 0]) + np.abs(n[:, 1])) + np.abs(n[:, 2])
    with np.errstate(all="ignore"):
        m = n / s[:, None]
    rx = np.where(m[:, 2] >= 0, m[:, 0], np.copysign(F(1.0) - np.abs(m[:, 1]), m[:, 0]))
    ry = np.where(m[:, 2] >= 0, m[:, 1], np.copysign(F(1.0) - np.abs(m[:, 0]), m[:, 1]))
    return np.stack([rx * F(0.5) + F(0.5), ry * F(0.5) + F(0.5)], 1).astype(F)


def render(e, cam, frames=1):
    w, h = sf.SIZE
    out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    for k in range(frames):
        if k:
            e.tick()
        e.render_camera(cam, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("case", ["sphere80", "transforms", "uv_layouts"])
def test_the_frame_carries_the_flagged_query(case, build):
    exact = BUILDS[build]
    c = nc.reference(case)
    pixels, scene = c["pixels"], c["scene"]
    e, cam = engine_for(case, exact, on=True)
    try:
        render(e, cam)
        d0, d1, _ = sf._gbuffer(e, cam, 1)
        sm = e.read_buffer(cam, Buffer.PRIM_SURFACE_MAP_B).reshape(-1, 4)
        planes = aov_planes(sf.SIZE, fill=12345)
        e.render_aovs(cam, planes, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        aov = planes[Aov.NORMAL].cpu().numpy().reshape(-1, 4)
        # the comparison target: the flagged query over the camera's own rays; exact leaf test, as primary visibility and the AOVs walk
        q = trace(e, pixels, mapped=True, coherent=True)
        plain = trace(e, pixels, coherent=True)
        hit = q["hit"] == 1
        assert hit.mean() >= 0.1 and np.array_equal(hit, np.any(d0 != 0, axis=1))
        changed = hit & np.any(bits(q["normal"]) != bits(plain["normal"]), axis=1)
        assert changed.sum() >= 0.3 * hit.sum(), "the map must bend much of what the camera sees"   # (uv_layouts: two quads of five are mapped)
        assert np.array_equal(bits(sm[:, :2]), bits(d0[:, 1:3])), "the surface map and the G-buffer hold different codes of the normal"
        xy = np.stack([np.arange(len(pixels)) % sf.SIZE[0], np.arange(len(pixels)) // sf.SIZE[0]], 1).astype(np.uint32)
        pick = gpu_pick(e, cam, xy)
        if exact:
            assert np.array_equal(bits(aov[:, :3][hit]), bits(q["normal"][hit])), f"{case} exact: ST_AOV_NORMAL differs from the flagged query"
            assert np.array_equal(bits(d0[:, 1:3][hit]), bits(encode32(q["normal"][hit]))), f"{case} exact: the G-buffer's code is not the flagged query's normal encoded"
            assert np.array_equal(bits(pick["normal"][hit]), bits(q["normal"][hit])), f"{case} exact: st_camera_pick differs from the flagged query"
        else:
            # the fast build resolves primary hits, picks and queries with differently contracted arithmetic (an ulp apart before this feature too): the
            # frame's outputs lie within the case's recorded tolerance of the flagged query
            allowed = nc.allowed(case, scene, c["psurf"], c["pmapped"], {h: e.image_rect(h) for h in scene.images})
            keep = hit & nc.compared(c["psurf"], c["pmapped"])
            g = sr.decode_gbuffer(d0, d1)["normal"]
            r = {"aov": sf.ratio(sf.angle(aov[:, :3][keep], q["normal"][keep]), allowed[keep]),
                 "gbuffer": sf.ratio(sf.angle(g[keep], q["normal"][keep]), allowed[keep]),
                 "pick": sf.ratio(sf.angle(pick["normal"][keep], q["normal"][keep]), allowed[keep])}
            print(f"{case} default: {int(keep.sum())} pixels, frame outputs against the flagged query, worst deviation / tolerance {r}")
            assert all(v <= 1.0 for v in r.values()), r
        # ST_AOV_NORMAL is the frame's own normal: its code is the G-buffer's wherever primary visibility encodes exactly (always, but the fast build's LDS scenes)
        if exact or case == "transforms":
            assert np.array_equal(bits(encode32(aov[:, :3][hit])), bits(d0[:, 1:3][hit])), f"{case} {build}: ST_AOV_NORMAL encoded is not the G-buffer's code"
        # the switch off again: the very next calls are unmapped
        e.set_normal_mapping(False)
        e.render_aovs(cam, planes, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        off = planes[Aov.NORMAL].cpu().numpy().reshape(-1, 4)
        assert (np.any(bits(off[:, :3]) != bits(aov[:, :3]), axis=1)).sum() >= 0.3 * hit.sum()
        unmapped_pick = gpu_pick(e, cam, xy)
        if exact:
            assert np.array_equal(bits(unmapped_pick["normal"][hit]), bits(trace(e, pixels)["normal"][hit])), "a pick with the switch off is mapped"
        # the pick in bits, in both builds: its own unmapped answer through the restatement is its mapped answer (a pick walks with k_ref_tracing's leaf
        # test, which in the fast build is not the query's: its barycentrics may differ from the query's by an ulp, its own two answers may not)
        same_but_normal(unmapped_pick, pick, f"{case} {build} pick")
        phit = unmapped_pick["hit"] == 1
        want, _, border = restated(e, scene, pixels, unmapped_pick)
        assert_bits(pick["normal"], want, phit & ~border, f"{case} {build} pick, switch on against its own unmapped answer")
    finally:
        e.close()


# ----------------------------------------------------------------------------- off is off
PLANES = [b for b in Buffer]


def observe(e, cam, frames=8):
    """everything a run of `frames` frames leaves: the composed frames, every plane of the last one, the ray count, the six AOVs, the launch list"""
    w, h = sf.SIZE
    out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    composed, launches = [], []
    for k in range(frames):
        if k:
            e.tick()
        e.render_camera(cam, out.data_ptr(), _stream())
        torch.cuda.synchronize()
        composed.append(out.cpu().numpy().copy()); launches.append(tuple(e.last_launches()))
    planes = aov_planes(sf.SIZE, fill=12345)
    e.render_aovs(cam, planes, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    return dict(composed=composed, launches=launches, rays=e.ray_count(cam), planes={b.name: e.read_buffer(cam, b).copy() for b in PLANES},
                aovs={k.name: v.cpu().numpy().copy() for k, v in planes.items()})


def assert_same_run(a, b, what):
    assert a["launches"] == b["launches"], f"{what}: the launch list changed"
    assert a["rays"] == b["rays"], f"{what}: the ray count changed"
    for k, (x, y) in enumerate(zip(a["composed"], b["composed"])):
        assert np.array_equal(bits(x), bits(y)), f"{what}: frame {k} differs"
    for name in a["planes"]:
        assert np.array_equal(a["planes"][name].view(np.uint32), b["planes"][name].view(np.uint32)), f"{what}: plane {name} differs"
    for name in a["aovs"]:
        assert np.array_equal(raw(a["aovs"][name]), raw(b["aovs"][name])), f"{what}: ST_AOV_{name} differs"


def _unmapped_scene(case):
    import copy
    s = copy.deepcopy(nc.scene_of(case)[0])
    for m in s.materials.values():
        m.normal_map_texture = None
    return s


@pytest.mark.parametrize("build", BUILDS)
def test_off_is_off(build):
    exact = BUILDS[build]
    case = "texel_grid"

    def run(scene, switch):
        e = Engine(device=0, exact=exact)
        try:
            e.keep_all_planes(True); e.set_seed(11)
            if switch is not None:
                e.set_normal_mapping(switch)
            cam = nc.drive(e, case, scene=scene)
            return observe(e, cam)
        finally:
            e.close()

    plain_scene = _unmapped_scene(case)
    untouched = run(plain_scene, None)
    assert_same_run(untouched, run(plain_scene, True), f"{build}: the switch on without a mapped material")
    mapped_untouched = run(None, None)
    assert_same_run(mapped_untouched, run(None, False), f"{build}: the switch off with mapped materials")
    # the map is not in the picture while the switch is off: mapped materials render what unmapped ones do
    assert_same_run(untouched, mapped_untouched, f"{build}: mapped materials with the switch off against unmapped ones")
    on = run(None, True)
    assert on["launches"] == untouched["launches"], "the launch list changed with the switch on"
    assert not np.array_equal(on["aovs"]["NORMAL"], untouched["aovs"]["NORMAL"]), "the switch on with mapped materials must change the NORMAL AOV"


def test_a_removed_image_returns_the_frame_to_unmapped_bits():
    case = "sphere80"
    e, cam = engine_for(case, True, on=True)
    ref, rcam = engine_for(case, True)
    try:
        e.set_seed(5); ref.set_seed(5)
        render(e, cam); render(ref, rcam)
        mapped_d0 = sf._gbuffer(e, cam, 1)[0]
        assert not np.array_equal(bits(mapped_d0), bits(sf._gbuffer(ref, rcam, 1)[0]))
        e.remove_image(nc.MAP_IMAGE); ref.remove_image(nc.MAP_IMAGE)
        e.tick(); ref.tick()
        a, b = render(e, cam), render(ref, rcam)
        for x, y in zip(sf._gbuffer(e, cam, 2), sf._gbuffer(ref, rcam, 2)):
            assert np.array_equal(bits(x), bits(y)), "a frame after the map's image is gone differs from the unmapped engine's"
        rays = nc.reference(case)["rays"]
        assert np.array_equal(raw(trace(e, rays, mapped=True)), raw(trace(e, rays))), "a handle whose image is gone still maps"
    finally:
        e.close(); ref.close()


# ----------------------------------------------------------------------------- everything that moves geometry
def moved_scene(k):
    """the `transforms` scene with every instance at another rotation, scale and place"""
    import copy
    s = copy.deepcopy(nc.scene_of("transforms")[0])
    s.instances = [(h, mesh, mat, sf._retransformed(x, i + k), x) for i, (h, mesh, mat, x, _) in enumerate(s.instances)]
    return s


def hold_to_restatement(e, scene, rays, what):
    plain, flagged = trace(e, rays), trace(e, rays, mapped=True)
    same_but_normal(plain, flagged, what)
    hit = plain["hit"] == 1
    want, was_mapped, border = restated(e, scene, rays, plain)
    assert (hit & was_mapped & ~border).sum() >= 0.1 * len(rays), f"{what}: too few mapped hits"
    assert_bits(flagged["normal"], want, hit & ~border, what)


@pytest.mark.parametrize("mode,build", [(4, "default"), (2, "default"), (0, "default"), (3, "default"), (0, "exact"), (2, "exact")],
                         ids=["auto", "refit_device", "rebuild", "build_device", "rebuild-exact", "refit_device-exact"])
def test_moved_instances_keep_their_mapped_normals(mode, build):
    e, _ = engine_for("transforms", BUILDS[build], refresh=mode)
    try:
        rays = nc.reference("transforms")["rays"]
        hold_to_restatement(e, nc.scene_of("transforms")[0], rays, f"mode {mode} {build}, first tick")
        for k in (1, 2):
            s = moved_scene(k)
            for h, mesh, mat, x, _ in s.instances:
                e.insert_instance(h, Instance(mesh, mat, x))
            e.tick()
            hold_to_restatement(e, s, rays, f"mode {mode} {build}, move {k}")
    finally:
        e.close()


TUBE = 7000


def tube_engine(exact):
    mesh, jt, wt = scenes.skinned_tube(8, 6, 4, length=1.2)
    e = Engine(device=0, exact=exact)
    e.set_blue_noise(scenes.load_blue_noise())
    e.insert_image(nc.MAP_IMAGE, sf.every_byte_image())
    e.insert_material(TUBE, Material(base_color=(0.6, 0.6, 0.6, 1.0), normal_map_texture=nc.MAP_IMAGE))
    uv = (0.1 + 0.8 * mesh.uvs.astype(np.float64)).astype(np.float32)        # every tap inside the 16 x 16 map
    mesh = Mesh(mesh.positions, mesh.normals, uv)
    e.insert_mesh(TUBE, mesh)
    e.insert_instance(TUBE, Instance(TUBE, TUBE, sf.translate(0.0, 0.0)))
    e.update_sun(Sun(azimuth=0.0, altitude=-1.0))
    scene = sr.Scene(meshes={TUBE: (mesh.positions, mesh.normals, mesh.uvs)}, materials={TUBE: Material(normal_map_texture=nc.MAP_IMAGE)},
                     images={nc.MAP_IMAGE: sf.every_byte_image()}, instances=[(TUBE, TUBE, TUBE, sf.translate(0.0, 0.0), sf.translate(0.0, 0.0))])
    return e, mesh, jt, wt, scene


def rays_at(e, n, seed):
    """rays at interior points of the engine's own world triangles, from either side"""
    tri = e.read_scene(1).view(np.float32).reshape(-1, 9, 4)[:, [0, 3, 6], :3].astype(np.float64)
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(tri), n)
    bu, bv = rng.uniform(0.1, 0.45, n), rng.uniform(0.1, 0.45, n)
    p0, e1, e2 = tri[pick, 0], tri[pick, 1] - tri[pick, 0], tri[pick, 2] - tri[pick, 0]
    nrm = np.cross(e1, e2); area = np.linalg.norm(nrm, axis=1, keepdims=True); nrm /= area
    return sf._aim(p0 + bu[:, None] * e1 + bv[:, None] * e2, nrm, rng, np.sqrt(area) * 3.0)


@pytest.mark.parametrize("build", BUILDS)
def test_a_reposed_skinned_tube_keeps_its_mapped_normals(build):
    e, mesh, jt, wt, scene = tube_engine(BUILDS[build])
    try:
        e.set_skin(TUBE, jt, wt, 4)
        e.tick()
        for k in range(3):
            e.set_pose(TUBE, scenes.bend_pose(4, 1.6, 0.7 * k, length=1.2))
            e.tick()
            hold_to_restatement(e, scene, rays_at(e, 1024, 40 + k), f"skinned tube {build}, pose {k}")
    finally:
        e.close()


@pytest.mark.parametrize("build", BUILDS)
def test_a_morphed_tube_keeps_its_mapped_normals(build):
    e, mesh, jt, wt, scene = tube_engine(BUILDS[build])
    try:
        dp, dn = scenes.tube_morph_targets(mesh, length=1.2)
        e.set_morph_targets(TUBE, dp, dn)
        e.tick()
        for k, w in enumerate(([0.0, 0.0, 0.0], [0.8, 0.1, 0.0], [0.2, 0.9, 0.4])):
            e.set_morph_weights(TUBE, w)
            e.tick()
            hold_to_restatement(e, scene, rays_at(e, 1024, 50 + k), f"morphed tube {build}, weights {k}")
    finally:
        e.close()


# ----------------------------------------------------------------------------- a property of the picture
def test_a_map_tilted_towards_the_light_is_brighter():
    """One 4 x 4 quad facing +z under one point light above its centre, seen from straight above: with the switch off the picture is symmetric in x. The
    map tilts the normal towards +x everywhere: on the left half (x < 0) that is towards the light, on the right half away from it. After 32
    Image{denoise} frames the left half's mean luminance must exceed the right's with the switch on.
    With the switch off the halves must agree within the frame's own noise. That noise is measured, not guessed: d = (left - right) / (left + right),
    averaged over the last 8 frames, is taken from six runs that differ only in their seed, and sigma is the standard deviation of the six. The halves
    agree when the median d lies within 3 sigma of zero; the map shows when every on-run d exceeds 10 sigma."""
    size = sf.SIZE
    img = np.zeros((8, 8, 4), np.uint8); img[..., 3] = 255
    img[..., :3] = (208, 128, 200)
    p, n, uv = sf.quad()
    p = (p.astype(np.float64) * 4.0 - [2.0, 2.0, 0.0]).astype(np.float32)

    def run(on, seed):
        e = Engine(device=0)
        try:
            e.set_blue_noise(scenes.load_blue_noise()); e.set_seed(seed)
            e.insert_image(nc.MAP_IMAGE, img)
            e.insert_material(1, Material(base_color=(0.8, 0.8, 0.8, 1.0), perceptual_roughness=1.0, reflectance=0.0, normal_map_texture=nc.MAP_IMAGE))
            e.insert_mesh(1, Mesh(p, n, uv))
            e.insert_instance(1, Instance(1, 1, sf.translate(0.0, 0.0)))
            e.insert_light(1, Light.point((0.0, 0.0, 3.0), 0.1, (1.0, 1.0, 1.0), 400.0))
            e.update_sun(Sun(azimuth=0.0, altitude=-1.0))
            e.set_normal_mapping(on)
            cam = e.create_camera(sf.camera_over((-2.0, -2.0), (2.0, 2.0), eye_offset=(0.0, 0.0)))
            out = torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda")
            d = []
            for k in range(32):
                e.tick()
                e.render_camera(cam, out.data_ptr(), _stream())
                if k >= 24:
                    torch.cuda.synchronize()
                    lum = out.cpu().numpy()[..., :3] @ np.array([0.2126, 0.7152, 0.0722])
                    w = size[0]
                    left, right = lum[12:36, w // 2 - 14:w // 2 - 2].mean(), lum[12:36, w // 2 + 2:w // 2 + 14].mean()
                    assert left > 0 and right > 0, "the quad must be lit"
                    d.append((left - right) / (left + right))
            return float(np.mean(d))
        finally:
            e.close()

    seeds = (3, 4, 5, 6, 7, 8)
    off = np.array([run(False, s) for s in seeds]); on = np.array([run(True, s) for s in seeds[:3]])
    sigma = float(off.std(ddof=1))
    print(f"relative left - right luminance, mean of the last 8 of 32 frames: off {np.round(off, 5).tolist()} (sigma over six seeds {sigma:.5f}), on {np.round(on, 5).tolist()}")
    assert sigma > 0.0
    assert abs(float(np.median(off))) <= 3.0 * sigma, "with the switch off the halves differ by more than the frame's own noise"
    assert on.min() > 10.0 * sigma and on.min() > 0.0, "with the switch on the half tilted towards the light must be the brighter one, far above the noise"


# ----------------------------------------------------------------------------- lifecycle and scheduling
@pytest.mark.parametrize("streams", [1, 2])
def test_the_switch_toggled_with_frames_in_flight(streams):
    """eight frames enqueued without a host join, the switch flipped before each: every frame is the frame a joined engine renders with that setting"""
    case = "transforms"
    w, h = sf.SIZE
    ss = [torch.cuda.Stream() for _ in range(streams)]

    def frames(join):
        e, cam = engine_for(case, False)
        try:
            e.set_seed(9)
            outs = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(8)]
            torch.cuda.synchronize()
            for k in range(8):
                s = ss[k % streams]
                e.set_normal_mapping(k % 3 != 0)
                if k:
                    e.tick(s.cuda_stream)
                e.render_camera(cam, outs[k].data_ptr(), s.cuda_stream)
                if join:
                    torch.cuda.synchronize()
            torch.cuda.synchronize()
            d0 = sf._gbuffer(e, cam, 8)[0]
            return [o.cpu().numpy() for o in outs], d0
        finally:
            e.close()

    (a, ga), (b, gb) = frames(False), frames(True)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(bits(x), bits(y)), f"{streams} stream(s): frame {k} in flight differs from the joined run's"
    assert np.array_equal(bits(ga), bits(gb))


@pytest.mark.parametrize("world", [2, 4])
def test_tiles_equal_one_frame_with_maps_on(world):
    """st_dist_init_local ranks with the switch on. A composed Image frame gathered from apron-less tiles is not the single engine's at any commit (the
    denoiser's taps cross tile borders); what normal mapping writes is per pixel: each rank's G-buffer and surface map inside its own tile are the single
    engine's bit for bit, with the gather running."""
    case = "transforms"
    size = sf.SIZE
    stream = torch.cuda.current_stream().cuda_stream
    one, cam = engine_for(case, False, on=True)
    ranks = []
    try:
        single = torch.zeros((size[1], size[0], 4), dtype=torch.float32, device="cuda")
        for r in range(world):
            e, c = engine_for(case, False, on=True)
            e.dist_init_local(r, world, 7700 + world)
            owned, _ = e.dist_set_partition(c, apron=0)
            ranks.append((e, c, torch.zeros_like(single), owned))
        full = torch.zeros_like(single)
        one.render_camera(cam, single.data_ptr(), stream)
        for r in range(world - 1, -1, -1):   # in-process transport: rank 0 last
            e, c, out, _ = ranks[r]
            e.render_camera(c, out.data_ptr(), stream)
            e.dist_gather(c, out.data_ptr(), full.data_ptr() if r == 0 else 0, stream)
        ranks[0][0].dist_wait(ranks[0][1], host=True)
        torch.cuda.synchronize()
        gathered = full.cpu().numpy()
        for e, c, out, (x0, y0, x1, y1) in ranks:      # the gathered frame is the ranks' tiles, bit for bit
            assert np.array_equal(bits(gathered[y0:y1, x0:x1]), bits(out.cpu().numpy()[y0:y1, x0:x1])), f"{world} tiles: the gathered frame is not a rank's tile"
        assert np.any(gathered[..., :3] != 0)
        for b in (Buffer.PRIM_GBUFFER_D0_B, Buffer.PRIM_GBUFFER_D1_B, Buffer.PRIM_SURFACE_MAP_B):
            want = one.read_buffer(cam, b).reshape(size[1], size[0], 4)
            assert np.any(want != 0)
            for e, c, _, (x0, y0, x1, y1) in ranks:
                got = e.read_buffer(c, b).reshape(size[1], size[0], 4)
                assert np.array_equal(bits(got[y0:y1, x0:x1]), bits(want[y0:y1, x0:x1])), f"{world} tiles: {b.name} of a tile differs from the single engine's"
    finally:
        for e, *_ in ranks:
            e.dist_shutdown(); e.close()
        one.close()


def test_destroy_with_the_switch_on_and_frames_in_flight():
    e, cam = engine_for("sphere80", False, on=True)
    w, h = sf.SIZE
    out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    for _ in range(3):
        e.tick(); e.render_camera(cam, out.data_ptr(), _stream())
    e.close()
    torch.cuda.synchronize()
    assert np.isfinite(out.cpu().numpy()).all()
