"""The scenes normal mapping (include/strolle_hip.h "normal mapping") is held to tests/normal_map_ref.py on; shared by tests/test_normal_map_abi.py (CPU: the
restatement against the definition — this is where TOLERANCES comes from) and tests/test_gpu_normal_map.py (GPU: both builds against both).

A case is one scene as the caller states it (surface_ref.Scene, normal maps on its materials), a 64 x 48 camera and 4,096 query rays with a fixed seed.
The meshes, images, transforms and uv ranges are tests/surface_families.py's. The rays aim at interior points of triangles, and in the texture cases at
positions whose four taps lie inside the map: the camera's own rays would cross the border strip of a 2 x 2 map (three quarters of it) and the
definition says nothing there.

    sphere80          one 80-triangle icosphere: its tree lives in LDS
    transforms        six of them (identity, rotation x scale, scale (1, 0.02, 30), shear, mirror, mirror x non-uniform scale): 480 triangles, not in LDS
    texel_grid        quads with maps of 2 x 2, 3 x 5, 16 x 16 (every byte value), 64 x 64 and 257 x 31 over uv [0, 1]
    wrap_m3.3_4.7, wrap_1000.25_1001.75   the same maps over those uv ranges
    uv_layouts        a mirrored uv layout, all three uvs equal, collinear uvs, a material without a map, a 4 x 4 map

TOLERANCES is measured on the CPU, never on a HIP build (tests/test_normal_map_abi.py measures again and fails if the table no longer follows): the angle
between map_f32 — fed what the ORACLE, which is the exact build bit for bit, reports for the unmapped hit — and map_f64, over the compared rays, as
a + b x slope x delta (surface_families.fit_texture; slope: radians per texel of sample position, delta: float32's resolution of that position), times
FACTOR = 4, this project's margin between a definition and a restatement."""
import copy
import math

import numpy as np

import normal_map_ref as nm
import surface_families as sf
import surface_ref as sr
from strolle_amd import Instance, Light, Material, Mesh, Sun, scenes

N_RAYS = sf.N_RAYS
FACTOR = 4.0
CAPS = dict(excluded=0.02, compared_mapped=0.10)
MAP_IMAGE = sf.IMAGE0 + 50
TEXTURE_CASES = ("texel_grid", "wrap_m3.3_4.7", "wrap_1000.25_1001.75")
CASES = ("sphere80", "transforms", "uv_layouts") + TEXTURE_CASES


def _inset_uv(mesh, lo, hi):
    """the mesh with its uvs mapped from [0, 1] into [lo, hi]: every tap of a 16 x 16 map then lies inside it"""
    p, n, uv = mesh
    return p, n, (lo + uv.astype(np.float64) * (hi - lo)).astype(np.float32)


def _sphere_scene(xforms):
    s = sr.Scene()
    s.meshes[sf.MESH0] = _inset_uv(sf.icosphere(), 0.1, 0.9)
    s.images[MAP_IMAGE] = sf.every_byte_image()
    s.materials[sf.MATERIAL0] = Material(base_color=(0.7, 0.6, 0.5, 1.0), normal_map_texture=MAP_IMAGE)
    for k, x in enumerate(xforms):
        s.instances.append((sf.INSTANCE0 + k, sf.MESH0, sf.MATERIAL0, x, x))
    return s


def _layouts_scene():
    """four quads: u mirrored; every uv equal; collinear uvs; the plain layout under a material without a map — and the plain layout with the map"""
    s = sr.Scene()
    s.images[MAP_IMAGE] = sf.noise_image(4, 4, 44)
    p, n, uv = sf.quad(0.15, 0.85)
    mirrored = uv.copy(); mirrored[..., 0] = np.float32(1.0) - uv[..., 0]
    equal = np.zeros_like(uv); equal[..., 0] = 0.3; equal[..., 1] = 0.6
    collinear = np.stack([uv[..., 0], uv[..., 0]], -1)                     # every uv on the line v = u: d = 0 exactly
    mapped, plain = Material(normal_map_texture=MAP_IMAGE), Material()
    for k, (layout, mat) in enumerate(((mirrored, mapped), (equal, mapped), (collinear, mapped), (uv, plain), (uv, mapped))):
        s.meshes[sf.MESH0 + k] = (p, n, layout.astype(np.float32))
        s.materials[sf.MATERIAL0 + k] = copy.copy(mat)
        x = sf.tilted(k, 1.25 * k, 0)
        s.instances.append((sf.INSTANCE0 + k, sf.MESH0 + k, sf.MATERIAL0 + k, x, x))
    return s, sf.camera_over((0, 0), (6.0, 1.0))


_scenes = {}


def scene_of(case):
    """(scene, camera) of a case; built once and left unchanged"""
    if case not in _scenes:
        if case == "sphere80":
            _scenes[case] = (_sphere_scene([sf.translate(0, 0)]), sf.camera_over((-1.0, -1.0), (1.0, 1.0)))
        elif case == "transforms":
            _scenes[case] = (_sphere_scene([x for _, x in sf.TRANSFORMS[:6]]), sf._transforms_camera())
        elif case == "uv_layouts":
            _scenes[case] = _layouts_scene()
        else:
            f = sf.frames(case)[0]
            s = copy.deepcopy(f.scene)
            for m in s.materials.values():
                m.normal_map_texture = m.base_color_texture          # the image is the map too: the same bytes through the other decode
            _scenes[case] = (s, f.camera)
    return _scenes[case]


def drive(e, case, images=None, scene=None):
    """the API calls that put the case's scene into engine e (product or oracle) and tick once; returns the camera handle.
    images: called instead of the plain insertion of the images (device-resident ones)."""
    s, camera = scene_of(case)
    s = scene or s
    e.set_blue_noise(scenes.load_blue_noise())
    if images is not None:
        images(e, s.images)
    else:
        for h, px in s.images.items():
            e.insert_image(h, px)
    for h, m in s.materials.items():
        e.insert_material(h, m)
    for h, (p, n, uv) in s.meshes.items():
        e.insert_mesh(h, Mesh(p, n, uv))
    for h, mesh, mat, x, _ in s.instances:
        e.insert_instance(h, Instance(mesh, mat, x))
    e.insert_light(1, Light.point((0.0, 5.0, 20.0), 0.1, (1.0, 1.0, 1.0), 200.0))
    e.update_sun(Sun(azimuth=0.0, altitude=-1.0))
    cam = e.create_camera(camera)
    e.tick()
    return cam


# ----------------------------------------------------------------------------- rays
def _texture_rays(case, s, rng, m):
    """m rays at chosen texel positions of every mapped quad (surface_families.case_rays' texture branch, without the camera's bundle)"""
    quads = [i for i, (_, _, mat, _, _) in enumerate(s.instances) if s.materials[mat].normal_map_texture]
    per = m // len(quads)
    targets, normals = [], []
    for j, i in enumerate(quads):
        _, mesh, mat, x, _ = s.instances[i]
        n = per if j + 1 < len(quads) else m - per * (len(quads) - 1)
        uv = s.meshes[mesh][2].astype(np.float64)
        lo, hi = uv.min(), uv.max()
        st = sf._texel_targets(s.images[s.materials[mat].normal_map_texture], rng, n, unit_range=False, coarse=case == "wrap_1000.25_1001.75")
        if case.startswith("wrap_"):
            periods = np.arange(math.floor(lo), math.ceil(hi))
            pos = st; st = (rng.choice(periods, (n, 2)) + pos - lo) / (hi - lo)
            for _ in range(16):
                st = np.where((st > 0.01) & (st < 0.99), st, (rng.choice(periods, (n, 2)) + pos - lo) / (hi - lo))
            st = np.where((st > 0.01) & (st < 0.99), st, rng.uniform(0.05, 0.95, (n, 2)))
        M = x.astype(np.float64)
        targets.append(np.concatenate([st, np.zeros((n, 1))], 1) @ M[:, :3].T + M[:, 3])
        normals.append(np.tile(M[:, :3] @ [0.0, 0.0, 1.0], (n, 1)))
    return sf._aim(np.concatenate(targets), np.concatenate(normals), rng, 1.0)


def _triangle_rays(s, rng, m):
    """m rays at interior points of randomly chosen triangles, from either side (surface_families.case_rays' generic branch)"""
    (p0, e1, e2), _, _ = sr.records(s)
    pick = rng.integers(0, len(p0), m)
    bu, bv = rng.uniform(0.05, 0.9, m), rng.uniform(0.05, 0.9, m)
    fold = bu + bv > 0.95; bu[fold], bv[fold] = 0.95 - bu[fold] + 0.05, 0.95 - bv[fold] + 0.05
    fold = bu + bv > 0.95; bu[fold] *= 0.5; bv[fold] *= 0.5
    P0, E1, E2 = (a.astype(np.float64)[pick] for a in (p0, e1, e2))
    nrm = np.cross(E1, E2); area = np.linalg.norm(nrm, axis=1, keepdims=True); nrm /= area
    return sf._aim(P0 + bu[:, None] * E1 + bv[:, None] * E2, nrm, rng, np.sqrt(area) * 3.0)


def case_rays(case):
    s, _ = scene_of(case)
    rng = np.random.default_rng(7000 + CASES.index(case))
    return _texture_rays(case, s, rng, N_RAYS) if case in TEXTURE_CASES else _triangle_rays(s, rng, N_RAYS)


# ----------------------------------------------------------------------------- what an engine reports for an unmapped hit -> map_f32's inputs
def first_slots(scene):
    """handle -> the instance's first triangle slot (instances take their slots in insertion order)"""
    out, at = {}, 0
    for h, mesh, _, _, _ in scene.instances:
        out[h] = at; at += len(scene.meshes[mesh][0])
    return out


def restate(scene, rays, hit, normal, uv, slot, triangles, materials, rects):
    """map_f32 over the rows `hit`: normal / uv [n, ...] float32 as an engine reports the UNMAPPED hit, slot [n] the winning triangle slot, triangles =
    read_scene(1), materials = read_scene(3), rects = {image handle: image_rect}. Returns (n' [n,3] float32 (zero off `hit`), mapped [n], border [n]: a tap
    outside the map's rectangle — the atlas around it is not among the inputs)."""
    tri = np.ascontiguousarray(triangles).view(np.float32).reshape(-1, 36)
    mats = np.ascontiguousarray(materials).view(np.float32).reshape(-1, 28)
    rows = np.flatnonzero(hit); sl = np.asarray(slot)[rows]
    p0, p1, p2 = tri[sl, 0:3], tri[sl, 12:15], tri[sl, 24:27]
    e1, e2 = (p1 - p0).astype(np.float32), (p2 - p0).astype(np.float32)
    uv0, uv1, uv2 = tri[sl][:, [3, 7]], tri[sl][:, [15, 19]], tri[sl][:, [27, 31]]
    handles = list(scene.materials)                                       # material slots follow insertion order
    inst_of = np.concatenate([np.full(len(scene.meshes[mesh][0]), i) for i, (_, mesh, _, _, _) in enumerate(scene.instances)])
    mat_slot = np.array([handles.index(m) for _, _, m, _, _ in scene.instances])[inst_of[sl]]
    rect = mats[mat_slot, 24:28]
    # the atlas is 8,192 texels wide (images.rs:28-29); its height follows from any map's rectangle: texels / the fraction the material holds
    heights = {round(rects[m.normal_map_texture][3] / float(mats[k, 27])) for k, m in enumerate(scene.materials.values()) if m.normal_map_texture and mats[k, 27] > 0}
    assert len(heights) <= 1, heights
    atlas_h = heights.pop() if heights else 256
    atlas = nm.build_atlas(scene.images, rects, atlas_h)
    s = nm.ray_sign(rays["direction"][rows], e1, e2)
    out32, mapped, taps = nm.map_f32(normal[rows], s, uv[rows], e1, e2, uv0, uv1, uv2, rect, atlas)
    # which rectangle a hit samples: the one whose fractions its material holds
    border = np.zeros(len(rows), bool)
    for h in scene.images:
        x, y, w, hh = rects[h]
        mine = np.isclose(rect[:, 0] * sr.ATLAS_EXTENT, x) & np.isclose(rect[:, 1] * atlas_h, y) & np.any(rect != 0, axis=1)
        border |= mine & ((taps[:, 0] < x) | (taps[:, 1] < y) | (taps[:, 2] > x + w - 1) | (taps[:, 3] > y + hh - 1))
    full = np.zeros((len(rays), 3), np.float32); full[rows] = out32
    fm = np.zeros(len(rays), bool); fm[rows] = mapped
    fb = np.zeros(len(rays), bool); fb[rows] = border
    return full, fm, fb


def texel_delta(scene, surf, rects):
    """[n]: float32's resolution of the map's sample position in texels (surface_families.texel_delta for the normal map)"""
    out = np.zeros(len(surf.instance))
    mat_of = np.array([m for _, _, m, _, _ in scene.instances])[np.where(surf.ans.hit, surf.instance, 0)]
    for handle, m in scene.materials.items():
        if m.normal_map_texture:
            rows = surf.ans.hit & (mat_of == handle)
            x, y, w, h = rects[m.normal_map_texture]
            out[rows] = 2.0 ** -24 * (max(x + w, y + h) + np.abs(surf.uv[rows]).max(axis=1) * max(w, h))
    return out


def compared(surf, mapped: nm.Mapped):
    """the rays the definition is compared on: surface_families.compared, and mapped, not a border sample of the map, not near a degeneracy"""
    return sf.compared(surf) & mapped.mapped & ~mapped.border & ~mapped.near_degenerate


def excluded(surf, mapped: nm.Mapped):
    """hits the definition says nothing about"""
    return surf.ans.hit & ((surf.ans.margin < sf.AMBIGUOUS) | surf.border | surf.undefined | mapped.border | mapped.near_degenerate)


def allowed(case, scene, surf, mapped, rects):
    """[n]: the case's tolerance on the angle between an answer and the definition"""
    t = TOLERANCES[case]
    return t["a"] + t["b"] * mapped.slope * texel_delta(scene, surf, rects)


# ----------------------------------------------------------------------------- the definition and the oracle's side, once per process
_refs = {}


def reference(case):
    """the case's rays and pixels, the definition's answers for both (surface_ref.surface, normal_map_ref.map_f64), and what the oracle reports for the
    unmapped hits; computed once per process, shared and left unchanged"""
    from oracle_binding import OracleEngine
    if case not in _refs:
        scene, camera = scene_of(case)
        rays, pixels = case_rays(case), sf.camera_rays(camera)
        surf, psurf = sr.surface(scene, rays), sr.surface(scene, pixels)
        orac = OracleEngine()
        try:
            drive(orac, case)
            rects = {h: orac.image_rect(h) for h in scene.images}
            _refs[case] = dict(scene=scene, camera=camera, rays=rays, pixels=pixels, surf=surf, psurf=psurf, mapped=nm.map_f64(scene, surf, rays),
                               pmapped=nm.map_f64(scene, psurf, pixels), rects=rects, probe=sf.probe_fields(sf.oracle_surface(orac, rays)),
                               triangles=orac.read_scene(1).copy(), materials=orac.read_scene(3).copy())
        finally:
            orac.close()
    return _refs[case]


def measure(case):
    """the restatement's worst deviation from the definition as (a, b), FACTOR x that rounded up, and the shares of rays excluded and compared"""
    c = reference(case)
    scene, surf, mapped, rays, probe = c["scene"], c["surf"], c["mapped"], c["rays"], c["probe"]
    hit = probe["t"] < np.float32(3.4028235e38)
    slot = probe["slot"].copy().view(np.uint32).astype(np.int64)
    got, got_mapped, _ = restate(scene, rays, hit, np.ascontiguousarray(probe["normal"]), np.ascontiguousarray(probe["uv"]), slot, c["triangles"], c["materials"], c["rects"])
    keep = compared(surf, mapped) & hit & (slot == surf.ans.slot)
    assert np.array_equal(got_mapped[keep], mapped.mapped[keep]), "the restatement applies a degeneracy rule where the definition does not"
    dev = sf.angle(got[keep], mapped.normal[keep])
    sd = (mapped.slope * texel_delta(scene, surf, c["rects"]))[keep]
    a, b = sf.fit_texture(dev, sd)
    n = len(rays)
    return dict(worst=dict(a=a, b=b, angle=float(dev.max(initial=0.0))), tolerance=dict(a=sf.round_up(FACTOR * a), b=sf.round_up(FACTOR * b)),
                shares=dict(excluded=float(excluded(surf, mapped).sum() / n), compared_mapped=float(keep.sum() / n), hits=float(surf.ans.hit.mean()),
                            unmapped_by_rule=float((surf.ans.hit & ~mapped.mapped).sum() / n)))


# TOLERANCES-BEGIN (python tests/normal_map_cases.py prints this table; tests/test_normal_map_abi.py holds it to the measurement)
TOLERANCES = {
    'sphere80': {'a': 0.0, 'b': 20.8},
    'transforms': {'a': 0.000276, 'b': 56.3},
    'uv_layouts': {'a': 1.75e-05, 'b': 33.1},
    'texel_grid': {'a': 0.0, 'b': 39.7},
    'wrap_m3.3_4.7': {'a': 0.0, 'b': 108.0},
    'wrap_1000.25_1001.75': {'a': 1.34e-05, 'b': 3.13},
}
# TOLERANCES-END


if __name__ == "__main__":
    import json
    report = {case: measure(case) for case in CASES}
    print(json.dumps(report, indent=1))
    print("TOLERANCES = {")
    for case in CASES:
        print(f"    {case!r}: {report[case]['tolerance']!r},")
    print("}")
