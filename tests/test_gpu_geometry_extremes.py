"""Every walk and both tree builders against brute force, at geometric extremes (tests/geometry_extremes.py lists the families and what each reaches).

The reference side is tests/walk_ref.py: a float64 Moeller-Trumbore over ALL triangles of the engine's own baked records, no tree. Against it, on every
ray the restatement does not call ambiguous (profiles/geometry_extremes.json holds each family's threshold and t tolerance, measured on the CPU against
the oracle by tests/test_walk_ref.py): hit / miss, the winning triangle and occlusion are IDENTICAL, t and the hit point are within the tolerance. A
conservative box may cost time, never a hit — so there is no agreement share here, unlike the 0.999 of tests/test_gpu_ray_query.py.

The stack contract (st_traverse.h "returns ST_ERR_BVH_TOO_DEEP once", st_engine.h): infinite f16 boxes make a wide walk enter every node, its stack may
fill. That is reported by the next tick, once, and the deeper stack is used from then on; the answers after that tick owe everything above. A wrong
answer under status OK is what this file exists to catch.

ST_GEOMETRY_EXTREMES_DUMP=<directory>: every case leaves what it observed there (tools/geometry_extremes_profile.py --gpu merges it into the profile)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import geometry_extremes as gx
import walk_ref
from oracle_binding import OracleEngine
from strolle_amd import Buffer, CameraMode, Engine, StrolleError
from strolle_amd.api import ST_ERR_BVH_TOO_DEEP
from test_gpu_ray_query import (_lib, _stream, assert_exact, assert_misses_are_clean, gpu_occluded, gpu_trace, make_rays, oracle_closest,
                                oracle_occluded)

pytestmark = pytest.mark.gpu

# exact / fast build, StTuning, st_set_bvh_refresh mode, whether the soup moves by a quarter of its extent after the first tick (so the tree is refitted)
CONFIGS = {
    "exact": dict(exact=True),
    "default": dict(exact=False),
    "no_wide": dict(exact=False, tuning=dict(wide_bvh=0)),                    # the compact stream
    "device_tree": dict(exact=False, refresh=3, big=True),                    # k_lbvh: keys, sort, wide-node writers
    "refit_host": dict(exact=False, refresh=1, moved=True),
    "refit_device": dict(exact=False, refresh=3, moved=True, big=True),
}
# the first tree of a scene that fits LDS is the host's (st_tick.cpp: the device builds only above kLdsSceneTexels / 4 triangles): `big` configurations
# run at 600 triangles only
CASES = [(f, n, c) for f, n in gx.CASES for c, o in CONFIGS.items() if n > 112 or not o.get("big")]
RENDER_CONFIGS = {"exact": dict(exact=True), "default": dict(exact=False), "no_packets": dict(exact=False, tuning=dict(primary_packets=0))}
SIZE = (96, 64)

_profile = gx.load_profile()["cases"]
_refs = {}


def _reference(tris, rays):
    """the restatement's answer for these records and rays: computed once, shared by the configurations that see the same scene, never changed"""
    key = (tris.tobytes(), rays.tobytes())
    if key not in _refs:
        if len(_refs) > 8:
            _refs.clear()
        _refs[key] = walk_ref.trace(*walk_ref.records(tris), rays)
    return _refs[key]


def _vertices(tris, slots):
    return np.ascontiguousarray(tris).view(np.float32).reshape(-1, 9, 4)[:, [0, 3, 6], :3].reshape(-1, 9)[slots]


def _engine(family, n, exact, tuning=None, refresh=None, moved=False, **_):
    """(engine, oracle engine with the same scene, mesh positions, the instances' translation)"""
    e, orac = Engine(device=0, exact=exact), OracleEngine()
    if tuning:
        e.set_tuning(**tuning)
    if refresh is not None:
        e.set_bvh_refresh(refresh)
    pos = gx.build_extreme(e, family, n); gx.build_extreme(orac, family, n)
    e.tick(); orac.tick()
    shift = None
    if refresh == 3 and n > 112:
        assert e.device_builds() >= 1, "the tree was not built on the device"
    if moved:
        shift = gx.quarter_extent(family, pos)
        refits0 = e.device_tree_refits() if refresh == 3 else e.bvh_refits()[1]
        gx.move(e, family, shift); gx.move(orac, family, shift)
        e.tick(); orac.tick()
        assert (e.device_tree_refits() if refresh == 3 else e.bvh_refits()[1]) == refits0 + 1, "the move was not answered by a refit"
    return e, orac, pos, shift


class StackContract:
    """Runs `ask` (a function that enqueues queries / frames and returns their answers) under the product's contract for a full wide stack: the tick after it
    may return ST_ERR_BVH_TOO_DEEP, at most once per engine; walk_overflow() must then show it; the answers asked again after that tick are the ones judged."""

    def __init__(self, e):
        self.e, self.reported = e, 0

    def answers(self, ask):
        got = ask()
        try:
            self.e.tick()
        except StrolleError as err:
            assert f"status {ST_ERR_BVH_TOO_DEEP}" in str(err), str(err)
            self.reported += 1
            assert self.reported <= 1, "a full stack was reported a second time"
            n, entries, _ = self.e.walk_overflow()
            assert n >= 1 and entries > 24, f"the tick reported a full stack, walk_overflow() does not show it: {(n, entries)}"
            got = ask()
            self.e.tick()            # the deeper stack holds: nothing more to report
        return got

    def observed(self):
        n, entries, packets_off = self.e.walk_overflow()
        return dict(overflowed=bool(self.reported), stack_entries=int(entries), packets_off=bool(packets_off))


def _dump(case, config, observed):
    d = os.environ.get("ST_GEOMETRY_EXTREMES_DUMP")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, f"{case.replace('/', '_')}_{config}.json"), "w") as f:
            json.dump(dict(case=case, config=config, observed=observed), f)


def _check(what, family, prof, extent, tris, ref, rows, hit, t, point, verts=None, occluded=None):
    """the assertions of this file for the rays `rows` of `ref`; returns the worst relative t deviation on the rays judged"""
    thr, tol = prof["threshold"], prof["t_tolerance"]
    sure = ref.decision_margin[rows] >= thr
    want = ref.hit[rows]
    bad = sure & (hit != want)
    assert not bad.any(), (f"{what}: {int(bad.sum())} non-ambiguous rays decide hit / miss differently from brute force (first rows {rows[bad][:5]}, "
                           f"margins {ref.decision_margin[rows][bad][:5]}, brute force says {want[bad][:5]})")
    if occluded is not None:
        bad = sure & (occluded != ref.occluded[rows])
        assert not bad.any(), f"{what}: occlusion differs from brute force on {int(bad.sum())} non-ambiguous rays (first rows {rows[bad][:5]})"
    both = sure & hit & want
    dev = np.abs(t[both].astype(np.float64) - ref.t[rows][both]) / ref.t[rows][both] if t is not None else np.zeros(0)
    worst = float(dev.max()) if len(dev) else 0.0
    print(f"{what}: {int(both.sum())} hits judged, {int((~sure).sum())} ambiguous, worst t deviation {worst:.3g} (tolerance {tol:.3g})")
    assert worst <= tol, f"{what}: t deviates by {worst:.3g}, tolerance {tol:.3g}"
    pdev = np.abs(point[both].astype(np.float64) - ref.point[rows][both]).max(axis=1) if both.any() else np.zeros(0)
    assert np.all(pdev <= tol * extent), f"{what}: the hit point is {float(pdev.max()):.3g} off, tolerance {tol * extent:.3g}"
    if verts is not None:
        same = both & (ref.margin[rows] >= thr)          # where two triangles tie in t either one is a correct winner
        bad = same.copy(); bad[same] = np.any(verts[same] != _vertices(tris, ref.slot[rows][same]), axis=1)
        assert not bad.any(), f"{what}: {int(bad.sum())} non-ambiguous rays found another triangle than brute force (first rows {rows[bad][:5]})"
    return worst


@pytest.mark.parametrize("family,n,config", CASES, ids=[f"{f}-{n}-{c}" for f, n, c in CASES])
def test_ray_queries_equal_brute_force(family, n, config):
    opts = CONFIGS[config]
    prof = _profile[gx.case_key(family, n)]
    e, orac, pos, shift = _engine(family, n, **opts)
    try:
        tris = e.read_scene(1).copy()                            # the engine's own records, after the tick (and the refit)
        assert np.array_equal(tris.view(np.uint32), orac.read_scene(1).view(np.uint32)), "the product and the oracle baked different records"
        lo, hi = gx.box_of(tris)
        extent = float(np.linalg.norm(hi.astype(np.float64) - lo))
        rays = gx.family_rays(family, n, tris)
        ref = _reference(tris, rays)
        world = pos if shift is None else (pos + shift).astype(np.float32)
        contract = StackContract(e)
        got, packet, occ = contract.answers(lambda: (gpu_trace(e, rays), gpu_trace(e, rays[:gx.N_BUNDLE], coherent=True), gpu_occluded(e, rays)))
        what = f"{family}/{n} {config}"
        rows = np.arange(len(rays))
        worst = 0.0
        for name, g, r, o in (("trace_rays", got, rows, occ), ("coherent bundle", packet, rows[:gx.N_BUNDLE], None)):
            assert_misses_are_clean(g)
            h = g["hit"] == 1
            assert np.all(np.isin(g["instance"][h], gx.instance_handles(family))) and np.all(g["triangle"][h] < len(world))
            verts = world[np.where(h, g["triangle"], 0)].reshape(-1, 9)
            worst = max(worst, _check(f"{what} {name}", family, prof, extent, tris, ref, r, h, g["t"], g["point"], verts, o))
        if opts["exact"]:                                        # the exact build additionally equals the oracle bit for bit, on ALL rays
            assert_exact(got, oracle_closest(orac, rays), what)
            assert np.array_equal(occ, oracle_occluded(orac, rays)), f"{what}: occlusion differs from the oracle"
        _dump(gx.case_key(family, n), config, dict(worst_t_deviation=worst, **contract.observed()))
    finally:
        e.close(); orac.close()


def _camera_rays(desc):
    c = desc.to_c(); w, h = desc.size
    out = np.zeros((h * w, 6), np.float32)
    for i in range(h * w):
        _lib.or_probe_camera_ray(C.byref(c), i % w, i // w, out[i].ctypes.data)
    return make_rays(out[:, :3], out[:, 3:], np.full(h * w, np.inf, np.float32))


RENDER_CASES = [(f, c) for f in gx.FAMILIES for c in RENDER_CONFIGS]


@pytest.mark.parametrize("family,config", RENDER_CASES, ids=[f"{f}-{c}" for f, c in RENDER_CASES])
def test_primary_visibility_equals_brute_force(family, config):
    """the path that draws the frame: one CameraMode.REFERENCE frame at depth 0, REF_HITS against the restatement of the same camera rays"""
    n = 600
    prof = _profile[gx.case_key(family, n)]
    e, orac, _, _ = _engine(family, n, **RENDER_CONFIGS[config])
    try:
        tris = e.read_scene(1).copy()
        lo, hi = gx.box_of(tris)
        extent = float(np.linalg.norm(hi.astype(np.float64) - lo))
        desc = gx.family_camera(*gx.ray_box(family, tris), size=SIZE)
        cam = e.create_camera(desc)
        e.tick()
        rays = _camera_rays(desc)
        ref = _reference(tris, rays)
        out = torch.zeros((SIZE[1], SIZE[0], 4), dtype=torch.float32, device="cuda")

        def frame():
            e.render_camera(cam, out.data_ptr(), _stream())
            torch.cuda.synchronize()
            return e.read_buffer(cam, Buffer.REF_HITS).reshape(SIZE[0] * SIZE[1], -1).copy()

        contract = StackContract(e)
        hits = contract.answers(frame)
        point = hits[:, :3]
        hit = np.any(point != 0, axis=1)                          # hit.rs: a zero point is a miss
        assert ref.hit.sum() >= 500 or family == "small", f"{family}: only {int(ref.hit.sum())} pixels see the scene"
        _check(f"{family}/{n} frame {config}", family, prof, extent, tris, ref, np.arange(len(rays)), hit, None, point)   # (REF_HITS keeps no t: the point stands for it)
        _dump(gx.case_key(family, n), f"frame_{config}", dict(hit_pixels=int(hit.sum()), **contract.observed()))
    finally:
        e.close(); orac.close()
