"""Both builds' long-run means against what the lighting estimators are SUPPOSED to converge to (light_ref.py), not against another program's frame.

Every other test of the ReSTIR and Reference kernels compares launches or frames with the oracle's, lane by lane within a tolerance: an estimate that
is 2 % too dark everywhere, a light pick whose pdf is slightly off or a fused launch that normalises one lane of its cell wrongly stays inside it.
Here each (case, mode) of light_cases.MATRIX runs 8 seeds x (64 warm-up + 1,000 averaged) frames on a fresh engine per seed, accumulates the composed
frame in a float64 tensor on the device (one read-back per seed), and takes the frame sum and every 8x8-block sum per channel over the pixels the
definition holds (no light in penumbra there). tools/estimator_expectation_profile.py (CPU oracle, 16 seeds) recorded each statistic's per-seed
spread sigma_seed and the oracle's own sums in tests/golden/estimator_expectation.npz and the systematic allowance b in
profiles/estimator_expectation.json; none of them comes from a GPU run.

    EXACT build   every sum equals the oracle's for the same 8 seeds, bit for bit (the recorded sum_8 row of tests/golden/estimator_expectation.npz)
    FAST build    definition-held statistics: |r_f - 1|   <= 5 sigma_seed / sqrt(8) + b
                  oracle-held statistics:     |r_f - r_o| <= 5 sigma_seed sqrt(1/8 + 1/16)     (GI_DIFFUSE, which has no closed form, and the
                                                                                                 rows "oracle_held" of the profile names)
                  its own per-seed spread <= 2 sigma_seed;  every frame finite (one non-finite frame leaves the float64 sum non-finite)
    FAST build with keep_all_planes, and with fuse = 0: a diffuse and the occluder case each — the lean and the fused launch structures are where a
                  lane can go missing.

Measured on one MI355X (the profile's "gpu" section): the fast build's worst statistic at 0.48 of its tolerance, its widest per-seed spread at 0.78
of the bound, no exact-build sum differing; 49 s for all 78 tests, 3.7 s the slowest. Of seven oracles broken one line at a time ("mutations") five
leave these tolerances; the two that do not are checkerboard-parity breaks that keep the mean unbiased on a static scene.

ST_ESTIMATOR_REPORT=<path> appends one JSON line per test (worst deviation in units of its tolerance, seconds)."""
import json
import math
import os
import time

import numpy as np
import pytest

import light_cases as lc
from strolle_amd import Engine

gpu = pytest.mark.gpu
K_FAST, K_SPREAD = 5.0, 2.0


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    return torch


def device_mean(case, mode, seed, exact, setup=None):
    """[h, w, 3] float64: the mean of FRAMES composed frames after WARMUP, on a fresh engine seeded `seed`; accumulated on the device"""
    torch = _torch()
    e = Engine(device=0, exact=exact)
    try:
        if setup:
            setup(e)
        case.build(e); e.set_seed(seed)
        cam_mode, depth = lc.MODE[mode]
        cam = e.create_camera(case.camera(cam_mode, depth))
        w, h = case.size
        out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
        acc = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream
        for f in range(lc.WARMUP + lc.FRAMES):
            e.tick()
            e.render_camera(cam, out.data_ptr(), stream)
            if f >= lc.WARMUP:
                acc += out[..., :3]
        return acc.cpu().numpy() / lc.FRAMES
    finally:
        e.close()


def _report(**row):
    path = os.environ.get("ST_ESTIMATOR_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def _row(case_name, mode):
    exp = lc.expectation(case_name, lc.DEFINED_BY.get(mode, mode))
    return lc.load_profile(), lc.recorded(case_name, mode), exp, lc.denominators(exp)[2]


@gpu
@pytest.mark.parametrize("case_name,mode", lc.MATRIX, ids=[f"{c}-{m}" for c, m in lc.MATRIX])
def test_exact_build_reproduces_the_oracles_sums(case_name, mode):
    t0 = time.time()
    _, rec, exp, recorded_names = _row(case_name, mode)
    case = lc.ALL_CASES[case_name]
    means = [device_mean(case, mode, s, exact=True) for s in lc.SEEDS8]
    assert all(np.isfinite(m).all() for m in means), "a non-finite frame"
    got, names = lc.sums(lc.pooled(means), exp.held)
    assert names == recorded_names and len(names) == len(rec["sum_8"])
    want = rec["sum_8"]
    differ = np.flatnonzero(got != want)
    _report(test="exact", case=case_name, mode=mode, differing=int(len(differ)), seconds=round(time.time() - t0, 2))
    assert not len(differ), f"{len(differ)} of {len(got)} sums differ from the oracle's; first: {names[differ[0]]} {got[differ[0]]!r} != {want[differ[0]]!r}"


def check_fast(case_name, mode, setup=None, label="fast"):
    t0 = time.time()
    prof, rec, exp, names = _row(case_name, mode)
    oracle_dev = lc.recorded_deviation(case_name, mode, rec)
    case = lc.ALL_CASES[case_name]
    means = [device_mean(case, mode, s, exact=False, setup=setup) for s in lc.SEEDS8]
    assert all(np.isfinite(m).all() for m in means), "a non-finite frame"
    dev, _ = lc.deviations(lc.pooled(means), exp)
    per_seed = np.array([lc.deviations(m, exp)[0] for m in means])
    sigma, b = rec["sigma_seed"], prof["b"]
    oracle_held = np.array([lc.oracle_held(prof, case_name, mode, n) for n in names])
    tol = np.where(oracle_held, K_FAST * sigma * math.sqrt(1 / 8 + 1 / 16), K_FAST * sigma / math.sqrt(8) + b)
    off = np.abs(dev - np.where(oracle_held, oracle_dev, 0.0))
    spread = per_seed.std(axis=0, ddof=1)
    with np.errstate(all="ignore"):
        units = np.where(tol > 0, off / tol, np.where(off > 0, np.inf, 0.0))
        spread_units = np.where(sigma > 0, spread / (K_SPREAD * sigma), np.where(spread > 0, np.inf, 0.0))
    k, ks = int(units.argmax()), int(spread_units.argmax())
    print(f"{label} {case_name} {mode}: frame deviation {dev[:3]}; worst {names[k]} {off[k]:.5f} = {units[k]:.2f} of its tolerance {tol[k]:.5f}; "
          f"worst spread {names[ks]} {spread[ks]:.5f} = {spread_units[ks]:.2f} of 2 sigma_seed")
    _report(test=label, case=case_name, mode=mode, frame_deviation=dev[:3].tolist(), worst=names[k], worst_in_tolerances=float(units[k]),
            worst_spread=names[ks], worst_spread_in_bounds=float(spread_units[ks]), seconds=round(time.time() - t0, 2))
    bad = np.flatnonzero(off > tol)
    assert not len(bad), (f"{len(bad)} of {len(off)} statistics leave their expectation; worst {names[k]}: deviation {dev[k]:+.5f}, "
                          f"{'oracle ' + format(oracle_dev[k], '+.5f') if oracle_held[k] else 'definition'}, tolerance {tol[k]:.5f}")
    wide = np.flatnonzero(spread > K_SPREAD * sigma)
    assert not len(wide), f"{len(wide)} statistics spread wider over seeds than 2 sigma_seed; worst {names[ks]}: {spread[ks]:.5f} against sigma_seed {sigma[ks]:.5f}"


@gpu
@pytest.mark.parametrize("case_name,mode", lc.MATRIX, ids=[f"{c}-{m}" for c, m in lc.MATRIX])
def test_fast_build_converges_to_the_expectation(case_name, mode):
    check_fast(case_name, mode)


VARIANT_ROWS = [("three", "DI_DIFFUSE"), ("occluder", "IMAGE")]


@gpu
@pytest.mark.parametrize("case_name,mode", VARIANT_ROWS, ids=[f"{c}-{m}" for c, m in VARIANT_ROWS])
def test_fast_build_keeping_all_planes_converges_to_the_expectation(case_name, mode):
    check_fast(case_name, mode, setup=lambda e: e.keep_all_planes(True), label="keep_all_planes")


@gpu
@pytest.mark.parametrize("case_name,mode", VARIANT_ROWS, ids=[f"{c}-{m}" for c, m in VARIANT_ROWS])
def test_fast_build_unfused_converges_to_the_expectation(case_name, mode):
    check_fast(case_name, mode, setup=lambda e: e.set_tuning(fuse=0), label="fuse=0")
