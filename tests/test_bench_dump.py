"""bench.py --dump-outputs on the host: dump_outputs() writes a frame up to 64 MB whole and a fixed sample of a larger one."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def _total_bytes(directory):
    return sum(os.path.getsize(os.path.join(directory, f)) for f in os.listdir(directory))


def test_a_frame_within_the_limit_is_written_whole(tmp_path):
    bench = _bench()
    frame = np.random.default_rng(1).random((64, 96, 4), dtype=np.float32)
    assert bench.dump_outputs(str(tmp_path), frame) == ["frame"]
    got = np.load(tmp_path / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, frame)


def test_a_frame_over_the_limit_is_a_fixed_sample_of_its_pixels(tmp_path):
    bench = _bench()
    height, width = 2160, 2048                                   # 70.8 MB of RGBA32F: over the 64 MB limit
    frame = np.random.default_rng(2).random((height, width, 4), dtype=np.float32)
    assert frame.nbytes > bench.DUMP_LIMIT_BYTES
    names = ["frame_sample", "frame_sample_index"]
    for run in ("a", "b"):
        assert bench.dump_outputs(str(tmp_path / run), frame) == names
        assert sorted(os.listdir(tmp_path / run)) == [n + ".npy" for n in names]
        assert _total_bytes(tmp_path / run) <= bench.DUMP_LIMIT_BYTES
    sample, index = np.load(tmp_path / "a" / "frame_sample.npy"), np.load(tmp_path / "a" / "frame_sample_index.npy")
    assert sample.dtype == np.float32 and index.dtype == np.float64 and sample.shape == (len(index), 4) and len(index) > 1 << 20
    flat = index.astype(np.int64)
    assert np.array_equal(flat, index) and (np.diff(flat) > 0).all() and 0 <= flat[0] and flat[-1] < height * width
    assert np.array_equal(frame.reshape(-1, 4)[flat], sample)
    # the same pixels on a second run, and for another frame of the same size
    assert np.array_equal(np.load(tmp_path / "b" / "frame_sample_index.npy"), index)
    assert np.array_equal(np.load(tmp_path / "b" / "frame_sample.npy"), sample)
    other = frame[::-1].copy()
    bench.dump_outputs(str(tmp_path / "c"), other)
    assert np.array_equal(np.load(tmp_path / "c" / "frame_sample_index.npy"), index)
    assert np.array_equal(np.load(tmp_path / "c" / "frame_sample.npy"), other.reshape(-1, 4)[flat])
