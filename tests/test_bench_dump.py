"""bench.py --dump-outputs (bench.dump_outputs): the frame as float32, whole when it fits, else a fixed
seeded sample of its pixels that is the same at every run. CPU only."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def _frame(h, w):
    return np.random.default_rng(3).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def test_small_frame_is_dumped_whole_as_float32(tmp_path):
    frame = _frame(7, 5)
    bench.dump_outputs(str(tmp_path / "out"), frame)
    assert os.listdir(tmp_path / "out") == ["frame_rgb.npy"]
    got = np.load(tmp_path / "out" / "frame_rgb.npy")
    assert got.dtype == np.float32 and got.shape == (7, 5, 3)
    assert np.array_equal(got, frame.astype(np.float32))


def test_large_frame_is_a_fixed_sample_below_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 40 * 12)  # 40 pixels of 3 float32
    frame = _frame(9, 11)
    bench.dump_outputs(str(tmp_path / "a"), frame)
    bench.dump_outputs(str(tmp_path / "b"), frame)
    a = np.load(tmp_path / "a" / "frame_rgb.npy")
    assert a.dtype == np.float32 and a.shape == (40, 3) and a.nbytes <= bench.DUMP_MAX_BYTES
    assert np.array_equal(a, np.load(tmp_path / "b" / "frame_rgb.npy"))
    idx = np.sort(np.random.default_rng(0).choice(99, 40, replace=False))
    assert np.array_equal(a, frame.reshape(-1, 3)[idx].astype(np.float32))


def test_headline_frame_fits_and_the_cap_is_below_64_mb():
    assert 1920 * 1080 * 3 * 4 <= bench.DUMP_MAX_BYTES < 64 * 10**6
