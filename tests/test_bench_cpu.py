"""bench.py's --dump-outputs files, without a GPU: the frame of the last timed
step as float32, or a fixed, seeded sample of a frame too big for the limit."""
import os

import numpy as np

import bench


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_of_a_1080p_frame_is_the_whole_frame(tmp_path):
    frame = np.random.default_rng(1).integers(0, 256, size=(1080, 1920, 3), dtype=np.uint8)
    assert bench.write_outputs(str(tmp_path), frame) == ["frame"]
    got = np.load(tmp_path / "frame.npy")
    assert got.dtype == np.float32 and got.shape == (1080, 1920, 3)
    assert np.array_equal(got, frame.astype(np.float32))
    assert _sizes(str(tmp_path)) <= bench.DUMP_LIMIT_BYTES


def test_dump_of_a_4k_frame_is_a_seeded_sample(tmp_path):
    frame = np.random.default_rng(2).integers(0, 256, size=(2160, 3840, 3), dtype=np.uint8)
    a, b = tmp_path / "a", tmp_path / "b"
    assert bench.write_outputs(str(a), frame) == ["frame_sample", "frame_sample_pixel"]
    bench.write_outputs(str(b), frame)
    assert _sizes(str(a)) <= bench.DUMP_LIMIT_BYTES
    for name in ("frame_sample", "frame_sample_pixel"):
        assert np.array_equal(np.load(a / (name + ".npy")), np.load(b / (name + ".npy")))
    values, pix = np.load(a / "frame_sample.npy"), np.load(a / "frame_sample_pixel.npy")
    assert values.dtype == np.float32 and pix.dtype == np.float64 and len(values) == len(pix) > 10 ** 6
    assert np.all(np.diff(pix) > 0) and pix[0] >= 0 and pix[-1] < 2160 * 3840
    assert np.array_equal(values, frame.reshape(-1, 3)[pix.astype(np.int64)].astype(np.float32))
