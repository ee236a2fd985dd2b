"""Supersampled frames, the parts that need no GPU: the numpy restatement of the resolve (mythtracer_amd/tiling.py,
resolve_ss), the claim the feature rests on -- the reference's sensor for s W x s H puts its rays on an s x s grid
inside every pixel of the W x H image (camera.cc:27-69) -- and the argument checks of the new entry points, which
come before any device call (include/mythtracer_hip.h, mt_render_chunk_ss ff.)."""
import ctypes

import numpy as np
import pytest

import orclib

import mythtracer_amd as M
from mythtracer_amd import binding, tiling

MT_ERR_ARG, MT_ERR_HIP = -1, -2
CORNELL_CAM = (50, 50, -120, 0, 0, 0, 60)


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    return native_libs


def slow_resolve(a, s):
    """The definition, one output byte at a time, in Python integers."""
    h, w, c = a.shape[0] // s, a.shape[1] // s, a.shape[2]
    n = s * s
    out = np.zeros((h, w, c), dtype=np.uint8)
    for y in range(h):
        for x in range(w):
            for k in range(c):
                total = sum(int(a[s * y + j, s * x + i, k]) for j in range(s) for i in range(s))
                out[y, x, k] = (total + n // 2) // n
    return out


@pytest.mark.parametrize("s", [2, 3, 4])
def test_resolve_of_a_constant_image_is_constant(s):
    for value in (0, 1, 127, 128, 254, 255):
        a = np.full((3 * s, 5 * s, 3), value, dtype=np.uint8)
        assert np.array_equal(tiling.resolve_ss(a, s), np.full((3, 5, 3), value, dtype=np.uint8))


def test_resolve_rounds_to_nearest_ties_up():
    block = lambda vals, s: np.array(vals, dtype=np.uint8).reshape(s, s, 1)
    assert tiling.resolve_ss(block([0, 0, 0, 1], 2), 2).tolist() == [[[0]]]      # 1/4 -> 0
    assert tiling.resolve_ss(block([0, 0, 1, 1], 2), 2).tolist() == [[[1]]]      # 2/4: the tie goes up
    assert tiling.resolve_ss(block([0, 1, 1, 1], 2), 2).tolist() == [[[1]]]
    assert tiling.resolve_ss(block([255] * 16, 4), 4).tolist() == [[[255]]]      # the largest sum, 4080
    assert tiling.resolve_ss(block([1] * 4 + [0] * 5, 3), 3).tolist() == [[[0]]]  # 4/9 -> 0
    assert tiling.resolve_ss(block([1] * 5 + [0] * 4, 3), 3).tolist() == [[[1]]]  # 5/9 -> 1
    assert tiling.resolve_ss(block([7], 1), 1).tolist() == [[[7]]]


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_resolve_equals_the_formula_on_random_bytes(s):
    rng = np.random.default_rng(1234 + s)
    a = rng.integers(0, 256, size=(7 * s, 11 * s, 3), dtype=np.uint8)
    got = tiling.resolve_ss(a, s)
    assert got.dtype == np.uint8 and got.shape == (7, 11, 3)
    assert np.array_equal(got, slow_resolve(a, s))


def test_resolve_refuses_sizes_that_are_no_multiple():
    a = np.zeros((6, 6, 3), dtype=np.uint8)
    assert tiling.resolve_ss(a, 3).shape == (2, 2, 3)
    for bad in (a[:5], a[:, :5]):
        with pytest.raises(ValueError):
            tiling.resolve_ss(bad, 2)
    with pytest.raises(ValueError):
        tiling.resolve_ss(a[:4, :4], 4 + 1)
    with pytest.raises(ValueError):
        tiling.resolve_ss(a, 0)
    with pytest.raises(ValueError):
        tiling.resolve_ss(a.astype(np.float32), 2)


@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("size", [(128, 128), (96, 64), (101, 67)])
def test_sample_grid_is_the_in_pixel_grid(s, size):
    """orclib.sensor = Camera::GetSensor + Sensor::Reset of the CPU oracle: origin, start_point, delta_scanline,
    delta_pixel.  For s W x s H the start point is the same corner of the same frustum, bit for bit (aov_vertical
    depends on H / W only), and a delta is the W x H delta over s, up to the one rounding of v / (s W) against
    (v / W) / s (camera.cc:58-62): 1 ulp per component."""
    W, H = size
    one = orclib.sensor(CORNELL_CAM, W, H).reshape(4, 3)
    many = orclib.sensor(CORNELL_CAM, s * W, s * H).reshape(4, 3)
    assert np.array_equal(many[0], one[0])  # origin
    assert np.array_equal(many[1], one[1])  # start_point
    for k in (2, 3):
        want = one[k] / s
        assert (np.abs(many[k] - want) <= np.spacing(np.abs(want))).all(), (k, many[k], want)
    # the host facade's sensor (what RayTrace hands to the kernels) is the oracle's
    assert np.array_equal(binding.sensor(CORNELL_CAM, s * W, s * H).reshape(4, 3), many)


def _calls(abi, ss, image_w, image_h):
    """The three new entry points with scene = NULL: the only way to their argument checks without a device."""
    sens = binding.mt_sensor()
    buf = np.zeros(64, dtype=np.uint8)
    yield "mt_render_chunk_ss", abi.lib.mt_render_chunk_ss(None, ctypes.byref(sens), image_w, image_h, 0, 0, 1, 1, ss, 5,
                                                           buf.ctypes.data, None)
    yield "mt_render_chunk_ss_device", abi.lib.mt_render_chunk_ss_device(None, ctypes.byref(sens), image_w, image_h, 0, 0,
                                                                         1, 1, ss, 5, buf.ctypes.data, None)
    yield "mt_resolve_tiles_device", abi.lib.mt_resolve_tiles_device(None, image_w, image_h, 4, 4, 0, 1, None, 1, ss,
                                                                     buf.ctypes.data, buf.ctypes.data, None)


@pytest.mark.parametrize("ss", [0, 5, -1])
def test_bad_factor_is_an_argument_error_before_the_scene_is_looked_at(ss):
    abi = M.hip_abi()
    for name, rc in _calls(abi, ss, 8, 8):
        assert rc == MT_ERR_ARG, (name, rc, abi.last_error())
        assert "ss" in abi.last_error(), (name, abi.last_error())


@pytest.mark.parametrize("ss,w,h", [(2, 50001, 8), (4, 25001, 8), (3, 8, 33334), (2, 0, 8)])
def test_sample_grid_beyond_the_size_limit_is_an_argument_error(ss, w, h):
    abi = M.hip_abi()
    for name, rc in _calls(abi, ss, w, h):
        assert rc == MT_ERR_ARG, (name, rc, abi.last_error())
        assert "size" in abi.last_error() and "ss" in abi.last_error(), (name, abi.last_error())


@pytest.mark.parametrize("ss,w,h", [(1, 8, 8), (2, 8, 8), (3, 8, 8), (4, 8, 8), (2, 50000, 8), (4, 25000, 25000)])
def test_good_factor_reaches_the_scene_check(ss, w, h):
    abi = M.hip_abi()
    for name, rc in _calls(abi, ss, w, h):
        assert rc == MT_ERR_ARG and rc != MT_ERR_HIP, (name, rc, abi.last_error())
        assert abi.last_error() == "scene is NULL", (name, abi.last_error())


def test_facade_checks_the_factor_before_it_needs_a_device():
    m = M.MythTracer()
    for bad in (7, 0, -2, 5):
        m.set_supersampling(bad)
        for call in (lambda: m.render(CORNELL_CAM, 8, 8), lambda: m.render_image(CORNELL_CAM, 8, 8)):
            with pytest.raises(RuntimeError) as e:
                call()
            assert "supersampling factor %d" % bad in str(e.value), str(e.value)
    m.set_supersampling(2)
    with pytest.raises(RuntimeError) as e:
        m.render(CORNELL_CAM, 8, 8, debug=True)
    assert "output_debug" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        m.render(CORNELL_CAM, 50001, 8)
    assert "out of range" in str(e.value)
    m.set_devices([0, 0])
    with pytest.raises(RuntimeError) as e:
        m.render_image(CORNELL_CAM, 8, 8)
    assert "several devices" in str(e.value)


def test_abi_version_and_symbols():
    assert binding.MT_ABI_VERSION == 5 == M.hip_abi().lib.mt_abi_version()
    for name in ("mt_render_chunk_ss", "mt_render_chunk_ss_device", "mt_resolve_tiles_device"):
        assert name in M.HIP_SYMBOLS and getattr(M.hip_abi().lib, name) is not None
