"""Adaptive supersampling, the parts that need no GPU: the numpy restatement of the contract (mythtracer_amd/tiling.py:
chunk_blocks, refine_mask, compose_adaptive; include/mythtracer_hip.h, mt_render_chunk_adaptive ff.), the refined
share of the committed goldens -- the condition that keeps the GPU tests from passing on all-or-nothing masks --, and
the argument checks of the new entry points, which come before any device call."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import mythtracer_amd as M
from mythtracer_amd import binding, tiling

MT_ERR_ARG = -1
CORNELL_CAM = (50, 50, -120, 0, 0, 0, 60)


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    return native_libs


def slow_mask(f, image_w, chunk, threshold):
    """The definition, one pair at a time, in Python integers."""
    cx, cy, cw, ch = chunk
    x0, y0, mw, mh = tiling.chunk_blocks(chunk)
    mask = np.zeros((mh, mw), dtype=bool)
    for y in range(ch):
        for x in range(cw):
            for dx, dy in ((1, 0), (0, 1)):
                if x + dx >= cw or y + dy >= ch:
                    continue  # (the pair would cross the chunk's border: no pair)
                if max(abs(int(f[y, x, c]) - int(f[y + dy, x + dx, c])) for c in range(3)) > threshold:
                    for px, py in ((x, y), (x + dx, y + dy)):
                        mask[(py + cy) // 8 - y0, (px + cx) // 8 - x0] = True
    tiles = [(by + y0) * ((image_w + 7) // 8) + bx + x0 for by in range(mh) for bx in range(mw) if mask[by, bx]]
    return mask, np.array(tiles, dtype=np.int32)


def test_flat_frame_has_an_empty_mask():
    f = np.full((20, 33, 3), 77, dtype=np.uint8)
    for t in (0, 16, 255):
        mask, tiles = tiling.refine_mask(f, 33, 20, None, t)
        assert mask.shape == (3, 5) and not mask.any() and tiles.size == 0 and tiles.dtype == np.int32


def test_a_pixel_at_a_block_corner_refines_the_four_touching_blocks():
    f = np.full((32, 32, 3), 10, dtype=np.uint8)
    f[16, 16, 1] = 200  # first pixel of block (2, 2): its pairs reach (15, 16) and (16, 15)
    mask, tiles = tiling.refine_mask(f, 32, 32, None, 16)
    want = np.zeros((4, 4), dtype=bool)
    want[2, 2] = want[2, 1] = want[1, 2] = True
    assert np.array_equal(mask, want)  # (15, 15) is no neighbour: the diagonal block stays
    # the four blocks around a corner: a pixel pair on each side of it
    f = np.full((32, 32, 3), 10, dtype=np.uint8)
    f[15, 15] = 200
    f[16, 16] = 200
    mask, tiles = tiling.refine_mask(f, 32, 32, None, 16)
    want = np.zeros((4, 4), dtype=bool)
    want[1:3, 1:3] = True
    assert np.array_equal(mask, want)
    assert tiles.tolist() == [5, 6, 9, 10]
    assert np.array_equal(mask, slow_mask(f, 32, (0, 0, 32, 32), 16)[0])


def test_a_pair_across_the_chunk_border_is_ignored():
    image = np.full((32, 32, 3), 10, dtype=np.uint8)
    image[:, :12] = 250  # a vertical edge between x = 11 and x = 12
    chunk = (12, 0, 20, 32)  # starts right of the edge: the edge's pairs straddle the border
    cx, cy, cw, ch = chunk
    mask, tiles = tiling.refine_mask(image[cy:cy + ch, cx:cx + cw], 32, 32, chunk, 16)
    assert mask.shape == (4, 3) and not mask.any() and tiles.size == 0
    chunk = (11, 0, 21, 32)  # one column more: the pairs exist, in block column 1
    cx, cy, cw, ch = chunk
    mask, tiles = tiling.refine_mask(image[cy:cy + ch, cx:cx + cw], 32, 32, chunk, 16)
    assert mask[:, 0].all() and not mask[:, 1:].any()
    assert tiles.tolist() == [1, 5, 9, 13]


def test_threshold_is_strict():
    for t in (0, 16, 100, 254):
        f = np.full((8, 16, 3), 0, dtype=np.uint8)
        f[3, 5, 2] = t  # a difference equal to the threshold
        assert not tiling.refine_mask(f, 16, 8, None, t)[0].any()
        f[3, 5, 2] = t + 1
        mask, tiles = tiling.refine_mask(f, 16, 8, None, t)
        assert mask.tolist() == [[True, False]] and tiles.tolist() == [0]
    f = np.zeros((8, 16, 3), dtype=np.uint8)
    f[::2] = 255
    assert not tiling.refine_mask(f, 16, 8, None, 255)[0].any()
    assert tiling.refine_mask(f, 16, 8, None, 254)[0].all()
    for bad in (-1, 256):
        with pytest.raises(ValueError):
            tiling.refine_mask(f, 16, 8, None, bad)


@pytest.mark.parametrize("chunk", [(13, 27, 65, 33), (159, 89, 1, 1), (8, 8, 8, 8), (150, 0, 10, 90), (3, 5, 7, 5),
                                   (7, 7, 2, 2), (0, 0, 160, 90)])
def test_chunks_off_the_block_grid(chunk):
    W, H = 160, 90
    cx, cy, cw, ch = chunk
    x0, y0, mw, mh = tiling.chunk_blocks(chunk)
    assert (x0, y0) == (cx // 8, cy // 8)
    assert mw == (cx + cw - 1) // 8 - cx // 8 + 1 and mh == (cy + ch - 1) // 8 - cy // 8 + 1
    rng = np.random.default_rng(cx * 1000 + cy)
    f = np.full((ch, cw, 3), 100, dtype=np.uint8)
    n = max(1, cw * ch // 50)
    f[rng.integers(0, ch, n), rng.integers(0, cw, n), rng.integers(0, 3, n)] = rng.integers(0, 256, n)
    for t in (0, 16, 254):
        mask, tiles = tiling.refine_mask(f, W, H, chunk, t)
        want_mask, want_tiles = slow_mask(f, W, chunk, t)
        assert mask.shape == (mh, mw)
        assert np.array_equal(mask, want_mask), (chunk, t)
        assert np.array_equal(tiles, want_tiles) and (np.diff(tiles) > 0).all()
        assert len(tiles) == mask.sum()


def test_compose_is_a_per_pixel_where():
    rng = np.random.default_rng(7)
    W, H = 160, 90
    for chunk in [(13, 27, 65, 33), (0, 0, 160, 90), (159, 89, 1, 1)]:
        cx, cy, cw, ch = chunk
        a = rng.integers(0, 256, (ch, cw, 3), dtype=np.uint8)
        b = rng.integers(0, 256, (ch, cw, 3), dtype=np.uint8)
        x0, y0, mw, mh = tiling.chunk_blocks(chunk)
        mask = rng.integers(0, 2, (mh, mw)).astype(bool)
        got = tiling.compose_adaptive(a, b, mask, chunk)
        for y in range(ch):
            for x in range(cw):
                src = b if mask[(y + cy) // 8 - y0, (x + cx) // 8 - x0] else a
                assert np.array_equal(got[y, x], src[y, x])
        with pytest.raises(ValueError):
            tiling.compose_adaptive(a, b, np.zeros((mh + 1, mw), dtype=bool), chunk)


@pytest.mark.parametrize("case", ["cornell_256", "mini_320x180", "room_240x135", "cornell_cam2_96x64", "f2_decal_96x64"])
def test_goldens_refine_some_blocks_but_not_all(case):
    """At threshold 16 the reference's frames have flat blocks and contrasty ones."""
    g = np.load(os.path.join(GOLDEN, case + ".npz"), allow_pickle=False)
    W, H = (int(v) for v in g["image"])
    assert tuple(int(v) for v in g["chunk"]) == (0, 0, W, H)
    mask, tiles = tiling.refine_mask(g["rgb"], W, H, None, 16)
    share = mask.mean()
    print("%s: %d of %d blocks refined (%.0f %%)" % (case, mask.sum(), mask.size, 100 * share))
    assert 0.05 < share < 0.95


def test_abi_version_and_symbols():
    assert binding.MT_ABI_VERSION == 5 == M.hip_abi().lib.mt_abi_version()
    header = open(os.path.join(ROOT, "include", "mythtracer_hip.h")).read()
    for name in ("mt_refine_mask_device", "mt_render_chunk_adaptive", "mt_render_chunk_adaptive_device"):
        assert name in M.HIP_SYMBOLS and getattr(M.hip_abi().lib, name) is not None
        assert "int %s(" % name in header
    assert "mt_adaptive_info" in header and "#define MT_ABI_VERSION 5" in header
    assert ctypes.sizeof(binding.mt_adaptive_info) == 16
    assert hasattr(M.hip_abi(), "render_chunk_adaptive") and hasattr(M.MythTracer, "set_adaptive_supersampling")


def _call(abi, ss=2, threshold=16, rgb=True, image=(8, 8), chunk=(0, 0, 1, 1), sensor=True, sensor_ss=True, device=False):
    """The composed entry points with scene = NULL: the only way to their argument checks without a device."""
    sens, sens_ss = binding.mt_sensor(), binding.mt_sensor()
    buf = np.zeros(64, dtype=np.uint8)
    args = [None, ctypes.byref(sens) if sensor else None, ctypes.byref(sens_ss) if sensor_ss else None, image[0], image[1],
            *chunk, ss, threshold, 5, buf.ctypes.data if rgb else None, None, None, None]
    rc = (abi.lib.mt_render_chunk_adaptive_device if device else abi.lib.mt_render_chunk_adaptive)(*args)
    return rc, abi.last_error()


@pytest.mark.parametrize("device", [False, True])
def test_argument_checks_come_in_order_before_any_device_call(device):
    abi = M.hip_abi()
    # everything wrong at once: ss speaks first, then the threshold, the output pointer, the image and chunk, the scene
    rc, msg = _call(abi, ss=5, threshold=300, rgb=False, chunk=(0, 0, 9, 9), device=device)
    assert rc == MT_ERR_ARG and "ss 5" in msg
    rc, msg = _call(abi, ss=2, image=(50001, 8), threshold=300, rgb=False, device=device)
    assert rc == MT_ERR_ARG and "sample grid" in msg
    rc, msg = _call(abi, threshold=300, rgb=False, chunk=(0, 0, 9, 9), device=device)
    assert rc == MT_ERR_ARG and "threshold" in msg
    rc, msg = _call(abi, threshold=-1, device=device)
    assert rc == MT_ERR_ARG and "threshold" in msg
    rc, msg = _call(abi, rgb=False, chunk=(0, 0, 9, 9), device=device)
    assert rc == MT_ERR_ARG and msg == ("d_rgb is NULL" if device else "out_rgb is NULL")
    rc, msg = _call(abi, chunk=(0, 0, 9, 9), device=device)
    assert rc == MT_ERR_ARG and "outside image" in msg
    for t in (0, 255):
        rc, msg = _call(abi, threshold=t, sensor=False, sensor_ss=False, device=device)
        assert rc == MT_ERR_ARG and msg == "scene is NULL"


def test_mask_building_block_checks_its_arguments():
    abi = M.hip_abi()
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    f = abi.lib.mt_refine_mask_device
    assert f(None, 8, 8, 0, 0, 8, 8, 256, p, None, p, p, None) == MT_ERR_ARG and "threshold" in abi.last_error()
    assert f(None, 8, 8, 0, 0, 8, 8, 16, None, None, p, p, None) == MT_ERR_ARG and "NULL" in abi.last_error()
    assert f(None, 8, 8, 0, 0, 9, 8, 16, p, None, p, p, None) == MT_ERR_ARG and "outside image" in abi.last_error()
    assert f(None, 8, 8, 0, 0, 8, 8, 16, p, None, p, p, None) == MT_ERR_ARG and abi.last_error() == "scene is NULL"


def test_facade_checks_before_it_needs_a_device():
    m = M.MythTracer()
    m.set_adaptive_supersampling(7, 16)
    with pytest.raises(RuntimeError, match="adaptive supersampling factor 7"):
        m.render(CORNELL_CAM, 8, 8)
    m.set_adaptive_supersampling(2, 300)
    with pytest.raises(RuntimeError, match="threshold 300"):
        m.render_image(CORNELL_CAM, 8, 8)
    m.set_adaptive_supersampling(2, 16)
    with pytest.raises(RuntimeError, match="output_debug"):
        m.render(CORNELL_CAM, 8, 8, debug=True)
    m.set_devices([0, 0])
    with pytest.raises(RuntimeError, match="several devices"):
        m.render_image(CORNELL_CAM, 8, 8)
    # adaptive wins over SetSupersampling: a bad plain factor is not looked at while adaptive is on
    m2 = M.MythTracer()
    m2.set_supersampling(9)
    m2.set_adaptive_supersampling(3, 16)
    with pytest.raises(RuntimeError, match="output_debug is not available with adaptive"):
        m2.render(CORNELL_CAM, 8, 8, debug=True)
    m2.set_adaptive_supersampling(1, 16)  # off: SetSupersampling's factor counts again
    with pytest.raises(RuntimeError, match="supersampling factor 9"):
        m2.render(CORNELL_CAM, 8, 8)
