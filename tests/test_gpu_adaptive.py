"""Adaptive supersampling on a real MI355X (-m gpu): mt_refine_mask_device, mt_render_chunk_adaptive,
mt_render_chunk_adaptive_device, MythTracer::SetAdaptiveSupersampling (include/mythtracer_hip.h; the kernels are
mythtracer_amd/csrc/mt_adaptive.h).

The contract: every byte of an adaptive chunk is the plain call's byte or the supersampled call's byte, and the block
mask of mythtracer_amd/tiling.py's refine_mask, computed from the plain bytes, decides which.  Both sides are this
project's own bytes and the only new arithmetic is an integer compare, so the bar is byte identity, no tolerance.
Against the reference's own frames the refined pixels carry test_gpu_supersampling.py's bar (1 LSB on at most
max(1, s*s*W*H // 10000) pixels); the unrefined pixels belong to another sensor's rays than those goldens.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding, scenegen, tiling  # noqa: E402

CORNELL_CAM = (50, 50, -120, 0, 0, 0, 60)
CORNELL_LIGHTS = [(50, 90, 50, .3, .3, .3, 1, 1, 1, 1, 1, 1)]
SIZES = [(96, 54), (101, 67), (37, 3)]  # 96 x 54: the bottom blocks are clipped
CHUNKS_160x90 = [(13, 27, 65, 33), (159, 89, 1, 1), (8, 8, 8, 8), (150, 0, 10, 90)]
THRESHOLD = 16


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"


@pytest.fixture(params=["state_machine", "ray_pool", "hybrid", "auto"])
def engine(request):
    """The tests that render run through the frame engines and the automatic choice (mt_scene_set_engine), selected
    through the API for the scenes created from now on."""
    abi = M.hip_abi()
    abi.set_default_engine({"state_machine": 1, "ray_pool": 2, "hybrid": 3, "auto": 0}[request.param])
    yield request.param
    abi.set_default_engine(0)


def view(scene):
    return (CORNELL_CAM, CORNELL_LIGHTS) if scene == "cornell" else (scenegen.ROOM_CAMERA, scenegen.ROOM_LIGHTS)


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def block_areas(tiles, W, H):
    """sum of area(block within the image) over the listed blocks"""
    return sum(cw * ch for _, _, cw, ch in (tiling.tile_rect(int(t), W, H, 8, 8) for t in tiles))


def check_contract(abi, h, cam, W, H, s, threshold, chunk=None, what=None):
    """One adaptive call against compose(plain call, supersampled call, numpy mask); returns (result, mask)."""
    chunk = chunk or (0, 0, W, H)
    s1, ss = binding.sensor(cam, W, H), binding.sensor(cam, s * W, s * H)
    plain = abi.render_chunk(h, s1, W, H, chunk=chunk)["rgb"]
    full = abi.render_chunk_ss(h, ss, W, H, s, chunk=chunk)["rgb"]
    mask, tiles = tiling.refine_mask(plain, W, H, chunk, threshold)
    got = abi.render_chunk_adaptive(h, s1, ss, W, H, s, threshold, chunk=chunk)
    assert np.array_equal(got["mask"], mask), what
    assert got["info"]["n_blocks"] == mask.size and got["info"]["n_refined"] == int(mask.sum()), what
    assert np.array_equal(got["rgb"], tiling.compose_adaptive(plain, full, mask, chunk)), what
    assert got["stats"]["rays_primary"] == chunk[2] * chunk[3] + s * s * block_areas(tiles, W, H), what
    assert got["stats"]["kernel_ms"] > 0 and got["stats"]["total_ms"] > 0
    return got, mask


def test_mask_kernel_against_numpy(scenes):
    """mt_refine_mask_device on bitmaps uploaded with torch: random bytes, and flat frames with planted pairs."""
    import torch
    abi = M.hip_abi()
    h = abi.scene_create(M.MythTracer(scenes["cornell"]).flatten())
    rng = np.random.default_rng(2024)
    cases = [(w, hh, (0, 0, w, hh)) for w, hh in [(96, 64), (101, 67), (37, 3), (1, 1), (8, 8), (9, 9)]]
    cases += [(160, 90, c) for c in CHUNKS_160x90]
    try:
        for W, H, chunk in cases:
            cx, cy, cw, ch = chunk
            noise = rng.integers(0, 256, (ch, cw, 3), dtype=np.uint8)
            near = (100 + rng.integers(0, 18, (ch, cw, 3))).astype(np.uint8)  # differences around threshold 16
            planted = np.full((ch, cw, 3), 100, dtype=np.uint8)
            n = max(1, cw * ch // 40)
            planted[rng.integers(0, ch, n), rng.integers(0, cw, n), rng.integers(0, 3, n)] = rng.integers(0, 256, n)
            planted[ch - 1, cw - 1, 0] = 255  # (a pair at the chunk's last pixel, where there is one)
            _, _, mw, mh = tiling.chunk_blocks(chunk)
            for name, f in (("noise", noise), ("near", near), ("planted", planted)):
                d_rgb = torch.from_numpy(f).cuda()
                for t in (0, 16, 254, 255):
                    want_mask, want_list = tiling.refine_mask(f, W, H, chunk, t)
                    for with_mask in (True, False):
                        d_mask = torch.full((mh * mw,), 9, dtype=torch.uint8, device="cuda")
                        d_list = torch.full((mh * mw,), -7, dtype=torch.int32, device="cuda")
                        d_count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
                        torch.cuda.synchronize()
                        abi.refine_mask_device(h, W, H, chunk, t, vp(d_rgb), vp(d_mask) if with_mask else None,
                                               vp(d_list), vp(d_count))
                        torch.cuda.synchronize()
                        what = (name, W, H, chunk, t, with_mask)
                        count = int(d_count.cpu()[0])
                        got_list = d_list.cpu().numpy()
                        assert count == len(want_list), what
                        assert np.array_equal(got_list[:count], want_list), what
                        assert (np.diff(got_list[:count]) > 0).all() and (got_list[count:] == -7).all(), what
                        if with_mask:
                            assert np.array_equal(d_mask.cpu().numpy().reshape(mh, mw), want_mask.astype(np.uint8)), what
                        else:
                            assert (d_mask.cpu().numpy() == 9).all()
    finally:
        abi.scene_destroy(h)


@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("scene", ["cornell", "mini", "room"])
def test_adaptive_chunk_is_the_composition(scene, s, scenes, engine):
    abi = M.hip_abi()
    cam, lights = view(scene)
    h = abi.scene_create(M.MythTracer(scenes[scene]).flatten())
    try:
        abi.set_lights(h, lights)
        for W, H in SIZES:
            got, mask = check_contract(abi, h, cam, W, H, s, THRESHOLD, what=(scene, s, W, H))
            print(scene, s, (W, H), "refined %d of %d" % (mask.sum(), mask.size), got["info"])
            if scene in ("cornell", "mini") and (W, H) != (37, 3):
                assert 0 < mask.sum() < mask.size, (scene, W, H)
    finally:
        abi.scene_destroy(h)


@pytest.mark.parametrize("s", [2, 3])
def test_adaptive_ragged_chunks(s, scenes, engine):
    """The contract per chunk, with the mask of THAT chunk's plain bytes (pairs across its border do not exist)."""
    abi = M.hip_abi()
    h = abi.scene_create(M.MythTracer(scenes["mini"]).flatten())
    try:
        abi.set_lights(h, scenegen.ROOM_LIGHTS)
        for chunk in CHUNKS_160x90:
            check_contract(abi, h, scenegen.ROOM_CAMERA, 160, 90, s, THRESHOLD, chunk=chunk, what=(s, chunk))
    finally:
        abi.scene_destroy(h)


def test_extremes(scenes, engine):
    abi = M.hip_abi()
    keys = ("rays_primary", "rays_secondary", "rays_shadow", "box_tests", "node_visits", "tri_tests", "mt_tests",
            "shaded_hits")
    h = abi.scene_create(M.MythTracer(scenes["cornell"]).flatten())
    try:
        abi.set_lights(h, CORNELL_LIGHTS)
        W, H = 101, 67
        s1, ss = binding.sensor(CORNELL_CAM, W, H), binding.sensor(CORNELL_CAM, 2 * W, 2 * H)
        abi.set_scheduling(h, True)
        plain = abi.render_chunk(h, s1, W, H)
        # threshold 255: nothing is refined, one launch
        abi.kernel_times(h)
        got = abi.render_chunk_adaptive(h, s1, ss, W, H, 2, 255)
        assert len(abi.kernel_times(h)[1]) == 1
        assert np.array_equal(got["rgb"], plain["rgb"]) and not got["mask"].any()
        assert got["info"]["n_refined"] == 0 and got["info"]["refine_history"] == 0
        # threshold 0: nearly everything, two launches
        got, mask = check_contract(abi, h, CORNELL_CAM, W, H, 2, 0)
        print("threshold 0: refined %d of %d" % (mask.sum(), mask.size))
        assert mask.mean() > 0.5
        abi.kernel_times(h)
        abi.render_chunk_adaptive(h, s1, ss, W, H, 2, 0)
        assert len(abi.kernel_times(h)[1]) == 2
        # ss 1: the plain call's bytes and counters (both the first launch of their geometry)
        abi.set_scheduling(h, True)
        plain = abi.render_chunk(h, s1, W, H)
        abi.set_scheduling(h, True)
        abi.kernel_times(h)
        one = abi.render_chunk_adaptive(h, s1, None, W, H, 1, THRESHOLD)
        assert len(abi.kernel_times(h)[1]) == 1
        assert np.array_equal(one["rgb"], plain["rgb"]) and not one["mask"].any() and one["info"]["n_refined"] == 0
        assert {k: one["stats"][k] for k in keys} == {k: plain["stats"][k] for k in keys}
        with pytest.raises(RuntimeError, match="sensor_ss"):
            abi.render_chunk_adaptive(h, s1, None, W, H, 2, THRESHOLD)
    finally:
        abi.scene_destroy(h)


def yawed(cam, deg):
    c = list(cam)
    c[4] += deg  # (x, y, z, pitch, yaw, roll, aov)
    return tuple(c)


def test_two_launches_two_histories(scenes):
    """The plain launch and the refinement launch keep their own cost histories, and a plain frame in between sees
    the one a plain frame would have left.  (Automatic engine: the default.)"""
    abi = M.hip_abi()
    h = abi.scene_create(M.MythTracer(scenes["mini"]).flatten())
    try:
        abi.set_lights(h, scenegen.ROOM_LIGHTS)
        W, H, s = 101, 67, 2
        cam = scenegen.ROOM_CAMERA
        s1, ss = binding.sensor(cam, W, H), binding.sensor(cam, s * W, s * H)
        r = [abi.render_chunk_adaptive(h, s1, ss, W, H, s, THRESHOLD) for _ in range(4)]
        print([q["info"] for q in r])
        assert r[0]["info"]["plain_history"] == 0
        assert all(q["info"]["plain_history"] == 1 for q in r[1:])
        assert all(q["info"]["refine_history"] == 1 for q in r[2:])
        assert all(np.array_equal(q["rgb"], r[0]["rgb"]) and np.array_equal(q["mask"], r[0]["mask"]) for q in r[1:])
        plain = abi.render_chunk(h, s1, W, H)["rgb"]
        keep = ~np.repeat(np.repeat(r[0]["mask"], 8, axis=0), 8, axis=1)[:H, :W]
        assert np.array_equal(plain[keep], r[0]["rgb"][keep])  # (the plain pass's bytes, where they survive)
        assert np.array_equal(tiling.refine_mask(plain, W, H, None, THRESHOLD)[0], r[0]["mask"])
        after = abi.render_chunk_adaptive(h, s1, ss, W, H, s, THRESHOLD)
        assert after["info"]["plain_history"] == 1 and after["info"]["refine_history"] == 1
        assert np.array_equal(after["rgb"], r[0]["rgb"])
        cam2 = yawed(cam, 2.0)
        moved = abi.render_chunk_adaptive(h, binding.sensor(cam2, W, H), binding.sensor(cam2, s * W, s * H), W, H, s,
                                          THRESHOLD)
        assert not np.array_equal(moved["mask"], r[0]["mask"]), "the yawed camera was to give another list"
        assert moved["info"]["plain_history"] == 1  # (a re-projected history is a history)
        assert moved["info"]["refine_history"] == 0
        abi.set_scheduling(h, True)
        fresh = abi.render_chunk_adaptive(h, s1, ss, W, H, s, THRESHOLD)
        assert fresh["info"]["plain_history"] == 0 and fresh["info"]["refine_history"] == 0
        assert np.array_equal(fresh["rgb"], r[0]["rgb"])
    finally:
        abi.scene_destroy(h)


def test_device_call_on_a_stream(scenes, engine):
    import torch
    abi = M.hip_abi()
    cam, lights = view("room")
    h = abi.scene_create(M.MythTracer(scenes["room"]).flatten())
    try:
        abi.set_lights(h, lights)
        W, H, s = 101, 67, 2
        s1, ss = binding.sensor(cam, W, H), binding.sensor(cam, s * W, s * H)
        want = abi.render_chunk_adaptive(h, s1, ss, W, H, s, THRESHOLD)
        sub = (13, 27, 65, 33)
        want_sub = abi.render_chunk_adaptive(h, s1, ss, W, H, s, THRESHOLD, chunk=sub)
        stream = torch.cuda.Stream()
        outs = [torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
        masks = [torch.full(want["mask"].shape, 9, dtype=torch.uint8, device="cuda") for _ in range(2)]
        part = torch.zeros((33, 65, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        sp = ctypes.c_void_p(stream.cuda_stream)
        with torch.cuda.stream(stream):
            infos = [abi.render_chunk_adaptive_device(h, s1, ss, W, H, (0, 0, W, H), s, THRESHOLD, 5, vp(o), vp(m), sp)
                     for o, m in zip(outs, masks)]
            infos.append(abi.render_chunk_adaptive_device(h, s1, ss, W, H, sub, s, THRESHOLD, 5, vp(part), None, sp))
            host = [o.cpu().numpy() for o in outs] + [part.cpu().numpy()]
            host_masks = [m.cpu().numpy() for m in masks]
        stream.synchronize()
        abi.read_stats(h)
        for i in range(2):
            assert np.array_equal(host[i], want["rgb"]), i
            assert np.array_equal(host_masks[i].astype(bool), want["mask"]), i
            assert infos[i]["n_refined"] == want["info"]["n_refined"]
        assert np.array_equal(host[2], want_sub["rgb"]) and infos[2]["n_refined"] == want_sub["info"]["n_refined"]
        with pytest.raises(RuntimeError, match="d_rgb is NULL"):
            abi.render_chunk_adaptive_device(h, s1, ss, W, H, (0, 0, W, H), s, THRESHOLD, 5, None)
    finally:
        abi.scene_destroy(h)


def test_facade_adaptive_supersampling(scenes, engine):
    abi = M.hip_abi()
    W, H, s = 96, 64, 2
    cam = scenegen.ROOM_CAMERA
    m = M.MythTracer(scenes["mini"])
    m.set_lights(scenegen.ROOM_LIGHTS)
    plain = m.render(cam, W, H)["rgb"]
    s1, ss = binding.sensor(cam, W, H), binding.sensor(cam, s * W, s * H)

    def contract(chunk):
        p = abi.render_chunk(m.device_scene(), s1, W, H, chunk=chunk)["rgb"]
        f = abi.render_chunk_ss(m.device_scene(), ss, W, H, s, chunk=chunk)["rgb"]
        mask, tiles = tiling.refine_mask(p, W, H, chunk, THRESHOLD)
        return tiling.compose_adaptive(p, f, mask, chunk), tiles

    want, tiles = contract((0, 0, W, H))
    assert not np.array_equal(want, plain)
    m.set_supersampling(3)  # adaptive wins
    m.set_adaptive_supersampling(s, THRESHOLD)
    r = m.render(cam, W, H)
    assert np.array_equal(r["rgb"], want)
    assert r["counters"]["rays_primary"] == W * H + s * s * block_areas(tiles, W, H) and r["kernel_ms"] > 0
    assert np.array_equal(m.render_image(cam, W, H), want)
    sub = (13, 27, 65, 33)
    assert np.array_equal(m.render(cam, W, H, chunk=sub)["rgb"], contract(sub)[0])
    with pytest.raises(RuntimeError, match="output_debug"):
        m.render(cam, W, H, debug=True)
    m.set_supersampling(1)
    m.set_adaptive_supersampling(1, THRESHOLD)  # off
    back = m.render(cam, W, H, debug=True)
    assert np.array_equal(back["rgb"], plain) and back["line"] is not None
    m2 = M.MythTracer(scenes["mini"])
    m2.set_lights(scenegen.ROOM_LIGHTS)
    m2.set_devices([0, 0])
    m2.set_adaptive_supersampling(s, THRESHOLD)
    with pytest.raises(RuntimeError, match="several devices"):
        m2.render_image(cam, W, H)
    assert np.array_equal(m2.render(cam, W, H)["rgb"], want)  # (a WorkChunk stays on the first device)


@pytest.mark.parametrize("case,scene,s,size", [("cornell_256", "cornell", 2, (128, 128)),
                                               ("mini_320x180", "mini", 2, (160, 90))])
def test_refined_pixels_against_the_reference_frames(case, scene, s, size, scenes, engine):
    """The reference's own frame at s W x s H, box-filtered, on the refined pixels."""
    g = np.load(os.path.join(GOLDEN, case + ".npz"), allow_pickle=False)
    W, H = size
    assert tuple(int(v) for v in g["image"]) == (s * W, s * H)
    want = tiling.resolve_ss(g["rgb"], s)
    abi = M.hip_abi()
    h = abi.scene_create(M.MythTracer(scenes[scene]).flatten())
    try:
        abi.set_lights(h, g["lights"].reshape(-1, 12))
        got = abi.render_chunk_adaptive(h, binding.sensor(g["cam"], W, H), binding.sensor(g["cam"], s * W, s * H), W, H,
                                        s, THRESHOLD)
        px = np.repeat(np.repeat(got["mask"], 8, axis=0), 8, axis=1)[:H, :W]
        assert 0 < px.sum() < px.size
        d = np.abs(got["rgb"].astype(np.int16) - want.astype(np.int16))[px]
        n_diff = int((d != 0).any(axis=-1).sum())
        print("%s ss %d: %d of %d refined pixels differ, max |diff| %d" % (case, s, n_diff, px.sum(), int(d.max(initial=0))))
        assert d.max(initial=0) <= 1
        assert n_diff <= max(1, s * s * W * H // 10000)
    finally:
        abi.scene_destroy(h)


def test_argument_checks_in_order():
    """Without a scene: a bad ss fails before a bad threshold, a bad threshold before a NULL output."""
    abi = M.hip_abi()
    sens = binding.mt_sensor()
    buf = np.zeros(64, dtype=np.uint8)

    def call(ss, threshold, rgb):
        rc = abi.lib.mt_render_chunk_adaptive(None, ctypes.byref(sens), ctypes.byref(sens), 8, 8, 0, 0, 8, 8, ss, threshold,
                                              5, rgb, None, None, None)
        assert rc == -1
        return abi.last_error()

    assert "ss 7" in call(7, 300, None)
    assert "threshold" in call(2, 300, None)
    assert call(2, 16, None) == "out_rgb is NULL"
    assert call(2, 16, buf.ctypes.data) == "scene is NULL"
