"""Supersampled frames on a real MI355X (-m gpu): mt_render_chunk_ss, mt_render_chunk_ss_device,
mt_resolve_tiles_device, MythTracer::SetSupersampling (include/mythtracer_hip.h; the resolve kernel is
mythtracer_amd/csrc/mt_resolve.h).

The contract: a supersampled W x H frame IS the frame of the plain calls at s W x s H, box-filtered s x s with the
integer mean of mythtracer_amd/tiling.py's resolve_ss.  Both sides of that statement are this project's own bytes and
the only new arithmetic is an integer mean, so the bar is byte identity, no tolerance.  Against the reference's own
frames (tests/golden/) the bar is the one test_gpu_parity.py has for a frame -- 1 LSB (pow) on at most 0.01 % of the
SAMPLES -- carried through the mean: a rounded mean of bytes moves by at most 1 when each input moves by at most 1,
and a differing sample touches one output pixel, so at most max(1, s*s*W*H // 10000) output pixels may differ by
1 LSB.  The tests print the count (expected: 0).
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
ALL_KEYS = ("rays_primary", "rays_secondary", "rays_shadow", "box_tests", "node_visits", "tri_tests", "mt_tests",
            "shaded_hits")
SIZES = [(96, 64), (101, 67), (37, 3), (1, 1)]  # among them sizes that are no multiples of 4 or 8
RAGGED_CHUNKS = [(0, 0, 1, 1), (159, 89, 1, 1), (3, 5, 7, 5), (150, 0, 10, 90), (0, 80, 160, 10), (8, 8, 8, 8),
                 (13, 27, 65, 33)]


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"


@pytest.fixture(params=["state_machine", "ray_pool", "hybrid", "auto"], autouse=True)
def engine(request):
    """Every test runs through the frame engines and the automatic choice (include/mythtracer_hip.h,
    mt_scene_set_engine), selected through the API for the scenes created from now on."""
    abi = M.hip_abi()
    abi.set_default_engine({"state_machine": 1, "ray_pool": 2, "hybrid": 3, "auto": 0}[request.param])
    yield request.param
    abi.set_default_engine(0)


def view(scene):
    return (CORNELL_CAM, CORNELL_LIGHTS) if scene == "cornell" else (scenegen.ROOM_CAMERA, scenegen.ROOM_LIGHTS)


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def scale(chunk, s):
    return tuple(s * v for v in chunk)


@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("scene", ["cornell", "mini", "room"])
def test_supersampled_chunk_is_the_resolved_sample_frame(scene, s, scenes):
    """mt_render_chunk_ss == resolve_ss(mt_render_chunk at s W x s H with the same sample sensor), byte for byte, and
    the work counted is the sample frame's.  (Both counted launches are the first of their geometry: the call that
    forgets the recorded costs stands between them, so that both take the same work order.)"""
    abi = M.hip_abi()
    cam, lights = view(scene)
    h = abi.scene_create(M.MythTracer(scenes[scene]).flatten())
    try:
        abi.set_lights(h, lights)
        for W, H in SIZES:
            sens = binding.sensor(cam, s * W, s * H)
            got = abi.render_chunk_ss(h, sens, W, H, s)
            abi.set_scheduling(h, True)  # forgets the costs
            samples = abi.render_chunk(h, sens, s * W, s * H)
            assert got["rgb"].shape == (H, W, 3)
            assert np.array_equal(got["rgb"], tiling.resolve_ss(samples["rgb"], s)), (scene, s, W, H)
            print(scene, s, (W, H), {k: (got["stats"][k], samples["stats"][k]) for k in ALL_KEYS})
            assert got["stats"]["rays_primary"] == s * s * W * H
            assert {k: got["stats"][k] for k in ALL_KEYS} == {k: samples["stats"][k] for k in ALL_KEYS}, (scene, s, W, H)
            assert got["stats"]["kernel_ms"] > 0
            again = abi.render_chunk_ss(h, sens, W, H, s)  # (the sample frame's geometry again: on cost history)
            assert np.array_equal(again["rgb"], got["rgb"])
    finally:
        abi.scene_destroy(h)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_supersampled_ragged_chunks(s, scenes):
    """A chunk (cx, cy, cw, ch) of the output image is the chunk (s cx, s cy, s cw, s ch) of the sample frame,
    resolved; a chunk outside the image is an argument error."""
    abi = M.hip_abi()
    h = abi.scene_create(M.MythTracer(scenes["mini"]).flatten())
    try:
        abi.set_lights(h, scenegen.ROOM_LIGHTS)
        W, H = 160, 90
        sens = binding.sensor(scenegen.ROOM_CAMERA, s * W, s * H)
        full = tiling.resolve_ss(abi.render_chunk(h, sens, s * W, s * H)["rgb"], s)
        for chunk in RAGGED_CHUNKS:
            got = abi.render_chunk_ss(h, sens, W, H, s, chunk=chunk)
            abi.set_scheduling(h, True)
            samples = abi.render_chunk(h, sens, s * W, s * H, chunk=scale(chunk, s))
            cx, cy, cw, ch = chunk
            assert got["rgb"].shape == (ch, cw, 3)
            assert np.array_equal(got["rgb"], tiling.resolve_ss(samples["rgb"], s)), (s, chunk)
            assert np.array_equal(got["rgb"], full[cy:cy + ch, cx:cx + cw]), (s, chunk)
            print(s, chunk, {k: (got["stats"][k], samples["stats"][k]) for k in ALL_KEYS})
            assert {k: got["stats"][k] for k in ALL_KEYS} == {k: samples["stats"][k] for k in ALL_KEYS}, (s, chunk)
        for bad in [(-1, 0, 4, 4), (0, 0, 0, 4), (156, 86, 8, 8), (0, 0, 161, 1), (0, 0, 1, 91)]:
            with pytest.raises(RuntimeError, match="outside image"):
                abi.render_chunk_ss(h, sens, W, H, s, chunk=bad)
        for bad_ss in (0, 5):
            with pytest.raises(RuntimeError, match="ss"):
                abi.render_chunk_ss(h, sens, W, H, bad_ss)
    finally:
        abi.scene_destroy(h)


def assert_resolved_close(got, want, n_samples, what):
    """<= 1 LSB on at most max(1, n_samples // 10000) output pixels (this file's docstring)."""
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    n_diff = int((d != 0).any(axis=-1).sum())
    print("%s: %d of %d pixels differ, max |diff| %d" % (what, n_diff, d.shape[0] * d.shape[1], int(d.max(initial=0))))
    assert d.max(initial=0) <= 1, what
    assert n_diff <= max(1, n_samples // 10000), what


@pytest.mark.parametrize("case,scene,s,size", [("cornell_256", "cornell", 2, (128, 128)),
                                               ("mini_320x180", "mini", 2, (160, 90)),
                                               ("room_240x135", "room", 3, (80, 45))])
def test_facade_against_the_reference_frames(case, scene, s, size, scenes):
    """The reference's own full frames, box-filtered, against MythTracer::SetSupersampling + RayTrace."""
    g = np.load(os.path.join(GOLDEN, case + ".npz"), allow_pickle=False)
    W, H = size
    assert tuple(int(v) for v in g["image"]) == (s * W, s * H) and tuple(int(v) for v in g["chunk"]) == (0, 0, s * W, s * H)
    want = tiling.resolve_ss(g["rgb"], s)
    m = M.MythTracer(scenes[scene])
    m.set_lights(g["lights"].reshape(-1, 12))
    m.set_supersampling(s)
    for frame in range(2):  # (the second one runs on cost history)
        r = m.render(g["cam"], W, H)
        assert_resolved_close(r["rgb"], want, s * s * W * H, "%s ss %d frame %d" % (case, s, frame))
        assert r["counters"]["rays_primary"] == s * s * W * H
    assert_resolved_close(m.render_image(g["cam"], W, H), want, s * s * W * H, "%s ss %d image overload" % (case, s))


def test_factor_one_is_the_plain_call(scenes):
    """ss = 1 through the new entry points: the plain call's bytes and counters, one launch, no resolve."""
    import torch
    abi = M.hip_abi()
    h = abi.scene_create(M.MythTracer(scenes["mini"]).flatten())
    try:
        abi.set_lights(h, scenegen.ROOM_LIGHTS)
        W, H = 101, 67
        sens = binding.sensor(scenegen.ROOM_CAMERA, W, H)
        for chunk in (None, (13, 27, 65, 33)):
            abi.set_scheduling(h, True)
            plain = abi.render_chunk(h, sens, W, H, chunk=chunk)
            abi.set_scheduling(h, True)
            abi.kernel_times(h)
            one = abi.render_chunk_ss(h, sens, W, H, 1, chunk=chunk)
            assert len(abi.kernel_times(h)[1]) == 1
            assert np.array_equal(one["rgb"], plain["rgb"])
            assert {k: one["stats"][k] for k in ALL_KEYS} == {k: plain["stats"][k] for k in ALL_KEYS}
        out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        abi.render_chunk_ss_device(h, sens, W, H, (0, 0, W, H), 1, 5, vp(out))
        torch.cuda.synchronize()
        abi.read_stats(h)
        full = abi.render_chunk(h, sens, W, H)["rgb"]
        assert np.array_equal(out.cpu().numpy(), full)
        # resolving with ss = 1 copies the slots
        T = 32
        f, st, n = tiling.rank_tiles(W, H, T, T, 0, 1)
        a = torch.randint(0, 256, (n * tiling.slot_bytes(T, T),), dtype=torch.uint8, device="cuda")
        b = torch.zeros_like(a)
        torch.cuda.synchronize()
        abi.resolve_tiles_device(h, W, H, T, T, f, st, None, n, 1, vp(a), vp(b))
        torch.cuda.synchronize()
        assert torch.equal(a, b)
    finally:
        abi.scene_destroy(h)


@pytest.mark.parametrize("s", [2, 3])
def test_device_call_on_a_stream(s, scenes):
    """mt_render_chunk_ss_device on a torch stream, then a copy to the host: the host call's bytes; twice in a row (the
    second launch runs on cost history) the same bytes."""
    import torch
    abi = M.hip_abi()
    cam, lights = view("room")
    h = abi.scene_create(M.MythTracer(scenes["room"]).flatten())
    try:
        abi.set_lights(h, lights)
        W, H = 101, 67
        sens = binding.sensor(cam, s * W, s * H)
        want = abi.render_chunk_ss(h, sens, W, H, s)["rgb"]
        stream = torch.cuda.Stream()
        outs = [torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(3)]
        part = torch.zeros((33, 65, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for out in outs:
                abi.render_chunk_ss_device(h, sens, W, H, (0, 0, W, H), s, 5, vp(out), ctypes.c_void_p(stream.cuda_stream))
            abi.render_chunk_ss_device(h, sens, W, H, (13, 27, 65, 33), s, 5, vp(part), ctypes.c_void_p(stream.cuda_stream))
            host = [out.cpu().numpy() for out in outs] + [part.cpu().numpy()]
        stream.synchronize()
        abi.read_stats(h)
        for i in range(3):
            assert np.array_equal(host[i], want), i
        assert np.array_equal(host[3], want[27:60, 13:78])
        with pytest.raises(RuntimeError, match="d_rgb is NULL"):
            abi.render_chunk_ss_device(h, sens, W, H, (0, 0, W, H), s, 5, None)
    finally:
        abi.scene_destroy(h)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("s,size,T", [(3, (200, 120), 64), (2, (264, 150), 16), (4, (37, 21), 8)])
def test_tiles_of_the_sample_frame_resolved_and_blitted(s, size, T, world, scenes):
    """The multi-GPU building block, `world` ranks on one GPU with a scene replica each: a rank renders its tiles of
    the SAMPLE frame (modular share, then a dealt list) at (s W, s H, s T, s T), resolves them with
    mt_resolve_tiles_device and blits them with the unchanged blit at (W, H, T, T): the single-launch
    mt_render_chunk_ss frame, byte for byte.  200 x 120 with 64 x 64 tiles: right and bottom tiles clipped."""
    import torch
    abi = M.hip_abi()
    flat = M.MythTracer(scenes["mini"]).flatten()
    W, H = size
    sens = binding.sensor(scenegen.ROOM_CAMERA, s * W, s * H)
    tx, ty = tiling.tile_grid(W, H, T, T)
    total = tx * ty
    assert tiling.tile_grid(s * W, s * H, s * T, s * T) == (tx, ty)
    hs = [abi.scene_create(flat) for _ in range(world + 1)]
    try:
        for hh in hs:
            abi.set_lights(hh, scenegen.ROOM_LIGHTS)
        single = abi.render_chunk_ss(hs[world], sens, W, H, s)["rgb"]
        # modular shares
        frame = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        for r in range(world):
            f, st, n = tiling.rank_tiles(W, H, T, T, r, world)
            samples = torch.zeros(n * tiling.slot_bytes(s * T, s * T), dtype=torch.uint8, device="cuda")
            slots = torch.zeros(n * tiling.slot_bytes(T, T), dtype=torch.uint8, device="cuda")
            abi.render_tiles_device(hs[r], sens, s * W, s * H, s * T, s * T, f, st, n, 5, vp(samples))
            abi.resolve_tiles_device(hs[r], W, H, T, T, f, st, None, n, s, vp(samples), vp(slots))
            abi.blit_tiles_device(hs[r], W, H, T, T, f, st, n, vp(slots), vp(frame))
            torch.cuda.synchronize()
            abi.read_stats(hs[r])
            # the slots are what the numpy restatement makes of the sample slots
            want = np.zeros_like(slots.cpu().numpy())
            smp = samples.cpu().numpy()
            for j in range(n):
                _, _, cw, ch = tiling.tile_rect(f + j * st, W, H, T, T)
                a = smp[j * tiling.slot_bytes(s * T, s * T):][:s * s * cw * ch * 3].reshape(s * ch, s * cw, 3)
                want[j * tiling.slot_bytes(T, T):][:cw * ch * 3] = tiling.resolve_ss(a, s).reshape(-1)
            assert np.array_equal(slots.cpu().numpy(), want), ("slots", r)
        assert np.array_equal(frame.cpu().numpy(), single), "modular"
        # dealt lists, from an order that is not the order by number
        order = torch.arange(total - 1, -1, -1, dtype=torch.int32, device="cuda")
        frame = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        owned = []
        for r in range(world):
            lst = torch.full((total,), -7, dtype=torch.int32, device="cuda")
            n = abi.deal_tiles_device(hs[r], vp(order), W, H, T, T, world, r, vp(lst))
            assert n == tiling.dealt_tile_count(total, world, r)
            lst = lst[:n].contiguous()
            owned += lst.cpu().numpy().tolist()
            samples = torch.zeros(n * tiling.slot_bytes(s * T, s * T), dtype=torch.uint8, device="cuda")
            slots = torch.zeros(n * tiling.slot_bytes(T, T), dtype=torch.uint8, device="cuda")
            for launch in range(2):  # (list_id unchanged: the second launch runs on the slots' cost history)
                abi.render_tile_list_device(hs[r], sens, s * W, s * H, s * T, s * T, vp(lst), n, 7, 5, vp(samples))
            abi.resolve_tiles_device(hs[r], W, H, T, T, 0, 1, vp(lst), n, s, vp(samples), vp(slots))
            abi.blit_tile_list_device(hs[r], W, H, T, T, vp(lst), n, vp(slots), vp(frame))
            torch.cuda.synchronize()
            abi.read_stats(hs[r])
        assert sorted(owned) == list(range(total))
        assert np.array_equal(frame.cpu().numpy(), single), "dealt"
        # argument checks with a real scene
        with pytest.raises(RuntimeError, match="tile selection"):
            abi.resolve_tiles_device(hs[0], W, H, T, T, 0, 1, None, total + 1, s, vp(samples), vp(slots))
        with pytest.raises(RuntimeError, match="same buffer"):
            abi.resolve_tiles_device(hs[0], W, H, T, T, 0, 1, None, 1, s, vp(slots), vp(slots))
        with pytest.raises(RuntimeError, match="NULL"):
            abi.resolve_tiles_device(hs[0], W, H, T, T, 0, 1, None, 1, s, None, vp(slots))
    finally:
        for hh in hs:
            abi.scene_destroy(hh)


def test_facade_supersampling(scenes):
    """MythTracer::SetSupersampling: both RayTrace overloads give the resolved sample frame; a debug buffer is
    refused with a message, and so is the W x H overload on several devices."""
    abi = M.hip_abi()
    W, H, s = 96, 64, 2
    m = M.MythTracer(scenes["mini"])
    m.set_lights(scenegen.ROOM_LIGHTS)
    plain = m.render(scenegen.ROOM_CAMERA, W, H)["rgb"]  # default: one ray per pixel
    samples = m.render(scenegen.ROOM_CAMERA, s * W, s * H)
    want = tiling.resolve_ss(samples["rgb"], s)
    direct = abi.render_chunk_ss(m.device_scene(), binding.sensor(scenegen.ROOM_CAMERA, s * W, s * H), W, H, s)["rgb"]
    assert np.array_equal(direct, want)
    m.set_supersampling(s)
    r = m.render(scenegen.ROOM_CAMERA, W, H)
    assert np.array_equal(r["rgb"], want)
    assert r["counters"]["rays_primary"] == s * s * W * H and r["kernel_ms"] > 0
    assert not np.array_equal(r["rgb"], plain)  # (it is another picture than the aliased one)
    assert np.array_equal(m.render_image(scenegen.ROOM_CAMERA, W, H), want)
    part = m.render(scenegen.ROOM_CAMERA, W, H, chunk=(13, 27, 65, 33))
    assert np.array_equal(part["rgb"], want[27:60, 13:78])
    with pytest.raises(RuntimeError, match="output_debug"):
        m.render(scenegen.ROOM_CAMERA, W, H, debug=True)
    m.set_supersampling(1)
    back = m.render(scenegen.ROOM_CAMERA, W, H, debug=True)
    assert np.array_equal(back["rgb"], plain) and back["line"] is not None
    m.set_supersampling(7)
    with pytest.raises(RuntimeError, match="supersampling factor 7"):
        m.render(scenegen.ROOM_CAMERA, W, H)
    # several devices: refused, never silently rendered on one
    m2 = M.MythTracer(scenes["mini"])
    m2.set_lights(scenegen.ROOM_LIGHTS)
    m2.set_devices([0, 0])
    assert np.array_equal(m2.render_image(scenegen.ROOM_CAMERA, W, H), plain)
    m2.set_supersampling(s)
    with pytest.raises(RuntimeError, match="several devices"):
        m2.render_image(scenegen.ROOM_CAMERA, W, H)
    assert np.array_equal(m2.render(scenegen.ROOM_CAMERA, W, H)["rgb"], want)  # (a WorkChunk stays on the first device)
