"""The light-buffer update on a real MI355X (-m gpu): mt_update_lightbuffer[_device], MythTracer::UpdateLightBuffer
(include/mythtracer_hip.h; the kernel is lightbuffer_update_kernel in mythtracer_amd/csrc/mt_lightbuffer.h).

The bar is identity, no tolerance: after set_lights(B), planes made under A and updated at the moved indices are
mt_render_lightbuffer's planes under B (power as uint64 views with NaN = NaN, in_shadow byte for byte) and the
restatement's (tests/lightbuffer_ref.py); the planes of the other lights keep every byte.  The moves are those of
tests/lightupdate_ref.py, which tests/test_lightupdate_cpu.py shows to be worth testing.  Every test prints its counts.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gbuffer_ref  # noqa: E402
import lightbuffer_ref as lr  # noqa: E402
import lightupdate_ref as lu  # noqa: E402
import orclib  # noqa: E402
from gbuffer_ref import same_bits  # noqa: E402

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding, scenegen  # noqa: E402

W, H = 96, 54
OFF_GRID = lu.OFF_GRID  # (5, 3, 61, 37): neither origin nor size a multiple of 8
UPDATE = binding.UPDATE_GBUFFER_PLANES
RELIGHT = binding.RELIGHT_GBUFFER_PLANES
MT_ERR_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"


class Scene:
    def __init__(self, obj):
        self.abi = M.hip_abi()
        self.flat = M.MythTracer(obj).flatten()
        self.h = self.abi.scene_create(self.flat)
        self.n_lights = 0

    def close(self):
        self.abi.scene_destroy(self.h)

    def set_lights(self, lights):
        self.abi.set_lights(self.h, lights)
        self.n_lights = len(lights)

    def lightbuffer(self, cam, w, h, chunk=None, channels=None, gbuffer_channels=UPDATE):
        return self.abi.render_lightbuffer(self.h, binding.sensor(cam, w, h), w, h, self.n_lights, chunk=chunk,
                                           channels=channels, gbuffer_channels=gbuffer_channels)

    def update(self, gb, lb, idx, planes=("power", "in_shadow")):
        """mt_update_lightbuffer on COPIES of lb's planes."""
        return self.abi.update_lightbuffer(self.h, gb, {n: lb[n].copy() for n in planes}, idx)

    def frame0(self, cam, w, h, chunk=None):
        return self.abi.render_chunk(self.h, binding.sensor(cam, w, h), w, h, chunk=chunk, max_depth=0)


@pytest.fixture
def make(scenes):
    made = []

    def _make(name):
        made.append(Scene(scenes[name]))
        return made[-1]
    yield _make
    for s in made:
        s.close()


def differing(a, b, what):
    n = int((a != b).any(axis=-1).sum())
    print("%s: %d of %d pixels differ" % (what, n, a.shape[0] * a.shape[1]))
    return n


def assert_planes_equal(got, want, what, planes=("power", "in_shadow")):
    if "power" in planes:
        assert same_bits(got["power"], want["power"], what + " power") == 0, what
    if "in_shadow" in planes:
        n = int((got["in_shadow"] != want["in_shadow"]).sum())
        print("%s in_shadow: %d of %d elements differ" % (what, n, want["in_shadow"].size))
        assert n == 0, what


def bench_moved(indices):
    """The bench lights with the listed ones moved (inside the room's box), each to a place of its own."""
    b = lr.BENCH_LIGHTS
    for i in indices:
        b = lu.moved(b, i, (150.0 + 40.0 * i, 120.0 - 15.0 * i, 250.0 - 60.0 * i))
    return b


@pytest.mark.parametrize("scene", list(lu.MOVES))
def test_contract_against_a_fresh_buffer(scene, scenes, make):
    """Planes under A + the G-buffer of the same launch, set_lights(B), update [moved] == a fresh buffer under B == the
    restatement; rays_shadow = the restatement's iterations of the listed light; no primary ray."""
    orc = orclib.OracleScene(scenes[scene])
    cam = lr.CAMERAS[scene]
    a, b, mv = lu.lights_before_and_after(scene)
    s = make(scene)
    for chunk in (None, OFF_GRID):
        what = "%s %s" % (scene, chunk)
        s.set_lights(a)
        old = s.lightbuffer(cam, W, H, chunk=chunk)
        s.set_lights(b)
        got = s.update(old, old, [mv])
        fresh = s.lightbuffer(cam, W, H, chunk=chunk)
        assert_planes_equal(got, fresh, what + " vs a fresh buffer")
        want = lr.ref_lightbuffer(orc, gbuffer_ref.oracle_gbuffer(orc, cam, W, H, chunk), b)
        assert_planes_equal(got, want, what + " vs the restatement")
        changed = int((old["in_shadow"][mv] != got["in_shadow"][mv]).sum())
        st = got["stats"]
        print(what, "rays_shadow", st["rays_shadow"], int(want["iterations"][mv].sum()), "in_shadow changed in", changed,
              "kernel_ms %.3f" % st["kernel_ms"])
        assert changed > 0
        assert st["rays_shadow"] == int(want["iterations"][mv].sum())
        assert st["rays_primary"] == 0 and st["shaded_hits"] == 0 and st["rays_secondary"] == 0
        assert st["kernel_ms"] > 0 and st["total_ms"] >= st["kernel_ms"] and st["node_visits"] > 0


def test_subsets_and_order(make):
    s = make("room")
    cam = scenegen.ROOM_CAMERA
    s.set_lights(lr.BENCH_LIGHTS)
    old = s.lightbuffer(cam, W, H)
    s.set_lights(bench_moved([0, 2]))
    fresh = s.lightbuffer(cam, W, H)
    both = s.update(old, old, [2, 0])
    one = s.update(old, old, [0])
    assert (one["in_shadow"][2] == old["in_shadow"][2]).all() and (one["in_shadow"][0] != old["in_shadow"][0]).any()
    two = s.update(old, one, [2])
    assert_planes_equal(both, two, "[2, 0] vs [0] then [2]")
    assert_planes_equal(both, fresh, "[2, 0] vs fresh")
    assert both["stats"]["rays_shadow"] == one["stats"]["rays_shadow"] + two["stats"]["rays_shadow"]
    # all three: a whole fresh buffer, whatever the arrays held
    s.set_lights(bench_moved([0, 1, 2]))
    junk = dict(power=np.full_like(old["power"], 7.25), in_shadow=np.full_like(old["in_shadow"], 77))
    allthree = s.update(old, junk, [1, 2, 0])
    assert_planes_equal(allthree, s.lightbuffer(cam, W, H), "all three vs fresh")


def test_unlisted_planes_are_untouched_in_both_forms(make):
    import torch
    s = make("room")
    cam = scenegen.ROOM_CAMERA
    s.set_lights(lr.BENCH_LIGHTS)
    old = s.lightbuffer(cam, W, H, chunk=OFF_GRID)
    ch, cw = old["material"].shape
    s.set_lights(bench_moved([1]))
    fresh = s.lightbuffer(cam, W, H, chunk=OFF_GRID)
    # host form: sentinels in the caller's arrays, updated in place
    lb = dict(power=np.full((3, ch, cw, 3), 7.25), in_shadow=np.full((3, ch, cw), 77, dtype=np.uint8))
    out = s.abi.update_lightbuffer(s.h, old, lb, [1])
    assert out["power"] is lb["power"] and out["in_shadow"] is lb["in_shadow"]
    for l in (0, 2):
        assert (lb["power"][l] == 7.25).all() and (lb["in_shadow"][l] == 77).all()
    assert same_bits(lb["power"][1], fresh["power"][1], "host form, listed plane") == 0
    assert np.array_equal(lb["in_shadow"][1], fresh["in_shadow"][1])
    # device form
    d_gb = dict(point=torch.from_numpy(old["point"]).cuda(), material=torch.from_numpy(old["material"]).cuda())
    d_lb = dict(power=torch.full((3, ch, cw, 3), 7.25, dtype=torch.float64, device="cuda"),
                in_shadow=torch.full((3, ch, cw), 77, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    s.abi.update_lightbuffer_device(s.h, cw, ch, {n: t.data_ptr() for n, t in d_gb.items()},
                                    {n: t.data_ptr() for n, t in d_lb.items()}, [1])
    torch.cuda.synchronize()
    power, shadow = d_lb["power"].cpu().numpy(), d_lb["in_shadow"].cpu().numpy()
    for l in (0, 2):
        assert (power[l] == 7.25).all() and (shadow[l] == 77).all()
    assert same_bits(power[1], fresh["power"][1], "device form, listed plane") == 0
    assert np.array_equal(shadow[1], fresh["in_shadow"][1])
    assert np.array_equal(d_gb["material"].cpu().numpy(), old["material"])  # gb is read, not written
    assert same_bits(d_gb["point"].cpu().numpy(), old["point"], "device form, point untouched") == 0
    print("unlisted planes: 2 x %d sentinel values and bytes intact in both forms" % (ch * cw))


def test_plane_subsets(make):
    s = make("room")
    cam = scenegen.ROOM_CAMERA
    s.set_lights(lr.BENCH_LIGHTS)
    old = s.lightbuffer(cam, W, H)
    s.set_lights(bench_moved([1]))
    fresh = s.lightbuffer(cam, W, H)
    for sub in (("power",), ("in_shadow",)):
        got = s.update(old, old, [1], planes=sub)
        assert set(got) == set(sub) | {"stats"}
        assert_planes_equal(got, fresh, "only %s" % sub[0], planes=sub)
        assert got["stats"]["rays_shadow"] > 0


def test_nine_indices_travel_through_device_memory(make):
    lights = [(40.0 * i, 150.0 + 10 * i, 380.0 - 40 * i, 0.02, 0.01 * i, 0.03, 0.2, 0.15, 0.1 + 0.02 * i, 0.1, 0.2, 0.1)
              for i in range(9)]
    new = [(380.0 - 40.0 * i, 100.0 + 12 * i, 30.0 + 35 * i) + l[3:] for i, l in enumerate(lights)]
    s = make("mini")
    cam = lr.CAMERAS["mini"]
    s.set_lights(lights)
    old = s.lightbuffer(cam, W, H)
    s.set_lights(new)
    fresh = s.lightbuffer(cam, W, H)
    order = [4, 8, 0, 6, 2, 7, 1, 5, 3]
    got = s.update(old, old, order)
    assert_planes_equal(got, fresh, "nine lights, scrambled")
    assert (got["in_shadow"] != old["in_shadow"]).any()
    assert got["stats"]["rays_shadow"] == fresh["stats"]["rays_shadow"]


def test_foreign_material_plane(make):
    """Indices outside the scene's materials: 255 and NaN there (mt_shade_direct's rule), everything else as fresh."""
    s = make("room")
    cam = scenegen.ROOM_CAMERA
    n_m = len(s.flat["materials"])
    s.set_lights(lr.BENCH_LIGHTS)
    old = s.lightbuffer(cam, W, H)
    s.set_lights(bench_moved([1]))
    fresh = s.lightbuffer(cam, W, H)
    material = old["material"].copy()
    foreign = np.zeros(material.shape, dtype=bool)
    foreign[::3, ::5] = True
    foreign &= material >= 0
    values = np.array([n_m, n_m + 1, 1000, 2 ** 31 - 1, -2, -(2 ** 31)], dtype=np.int32)
    material[foreign] = values[np.arange(int(foreign.sum())) % len(values)]
    got = s.update(dict(point=old["point"], material=material), old, [1])
    print("foreign material plane: %d of %d pixels, %d materials in the scene" % (int(foreign.sum()), foreign.size, n_m))
    assert foreign.sum() > 50
    assert (got["in_shadow"][1][foreign] == 255).all() and np.isnan(got["power"][1][foreign]).all()
    assert np.array_equal(got["in_shadow"][1][~foreign], fresh["in_shadow"][1][~foreign])
    assert same_bits(got["power"][1][~foreign], fresh["power"][1][~foreign], "outside the foreign pixels") == 0


def test_degenerate_chunks(make):
    s = make("mini_nomtl")
    s.set_lights(lr.BENCH_LIGHTS)
    old = s.lightbuffer(scenegen.ROOM_CAMERA, W, H)
    s.set_lights(bench_moved([1]))
    junk = dict(power=np.zeros_like(old["power"]), in_shadow=np.zeros_like(old["in_shadow"]))
    got = s.update(old, junk, [1])
    assert (got["in_shadow"][1] == 255).all() and np.isnan(got["power"][1]).all()
    assert got["stats"]["rays_shadow"] == 0 and got["stats"]["node_visits"] == 0
    r = make("room")
    cam = scenegen.ROOM_CAMERA
    for chunk in ((40, 20, 1, 1), (40, 20, 9, 9)):  # 9x9: the edge blocks hold one live lane
        r.set_lights(lr.BENCH_LIGHTS)
        old = r.lightbuffer(cam, W, H, chunk=chunk)
        r.set_lights(bench_moved([0, 1, 2]))
        got = r.update(old, old, [0, 1, 2])
        fresh = r.lightbuffer(cam, W, H, chunk=chunk)
        assert_planes_equal(got, fresh, "chunk %s" % (chunk,))
        assert got["stats"]["rays_shadow"] == fresh["stats"]["rays_shadow"] > 0


def test_list_checks_in_order(make):
    """Checks 6 and 7 of the header (they read the scene's light count); 5 before them, the chunk before all three."""
    s = make("mini")
    s.set_lights(lr.BENCH_LIGHTS)
    gb = dict(point=np.zeros((8, 8, 3)), material=np.zeros((8, 8), dtype=np.int32))
    lb = dict(power=np.zeros((3, 8, 8, 3)))
    for idx, text in (([3], "light index 3 outside the scene's 3 lights"), ([0, -1], "light index -1 outside"),
                      ([1, 2, 1], "light index 1 is listed twice"), ([2, 2, 7], "light index 7 outside"),
                      ([], "bad light index list")):
        with pytest.raises(RuntimeError, match=text):
            s.abi.update_lightbuffer(s.h, gb, lb, idx)
        d = {n: a.ctypes.data for n, a in gb.items()}  # (never read: the call is refused first)
        with pytest.raises(RuntimeError, match=text):
            s.abi.update_lightbuffer_device(s.h, 8, 8, d, dict(power=lb["power"].ctypes.data), idx)
    with pytest.raises(RuntimeError, match="chunk size 0x8 out of range"):
        s.abi.update_lightbuffer_device(s.h, 0, 8, d, dict(power=lb["power"].ctypes.data), [5, 5])
    assert (lb["power"] == 0).all()


def test_device_calls_on_a_stream_then_a_relight(make):
    import torch
    s = make("room")
    cam = scenegen.ROOM_CAMERA
    w, h = 101, 67
    sens = binding.sensor(cam, w, h)
    a, b = lr.BENCH_LIGHTS, bench_moved([1])
    stream = torch.cuda.Stream()
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    g = dict(point=f64(h, w, 3), normal=f64(h, w, 3), albedo=f64(h, w, 3),
             material=torch.zeros((h, w), dtype=torch.int32, device="cuda"))
    lb = dict(power=f64(3, h, w, 3), in_shadow=torch.full((3, h, w), 77, dtype=torch.uint8, device="cuda"))
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    gp = {n: t.data_ptr() for n, t in g.items()}
    lp = {n: t.data_ptr() for n, t in lb.items()}
    s.set_lights(a)
    torch.cuda.synchronize()
    s.abi.read_stats(s.h)
    with torch.cuda.stream(stream):
        sp = ctypes.c_void_p(stream.cuda_stream)
        s.abi.render_lightbuffer_device(s.h, sens, w, h, (0, 0, w, h), lp, gp, sp)
        stream.synchronize()  # (set_lights uploads synchronously: the buffer under A must be finished first)
        made = s.abi.read_stats(s.h)
        s.set_lights(b)
        s.abi.update_lightbuffer_device(s.h, w, h, {n: gp[n] for n in UPDATE}, lp, [1], sp)
        s.abi.shade_direct_device(s.h, sens, w, h, (0, 0, w, h), gp, lp, b, rgb.data_ptr(), sp)
    stream.synchronize()
    st = s.abi.read_stats(s.h)
    fresh = s.lightbuffer(cam, w, h)
    frame = s.frame0(cam, w, h)["rgb"]
    print("stream: rays_primary", made["rays_primary"], "then", st["rays_primary"], "rays_shadow", st["rays_shadow"])
    assert made["rays_primary"] == w * h and st["rays_primary"] == 0 and st["rays_shadow"] > 0
    assert_planes_equal({n: t.cpu().numpy() for n, t in lb.items()}, fresh, "device calls on a stream")
    assert differing(rgb.cpu().numpy(), frame, "relit after the update vs mt_render_chunk under B") == 0


@pytest.mark.parametrize("layout", [0, 1])
def test_deep_layout(layout, scenes, make):
    """An octree of 16 levels, both settings of MT_TUNE_DEEP_LAYOUT: the DEEP instantiations of the kernel."""
    w, h = 48, 27
    s = make("loft")
    assert s.flat["tree_depth"] >= 16
    s.abi.set_tuning(s.h, "DEEP_LAYOUT", float(layout))
    cam = scenegen.ROOM_CAMERA
    b = bench_moved([1])
    s.set_lights(lr.BENCH_LIGHTS)
    old = s.lightbuffer(cam, w, h)
    s.set_lights(b)
    got = s.update(old, old, [1])
    assert_planes_equal(got, s.lightbuffer(cam, w, h), "loft, layout %d, vs fresh" % layout)
    orc = orclib.OracleScene(scenes["loft"])
    want = lr.ref_lightbuffer(orc, gbuffer_ref.oracle_gbuffer(orc, cam, w, h), b)
    assert_planes_equal(got, want, "loft, layout %d, vs the restatement" % layout)
    assert got["stats"]["rays_shadow"] == int(want["iterations"][1].sum())


def test_frame_kernels_are_untouched_by_the_update(make):
    """The recipe of test_gpu_lightbuffer.py: a depth-5 frame before and after is byte-identical, the update adds no
    entry to mt_scene_kernel_times, and the second frame is the repeated launch it would have been."""
    w, h = 1920, 1080
    cam = scenegen.ROOM_CAMERA
    sens = binding.sensor(cam, w, h)
    s = make("room")
    s.set_lights(lr.BENCH_LIGHTS)
    s.abi.set_engine(s.h, 1)
    s.abi.kernel_times(s.h)
    old = s.lightbuffer(cam, w, h)  # (before the first frame: as the existing test shows, it leaves no trace either)
    s.abi.kernel_times(s.h)
    f1 = s.abi.render_chunk(s.h, sens, w, h)["rgb"]
    got = s.update(old, old, [0, 2])  # same lights: the planes must not change either
    f2 = s.abi.render_chunk(s.h, sens, w, h)["rgb"]
    assert np.array_equal(f1, f2)
    assert_planes_equal(got, old, "update under unchanged lights")
    pm, rm = s.abi.kernel_times(s.h)
    print("primary_ms", pm, "render_ms", rm)
    assert len(pm) == 2, pm
    assert pm[1] < pm[0] / 3, pm  # second frame: the order kernels, not primary_kernel (see test_gpu_gbuffer.py)


def test_facade_and_python_round_trip(scenes, make, tmp_path):
    """MythTracer.update_lightbuffer (UpdateLightBuffer through the ctypes shim) and a C++ program against the facade's
    headers (tests/seam/lightupdate_driver.cc)."""
    from mythtracer_amd import build
    cam = lr.CAMERAS["mini"]
    w, h = 61, 37
    a, b, mv = lr.BENCH_LIGHTS, bench_moved([1]), 1
    s = make("mini")
    s.set_lights(b)
    want = s.lightbuffer(cam, w, h)
    m = M.MythTracer(scenes["mini"])
    m.set_lights(a)
    old = m.lightbuffer(cam, w, h)
    keys = set(old)
    kept = {n: old[n].copy() for n in ("power", "in_shadow")}
    m.set_lights(b)
    got = m.update_lightbuffer(old, old, [mv])
    assert set(got) == {"power", "in_shadow", "counters", "kernel_ms", "total_ms"} and set(old) == keys
    assert_planes_equal(got, want, "facade")
    assert_planes_equal(old, kept, "facade: the arguments are unchanged")
    assert got["counters"]["rays_primary"] == 0 and got["kernel_ms"] > 0
    assert got["counters"]["rays_shadow"] == s.update(want, want, [mv])["stats"]["rays_shadow"]
    only = m.update_lightbuffer(old, dict(in_shadow=old["in_shadow"]), [mv])
    assert set(only) == {"in_shadow", "counters", "kernel_ms", "total_ms"}
    assert np.array_equal(only["in_shadow"], want["in_shadow"])
    m.set_max_level(0)
    assert differing(m.relight(cam, w, h, old, got)["rgb"], m.render(cam, w, h)["rgb"], "facade: relit after the update") == 0
    # the C++ driver
    exe = str(tmp_path / "lightupdate_driver")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "seam", "lightupdate_driver.cc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(build.HOST, "include"), "-I", build.INC,
                           "-o", exe, src, "-L", build.LIB, "-lmythtracer_host", "-lmythtracer_hip",
                           "-Wl,-rpath," + build.LIB])
    out = str(tmp_path / "u.bin")
    args = [exe, scenes["mini"], str(w), str(h)] + [repr(float(c)) for c in cam] + [str(len(a))]
    args += [repr(float(v)) for l in a for v in l] + [str(mv)] + [repr(float(v)) for v in b[mv][:3]] + [out]
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode().split() == ["primary", "0", "shadow", str(got["counters"]["rays_shadow"])]
    raw = open(out, "rb").read()
    n, nl = w * h, len(a)
    assert len(raw) == 2 * nl * n * 25 + 2 * n * 3
    planes = []
    for k in range(2):  # the updated buffer, then a fresh one under the moved light
        off = k * nl * n * 25
        planes.append(dict(power=np.frombuffer(raw, dtype=np.float64, count=nl * n * 3, offset=off).reshape(nl, h, w, 3),
                           in_shadow=np.frombuffer(raw, dtype=np.uint8, count=nl * n, offset=off + nl * n * 24).reshape(nl, h, w)))
    assert_planes_equal(planes[0], want, "C++ driver, updated")
    assert_planes_equal(planes[1], want, "C++ driver, fresh")
    frames = np.frombuffer(raw, dtype=np.uint8, offset=2 * nl * n * 25).reshape(2, h, w, 3)
    assert differing(frames[0], frames[1], "driver: ShadeDirect after the update vs RayTrace at level 0") == 0
    assert differing(frames[0], s.frame0(cam, w, h)["rgb"], "driver vs mt_render_chunk") == 0


def test_updating_one_light_costs_less_than_the_whole_buffer_at_1080p(make):
    w, h = 1920, 1080
    cam = scenegen.ROOM_CAMERA
    s = make("room")
    s.set_lights(lr.BENCH_LIGHTS)
    old = s.lightbuffer(cam, w, h)  # (warms the process up, and is the input)
    s.set_lights(bench_moved([1]))
    s.update(old, old, [1])
    whole = s.lightbuffer(cam, w, h)
    got = s.update(old, old, [1])
    print("1080p room, 3 lights: lightbuffer_kernel %.3f ms, update of one light %.3f ms"
          % (whole["stats"]["kernel_ms"], got["stats"]["kernel_ms"]))
    assert_planes_equal(got, whole, "1080p")
    assert got["stats"]["kernel_ms"] < whole["stats"]["kernel_ms"]
