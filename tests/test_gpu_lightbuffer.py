"""The direct-light buffer and the relight pass on a real MI355X (-m gpu): mt_render_lightbuffer[_device],
mt_shade_direct[_device], MythTracer::RayTraceLightBuffer / ShadeDirect (include/mythtracer_hip.h; the kernels are in
mythtracer_amd/csrc/mt_lightbuffer.h).

The bar is identity, no tolerance.  The light-buffer planes are held to the restatement of tests/lightbuffer_ref.py
(power as uint64 views with NaN = NaN, in_shadow equal, every pixel), which tests/test_lightbuffer_cpu.py pins to the
oracle's own frames and to goldens made with the reference's IntersectRay; the relit frames to mt_render_chunk at
max_depth = 0 and to the oracle's max_level = 0 frame, byte for byte.  Every test prints its counts.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gbuffer_ref  # noqa: E402
import lightbuffer_ref as lr  # noqa: E402
import orclib  # noqa: E402
from gbuffer_ref import same_bits  # noqa: E402

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding, scenegen  # noqa: E402

W, H = 96, 54
SCENES = ["cornell", "f2_decal", "mini", "room"]
RELIGHT = binding.RELIGHT_GBUFFER_PLANES
OFF_GRID = (5, 3, 61, 37)  # neither origin nor size a multiple of 8


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

    def lightbuffer(self, cam, w, h, chunk=None, channels=None, gbuffer_channels=()):
        return self.abi.render_lightbuffer(self.h, binding.sensor(cam, w, h), w, h, self.n_lights, chunk=chunk,
                                           channels=channels, gbuffer_channels=gbuffer_channels)

    def gbuffer(self, cam, w, h, chunk=None, channels=None):
        return self.abi.render_gbuffer(self.h, binding.sensor(cam, w, h), w, h, chunk=chunk, channels=channels)

    def relight(self, cam, w, h, gb, lb, lights, chunk=None):
        return self.abi.shade_direct(self.h, binding.sensor(cam, w, h), w, h, gb, lb, lights, chunk=chunk)

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


def assert_lightbuffer_equal(got, want, what):
    assert same_bits(got["power"], want["power"], what + " power") == 0, what
    n = int((got["in_shadow"] != want["in_shadow"]).sum())
    print("%s in_shadow: %d of %d elements differ" % (what, n, want["in_shadow"].size))
    assert n == 0, what


@pytest.mark.parametrize("scene", SCENES)
def test_planes_and_counters_against_the_restatement(scene, scenes, make):
    """power bit-identical, in_shadow equal, rays_shadow / rays_primary / shaded_hits the restatement's: the full
    frame and an off-grid chunk, both light sets, every pixel (f2_decal and the room cross glass)."""
    orc = orclib.OracleScene(scenes[scene])
    cam = lr.CAMERAS[scene]
    s = make(scene)
    for chunk in (None, OFF_GRID):
        gb = gbuffer_ref.oracle_gbuffer(orc, cam, W, H, chunk)
        for key, lights in lr.light_sets(scene).items():
            want = lr.ref_lightbuffer(orc, gb, lights)
            s.set_lights(lights)
            got = s.lightbuffer(cam, W, H, chunk=chunk)
            what = "%s %s %s" % (scene, key, chunk)
            assert_lightbuffer_equal(got, want, what)
            st = got["stats"]
            print(what, "rays_shadow", st["rays_shadow"], want["rays_shadow"], "longest loop", int(want["iterations"].max()))
            assert st["rays_primary"] == gb["prim"].size
            assert st["rays_shadow"] == want["rays_shadow"]
            assert st["shaded_hits"] == int((gb["prim"] >= 0).sum())
            assert st["rays_secondary"] == 0 and st["kernel_ms"] > 0
            assert np.array_equal(got["in_shadow"][0] == 255, ~((gb["prim"] >= 0) & (gb["material"] >= 0)))


@pytest.mark.parametrize("scene", ["cornell", "mini", "room"])
def test_planes_against_the_reference_made_goldens(scene, make):
    g = lr.load_golden(scene)
    s = make(scene)
    for key, lights in lr.light_sets(scene).items():
        s.set_lights(lights)
        got = s.lightbuffer(lr.CAMERAS[scene], W, H)
        assert_lightbuffer_equal(got, dict(power=g["power_" + key], in_shadow=g["in_shadow_" + key]), "golden %s %s" % (scene, key))
        assert got["stats"]["rays_shadow"] == int(g["iterations_" + key].sum())


def test_material_less_scene_gets_255_everywhere(make):
    s = make("mini_nomtl")
    s.set_lights(lr.BENCH_LIGHTS)
    got = s.lightbuffer(scenegen.ROOM_CAMERA, W, H)
    assert (got["in_shadow"] == 255).all() and np.isnan(got["power"]).all()
    assert got["stats"]["rays_shadow"] == 0 and got["stats"]["shaded_hits"] > 0


def test_gbuffer_planes_from_the_combined_launch_and_plane_subsets(make):
    """The G-buffer planes the combined launch writes are mt_render_gbuffer's bits; subsets of either struct's planes
    give the same bits; a light-buffer plane alone works."""
    s = make("room")
    s.set_lights(lr.BENCH_LIGHTS)
    cam = scenegen.ROOM_CAMERA
    w, h = 101, 67
    for chunk in (None, (13, 27, 65, 33)):
        alone = s.gbuffer(cam, w, h, chunk=chunk)
        both = s.lightbuffer(cam, w, h, chunk=chunk, gbuffer_channels=None)
        for p in gbuffer_ref.ALL_PLANES:
            if p in gbuffer_ref.F64_PLANES:
                assert same_bits(both[p], alone[p], "combined %s %s" % (p, chunk)) == 0
            else:
                assert np.array_equal(both[p], alone[p]), p
        plain = s.lightbuffer(cam, w, h, chunk=chunk)
        assert set(plain) == {"power", "in_shadow", "stats"}
        assert_lightbuffer_equal(both, plain, "with and without G-buffer planes %s" % (chunk,))
        for sub in (("power",), ("in_shadow",)):
            for gsub in ((), RELIGHT, ("depth",), ("albedo", "prim")):
                got = s.lightbuffer(cam, w, h, chunk=chunk, channels=sub, gbuffer_channels=gsub)
                assert set(got) == set(sub) | set(gsub) | {"stats"}
                if "power" in sub:
                    assert same_bits(got["power"], plain["power"], "subset power") == 0
                else:
                    assert np.array_equal(got["in_shadow"], plain["in_shadow"])
                for p in gsub:
                    if p in gbuffer_ref.F64_PLANES:
                        assert same_bits(got[p], alone[p], "subset %s" % p) == 0
                    else:
                        assert np.array_equal(got[p], alone[p])
                assert got["stats"]["rays_shadow"] == plain["stats"]["rays_shadow"]
    # zero lights: valid with a G-buffer plane only
    s.set_lights([])
    got = s.lightbuffer(cam, w, h, gbuffer_channels=("depth",))
    assert got["power"].shape == (0, h, w, 3) and got["stats"]["rays_shadow"] == 0
    assert same_bits(got["depth"], s.gbuffer(cam, w, h, channels=("depth",))["depth"], "depth, zero lights") == 0
    with pytest.raises(RuntimeError, match="no lights are set"):
        s.lightbuffer(cam, w, h)
    with pytest.raises(RuntimeError, match="no plane of the mt_lightbuffer"):
        s.lightbuffer(cam, w, h, channels=())


@pytest.mark.parametrize("scene", SCENES)
def test_relit_frame_with_unchanged_lights(scene, scenes, make):
    """mt_shade_direct == mt_render_chunk(max_depth=0) == the oracle's max_level=0 frame; full frame and chunk."""
    orc = orclib.OracleScene(scenes[scene])
    cam = lr.CAMERAS[scene]
    s = make(scene)
    for key, lights in lr.light_sets(scene).items():
        s.set_lights(lights)
        orc.set_lights(lights)
        for chunk in (None, OFF_GRID):
            b = s.lightbuffer(cam, W, H, chunk=chunk, gbuffer_channels=RELIGHT)
            got = s.relight(cam, W, H, b, b, lights, chunk=chunk)
            what = "%s %s %s" % (scene, key, chunk)
            assert differing(got["rgb"], s.frame0(cam, W, H, chunk=chunk)["rgb"], what + " vs mt_render_chunk") == 0
            assert differing(got["rgb"], orc.render(cam, W, H, chunk=chunk, max_level=0)["rgb"], what + " vs oracle") == 0
            assert got["stats"]["kernel_ms"] > 0 and got["stats"]["rays_primary"] == 0


def test_relit_room_at_1080p(scenes, make):
    w, h = 1920, 1080
    cam = scenegen.ROOM_CAMERA
    s = make("room")
    s.set_lights(lr.BENCH_LIGHTS)
    b = s.lightbuffer(cam, w, h, gbuffer_channels=RELIGHT)
    got = s.relight(cam, w, h, b, b, lr.BENCH_LIGHTS)
    frame = s.frame0(cam, w, h)
    print("1080p room: lightbuffer_kernel %.3f ms, shade_direct_kernel %.3f ms, max_depth=0 frame %.3f ms"
          % (b["stats"]["kernel_ms"], got["stats"]["kernel_ms"], frame["stats"]["kernel_ms"]))
    assert differing(got["rgb"], frame["rgb"], "1080p vs mt_render_chunk") == 0
    # the one ordering the feature rests on: a relight costs less than the re-trace it replaces
    assert got["stats"]["kernel_ms"] < frame["stats"]["kernel_ms"]
    orc = orclib.OracleScene(scenes["room"])
    orc.set_lights(lr.BENCH_LIGHTS)
    assert differing(got["rgb"], orc.render(cam, w, h, max_level=0)["rgb"], "1080p vs oracle") == 0
    assert b["stats"]["rays_primary"] == w * h


@pytest.mark.parametrize("scene", SCENES)
def test_relit_frame_with_edited_colours_and_the_old_buffers(scene, make):
    """The buffers are made ONCE; after every colour edit mt_shade_direct over them equals a FRESH max_depth = 0 frame
    under the new lights (an ambient above the stored power and a zero specular among the edits)."""
    cam = lr.CAMERAS[scene]
    s = make(scene)
    for key, lights in lr.light_sets(scene).items():
        s.set_lights(lights)
        b = s.lightbuffer(cam, W, H, gbuffer_channels=RELIGHT)
        before = s.frame0(cam, W, H)["rgb"]
        for k in range(4):
            new = lr.edited(lights, k)
            got = s.relight(cam, W, H, b, b, new)["rgb"]
            s.set_lights(new)
            fresh = s.frame0(cam, W, H)["rgb"]
            assert differing(got, fresh, "%s %s edit %d" % (scene, key, k)) == 0
            if k == 0:
                assert (fresh != before).any()


def test_more_lights_than_travel_with_the_launch(scenes, make):
    """Nine lights: the relight reads them from device memory."""
    lights = [(40.0 * i, 150.0 + 10 * i, 380.0 - 40 * i, 0.02, 0.01 * i, 0.03, 0.2, 0.15, 0.1 + 0.02 * i, 0.1, 0.2, 0.1)
              for i in range(9)]
    s = make("mini")
    s.set_lights(lights)
    cam = lr.CAMERAS["mini"]
    b = s.lightbuffer(cam, W, H, gbuffer_channels=RELIGHT)
    assert b["power"].shape == (9, H, W, 3)
    assert differing(s.relight(cam, W, H, b, b, lights)["rgb"], s.frame0(cam, W, H)["rgb"], "nine lights") == 0
    new = lr.edited(lights, 0)
    got = s.relight(cam, W, H, b, b, new)["rgb"]
    s.set_lights(new)
    assert differing(got, s.frame0(cam, W, H)["rgb"], "nine lights, edited") == 0


def test_device_calls_on_a_stream(make):
    import torch
    s = make("room")
    s.set_lights(lr.BENCH_LIGHTS)
    cam = scenegen.ROOM_CAMERA
    w, h = 101, 67
    sens = binding.sensor(cam, w, h)
    want = s.lightbuffer(cam, w, h, gbuffer_channels=RELIGHT)
    frame = s.frame0(cam, w, h)["rgb"]
    stream = torch.cuda.Stream()
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    g = dict(point=f64(h, w, 3), normal=f64(h, w, 3), albedo=f64(h, w, 3),
             material=torch.zeros((h, w), dtype=torch.int32, device="cuda"))
    lb = dict(power=f64(3, h, w, 3), in_shadow=torch.full((3, h, w), 77, dtype=torch.uint8, device="cuda"))
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s.abi.read_stats(s.h)
    with torch.cuda.stream(stream):
        sp = ctypes.c_void_p(stream.cuda_stream)
        s.abi.render_lightbuffer_device(s.h, sens, w, h, (0, 0, w, h), {n: t.data_ptr() for n, t in lb.items()},
                                        {n: t.data_ptr() for n, t in g.items()}, sp)
        s.abi.shade_direct_device(s.h, sens, w, h, (0, 0, w, h), {n: t.data_ptr() for n, t in g.items()},
                                  {n: t.data_ptr() for n, t in lb.items()}, lr.BENCH_LIGHTS, rgb.data_ptr(), sp)
    stream.synchronize()
    st = s.abi.read_stats(s.h)
    assert st["rays_primary"] == w * h and st["rays_shadow"] == want["stats"]["rays_shadow"]
    assert_lightbuffer_equal({n: t.cpu().numpy() for n, t in lb.items()}, want, "device call")
    for n in RELIGHT[:3]:
        assert same_bits(g[n].cpu().numpy(), want[n], "device call " + n) == 0
    assert np.array_equal(g["material"].cpu().numpy(), want["material"])
    assert differing(rgb.cpu().numpy(), frame, "device relight") == 0


@pytest.mark.parametrize("scene", ["loft"])
def test_deep_layout(scene, scenes, make):
    """An octree of 16 levels: a DEEP instantiation of lightbuffer_kernel."""
    w, h = 48, 27
    s = make(scene)
    assert s.flat["tree_depth"] >= 16
    s.set_lights(lr.BENCH_LIGHTS)
    cam = scenegen.ROOM_CAMERA
    b = s.lightbuffer(cam, w, h, gbuffer_channels=RELIGHT)
    assert differing(s.relight(cam, w, h, b, b, lr.BENCH_LIGHTS)["rgb"], s.frame0(cam, w, h)["rgb"], scene) == 0
    orc = orclib.OracleScene(scenes[scene])
    want = lr.ref_lightbuffer(orc, gbuffer_ref.oracle_gbuffer(orc, cam, w, h), lr.BENCH_LIGHTS)
    assert_lightbuffer_equal(b, want, scene)


def test_frame_kernels_are_untouched_by_the_calls(make):
    """A depth-5 frame before and after a light-buffer call and a relight is byte-identical, the calls add no entry to
    mt_scene_kernel_times, and the second frame is the repeated launch it would have been."""
    w, h = 1920, 1080
    cam = scenegen.ROOM_CAMERA
    sens = binding.sensor(cam, w, h)
    s = make("room")
    s.set_lights(lr.BENCH_LIGHTS)
    s.abi.set_engine(s.h, 1)
    s.abi.kernel_times(s.h)
    f1 = s.abi.render_chunk(s.h, sens, w, h)["rgb"]
    b = s.lightbuffer(cam, w, h, gbuffer_channels=RELIGHT)
    s.relight(cam, w, h, b, b, lr.edited(lr.BENCH_LIGHTS, 0))  # (does not touch the scene's lights)
    f2 = s.abi.render_chunk(s.h, sens, w, h)["rgb"]
    assert np.array_equal(f1, f2)
    pm, rm = s.abi.kernel_times(s.h)
    print("primary_ms", pm, "render_ms", rm)
    assert len(pm) == 2, pm
    assert pm[1] < pm[0] / 3, pm  # second frame: the order kernels, not primary_kernel (see test_gpu_gbuffer.py)


def test_facade_and_python_round_trip(scenes, make, tmp_path):
    """MythTracer.lightbuffer / relight (RayTraceLightBuffer / ShadeDirect through the ctypes shim) and a C++ program
    against the facade's headers (tests/seam/lightbuffer_driver.cc)."""
    from mythtracer_amd import build
    cam = lr.CAMERAS["mini"]
    w, h = 61, 37
    lights = lr.BENCH_LIGHTS
    s = make("mini")
    s.set_lights(lights)
    want = s.lightbuffer(cam, w, h, gbuffer_channels=RELIGHT)
    m = M.MythTracer(scenes["mini"])
    m.set_lights(lights)
    m.set_supersampling(2)  # ignored
    b = m.lightbuffer(cam, w, h)
    assert set(b) == {"power", "in_shadow"} | set(RELIGHT) | {"counters", "kernel_ms", "total_ms"}
    assert_lightbuffer_equal(b, want, "facade")
    assert b["counters"]["rays_shadow"] == want["stats"]["rays_shadow"] and b["kernel_ms"] > 0
    m.set_supersampling(1)
    m.set_max_level(0)
    assert differing(m.relight(cam, w, h, b, b)["rgb"], m.render(cam, w, h)["rgb"], "facade relight") == 0
    new = lr.edited(lights, 0)
    relit = m.relight(cam, w, h, b, b, lights=new)["rgb"]
    assert differing(relit, m.render(cam, w, h)["rgb"], "facade relight, edited") == 0  # (relight set the lights)
    part = m.lightbuffer(cam, w, h, chunk=OFF_GRID[:2] + (33, 17), channels=("in_shadow",), gbuffer_channels=())
    assert set(part) == {"in_shadow", "counters", "kernel_ms", "total_ms"}
    m.set_lights(lights)
    assert np.array_equal(m.lightbuffer(cam, w, h, chunk=(5, 3, 33, 17), channels=("in_shadow",), gbuffer_channels=())["in_shadow"],
                          want["in_shadow"][:, 3:20, 5:38])
    # the C++ driver
    exe = str(tmp_path / "lightbuffer_driver")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "seam", "lightbuffer_driver.cc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(build.HOST, "include"), "-I", build.INC,
                           "-o", exe, src, "-L", build.LIB, "-lmythtracer_host", "-lmythtracer_hip",
                           "-Wl,-rpath," + build.LIB])
    out = str(tmp_path / "l.bin")
    args = [exe, scenes["mini"], str(w), str(h)] + [repr(float(c)) for c in cam] + [str(len(lights))]
    args += [repr(float(v)) for l in lights for v in l] + [out]
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode().split() == ["primary", str(w * h), "shadow", str(want["stats"]["rays_shadow"])]
    raw = open(out, "rb").read()
    n, nl = w * h, len(lights)
    assert len(raw) == nl * n * 25 + 3 * n * 3
    power = np.frombuffer(raw, dtype=np.float64, count=nl * n * 3).reshape(nl, h, w, 3)
    shadow = np.frombuffer(raw, dtype=np.uint8, count=nl * n, offset=nl * n * 24).reshape(nl, h, w)
    assert_lightbuffer_equal(dict(power=power, in_shadow=shadow), want, "C++ driver")
    frames = np.frombuffer(raw, dtype=np.uint8, offset=nl * n * 25).reshape(3, h, w, 3)
    s.set_lights(lights)
    assert differing(frames[0], s.frame0(cam, w, h)["rgb"], "driver, same lights") == 0
    assert differing(frames[1], frames[2], "driver, edited lights: ShadeDirect vs RayTrace") == 0
    assert (frames[1] != frames[0]).any()
