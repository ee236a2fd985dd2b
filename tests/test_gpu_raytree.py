"""The ray-tree buffer on a real MI355X (-m gpu): mt_raytree_create / info / read_layer / shade[_device] / destroy,
MythTracer::BuildRayTree / ShadeRayTree (include/mythtracer_hip.h; the kernels are in mythtracer_amd/csrc/mt_raytree.h).

The bar is identity, no tolerance.  Every plane of every layer is held to the restatement of tests/raytree_ref.py
(doubles as uint64 views with NaN = NaN, bytes and indices equal, every ray), which tests/test_raytree_cpu.py pins to the
oracle's own frames; the shaded frames to mt_render_chunk at the same max_depth and to the oracle, byte for byte.  Every
test prints its counts.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import lightbuffer_ref as lr  # noqa: E402
import orclib  # noqa: E402
import raytree_ref as rr  # noqa: E402
from gbuffer_ref import same_bits  # noqa: E402

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding, scenegen, tiling  # noqa: E402

W, H = 96, 54
SCENES = ["cornell", "f2_decal", "mini", "room", "two_way"]
OFF_GRID = (5, 3, 61, 37)  # neither origin nor size a multiple of 8
CHUNKS = (None, OFF_GRID)
DEPTHS = (0, 1, 2, 5)


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"


def obj_of(scenes, name):
    return rr.TWO_WAY if name == "two_way" else scenes[name]


class Scene:
    def __init__(self, obj):
        self.abi = M.hip_abi()
        self.flat = M.MythTracer(obj).flatten()
        self.h = self.abi.scene_create(self.flat)
        self.trees = []

    def close(self):
        for t in self.trees:
            self.abi.raytree_destroy(t)
        self.abi.scene_destroy(self.h)

    def set_lights(self, lights):
        self.abi.set_lights(self.h, lights)

    def tree(self, cam, w, h, chunk=None, depth=5):
        t, stats = self.abi.raytree_create(self.h, binding.sensor(cam, w, h), w, h, chunk=chunk, max_depth=depth)
        self.trees.append(t)
        return t, stats

    def destroy(self, t):
        self.trees.remove(t)
        self.abi.raytree_destroy(t)

    def frame(self, cam, w, h, chunk=None, depth=5):
        return self.abi.render_chunk(self.h, binding.sensor(cam, w, h), w, h, chunk=chunk, max_depth=depth)


@pytest.fixture
def make(scenes):
    made = []

    def _make(name):
        made.append(Scene(obj_of(scenes, name)))
        return made[-1]
    yield _make
    for s in made:
        s.close()


@pytest.fixture(scope="module")
def restated(scenes):
    """(scene, light set, chunk) -> (oracle, the restated tree at depth 5), made once and left unchanged."""
    made, oracles = {}, {}

    def get(scene, which, chunk=None):
        if scene not in oracles:
            oracles[scene] = orclib.OracleScene(obj_of(scenes, scene))
        key = (scene, which, chunk)
        if key not in made:
            made[key] = rr.build(oracles[scene], rr.CAMERAS[scene], W, H, lr.light_sets(scene)[which], 5, chunk=chunk)
        return oracles[scene], made[key]
    return get


def differing(a, b, what):
    n = int((a != b).any(axis=-1).sum())
    print("%s: %d of %d pixels differ" % (what, n, a.shape[0] * a.shape[1]))
    return n


def dense_materials(flat, orc, lay):
    """A restated layer's material plane in the numbering of the scene description the kernel was given (the material
    of the stream triangle whose AddPrimitive index is the oracle's `prim`), after checking by value that it IS the
    oracle's material."""
    pos = np.full(len(flat["tri_id"]), -1, dtype=np.int64)
    pos[flat["tri_id"]] = np.arange(len(flat["tri_id"]))
    mats = orc.materials()
    want = np.full(lay["prim"].shape, -1, dtype=np.int32)
    hit = lay["prim"] >= 0
    want[hit] = flat["tri_material"][pos[lay["prim"][hit]]]
    assert np.array_equal(want < 0, lay["material"] < 0)
    for dense, om in set(zip(want[want >= 0].tolist(), lay["material"][want >= 0].tolist())):
        assert np.array_equal(flat["materials"][dense]["values"], mats[om][1])
    return want


def assert_tree_equal(s, t, orc, want, what):
    """Every plane of every layer of tree `t` against the restated tree `want`."""
    info = s.abi.raytree_info(t)
    print(what, "layers", info["n_rays"], "restated", want["n_rays"], "bytes", info["bytes"])
    assert info["n_rays"] == want["n_rays"] and info["n_layers"] == len(want["layers"])
    for k, lay in enumerate(want["layers"]):
        got = s.abi.raytree_read_layer(t, k)
        assert ("pixel" in got) == (k == 0)
        for name in rr.F64_PLANES:
            assert same_bits(got[name], lay[name], "%s layer %d %s" % (what, k, name)) == 0
        for name in ("in_object", "in_shadow", "child_refl", "child_refr"):
            n = int((got[name] != lay[name]).sum())
            print("%s layer %d %s: %d of %d elements differ" % (what, k, name, n, lay[name].size))
            assert n == 0 and got[name].dtype == lay[name].dtype
        assert np.array_equal(got["material"], dense_materials(s.flat, orc, lay)), (what, k)
        if k == 0:
            assert np.array_equal(got["pixel"], lay["pixel"])


# ---- planes

@pytest.mark.parametrize("scene", SCENES)
def test_planes_and_counters_against_the_restatement(scene, make, restated):
    """Every plane of every layer bit-identical to the restatement, layer 0 in tiling.py's order, info.n_rays and the
    create stats the restatement's and mt_render_chunk's own: the full frame and an off-grid chunk, both light sets."""
    cam = rr.CAMERAS[scene]
    s = make(scene)
    for chunk in CHUNKS:
        cw, ch = chunk[2:] if chunk else (W, H)
        for which, lights in lr.light_sets(scene).items():
            orc, want = restated(scene, which, chunk)
            s.set_lights(lights)
            t, st = s.tree(cam, W, H, chunk, 5)
            what = "%s %s %s" % (scene, which, chunk)
            assert_tree_equal(s, t, orc, want, what)
            info = s.abi.raytree_info(t)
            assert info["n_lights"] == len(lights) and info["max_depth"] == 5 and info["image"] == (W, H)
            assert info["chunk"] == (chunk if chunk else (0, 0, W, H)) and info["bytes"] > 0
            assert np.array_equal(s.abi.raytree_read_layer(t, 0, ("pixel",))["pixel"], tiling.raytree_layer0_order(cw, ch))
            frame = s.frame(cam, W, H, chunk, 5)["stats"]
            for name in ("rays_primary", "rays_secondary", "rays_shadow", "shaded_hits"):
                print(what, name, st[name], want[name], frame[name])
                assert st[name] == want[name] == frame[name]
            assert st["kernel_ms"] > 0 and st["total_ms"] >= st["kernel_ms"]
            s.destroy(t)


# ---- shade

@pytest.mark.parametrize("scene", SCENES)
def test_shaded_frames(scene, scenes, make):
    """mt_raytree_shade == mt_render_chunk(max_depth = d) == the oracle's frame for d in 0, 1, 2, 5: with unchanged
    lights, and -- from the OLD tree -- after each of the four colour edits against FRESH frames under the new lights."""
    cam = rr.CAMERAS[scene]
    orc = orclib.OracleScene(obj_of(scenes, scene))
    s = make(scene)
    for chunk in CHUNKS:
        for which, lights in lr.light_sets(scene).items():
            for d in DEPTHS:
                s.set_lights(lights)
                t, _ = s.tree(cam, W, H, chunk, d)
                before = None
                for k in (None, 0, 1, 2, 3):
                    new = lights if k is None else lr.edited(lights, k)
                    got = s.abi.raytree_shade(t, new)
                    s.set_lights(new)  # (the shade neither read nor changed the scene's lights)
                    orc.set_lights(new)
                    what = "%s %s %s d=%d edit %s" % (scene, which, chunk, d, k)
                    fresh = s.frame(cam, W, H, chunk, d)["rgb"]
                    assert differing(got["rgb"], fresh, what + " vs mt_render_chunk") == 0
                    assert differing(got["rgb"], orc.render(cam, W, H, chunk=chunk, max_level=d)["rgb"], what + " vs oracle") == 0
                    assert got["stats"]["kernel_ms"] > 0
                    assert all(got["stats"][n] == 0 for n in binding.STAT_NAMES)
                    if k is None:
                        before = fresh
                    elif k == 0:
                        assert (fresh != before).any()  # the edit is visible
                s.destroy(t)


# ---- small and odd shapes

def test_small_and_odd_shapes(scenes, make):
    cam = rr.CAMERAS["cornell"]
    lights = lr.light_sets("cornell")["one"]
    orc = orclib.OracleScene(scenes["cornell"])
    orc.set_lights(lights)
    s = make("cornell")
    s.set_lights(lights)
    # one pixel (of the mirror's reflection region or not: whatever the oracle says)
    for chunk in ((48, 40, 1, 1), (0, 0, 1, 1)):
        t, st = s.tree(cam, W, H, chunk, 5)
        want = rr.build(orc, cam, W, H, lights, 5, chunk=chunk)
        assert_tree_equal(s, t, orc, want, "1x1 %s" % (chunk,))
        assert st["rays_primary"] == 1
        assert differing(s.abi.raytree_shade(t, lights)["rgb"], orc.render(cam, W, H, chunk=chunk)["rgb"], "1x1") == 0
    # a chunk that only misses: the camera turned away from the box
    away = (50.0, 50.0, -120.0, 0.0, 180.0, 0.0, 100.0)
    t, st = s.tree(away, W, H, (8, 8, 20, 10), 5)
    info = s.abi.raytree_info(t)
    print("misses only:", info["n_rays"], st["shaded_hits"])
    assert info["n_layers"] == 1 and info["n_rays"] == [200] and st["shaded_hits"] == 0 and st["rays_shadow"] == 0
    lay = s.abi.raytree_read_layer(t, 0)
    assert np.isnan(lay["point"]).all() and (lay["material"] == -1).all() and (lay["in_shadow"] == 255).all()
    assert (lay["child_refl"] == -1).all() and (lay["child_refr"] == -1).all()
    assert not s.abi.raytree_shade(t, lights)["rgb"].any()
    # a layer of fewer than 64 rays
    t, _ = s.tree(cam, W, H, None, 5)
    n1 = s.abi.raytree_info(t)["n_rays"][1]
    print("cornell: %d secondary rays in layer 1" % n1)
    assert 0 < n1 < 64


@pytest.mark.parametrize("cw", [63, 64, 65])
def test_a_wave_ends_inside_at_and_past_an_item(cw, scenes, make):
    """One row of blocks, 63 / 64 / 65 pixels wide and 5 high: the last block is cut by both edges, and a wave's 64 rays
    end inside, at and past the list's items."""
    scene = "two_way"
    cam = rr.CAMERAS[scene]
    lights = lr.light_sets(scene)["one"]
    chunk = (17, 30, cw, 5)
    orc = orclib.OracleScene(rr.TWO_WAY)
    orc.set_lights(lights)
    s = make(scene)
    s.set_lights(lights)
    t, st = s.tree(cam, W, H, chunk, 5)
    want = rr.build(orc, cam, W, H, lights, 5, chunk=chunk)
    assert_tree_equal(s, t, orc, want, "width %d" % cw)
    assert differing(s.abi.raytree_shade(t, lights)["rgb"], orc.render(cam, W, H, chunk=chunk)["rgb"], "width %d" % cw) == 0
    assert st["rays_secondary"] == want["rays_secondary"] > 0


# ---- lights

def test_zero_lights(make):
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cornell_nolights_64.npz"))
    print("golden keys", list(g.keys()))
    w, h = (int(v) for v in g["image"])
    cam = tuple(float(v) for v in g["cam"])
    s = make("cornell")
    s.set_lights([])
    t, st = s.tree(cam, w, h, None, 5)
    info = s.abi.raytree_info(t)
    assert info["n_lights"] == 0 and st["rays_shadow"] == 0 and st["rays_secondary"] > 0
    lay = s.abi.raytree_read_layer(t, 0)
    assert lay["power"].shape == (0, w * h, 3) and lay["in_shadow"].shape == (0, w * h)
    got = s.abi.raytree_shade(t, [])["rgb"]
    assert differing(got, g["rgb"], "zero lights vs the golden") == 0
    assert differing(got, s.frame(cam, w, h)["rgb"], "zero lights vs mt_render_chunk") == 0
    with pytest.raises(RuntimeError, match="1 lights for a ray tree made with 0"):
        s.abi.raytree_shade(t, [(0.0,) * 12])


def test_more_lights_than_travel_with_the_launch(make):
    """Nine lights: the shade reads them from device memory."""
    lights = [(40.0 * i, 150.0 + 10 * i, 380.0 - 40 * i, 0.02, 0.01 * i, 0.03, 0.2, 0.15, 0.1 + 0.02 * i, 0.1, 0.2, 0.1)
              for i in range(9)]
    s = make("mini")
    s.set_lights(lights)
    cam = rr.CAMERAS["mini"]
    t, st = s.tree(cam, W, H)
    assert s.abi.raytree_read_layer(t, 1, ("power",))["power"].shape[0] == 9
    frame = s.frame(cam, W, H)
    assert st["rays_shadow"] == frame["stats"]["rays_shadow"]
    assert differing(s.abi.raytree_shade(t, lights)["rgb"], frame["rgb"], "nine lights") == 0
    new = lr.edited(lights, 0)
    got = s.abi.raytree_shade(t, new)["rgb"]
    s.set_lights(new)
    assert differing(got, s.frame(cam, W, H)["rgb"], "nine lights, edited") == 0
    with pytest.raises(RuntimeError, match="8 lights for a ray tree made with 9"):
        s.abi.raytree_shade(t, lights[:8])


# ---- argument checks that need a scene or a tree

def test_argument_checks_with_a_scene(make):
    s = make("cornell")
    s.set_lights(lr.light_sets("cornell")["one"])
    abi = s.abi
    sens = abi.make_sensor(binding.sensor(rr.CAMERAS["cornell"], W, H))

    def create(sensor, depth):
        t = abi.lib.mt_raytree_create(s.h, ctypes.byref(sensor) if sensor is not None else None, W, H, 0, 0, W, H, depth, None)
        assert not t
        return abi.last_error()

    # the sensor before max_depth
    assert create(None, 17) == "sensor is NULL"
    assert create(sens, -1) == "max_depth -1 outside [0, 16]"
    assert create(sens, 17) == "max_depth 17 outside [0, 16]"
    t, _ = s.tree(rr.CAMERAS["cornell"], W, H, None, 2)
    rgb = np.zeros((H, W, 3), dtype=np.uint8)
    light = binding.mt_light()
    for fn in (abi.lib.mt_raytree_shade, abi.lib.mt_raytree_shade_device):
        assert fn(t, None, -1, None, None) == -1 and "output bitmap is NULL" in abi.last_error()
        assert fn(t, None, -1, rgb.ctypes.data, None) == -1 and "bad lights argument" in abi.last_error()
        assert fn(t, None, 1, rgb.ctypes.data, None) == -1 and "bad lights argument" in abi.last_error()
        assert fn(t, ctypes.addressof(light), 0, rgb.ctypes.data, None) == -1
        assert "0 lights for a ray tree made with 1" in abi.last_error()
    n_layers = abi.raytree_info(t)["n_layers"]
    out = binding.mt_raytree_layer()
    assert abi.lib.mt_raytree_info(t, None) == -1 and "mt_raytree_desc is NULL" in abi.last_error()
    for layer in (-1, n_layers):
        assert abi.lib.mt_raytree_read_layer(t, layer, None) == -1
        assert "layer %d outside the ray tree's %d layers" % (layer, n_layers) in abi.last_error()
    assert abi.lib.mt_raytree_read_layer(t, 0, None) == -1 and "mt_raytree_layer is NULL" in abi.last_error()
    assert n_layers >= 2
    out.pixel = rgb.ctypes.data
    assert abi.lib.mt_raytree_read_layer(t, 1, ctypes.byref(out)) == -1 and "only layer 0" in abi.last_error()
    with pytest.raises(ValueError, match="unknown ray-tree plane"):
        abi.raytree_read_layer(t, 0, ("colour",))


# ---- streams, several trees, deep layouts

def test_shade_device_on_a_stream(make):
    import torch
    scene = "two_way"
    cam = rr.CAMERAS[scene]
    lights = lr.light_sets(scene)["bench"]
    s = make(scene)
    s.set_lights(lights)
    t, _ = s.tree(cam, W, H)
    new = lr.edited(lights, 0)
    want_old = s.frame(cam, W, H)["rgb"]
    s.set_lights(new)
    want_new = s.frame(cam, W, H)["rgb"]
    stream = torch.cuda.Stream()
    rgb = torch.zeros((2, H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        sp = ctypes.c_void_p(stream.cuda_stream)
        # an earlier device call of the same scene on the same stream, then two shades in stream order
        d_frame = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        s.abi.render_chunk_device(s.h, binding.sensor(cam, W, H), W, H, (0, 0, W, H), 5, d_frame.data_ptr(), None, sp)
        s.abi.raytree_shade_device(t, lights, rgb[0].data_ptr(), sp)
        s.abi.raytree_shade_device(t, new, rgb[1].data_ptr(), sp)
    stream.synchronize()
    assert differing(d_frame.cpu().numpy(), want_new, "frame on the stream") == 0
    assert differing(rgb[0].cpu().numpy(), want_old, "device shade, the tree's lights") == 0
    assert differing(rgb[1].cpu().numpy(), want_new, "device shade, edited lights") == 0


def test_two_trees_of_one_scene(make):
    scene = "mini"
    cam = rr.CAMERAS[scene]
    lights = lr.light_sets(scene)["bench"]
    s = make(scene)
    s.set_lights(lights)
    full, _ = s.tree(cam, W, H, None, 5)
    part, _ = s.tree(cam, W, H, OFF_GRID, 2)
    want_full = s.frame(cam, W, H, None, 5)["rgb"]
    want_part = s.frame(cam, W, H, OFF_GRID, 2)["rgb"]
    for _ in range(2):
        assert differing(s.abi.raytree_shade(full, lights)["rgb"], want_full, "full tree") == 0
        assert differing(s.abi.raytree_shade(part, lights)["rgb"], want_part, "chunk tree") == 0
    third, _ = s.tree(cam, W, H, None, 1)
    s.destroy(full)  # (the oldest first: destroy order does not matter among trees)
    assert differing(s.abi.raytree_shade(part, lights)["rgb"], want_part, "chunk tree, after a destroy") == 0
    assert differing(s.abi.raytree_shade(third, lights)["rgb"], s.frame(cam, W, H, None, 1)["rgb"], "third tree") == 0
    s.destroy(third)
    s.destroy(part)


@pytest.mark.parametrize("scene", ["loft"])
def test_deep_layout(scene, scenes, make):
    """An octree of 16 levels: a DEEP instantiation of raytree_trace_kernel.  (32x18: the restatement of this scene is
    the slow part.)"""
    w, h = 32, 18
    s = make(scene)
    assert s.flat["tree_depth"] >= 16
    s.set_lights(lr.BENCH_LIGHTS)
    cam = scenegen.ROOM_CAMERA
    t, st = s.tree(cam, w, h)
    frame = s.frame(cam, w, h)
    assert differing(s.abi.raytree_shade(t, lr.BENCH_LIGHTS)["rgb"], frame["rgb"], scene) == 0
    orc = orclib.OracleScene(scenes[scene])
    want = rr.build(orc, cam, w, h, lr.BENCH_LIGHTS, 5)
    assert_tree_equal(s, t, orc, want, scene)
    for name in ("rays_secondary", "rays_shadow", "shaded_hits"):
        assert st[name] == want[name] == frame["stats"][name]


def test_frame_kernels_are_untouched_by_the_calls(make):
    """A depth-5 frame before and after a tree's creation and a shade is byte-identical, the calls add no entry to
    mt_scene_kernel_times, and the second frame is the repeated launch it would have been."""
    w, h = 1920, 1080
    cam = scenegen.ROOM_CAMERA
    sens = binding.sensor(cam, w, h)
    s = make("room")
    s.set_lights(lr.BENCH_LIGHTS)
    s.abi.set_engine(s.h, 1)
    s.abi.kernel_times(s.h)
    f1 = s.abi.render_chunk(s.h, sens, w, h)["rgb"]
    t, _ = s.tree(cam, w, h)
    s.abi.raytree_shade(t, lr.edited(lr.BENCH_LIGHTS, 0))  # (does not touch the scene's lights)
    f2 = s.abi.render_chunk(s.h, sens, w, h)["rgb"]
    assert np.array_equal(f1, f2)
    pm, rm = s.abi.kernel_times(s.h)
    print("primary_ms", pm, "render_ms", rm)
    assert len(pm) == 2, pm
    assert pm[1] < pm[0] / 3, pm  # second frame: the order kernels, not primary_kernel (see test_gpu_gbuffer.py)


# ---- facade and Python

def test_facade_and_python_round_trip(scenes, make, tmp_path):
    """MythTracer.raytree (BuildRayTree / ShadeRayTree through the ctypes shim) and a C++ program against the facade's
    headers (tests/seam/raytree_driver.cc)."""
    from mythtracer_amd import build
    cam = rr.CAMERAS["two_way"]
    w, h = 61, 37
    lights = lr.light_sets("two_way")["bench"]
    m = M.MythTracer(rr.TWO_WAY)
    m.set_lights(lights)
    m.set_supersampling(2)  # does not apply
    tree = m.raytree(cam, w, h, max_depth=3)
    m.set_supersampling(1)
    frame = m.render(cam, w, h)  # (max_depth went through set_max_level)
    info = tree.info
    print("facade:", info["n_rays"], tree.counters)
    assert info["max_depth"] == 3 and info["n_lights"] == 3 and info["chunk"] == (0, 0, w, h)
    for name in ("rays_primary", "rays_secondary", "rays_shadow", "shaded_hits"):
        assert tree.counters[name] == frame["counters"][name]
    assert sum(info["n_rays"][1:]) == frame["counters"]["rays_secondary"] and tree.kernel_ms > 0
    assert np.array_equal(tree.layer(0, ("pixel",))["pixel"], tiling.raytree_layer0_order(w, h))
    assert differing(tree.shade()["rgb"], frame["rgb"], "facade shade") == 0
    new = lr.edited(lights, 0)
    relit = tree.shade(lights=new)
    assert relit["kernel_ms"] > 0
    assert differing(relit["rgb"], m.render(cam, w, h)["rgb"], "facade shade, edited") == 0  # (shade set the lights)
    m.set_lights(lights[:2])
    with pytest.raises(RuntimeError, match="another number of lights"):
        tree.shade()
    part = m.raytree(cam, w, h, chunk=(5, 3, 33, 17))
    m.set_lights(lights)
    with pytest.raises(RuntimeError, match="another number of lights"):
        part.shade()
    part.close()
    with pytest.raises(RuntimeError, match="closed"):
        part.info
    part = m.raytree(cam, w, h, chunk=(5, 3, 33, 17))
    assert differing(part.shade()["rgb"], m.render(cam, w, h, chunk=(5, 3, 33, 17))["rgb"], "facade chunk") == 0
    m.close()  # closes the trees it still has, then the scene
    assert tree.h is None and part.h is None
    # the C++ driver
    exe = str(tmp_path / "raytree_driver")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "seam", "raytree_driver.cc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(build.HOST, "include"), "-I", build.INC,
                           "-o", exe, src, "-L", build.LIB, "-lmythtracer_host", "-lmythtracer_hip",
                           "-Wl,-rpath," + build.LIB])
    out = str(tmp_path / "t.bin")
    args = [exe, rr.TWO_WAY, str(w), str(h), "3"] + [repr(float(c)) for c in cam] + [str(len(lights))]
    args += [repr(float(v)) for l in lights for v in l] + [out]
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    words = r.stdout.decode().split()
    print("driver:", words)
    assert words == (["layers", str(info["n_layers"]), "rays"] + [str(n) for n in info["n_rays"]] +
                     ["secondary", str(frame["counters"]["rays_secondary"]), "shadow", str(frame["counters"]["rays_shadow"])])
    frames = np.frombuffer(open(out, "rb").read(), dtype=np.uint8).reshape(4, h, w, 3)
    assert differing(frames[0], frame["rgb"], "driver, RayTrace") == 0
    assert differing(frames[1], frames[0], "driver, same lights: ShadeRayTree vs RayTrace") == 0
    assert differing(frames[2], frames[3], "driver, edited lights: ShadeRayTree vs RayTrace") == 0
    assert (frames[2] != frames[0]).any()


# ---- the workload's size

def test_shaded_room_at_1080p(make):
    """The one test of this size: room, 1920x1080, bench camera and lights, d = 5.  The shaded frame is the rendered one
    byte for byte, and a shade costs less device time than the frame it replaces -- the ordering the feature exists for.
    No ratio is fixed."""
    w, h = 1920, 1080
    cam = scenegen.ROOM_CAMERA
    s = make("room")
    s.set_lights(lr.BENCH_LIGHTS)
    frame = s.frame(cam, w, h)
    frame = s.frame(cam, w, h)  # (the repeated launch: ordered by the first one's costs)
    t, st = s.tree(cam, w, h)
    info = s.abi.raytree_info(t)
    got = s.abi.raytree_shade(t, lr.BENCH_LIGHTS)
    got = s.abi.raytree_shade(t, lr.BENCH_LIGHTS)
    print("1080p room: create %.3f ms kernels / %.3f ms wall, layers %s, trace_ms %s, %.1f MB; shade %.3f ms; frame %.3f ms"
          % (st["kernel_ms"], st["total_ms"], info["n_rays"], ["%.3f" % v for v in info["trace_ms"]], info["bytes"] / 1e6,
             got["stats"]["kernel_ms"], frame["stats"]["kernel_ms"]))
    assert differing(got["rgb"], frame["rgb"], "1080p vs mt_render_chunk") == 0
    for name in ("rays_primary", "rays_secondary", "rays_shadow", "shaded_hits"):
        assert st[name] == frame["stats"][name], name
    assert got["stats"]["kernel_ms"] < frame["stats"]["kernel_ms"]
    new = lr.edited(lr.BENCH_LIGHTS, 0)
    relit = s.abi.raytree_shade(t, new)["rgb"]
    s.set_lights(new)
    assert differing(relit, s.frame(cam, w, h)["rgb"], "1080p, edited") == 0
