"""Ray-list trees and linear colours on a real MI355X (-m gpu): mt_raytree_create_rays[_device],
mt_raytree_shade_colors[_device], mt_trace_rays, MythTracer::BuildRayTree(rays) / ShadeRayTree(colours) / TraceRays
(include/mythtracer_hip.h; the two kernels are at the end of mythtracer_amd/csrc/mt_raytree.h).

The bar is identity.  A tree made from the sensor's rays is the sensor tree in every plane of every layer (doubles as
uint64 views with NaN = NaN, bytes and indices equal, every ray) and shades to mt_render_chunk's bytes; a layer handed
in as a list gives the layers below it; lists no sensor makes are held to tests/raylist_ref.py, which
tests/test_raylist_cpu.py pins to a per-ray restatement of TraceRayWorker.  The one tolerance is on the linear colours
against numpy's, where a specular term went through pow; V3DtoRGB of the colours is mt_raytree_shade's bitmap exactly.
Every test prints its counts.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gbuffer_ref  # noqa: E402
import lightbuffer_ref as lr  # noqa: E402
import orclib  # noqa: E402
import raylist_ref as rl  # noqa: E402
import raytree_ref as rr  # noqa: E402
import raytree_update_ref as ru  # noqa: E402
from gbuffer_ref import same_bits  # noqa: E402

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding, scenegen, tiling  # noqa: E402

W, H = 96, 54
COUNTERS = ("rays_primary", "rays_secondary", "rays_shadow", "shaded_hits")
PLANES = rr.F64_PLANES + rr.INT_PLANES + ("material",)
NINE_LIGHTS = [(40.0 * i, 150.0 + 10 * i, 380.0 - 40 * i, 0.02, 0.01 * i, 0.03, 0.2, 0.15, 0.1 + 0.02 * i, 0.1, 0.2, 0.1)
               for i in range(9)]


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

    def tree(self, cam, w, h, depth=5):
        t, stats = self.abi.raytree_create(self.h, binding.sensor(cam, w, h), w, h, max_depth=depth)
        self.trees.append(t)
        return t, stats

    def tree_of_rays(self, rays, list_w=None, depth=5, **kw):
        t, stats = self.abi.raytree_create_rays(self.h, rays, list_w, max_depth=depth, **kw)
        self.trees.append(t)
        return t, stats

    def destroy(self, t):
        self.trees.remove(t)
        self.abi.raytree_destroy(t)

    def frame(self, cam, w, h, depth=5):
        return self.abi.render_chunk(self.h, binding.sensor(cam, w, h), w, h, max_depth=depth)


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
def two_way():
    """The oracle of two_way and the restated trees of its lists, made once and left unchanged."""
    orc = orclib.OracleScene(rr.TWO_WAY)
    made = {}

    def restated(name, lights_key="bench"):
        if (name, lights_key) not in made:
            rays, w, h, _ = LISTS[name](orc)
            lights = LIGHTS[lights_key]
            made[name, lights_key] = rl.build_from_rays(orc, rays, w, h, lights, 5)
        return made[name, lights_key]
    return orc, restated


# the lists no sensor makes: name -> oracle -> (rays, list_w, list_h, the restatement's layer sizes)
LISTS = {
    "panorama 40x20": lambda orc: (rl.panorama_rays(40, 20), 40, 20, [800, 392, 99, 9]),
    "panorama 21x13": lambda orc: (rl.panorama_rays(21, 13), 21, 13, [273, 133, 31, 4]),
    "orthographic (0, 0, 1)": lambda orc: (rl.orthographic_rays(orc, 20, 10), 20, 10, [200, 59, 26, 13, 26, 13]),
    "orthographic (0, 0, 2)": lambda orc: (rl.orthographic_rays(orc, 20, 10, direction=(0.0, 0.0, 2.0)), 20, 10,
                                           [200, 59, 26, 13, 26, 13]),
}
LIGHTS = {"bench": lr.light_sets("two_way")["bench"], "one": lr.light_sets("two_way")["one"], "none": [],
          "nine": NINE_LIGHTS, "moved": ru.lights_before_and_after("two_way")[1]}


def differing(a, b, what):
    a, b = a.reshape(-1, 3), b.reshape(-1, 3)
    n = int((a != b).any(axis=-1).sum())
    print("%s: %d of %d rays differ" % (what, n, a.shape[0]))
    return n


def dense_materials(flat, orc, lay):
    """A restated layer's material plane in the numbering of the scene description the kernel was given (as
    tests/test_gpu_raytree.py does it), after checking by value that it IS the oracle's material."""
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


def assert_tree_is_restated(s, t, orc, want, what):
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


def assert_same_trees(s, a, b, what, first=0, pixel=True):
    """Tree `b` against the layers of tree `a` from `first` on, both read back: every plane of every layer."""
    ia, ib = s.abi.raytree_info(a), s.abi.raytree_info(b)
    print(what, "layers", ia["n_rays"][first:], ib["n_rays"])
    assert ia["n_rays"][first:] == ib["n_rays"] and ia["n_lights"] == ib["n_lights"]
    for k in range(ib["n_layers"]):
        la, lb = s.abi.raytree_read_layer(a, first + k), s.abi.raytree_read_layer(b, k)
        for name in PLANES:
            if name in rr.F64_PLANES:
                assert same_bits(lb[name], la[name], "%s layer %d %s" % (what, k, name)) == 0
            else:
                assert lb[name].dtype == la[name].dtype and np.array_equal(lb[name], la[name]), (what, k, name)
        if k == 0 and first == 0 and pixel:
            assert np.array_equal(lb["pixel"], la["pixel"])


# ---- the sensor's rays as a list

@pytest.mark.parametrize("scene", ["cornell", "two_way", "mini", "f2_decal"])
def test_the_sensors_rays_as_a_list(scene, make):
    """mt_raytree_create_rays from the sensor's rays is mt_raytree_create's tree in every plane of every layer, with its
    counters, and shades to mt_render_chunk's frame, under both light sets."""
    cam = rr.CAMERAS[scene]
    s = make(scene)
    rays = gbuffer_ref.pixel_rays(cam, W, H).reshape(W * H, 6)
    for which, lights in lr.light_sets(scene).items():
        s.set_lights(lights)
        t0, st0 = s.tree(cam, W, H)
        t1, st1 = s.tree_of_rays(rays, W)
        what = "%s %s" % (scene, which)
        assert_same_trees(s, t0, t1, what)
        i0, i1 = s.abi.raytree_info(t0), s.abi.raytree_info(t1)
        assert (i0["from_rays"], i1["from_rays"]) == (0, 1)
        assert i1["image"] == (W, H) and i1["chunk"] == (0, 0, W, H) and i1["max_depth"] == 5 and i1["bytes"] > 0
        assert np.array_equal(s.abi.raytree_read_layer(t1, 0, ("pixel",))["pixel"], tiling.raytree_layer0_order(W, H))
        for name in COUNTERS:
            print(what, name, st0[name], st1[name])
            assert st0[name] == st1[name]
        assert st1["rays_primary"] == W * H and st1["kernel_ms"] > 0 and st1["total_ms"] >= st1["kernel_ms"]
        frame = s.frame(cam, W, H)["rgb"]
        assert differing(s.abi.raytree_shade(t1, lights)["rgb"], frame, what + " shade vs mt_render_chunk") == 0
        if scene == "two_way":  # the rays from the sensor tree's own layer 0, un-permuted by `pixel`
            lay = s.abi.raytree_read_layer(t0, 0, ("ray", "pixel"))
            own = np.zeros((W * H, 6))
            own[lay["pixel"]] = lay["ray"]
            assert same_bits(own, rays, "layer 0 un-permuted vs pixel_rays") == 0
            t2, _ = s.tree_of_rays(own, W)
            assert_same_trees(s, t0, t2, what + " (own rays)")
            assert differing(s.abi.raytree_shade(t2, lights)["rgb"], frame, what + " (own rays) shade") == 0
            s.destroy(t2)
        s.destroy(t1)
        s.destroy(t0)


# ---- a sub-tree as a list

@pytest.mark.parametrize("k", [1, 2])
def test_a_layer_as_a_list_gives_the_layers_below_it(k, make):
    """Layer k of a sensor tree, read back and handed in as an n x 1 list with its in_object and coef and max_depth - k,
    gives that tree's layers k onwards: through the host form and the device form (torch tensors)."""
    import torch
    scene = "two_way"
    s = make(scene)
    s.set_lights(LIGHTS["bench"])
    t0, _ = s.tree(rr.CAMERAS[scene], W, H)
    lay = s.abi.raytree_read_layer(t0, k, ("ray", "in_object", "coef"))
    n = len(lay["ray"])
    assert n == {1: 4353, 2: 1561}[k] and lay["in_object"].any() and (lay["coef"] != 1.0).any()
    t1, st = s.tree_of_rays(lay["ray"], None, 5 - k, in_object=lay["in_object"], coef=lay["coef"])
    assert_same_trees(s, t0, t1, "two_way from layer %d, host form" % k, first=k)
    info = s.abi.raytree_info(t1)
    assert info["n_layers"] == 6 - k and info["chunk"] == (0, 0, n, 1) and st["rays_primary"] == n
    assert np.array_equal(s.abi.raytree_read_layer(t1, 0, ("pixel",))["pixel"], np.arange(n))
    d = [torch.from_numpy(lay[name]).cuda() for name in ("ray", "in_object", "coef")]
    torch.cuda.synchronize()  # the list is read on the scene's default stream: it must be finished
    t2, st2 = s.tree_of_rays(d[0], None, 5 - k, in_object=d[1], coef=d[2], device=True)
    assert_same_trees(s, t0, t2, "two_way from layer %d, device form" % k, first=k)
    assert_same_trees(s, t1, t2, "host form vs device form")
    for name in COUNTERS:
        assert st[name] == st2[name], name


# ---- lists no sensor makes

@pytest.mark.parametrize("name", list(LISTS))
def test_lists_no_sensor_makes(name, make, two_way):
    orc, restated = two_way
    rays, w, h, layers = LISTS[name](orc)
    want = restated(name)
    # (first the restatement: edited inputs cannot quietly turn this into a one-layer test)
    assert want["n_rays"] == layers, (name, want["n_rays"])
    lights = LIGHTS["bench"]
    s = make("two_way")
    s.set_lights(lights)
    t, st = s.tree_of_rays(rays, w)
    assert_tree_is_restated(s, t, orc, want, name)
    for c in COUNTERS:
        print(name, c, st[c], want[c])
        assert st[c] == want[c]
    assert s.abi.raytree_info(t)["chunk"] == (0, 0, w, h)
    assert differing(s.abi.raytree_shade(t, lights)["rgb"], rr.shade(orc, want, lights, w, h), name + " shade") == 0
    if name.startswith("orthographic"):
        assert (rays[:, 3] == 0.0).all() and (rays[:, 4] == 0.0).all()
        hits = int((~np.isnan(s.abi.raytree_read_layer(t, 0, ("point",))["point"][:, 0])).sum())
        print(name, "first hits", hits)
        assert hits == 67


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_a_wave_ends_inside_at_and_past_an_item(n, make, two_way):
    """n x 1 lists of the panorama's first rays: the list's last wave ends inside, at and past an item of 64."""
    orc, _ = two_way
    lights = LIGHTS["bench"]
    rays = rl.panorama_rays(40, 20)[:n]
    want = rl.build_from_rays(orc, rays, n, 1, lights, 5)
    s = make("two_way")
    s.set_lights(lights)
    t, st = s.tree_of_rays(rays)
    assert_tree_is_restated(s, t, orc, want, "%d x 1" % n)
    assert st["rays_primary"] == n and st["shaded_hits"] == want["shaded_hits"]
    assert np.array_equal(s.abi.raytree_read_layer(t, 0, ("pixel",))["pixel"], np.arange(n))
    assert differing(s.abi.raytree_shade(t, lights)["rgb"], rr.shade(orc, want, lights, n, 1), "%d x 1 shade" % n) == 0
    got = s.abi.trace_rays(s.h, rays)
    assert got["rgb"].shape == (1, n, 3) and differing(got["rgb"], rr.shade(orc, want, lights, n, 1), "mt_trace_rays") == 0


# ---- the relight family

def test_relight_family_on_the_panorama(make, two_way):
    orc, restated = two_way
    name = "panorama 40x20"
    rays, w, h, _ = LISTS[name](orc)
    want = restated(name)
    lights = LIGHTS["bench"]
    s = make("two_way")
    s.set_lights(lights)
    t, _ = s.tree_of_rays(rays, w)
    before = None
    for k in (None, 0, 1, 2, 3):  # colour edits, from the old tree, against the restatement's bytes
        new = lights if k is None else lr.edited(lights, k)
        got = s.abi.raytree_shade(t, new)
        assert differing(got["rgb"], rr.shade(orc, want, new, w, h), "panorama, edit %s" % k) == 0
        assert all(got["stats"][c] == 0 for c in binding.STAT_NAMES)
        if k is None:
            before = got["rgb"]
        elif k == 0:
            assert (got["rgb"] != before).any()  # the edit is visible
    # a moved light: update == a fresh tree under the moved lights, bit for bit
    A, B, moved = ru.lights_before_and_after("two_way")
    assert A == [tuple(float(v) for v in l) for l in lights]
    s.set_lights(B)
    st = s.abi.raytree_update_lights(t, [moved])
    fresh, _ = s.tree_of_rays(rays, w)
    assert_same_trees(s, fresh, t, "panorama, updated vs fresh under the moved lights")
    assert_tree_is_restated(s, t, orc, restated(name, "moved"), "panorama, updated")
    print("update: %d shadow rays" % st["rays_shadow"])
    assert st["rays_primary"] == st["rays_secondary"] == 0 and st["rays_shadow"] > 0
    assert (s.abi.raytree_shade(t, B)["rgb"] != before).any()


@pytest.mark.parametrize("which", ["none", "nine"])
def test_zero_lights_and_more_lights_than_travel_with_the_launch(which, make, two_way):
    orc, restated = two_way
    name = "panorama 21x13"
    rays, w, h, _ = LISTS[name](orc)
    lights = LIGHTS[which]
    want = restated(name, which)
    s = make("two_way")
    s.set_lights(lights)
    t, st = s.tree_of_rays(rays, w)
    assert_tree_is_restated(s, t, orc, want, "%s, %d lights" % (name, len(lights)))
    assert s.abi.raytree_info(t)["n_lights"] == len(lights) and st["rays_shadow"] == want["rays_shadow"]
    assert (st["rays_shadow"] == 0) == (which == "none")
    rgb = s.abi.raytree_shade(t, lights)["rgb"]
    assert differing(rgb, rr.shade(orc, want, lights, w, h), "%d lights" % len(lights)) == 0
    color = s.abi.raytree_shade_colors(t, lights)["color"]
    assert np.array_equal(rr.v3d_to_rgb(color.reshape(-1, 3)), rgb.reshape(-1, 3))
    got = s.abi.trace_rays(s.h, rays, w)  # (the scene's current lights)
    assert differing(got["rgb"], rgb, "mt_trace_rays, %d lights" % len(lights)) == 0
    assert same_bits(got["color"], color, "mt_trace_rays colours") == 0
    if which == "nine":
        new = lr.edited(lights, 0)
        assert differing(s.abi.raytree_shade(t, new)["rgb"], rr.shade(orc, want, new, w, h), "nine lights, edited") == 0
        with pytest.raises(RuntimeError, match="8 lights for a ray tree made with 9"):
            s.abi.raytree_shade_colors(t, lights[:8])


# ---- linear colours

def orc_bytes(color):
    """MythTracer::V3DtoRGB as the oracle's library has it, ray by ray."""
    return np.array([orclib.v3d_to_rgb(c) for c in color.reshape(-1, 3)], dtype=np.uint8)


def specular_bound(ref):
    """The bound test_linear_colours derives for a colour with specular terms below it (tests/test_gpu_hostile.py imports
    it): ulps x lights x layers with factors of order one, 1e-12 max(1, |c|)."""
    return 1e-12 * np.maximum(1.0, np.abs(ref))


@pytest.mark.parametrize("kind", ["sensor", "panorama"])
def test_linear_colours(kind, make, two_way):
    """V3DtoRGB of mt_raytree_shade_colors[_device] is mt_raytree_shade's bitmap exactly.  Against the restatement's
    doubles: the same bits in every ray whose subtree added no specular term; elsewhere |d| <= 1e-12 max(1, |c|) --
    device and numpy pow may differ by an ulp or two per specular term, a ray sums at most lights x layers of them with
    factors of order one, and an ulp of a colour of order one is 2.2e-16."""
    import torch
    orc, restated = two_way
    lights = LIGHTS["bench"]
    s = make("two_way")
    s.set_lights(lights)
    if kind == "sensor":
        w, h = W, H
        t, _ = s.tree(rr.CAMERAS["two_way"], w, h)
        want = rr.build(orc, rr.CAMERAS["two_way"], w, h, lights, 5)
    else:
        rays, w, h, _ = LISTS["panorama 40x20"](orc)
        t, _ = s.tree_of_rays(rays, w)
        want = restated("panorama 40x20")
    largest = 0.0
    for k in (None, 0):
        new = lights if k is None else lr.edited(lights, k)
        rgb = s.abi.raytree_shade(t, new)["rgb"]
        got = s.abi.raytree_shade_colors(t, new)
        color = got["color"]
        assert color.shape == (h, w, 3) and got["stats"]["kernel_ms"] > 0
        assert all(got["stats"][c] == 0 for c in binding.STAT_NAMES)
        assert differing(orc_bytes(color), rgb, "%s edit %s: V3DtoRGB(colours) vs mt_raytree_shade" % (kind, k)) == 0
        print("%s edit %s: %d channels above 1.0, largest %.6f" % (kind, k, int((color > 1.0).sum()), color.max()))
        # the device form on a torch stream
        stream = torch.cuda.Stream()
        d_color = torch.full((h, w, 3), -1.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            s.abi.raytree_shade_colors_device(t, new, d_color.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
        stream.synchronize()
        assert same_bits(d_color.cpu().numpy(), color, "%s edit %s: device form vs host form" % (kind, k)) == 0
        # against the restatement's doubles
        term = {}
        ref = rl.colors(orc, want, new, term)
        spec = term["specular"]
        c = color.reshape(-1, 3)
        plain = same_bits(c[~spec], ref[~spec], "%s edit %s: rays without a specular term" % (kind, k))
        assert plain == 0 and (~spec).any() and spec.any()
        d = np.abs(c[spec] - ref[spec])
        bound = specular_bound(ref[spec])
        largest = max(largest, float(d.max()))
        print("%s edit %s: %d rays with a specular term, largest |d| %.3e (largest colour %.3f), %d channels not bit-equal"
              % (kind, k, int(spec.sum()), d.max(), np.abs(ref[spec]).max(), int((d > 0).sum())))
        assert (d <= bound).all()
    print("%s: largest difference to the restatement's colours %.3e" % (kind, largest))


# ---- mt_trace_rays

def test_trace_rays_is_create_shade_destroy(make, two_way):
    orc, _ = two_way
    rays, w, h, _ = LISTS["panorama 40x20"](orc)
    lights = LIGHTS["one"]
    s = make("two_way")
    s.set_lights(lights)
    t, st = s.tree_of_rays(rays, w)
    rgb = s.abi.raytree_shade(t, lights)["rgb"]
    color = s.abi.raytree_shade_colors(t, lights)["color"]
    s.destroy(t)
    got = s.abi.trace_rays(s.h, rays, w)
    assert differing(got["rgb"], rgb, "mt_trace_rays bytes") == 0
    assert same_bits(got["color"], color, "mt_trace_rays colours") == 0
    for name in binding.STAT_NAMES:
        print("mt_trace_rays", name, got["stats"][name], st[name])
    for name in COUNTERS:
        assert got["stats"][name] == st[name]
    assert got["stats"]["kernel_ms"] > 0 and got["stats"]["total_ms"] >= got["stats"]["kernel_ms"]
    only_rgb = s.abi.trace_rays(s.h, rays, w, color=False)
    only_color = s.abi.trace_rays(s.h, rays, w, rgb=False)
    assert "color" not in only_rgb and differing(only_rgb["rgb"], rgb, "bytes only") == 0
    assert "rgb" not in only_color and same_bits(only_color["color"], color, "colours only") == 0
    # a list with its own in_object and coef, n x 1
    io = (np.arange(w * h) % 3 == 0).astype(np.uint8)
    coef = np.where(np.arange(w * h) % 5 == 0, 0.005, 0.75)
    want = rl.build_from_rays(orc, rays, w * h, 1, lights, 5, in_object=io, coef=coef)
    got = s.abi.trace_rays(s.h, rays, None, in_object=io, coef=coef)
    print("with in_object and coef: layers", want["n_rays"])
    assert want["n_rays"] != [800, 392, 99, 9]
    assert differing(got["rgb"], rr.shade(orc, want, lights, w * h, 1), "mt_trace_rays with in_object and coef") == 0


def test_frame_kernels_are_untouched_by_the_calls(make):
    """A depth-5 frame before and after a ray-list tree, its shades and an mt_trace_rays is byte-identical, the calls
    add no entry to mt_scene_kernel_times, and the second frame is the repeated launch it would have been."""
    w, h = 1920, 1080
    cam = scenegen.ROOM_CAMERA
    sens = binding.sensor(cam, w, h)
    s = make("room")
    s.set_lights(lr.BENCH_LIGHTS)
    s.abi.set_engine(s.h, 1)
    s.abi.kernel_times(s.h)
    f1 = s.abi.render_chunk(s.h, sens, w, h)["rgb"]
    rays = rl.panorama_rays(64, 32, eye=cam[:3])
    t, st = s.tree_of_rays(rays, 64)
    print("room panorama: layers", s.abi.raytree_info(t)["n_rays"])
    assert st["rays_secondary"] > 0
    s.abi.raytree_shade(t, lr.edited(lr.BENCH_LIGHTS, 0))  # (does not touch the scene's lights)
    s.abi.raytree_shade_colors(t, lr.BENCH_LIGHTS)
    s.abi.trace_rays(s.h, rays, 64)
    f2 = s.abi.render_chunk(s.h, sens, w, h)["rgb"]
    assert np.array_equal(f1, f2)
    pm, rm = s.abi.kernel_times(s.h)
    print("primary_ms", pm, "render_ms", rm)
    assert len(pm) == 2, pm
    assert pm[1] < pm[0] / 3, pm  # second frame: the order kernels, not primary_kernel (see test_gpu_gbuffer.py)


# ---- refusals of the device form

@pytest.mark.parametrize("what", ["a NaN", "a zero direction"])
def test_the_device_form_refuses_a_bad_ray_before_it_traces(what, make, two_way):
    """One bad ray at index 70 of 130, in device memory where the host cannot scan: NULL, MT_ERR_ARG's message with the
    count and the index, no work counter moved; the next valid call on the same scene gives the right tree."""
    import torch
    orc, _ = two_way
    lights = LIGHTS["bench"]
    good = rl.panorama_rays(13, 10)
    bad = good.copy()
    if what == "a NaN":
        bad[70, 1] = np.nan
    else:
        bad[70, 3:] = 0.0
    s = make("two_way")
    s.set_lights(lights)
    d_bad, d_good = torch.from_numpy(bad).cuda(), torch.from_numpy(good).cuda()
    torch.cuda.synchronize()
    for w, h in ((130, 1), (13, 10)):
        rays = binding.mt_ray_list(d_bad.data_ptr(), None, None, w, h)
        st = binding.mt_stats()
        t = s.abi.lib.mt_raytree_create_rays_device(s.h, ctypes.addressof(rays), 5, ctypes.addressof(st))
        assert not t
        assert s.abi.last_error() == "1 rays of the list cannot be traced, the first at index 70", s.abi.last_error()
        counters = s.abi.read_stats(s.h)
        print(what, (w, h), "counters after the refusal", counters)
        assert all(counters[c] == 0 for c in binding.STAT_NAMES)
    with pytest.raises(RuntimeError, match="mt_raytree_create_rays_device: 1 rays of the list cannot be traced"):
        s.abi.raytree_create_rays(s.h, d_bad, 13, device=True)
    with pytest.raises(RuntimeError, match="mt_raytree_create_rays: 1 rays of the list cannot be traced, the first at index 70"):
        s.abi.raytree_create_rays(s.h, bad, 13)  # (the host form finds it on the host)
    t, st = s.tree_of_rays(d_good, 13, device=True)
    want = rl.build_from_rays(orc, good, 13, 10, lights, 5)
    assert_tree_is_restated(s, t, orc, want, "after the refusal")
    assert st["rays_primary"] == 130 and st["rays_secondary"] == want["rays_secondary"] > 0


# ---- facade and Python

def test_facade_and_python_round_trip(make, two_way):
    """MythTracer::BuildRayTree(rays, width), ShadeRayTree(tree, &colours), UpdateRayTree and TraceRays through the
    mth_ wrappers, against the ABI calls."""
    orc, _ = two_way
    rays, w, h, layers = LISTS["panorama 40x20"](orc)
    lights = LIGHTS["bench"]
    s = make("two_way")
    s.set_lights(lights)
    t, st = s.tree_of_rays(rays, w, 3)
    rgb = s.abi.raytree_shade(t, lights)["rgb"]
    color = s.abi.raytree_shade_colors(t, lights)["color"]
    m = M.MythTracer(rr.TWO_WAY)
    m.set_lights(lights)
    tree = m.raytree_rays(rays, w, max_depth=3)
    info = tree.info
    print("facade:", info["n_rays"], tree.counters)
    assert info["from_rays"] == 1 and info["max_depth"] == 3 and info["chunk"] == (0, 0, w, h)
    assert info["n_rays"] == s.abi.raytree_info(t)["n_rays"] == layers[:4]
    for name in COUNTERS:
        assert tree.counters[name] == st[name]
    assert tree.kernel_ms > 0
    assert differing(tree.shade()["rgb"], rgb, "facade shade") == 0
    assert same_bits(tree.shade_colors()["color"], color, "facade colours") == 0
    got = m.trace_rays(rays, w)
    assert got["color"].shape == (w * h, 3) and got["rgb"].shape == (w * h, 3)
    assert differing(got["rgb"], rgb, "facade TraceRays bytes") == 0
    assert same_bits(got["color"], color.reshape(-1, 3), "facade TraceRays colours") == 0
    for name in COUNTERS:
        assert got["counters"][name] == st[name]
    assert "color" not in m.trace_rays(rays, w, color=False)
    # n x 1: the same colours in the same (caller's) order
    plain = m.trace_rays(rays, 0)
    assert same_bits(plain["color"], color.reshape(-1, 3), "facade TraceRays, n x 1") == 0
    # the relight family through the facade
    new = lr.edited(lights, 0)
    assert differing(tree.shade(lights=new)["rgb"], s.abi.raytree_shade(t, new)["rgb"], "facade shade, edited") == 0
    A, B, moved = ru.lights_before_and_after("two_way")
    up = tree.update([moved], lights=B)
    s.set_lights(B)
    s.abi.raytree_update_lights(t, [moved])
    assert up["counters"]["rays_shadow"] > 0
    assert same_bits(tree.shade_colors()["color"], s.abi.raytree_shade_colors(t, B)["color"], "facade, moved light") == 0
    bad = rays.copy()
    bad[70, 4] = np.inf
    with pytest.raises(RuntimeError, match="1 rays of the list cannot be traced, the first at index 70"):
        m.raytree_rays(bad, w)
    with pytest.raises(RuntimeError, match="1 rays of the list cannot be traced, the first at index 70"):
        m.trace_rays(bad, w)
    m.set_lights(lights[:2])
    with pytest.raises(RuntimeError, match="another number of lights"):
        tree.shade_colors()
    tree.close()
    m.close()
