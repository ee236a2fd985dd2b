"""Ray-list trees and linear colours, the parts that need no GPU (include/mythtracer_hip.h, mt_raytree_create_rays ff.).

a. The five symbols exist, the ABI version is still 5, mt_raytree_desc kept its layout, and every argument check --
   the host form's scan of the list's content included -- answers MT_ERR_ARG with its message before any device call,
   in the documented order; the facade refuses bad input before it needs a device.
b. The rules of a ray-list tree (tests/raylist_ref.py), on cornell and two_way at 96x54 and depth 5: the sensor's rays
   handed in as a 96x54 list give the sensor tree of tests/raytree_ref.py in every plane of every layer, `pixel`
   included; layer k of a sensor tree handed in as an n x 1 list with its in_object and coef and max_depth - k gives
   that tree's layers k onwards.  Zero differing values.
c. The restated tree is held to the oracle on lists no sensor makes: its shade and its linear colours at n x 1 equal a
   per-ray restatement of TraceRayWorker (raylist_ref.trace_ray), whose own check is that every pixel ray of a sensor
   frame reproduces OracleScene.render's bytes.
"""
import ctypes

import numpy as np
import pytest

import gbuffer_ref
import lightbuffer_ref as lr
import orclib
import raylist_ref as rl
import raytree_ref as rr

import mythtracer_amd as M
from mythtracer_amd import binding

MT_ERR_ARG, MT_ERR_HIP = -1, -2
W, H = 96, 54
SYMBOLS = ("mt_raytree_create_rays", "mt_raytree_create_rays_device", "mt_raytree_shade_colors",
           "mt_raytree_shade_colors_device", "mt_trace_rays")
PLANES = rr.F64_PLANES + rr.INT_PLANES + ("material", "prim", "iterations")


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    return native_libs


@pytest.fixture(scope="module")
def sensor_trees(scenes):
    """scene -> (oracle, lights, the sensor tree of raytree_ref at 96x54 and depth 5), made once and left unchanged."""
    made = {}

    def get(scene):
        if scene not in made:
            orc = orclib.OracleScene(rr.TWO_WAY if scene == "two_way" else scenes[scene])
            lights = lr.light_sets(scene)["bench"]
            made[scene] = (orc, lights, rr.build(orc, rr.CAMERAS[scene], W, H, lights, 5))
        return made[scene]
    return get


def differing_values(a, b, what, first=0):
    """The number of differing values between tree `a` from layer `first` on and tree `b`: doubles by their bits with
    NaN = NaN, everything else exactly."""
    print(what, a["n_rays"][first:], b["n_rays"])
    assert a["n_rays"][first:] == b["n_rays"]
    total = 0
    for k, (la, lb) in enumerate(zip(a["layers"][first:], b["layers"])):
        for name in PLANES + (("pixel",) if k == 0 and first == 0 else ()):
            if name in rr.F64_PLANES:
                total += gbuffer_ref.same_bits(lb[name], la[name], "%s layer %d %s" % (what, k, name))
            else:
                assert lb[name].shape == la[name].shape, (what, k, name)
                total += int((lb[name] != la[name]).sum())
    print("%s: %d differing values" % (what, total))
    return total


# ---- a. symbols, argument checks, facade

def test_symbols_abi_version_and_layout():
    abi = M.hip_abi()
    assert binding.MT_ABI_VERSION == 5 == abi.lib.mt_abi_version()
    for name in SYMBOLS:
        assert name in M.HIP_SYMBOLS and getattr(abi.lib, name) is not None
    for name in ("mth_raytree_build_rays", "mth_raytree_shade_colors", "mth_trace_rays"):
        assert getattr(M.host_lib(), name) is not None
    # the desc kept its size; from_rays stands where `reserved` stood
    assert ctypes.sizeof(binding.mt_raytree_desc) == 10 * 4 + 17 * 8 + 17 * 8 + 8
    assert binding.mt_raytree_desc.from_rays.offset == 9 * 4
    assert ctypes.sizeof(binding.mt_ray_list) == 3 * ctypes.sizeof(ctypes.c_void_p) + 8
    for name in ("raytree_create_rays", "raytree_shade_colors", "raytree_shade_colors_device", "trace_rays"):
        assert callable(getattr(abi, name))


def good_rays(n):
    r = np.zeros((n, 6))
    r[:, 0:3] = (150.0, 125.0, 200.0)
    r[:, 3:] = (0.0, 0.0, 2.0)  # two exact zeros, not normalised: valid
    r[::2, 3:] = (1.0, 0.0, 0.5)
    return r


def test_create_argument_checks_come_before_any_device_call():
    abi = M.hip_abi()
    r = good_rays(130)
    # the checks up to the list's content read nothing of the scene but whether it is NULL: any address stands for one
    no_scene = np.zeros(8192, dtype=np.uint8)
    scene = no_scene.ctypes.data

    def create(fn, s, rays, depth):
        t = fn(s, ctypes.addressof(rays) if rays is not None else None, depth, None)
        assert not t
        return abi.last_error()

    def ray_list(w, h, ray=r, in_object=None, coef=None):
        keep.extend([ray, in_object, coef])
        return binding.mt_ray_list(ray.ctypes.data if ray is not None else None,
                                   in_object.ctypes.data if in_object is not None else None,
                                   coef.ctypes.data if coef is not None else None, w, h)

    keep = []
    for name in ("mt_raytree_create_rays", "mt_raytree_create_rays_device"):
        fn = getattr(abi.lib, name)
        # 1. the list, before its size, the scene and max_depth
        assert create(fn, None, None, 99) == "the ray list is NULL"
        assert create(fn, None, ray_list(0, 0, ray=None), 99) == "the ray list is NULL"
        # 2. the size, before the scene and max_depth
        for w, h in ((0, 1), (1, 0), (-1, 1), (5, -2)):
            assert create(fn, None, ray_list(w, h), 99) == "ray list size %dx%d out of range" % (w, h)
        for w, h in ((65536, 32768), (2147483647, 2), (2147483647, 2147483647)):
            assert create(fn, None, ray_list(w, h), 99) == \
                "layer 0 of the ray tree would have %d rays (2^31 or more)" % (w * h)
        # 3. the scene, before max_depth (and 100000 per side is no limit here)
        assert create(fn, None, ray_list(130, 1), 99) == "scene is NULL"
        assert create(fn, None, ray_list(200000, 1), -1) == "scene is NULL"
        # 4. max_depth
        for depth in (-1, 17):
            assert create(fn, scene, ray_list(130, 1), depth) == "max_depth %d outside [0, 16]" % depth
    # 5. the host form: the content of the list
    fn = abi.lib.mt_raytree_create_rays

    def refused(count, first, **planes):
        ray = planes.pop("ray", r)
        for w, h in ((130, 1), (13, 10)):
            got = create(fn, scene, ray_list(w, h, ray=ray, **planes), 5)
            assert got == "%d rays of the list cannot be traced, the first at index %d" % (count, first), got

    bad = r.copy()
    bad[7, 1] = np.nan  # a NaN origin
    refused(1, 7, ray=bad)
    bad = r.copy()
    bad[129, 4] = -np.inf  # an infinite direction component
    refused(1, 129, ray=bad)
    bad = r.copy()
    bad[70, 3:] = 0.0  # a zero direction
    bad[71, 3:] = (0.0, -0.0, 0.0)
    bad[100, 0] = np.inf
    refused(3, 70, ray=bad)
    in_object = np.zeros(130, dtype=np.uint8)
    in_object[5] = 1  # valid
    in_object[64] = 2
    refused(1, 64, in_object=in_object)
    coef = np.full(130, 0.25)
    coef[0] = np.nan
    coef[3] = np.inf
    refused(2, 0, coef=coef)
    assert not no_scene.any()  # (and nothing wrote to what stood for the scene)


def test_shade_colors_and_trace_rays_argument_checks():
    abi = M.hip_abi()
    buf = np.zeros(64)
    p = buf.ctypes.data
    light = binding.mt_light()

    def arg_error(rc, text):
        assert rc == MT_ERR_ARG and rc != MT_ERR_HIP, (rc, abi.last_error())
        assert text in abi.last_error(), abi.last_error()

    for name in ("mt_raytree_shade_colors", "mt_raytree_shade_colors_device"):
        fn = getattr(abi.lib, name)
        # mt_raytree_shade's order: the output, then the tree -- before the lights
        arg_error(fn(None, None, -1, None, None), "output colours are NULL")
        arg_error(fn(None, ctypes.addressof(light), 1, None, None), "output colours are NULL")
        arg_error(fn(None, None, -1, p, None), "ray tree is NULL")
    r = good_rays(4)
    rays = binding.mt_ray_list(r.ctypes.data, None, None, 4, 1)
    # both outputs NULL comes first, then create's checks
    arg_error(abi.lib.mt_trace_rays(None, None, 99, None, None, None), "out_color and out_rgb are both NULL")
    arg_error(abi.lib.mt_trace_rays(None, None, 99, p, None, None), "the ray list is NULL")
    arg_error(abi.lib.mt_trace_rays(None, ctypes.addressof(rays), 99, None, p, None), "scene is NULL")
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.raytree_create_rays(None, r)
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.trace_rays(None, r, list_w=2)
    with pytest.raises(RuntimeError, match="ray tree is NULL"):
        abi.raytree_shade_colors(None, [(0.0,) * 12])
    with pytest.raises(ValueError, match="cannot be 3 wide"):
        abi.raytree_create_rays(None, r, list_w=3)
    with pytest.raises(ValueError, match="the same n rays"):
        abi.raytree_create_rays(None, r, coef=np.ones(3))


def test_facade_refuses_before_it_needs_a_device():
    r = good_rays(6)
    m = M.MythTracer()
    with pytest.raises(RuntimeError, match="the ray list is empty"):
        m.raytree_rays(np.zeros((0, 6)))
    with pytest.raises(RuntimeError, match="the ray list is empty"):
        m.trace_rays(np.zeros((0, 6)))
    for width in (4, 7, -1):
        with pytest.raises(RuntimeError, match="list_width %d does not divide the 6 rays" % width):
            m.raytree_rays(r, width)
        with pytest.raises(RuntimeError, match="list_width %d does not divide the 6 rays" % width):
            m.trace_rays(r, width)
    with pytest.raises(RuntimeError, match="both NULL"):
        m.trace_rays(r, color=False, rgb=False)
    with pytest.raises(RuntimeError, match="recursion level 17 outside 0 .. 16"):
        m.raytree_rays(r, max_depth=17)
    assert not m.L.mth_raytree_shade_colors(m.h, None, None, 0, None)
    assert "RayTree is NULL" in m.last_error()
    several = M.MythTracer()
    several.set_devices([0, 0])
    with pytest.raises(RuntimeError, match="several devices"):
        several.raytree_rays(r)
    with pytest.raises(RuntimeError, match="several devices"):
        several.trace_rays(r)


# ---- b. the rules of a ray-list tree

@pytest.mark.parametrize("scene", ["cornell", "two_way"])
def test_the_sensors_rays_as_a_list_give_the_sensor_tree(scene, sensor_trees):
    orc, lights, want = sensor_trees(scene)
    rays = gbuffer_ref.pixel_rays(rr.CAMERAS[scene], W, H).reshape(W * H, 6)
    got = rl.build_from_rays(orc, rays, W, H, lights, 5)
    assert differing_values(want, got, "%s as a %dx%d list" % (scene, W, H)) == 0
    assert len(want["n_rays"]) == (2 if scene == "cornell" else 6)
    for name in ("rays_primary", "rays_secondary", "rays_shadow", "shaded_hits"):
        assert got[name] == want[name]
    # the same rays un-permuted from the tree's own layer 0
    own = np.zeros((W * H, 6))
    own[want["layers"][0]["pixel"]] = want["layers"][0]["ray"]
    assert gbuffer_ref.same_bits(own, rays, "layer 0 un-permuted") == 0


@pytest.mark.parametrize("k", [1, 2])
def test_a_layer_as_a_list_gives_the_layers_below_it(k, sensor_trees):
    orc, lights, want = sensor_trees("two_way")
    lay = want["layers"][k]
    n = len(lay["ray"])
    got = rl.build_from_rays(orc, lay["ray"], n, 1, lights, 5 - k, in_object=lay["in_object"], coef=lay["coef"])
    assert len(got["layers"]) == 6 - k and n == {1: 4353, 2: 1561}[k]
    assert differing_values(want, got, "two_way from layer %d" % k, first=k) == 0
    assert np.array_equal(got["layers"][0]["pixel"], np.arange(n))
    assert lay["in_object"].any() and (lay["coef"] != 1.0).any()  # the list's own in_object and coef matter


# ---- c. the restatement against TraceRayWorker, ray by ray

def test_the_per_ray_restatement_renders_the_oracles_frame():
    """trace_ray over every pixel ray of a sensor frame, through V3DtoRGB, is OracleScene.render byte for byte."""
    scene, w, h = "two_way", W, H
    orc = orclib.OracleScene(rr.TWO_WAY)
    lights = lr.light_sets(scene)["bench"]
    orc.set_lights(lights)
    rays = gbuffer_ref.pixel_rays(rr.CAMERAS[scene], w, h).reshape(w * h, 6)
    got = rr.v3d_to_rgb(rl.trace_rays(orc, rays, lights, 5)).reshape(h, w, 3)
    want = orc.render(rr.CAMERAS[scene], w, h, max_level=5)
    n = int((got != want["rgb"]).any(axis=-1).sum())
    print("per-ray restatement vs the oracle: %d of %d pixels differ; %d secondary rays in the frame"
          % (n, w * h, want["counters"]["rays_secondary"]))
    assert n == 0 and want["counters"]["rays_secondary"] > 500


def lists_no_sensor_makes(orc):
    return {"panorama 21x13": (rl.panorama_rays(21, 13), [273, 133, 31, 4]),
            "panorama 40x20": (rl.panorama_rays(40, 20), [800, 392, 99, 9]),
            "orthographic (0, 0, 1)": (rl.orthographic_rays(orc, 20, 10), [200, 59, 26, 13, 26, 13]),
            "orthographic (0, 0, 2)": (rl.orthographic_rays(orc, 20, 10, direction=(0.0, 0.0, 2.0)),
                                       [200, 59, 26, 13, 26, 13])}


@pytest.mark.parametrize("which", ["bench", "one"])
def test_lists_no_sensor_makes_against_the_per_ray_restatement(which):
    orc = orclib.OracleScene(rr.TWO_WAY)
    lights = lr.light_sets("two_way")[which]
    for name, (rays, layers) in lists_no_sensor_makes(orc).items():
        n = len(rays)
        tree = rl.build_from_rays(orc, rays, n, 1, lights, 5)
        print(name, which, "layers", tree["n_rays"])
        assert tree["n_rays"] == layers
        want = rl.trace_rays(orc, rays, lights, 5)
        got = rl.colors(orc, tree, lights)
        # (the same numpy operations in the same order on both roads: the colours agree in every bit)
        assert gbuffer_ref.same_bits(got, want, name + " colours") == 0
        rgb = rr.shade(orc, tree, lights, n, 1).reshape(n, 3)
        assert np.array_equal(rgb, rr.v3d_to_rgb(want)) and rgb.any()
    # the layout does not matter to a ray: the 40x20 list traced as 40x20 gives the same colours
    rays = rl.panorama_rays(40, 20)
    a = rl.build_from_rays(orc, rays, 40, 20, lights, 5)
    b = rl.build_from_rays(orc, rays, 800, 1, lights, 5)
    assert a["n_rays"] == b["n_rays"] and not np.array_equal(a["layers"][0]["pixel"], b["layers"][0]["pixel"])
    assert gbuffer_ref.same_bits(rl.colors(orc, a, lights), rl.colors(orc, b, lights), "40x20 vs 800x1") == 0


def test_the_lists_reach_what_a_sensor_does_not():
    orc = orclib.OracleScene(rr.TWO_WAY)
    lights = lr.light_sets("two_way")["bench"]
    rays = rl.panorama_rays(40, 20)
    tree = rl.build_from_rays(orc, rays, 40, 20, lights, 5)
    hits = int((tree["layers"][0]["prim"] >= 0).sum())
    both = sum(int(((l["child_refl"] >= 0) & (l["child_refr"] >= 0)).sum()) for l in tree["layers"])
    cam_dir = rays[:, 5]  # (the scenes' cameras look along +z)
    print("panorama 40x20: %d first hits, %d rays with both children, %d rays with z < 0" % (hits, both, int((cam_dir < 0).sum())))
    assert hits == 394 and both == 19 and int((cam_dir < 0).sum()) == 400
    ortho = rl.orthographic_rays(orc, 20, 10)
    assert (ortho[:, 3] == 0.0).all() and (ortho[:, 4] == 0.0).all()
    a = rl.build_from_rays(orc, ortho, 20, 10, lights, 5)
    b = rl.build_from_rays(orc, rl.orthographic_rays(orc, 20, 10, direction=(0.0, 0.0, 2.0)), 20, 10, lights, 5)
    assert np.array_equal(a["layers"][0]["prim"], b["layers"][0]["prim"]) and a["n_rays"] == b["n_rays"]
