"""The ray-tree buffer, the parts that need no GPU (include/mythtracer_hip.h, mt_raytree_create ff.).

a. The RESTATEMENT the GPU tests lean on (tests/raytree_ref.py) is pinned to the oracle: on cornell, mini, room and
   two_way at 96x54, under the bench's three lights and under one light, for max_depth 0 .. 5 (and 7 on room, whose
   frames still change up to there), shade(restated tree, lights) is OracleScene.render(max_level = d) byte for byte,
   every pixel -- and again, from the SAME tree, for the four colour edits of lightbuffer_ref.edited against a fresh
   oracle render under those colours.  The tree's ray counts are the oracle's rays_secondary, rays_shadow and
   shaded_hits.  Layer 0 is held to gbuffer_ref.oracle_gbuffer and lightbuffer_ref (planes, loops, direct frame), so the
   restated plane rules and direct term are those modules', not a second opinion.
b. The inputs are worth testing: deep layers, rays with both children, reflections refused by the coefficient alone and
   by in_object alone, glass crossed by a shadow loop of a secondary ray.
c. The symbols exist, the ABI version is still 5, the argument checks that can be reached without a device come before
   any device call in the documented order, and the Python bindings and the facade refuse bad input before they need one.
"""
import ctypes

import numpy as np
import pytest

import gbuffer_ref
import lightbuffer_ref as lr
import orclib
import raytree_ref as rr

import mythtracer_amd as M
from mythtracer_amd import binding, tiling

MT_ERR_ARG, MT_ERR_HIP = -1, -2
W, H = 96, 54
SCENES = ["cornell", "mini", "room", "two_way"]
DEEPEST = {"room": 7}  # else 5
SYMBOLS = ("mt_raytree_create", "mt_raytree_destroy", "mt_raytree_info", "mt_raytree_read_layer", "mt_raytree_shade",
           "mt_raytree_shade_device")


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    return native_libs


@pytest.fixture(scope="module")
def restated(scenes):
    """(scene, light set) -> (oracle, the restated tree at the scene's deepest level), made once."""
    made, oracles = {}, {}

    def get(scene, which):
        if scene not in oracles:
            oracles[scene] = orclib.OracleScene(rr.TWO_WAY if scene == "two_way" else scenes[scene])
        if (scene, which) not in made:
            lights = lr.light_sets(scene)[which]
            made[scene, which] = rr.build(oracles[scene], rr.CAMERAS[scene], W, H, lights, DEEPEST.get(scene, 5))
        return oracles[scene], made[scene, which]
    return get


def differing(a, b, what):
    n = int((a != b).any(axis=-1).sum())
    print("%s: %d of %d pixels differ" % (what, n, a.shape[0] * a.shape[1]))
    return n


# ---- a. the restatement against the oracle

@pytest.mark.parametrize("which", ["bench", "one"])
@pytest.mark.parametrize("scene", SCENES)
def test_restated_tree_shades_to_the_oracles_frame(scene, which, restated):
    orc, deep = restated(scene, which)
    lights = lr.light_sets(scene)[which]
    cam = rr.CAMERAS[scene]
    depths = list(range(6)) + ([7] if scene == "room" else [])
    previous = None
    for d in depths:
        tree = rr.truncated(deep, d)
        orc.set_lights(lights)
        want = orc.render(cam, W, H, max_level=d)
        got = rr.shade(orc, tree, lights, W, H)
        assert got.shape == want["rgb"].shape == (H, W, 3)
        assert differing(got, want["rgb"], "%s %s d=%d" % (scene, which, d)) == 0
        print("  layers", tree["n_rays"], "secondary", tree["rays_secondary"], "shadow", tree["rays_shadow"])
        assert tree["rays_primary"] == want["counters"]["rays_primary"] == W * H
        assert tree["rays_secondary"] == want["counters"]["rays_secondary"]
        assert tree["rays_shadow"] == want["counters"]["rays_shadow"]
        assert tree["shaded_hits"] == want["counters"]["shaded_hits"]
        if previous is not None and scene in ("mini", "room") and d <= (7 if scene == "room" else 5):
            changed = int((previous != want["rgb"]).any(axis=-1).sum())
            print("  level %d changes %d pixels of the oracle's frame" % (d, changed))
        previous = want["rgb"]
        for k in range(4):  # edited colours, the OLD tree, a fresh oracle render
            new = lr.edited(lights, k)
            orc.set_lights(new)
            fresh = orc.render(cam, W, H, max_level=d)["rgb"]
            assert differing(rr.shade(orc, tree, new, W, H), fresh, "%s %s d=%d edit %d" % (scene, which, d, k)) == 0
            if k == 0:
                assert (fresh != want["rgb"]).any()  # the edit is visible


def test_a_truncated_tree_is_the_tree_built_shallower(restated):
    orc, deep = restated("two_way", "one")
    for d in (0, 2):
        a = rr.truncated(deep, d)
        b = rr.build(orc, rr.CAMERAS["two_way"], W, H, lr.light_sets("two_way")["one"], d)
        assert a["n_rays"] == b["n_rays"]
        for la, lb in zip(a["layers"], b["layers"]):
            for name in rr.F64_PLANES:
                assert gbuffer_ref.same_bits(la[name], lb[name], "d=%d %s" % (d, name)) == 0
            for name in rr.INT_PLANES:
                assert np.array_equal(la[name], lb[name]), (d, name)


@pytest.mark.parametrize("scene", ["cornell", "room"])
def test_layer_0_is_the_gbuffer_and_the_light_buffer(scene, restated):
    """Layer 0 in pixel order is gbuffer_ref.oracle_gbuffer + lightbuffer_ref.ref_lightbuffer, and its quantised direct
    term is lightbuffer_ref.shade: raytree_ref's plane rules and direct term are theirs."""
    orc, deep = restated(scene, "bench")
    lights = lr.light_sets(scene)["bench"]
    lay = deep["layers"][0]
    order = lay["pixel"]
    assert np.array_equal(order, tiling.raytree_layer0_order(W, H))
    gb = gbuffer_ref.oracle_gbuffer(orc, rr.CAMERAS[scene], W, H)
    lb = lr.ref_lightbuffer(orc, gb, lights)
    for name in ("point", "normal", "albedo"):
        assert gbuffer_ref.same_bits(lay[name], gb[name].reshape(-1, 3)[order], name) == 0
    assert np.array_equal(lay["material"], gb["material"].reshape(-1)[order])
    assert gbuffer_ref.same_bits(lay["ray"], gb["rays"].reshape(-1, 6)[order], "ray") == 0
    assert gbuffer_ref.same_bits(lay["power"], lb["power"].reshape(len(lights), -1, 3)[:, order], "power") == 0
    assert np.array_equal(lay["in_shadow"], lb["in_shadow"].reshape(len(lights), -1)[:, order])
    rgb = np.zeros((W * H, 3), dtype=np.uint8)
    rgb[order] = rr.v3d_to_rgb(rr.direct_term(orc, lay, lights))
    assert differing(rgb.reshape(H, W, 3), lr.shade(orc, gb, lb, lights), "direct term") == 0
    # the vectorised V3DtoRGB is the oracle's
    c = rr.direct_term(orc, lay, lr.edited(lights, 1))[:500] * 1.5 - 0.2
    assert np.array_equal(rr.v3d_to_rgb(c), np.array([orclib.v3d_to_rgb(v) for v in c]))


def test_layer_0_order():
    for cw, ch in ((1, 1), (8, 8), (9, 7), (63, 5), (64, 8), (65, 9), (96, 54), (61, 37)):
        order = tiling.raytree_layer0_order(cw, ch)
        assert sorted(order.tolist()) == list(range(cw * ch))  # every pixel once
        # the closed form of include/mythtracer_hip.h
        y, x = np.divmod(np.arange(cw * ch), cw)
        bw = np.minimum(8, cw - 8 * (x // 8))
        bh = np.minimum(8, ch - 8 * (y // 8))
        index = 8 * (y // 8) * cw + 8 * (x // 8) * bh + (y % 8) * bw + x % 8
        assert np.array_equal(order[index], np.arange(cw * ch)), (cw, ch)
    assert tiling.raytree_layer0_order(9, 2).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 8, 17]
    with pytest.raises(ValueError, match="empty"):
        tiling.raytree_layer0_order(0, 4)


# ---- b. the inputs are worth testing

def test_the_scenes_reach_every_branch(restated):
    for scene in ("mini", "room"):
        tree = rr.truncated(restated(scene, "bench")[1], 5)
        print("%s: rays per layer at d = 5: %s" % (scene, tree["n_rays"]))
        assert len(tree["n_rays"]) == 6 and all(n > 0 for n in tree["n_rays"])
    tree = restated("two_way", "bench")[1]
    both = sum(int(((l["child_refl"] >= 0) & (l["child_refr"] >= 0)).sum()) for l in tree["layers"])
    by_coef = sum(int(l["refused"]["by_coef"].sum()) for l in tree["layers"])
    by_in_object = sum(int(l["refused"]["by_in_object"].sum()) for l in tree["layers"])
    print("two_way: layers %s; %d rays with both children; reflection refused by coef alone %d, by in_object alone %d"
          % (tree["n_rays"], both, by_coef, by_in_object))
    assert both >= 50
    assert by_coef >= 1
    assert by_in_object >= 1
    room = rr.truncated(restated("room", "bench")[1], 5)
    glass = sum(int((l["iterations"] >= 2).sum()) for l in room["layers"][1:])
    print("room: %d shadow loops of >= 2 iterations in layers >= 1" % glass)
    assert glass >= 1


def test_no_material_of_the_other_scenes_goes_both_ways(scenes):
    """Why two_way exists: a ray has both children only on a material with Refl and Tr together."""
    for scene in ("cornell", "mini", "room"):
        for name, values, _ in orclib.OracleScene(scenes[scene]).materials():
            assert not (values[10] > 0.0 and values[11] > 0.0), (scene, name)
    pane = {n: v for n, v, _ in orclib.OracleScene(rr.TWO_WAY).materials()}["pane"]
    assert pane[10] > 0.0 and pane[11] > 0.0


# ---- c. symbols and argument checks

def test_symbols_and_abi_version():
    abi = M.hip_abi()
    assert binding.MT_ABI_VERSION == 5 == abi.lib.mt_abi_version()
    for name in SYMBOLS:
        assert name in M.HIP_SYMBOLS and getattr(abi.lib, name) is not None
    assert ctypes.sizeof(binding.mt_raytree_layer) == 12 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(binding.mt_raytree_desc) == 10 * 4 + 17 * 8 + 17 * 8 + 8
    assert list(binding.RAYTREE_PLANES) == ["ray", "in_object", "coef", "point", "normal", "albedo", "material", "power",
                                            "in_shadow", "child_refl", "child_refr", "pixel"]


def test_create_argument_checks_come_before_any_device_call():
    abi = M.hip_abi()
    sens = binding.mt_sensor()

    def create(scene, sensor, image, chunk, depth):
        t = abi.lib.mt_raytree_create(scene, ctypes.byref(sensor) if sensor is not None else None, image[0], image[1],
                                      *chunk, depth, None)
        assert not t
        return abi.last_error()

    # image size, then the chunk: mt_render_chunk's limits and messages -- before the scene, the sensor and max_depth
    for image in ((0, 8), (8, 0), (-1, 8), (100001, 8), (8, 100001)):
        assert create(None, None, image, (0, 0, 1, 1), -1) == "image size %dx%d out of range" % image
    for chunk in ((-1, 0, 4, 4), (0, 0, 0, 4), (5, 5, 4, 4), (0, 0, 9, 1), (8, 0, 1, 1), (0, 0, 2147483647, 1)):
        assert create(None, None, (8, 8), chunk, 99) == "chunk %d,%d %dx%d outside image 8x8" % chunk
    # the scene before the sensor and before max_depth
    assert create(None, None, (8, 8), (0, 0, 8, 8), -1) == "scene is NULL"
    assert create(None, sens, (8, 8), (0, 0, 8, 8), 17) == "scene is NULL"


def test_tree_argument_checks_come_before_any_device_call():
    abi = M.hip_abi()
    buf = np.zeros(64)
    p = buf.ctypes.data
    light = binding.mt_light()

    def arg_error(rc, text):
        assert rc == MT_ERR_ARG and rc != MT_ERR_HIP, (rc, abi.last_error())
        assert text in abi.last_error(), abi.last_error()

    for name in ("mt_raytree_shade", "mt_raytree_shade_device"):
        fn = getattr(abi.lib, name)
        # the bitmap, then the tree -- before the lights
        arg_error(fn(None, None, -1, None, None), "output bitmap is NULL")
        arg_error(fn(None, ctypes.addressof(light), 1, None, None), "output bitmap is NULL")
        arg_error(fn(None, None, -1, p, None), "ray tree is NULL")
        arg_error(fn(None, ctypes.addressof(light), 1, p, None), "ray tree is NULL")
    arg_error(abi.lib.mt_raytree_info(None, None), "ray tree is NULL")
    arg_error(abi.lib.mt_raytree_read_layer(None, -1, None), "ray tree is NULL")
    abi.lib.mt_raytree_destroy(None)  # NULL is fine


def test_python_bindings_refuse_bad_input():
    abi = M.hip_abi()
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.raytree_create(None, np.zeros(12), 8, 8)
    with pytest.raises(RuntimeError, match="chunk 4,4 8x8 outside image 8x8"):
        abi.raytree_create(None, np.zeros(12), 8, 8, chunk=(4, 4, 8, 8))
    with pytest.raises(RuntimeError, match="ray tree is NULL"):
        abi.raytree_info(None)
    with pytest.raises(RuntimeError, match="ray tree is NULL"):
        abi.raytree_read_layer(None, 0)
    with pytest.raises(RuntimeError, match="ray tree is NULL"):
        abi.raytree_shade(None, [(0.0,) * 12])


def test_facade_refuses_before_it_needs_a_device():
    cam = (50, 50, -120, 0, 0, 0, 60)
    m = M.MythTracer()
    m.set_devices([0, 0])
    with pytest.raises(RuntimeError, match="several devices"):
        m.raytree(cam, 8, 8)
    m2 = M.MythTracer()
    with pytest.raises(RuntimeError, match="empty chunk"):
        m2.raytree(cam, 8, 8, chunk=(0, 0, 0, 8))
    with pytest.raises(RuntimeError, match="recursion level 17 outside 0 .. 16"):
        m2.raytree(cam, 8, 8, max_depth=17)
    with pytest.raises(RuntimeError, match="recursion level -1 outside"):
        m2.raytree(cam, 8, 8, max_depth=-1)
    assert not m2.L.mth_raytree_shade(m2.h, None, None, 0, None)
    assert "RayTree is NULL" in m2.last_error()
