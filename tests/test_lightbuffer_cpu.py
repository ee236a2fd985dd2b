"""The direct-light buffer and the relight pass, the parts that need no GPU (include/mythtracer_hip.h,
mt_render_lightbuffer / mt_shade_direct).

a. The RESTATEMENT the GPU tests lean on (tests/lightbuffer_ref.py) is pinned to the oracle: on cornell, f2_decal, mini
   and room at 96x54, under the bench's three lights and under one light, shade(oracle G-buffer, restated light buffer,
   lights) is OracleScene.render(max_level=0) byte for byte, every pixel -- and again, with the SAME light buffer, for
   edited light colours against a fresh oracle render under those colours.  No byte may differ.
b. The restated light buffer is pinned, bit for bit, to goldens whose shadow rays the compiled reference's IntersectRay
   answered (tests/golden/make_lightbuffer_golden.py).
c. The symbols exist, the ABI version is still 5, and the argument checks of the four entry points come before any
   device call, in the documented order.
"""
import ctypes

import numpy as np
import pytest

import gbuffer_ref
import lightbuffer_ref as lr
import orclib

import mythtracer_amd as M
from mythtracer_amd import binding

MT_ERR_ARG, MT_ERR_HIP = -1, -2
W, H = 96, 54
SCENES = ["cornell", "f2_decal", "mini", "room"]
RENDER = ("mt_render_lightbuffer", "mt_render_lightbuffer_device")
SHADE = ("mt_shade_direct", "mt_shade_direct_device")


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    return native_libs


@pytest.fixture(scope="module")
def restated(scenes):
    """scene -> (oracle, oracle G-buffer, {light set: restated light buffer}), made once."""
    made = {}

    def get(scene):
        if scene not in made:
            orc = orclib.OracleScene(scenes[scene])
            gb = gbuffer_ref.oracle_gbuffer(orc, lr.CAMERAS[scene], W, H)
            made[scene] = (orc, gb, {k: lr.ref_lightbuffer(orc, gb, l) for k, l in lr.light_sets(scene).items()})
        return made[scene]
    return get


def differing(a, b, what):
    n = int((a != b).any(axis=-1).sum())
    print("%s: %d of %d pixels differ" % (what, n, a.shape[0] * a.shape[1]))
    return n


@pytest.mark.parametrize("which", ["bench", "one"])
@pytest.mark.parametrize("scene", SCENES)
def test_restated_relight_is_the_oracles_direct_frame(scene, which, restated):
    orc, gb, lbs = restated(scene)
    lights = lr.light_sets(scene)[which]
    lb = lbs[which]
    orc.set_lights(lights)
    want = orc.render(lr.CAMERAS[scene], W, H, max_level=0)
    got = lr.shade(orc, gb, lb, lights)
    assert got.shape == want["rgb"].shape == (H, W, 3)
    assert differing(got, want["rgb"], "%s %s" % (scene, which)) == 0
    # the counts the GPU test compares with: the oracle's own
    assert lb["rays_shadow"] == want["counters"]["rays_shadow"]
    assert int(((gb["prim"] >= 0)).sum()) == want["counters"]["shaded_hits"]
    # edited colours, the OLD light buffer, a fresh oracle render
    for k in range(4):
        new = lr.edited(lights, k)
        orc.set_lights(new)
        fresh = orc.render(lr.CAMERAS[scene], W, H, max_level=0)["rgb"]
        assert differing(lr.shade(orc, gb, lb, new), fresh, "%s %s edit %d" % (scene, which, k)) == 0
        if k == 0:
            assert (fresh != want["rgb"]).any()  # the edit is visible


def test_the_scenes_cover_glass_and_all_three_outcomes(restated):
    _, _, lbs = restated("room")
    it = lbs["bench"]["iterations"]
    print("room: %d loops of >= 2 iterations, longest %d" % (int((it >= 2).sum()), int(it.max())))
    assert (it >= 2).any()
    _, gb, lbs = restated("cornell")
    s = lbs["one"]["in_shadow"]
    counts = [int((s == v).sum()) for v in (0, 1, 255)]
    print("cornell, one light: lit / shadowed / no loop", counts)
    assert all(counts)
    assert np.isnan(lbs["one"]["power"][s == 255]).all() and not np.isnan(lbs["one"]["power"][s != 255]).any()
    assert np.array_equal(s[0] == 255, gb["prim"] < 0)


@pytest.mark.parametrize("scene", ["cornell", "mini", "room"])
def test_restatement_reproduces_the_reference_made_goldens(scene, restated):
    g = lr.load_golden(scene)
    _, _, lbs = restated(scene)
    assert np.array_equal(g["cam"], np.array(lr.CAMERAS[scene]))
    for key, lights in lr.light_sets(scene).items():
        assert np.array_equal(g["lights_" + key], np.array(lights))
        lb = lbs[key]
        assert gbuffer_ref.same_bits(lb["power"], g["power_" + key], "%s %s power" % (scene, key)) == 0
        assert np.array_equal(lb["in_shadow"], g["in_shadow_" + key])
        assert np.array_equal(lb["iterations"], g["iterations_" + key])


def test_the_goldens_cover_glass_and_all_three_outcomes():
    glass = mixes = 0
    for scene in ("cornell", "mini", "room"):
        g = lr.load_golden(scene)
        for key in ("bench", "one"):
            glass += int((g["iterations_" + key] >= 2).sum())
            mixes += int(all(int((g["in_shadow_" + key] == v).sum()) for v in (0, 1, 255)))
        assert int(g["glass_loops"]) == sum(int((g["iterations_" + k] >= 2).sum()) for k in ("bench", "one"))
    print("goldens: %d loops of >= 2 iterations, %d (scene, lights) with all three outcomes" % (glass, mixes))
    assert glass > 0 and mixes > 0


# ---- c. symbols and argument checks

def _call(abi, name, scene, sens, image, chunk, gb, lb, lights=None, n_lights=0, rgb=None):
    fn = getattr(abi.lib, name)
    head = [scene, ctypes.byref(sens) if sens is not None else None, image[0], image[1], *chunk,
            ctypes.byref(gb) if gb is not None else None, ctypes.byref(lb) if lb is not None else None]
    if name in RENDER:
        return fn(*head, None)
    return fn(*head, lights, n_lights, rgb, None)  # (stats or stream)


def test_symbols_and_abi_version():
    abi = M.hip_abi()
    assert binding.MT_ABI_VERSION == 5 == abi.lib.mt_abi_version()
    for name in RENDER + SHADE:
        assert name in M.HIP_SYMBOLS and getattr(abi.lib, name) is not None
    assert ctypes.sizeof(binding.mt_lightbuffer) == 2 * ctypes.sizeof(ctypes.c_void_p)
    assert list(binding.LIGHTBUFFER_PLANES) == ["power", "in_shadow"]


@pytest.mark.parametrize("name", RENDER)
def test_lightbuffer_argument_checks_come_before_any_device_call(name):
    abi = M.hip_abi()
    buf = np.zeros(64)
    sens = binding.mt_sensor()
    power = binding.mt_lightbuffer(power=buf.ctypes.data)
    shadow = binding.mt_lightbuffer(in_shadow=buf.ctypes.data)

    def arg_error(rc, text):
        assert rc == MT_ERR_ARG and rc != MT_ERR_HIP, (name, rc, abi.last_error())
        assert text in abi.last_error(), (name, abi.last_error())

    for lb in (power, shadow):
        arg_error(_call(abi, name, None, sens, (8, 8), (0, 0, 8, 8), None, lb), "scene is NULL")
        assert abi.last_error() == "scene is NULL"
    # `lb` before everything else; a G-buffer does not stand in for it
    arg_error(_call(abi, name, None, sens, (0, 8), (0, 0, 8, 8), None, None), "mt_lightbuffer is NULL")
    arg_error(_call(abi, name, None, sens, (0, 8), (0, 0, 8, 8), None, binding.mt_lightbuffer()), "no plane of the mt_lightbuffer")
    arg_error(_call(abi, name, None, sens, (8, 8), (0, 0, 8, 8), binding.mt_gbuffer(depth=buf.ctypes.data),
                    binding.mt_lightbuffer()), "no plane of the mt_lightbuffer")
    # image size, then the chunk: mt_render_chunk's limits and messages
    for image in ((0, 8), (8, 0), (-1, 8), (100001, 8), (8, 100001)):
        arg_error(_call(abi, name, None, sens, image, (0, 0, 1, 1), None, power), "image size %dx%d out of range" % image)
    for chunk in ((-1, 0, 4, 4), (0, 0, 0, 4), (5, 5, 4, 4), (0, 0, 9, 1), (8, 0, 1, 1), (0, 0, 2147483647, 1)):
        arg_error(_call(abi, name, None, sens, (8, 8), chunk, None, power), "chunk %d,%d %dx%d outside image 8x8" % chunk)
    # the scene before the sensor
    arg_error(_call(abi, name, None, None, (8, 8), (0, 0, 8, 8), None, power), "scene is NULL")


@pytest.mark.parametrize("name", SHADE)
def test_shade_argument_checks_come_before_any_device_call(name):
    abi = M.hip_abi()
    buf = np.zeros(64)
    p = buf.ctypes.data
    sens = binding.mt_sensor()
    gb = binding.mt_gbuffer(point=p, normal=p, albedo=p, material=p)
    lb = binding.mt_lightbuffer(power=p, in_shadow=p)
    light = binding.mt_light()

    def arg_error(rc, text):
        assert rc == MT_ERR_ARG and rc != MT_ERR_HIP, (name, rc, abi.last_error())
        assert text in abi.last_error(), (name, abi.last_error())

    ok = dict(lights=ctypes.addressof(light), n_lights=1, rgb=p)
    arg_error(_call(abi, name, None, sens, (8, 8), (0, 0, 8, 8), gb, lb, **ok), "scene is NULL")
    assert abi.last_error() == "scene is NULL"
    # the pointers first: lb, gb, the bitmap
    arg_error(_call(abi, name, None, sens, (0, 8), (0, 0, 8, 8), gb, None, **ok), "mt_lightbuffer is NULL")
    for half in (binding.mt_lightbuffer(power=p), binding.mt_lightbuffer(in_shadow=p)):
        arg_error(_call(abi, name, None, sens, (0, 8), (0, 0, 8, 8), gb, half, **ok), "both planes of the mt_lightbuffer")
    arg_error(_call(abi, name, None, sens, (0, 8), (0, 0, 8, 8), None, lb, **ok), "mt_gbuffer is NULL")
    for missing in binding.RELIGHT_GBUFFER_PLANES:
        planes = {n: p for n in binding.RELIGHT_GBUFFER_PLANES if n != missing}
        planes["depth"] = p  # (another plane does not help)
        arg_error(_call(abi, name, None, sens, (0, 8), (0, 0, 8, 8), binding.mt_gbuffer(**planes), lb, **ok),
                  "point, normal, albedo and material")
    arg_error(_call(abi, name, None, sens, (0, 8), (0, 0, 8, 8), gb, lb, lights=ctypes.addressof(light), n_lights=1, rgb=None),
              "output bitmap is NULL")
    # image size and chunk
    for image in ((0, 8), (8, 0), (100001, 8)):
        arg_error(_call(abi, name, None, sens, image, (0, 0, 1, 1), gb, lb, **ok), "image size %dx%d out of range" % image)
    for chunk in ((-1, 0, 4, 4), (0, 0, 0, 4), (5, 5, 4, 4), (0, 0, 9, 1)):
        arg_error(_call(abi, name, None, sens, (8, 8), chunk, gb, lb, **ok), "chunk %d,%d %dx%d outside image 8x8" % chunk)
    # the scene before the sensor and before the lights
    arg_error(_call(abi, name, None, None, (8, 8), (0, 0, 8, 8), gb, lb, lights=None, n_lights=-1, rgb=p), "scene is NULL")


def test_python_bindings_refuse_bad_planes():
    abi = M.hip_abi()
    with pytest.raises(ValueError, match="unknown light-buffer plane"):
        abi.render_lightbuffer(None, np.zeros(12), 8, 8, 1, channels=("power", "colour"))
    with pytest.raises(ValueError, match="unknown G-buffer plane"):
        abi.render_lightbuffer(None, np.zeros(12), 8, 8, 1, gbuffer_channels=("colour",))
    with pytest.raises(RuntimeError, match="no plane of the mt_lightbuffer"):
        abi.render_lightbuffer(None, np.zeros(12), 8, 8, 1, channels=())
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.render_lightbuffer(None, np.zeros(12), 8, 8, 1)
    gb = {n: np.zeros((8, 8) + ((k,) if k > 1 else ()), dtype=dt)
          for n, (dt, k) in binding.GBUFFER_PLANES.items() if n in binding.RELIGHT_GBUFFER_PLANES}
    lb = dict(power=np.zeros((1, 8, 8, 3)), in_shadow=np.zeros((1, 8, 8), dtype=np.uint8))
    light = [(0.0,) * 12]
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.shade_direct(None, np.zeros(12), 8, 8, gb, lb, light)
    with pytest.raises(ValueError, match="needs the G-buffer plane 'albedo'"):
        abi.shade_direct(None, np.zeros(12), 8, 8, {n: a for n, a in gb.items() if n != "albedo"}, lb, light)
    with pytest.raises(ValueError, match="needs the light-buffer plane 'in_shadow'"):
        abi.shade_direct(None, np.zeros(12), 8, 8, gb, dict(power=lb["power"]), light)
    with pytest.raises(ValueError, match="2 lights for a light buffer of 1"):
        abi.shade_direct(None, np.zeros(12), 8, 8, gb, lb, light * 2)
    with pytest.raises(ValueError, match="do not fit"):
        abi.shade_direct(None, np.zeros(12), 8, 8, gb, dict(lb, in_shadow=np.zeros((1, 8, 4), dtype=np.uint8)), light)


def test_facade_refuses_before_it_needs_a_device():
    cam = (50, 50, -120, 0, 0, 0, 60)
    m = M.MythTracer()
    m.set_devices([0, 0])
    with pytest.raises(RuntimeError, match="several devices"):
        m.lightbuffer(cam, 8, 8)
    m2 = M.MythTracer()
    with pytest.raises(RuntimeError, match="no plane"):
        m2.lightbuffer(cam, 8, 8, channels=())
    with pytest.raises(RuntimeError, match="empty chunk"):
        m2.lightbuffer(cam, 8, 8, chunk=(0, 0, 0, 8))
    m2.set_lights([(1.0,) * 12])
    gb = {n: np.zeros((8, 8) + ((k,) if k > 1 else ()), dtype=dt)
          for n, (dt, k) in binding.GBUFFER_PLANES.items() if n in binding.RELIGHT_GBUFFER_PLANES}
    lb = dict(power=np.zeros((2, 8, 8, 3)), in_shadow=np.zeros((2, 8, 8), dtype=np.uint8))
    with pytest.raises(RuntimeError, match="another number of lights"):
        m2.relight(cam, 8, 8, gb, lb)
