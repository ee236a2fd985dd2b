"""The primary-hit G-buffer, the parts that need no GPU (include/mythtracer_hip.h, mt_render_gbuffer).

1. The DEFINITION the GPU test leans on.  tests/golden/gbuffer_<scene>_96x54.npz were written by the compiled
   reference (tests/golden/make_gbuffer_golden.py: its sensor's ray of every pixel, then its IntersectRay / GetNormal /
   GetUVW over those rays).  The CPU oracle reproduces them bit for bit -- orclib.sensor + sensor_ray + Scene.intersect
   for every pixel, compared as uint64 views, NaN = NaN on the misses.  That pins depth, point, normal, uvw and line_no
   to the reference, and with them the oracle's three other planes, which the reference's driver cannot give and which
   tests/gbuffer_ref.py derives like this:
     prim      the oracle's `tri` IS the AddPrimitive index (its triangles are stored in AddPrimitive order);
     material  OracleScene.triangles()'s material index of that triangle, -1 = none;
     albedo    ambient * tex_color_at(u, v) elementwise in fp64 where the material has a texture, else ambient
               (mythtracer.cc:58-64); NaN without a material.
2. The argument checks of the two entry points, which come before any device call: `out`, image size and chunk, scene.
"""
import ctypes

import numpy as np
import pytest

import gbuffer_ref
import orclib

import mythtracer_amd as M
from mythtracer_amd import binding

MT_ERR_ARG, MT_ERR_HIP = -1, -2
NAMES = ("mt_render_gbuffer", "mt_render_gbuffer_device")


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    return native_libs


@pytest.mark.parametrize("scene", ["cornell", "mini", "room"])
def test_oracle_reproduces_the_reference_made_goldens(scene, scenes):
    g = gbuffer_ref.load_golden(scene)
    W, H = (int(v) for v in g["image"])
    cam = tuple(float(v) for v in g["cam"])
    orc = orclib.OracleScene(scenes[scene])
    o = gbuffer_ref.oracle_gbuffer(orc, cam, W, H)
    # the rays first: the oracle's sensor is the reference's
    assert gbuffer_ref.same_bits(o["rays"][..., 3:], g["dirs"], scene + " ray directions") == 0
    assert np.array_equal(o["line_no"], g["line"])
    miss = g["line"] < 0
    print(scene, int(miss.sum()), "misses of", miss.size)
    if scene == "cornell":
        assert miss.any() and (~miss).any()  # the background is in view
    for plane, key in (("depth", "t"), ("point", "point"), ("normal", "normal"), ("uvw", "uvw")):
        assert np.isnan(g[key][miss]).all() and np.isnan(o[plane][miss]).all()
        assert gbuffer_ref.same_bits(o[plane], g[key], "%s %s" % (scene, plane)) == 0
    # the derived planes are well-formed: prim / material -1 exactly on the misses (these scenes have materials)
    assert np.array_equal(o["prim"] < 0, miss) and np.array_equal(o["material"] < 0, miss)
    assert np.array_equal(np.isnan(o["albedo"]).any(axis=-1), miss)
    data, _, line = orc.triangles()
    assert np.array_equal(line[o["prim"][~miss]], g["line"][~miss])  # `tri` indexes the AddPrimitive order
    assert len(data) == orc.num_triangles


def test_axis_aligned_cameras_have_a_zero_component_column():
    """Two of the three golden cameras have yaw 0: a pixel column whose rays have x = 0 exactly (1 / 0 = inf and
    0 * inf = NaN in Node::NodeIntersectRay)."""
    for scene, expect in (("cornell", True), ("mini", False), ("room", True)):
        g = gbuffer_ref.load_golden(scene)
        assert bool((g["dirs"] == 0.0).any()) == expect, scene


def _sensor():
    return binding.mt_sensor()


def _gb(**planes):
    return binding.mt_gbuffer(**planes)


def _call(abi, name, scene, sens, image, chunk, out):
    fn = getattr(abi.lib, name)
    return fn(scene, ctypes.byref(sens) if sens is not None else None, image[0], image[1], *chunk,
              ctypes.byref(out) if out is not None else None, None)


def test_symbols_and_abi_version():
    abi = M.hip_abi()
    assert binding.MT_ABI_VERSION == 5 == abi.lib.mt_abi_version()
    for name in NAMES:
        assert name in M.HIP_SYMBOLS and getattr(abi.lib, name) is not None


@pytest.mark.parametrize("name", NAMES)
def test_argument_checks_come_before_any_device_call(name):
    abi = M.hip_abi()
    buf = np.zeros(64)
    one = _gb(depth=buf.ctypes.data)
    sens = _sensor()

    def arg_error(rc, text):
        assert rc == MT_ERR_ARG and rc != MT_ERR_HIP, (name, rc, abi.last_error())
        assert text in abi.last_error(), (name, abi.last_error())

    # a NULL scene with everything else in order
    arg_error(_call(abi, name, None, sens, (8, 8), (0, 0, 8, 8), one), "scene is NULL")
    assert abi.last_error() == "scene is NULL"
    # no mt_gbuffer, or one without a plane
    arg_error(_call(abi, name, None, sens, (8, 8), (0, 0, 8, 8), None), "mt_gbuffer is NULL")
    arg_error(_call(abi, name, None, sens, (8, 8), (0, 0, 8, 8), _gb()), "no plane")
    # image size: mt_render_chunk's limits and message
    for image in ((0, 8), (8, 0), (-1, 8), (100001, 8), (8, 100001)):
        arg_error(_call(abi, name, None, sens, image, (0, 0, 1, 1), one), "image size %dx%d out of range" % image)
    # chunks outside the image or empty: mt_render_chunk's message
    for chunk in ((-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (5, 5, 4, 4), (0, 0, 9, 1), (0, 0, 1, 9),
                  (8, 0, 1, 1), (0, 0, 2147483647, 1)):
        arg_error(_call(abi, name, None, sens, (8, 8), chunk, one), "chunk %d,%d %dx%d outside image 8x8" % chunk)
    # every single plane is enough to pass the `out` check
    for plane in binding.GBUFFER_PLANES:
        arg_error(_call(abi, name, None, sens, (8, 8), (0, 0, 8, 8), _gb(**{plane: buf.ctypes.data})), "scene is NULL")


def test_python_bindings_refuse_unknown_planes():
    abi = M.hip_abi()
    with pytest.raises(ValueError, match="unknown G-buffer plane"):
        abi.render_gbuffer(None, np.zeros(12), 8, 8, channels=("depth", "colour"))
    with pytest.raises(RuntimeError, match="no plane"):
        abi.render_gbuffer(None, np.zeros(12), 8, 8, channels=())
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.render_gbuffer(None, np.zeros(12), 8, 8)
    assert list(binding.GBUFFER_PLANES) == ["depth", "point", "normal", "uvw", "albedo", "prim", "line_no", "material"]
    assert ctypes.sizeof(binding.mt_gbuffer) == 8 * ctypes.sizeof(ctypes.c_void_p)


def test_facade_refuses_several_devices_before_it_needs_one():
    m = M.MythTracer()
    m.set_devices([0, 0])
    with pytest.raises(RuntimeError) as e:
        m.gbuffer((50, 50, -120, 0, 0, 0, 60), 8, 8)
    assert "several devices" in str(e.value), str(e.value)
    m2 = M.MythTracer()
    with pytest.raises(RuntimeError) as e:
        m2.gbuffer((50, 50, -120, 0, 0, 0, 60), 8, 8, channels=())
    assert "no plane" in str(e.value), str(e.value)
    m2.set_supersampling(7)  # ignored by the G-buffer: the next message is not about the factor
    with pytest.raises(RuntimeError) as e:
        m2.gbuffer((50, 50, -120, 0, 0, 0, 60), 8, 8, chunk=(0, 0, 0, 8))
    assert "empty chunk" in str(e.value), str(e.value)
