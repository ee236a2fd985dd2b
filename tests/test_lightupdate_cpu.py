"""The light-buffer update (include/mythtracer_hip.h, mt_update_lightbuffer[_device]), the parts that need no GPU.

a. The symbols exist and the ABI version is still 5.
b. Every argument check is reached without a device, in the documented order: lb, gb, chunk size, scene, the list, an
   index out of range, a duplicate.
c. The moves of tests/lightupdate_ref.py are worth testing, by the oracle alone: between the old and the new plane of
   the moved light in_shadow differs in at least 1 % of the lit pixels, 0 and 1 both occur in the new plane (both in the
   whole frame and inside the off-grid chunk that the GPU tests update), glass is crossed on f2_decal and room, and the
   planes of the unmoved lights are bit-identical.
d. The Python bindings refuse a missing plane, wrong shapes and wrong dtypes; the facade refuses before it needs a device.
"""
import ctypes

import numpy as np
import pytest

import gbuffer_ref
import lightbuffer_ref as lr
import lightupdate_ref as lu
import orclib

import mythtracer_amd as M
from mythtracer_amd import binding

MT_ERR_ARG, MT_ERR_HIP = -1, -2
W, H = 96, 54
NAMES = ("mt_update_lightbuffer", "mt_update_lightbuffer_device")


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    return native_libs


def test_symbols_and_abi_version():
    abi = M.hip_abi()
    assert binding.MT_ABI_VERSION == 5 == abi.lib.mt_abi_version()
    for name in NAMES:
        assert name in M.HIP_SYMBOLS and getattr(abi.lib, name) is not None
    assert binding.host_lib().mth_update_lightbuffer is not None
    assert binding.UPDATE_GBUFFER_PLANES == ("point", "material")


@pytest.mark.parametrize("name", NAMES)
def test_argument_checks_come_before_any_device_call(name):
    abi = M.hip_abi()
    fn = getattr(abi.lib, name)
    buf = np.zeros(64)
    p = buf.ctypes.data
    idx = (ctypes.c_int32 * 2)(0, 0)
    gb = binding.mt_gbuffer(point=p, material=p)
    power = binding.mt_lightbuffer(power=p)
    shadow = binding.mt_lightbuffer(in_shadow=p)

    def call(scene, cw, ch, g, li, n, lb):
        return fn(scene, cw, ch, ctypes.byref(g) if g is not None else None, li, n,
                  ctypes.byref(lb) if lb is not None else None, None)

    def arg_error(rc, text):
        assert rc == MT_ERR_ARG and rc != MT_ERR_HIP, (name, rc, abi.last_error())
        assert text in abi.last_error(), (name, abi.last_error())

    # everything right but the scene: the fourth check is reached, for either plane alone
    for lb in (power, shadow):
        arg_error(call(None, 8, 8, gb, idx, 1, lb), "scene is NULL")
        assert abi.last_error() == "scene is NULL"
    # 1. lb, before everything else (every later argument is wrong too: the earlier message wins)
    arg_error(call(None, 0, 8, None, None, 0, None), "mt_lightbuffer is NULL")
    arg_error(call(None, 0, 8, None, None, 0, binding.mt_lightbuffer()), "no plane of the mt_lightbuffer")
    # 2. gb
    arg_error(call(None, 0, 8, None, None, 0, power), "mt_gbuffer is NULL")
    for planes in (dict(point=p), dict(material=p), dict(depth=p, normal=p, albedo=p)):
        arg_error(call(None, 0, 8, binding.mt_gbuffer(**planes), None, 0, power), "point and material planes")
    # 3. the chunk, before the scene
    for cw, ch in ((0, 8), (8, 0), (-1, 8), (100001, 8), (8, 100001)):
        arg_error(call(None, cw, ch, gb, None, 0, power), "chunk size %dx%d out of range" % (cw, ch))
    # 4. the scene, before the list
    arg_error(call(None, 100000, 100000, gb, None, 0, power), "scene is NULL")
    arg_error(call(None, 1, 1, gb, idx, -1, shadow), "scene is NULL")
    # 5. the list: n_idx <= 0 or NULL is refused before the scene is looked into (a scene cannot be made without a
    # device, so the handle here is a stand-in that must not be read.  It is 4 MiB of zeros, far larger than an mt_scene:
    # should the order of the checks ever change, the library reads a scene of no lights inside this buffer and the
    # test fails on the message instead of reading outside it).  6. and 7. compare the list with the scene's light
    # count and so need a real scene: tests/test_gpu_lightupdate.py, test_list_checks_in_order, with the same calls.
    handle_buf = np.zeros(1 << 19)
    handle = ctypes.c_void_p(handle_buf.ctypes.data)
    for li, n in ((idx, 0), (idx, -3), (None, 2)):
        arg_error(call(handle, 8, 8, gb, li, n, power), "bad light index list")



# ---- c. the moves are worth testing (the oracle alone)

@pytest.fixture(scope="module")
def restated(scenes):
    """scene -> (G-buffer, planes under A, planes under B, moved index), made once and left unchanged."""
    made = {}

    def get(scene):
        if scene not in made:
            orc = orclib.OracleScene(scenes[scene])
            gb = gbuffer_ref.oracle_gbuffer(orc, lr.CAMERAS[scene], W, H)
            a, b, mv = lu.lights_before_and_after(scene)
            made[scene] = (gb, lr.ref_lightbuffer(orc, gb, a), lr.ref_lightbuffer(orc, gb, b), mv, orc)
        return made[scene]
    return get


@pytest.mark.parametrize("scene", list(lu.MOVES))
def test_the_moves_are_worth_testing(scene, restated, scenes):
    gb, old, new, mv, orc = restated(scene)
    a, b, _ = lu.lights_before_and_after(scene)
    assert len(a) == len(b) and all(x == y for i, (x, y) in enumerate(zip(a, b)) if i != mv)
    assert a[mv][:3] != b[mv][:3] and a[mv][3:] == b[mv][3:]
    if scene != "f2_decal":  # (see lightupdate_ref: the slab's own light stands outside its box too)
        box = M.MythTracer(scenes[scene]).root_aabb()
        assert all(box[k] < b[mv][k] < box[3 + k] for k in range(3)), (box, b[mv][:3])
    lit = (gb["prim"] >= 0) & (gb["material"] >= 0)
    assert np.array_equal(lit, lu.lit_of(gb))  # the planes the update reads say the same
    differ = int(((old["in_shadow"][mv] != new["in_shadow"][mv]) & lit).sum())
    print("%s: in_shadow of light %d differs in %d of %d lit pixels; new plane: %d lit, %d shadowed"
          % (scene, mv, differ, int(lit.sum()), int((new["in_shadow"][mv] == 0).sum()), int((new["in_shadow"][mv] == 1).sum())))
    assert differ >= 0.01 * lit.sum()
    assert (new["in_shadow"][mv] == 0).any() and (new["in_shadow"][mv] == 1).any()
    # the same inside the off-grid chunk of the GPU tests (same sensor: its planes are this window of the frame's)
    x, y, cw, ch = lu.OFF_GRID
    win = (slice(y, y + ch), slice(x, x + cw))
    differ_c, lit_c, new_c = int(((old["in_shadow"][mv] != new["in_shadow"][mv]) & lit)[win].sum()), lit[win], new["in_shadow"][mv][win]
    print("%s: in chunk %s in_shadow differs in %d of %d lit pixels; new plane: %d lit, %d shadowed"
          % (scene, lu.OFF_GRID, differ_c, int(lit_c.sum()), int((new_c == 0).sum()), int((new_c == 1).sum())))
    assert differ_c >= 0.01 * lit_c.sum()
    assert (new_c == 0).any() and (new_c == 1).any()
    if scene in lu.GLASS_SCENES:
        p = new["power"][mv][lit]
        assert ((p > 0) & (p < 1)).any()
    for l in range(len(a)):
        if l != mv:
            assert gbuffer_ref.same_bits(old["power"][l], new["power"][l], "%s light %d power" % (scene, l)) == 0
            assert np.array_equal(old["in_shadow"][l], new["in_shadow"][l])
    # the restatement from the STORED planes alone (what the kernel starts from) is the restatement from the trace
    again = lr.shadow_loops(lr.oracle_intersector(orc), gb["point"], lu.lit_of(gb), [b[mv]])
    assert gbuffer_ref.same_bits(again["power"][0], new["power"][mv], scene + " from stored planes") == 0
    assert np.array_equal(again["in_shadow"][0], new["in_shadow"][mv])


# ---- d. bindings and facade

def _planes(n_l=2, ch=8, cw=8):
    gb = dict(point=np.zeros((ch, cw, 3)), material=np.zeros((ch, cw), dtype=np.int32))
    lb = dict(power=np.zeros((n_l, ch, cw, 3)), in_shadow=np.zeros((n_l, ch, cw), dtype=np.uint8))
    return gb, lb


@pytest.mark.parametrize("which", ["abi", "facade"])
def test_python_bindings_refuse_bad_planes(which):
    abi = M.hip_abi()
    m = M.MythTracer()
    call = (lambda g, l, i: abi.update_lightbuffer(None, g, l, i)) if which == "abi" else m.update_lightbuffer
    gb, lb = _planes()
    for missing in ("point", "material"):
        with pytest.raises(ValueError, match="needs the G-buffer plane %r" % missing):
            call({n: a for n, a in gb.items() if n != missing}, lb, [0])
    with pytest.raises(ValueError, match="needs a light-buffer plane"):
        call(gb, {}, [0])
    with pytest.raises(ValueError, match="'material' has dtype int64"):
        call(dict(gb, material=np.zeros((8, 8), dtype=np.int64)), lb, [0])
    with pytest.raises(ValueError, match="'point' has dtype float32"):
        call(dict(gb, point=np.zeros((8, 8, 3), dtype=np.float32)), lb, [0])
    with pytest.raises(ValueError, match="'point' has shape"):
        call(dict(gb, point=np.zeros((8, 4, 3))), lb, [0])
    with pytest.raises(ValueError, match="'material' has shape"):
        call(dict(gb, material=np.zeros(64, dtype=np.int32)), lb, [0])
    with pytest.raises(ValueError, match="'power' must be a writeable C-contiguous numpy array of dtype float64"):
        call(gb, dict(lb, power=np.zeros((2, 8, 8, 3), dtype=np.float32)), [0])
    with pytest.raises(ValueError, match="'in_shadow' must be"):
        call(gb, dict(lb, in_shadow=np.zeros((2, 8, 8), dtype=np.int8)), [0])
    with pytest.raises(ValueError, match="'in_shadow' of shape .* does not fit"):
        call(gb, dict(lb, in_shadow=np.zeros((2, 8, 4), dtype=np.uint8)), [0])
    with pytest.raises(ValueError, match="'in_shadow' of shape .* does not fit"):
        call(gb, dict(lb, in_shadow=np.zeros((3, 8, 8), dtype=np.uint8)), [0])  # another light count than power's
    if which == "abi":
        with pytest.raises(ValueError, match="'power' must be"):
            call(gb, dict(lb, power=np.zeros((2, 8, 8, 6))[..., ::2]), [0])  # not contiguous: cannot be updated in place
        with pytest.raises(RuntimeError, match="scene is NULL"):
            call(gb, lb, [0])
        with pytest.raises(ValueError, match="unknown light-buffer plane"):
            abi.update_lightbuffer_device(None, 8, 8, dict(point=1, material=1), dict(colour=1), [0])
        with pytest.raises(ValueError, match="unknown G-buffer plane"):
            abi.update_lightbuffer_device(None, 8, 8, dict(colour=1), dict(power=1), [0])
        with pytest.raises(RuntimeError, match="scene is NULL"):
            abi.update_lightbuffer_device(None, 8, 8, dict(point=1, material=1), dict(power=1), [0])


def test_facade_refuses_before_it_needs_a_device():
    gb, lb = _planes()
    m = M.MythTracer()
    m.set_lights([(1.0,) * 12] * 2)
    m.set_devices([0, 0])
    with pytest.raises(RuntimeError, match="several devices"):
        m.update_lightbuffer(gb, lb, [0])
    m2 = M.MythTracer()
    m2.set_lights([(1.0,) * 12])
    with pytest.raises(RuntimeError, match="another number of lights"):
        m2.update_lightbuffer(gb, lb, [0])
    m2.set_lights([(1.0,) * 12] * 2)
    with pytest.raises(RuntimeError, match="no light is listed"):
        m2.update_lightbuffer(gb, lb, [])
    assert np.array_equal(lb["power"], np.zeros((2, 8, 8, 3)))  # (the arguments are never written)
