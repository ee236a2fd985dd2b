"""The ray-tree update, the parts that need no GPU (include/mythtracer_hip.h, mt_raytree_update_lights).

a. The symbols exist, the ABI version is still 5, the argument checks that can be reached without a device come before
   any device call in the documented order, and the facade refuses bad input before it needs one.  (The checks that
   read a tree need a real tree: tests/test_gpu_raytree_update.py.)
b. The moves of tests/raytree_update_ref.py are worth testing AT DEPTH, by the oracle alone (tests/raytree_ref.py): at
   96x54 and depth 5, whole frame and off-grid chunk, between the tree under lights A and the tree under lights B (one
   light moved) nothing but the moved light's planes differs in any layer; those planes under B are
   lightbuffer_ref.shadow_loops from the STORED point and lit mask alone -- what the update computes --; on mini, room
   and two_way the moved light's in_shadow changes in at least 1 % of the lit rays of the layers >= 1 taken together,
   with 0 and 1 both present there; and the two shaded frames differ.
   cornell (its chunk has one layer, its frame a second one of 33 rays none of which changes) and f2_decal (one layer)
   cover layer 0 and the few-rays case only: nothing is asserted about a change at depth there.
"""
import ctypes

import numpy as np
import pytest

import lightbuffer_ref as lr
import orclib
import raytree_ref as rr
import raytree_update_ref as ru

import mythtracer_amd as M
from mythtracer_amd import binding

MT_ERR_ARG, MT_ERR_HIP = -1, -2
W, H = ru.W, ru.H
SYMBOLS = ("mt_raytree_update_lights", "mt_raytree_update_lights_device")


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    return native_libs


# ---- a. symbols, argument checks, facade

def test_symbols_and_abi_version():
    abi = M.hip_abi()
    assert binding.MT_ABI_VERSION == 5 == abi.lib.mt_abi_version()
    for name in SYMBOLS:
        assert name in M.HIP_SYMBOLS and getattr(abi.lib, name) is not None
    assert getattr(M.host_lib(), "mth_raytree_update") is not None
    assert callable(abi.raytree_update_lights) and callable(abi.raytree_update_lights_device)
    assert callable(binding.RayTree.update)


def test_argument_checks_come_before_any_device_call():
    abi = M.hip_abi()
    idx = np.array([0, 1], dtype=np.int32)
    for name in SYMBOLS:
        fn = getattr(abi.lib, name)
        for args in ((idx.ctypes.data, 2), (idx.ctypes.data, 0), (idx.ctypes.data, -1), (None, 2), (None, 0)):
            rc = fn(None, args[0], args[1], None)  # a NULL tree: its message wins over a bad list's
            assert rc == MT_ERR_ARG and rc != MT_ERR_HIP, (name, rc, abi.last_error())
            assert abi.last_error() == "the ray tree is NULL", (name, args, abi.last_error())
    with pytest.raises(RuntimeError, match="ray tree is NULL"):
        abi.raytree_update_lights(None, [0])
    with pytest.raises(RuntimeError, match="ray tree is NULL"):
        abi.raytree_update_lights(None, [])
    with pytest.raises(RuntimeError, match="ray tree is NULL"):
        abi.raytree_update_lights_device(None, [0])


def test_facade_refuses_before_it_needs_a_device():
    idx = np.array([0], dtype=np.int32)
    m = M.MythTracer()
    m.set_devices([0, 0])
    assert not m.L.mth_raytree_update(m.h, None, idx.ctypes.data, 1, None, None)
    assert "several devices" in m.last_error()
    m2 = M.MythTracer()
    assert not m2.L.mth_raytree_update(m2.h, None, idx.ctypes.data, 0, None, None)
    assert "no light is listed" in m2.last_error()
    assert not m2.L.mth_raytree_update(m2.h, None, None, 1, None, None)
    assert "no light is listed" in m2.last_error()
    assert not m2.L.mth_raytree_update(m2.h, None, idx.ctypes.data, 1, None, None)
    assert "RayTree is NULL" in m2.last_error()
    closed = binding.RayTree(m2, None, {}, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="closed"):
        closed.update([0])


# ---- b. the moves are worth testing at depth

def changed_at_depth(a, b, moved):
    """(differing, lit) over the layers >= 1 for the moved light's in_shadow, and the values that occur there under B."""
    differing = lit = 0
    values = set()
    for la, lb in zip(a["layers"][1:], b["layers"][1:]):
        mask = ru.lit_of(lb)
        differing += int((la["in_shadow"][moved][mask] != lb["in_shadow"][moved][mask]).sum())
        lit += int(mask.sum())
        values |= set(np.unique(lb["in_shadow"][moved][mask]).tolist())
    return differing, lit, values


@pytest.mark.parametrize("scene", ru.SCENES)
def test_the_moves_change_the_moved_lights_planes_and_nothing_else(scene, scenes):
    orc = orclib.OracleScene(ru.obj_of(scenes, scene))
    cam = rr.CAMERAS[scene]
    A, B, moved = ru.lights_before_and_after(scene)
    shadow = lr.oracle_intersector(orc)
    for chunk in ru.CHUNKS:
        cw, ch = chunk[2:] if chunk else (W, H)
        a = rr.build(orc, cam, W, H, A, 5, chunk=chunk)
        b = rr.build(orc, cam, W, H, B, 5, chunk=chunk)
        what = "%s %s" % (scene, "chunk" if chunk else "frame")
        print(what, "layers under A", a["n_rays"], "under B", b["n_rays"])
        assert a["n_rays"] == b["n_rays"]
        for k, (la, lb) in enumerate(zip(a["layers"], b["layers"])):
            for name in ru.UNCHANGED_PLANES + (("pixel",) if k == 0 else ()):
                assert ru.same_plane(la[name], lb[name]), (what, k, name)
            for l in range(len(A)):
                if l != moved:
                    assert ru.same_plane(la["power"][l], lb["power"][l]), (what, k, l)
                    assert np.array_equal(la["in_shadow"][l], lb["in_shadow"][l]), (what, k, l)
            # the moved light's planes under B from the STORED point and lit mask alone
            n = len(la["ray"])
            sl = lr.shadow_loops(shadow, la["point"].reshape(1, n, 3), ru.lit_of(la).reshape(1, n), [B[moved]])
            assert ru.same_plane(sl["power"].reshape(n, 3), lb["power"][moved]), (what, k)
            assert np.array_equal(sl["in_shadow"].reshape(n), lb["in_shadow"][moved]), (what, k)
            assert np.array_equal(sl["iterations"].reshape(n), lb["iterations"][moved]), (what, k)
            n0 = int((la["in_shadow"][moved] != lb["in_shadow"][moved]).sum())
            print("  layer %d: %d rays, %d lit, moved light's in_shadow differs at %d" % (k, n, int(ru.lit_of(la).sum()), n0))
        differing, lit, values = changed_at_depth(a, b, moved)
        print("%s: layers >= 1: %d / %d lit rays differ, values %s" % (what, differing, lit, sorted(values)))
        if scene in ru.DEEP_SCENES:
            assert lit > 0 and differing * 100 >= lit, (what, differing, lit)
            assert {0, 1} <= values, (what, values)
        # (cornell and f2_decal: layer 0 and the few-rays case only; nothing asserted at depth)
        fa = rr.shade(orc, a, A, cw, ch)
        fb = rr.shade(orc, b, B, cw, ch)
        n = int((fa != fb).any(axis=-1).sum())
        print("%s: %d of %d pixels of the shaded frames differ" % (what, n, cw * ch))
        assert n > 0
