"""Material edits in place, the parts that need no GPU (include/mythtracer_hip.h, mt_scene_set_materials and
mt_raytree_update_materials).

a. The symbols exist, the ABI version is still 5, the argument checks that can be reached without a device come before
   any device call in the documented order, and the facade refuses bad input before it needs one.
b. What each edit of tests/material_edit_ref.py changes in a stored tree, by the oracle alone (tests/raytree_ref.py) on
   two_way.obj at 96x54, the bench's lights, depth 5: between the tree of the scene as it is (A) and the tree of a scene
   BUILT with the edited .mtl (B), exactly the planes of TABLE differ, in exactly that many entries per layer (every
   double counted: an albedo is three, a light's power three per light); a shape-breaking edit gives B's ray counts, and
   the restated check pass (material_edit_ref.check_pass) finds its first mismatch at the first ray, in the first
   layer, whose children differ between A and B.  The same edits in
   the off-grid chunk of the sibling tests, with the counts this file records.
c. The restated tree under B shades to OracleScene.render under B with zero differing bytes, at depths 0, 1, 2 and 5.
"""
import ctypes

import numpy as np
import pytest

import material_edit_ref as me
import orclib
import raytree_ref as rr

import mythtracer_amd as M
from mythtracer_amd import binding

MT_ERR_ARG, MT_ERR_HIP = -1, -2
W, H = me.W, me.H
CAM = rr.CAMERAS["two_way"]
SYMBOLS = ("mt_scene_set_materials", "mt_scene_get_materials", "mt_raytree_update_materials")

# edit -> {plane: entries that differ per layer 0 .. 5}, whole frame
TABLE = {
    "colour": {"albedo": [75, 660, 405, 27, 3, 0]},
    "mirror 0.5": {"coef": [0, 100, 231, 87, 6, 2]},
    "pane refl": {"coef": [0, 631, 314, 62, 6, 2]},
    "floor 0.2": {"coef": [0, 109, 134, 68, 0, 0]},
    "pane Tr": {"power": [384, 111, 42, 39, 0, 0]},
    "pane Tf": {"power": [256, 74, 28, 26, 0, 0]},
    "composite": {"albedo": [75, 660, 405, 27, 3, 0], "coef": [0, 100, 231, 87, 6, 2], "power": [384, 111, 42, 39, 0, 0]},
}
# edit -> B's rays per layer, whole frame
SHAPES = {
    "mirror 0.125": [5184, 4353, 1561, 229, 3],
    "blue refl": [5184, 4378, 1618, 407, 60, 12],
    "pane opaque": [5184, 3722, 1326, 229, 3, 2],
}
# the off-grid chunk, as this test found them (rays per layer of A: OFF_GRID_A)
OFF_GRID_A = [2257, 2210, 952, 120, 6, 2]
OFF_GRID_TABLE = {
    "colour": {"albedo": [12, 321, 174, 0, 3, 0]},
    "mirror 0.5": {"coef": [0, 44, 31, 61, 6, 2]},
    "pane refl": {"coef": [0, 346, 202, 31, 6, 2]},
    "floor 0.2": {},  # (no ray of the chunk's tree has the floor above it: nothing differs, and the update must say so)
    "pane Tr": {"power": [114, 0, 0, 0, 0, 0]},
    "pane Tf": {"power": [76, 0, 0, 0, 0, 0]},
    "composite": {"albedo": [12, 321, 174, 0, 3, 0], "coef": [0, 44, 31, 61, 6, 2], "power": [114, 0, 0, 0, 0, 0]},
}
OFF_GRID_SHAPES = {
    "mirror 0.125": [2257, 2210, 952, 120, 3],
    "blue refl": [2257, 2214, 998, 205, 11, 12],
    "pane opaque": [2257, 1864, 750, 120, 3, 2],
}


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    return native_libs


# ---- a. symbols, argument checks, facade

def test_symbols_and_abi_version():
    abi = M.hip_abi()
    assert binding.MT_ABI_VERSION == 5 == abi.lib.mt_abi_version()
    for name in SYMBOLS:
        assert name in M.HIP_SYMBOLS and getattr(abi.lib, name) is not None
    for name in ("mth_update_materials", "mth_raytree_update_materials"):
        assert getattr(M.host_lib(), name) is not None
    assert callable(abi.set_materials) and callable(abi.get_materials) and callable(abi.raytree_update_materials)
    assert callable(binding.MythTracer.update_materials) and callable(binding.RayTree.update_materials)


def test_argument_checks_come_before_any_device_call():
    abi = M.hip_abi()
    table = (binding.mt_material * 2)()
    for fn in (abi.lib.mt_scene_set_materials, abi.lib.mt_scene_get_materials):
        for args in ((table, 2), (table, 0), (None, 2), (None, 0), (table, -1)):
            rc = fn(None, args[0], args[1])  # a NULL scene: its message wins over everything about the array
            assert rc == MT_ERR_ARG and rc != MT_ERR_HIP, (rc, abi.last_error())
            assert abi.last_error() == "scene is NULL", abi.last_error()
    st = binding.mt_stats()
    for stats in (None, ctypes.addressof(st)):
        assert abi.lib.mt_raytree_update_materials(None, stats) == MT_ERR_ARG
        assert abi.last_error() == "the ray tree is NULL"
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.set_materials(None, [])
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.get_materials(None, 3)
    with pytest.raises(RuntimeError, match="ray tree is NULL"):
        abi.raytree_update_materials(None)


def test_facade_refuses_before_it_needs_a_device():
    m = M.MythTracer()
    m.set_devices([0, 0])
    assert not m.L.mth_raytree_update_materials(m.h, None, None, None)
    assert "several devices" in m.last_error()
    m2 = M.MythTracer(rr.TWO_WAY)
    assert not m2.L.mth_raytree_update_materials(m2.h, None, None, None)
    assert "RayTree is NULL" in m2.last_error()
    closed = binding.RayTree(m2, None, {}, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="closed"):
        closed.update_materials()
    with pytest.raises(RuntimeError, match="no material named nothing"):
        m2.update_materials({"nothing": {"ka": (0.5, 0.5, 0.5)}})
    with pytest.raises(RuntimeError, match="no material field"):
        m2.update_materials({"pane": {"colour": 1.0}})
    v = np.zeros(16)
    assert not m2.L.mth_update_materials(m2.h, b"nothing", v.ctypes.data)
    assert "no material named nothing" in m2.last_error()
    # (the refused edits left the facade's materials alone)
    assert m2.get_material("pane")[0][11] == 0.6


# ---- b. what the edits change in a stored tree

@pytest.fixture(scope="module")
def base():
    orc = orclib.OracleScene(rr.TWO_WAY)
    return orc, {chunk: rr.build(orc, CAM, W, H, me.LIGHTS, 5, chunk=chunk) for chunk in me.CHUNKS}


@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            d = tmp_path_factory.mktemp("variant")
            made[name] = orclib.OracleScene(me.variant(rr.TWO_WAY, me.EDITS[name], str(d)))
        return made[name]
    return get


def test_the_variants_hold_the_edits_numbers_and_nothing_else(base, variants):
    orc, trees = base
    assert trees[None]["n_rays"] == me.TREE_A
    print("off-grid chunk: A has", trees[me.OFF_GRID]["n_rays"])
    assert trees[me.OFF_GRID]["n_rays"] == OFF_GRID_A
    for name, edit in me.EDITS.items():
        me.check_variant(orc.materials(), variants(name).materials(), edit)


@pytest.mark.parametrize("chunk", me.CHUNKS, ids=["frame", "chunk"])
@pytest.mark.parametrize("name", list(me.SAME_SHAPE))
def test_a_same_shape_edit_changes_exactly_its_planes(name, chunk, base, variants):
    _, trees = base
    a = trees[chunk]
    orc_b = variants(name)
    b = rr.build(orc_b, CAM, W, H, me.LIGHTS, 5, chunk=chunk)
    assert me.same_shape(a, b)
    got = me.diff_table(a, b)
    print("%s %s: %s" % (name, "chunk" if chunk else "frame", got))
    assert got == (OFF_GRID_TABLE if chunk else TABLE)[name]
    # the restated check pass agrees: no mismatch, and the coefficients it carries down are B's, bit for bit
    cp = me.check_pass(a, orc_b.materials())
    assert cp["count"] == 0 and cp["first"] is None
    for c, lay in zip(cp["coef"], b["layers"]):
        assert np.array_equal(c.view(np.uint64), lay["coef"].view(np.uint64))
    # in_shadow follows power where a pane's transparency decides (counted with it; never alone)
    assert "in_shadow" not in got or "power" in got


@pytest.mark.parametrize("chunk", me.CHUNKS, ids=["frame", "chunk"])
@pytest.mark.parametrize("name", list(me.SHAPE_BREAKING))
def test_a_shape_breaking_edit_and_its_first_mismatch(name, chunk, base, variants):
    _, trees = base
    a = trees[chunk]
    orc_b = variants(name)
    b = rr.build(orc_b, CAM, W, H, me.LIGHTS, 5, chunk=chunk)
    cp = me.check_pass(a, orc_b.materials())
    print("%s %s: B has %s, %d mismatches, the first at %s" % (name, "chunk" if chunk else "frame", b["n_rays"], cp["count"], cp["first"]))
    want = (OFF_GRID_SHAPES if chunk else SHAPES)[name]
    assert b["n_rays"] == want
    if not me.same_shape(a, b):
        assert cp["count"] > 0
        # the first mismatch is in the first layer whose children differ
        k = next(i for i, (x, y) in enumerate(zip(a["layers"], b["layers"]))
                 if not (np.array_equal(x["child_refl"], y["child_refl"]) and np.array_equal(x["child_refr"], y["child_refr"])))
        assert cp["first"][0] == k
        x, y = a["layers"][k], b["layers"][k]
        differs = ((x["child_refl"] >= 0) != (y["child_refl"] >= 0)) | ((x["child_refr"] >= 0) != (y["child_refr"] >= 0))
        assert cp["first"][1] == int(np.nonzero(differs)[0][0])
    else:
        assert cp["count"] == 0
    if chunk is None and name == "mirror 0.125":
        # the case only a PROPAGATED coefficient finds: a child of layer 3 or 4 that B no longer spawns
        assert cp["first"][0] in (3, 4)
        k, i = cp["first"]
        assert a["layers"][k]["child_refl"][i] >= 0 and a["layers"][k]["coef"][i] > 0.01 >= cp["coef"][k][i]
        # at depth 2 the changed layer does not exist: the shape survives
        assert me.check_pass(rr.truncated(a, 2), orc_b.materials())["count"] == 0
    if chunk is None and name == "blue refl":
        k, i = cp["first"]
        assert a["layers"][k]["child_refl"][i] < 0  # a child the tree does not have
    if chunk is None and name == "pane opaque":
        k, i = cp["first"]
        assert a["layers"][k]["child_refr"][i] >= 0  # a child the tree has is no longer spawned


# ---- c. the restated tree under B is the oracle's frame under B

@pytest.mark.parametrize("name", ["colour", "mirror 0.5", "pane Tr", "composite"])
def test_the_restated_tree_under_b_shades_to_the_oracles_frame(name, variants):
    orc_b = variants(name)
    orc_b.set_lights(me.LIGHTS)
    b5 = rr.build(orc_b, CAM, W, H, me.LIGHTS, 5)
    for d in (0, 1, 2, 5):
        rgb = rr.shade(orc_b, rr.truncated(b5, d), me.LIGHTS, W, H)
        want = orc_b.render(CAM, W, H, max_level=d)["rgb"]
        n = int((rgb != want).sum())
        print("%s d=%d: %d bytes differ" % (name, d, n))
        assert n == 0


# ---- d. the pane no ray hits

def test_the_hidden_pane_is_crossed_by_shadow_rays_only():
    """material_edit_ref.hidden_pane_scene: no ray of the tree hits the pane, and its transparency changes the light
    plane of the rays in its shadow -- 224 of the 256, three doubles each -- and nothing else."""
    w, h = me.HIDDEN_SIZE
    trees = []
    for tr in (0.6, 0.5):
        orc = orclib.OracleScene()
        floor, pane = me.hidden_pane_scene(orc, tr)
        orc.finalize()
        t = rr.build(orc, me.HIDDEN_CAMERA, w, h, me.HIDDEN_LIGHTS, 5)
        assert t["n_rays"] == [w * h] and (t["layers"][0]["material"] == floor).all()
        trees.append(t)
    got = me.diff_table(*trees)
    print("hidden pane:", got)
    assert got == {"power": [672]}
