"""Triangles given another material in place, the parts that need no GPU (include/mythtracer_hip.h,
mt_scene_set_triangle_materials, mt_scene_set_raytree_tri and the reassignment the two ray-tree material calls take).

a. The symbols exist, the ABI version is still 5, the argument checks that can be reached without a device return
   MT_ERR_ARG and never MT_ERR_HIP, and the facade refuses bad input before it needs a device.
b. The facade's flatten() after assign_material is the flat description with exactly those entries replaced.
c. The reassignments of tests/assign_ref.py, by the oracle alone (tests/raytree_ref.py) on two_way.obj at 96 x 54, the
   bench's lights, depth 5: the tree of a scene BUILT with each assignment -- a variant .obj whose usemtl lines were
   rewritten, and the same triangles added one by one -- has the rays per layer assign_ref.ROWS records, and what each
   row is there to exercise holds.  The cases with no .obj spelling ("no material", one triangle of a quad, the textured
   target on room_tex) are built the same way; their counts are printed and held.
d. The shadow-visible rule restated (assign_ref.shadow_visible) says what ROWS says, and where it says "not visible" no
   light plane of a layer that kept its size moves.
"""
import ctypes

import numpy as np
import pytest

import assign_ref as ar
import lightbuffer_ref as lr
import material_edit_ref as me
import orclib
import raytree_ref as rr

import mythtracer_amd as M
from mythtracer_amd import binding, scenegen

MT_ERR_ARG, MT_ERR_HIP = -1, -2
W, H = ar.W, ar.H
CAM = ar.CAM
SYMBOLS = ("mt_scene_set_triangle_materials", "mt_scene_get_triangle_materials", "mt_scene_set_raytree_tri",
           "mt_raytree_read_tri", "mt_raytree_keeps_tri")


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    return native_libs


# ---- a. symbols, argument checks, facade

def test_symbols_and_abi_version():
    abi = M.hip_abi()
    assert binding.MT_ABI_VERSION == 5 == abi.lib.mt_abi_version()
    for name in SYMBOLS:
        assert name in M.HIP_SYMBOLS and getattr(abi.lib, name) is not None
    for name in ("mth_assign_material", "mth_update_triangle_materials", "mth_set_raytree_keep_triangles"):
        assert getattr(M.host_lib(), name) is not None
    for name in ("set_triangle_materials", "get_triangle_materials", "set_raytree_tri", "raytree_keeps_tri", "raytree_read_tri"):
        assert callable(getattr(abi, name))
    for name in ("assign_material", "update_triangle_materials", "set_raytree_keep_triangles"):
        assert callable(getattr(binding.MythTracer, name))


def test_argument_checks_come_before_any_device_call():
    abi = M.hip_abi()
    arr = np.zeros(4, dtype=np.int32)
    for fn in (abi.lib.mt_scene_set_triangle_materials, abi.lib.mt_scene_get_triangle_materials):
        for p, n in ((arr.ctypes.data, 4), (arr.ctypes.data, 0), (None, 4), (None, 0), (arr.ctypes.data, -1)):
            rc = fn(None, p, n)  # a NULL scene: its message wins over everything about the array
            assert rc == MT_ERR_ARG and rc != MT_ERR_HIP, (rc, abi.last_error())
            assert abi.last_error() == "scene is NULL", abi.last_error()
    for keep in (0, 1, 2, -1):
        assert abi.lib.mt_scene_set_raytree_tri(None, keep) == MT_ERR_ARG
        assert abi.last_error() == "scene is NULL"
    assert abi.lib.mt_raytree_keeps_tri(None) == MT_ERR_ARG
    assert abi.last_error() == "the ray tree is NULL"
    for layer in (0, -1, 99):
        for out in (arr.ctypes.data, None):
            assert abi.lib.mt_raytree_read_tri(None, layer, out) == MT_ERR_ARG
            assert abi.last_error() == "the ray tree is NULL"
    st = binding.mt_stats()
    info = binding.mt_raytree_regrow_info()
    assert abi.lib.mt_raytree_update_materials(None, ctypes.addressof(st)) == MT_ERR_ARG
    assert abi.lib.mt_raytree_regrow_materials(None, ctypes.addressof(info), ctypes.addressof(st)) == MT_ERR_ARG
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.set_triangle_materials(None, [0, 1])
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.get_triangle_materials(None, 3)
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.set_raytree_tri(None, True)
    with pytest.raises(RuntimeError, match="ray tree is NULL"):
        abi.raytree_keeps_tri(None)


def test_facade_refuses_before_it_needs_a_device():
    m = M.MythTracer(rr.TWO_WAY)
    n = len(m.flatten()["tri_id"])
    with pytest.raises(RuntimeError, match="no material named nothing"):
        m.assign_material([0], "nothing")
    with pytest.raises(RuntimeError, match="triangle index %d outside the scene's %d triangles" % (n, n)):
        m.assign_material([0, n], "mirror")
    with pytest.raises(RuntimeError, match="triangle index -1 outside"):
        m.assign_material([-1], None)
    # (the refused calls changed no triangle)
    assert np.array_equal(m.flatten()["tri_material"], M.MythTracer(rr.TWO_WAY).flatten()["tri_material"])
    # the switch needs no device, before or after the upload
    m.set_raytree_keep_triangles(True)
    m.set_raytree_keep_triangles(False)
    # the tree calls with several devices
    multi = M.MythTracer()
    multi.set_devices([0, 0])
    multi.set_raytree_keep_triangles(True)
    assert not multi.L.mth_raytree_update_materials(multi.h, None, None, None)
    assert "several devices" in multi.last_error()
    assert not multi.L.mth_raytree_regrow(multi.h, None, None, None)
    assert "several devices" in multi.last_error()


# ---- b. the facade's assignment

def same_assignment(flat_a, tri_material, flat_b):
    """flat_b's triangles carry, by VALUE, the materials `tri_material` names in flat_a's table (a facade that flattens
    again numbers its dense table by first use: the indices may differ, the materials may not)."""
    assert np.array_equal(flat_a["tri_id"], flat_b["tri_id"])
    for s, (want, got) in enumerate(zip(tri_material, flat_b["tri_material"])):
        assert (want < 0) == (got < 0), s
        if want >= 0:
            a, b = flat_a["materials"][want], flat_b["materials"][got]
            assert np.array_equal(a["values"], b["values"]) and a["tex"] == b["tex"], s
    return True


@pytest.mark.parametrize("name", list(ar.ROWS) + list(ar.EXTRA))
def test_flatten_after_assign_material_is_the_flat_assignment_replaced(name):
    moves = dict(ar.ROWS, **ar.EXTRA)[name][0]
    flat = M.MythTracer(rr.TWO_WAY).flatten()
    want = ar.reassigned(flat, rr.TWO_WAY, moves)
    changed = int((want != flat["tri_material"]).sum())
    print("%s: %d of %d triangles reassigned" % (name, changed, len(want)))
    assert changed > 0
    m = M.MythTracer(rr.TWO_WAY)
    to = ar.targets(rr.TWO_WAY, ar.add_order_lines(flat), moves)
    for target in set(to.values()):
        m.assign_material([i for i, t in to.items() if t == target], target)
    flat_b = m.flatten()
    assert same_assignment(flat, want, flat_b)
    # the entries the moves do not reach are the old ones: where the dense table kept its order, index for index
    if len(flat_b["materials"]) == len(flat["materials"]) and all(
            np.array_equal(a["values"], b["values"]) for a, b in zip(flat["materials"], flat_b["materials"])):
        assert np.array_equal(flat_b["tri_material"], want)


def test_the_quad_scene_through_add_triangle():
    m = M.MythTracer()
    ar.quad_scene(m)
    flat = m.flatten()
    want = np.array(flat["tri_material"])
    pos = int(np.nonzero(flat["tri_id"] == ar.QUAD_TRIANGLE)[0][0])
    pane = int(flat["tri_material"][int(np.nonzero(flat["tri_id"] == 2)[0][0])])
    want[pos] = pane
    m.assign_material([ar.QUAD_TRIANGLE], "pane")
    assert same_assignment(flat, want, m.flatten())
    b = M.MythTracer()
    ar.quad_scene(b, True)
    assert same_assignment(flat, want, b.flatten())


# ---- c. the table

@pytest.fixture(scope="module")
def base():
    orc = orclib.OracleScene(rr.TWO_WAY)
    tree = rr.build(orc, CAM, W, H, ar.LIGHTS, 5)
    assert tree["n_rays"] == ar.TREE_A
    return orc, tree


def differing_rays(a, b, plane):
    """Rays of a per-ray plane (n, k) of doubles that differ in a bit between two restated layers, NaN = NaN."""
    x, y = a[plane], b[plane]
    d = (x.view(np.uint64) != y.view(np.uint64)) & ~(np.isnan(x) & np.isnan(y))
    return int(d.reshape(len(x), -1).any(axis=1).sum())


def light_planes_moving(a, b):
    """Entries of power and in_shadow that differ, per layer, over the layers two trees have at the same size."""
    return [me.differing_entries(x, y, "power") + me.differing_entries(x, y, "in_shadow")
            for x, y in zip(a["layers"], b["layers"]) if len(x["coef"]) == len(y["coef"])]


def first_count_difference(a, b):
    for k in range(max(len(a), len(b))):
        if k >= len(a) or k >= len(b) or a[k] != b[k]:
            return k
    return None


@pytest.mark.parametrize("name", list(ar.ROWS))
def test_the_table(name, base, tmp_path):
    moves, want, shadow = ar.ROWS[name]
    orc_a, tree_a = base
    orc = orclib.OracleScene(ar.variant_obj(rr.TWO_WAY, moves, str(tmp_path)))
    # the variant holds the same triangles and the same material table; only the moved triangles' materials differ
    da, ma, _ = orc_a.triangles()
    db, mb, _ = orc.triangles()
    assert np.array_equal(da, db)
    assert [(n, v.tolist(), t) for n, v, t in orc_a.materials()] == [(n, v.tolist(), t) for n, v, t in orc.materials()]
    names = [m[0] for m in orc.materials()]
    to = ar.targets(rr.TWO_WAY, orc_a.triangles()[2], moves)
    for i in range(len(ma)):
        assert mb[i] == (names.index(to[i]) if i in to else ma[i]), i
    tree = rr.build(orc, CAM, W, H, ar.LIGHTS, 5)
    print("%s: rays per layer %s" % (name, tree["n_rays"]))
    assert tree["n_rays"] == want
    # the same triangles added one by one give the same tree and frame
    added = ar.oracle_with(rr.TWO_WAY, moves)
    assert rr.build(added, CAM, W, H, ar.LIGHTS, 5)["n_rays"] == want
    orc.set_lights(ar.LIGHTS)
    added.set_lights(ar.LIGHTS)
    assert np.array_equal(orc.render(CAM, W, H)["rgb"], added.render(CAM, W, H)["rgb"])
    assert (name in ar.SAME_SHAPE) == (tree["n_rays"] == tree_a["n_rays"] and me.same_shape(tree_a, tree))
    moving = light_planes_moving(tree_a, tree)
    print("%s: light-plane entries moving in the layers of equal size: %s" % (name, moving))
    if not shadow:
        assert not any(moving), (name, moving)
    if name == "left->right":
        table = me.diff_table(tree_a, tree)
        print(name, table)
        assert sorted(table) == ["albedo", "material"]
        assert [differing_rays(a, b, "albedo") for a, b in zip(tree_a["layers"], tree["layers"])] == ar.LEFT_RIGHT_ALBEDO
        assert table["material"] == ar.LEFT_RIGHT_ALBEDO
    if name == "mirror->left":
        # only the coef > 0.01 cut moves: the layers that stay are the old ones in shape
        assert tree["n_rays"][:4] == tree_a["n_rays"][:4] and len(tree["n_rays"]) == len(tree_a["n_rays"]) - 1
        for a, b in zip(tree_a["layers"][:3], tree["layers"][:3]):
            assert np.array_equal(a["child_refl"], b["child_refl"]) and np.array_equal(a["child_refr"], b["child_refr"])
    if name in ("pane->blue", "mirror->left"):
        assert len(tree["n_rays"]) < len(tree_a["n_rays"])  # layers disappear
    if name in ("blue->pane", "blue->mirror", "ceiling->pane"):
        assert sum(tree["n_rays"]) > sum(tree_a["n_rays"])
    if name == "ceiling->pane":
        assert moving[0] == 0  # by the rule a shadow ray may see it; no light plane of layer 0 moves
    if name in ar.FIRST_DIFFERENCE:
        assert first_count_difference(tree_a["n_rays"], tree["n_rays"]) == ar.FIRST_DIFFERENCE[name]
    if name.startswith("blue#2"):
        # a triangle no primary ray sees: layer 0 is A's, bit for bit
        assert not any(me.differing_entries(tree_a["layers"][0], tree["layers"][0], p) for p in me.PLANES)


def test_the_cases_with_no_obj_spelling(base, scenes, tmp_path):
    orc_a, tree_a = base
    for name, (moves, want, shadow) in ar.EXTRA.items():
        tree = rr.build(ar.oracle_with(rr.TWO_WAY, moves), CAM, W, H, ar.LIGHTS, 5)
        print("%s: rays per layer %s" % (name, tree["n_rays"]))
        assert tree["n_rays"] == want
    # mirror -> none -> mirror, and any chain A -> B -> A, ends at A: the assignment is A's
    back = rr.build(ar.oracle_with(rr.TWO_WAY, [("mirror", None, None, None), ("mirror", None, None, "mirror")]), CAM, W, H, ar.LIGHTS, 5)
    assert back["n_rays"] == ar.TREE_A
    # one triangle of a quad
    w, h = ar.QUAD_SIZE
    for flag, want in ((False, ar.QUAD_A), (True, ar.QUAD_B)):
        orc = orclib.OracleScene()
        ar.quad_scene(orc, flag)
        orc.finalize()
        tree = rr.build(orc, ar.QUAD_CAMERA, w, h, ar.QUAD_LIGHTS, 5)
        print("quad scene, triangle %d reassigned: %s: rays per layer %s" % (ar.QUAD_TRIANGLE, flag, tree["n_rays"]))
        assert tree["n_rays"] == want
    # room_tex: the red wall given the textured floor material
    w, h = ar.ROOM_TEX["image"]
    lights = lr.BENCH_LIGHTS[:ar.ROOM_TEX["n_lights"]]
    for moves, want in (([], ar.ROOM_TEX_A), (ar.ROOM_TEX_MOVES, ar.ROOM_TEX_B)):
        orc = orclib.OracleScene(ar.variant_obj(scenes["room_tex"], moves, str(tmp_path / ("room_tex%d" % len(moves)))))
        tree = rr.build(orc, scenegen.ROOM_CAMERA, w, h, lights, ar.ROOM_TEX["depth"], chunk=ar.ROOM_TEX["chunk"])
        names = [m[0] for m in orc.materials()]
        on = {n: int((tree["layers"][0]["material"] == names.index(n)).sum()) for n in ("red", "floor")}
        print("room_tex %s: rays per layer %s, layer-0 rays on red / floor: %s" % (moves, tree["n_rays"], on))
        assert tree["n_rays"] == want
        assert (on["red"] == 0) == bool(moves) and orc.materials()[names.index("floor")][2] >= 0


# ---- d. the shadow-visible rule

def test_the_shadow_rule_restated_says_what_the_table_says():
    flat = M.MythTracer(rr.TWO_WAY).flatten()
    values = ar.flat_values(flat)
    for name, (moves, _, shadow) in dict(ar.ROWS, **ar.EXTRA).items():
        now = ar.reassigned(flat, rr.TWO_WAY, moves)
        pairs = ar.changed_pairs(flat["tri_material"], now)
        assert pairs
        got = ar.shadow_visible(values, values, pairs)
        print("%s: %d changed triangles, shadow-visible: %s" % (name, len(pairs), got))
        assert got == shadow, name
        assert not ar.shadow_visible(values, values, [(a, a) for a, _ in pairs])
    # the rule's four clauses on planted tables
    opaque, pane = np.zeros(16), np.zeros(16)
    pane[11], pane[12:15] = 0.5, (0.9, 0.9, 1.0)
    tinted = pane.copy()
    tinted[12:15] = (0.5, 0.9, 1.0)
    filtered_opaque = opaque.copy()
    filtered_opaque[12:15] = (0.5, 0.9, 1.0)
    table = [opaque, pane, tinted, filtered_opaque]
    assert ar.shadow_visible(table, table, [(0, -1)]) and ar.shadow_visible(table, table, [(-1, 0)])
    assert ar.shadow_visible(table, table, [(0, 1)]) and ar.shadow_visible(table, table, [(1, 0)])
    assert ar.shadow_visible(table, table, [(1, 2)])
    assert not ar.shadow_visible(table, table, [(0, 3)])  # both opaque: the filter is never read
    # a under the OLD table, b under the new one
    assert ar.shadow_visible([opaque, opaque], [opaque, pane], [(0, 1)])
    assert not ar.shadow_visible([opaque, pane], [opaque, opaque], [(0, 1)])
