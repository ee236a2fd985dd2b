"""Triangles added and removed in place, without a GPU: tests/native/edit_check.cc, a stand-alone program around
mythtracer_amd/csrc/mt_edit.h that checks the refusals in their order and the composition of the edited scene's host
mirrors against brute force, built with the address and undefined-behaviour sanitizers (their runtimes linked
statically) and run as a program of its own; the new C-ABI call's NULL-scene refusal, which needs no device; the
binding's declarations; and tests/edit_triangles_ref.py itself -- its mirrors against a search, and every planted edit
against what its name promises, so that the GPU test cannot pass on an edit that changes nothing."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import edit_triangles_ref as ed
import move_ref as mv
import tree_build_ref as tb

import mythtracer_amd as M
from mythtracer_amd import binding, build

HERE = os.path.dirname(os.path.abspath(__file__))
MT_ERR_ARG, MT_ERR_HIP = -1, -2
EDITS = ed.edits()


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    return native_libs


def test_edit_check(tmp_path):
    exe = str(tmp_path / "edit_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-I", build.INC, "-I", build.CSRC,
                         "-o", exe, os.path.join(HERE, "native", "edit_check.cc")],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert cc.returncode == 0, cc.stdout.decode()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    print(r.stdout.decode())
    assert r.returncode == 0, r.stdout.decode()
    assert "all checks held" in r.stdout.decode()


def test_symbols_and_abi_version():
    abi = M.hip_abi()
    assert binding.MT_ABI_VERSION == 5 == abi.lib.mt_abi_version()
    assert "mt_scene_edit_triangles" in M.HIP_SYMBOLS and abi.lib.mt_scene_edit_triangles is not None
    assert len(abi.lib.mt_scene_edit_triangles.argtypes) == 10
    for name in ("mth_add_triangles", "mth_remove_triangles", "mth_update_triangles_in_place"):
        assert getattr(M.host_lib(), name) is not None
    assert callable(abi.scene_edit_triangles)
    for name in ("add_triangles", "remove_triangles", "update_triangles_in_place"):
        assert callable(getattr(binding.MythTracer, name))


def test_a_null_scene_is_refused_before_any_device_call():
    abi = M.hip_abi()
    idx, v, m, info = np.zeros(4, dtype=np.int32), np.zeros(36), np.zeros(4, dtype=np.int32), binding.mt_build_info()
    p, q = v.ctypes.data, m.ctypes.data
    for args in ((idx.ctypes.data, 4, 4, p, p, p, q, q, ctypes.byref(info)), (None, 4, 4, None, None, None, None, None, None),
                 (None, -1, -1, None, None, None, None, None, None), (None, 0, 0, None, None, None, None, None, None)):
        rc = abi.lib.mt_scene_edit_triangles(None, *args)  # its message wins over everything about the lists
        assert rc == MT_ERR_ARG and rc != MT_ERR_HIP, (rc, abi.last_error())
        assert abi.last_error() == "scene is NULL"
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.scene_edit_triangles(None, [0], None)
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.scene_edit_triangles(None, None, ed.added(np.zeros((2, 3, 3))))
    short = ed.added(np.zeros((2, 3, 3)))
    short["tri_uvw"] = short["tri_uvw"][:1]
    with pytest.raises(ValueError, match="9 per triangle"):
        abi.scene_edit_triangles(None, None, short)


def test_the_facade_refuses_a_batch_while_moves_are_pending():
    """Host only: moved vertices name triangles by indices that a removal would renumber."""
    m = M.MythTracer(tb.TWO_WAY)
    n = m.triangles()[0].shape[0]
    v = m.triangles()[0][:2, :9].reshape(2, 3, 3).copy()
    m.set_triangle_vertices([1], v[1:] + 1.0)
    with pytest.raises(RuntimeError, match="UpdateGeometryInPlace"):
        m.remove_triangles([0])
    with pytest.raises(RuntimeError, match="UpdateGeometryInPlace"):
        m.add_triangles(v)
    assert m.triangles()[0].shape[0] == n
    m.update_geometry()  # (takes the moved vertices; nothing is pending afterwards)
    m.remove_triangles([0])
    m.add_triangles(v)
    assert m.triangles()[0].shape[0] == n + 1 and len(m.tree()["prim_ids"]) == n + 1  # nothing uploaded: the tree is built anew
    with pytest.raises(RuntimeError, match="UpdateTrianglesInPlace"):
        m.set_triangle_vertices([0], v[:1])
    with pytest.raises(RuntimeError, match="update"):
        m.remove_triangles([0])


# ---- edit_triangles_ref

def test_the_new_order_is_delete_then_concatenate():
    """new index = old index - the removed indices below it, by counting; the added follow in the order given"""
    rng = np.random.RandomState(4)
    for n in (1, 2, 15, 16, 17, 1025):
        for n_remove in (0, 1, n // 2, n - 1):
            remove = rng.permutation(n)[:n_remove]
            got = ed.new_order(np.arange(n) * 10, remove, np.array([-1, -2, -3]))
            want = [a * 10 for a in range(n) if a not in set(remove.tolist())] + [-1, -2, -3]
            assert list(got) == want
            for a in range(n):
                if a not in set(remove.tolist()):
                    assert got[a - int((remove < a).sum())] == a * 10


def test_the_mirrors_follow_their_triangles():
    """tri_mtl and the stamp planes are per stream position; after the edit the entry at p belongs to the triangle with
    the new add index new_tri_id[p]: a survivor keeps its entry, an added triangle has its own material and stamp 0."""
    v, steps = EDITS["swap_in_one_call"]
    tris = mv.scene_of(v)
    state = ed.state_of(tris)
    n = len(v)
    by_add = 7 + np.arange(n, dtype=np.uint32)
    state["tri_mtl"] = (np.arange(n, dtype=np.int32) * 10)[state["tri_id"]]
    state["stamp"] = [None, by_add[state["tri_id"]]]
    remove, add_v = steps[1]
    add = ed.added(add_v)
    now = ed.after_edit(state, remove, add)
    assert now["geo"] == 1 and len(now["tri_id"]) == n - 5 + 6 and now["stamp"][0] is None
    survivors = [a for a in range(n) if a not in set(remove.tolist())]
    for p, a_new in enumerate(now["tri_id"]):
        if a_new < len(survivors):
            assert now["tri_mtl"][p] == survivors[a_new] * 10 and now["stamp"][1][p] == 7 + survivors[a_new]
        else:
            assert now["tri_mtl"][p] == add["tri_material"][a_new - len(survivors)] and now["stamp"][1][p] == 0
    assert np.array_equal(now["tris"]["tri_line_no"][:len(survivors)], tris["tri_line_no"][survivors])
    assert ed.after_edit(now, [], None) is now and ed.after_edit(now, None, None) is now  # the no-op


def _trees(name):
    v, steps = EDITS[name]
    vs = ed.vertices_after(v, steps)
    return [tb.build(x) for x in vs], vs


def _rows(v):
    r = tb.bits(np.asarray(v).reshape(-1, 9))
    return r[np.lexsort(r.T[::-1])]


@pytest.mark.parametrize("name", sorted(EDITS))
def test_every_chain_ends_where_it_began(name):
    """... with the triangles it began with; in their order too, unless the name says otherwise"""
    trees, vs = _trees(name)
    assert np.array_equal(_rows(vs[-1]), _rows(vs[0]))
    assert tb.differences(trees[1], trees[0]) != []
    if name in ed.OTHER_ORDER:
        assert not np.array_equal(tb.bits(vs[-1]), tb.bits(vs[0])) and tb.differences(trees[-1], trees[0]) != []
    else:
        assert np.array_equal(tb.bits(vs[-1]), tb.bits(vs[0])) and tb.differences(trees[-1], trees[0]) == []
    for (remove, add_v), before in zip(EDITS[name][1], vs):  # every step is a legal edit that is not the no-op
        assert len(set(remove.tolist())) == len(remove) and all(0 <= a < len(before) for a in remove)
        assert len(remove) + (0 if add_v is None else len(add_v)) > 0


def _own(tree, node=0):
    return int(tree["prim_count"][node])


def test_the_planted_edits_do_what_their_names_say():
    t, _ = _trees("leaf_15_to_16")
    assert t[0]["prim_count"][1] == 15 and t[0]["first_child"][1] == 0 and t[1]["first_child"][1] != 0
    assert len(t[1]["first_child"]) > len(t[0]["first_child"]) == len(t[2]["first_child"])
    t, vs = _trees("sixteenth_out_and_in")
    assert t[0]["first_child"][1] != 0 and t[1]["first_child"][1] == 0 and t[1]["prim_count"][1] == 15
    assert len(t[0]["first_child"]) > len(t[1]["first_child"]) and len(t[2]["first_child"]) == len(t[0]["first_child"])
    assert not np.array_equal(t[2]["tri_id"], t[0]["tri_id"])
    t, _ = _trees("short_to_long")
    assert (_own(t[0]), _own(t[1]), _own(t[2])) == (ed.SHORT, ed.SHORT + 1, ed.SHORT)
    t, _ = _trees("long_across_pad")
    assert (_own(t[0]), _own(t[1]), _own(t[2])) == (ed.PAD, ed.PAD + 1, ed.PAD)
    t, _ = _trees("root_grows_and_shrinks")
    assert t[1]["node_aabb"][0, 3] > t[0]["node_aabb"][0, 3] == 8.0 == t[2]["node_aabb"][0, 3]
    for name in ("nan_in_v0", "nan_in_v1"):
        _, vs = _trees(name)
        assert not np.isnan(vs[0]).any() and np.isnan(vs[1]).any()
    assert np.isnan(_trees("nan_in_v0")[0][1]["tri_aabb"]).any() and not np.isnan(_trees("nan_in_v1")[0][1]["tri_aabb"]).any()
    for name in ("plus_inf", "minus_inf", "both_inf"):
        t, _ = _trees(name)
        assert np.isinf(t[1]["tri_aabb"]).any() and not np.isinf(t[0]["tri_aabb"]).any()
    t, _ = _trees("chain_deepens")
    assert t[0]["depth"] < ed.DEEP_FROM <= t[1]["depth"] <= 16
    t, _ = _trees("chain_past_16")
    assert t[0]["depth"] < ed.DEEP_FROM and 16 < t[1]["depth"] <= 24
    _, vs = _trees("remove_forms")
    assert [len(x) for x in vs] == [65, 64, 63, 31, 1, 65]
    (r0, _), (r1, _), (r2, _), _, (r4, a4) = EDITS["remove_forms"][1]
    assert list(r0) == [0] and list(r1) == [63] and list(r2) != sorted(r2) and len(r4) == 1 and len(a4) == 65
    _, vs = _trees("swap_in_one_call")
    assert [len(x) for x in vs] == [63, 63, 64, 63]
    assert all(len(r) > 0 and a is not None for r, a in EDITS["swap_in_one_call"][1])
    _, vs = _trees("counts")
    sizes = [len(x) for x in vs]
    for pair in ((1, 2), (15, 16), (16, 15), (63, 65), (65, 1)):
        assert pair in list(zip(sizes, sizes[1:])), pair
    _, vs = _trees("n1024")
    assert [len(x) for x in vs] == [1024, 1025, 1024]
    add = ed.added(np.zeros((7, 3, 3)))
    textured = {i for i, m in enumerate(mv.MATERIALS) if m["tex"] >= 0}
    assert -1 in add["tri_material"] and textured & set(add["tri_material"].tolist())
    assert not set(add["tri_line_no"].tolist()) & set(mv.scene_of(np.zeros((2000, 3, 3)))["tri_line_no"].tolist())


def test_the_frame_tests_scene_is_visible():
    """The frames with history, the no-op test and the other calls render `shuffled`: by its geometry well over 200
    pixels of the 64 x 48 frame are covered, before and after the edit, and a tenth of the triangles is exchanged."""
    v, steps = EDITS["shuffled"]
    vs = ed.vertices_after(v, steps)
    assert all(mv.expected_hit_pixels(x) > 200 for x in vs)
    assert len(v) == 1000 and len(steps[0][0]) == 100 == len(steps[0][1])
    assert tb.differences(tb.build(vs[1]), tb.build(vs[0])) != []


def test_the_edit_after_other_edits_is_visible():
    v, remove, add_v = ed.visible_edit()
    after = ed.new_order(v, remove, add_v)
    assert len(after) == len(v) + 1 and mv.expected_hit_pixels(v) > 200 and mv.expected_hit_pixels(after) > 200


def test_the_depth_refusal_is_planted():
    v, add_v = ed.never_separate_edit()
    assert tb.build(v)["depth"] <= 8
    with pytest.raises(tb.DepthExceeded, match="octree depth 65 exceeds MT_MAX_TREE_DEPTH 64"):
        tb.build(np.concatenate([v, add_v]))
