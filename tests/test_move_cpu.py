"""Triangles moved in place, without a GPU: tests/native/move_check.cc, a stand-alone program around
mythtracer_amd/csrc/mt_move.h that checks the index-list refusals in their order and the permutation of the scene's host
mirrors against brute force, built with the address and undefined-behaviour sanitizers (their runtimes linked
statically) and run as a program of its own; the two new C-ABI calls' NULL-scene refusal, which needs no device; the
binding's declarations; and tests/move_ref.py itself -- its composed permutation against a search, and every planted
move against what its name promises, so that the GPU test cannot pass on a move that moves nothing."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import move_ref as mv
import tree_build_ref as tb

import mythtracer_amd as M
from mythtracer_amd import binding, build

HERE = os.path.dirname(os.path.abspath(__file__))
MT_ERR_ARG, MT_ERR_HIP = -1, -2
MOVES = mv.moves()


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    return native_libs


def test_move_check(tmp_path):
    exe = str(tmp_path / "move_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-I", build.INC, "-I", build.CSRC,
                         "-o", exe, os.path.join(HERE, "native", "move_check.cc")],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert cc.returncode == 0, cc.stdout.decode()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    print(r.stdout.decode())
    assert r.returncode == 0, r.stdout.decode()
    assert "all checks held" in r.stdout.decode()


def test_symbols_and_abi_version():
    abi = M.hip_abi()
    assert binding.MT_ABI_VERSION == 5 == abi.lib.mt_abi_version()
    for name in ("mt_scene_set_triangle_vertices", "mt_scene_get_triangle_vertices", "mt_scene_move_times_last"):
        assert name in M.HIP_SYMBOLS and getattr(abi.lib, name) is not None
    assert getattr(M.host_lib(), "mth_update_geometry_in_place") is not None
    for name in ("scene_set_triangle_vertices", "scene_get_triangle_vertices", "scene_move_times"):
        assert callable(getattr(abi, name))
    assert callable(binding.MythTracer.update_geometry_in_place)


def test_a_null_scene_is_refused_before_any_device_call():
    abi = M.hip_abi()
    idx, v, info = np.zeros(4, dtype=np.int32), np.zeros(36), binding.mt_build_info()
    for a, n, p, i in ((idx.ctypes.data, 4, v.ctypes.data, ctypes.byref(info)), (None, 4, None, None), (None, -1, None, None),
                       (None, 0, None, None)):
        rc = abi.lib.mt_scene_set_triangle_vertices(None, a, n, p, i)  # its message wins over everything about the list
        assert rc == MT_ERR_ARG and rc != MT_ERR_HIP, (rc, abi.last_error())
        assert abi.last_error() == "scene is NULL"
    for p, n in ((v.ctypes.data, 4), (None, 4), (None, 0), (v.ctypes.data, -1)):
        assert abi.lib.mt_scene_get_triangle_vertices(None, p, n) == MT_ERR_ARG
        assert abi.last_error() == "scene is NULL"
    assert abi.lib.mt_scene_move_times_last(None, v.ctypes.data) == MT_ERR_ARG and abi.last_error() == "scene is NULL"
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.scene_set_triangle_vertices(None, [0], np.zeros((1, 3, 3)))
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.scene_get_triangle_vertices(None, 3)
    with pytest.raises(ValueError, match="9 per triangle"):
        abi.scene_set_triangle_vertices(None, [0, 1], np.zeros((1, 3, 3)))


# ---- move_ref

def test_compose_is_the_search():
    rng = np.random.RandomState(5)
    for n in (0, 1, 15, 16, 17, 1025):
        old, new = rng.permutation(n), rng.permutation(n)
        src = mv.compose(old, new)
        want = [int(np.nonzero(old == a)[0][0]) for a in new]
        assert list(src) == want
        assert list(mv.compose(old, old)) == list(range(n))


def test_the_mirrors_follow_their_triangles():
    """tri_mtl and the stamp planes are per stream position; after the move the entry at p belongs to add index
    new_tri_id[p], as before the move the entry at q belonged to old_tri_id[q]."""
    v, steps = MOVES["leaf_15_to_16"]
    tree = tb.build(v)
    n = len(v)
    by_add = np.arange(n) * 10
    state = dict(vertex=v, tri_id=tree["tri_id"], tri_mtl=by_add[tree["tri_id"]], stamp=[None, (by_add + 1)[tree["tri_id"]]], geo=0)
    now = mv.after_move(state, *steps[0])
    assert now["geo"] == 1 and not np.array_equal(now["tri_id"], state["tri_id"])
    assert np.array_equal(now["tri_mtl"], by_add[now["tri_id"]]) and now["stamp"][0] is None
    assert np.array_equal(now["stamp"][1], (by_add + 1)[now["tri_id"]])
    # the same vertices again, by bits: nothing moves, nothing is bumped
    assert mv.after_move(now, steps[0][0], steps[0][1]) is now
    assert len(mv.changed_triangles(now["vertex"], *steps[0])) == 0
    # -0.0 for +0.0 is a change; NaN for the same NaN is none
    z = np.zeros((1, 3, 3))
    assert len(mv.changed_triangles(z, [0], -z)) == 1
    assert len(mv.changed_triangles(np.full((1, 3, 3), mv.NAN), [0], np.full((1, 3, 3), mv.NAN))) == 0


def _trees(name):
    v, steps = MOVES[name]
    out = [tb.build(v)]
    cur = v.copy()
    for idx, listed in steps:
        cur = cur.copy()
        cur[idx] = listed
        out.append(tb.build(cur))
    return out, cur


@pytest.mark.parametrize("name", sorted(MOVES))
def test_every_chain_ends_where_it_began(name):
    trees, last = _trees(name)
    assert np.array_equal(tb.bits(last), tb.bits(MOVES[name][0]))
    assert tb.differences(trees[-1], trees[0]) == []
    assert tb.differences(trees[1], trees[0]) != []


def _own(tree, node=0):
    return int(tree["prim_count"][node])


def test_the_planted_moves_do_what_their_names_say():
    t, _ = _trees("nudge")
    assert tb.differences(t[1], t[0]) == ["tri_aabb (%d vs %d values)" % (t[0]["tri_aabb"].size, t[0]["tri_aabb"].size)]
    t, _ = _trees("to_sibling")
    assert np.array_equal(t[0]["first_child"], t[1]["first_child"]) and not np.array_equal(t[0]["prim_count"], t[1]["prim_count"])
    assert _own(t[0]) == _own(t[1])
    t, _ = _trees("onto_plane")
    assert _own(t[1]) == _own(t[0]) + 1
    t, _ = _trees("leaf_15_to_16")
    assert t[0]["prim_count"][1] == 15 and t[0]["first_child"][1] == 0 and t[1]["first_child"][1] != 0
    assert len(t[1]["first_child"]) > len(t[0]["first_child"])
    t, _ = _trees("short_to_long")
    assert (_own(t[0]), _own(t[1])) == (mv.SHORT, mv.SHORT + 1)
    t, _ = _trees("long_across_pad")
    assert (_own(t[0]), _own(t[1])) == (mv.PAD, mv.PAD + 1)
    t, _ = _trees("root_grows")
    assert t[1]["node_aabb"][0, 3] > t[0]["node_aabb"][0, 3] == 8.0
    t, _ = _trees("root_shrinks")
    assert t[1]["node_aabb"][0, 3] == 8.0 < t[0]["node_aabb"][0, 3]
    t, _ = _trees("negative_zero")
    signs = lambda tree: int(np.signbit(tree["tri_aabb"][tree["tri_aabb"] == 0.0]).sum())  # noqa: E731
    assert signs(t[1]) > signs(t[0]) == 0
    for name in ("nan_in_v0", "nan_in_v1"):
        t, _ = _trees(name)
        assert not np.isnan(MOVES[name][0]).any() and np.isnan(MOVES[name][1][0][1]).any()
    assert np.isnan(_trees("nan_in_v0")[0][1]["tri_aabb"]).any() and not np.isnan(_trees("nan_in_v1")[0][1]["tri_aabb"]).any()
    for name in ("plus_inf", "minus_inf", "both_inf"):
        t, _ = _trees(name)
        assert np.isinf(t[1]["tri_aabb"]).any() and not np.isinf(t[0]["tri_aabb"]).any()
    t, _ = _trees("chain_deepens")
    assert t[0]["depth"] < mv.DEEP_FROM <= t[1]["depth"] <= 16
    t, _ = _trees("chain_past_16")
    assert t[0]["depth"] < mv.DEEP_FROM and 16 < t[1]["depth"] <= 24
    for n in (1, 15, 16, 63, 65, 1025):
        assert len(MOVES["n%d" % n][0]) == n
    forms = [len(idx) for idx, _ in MOVES["list_forms"][1]]
    assert forms == [65, 1, 33, 65] and list(MOVES["list_forms"][1][2][0]) != sorted(MOVES["list_forms"][1][2][0])


def test_the_frame_tests_scene_is_visible():
    """The frames with history, the no-op test and the other calls render `shuffled`: by its geometry about a tenth of
    the 64 x 48 frame is covered, before and after the move, and a third of the triangles move by up to 0.75."""
    v, steps = MOVES["shuffled"]
    idx, listed = steps[0]
    w = v.copy()
    w[idx] = listed
    assert mv.expected_hit_pixels(v) > 200 and mv.expected_hit_pixels(w) > 200
    assert len(idx) == len(v) // 3 and np.abs(listed - v[idx]).max() > 0.5


def test_the_depth_refusal_is_planted():
    v, idx, listed = mv.never_separate_move()
    assert tb.build(v)["depth"] <= 8
    w = v.copy()
    w[idx] = listed
    with pytest.raises(tb.DepthExceeded, match="octree depth 65 exceeds MT_MAX_TREE_DEPTH 64"):
        tb.build(w)
