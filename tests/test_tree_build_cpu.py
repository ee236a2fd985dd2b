"""The tree build's claims, without a GPU: the level-by-level restatement (tests/tree_build_ref.py) equals the host
builder's dump on every planted input and on the committed scenes; the device-build switch fails loudly where there is
no GPU; moved vertices give a newly loaded facade's tree.  All comparisons are by bits.
"""
import numpy as np
import pytest

import tree_build_ref as tb

import mythtracer_amd as M

PLANTED = tb.planted()


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    pass


def _host(v):
    return tb.host_dump(tb.facade_of(M, v))


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_restatement_equals_the_host_builder(name):
    v = PLANTED[name]
    want = _host(v)
    got = tb.build(v)
    print("%s: %d triangles, %d nodes, depth %d" % (name, len(v), len(want["first_child"]), want["depth"]))
    assert tb.differences(got, want) == []
    # what the GPU algorithm rests on: ascending add index within a node
    for b, c in zip(want["prim_begin"], want["prim_count"]):
        assert np.all(np.diff(want["tri_id"][b:b + c]) > 0)


def test_planted_inputs_do_what_their_names_say():
    d = {k: tb.build(v) for k, v in PLANTED.items()}
    assert d["n0"]["depth"] == 1 and len(d["n0"]["first_child"]) == 1 and not d["n0"]["node_aabb"].any()
    assert d["n15"]["depth"] == 1 and d["n16"]["depth"] >= 2
    t = d["child_gets_15"]
    assert t["depth"] == 2 and t["prim_count"][1] == 15
    t = d["child_gets_16"]
    assert t["depth"] >= 3 and t["first_child"][8] != 0 and tb.build(PLANTED["child_gets_16"][:15])["depth"] == 1
    assert 10 <= d["corner_chain_10"]["depth"] <= 13
    assert 25 <= d["deep_chain_25"]["depth"] <= 28
    # points on the planes: the first child that contains them (child 0 for the centre itself)
    t = d["points_on_planes"]
    home = np.zeros(len(PLANTED["points_on_planes"]), dtype=int)
    for node, (b, c) in enumerate(zip(t["prim_begin"], t["prim_count"])):
        home[t["tri_id"][b:b + c]] = node
    assert all(h != 0 for h in home[:7]), home[:7]  # none of them stays in the root
    # the root reaches back to the origin; zero bounds are +0.0, NaN never enters it
    assert np.array_equal(tb.bits(d["far_positive"]["node_aabb"][0, :3]), tb.bits(np.zeros(3)))
    assert np.array_equal(tb.bits(d["far_negative"]["node_aabb"][0, 3:]), tb.bits(np.zeros(3)))
    z = d["negative_zero"]
    assert np.signbit(z["tri_aabb"]).any() and (z["tri_aabb"] == 0.0).any()
    assert not np.signbit(z["node_aabb"][0][z["node_aabb"][0] == 0.0]).any()
    assert not np.isnan(d["nan_in_v0"]["node_aabb"][0]).any() and np.isnan(d["nan_in_v0"]["tri_aabb"]).any()
    assert not np.isnan(d["nan_in_v1"]["tri_aabb"]).any()
    assert np.isinf(d["plus_inf"]["node_aabb"][0]).any() and np.isnan(d["both_inf"]["node_center"][0]).any()
    with pytest.raises(tb.DepthExceeded):
        tb.build(tb.never_separate())


def test_restatement_equals_the_host_builder_on_the_grid():
    v = tb.grid16()
    want = _host(v)
    first = want["first_child"]
    assert len(v) == 65536 and (np.diff(first[first != 0]) == 8).all()
    assert tb.differences(tb.build(v), want) == []


@pytest.mark.parametrize("scene", ["two_way", "cornell", "mini", "room"])
def test_restatement_equals_the_host_builder_on_scenes(scene, scenes):
    path = tb.TWO_WAY if scene == "two_way" else scenes[scene]
    m = M.MythTracer(path)
    want = tb.host_dump(m)
    data, _, _ = m.triangles()
    assert tb.differences(tb.build(data[:, :9]), want) == []


def test_device_build_without_a_usable_gpu_fails_loudly():
    """Device 99 exists nowhere: with the switch on Prepare fails with the build's message, and no host-built tree
    stands in its place.  (Without any GPU the message is the runtime's, with GPUs it names the device.)"""
    m = tb.facade_of(M, PLANTED["n64"], device=99)
    m.set_device_tree_build(True)
    with pytest.raises(RuntimeError, match="device tree build failed"):
        m.prepare()
    assert len(m.tree()["first_child"]) == 0
    m.set_device_tree_build(False)
    assert len(m.tree()["first_child"]) > 1  # the host builder, once it is asked


def _moved(v, idx, shift):
    out = v.copy()
    out[idx] = out[idx] + np.asarray(shift, dtype=np.float64)
    return out


@pytest.mark.parametrize("case", ["inside", "shrinks_root", "grows_root"])
def test_moved_vertices_give_a_new_facades_tree(case):
    v = PLANTED["shuffled"].copy()
    v[7] += 30.0  # one triangle far out: the root box hangs on it
    idx, shift = {"inside": (np.arange(100, 140), (0.75, -0.5, 0.25)), "shrinks_root": (np.array([7]), (-30.0, -30.0, -30.0)),
                  "grows_root": (np.array([3, 4]), (-50.0, 0.0, 60.0))}[case]
    m = tb.facade_of(M, v)
    before = tb.host_dump(m)
    moved = _moved(v, idx, shift)
    m.set_triangle_vertices(idx, moved[idx])
    m.update_geometry()
    got = tb.host_dump(m)
    want = _host(moved)
    assert tb.differences(got, want) == []
    assert tb.differences(got, before) != []
    assert np.array_equal(m.root_aabb(), want["node_aabb"][0])
    if case == "shrinks_root":
        assert (want["node_aabb"][0, 3:] < before["node_aabb"][0, 3:]).all()


def test_set_triangle_vertices_refuses_a_bad_index():
    m = tb.facade_of(M, PLANTED["n16"])
    before = tb.host_dump(m)
    with pytest.raises(RuntimeError, match="triangle index 16 outside the scene's 16 triangles"):
        m.set_triangle_vertices([2, 16], np.zeros((2, 3, 3)))
    with pytest.raises(ValueError):
        m.set_triangle_vertices([2], np.zeros((2, 3, 3)))
    assert tb.differences(tb.host_dump(m), before) == []
