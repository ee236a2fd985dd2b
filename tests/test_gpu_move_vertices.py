"""Triangles moved in place, on a real MI355X (-m gpu): mt_scene_set_triangle_vertices / mt_scene_get_triangle_vertices
and MythTracer::UpdateGeometryInPlace (include/mythtracer_hip.h; the kernels are in mythtracer_amd/csrc/mt_build.h, the
host bookkeeping in mt_move.h).

The bar is identity, no tolerance: after every move the scene is compared with a scene NEWLY made by
mt_scene_create_triangles from the same add-order arrays with the new vertices -- every array of mt_scene_read_tree, a
64 x 48 depth-5 frame with its debug planes and counters, every G-buffer and light-buffer plane, every getter.  The
planted moves are tests/move_ref.py's, which tests/test_move_cpu.py holds to what their names promise without a GPU.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import move_ref as mv  # noqa: E402
import tree_build_ref as tb  # noqa: E402
import vertex_attr_ref as va  # noqa: E402
from test_gpu_tree_build import DEPTH_MESSAGE, blue_block, moved_copy  # noqa: E402

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding  # noqa: E402

MOVES = mv.moves()
W, H, DEPTH = mv.W, mv.H, mv.DEPTH
MT_ERR_ARG, MT_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"


def counters(stats):
    return {k: v for k, v in stats.items() if not k.endswith("_ms")}


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(tb.bits(a), tb.bits(b))


def look(abi, h, view, frames=1):
    """Everything the contract names that a host call gives, from scene h under the camera and lights of `view`.  The
    counters of a frame are compared between frames scheduled alike: the cost history, a forecast that a moved scene
    keeps and a new scene does not have, is switched off here on both (test_frames_after_a_move_with_history renders
    with it)."""
    cam, lights = view
    abi.set_lights(h, lights)
    abi.set_scheduling(h, False)
    sens = binding.sensor(cam, W, H)
    out = dict(tree=abi.scene_read_tree(h))
    nt = len(out["tree"]["tri_id"])
    for f in range(frames):
        frame = abi.render_chunk(h, sens, W, H, max_depth=DEPTH, debug=True)
        out.update({"rgb%d" % f: frame["rgb"], "line%d" % f: frame["line"], "point%d" % f: frame["point"],
                    "stats%d" % f: counters(frame["stats"])})
    gb = abi.render_gbuffer(h, sens, W, H)
    out["gb_stats"] = counters(gb.pop("stats"))
    out.update({"gb_" + k: v for k, v in gb.items()})
    lb = abi.render_lightbuffer(h, sens, W, H, len(lights))
    out["lb_stats"] = counters(lb.pop("stats"))
    out.update({"lb_" + k: v for k, v in lb.items()})
    out.update(vertices=abi.scene_get_triangle_vertices(h, nt), normals=abi.get_triangle_normals(h, nt),
               uvw=abi.get_triangle_uvw(h, nt), mtl=abi.get_triangle_materials(h, nt))
    return out


def differences(got, want):
    out = ["tree: " + d for d in tb.differences(got["tree"], want["tree"])]
    for k in sorted(want):
        if k == "tree":
            continue
        if isinstance(want[k], dict):
            if got[k] != want[k]:
                out.append("%s: %r != %r" % (k, got[k], want[k]))
        elif not same(got[k], want[k]):
            out.append(k)
    return out


def view_of(v):
    return mv.camera_for(v), mv.lights_for(v)


def new_scene_look(abi, tris, v, view, frames=1):
    h, _ = abi.scene_create_triangles(mv.with_vertices(tris, v))
    try:
        return look(abi, h, view, frames)
    finally:
        abi.scene_destroy(h)


# ---- (a) the planted moves

@pytest.mark.parametrize("name", sorted(MOVES))
def test_moved_scene_is_the_new_scene(name):
    abi = M.hip_abi()
    v, steps = MOVES[name]
    tris = mv.scene_of(v)
    cur = v.copy()
    h, _ = abi.scene_create_triangles(tris)
    try:
        first = look(abi, h, view_of(v))  # (frames before the move: the scene has launch state)
        assert not any(abi.scene_move_times(h).values())  # (no set yet that changed a triangle)
        if name == "shuffled":  # the scene the frame tests render: the camera must see about what its geometry promises
            # (triangles smaller than a pixel are hit or missed by chance and nearer ones hide farther ones: a quarter
            # of the estimate, which tests/test_move_cpu.py holds above 200 pixels, is asked for)
            assert (first["gb_prim"] >= 0).sum() > mv.expected_hit_pixels(v) / 4.0, "the camera sees too little"
        for k, (idx, listed) in enumerate(steps):
            info = abi.scene_set_triangle_vertices(h, idx, listed)
            cur = cur.copy()
            cur[idx] = listed
            want_tree = tb.build(cur)
            assert (info["n_nodes"], info["depth"]) == (len(want_tree["first_child"]), want_tree["depth"]), (name, k)
            assert info["total_ms"] >= info["kernel_ms"] > 0.0
            parts = abi.scene_move_times(h)  # the parts of this set: each took time, together no more than the call
            assert sorted(parts) == ["build", "layout", "readback", "regather", "upload"] and min(parts.values()) > 0.0
            assert parts["build"] >= info["kernel_ms"] and sum(parts.values()) <= info["total_ms"]
            view = view_of(cur)
            got, want = look(abi, h, view), new_scene_look(abi, tris, cur, view)
            assert differences(got, want) == [], (name, k)
            assert tb.differences(got["tree"], want_tree) == [], (name, k)
            assert same(got["vertices"], cur)
        assert differences(look(abi, h, view_of(v)), first) == []  # every chain ends where it began
    finally:
        abi.scene_destroy(h)


# ---- (b) with history, on every engine

@pytest.mark.parametrize("lean", [1, 2])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("engine", [0, 1, 2, 3])
def test_frames_after_a_move_with_history(engine, mode, lean):
    abi = M.hip_abi()
    v, steps = MOVES["shuffled"]
    idx, listed = steps[0]
    tris = mv.scene_of(v)
    cur = v.copy()
    cur[idx] = listed
    view = view_of(v)
    sens = binding.sensor(view[0], W, H)

    def switches(h):
        abi.set_engine(h, engine)
        abi.set_traversal_mode(h, mode)
        abi.set_tuning(h, "LEAN_KERNEL", lean)
        abi.set_lights(h, view[1])

    def frames(h, n):
        return [abi.render_chunk(h, sens, W, H, max_depth=DEPTH, debug=True) for _ in range(n)]

    h, _ = abi.scene_create_triangles(tris)
    g, _ = abi.scene_create_triangles(mv.with_vertices(tris, cur))
    try:
        switches(h)
        switches(g)
        before = frames(h, 2)
        abi.scene_set_triangle_vertices(h, idx, listed)
        got, want = frames(h, 3), frames(g, 3)
        assert not np.array_equal(got[0]["rgb"], before[1]["rgb"])
        for a, b in zip(got, want):
            assert np.array_equal(a["rgb"], b["rgb"]) and np.array_equal(a["line"], b["line"]) and same(a["point"], b["point"])
    finally:
        abi.scene_destroy(h)
        abi.scene_destroy(g)


# ---- (c) a chain of moves, and the moves undone

def test_three_moves_and_back():
    abi = M.hip_abi()
    v = MOVES["n65"][0]
    rng = np.random.RandomState(11)
    tris = mv.scene_of(v)
    view = view_of(v)
    h, _ = abi.scene_create_triangles(tris)
    try:
        original = look(abi, h, view, frames=2)
        cur, undo = v.copy(), []
        for _ in range(3):
            idx = rng.permutation(65)[:20].astype(np.int32)
            undo.append((idx, cur[idx].copy()))
            listed = cur[idx] + 2.0 * (rng.random_sample((20, 3, 3)) - 0.5)
            abi.scene_set_triangle_vertices(h, idx, listed)
            cur[idx] = listed
            assert differences(look(abi, h, view), new_scene_look(abi, tris, cur, view)) == []
        for idx, was in reversed(undo):
            abi.scene_set_triangle_vertices(h, idx, was)
        assert differences(look(abi, h, view, frames=2), original) == []
    finally:
        abi.scene_destroy(h)


# ---- (d) after other edits: the attributes follow their triangles by add index

def tree_planes(abi, t):
    info = abi.raytree_info(t)
    out = dict(n_layers=info["n_layers"], n_rays=list(info["n_rays"]))
    for k in range(info["n_layers"]):
        for name, a in abi.raytree_read_layer(t, k).items():
            out["%d_%s" % (k, name)] = a
        out["%d_tri" % k] = abi.raytree_read_tri(t, k)
        out["%d_uvw" % k] = abi.raytree_read_uvw(t, k)
    return out


def test_move_after_other_edits_and_a_regrow_in_the_new_order():
    abi = M.hip_abi()
    v, steps = MOVES["leaf_15_to_16"]
    idx, listed = steps[0]
    n = len(v)
    tris = mv.scene_of(v)
    rng = np.random.RandomState(3)
    # the edits, by ADD index
    mats = [dict(values=m["values"].copy(), tex=m["tex"]) for m in mv.MATERIALS]
    mats[0]["values"][0:3] = (0.2, 0.9, 0.4)
    mats[3]["tex"] = 0
    texels = rng.randint(0, 256, (3, 5, 3)).astype(np.uint8)
    mtl = np.roll(tris["tri_material"], 1)
    nrm = tris["tri_normal"].reshape(n, 3, 3).copy()
    nrm[::2] = nrm[::2][:, ::-1]
    uvw = tris["tri_uvw"].reshape(n, 3, 3).copy()
    uvw[1::3, :, :2] += 0.25
    nrm2 = nrm.copy()
    nrm2[[idx[0], 3, 7, 12]] = [[0.0, 1.0, 0.0]] * 3  # the moved triangle's normal and three more, edited after the move
    view = view_of(v)
    sens = binding.sensor(view[0], W, H)
    cur = v.copy()
    cur[idx] = listed

    def edited(final_normals):
        out = mv.with_vertices(tris, cur)
        out.update(tri_material=mtl, tri_normal=final_normals.reshape(-1, 9), tri_uvw=uvw.reshape(-1, 9), materials=mats,
                   textures=[dict(texels=texels), tris["textures"][1]])
        return out

    h, _ = abi.scene_create_triangles(tris)
    trees = []
    try:
        ids = abi.scene_read_tree(h)["tri_id"]
        abi.set_materials(h, mats)
        abi.set_texture(h, 0, texels)
        abi.set_triangle_materials(h, mtl[ids])
        abi.set_triangle_normals(h, nrm[ids])
        abi.set_triangle_uvw(h, uvw[ids])
        abi.scene_set_triangle_vertices(h, idx, listed)
        g, _ = abi.scene_create_triangles(edited(nrm))
        try:
            assert differences(look(abi, h, view), look(abi, g, view)) == []
        finally:
            abi.scene_destroy(g)
        ids = abi.scene_read_tree(h)["tri_id"]  # the NEW order
        assert same(abi.get_triangle_normals(h, n), nrm[ids]) and np.array_equal(abi.get_triangle_materials(h, n), mtl[ids])
        # a tree with tri and uvw, one normal edited in the new order, a regrow: the stamp planes were permuted
        abi.set_raytree_tri(h, True)
        abi.set_raytree_uvw(h, True)
        abi.set_lights(h, view[1])
        t, _ = abi.raytree_create(h, sens, W, H, max_depth=DEPTH)
        trees.append(t)
        abi.set_triangle_normals(h, nrm2[ids])
        abi.raytree_regrow(t)
        g, _ = abi.scene_create_triangles(edited(nrm2))
        try:
            abi.set_raytree_tri(g, True)
            abi.set_raytree_uvw(g, True)
            abi.set_lights(g, view[1])
            assert np.array_equal(abi.scene_read_tree(g)["tri_id"], ids)
            u, _ = abi.raytree_create(g, sens, W, H, max_depth=DEPTH)
            try:
                got, want = tree_planes(abi, t), tree_planes(abi, u)
            finally:
                abi.raytree_destroy(u)
        finally:
            abi.scene_destroy(g)
        assert want["n_rays"][0] == W * H and (want["0_tri"] >= 0).any()
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k] == want[k] if isinstance(want[k], (int, list)) else same(got[k], want[k]), k
    finally:
        for t in trees:
            abi.raytree_destroy(t)
        abi.scene_destroy(h)


def texels_of(seed, shape):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def with_texture0(tris, texels0, texels1=None):
    """tris with texture 0, and texture 1 where given, replaced"""
    t1 = tris["textures"][1] if texels1 is None else dict(texels=texels1)
    return dict(tris, textures=[dict(texels=texels0), t1])


def test_textures_set_between_and_after_moves():
    """A texture set patches the scene's table allocations, a move replaces its geometry allocations: texture 0 is
    replaced on both sides of a move, texture 1 between two moves, and every state is the newly made scene's."""
    abi = M.hip_abi()
    v, steps = MOVES["leaf_15_to_16"]
    (idx, listed), (_, back) = steps
    tris = mv.scene_of(v)
    assert {m["tex"] for m in tris["materials"]} >= {0, 1}  # a material names each texture
    original = [t["texels"] for t in tris["textures"]]
    a, b, c = texels_of(21, (3, 5, 3)), texels_of(22, (2, 2, 3)), texels_of(23, (7, 1, 3))
    assert len({a.shape, c.shape, original[0].shape}) == 3 and b.shape != original[1].shape
    moved = v.copy()
    moved[idx] = listed
    view = view_of(v)
    sens = binding.sensor(view[0], W, H)
    h, _ = abi.scene_create_triangles(tris)
    try:
        first = look(abi, h, view)
        abi.set_texture(h, 0, a)
        abi.scene_set_triangle_vertices(h, idx, listed)
        assert differences(look(abi, h, view), new_scene_look(abi, with_texture0(tris, a), moved, view)) == []
        abi.set_texture(h, 1, b)
        albedo_a = abi.render_gbuffer(h, sens, W, H, channels=("albedo",))["albedo"]
        abi.set_texture(h, 0, c)
        albedo_c = abi.render_gbuffer(h, sens, W, H, channels=("albedo",))["albedo"]
        assert not same(albedo_a, albedo_c), "no texel of texture 0 shows"
        abi.scene_set_triangle_vertices(h, idx, back)
        assert differences(look(abi, h, view), new_scene_look(abi, with_texture0(tris, c, b), v, view)) == []
        abi.set_texture(h, 0, original[0])
        abi.set_texture(h, 1, original[1])
        last = look(abi, h, view)
        assert differences(last, new_scene_look(abi, tris, v, view)) == []
        assert differences(last, first) == []
    finally:
        abi.scene_destroy(h)


# ---- (e) no-op sets, old trees

def test_noop_set_bumps_nothing_and_a_real_move_retires_old_trees():
    abi = M.hip_abi()
    v, steps = MOVES["shuffled"]
    idx, listed = steps[0]
    tris = mv.scene_of(v)
    view = view_of(v)
    sens = binding.sensor(view[0], W, H)
    h, _ = abi.scene_create_triangles(tris)
    t = None
    try:
        abi.set_raytree_tri(h, True)
        abi.set_lights(h, view[1])
        before = look(abi, h, view)
        t, _ = abi.raytree_create(h, sens, W, H, max_depth=DEPTH)
        shaded = abi.raytree_shade(t, view[1])["rgb"]
        assert np.array_equal(shaded, before["rgb0"])
        # the live vertices again, by bits: all of them, one, none
        for ids in (np.arange(len(v)), idx, np.zeros(0, dtype=np.int32)):
            info = abi.scene_set_triangle_vertices(h, ids, v[ids])
            assert info["n_nodes"] == 0 and info["total_ms"] == 0.0
        assert abi.lib.mt_scene_set_triangle_vertices(h, None, 0, None, None) == 0
        assert np.array_equal(abi.raytree_shade(t, view[1])["rgb"], shaded)  # the tree still shades
        abi.raytree_update_materials(t)
        assert differences(look(abi, h, view), before) == []
        planes = tree_planes_plain(abi, t)
        abi.scene_set_triangle_vertices(h, idx, listed)
        rgb, st = np.zeros((H, W, 3), dtype=np.uint8), binding.mt_stats()
        col = np.zeros((H, W, 3))
        lights = np.asarray(view[1], dtype=np.float64)
        one = np.zeros(1, dtype=np.int32)
        calls = (lambda: abi.lib.mt_raytree_shade(t, lights.ctypes.data, len(lights), rgb.ctypes.data, C.addressof(st)),
                 lambda: abi.lib.mt_raytree_shade_colors(t, lights.ctypes.data, len(lights), col.ctypes.data, C.addressof(st)),
                 lambda: abi.lib.mt_raytree_update_lights(t, one.ctypes.data, 1, C.addressof(st)),
                 lambda: abi.lib.mt_raytree_update_materials(t, C.addressof(st)),
                 lambda: abi.lib.mt_raytree_regrow_materials(t, None, C.addressof(st)))
        for call in calls:
            assert call() == MT_ERR_ARG
            assert "triangles were moved" in abi.last_error() and "destroy the tree" in abi.last_error()
        # ... also once the materials are stale too: the geometry check stands before that one
        mats = [dict(values=m["values"] * 0.5, tex=m["tex"]) for m in mv.MATERIALS]
        abi.set_materials(h, mats)
        for call in calls:
            assert call() == MT_ERR_ARG and "triangles were moved" in abi.last_error()
        now = tree_planes_plain(abi, t)
        assert sorted(now) == sorted(planes) and all(same(now[k], planes[k]) for k in planes)
        assert abi.raytree_info(t)["n_layers"] >= 1
        abi.raytree_destroy(t)
        t = None
        # a new tree shades the moved scene's frame
        abi.set_materials(h, mv.MATERIALS)
        t, _ = abi.raytree_create(h, sens, W, H, max_depth=DEPTH)
        frame = abi.render_chunk(h, sens, W, H, max_depth=DEPTH)["rgb"]
        assert np.array_equal(abi.raytree_shade(t, view[1])["rgb"], frame) and not np.array_equal(frame, before["rgb0"])
    finally:
        if t:
            abi.raytree_destroy(t)
        abi.scene_destroy(h)


def tree_planes_plain(abi, t):
    info = abi.raytree_info(t)
    out = {}
    for k in range(info["n_layers"]):
        for name, a in abi.raytree_read_layer(t, k).items():
            out["%d_%s" % (k, name)] = a
        out["%d_tri" % k] = abi.raytree_read_tri(t, k)
    return out


# ---- (f) refusals leave the scene as it was

def test_depth_refusal_leaves_the_scene_as_it_was():
    abi = M.hip_abi()
    v, idx, listed = mv.never_separate_move()
    tris = mv.scene_of(v)
    view = view_of(v)
    h, _ = abi.scene_create_triangles(tris)
    try:
        before = look(abi, h, view)
        for _ in range(2):
            info = binding.mt_build_info()
            rc = abi.lib.mt_scene_set_triangle_vertices(h, idx.ctypes.data, len(idx), listed.ctypes.data, C.byref(info))
            assert rc == MT_ERR_UNSUPPORTED and abi.last_error() == DEPTH_MESSAGE
            assert differences(look(abi, h, view), before) == []
        # the next legal move works
        legal = v[idx] + np.array([0.0, 0.0, 0.125])
        abi.scene_set_triangle_vertices(h, idx, legal)
        cur = v.copy()
        cur[idx] = legal
        assert differences(look(abi, h, view), new_scene_look(abi, tris, cur, view)) == []
    finally:
        abi.scene_destroy(h)


def test_a_refused_move_after_a_texture_set_keeps_both():
    abi = M.hip_abi()
    v, idx, listed = mv.never_separate_move()
    tris = mv.scene_of(v)
    view = view_of(v)
    a, c = texels_of(21, (3, 5, 3)), texels_of(23, (7, 1, 3))
    h, _ = abi.scene_create_triangles(tris)
    try:
        abi.set_texture(h, 0, a)
        before = look(abi, h, view)
        assert differences(before, new_scene_look(abi, with_texture0(tris, a), v, view)) == []
        info = binding.mt_build_info()
        rc = abi.lib.mt_scene_set_triangle_vertices(h, idx.ctypes.data, len(idx), listed.ctypes.data, C.byref(info))
        assert rc == MT_ERR_UNSUPPORTED and abi.last_error() == DEPTH_MESSAGE
        assert differences(look(abi, h, view), before) == []  # the geometry and the new texture, both as they were
        legal = v[idx] + np.array([0.0, 0.0, 0.125])
        abi.scene_set_triangle_vertices(h, idx, legal)
        cur = v.copy()
        cur[idx] = legal
        assert differences(look(abi, h, view), new_scene_look(abi, with_texture0(tris, a), cur, view)) == []
        abi.set_texture(h, 0, c)
        assert differences(look(abi, h, view), new_scene_look(abi, with_texture0(tris, c), cur, view)) == []
    finally:
        abi.scene_destroy(h)


def test_argument_checks_in_their_documented_order():
    abi = M.hip_abi()
    v = MOVES["n16"][0]
    tris = mv.scene_of(v)
    view = view_of(v)
    h, _ = abi.scene_create_triangles(tris)
    # a scene made without tri_id: one empty node
    keep = [np.zeros(6), np.zeros(3), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)]
    d = binding.mt_scene_desc()
    d.struct_size, d.abi_version, d.n_nodes, d.tree_depth = C.sizeof(binding.mt_scene_desc), binding.MT_ABI_VERSION, 1, 1
    d.node_aabb, d.node_center, d.node_first_child, d.node_prim_begin, d.node_prim_count = (k.ctypes.data for k in keep)
    bare = abi.lib.mt_scene_create(C.byref(d))
    assert bare, abi.last_error()
    ok = np.array([2, 0, 1], dtype=np.int32)
    outside = np.array([2, 16, 2], dtype=np.int32)
    negative = np.array([-1, 0, 0], dtype=np.int32)
    twice = np.array([1, 0, 1], dtype=np.int32)
    vs = np.zeros((16, 9))
    setter, getter = abi.lib.mt_scene_set_triangle_vertices, abi.lib.mt_scene_get_triangle_vertices
    try:
        before = look(abi, h, view)
        for args, msg in (((None, None, -1, None), "scene is NULL"),
                          ((bare, None, -1, None), "the scene was made without tri_id"),
                          ((h, None, -1, None), "-1 listed triangles for a scene of 16"),
                          ((h, None, 17, None), "17 listed triangles for a scene of 16"),
                          ((h, None, 3, None), "the index list is NULL"),
                          ((h, outside.ctypes.data, 3, None), "the vertex array is NULL"),
                          ((h, outside.ctypes.data, 3, vs.ctypes.data), "entry 1: add index 16 outside 0..15"),
                          ((h, negative.ctypes.data, 3, vs.ctypes.data), "entry 0: add index -1 outside 0..15"),
                          ((h, twice.ctypes.data, 3, vs.ctypes.data), "add index 1 is listed twice")):
            assert setter(*args, None) == MT_ERR_ARG and abi.last_error() == msg, (msg, abi.last_error())
            assert differences(look(abi, h, view), before) == [], msg
        for args, msg in (((None, None, 3), "scene is NULL"), ((bare, None, 3), "the scene was made without tri_id"),
                          ((h, None, 15), "15 triangles for a scene made with 16"), ((h, None, 16), "the output array is NULL")):
            assert getter(*args) == MT_ERR_ARG and abi.last_error() == msg, (msg, abi.last_error())
        assert setter(bare, None, 0, None, None) == MT_ERR_ARG  # (no tri_id comes before the empty list)
        assert setter(h, ok.ctypes.data, 3, v[ok].ctypes.data, None) == 0  # accepted: the live vertices, a no-op
        assert differences(look(abi, h, view), before) == []
    finally:
        abi.lib.mt_scene_destroy(bare)
        abi.scene_destroy(h)


def test_a_tri_id_that_is_no_permutation_is_refused():
    """mt_scene_create takes the caller's tri_id unchecked; the move's kernels scatter through it, so the first set
    checks it on the host: MT_ERR_ARG before any device call, the scene as it was."""
    abi = M.hip_abi()
    v, steps = MOVES["n16"]
    h0, _ = abi.scene_create_triangles(mv.scene_of(v))
    tree = abi.scene_read_tree(h0)
    abi.scene_destroy(h0)
    ids = tree["tri_id"]
    tris = mv.scene_of(v)
    flat = dict(tree_depth=tree["depth"], node_aabb=tree["node_aabb"], node_center=tree["node_center"],
                node_first_child=tree["first_child"], node_prim_begin=tree["prim_begin"], node_prim_count=tree["prim_count"],
                tri_aabb=tree["tri_aabb"][ids], materials=tris["materials"], textures=tris["textures"])
    for k in ("tri_vertex", "tri_normal", "tri_uvw", "tri_material", "tri_line_no"):
        flat[k] = tris[k][ids]
    view = view_of(v)
    idx, listed = steps[0]
    for bad in (np.where(ids == ids[3], ids[4], ids), np.where(ids == ids[3], 16, ids), np.where(ids == ids[3], -1, ids)):
        flat["tri_id"] = bad.astype(np.int32)
        h = abi.scene_create(flat)
        try:
            sens = binding.sensor(view[0], W, H)
            abi.set_lights(h, view[1])
            before = abi.render_chunk(h, sens, W, H, max_depth=DEPTH)["rgb"]
            for _ in range(2):
                with pytest.raises(RuntimeError, match="the scene's tri_id is no permutation of its triangles"):
                    abi.scene_set_triangle_vertices(h, idx, listed)
            assert np.array_equal(abi.render_chunk(h, sens, W, H, max_depth=DEPTH)["rgb"], before)
        finally:
            abi.scene_destroy(h)
    # ... and with the build's own tri_id the same description moves like the scene made from triangles
    flat["tri_id"] = ids
    h = abi.scene_create(flat)
    try:
        abi.scene_set_triangle_vertices(h, idx, listed)
        cur = v.copy()
        cur[idx] = listed
        assert differences(look(abi, h, view), new_scene_look(abi, tris, cur, view)) == []
    finally:
        abi.scene_destroy(h)


# ---- (g) the other calls of the contract

def test_other_calls_after_a_move():
    """Supersampled and adaptive frames, replicas of a multi-GPU frame, ray trees, ray lists and closest hits."""
    abi = M.hip_abi()
    v, steps = MOVES["shuffled"]
    idx, listed = steps[0]
    tris = mv.scene_of(v)
    cur = v.copy()
    cur[idx] = listed
    view = view_of(v)
    sens, sens2 = binding.sensor(view[0], W, H), binding.sensor(view[0], 2 * W, 2 * H)
    rng = np.random.RandomState(9)
    rays = np.concatenate([np.tile(view[0][:3], (256, 1)), rng.random_sample((256, 3)) - np.array([0.5, 0.5, -1.0])], axis=1)

    def tiled(h):
        """The tile form (every second 16 x 16 tile from tile 1) and the tile-list form (a list against the grid's
        order), each blitted into a frame of its own; the tiles not rendered stay zero."""
        import torch
        from mythtracer_amd import tiling
        vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        T = 16
        out = {}
        first, stride, n = tiling.rank_tiles(W, H, T, T, 1, 2)
        slots = torch.zeros(n * tiling.slot_bytes(T, T), dtype=torch.uint8, device="cuda")
        frame = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        abi.render_tiles_device(h, sens, W, H, T, T, first, stride, n, DEPTH, vp(slots))
        abi.blit_tiles_device(h, W, H, T, T, first, stride, n, vp(slots), vp(frame))
        torch.cuda.synchronize()
        out["tiles"] = frame.cpu().numpy()
        tiles = [11, 0, 5, 6, 2]
        lst = torch.tensor(tiles, dtype=torch.int32, device="cuda")
        slots = torch.zeros(len(tiles) * tiling.slot_bytes(T, T), dtype=torch.uint8, device="cuda")
        frame = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        abi.render_tile_list_device(h, sens, W, H, T, T, vp(lst), len(tiles), 7, DEPTH, vp(slots))
        abi.blit_tile_list_device(h, W, H, T, T, vp(lst), len(tiles), vp(slots), vp(frame))
        torch.cuda.synchronize()
        out["tile_list"] = frame.cpu().numpy()
        abi.read_stats(h)
        return out

    def calls(hs):
        h = hs[0]
        for s in hs:
            abi.set_lights(s, view[1])
            abi.set_raytree_tri(s, True)
        out = dict(ss=abi.render_chunk_ss(h, sens2, W, H, 2, max_depth=DEPTH)["rgb"])
        ad = abi.render_chunk_adaptive(h, sens, sens2, W, H, 2, 16, max_depth=DEPTH)
        out.update(adaptive=ad["rgb"], mask=ad["mask"])
        out["multi"] = abi.render_frame_multi(hs, sens, W, H, tile_w=32, tile_h=32, max_depth=DEPTH)["rgb"]
        t, st = abi.raytree_create(h, sens, W, H, max_depth=DEPTH)
        try:
            out.update({"tree_" + k: a for k, a in tree_planes_plain(abi, t).items()})
            out["tree_stats"] = counters(st)
        finally:
            abi.raytree_destroy(t)
        traced = abi.trace_rays(h, rays, max_depth=DEPTH)
        out.update(traced_color=traced["color"], traced_rgb=traced["rgb"], traced_stats=counters(traced["stats"]))
        out.update(tiled(h))
        hit = abi.intersect_rays(h, rays)
        out.update(hit_tri=hit["tri"], hit_line=hit["line"], hit_t=hit["t"], hit_point=hit["point"])
        return out

    hs = [abi.scene_create_triangles(tris)[0] for _ in range(2)]
    gs = [abi.scene_create_triangles(mv.with_vertices(tris, cur))[0] for _ in range(2)]
    try:
        before = calls(hs)
        for h in hs:
            abi.scene_set_triangle_vertices(h, idx, listed)
        got, want = calls(hs), calls(gs)
        assert (want["hit_tri"] >= 0).any() and not np.array_equal(before["ss"], want["ss"])
        assert want["tiles"].any() and want["tile_list"].any() and not np.array_equal(before["tile_list"], want["tile_list"])
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k] == want[k] if isinstance(want[k], dict) else same(got[k], want[k]), k
    finally:
        for s in hs + gs:
            abi.scene_destroy(s)


# ---- (h) the facade

@pytest.mark.parametrize("replicas", [1, 2])
def test_facade_moves_the_blue_block_in_place(replicas):
    Wf, Hf = va.W, va.H
    devices = ([0, 1] if M.hip_abi().device_count() >= 2 else [0, 0])[:replicas]
    m = M.MythTracer(tb.TWO_WAY)
    m.set_devices(devices)
    m.set_lights(va.LIGHTS)
    render = (lambda f: f.render(va.CAM, Wf, Hf, debug=True)["rgb"]) if replicas == 1 else (lambda f: f.render_image(va.CAM, Wf, Hf))
    before = render(m)
    scene_before = m.device_scene()
    idx, v = blue_block(m)
    moved = v + np.array([-45.0, 10.0, -60.0])
    m.set_triangle_vertices(idx, moved)
    m.update_geometry_in_place()
    assert m.device_scene() == scene_before  # the uploaded scene stayed
    new = moved_copy(tb.TWO_WAY, idx, moved)
    new.set_devices(devices)
    new.set_lights(va.LIGHTS)
    got, want = render(m), render(new)
    assert not np.array_equal(got, before) and np.array_equal(got, want)
    assert tb.differences(tb.host_dump(m), tb.host_dump(new)) == []
    if replicas == 1:
        a, b = m.render(va.CAM, Wf, Hf, debug=True), new.render(va.CAM, Wf, Hf, debug=True)
        assert np.array_equal(a["line"], b["line"]) and np.array_equal(a["point"], b["point"], equal_nan=True)
        assert a["counters"] == b["counters"]
    # UpdateTriangleMaterials and UpdateTriangleAttributes speak the new order
    flipped = -m.triangles()[0][idx, 9:18].reshape(-1, 3, 3)
    mirror = m.get_material("mirror")[0]
    dense = [i for i, mat in enumerate(M.MythTracer(tb.TWO_WAY).flatten()["materials"]) if np.array_equal(mat["values"], mirror)]
    assert len(dense) == 1  # (moved_copy names its materials m<index in the .obj scene's table>)
    for f in (m, new):
        f.assign_material(idx[:2], "mirror" if f is m else "m%d" % dense[0])
        f.update_triangle_materials()
        f.set_triangle_normals(idx, flipped)
        f.update_triangle_attributes()
    assert np.array_equal(render(m), render(new))
    # a second move, back
    m.set_triangle_vertices(idx, v)
    m.update_geometry_in_place()
    back = moved_copy(tb.TWO_WAY, idx, v)
    assert tb.differences(tb.host_dump(m), tb.host_dump(back)) == []


def test_update_geometry_in_place_closes_the_facades_ray_trees():
    m = M.MythTracer(tb.TWO_WAY)
    m.set_lights(va.LIGHTS)
    tree = m.raytree(va.CAM, va.W, va.H)
    idx, v = blue_block(m)
    m.set_triangle_vertices(idx, v + 1.0)
    m.update_geometry_in_place()
    with pytest.raises(RuntimeError, match="closed"):
        tree.info
    fresh = m.raytree(va.CAM, va.W, va.H)
    assert fresh.info["n_layers"] >= 1
    assert np.array_equal(fresh.shade()["rgb"], m.render(va.CAM, va.W, va.H)["rgb"])
    fresh.close()


def test_update_geometry_in_place_before_any_upload_is_update_geometry_and_prepare():
    m = M.MythTracer(tb.TWO_WAY)
    m.set_lights(va.LIGHTS)
    idx, v = blue_block(m)
    moved = v + np.array([-45.0, 10.0, -60.0])
    m.set_triangle_vertices(idx, moved)
    m.update_geometry_in_place()
    assert m.device_scene()
    new = moved_copy(tb.TWO_WAY, idx, moved)
    new.set_lights(va.LIGHTS)
    assert np.array_equal(m.render(va.CAM, va.W, va.H)["rgb"], new.render(va.CAM, va.W, va.H)["rgb"])
