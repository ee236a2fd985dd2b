"""Triangles added and removed in place, on a real MI355X (-m gpu): mt_scene_edit_triangles and
MythTracer::UpdateTrianglesInPlace (include/mythtracer_hip.h; the kernels are in mythtracer_amd/csrc/mt_build.h, the
host bookkeeping in mt_edit.h).

The bar is identity, no tolerance: after every edit the scene is compared with a scene NEWLY made by
mt_scene_create_triangles from the resulting add-order arrays -- every array of mt_scene_read_tree, a 64 x 48 depth-5
frame with its debug planes and counters, every G-buffer and light-buffer plane, every getter.  The planted edits are
tests/edit_triangles_ref.py's, which tests/test_edit_triangles_cpu.py holds to what their names promise without a GPU.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import edit_triangles_ref as ed  # noqa: E402
import move_ref as mv  # noqa: E402
import tree_build_ref as tb  # noqa: E402
import vertex_attr_ref as va  # noqa: E402

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding  # noqa: E402

EDITS = ed.edits()
W, H, DEPTH = ed.W, ed.H, ed.DEPTH
MT_ERR_ARG, MT_ERR_UNSUPPORTED = -1, -3
DEPTH_MESSAGE = "octree depth 65 exceeds MT_MAX_TREE_DEPTH 64"


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
    counters of a frame are compared between frames scheduled alike: the cost history, a forecast that an edited scene
    keeps and a new scene does not have, is switched off here on both (test_frames_after_an_edit_with_history renders
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


def view_of(tris):
    """a camera that sees the scene's finite part, from the +0.0-anchored box the root has"""
    v = tris["tri_vertex"]
    return mv.camera_for(v), mv.lights_for(v)


def new_scene_look(abi, tris, view, frames=1):
    h, _ = abi.scene_create_triangles(tris)
    try:
        return look(abi, h, view, frames)
    finally:
        abi.scene_destroy(h)


def edit(abi, h, tris, remove, add_v, seed=23):
    """One edit on the scene h whose add-order arrays are tris: (the build's info, the arrays afterwards)"""
    add = ed.added(add_v, seed=seed)
    return abi.scene_edit_triangles(h, remove, add), ed.apply(tris, remove, add)


# ---- (a) the planted edits

@pytest.mark.parametrize("name", sorted(EDITS))
def test_edited_scene_is_the_new_scene(name):
    abi = M.hip_abi()
    v, steps = EDITS[name]
    tris = mv.scene_of(v)
    cur = tris
    h, _ = abi.scene_create_triangles(tris)
    try:
        first = look(abi, h, view_of(tris))  # (frames before the edit: the scene has launch state)
        assert not any(abi.scene_move_times(h).values())  # (no move or edit yet)
        if name == "shuffled":  # the scene the frame tests render: the camera must see about what its geometry promises
            assert (first["gb_prim"] >= 0).sum() > 200 / 4.0, "the camera sees too little"
        for k, (remove, add_v) in enumerate(steps):
            info, cur = edit(abi, h, cur, remove, add_v, seed=23 + k)
            want_tree = tb.build(cur["tri_vertex"].reshape(-1, 3, 3))
            assert (info["n_nodes"], info["depth"]) == (len(want_tree["first_child"]), want_tree["depth"]), (name, k)
            assert info["total_ms"] >= info["kernel_ms"] > 0.0
            parts = abi.scene_move_times(h)  # the parts of this edit: each took time, together no more than the call
            assert sorted(parts) == ["build", "layout", "readback", "regather", "upload"] and min(parts.values()) > 0.0
            assert parts["build"] >= info["kernel_ms"] and sum(parts.values()) <= info["total_ms"]
            view = view_of(cur)
            got, want = look(abi, h, view), new_scene_look(abi, cur, view)
            assert differences(got, want) == [], (name, k)
            assert tb.differences(got["tree"], want_tree) == [], (name, k)
            assert same(got["vertices"], cur["tri_vertex"].reshape(-1, 3, 3))
        # every chain ends where it began: with the same triangles, and -- in the same order -- with the first look
        assert same(np.sort(tb.bits(cur["tri_vertex"]), axis=0), np.sort(tb.bits(tris["tri_vertex"]), axis=0))
        if name not in ed.OTHER_ORDER:
            back = dict(cur, **{k: tris[k] for k in ("tri_normal", "tri_uvw", "tri_material", "tri_line_no")})
            if all(same(cur[k], back[k]) for k in ed.PER_TRIANGLE):
                assert differences(look(abi, h, view_of(tris)), first) == []
            else:  # (re-appended triangles carry the added attributes: the geometry is the first look's)
                last = look(abi, h, view_of(tris))
                assert tb.differences(last["tree"], first["tree"]) == [] and same(last["vertices"], first["vertices"])
    finally:
        abi.scene_destroy(h)


# ---- (b) with history, on every engine

@pytest.mark.parametrize("lean", [1, 2])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("engine", [0, 1, 2, 3])
def test_frames_after_an_edit_with_history(engine, mode, lean):
    abi = M.hip_abi()
    v, steps = EDITS["shuffled"]
    remove, add_v = steps[0]
    tris = mv.scene_of(v)
    view = view_of(tris)
    sens = binding.sensor(view[0], W, H)

    def switches(h):
        abi.set_engine(h, engine)
        abi.set_traversal_mode(h, mode)
        abi.set_tuning(h, "LEAN_KERNEL", lean)
        abi.set_lights(h, view[1])

    def frames(h, n):
        return [abi.render_chunk(h, sens, W, H, max_depth=DEPTH, debug=True) for _ in range(n)]

    h, _ = abi.scene_create_triangles(tris)
    g = None
    try:
        switches(h)
        before = frames(h, 2)
        _, cur = edit(abi, h, tris, remove, add_v)
        g, _ = abi.scene_create_triangles(cur)
        switches(g)
        got, want = frames(h, 3), frames(g, 3)
        assert not np.array_equal(got[0]["rgb"], before[1]["rgb"])
        for a, b in zip(got, want):
            assert np.array_equal(a["rgb"], b["rgb"]) and np.array_equal(a["line"], b["line"]) and same(a["point"], b["point"])
    finally:
        abi.scene_destroy(h)
        if g:
            abi.scene_destroy(g)


# ---- (c) a chain of edits

def test_three_edits_in_a_row():
    abi = M.hip_abi()
    v = tb.planted()["n65"]
    rng = np.random.RandomState(11)
    tris = mv.scene_of(v)
    view = view_of(tris)
    h, _ = abi.scene_create_triangles(tris)
    try:
        cur = tris
        for k, (n_out, n_in) in enumerate(((20, 3), (7, 30), (11, 11))):
            n = len(cur["tri_material"])
            remove = rng.permutation(n)[:n_out].astype(np.int32)
            _, cur = edit(abi, h, cur, remove, tb._uniform(rng, n_in, size=0.5), seed=40 + k)
            assert len(cur["tri_material"]) == n - n_out + n_in
            assert differences(look(abi, h, view, frames=2), new_scene_look(abi, cur, view, frames=2)) == [], k
    finally:
        abi.scene_destroy(h)


# ---- (d) after other edits: the attributes follow their triangles, the stamp planes are resized

def tree_planes(abi, t, uvw=True):
    info = abi.raytree_info(t)
    out = dict(n_layers=info["n_layers"], n_rays=list(info["n_rays"]))
    for k in range(info["n_layers"]):
        for name, a in abi.raytree_read_layer(t, k).items():
            out["%d_%s" % (k, name)] = a
        out["%d_tri" % k] = abi.raytree_read_tri(t, k)
        if uvw:
            out["%d_uvw" % k] = abi.raytree_read_uvw(t, k)
    return out


def test_edit_after_other_edits_then_sets_and_a_regrow_in_the_new_order():
    abi = M.hip_abi()
    v, remove, add_v = ed.visible_edit()  # 5 out, 6 in
    n = len(v)
    tris = mv.scene_of(v)
    rng = np.random.RandomState(3)
    # the edits before, by ADD index
    mats = [dict(values=m["values"].copy(), tex=m["tex"]) for m in mv.MATERIALS]
    mats[0]["values"][0:3] = (0.2, 0.9, 0.4)
    mats[3]["tex"] = 0
    texels = rng.randint(0, 256, (3, 5, 3)).astype(np.uint8)
    edited = dict(tris, materials=mats, textures=[dict(texels=texels), tris["textures"][1]])
    edited["tri_material"] = np.roll(tris["tri_material"], 1)
    nrm = tris["tri_normal"].reshape(n, 3, 3).copy()
    nrm[::2] = nrm[::2][:, ::-1]
    uvw = tris["tri_uvw"].reshape(n, 3, 3).copy()
    uvw[1::3, :, :2] += 0.25
    edited.update(tri_normal=nrm.reshape(-1, 9), tri_uvw=uvw.reshape(-1, 9))
    view = view_of(tris)
    sens = binding.sensor(view[0], W, H)
    h, _ = abi.scene_create_triangles(tris)
    trees = []
    try:
        ids = abi.scene_read_tree(h)["tri_id"]
        abi.set_materials(h, mats)
        abi.set_texture(h, 0, texels)
        abi.set_triangle_materials(h, edited["tri_material"][ids])
        abi.set_triangle_normals(h, nrm[ids])
        abi.set_triangle_uvw(h, uvw[ids])
        _, cur = edit(abi, h, edited, remove, add_v)
        m = len(cur["tri_material"])
        assert m == n + 1
        assert differences(look(abi, h, view), new_scene_look(abi, cur, view)) == []
        ids = abi.scene_read_tree(h)["tri_id"]  # the NEW order, the new count
        assert same(abi.get_triangle_normals(h, m), cur["tri_normal"].reshape(m, 3, 3)[ids])
        assert np.array_equal(abi.get_triangle_materials(h, m), cur["tri_material"][ids])
        # the calls that speak of every triangle refuse the old count
        for call in (lambda: abi.get_triangle_normals(h, n), lambda: abi.get_triangle_uvw(h, n),
                     lambda: abi.get_triangle_materials(h, n), lambda: abi.scene_get_triangle_vertices(h, n),
                     lambda: abi.set_triangle_normals(h, nrm), lambda: abi.set_triangle_uvw(h, uvw),
                     lambda: abi.set_triangle_materials(h, edited["tri_material"])):
            with pytest.raises(RuntimeError, match="%d triangles for a scene made with %d" % (n, m)):
                call()
        with pytest.raises(RuntimeError, match="entry 0: add index %d outside 0..%d" % (m, m - 1)):
            abi.scene_set_triangle_vertices(h, [m], np.zeros((1, 3, 3)))
        # a tree with tri and uvw, normals edited in the new order (a survivor's and an added triangle's), a regrow:
        # the stamp planes have the new count, an added triangle's stamp was 0
        abi.set_raytree_tri(h, True)
        abi.set_raytree_uvw(h, True)
        abi.set_lights(h, view[1])
        t, _ = abi.raytree_create(h, sens, W, H, max_depth=DEPTH)
        trees.append(t)
        nrm2 = cur["tri_normal"].reshape(m, 3, 3).copy()
        nrm2[[3, 7, 12, m - 1, m - 4]] = [[0.0, 1.0, 0.0]] * 3
        abi.set_triangle_normals(h, nrm2[ids])
        abi.raytree_regrow(t)
        final = dict(cur, tri_normal=nrm2.reshape(-1, 9))
        g, _ = abi.scene_create_triangles(final)
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
        # a move and a reassignment in the new numbering
        idx = np.array([m - 1, 0, 5], dtype=np.int32)
        moved = final["tri_vertex"].reshape(m, 3, 3)[idx] + np.array([0.25, -0.5, 0.125])
        abi.scene_set_triangle_vertices(h, idx, moved)
        vtx = final["tri_vertex"].reshape(m, 3, 3).copy()
        vtx[idx] = moved
        mtl = np.roll(final["tri_material"], 2)
        abi.set_triangle_materials(h, mtl[abi.scene_read_tree(h)["tri_id"]])
        final = dict(final, tri_vertex=vtx.reshape(-1, 9), tri_material=mtl)
        assert differences(look(abi, h, view), new_scene_look(abi, final, view)) == []
    finally:
        for t in trees:
            abi.raytree_destroy(t)
        abi.scene_destroy(h)


def texels_of(seed, shape):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def test_textures_set_before_and_after_an_edit():
    """A texture set patches the scene's table allocations, an edit replaces its geometry allocations."""
    abi = M.hip_abi()
    v, steps = EDITS["leaf_15_to_16"]
    tris = mv.scene_of(v)
    assert {m["tex"] for m in tris["materials"]} >= {0, 1}
    a, b = texels_of(21, (3, 5, 3)), texels_of(23, (7, 1, 3))
    view = view_of(tris)
    h, _ = abi.scene_create_triangles(tris)
    try:
        abi.set_texture(h, 0, a)
        _, cur = edit(abi, h, tris, *steps[0])
        cur = dict(cur, textures=[dict(texels=a), tris["textures"][1]])
        assert differences(look(abi, h, view), new_scene_look(abi, cur, view)) == []
        abi.set_texture(h, 0, b)
        cur = dict(cur, textures=[dict(texels=b), tris["textures"][1]])
        got = look(abi, h, view)
        assert differences(got, new_scene_look(abi, cur, view)) == []
        _, cur = edit(abi, h, cur, *steps[1])
        assert differences(look(abi, h, view), new_scene_look(abi, cur, view)) == []
    finally:
        abi.scene_destroy(h)


# ---- (e) the no-op, old trees

def test_noop_changes_nothing_and_an_edit_retires_old_trees():
    abi = M.hip_abi()
    v, steps = EDITS["shuffled"]
    tris = mv.scene_of(v)
    view = view_of(tris)
    sens = binding.sensor(view[0], W, H)
    h, _ = abi.scene_create_triangles(tris)
    t = None
    try:
        abi.set_raytree_tri(h, True)
        abi.set_lights(h, view[1])
        _, cur = edit(abi, h, tris, np.array([5], dtype=np.int32), None)  # (so that the times of a last edit exist)
        before = look(abi, h, view)
        times = abi.scene_move_times(h)
        assert min(times.values()) > 0.0
        t, _ = abi.raytree_create(h, sens, W, H, max_depth=DEPTH)
        shaded = abi.raytree_shade(t, view[1])["rgb"]
        assert np.array_equal(shaded, before["rgb0"])
        for remove, add in ((None, None), ([], None), (np.zeros(0, dtype=np.int32), ed.added(np.zeros((0, 3, 3))))):
            info = abi.scene_edit_triangles(h, remove, add)
            assert info["n_nodes"] == 0 and info["total_ms"] == 0.0
        assert abi.lib.mt_scene_edit_triangles(h, None, 0, 0, None, None, None, None, None, None) == 0
        assert abi.scene_move_times(h) == times
        # the generations are seen through a tree: it still shades (the geometry generation is its own) and it is not
        # stale (the material, texture, assignment and attribute generations are)
        assert np.array_equal(abi.raytree_shade(t, view[1])["rgb"], shaded)
        abi.raytree_update_materials(t)
        assert differences(look(abi, h, view), before) == []
        planes = tree_planes(abi, t, uvw=False)
        # removing a triangle and adding an identical one renumbers: an edit
        last = len(cur["tri_material"]) - 1
        again = {k: cur[k][[0]] for k in ed.PER_TRIANGLE}
        abi.scene_edit_triangles(h, [0], again)
        cur = ed.apply(cur, [0], again)
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
        now = tree_planes(abi, t, uvw=False)  # still readable, and destroyable
        assert sorted(now) == sorted(planes) and all(
            now[k] == planes[k] if isinstance(planes[k], (int, list)) else same(now[k], planes[k]) for k in planes)
        abi.raytree_destroy(t)
        t = None
        got = look(abi, h, view)
        assert differences(got, new_scene_look(abi, cur, view)) == []
        assert got["tree"]["tri_id"].max() == last and same(got["rgb0"], before["rgb0"])  # the same triangles, renumbered
        # a new tree shades the edited scene's frame
        t, _ = abi.raytree_create(h, sens, W, H, max_depth=DEPTH)
        assert np.array_equal(abi.raytree_shade(t, view[1])["rgb"], got["rgb0"])
    finally:
        if t:
            abi.raytree_destroy(t)
        abi.scene_destroy(h)


# ---- (f) refusals leave the scene as it was

def test_depth_refusal_leaves_the_scene_as_it_was():
    abi = M.hip_abi()
    v, add_v = ed.never_separate_edit()
    tris = mv.scene_of(v)
    view = view_of(tris)
    add = ed.added(add_v)
    ptr = [add[k].ctypes.data for k in ed.PER_TRIANGLE]
    h, _ = abi.scene_create_triangles(tris)
    try:
        before = look(abi, h, view)
        for _ in range(2):
            info = binding.mt_build_info()
            rc = abi.lib.mt_scene_edit_triangles(h, None, 0, len(add_v), *ptr, C.byref(info))
            assert rc == MT_ERR_UNSUPPORTED and abi.last_error() == DEPTH_MESSAGE
            assert differences(look(abi, h, view), before) == []
        # the next legal edit works
        _, cur = edit(abi, h, tris, [1], add_v + np.linspace(0.0, -0.5, 16).reshape(16, 1, 1))
        assert differences(look(abi, h, view), new_scene_look(abi, cur, view)) == []
    finally:
        abi.scene_destroy(h)


def test_argument_checks_in_their_documented_order():
    abi = M.hip_abi()
    v = tb.planted()["n16"]
    tris = mv.scene_of(v)
    view = view_of(tris)
    h, _ = abi.scene_create_triangles(tris)
    # a scene made without tri_id: one empty node; a scene of zero triangles with a tri_id
    keep = [np.zeros(6), np.zeros(3), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)]
    d = binding.mt_scene_desc()
    d.struct_size, d.abi_version, d.n_nodes, d.tree_depth = C.sizeof(binding.mt_scene_desc), binding.MT_ABI_VERSION, 1, 1
    d.node_aabb, d.node_center, d.node_first_child, d.node_prim_begin, d.node_prim_count = (k.ctypes.data for k in keep)
    bare = abi.lib.mt_scene_create(C.byref(d))
    assert bare, abi.last_error()
    d.tri_id = keep[2].ctypes.data  # (no triangle reads it)
    empty = abi.lib.mt_scene_create(C.byref(d))
    assert empty, abi.last_error()
    outside = np.array([2, 16, 2], dtype=np.int32)
    negative = np.array([-1, 0, 0], dtype=np.int32)
    twice = np.array([1, 0, 1], dtype=np.int32)
    every = np.arange(16, dtype=np.int32)
    a = np.zeros((2, 9))
    p = a.ctypes.data
    mtl_ok, mtl_high, mtl_low = (np.array(m, dtype=np.int32) for m in ((-1, 3), (0, 4), (-2, 9)))
    q, bad, low = mtl_ok.ctypes.data, mtl_high.ctypes.data, mtl_low.ctypes.data
    call = abi.lib.mt_scene_edit_triangles
    N = None
    try:
        before = look(abi, h, view)
        for args, msg in (((None, N, -1, -1, N, N, N, N, N), "scene is NULL"),
                          ((bare, N, -1, -1, N, N, N, N, N), "the scene was made without tri_id"),
                          ((empty, N, -1, -1, N, N, N, N, N), "a scene of 0 triangles cannot be edited"),
                          ((h, N, -1, -1, N, N, N, N, N), "-1 triangles to remove from a scene of 16"),
                          ((h, N, 17, -1, N, N, N, N, N), "17 triangles to remove from a scene of 16"),
                          ((h, N, 3, -1, N, N, N, N, N), "-1 triangles to add"),
                          ((h, N, 3, 2, N, N, N, N, N), "the remove list is NULL"),
                          ((h, outside.ctypes.data, 3, 2, N, N, N, N, N), "the added triangles' vertex array is NULL"),
                          ((h, outside.ctypes.data, 3, 2, p, N, N, N, N), "the added triangles' normal array is NULL"),
                          ((h, outside.ctypes.data, 3, 2, p, p, N, N, N), "the added triangles' uvw array is NULL"),
                          ((h, outside.ctypes.data, 3, 2, p, p, p, N, N), "the added triangles' material array is NULL"),
                          ((h, outside.ctypes.data, 3, 2, p, p, p, bad, N), "the added triangles' line_no array is NULL"),
                          ((h, outside.ctypes.data, 3, 2, p, p, p, bad, q), "entry 1: remove index 16 outside 0..15"),
                          ((h, negative.ctypes.data, 3, 2, p, p, p, bad, q), "entry 0: remove index -1 outside 0..15"),
                          ((h, twice.ctypes.data, 3, 2, p, p, p, bad, q), "remove index 1 is listed twice"),
                          ((h, every.ctypes.data, 16, 0, N, N, N, N, N), "the edit leaves 0 triangles: a scene holds 1..2147483647"),
                          ((h, N, 0, 0x7fffffff, p, p, p, bad, q), "the edit leaves 2147483663 triangles: a scene holds 1..2147483647"),
                          ((h, every.ctypes.data, 3, 2, p, p, p, bad, q), "triangle 1: material index 4 outside -1..3"),
                          ((h, every.ctypes.data, 3, 2, p, p, p, low, q), "triangle 0: material index -2 outside -1..3")):
            assert call(*args, None) == MT_ERR_ARG and abi.last_error() == msg, (msg, abi.last_error())
            assert differences(look(abi, h, view), before) == [], msg
        assert call(bare, N, 0, 0, N, N, N, N, N, None) == MT_ERR_ARG  # (no tri_id comes before the no-op)
        assert call(empty, N, 0, 0, N, N, N, N, N, None) == MT_ERR_ARG  # (and so does the empty scene)
        assert call(h, N, 0, 0, N, N, N, N, N, None) == 0  # accepted: the no-op
        assert differences(look(abi, h, view), before) == []
    finally:
        abi.lib.mt_scene_destroy(bare)
        abi.lib.mt_scene_destroy(empty)
        abi.scene_destroy(h)


def test_a_tri_id_that_is_no_permutation_is_refused():
    """mt_scene_create takes the caller's tri_id unchecked; the edit's kernels scatter through it, so the first edit (or
    move) checks it on the host: MT_ERR_ARG before any device call, the scene as it was."""
    abi = M.hip_abi()
    v = tb.planted()["n16"]
    tris = mv.scene_of(v)
    h0, _ = abi.scene_create_triangles(tris)
    tree = abi.scene_read_tree(h0)
    abi.scene_destroy(h0)
    ids = tree["tri_id"]
    flat = dict(tree_depth=tree["depth"], node_aabb=tree["node_aabb"], node_center=tree["node_center"],
                node_first_child=tree["first_child"], node_prim_begin=tree["prim_begin"], node_prim_count=tree["prim_count"],
                tri_aabb=tree["tri_aabb"][ids], materials=tris["materials"], textures=tris["textures"])
    for k in ed.PER_TRIANGLE:
        flat[k] = tris[k][ids]
    view = view_of(tris)
    sens = binding.sensor(view[0], W, H)
    flat["tri_id"] = np.where(ids == ids[3], ids[4], ids).astype(np.int32)
    h = abi.scene_create(flat)
    try:
        abi.set_lights(h, view[1])
        before = abi.render_chunk(h, sens, W, H, max_depth=DEPTH)["rgb"]
        for _ in range(2):
            with pytest.raises(RuntimeError, match="the scene's tri_id is no permutation of its triangles"):
                abi.scene_edit_triangles(h, [2], None)
        assert np.array_equal(abi.render_chunk(h, sens, W, H, max_depth=DEPTH)["rgb"], before)
    finally:
        abi.scene_destroy(h)
    # ... and with the build's own tri_id the same description is edited like the scene made from triangles
    flat["tri_id"] = ids
    h = abi.scene_create(flat)
    try:
        _, cur = edit(abi, h, tris, [2, 9], tb._uniform(np.random.RandomState(2), 3))
        assert differences(look(abi, h, view), new_scene_look(abi, cur, view)) == []
    finally:
        abi.scene_destroy(h)


# ---- (g) the other calls of the contract

def test_other_calls_after_an_edit():
    """Supersampled and adaptive frames, replicas of a multi-GPU frame, tiles and tile lists, ray trees, ray lists and
    closest hits."""
    abi = M.hip_abi()
    v, steps = EDITS["shuffled"]
    remove, add_v = steps[0]
    tris = mv.scene_of(v)
    add = ed.added(add_v)
    cur = ed.apply(tris, remove, add)
    view = view_of(tris)
    sens, sens2 = binding.sensor(view[0], W, H), binding.sensor(view[0], 2 * W, 2 * H)
    rng = np.random.RandomState(9)
    rays = np.concatenate([np.tile(view[0][:3], (256, 1)), rng.random_sample((256, 3)) - np.array([0.5, 0.5, -1.0])], axis=1)

    def tiled(h):
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
            out.update({"tree_%s" % k: a for k, a in tree_planes(abi, t, uvw=False).items()})
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
    gs = [abi.scene_create_triangles(cur)[0] for _ in range(2)]
    try:
        before = calls(hs)
        for h in hs:
            abi.scene_edit_triangles(h, remove, add)
        got, want = calls(hs), calls(gs)
        assert (want["hit_tri"] >= 0).any() and not np.array_equal(before["ss"], want["ss"])
        assert want["tiles"].any() and want["tile_list"].any() and not np.array_equal(before["tile_list"], want["tile_list"])
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k] == want[k] if isinstance(want[k], (dict, int, list)) else same(got[k], want[k]), k
    finally:
        for s in hs + gs:
            abi.scene_destroy(s)


# ---- (h) the facade

def block_of(m):
    """(add indices, vertices, normals, uvw -- each (k, 3, 3)) of two_way.obj's blue block (x 170..230, y 0..120,
    z 250..300), whose material is `blue`"""
    data, _, _ = m.triangles()
    box = data[:, 27:33]
    inside = ((box[:, :3] >= (170.0, 0.0, 250.0)) & (box[:, 3:] <= (230.0, 120.0, 300.0))).all(axis=1)
    idx = np.nonzero(inside)[0].astype(np.int32)
    assert 2 <= len(idx) < len(data)
    return (idx,) + tuple(data[idx, 9 * k:9 * k + 9].reshape(-1, 3, 3).copy() for k in range(3))


@pytest.mark.parametrize("replicas", [1, 2])
def test_facade_adds_a_block_and_removes_it(replicas):
    Wf, Hf = va.W, va.H
    devices = ([0, 1] if M.hip_abi().device_count() >= 2 else [0, 0])[:replicas]
    render = (lambda f: f.render(va.CAM, Wf, Hf, debug=True)["rgb"]) if replicas == 1 else (lambda f: f.render_image(va.CAM, Wf, Hf))

    def facade():
        f = M.MythTracer(tb.TWO_WAY)
        f.set_devices(devices)
        f.set_lights(va.LIGHTS)
        return f

    m = facade()
    before = render(m)
    scene_before = m.device_scene()
    idx, v, nrm, uvw = block_of(m)
    n = m.triangles()[0].shape[0]
    shifted = v + np.array([-45.0, 10.0, -60.0])
    with pytest.raises(RuntimeError, match="no material named nothing"):
        m.add_triangles(shifted, nrm, uvw, material="nothing")
    # the refusals of the one-batch rule
    m.add_triangles(shifted, nrm, uvw, material="blue", line_no=7000)
    with pytest.raises(RuntimeError, match="update"):
        m.remove_triangles(idx)  # a removal after an addition: its indices would not be the uploaded scene's
    with pytest.raises(RuntimeError, match="pending"):
        m.set_triangle_vertices(idx, shifted)
    m.update_triangles_in_place()
    assert m.device_scene() == scene_before  # the uploaded scene stayed
    assert m.triangles()[0].shape[0] == n + len(idx)
    # a facade that holds the same triangles from the start
    new = facade()
    new.add_triangles(shifted, nrm, uvw, material="blue", line_no=7000)
    got, want = render(m), render(new)
    assert not np.array_equal(got, before) and np.array_equal(got, want)
    assert tb.differences(tb.host_dump(m), tb.host_dump(new)) == []
    if replicas == 1:
        a, b = m.render(va.CAM, Wf, Hf, debug=True), new.render(va.CAM, Wf, Hf, debug=True)
        assert np.array_equal(a["line"], b["line"]) and np.array_equal(a["point"], b["point"], equal_nan=True)
        assert a["counters"] == b["counters"]
    # UpdateTriangleAttributes speaks the new order: the added block's normals flipped
    block = np.arange(n, n + len(idx), dtype=np.int32)
    flipped = -m.triangles()[0][block, 9:18].reshape(-1, 3, 3)
    for f in (m, new):
        f.set_triangle_normals(block, flipped)
        f.update_triangle_attributes()
    assert np.array_equal(render(m), render(new))
    # the block removed again: the first frame; a second removal before the update is refused, and moves wait
    m.remove_triangles(block)
    with pytest.raises(RuntimeError, match="update"):
        m.remove_triangles(idx)
    m.update_triangles_in_place()
    assert m.device_scene() == scene_before and m.triangles()[0].shape[0] == n
    assert np.array_equal(render(m), before)
    assert tb.differences(tb.host_dump(m), tb.host_dump(facade())) == []
    # moves pending: the edit's update names the move's
    m.set_triangle_vertices(idx, shifted)
    with pytest.raises(RuntimeError, match="UpdateGeometryInPlace"):
        m.update_triangles_in_place()
    m.update_geometry_in_place()
    # remove and add in one update: the moved block out, the original in
    m.remove_triangles(idx)
    m.add_triangles(v, nrm, uvw, material="blue", line_no=7000)
    m.update_triangles_in_place()
    assert np.array_equal(render(m), before)


def test_update_triangles_in_place_closes_the_facades_ray_trees_and_works_before_any_upload():
    m = M.MythTracer(tb.TWO_WAY)
    m.set_lights(va.LIGHTS)
    idx, v, nrm, uvw = block_of(m)
    m.add_triangles(v + 1.0, nrm, uvw, material="blue", line_no=1)
    m.update_triangles_in_place()  # nothing uploaded yet: UpdateGeometry() + Prepare()
    assert m.device_scene()
    tree = m.raytree(va.CAM, va.W, va.H)
    m.remove_triangles(idx)
    m.update_triangles_in_place()
    with pytest.raises(RuntimeError, match="closed"):
        tree.info
    fresh = m.raytree(va.CAM, va.W, va.H)
    assert fresh.info["n_layers"] >= 1
    assert np.array_equal(fresh.shade()["rgb"], m.render(va.CAM, va.W, va.H)["rgb"])
    fresh.close()


def test_moves_and_a_batch_are_never_pending_together():
    """A removal renumbers the triangles that moved indices name, so neither may wait for the other's update; and while a
    batch is pending the flat tree describes the old triangles, so nothing reads it."""
    m = M.MythTracer(tb.TWO_WAY)
    m.set_lights(va.LIGHTS)
    before = m.render(va.CAM, va.W, va.H)["rgb"]
    idx, v, nrm, uvw = block_of(m)
    n = m.triangles()[0].shape[0]
    assert idx[0] > 0
    # moves pending: no batch may begin (the reviewer's sequence ends at its second step)
    m.set_triangle_vertices(idx[-1:], v[-1:] + 1.0)
    with pytest.raises(RuntimeError, match="UpdateGeometryInPlace"):
        m.remove_triangles([0])
    with pytest.raises(RuntimeError, match="UpdateGeometryInPlace"):
        m.add_triangles(v, nrm, uvw, material="blue")
    with pytest.raises(RuntimeError, match="UpdateGeometryInPlace"):
        m.update_triangles_in_place()
    assert m.triangles()[0].shape[0] == n  # nothing was removed or added
    m.set_triangle_vertices(idx[-1:], v[-1:])
    m.update_geometry_in_place()
    assert np.array_equal(m.render(va.CAM, va.W, va.H)["rgb"], before)
    # a batch pending: no move, no update of moves, no reader of the flat tree
    m.remove_triangles([0])
    for call, what in ((lambda: m.update_geometry_in_place(), "UpdateTrianglesInPlace"),
                       (lambda: m.set_triangle_vertices(idx[-1:] - 1, v[-1:]), "UpdateTrianglesInPlace"),
                       (lambda: m.update_triangle_materials(), "UpdateTrianglesInPlace"),
                       (lambda: m.update_triangle_attributes(), "UpdateTrianglesInPlace"),
                       (lambda: m.flatten(), "UpdateTrianglesInPlace"), (lambda: m.tree(), "UpdateTrianglesInPlace")):
        with pytest.raises(RuntimeError, match=what):
            call()
    m.update_triangles_in_place()
    new = M.MythTracer(tb.TWO_WAY)
    new.set_lights(va.LIGHTS)
    new.remove_triangles([0])
    assert np.array_equal(m.render(va.CAM, va.W, va.H)["rgb"], new.render(va.CAM, va.W, va.H)["rgb"])
    assert tb.differences(tb.host_dump(m), tb.host_dump(new)) == [] and len(m.flatten()["tri_id"]) == n - 1


def test_before_any_upload_the_update_takes_moved_vertices_too():
    m = M.MythTracer(tb.TWO_WAY)
    m.set_lights(va.LIGHTS)
    idx, v, nrm, uvw = block_of(m)
    moved = v + np.array([-45.0, 10.0, -60.0])
    m.set_triangle_vertices(idx, moved)
    m.update_triangles_in_place()  # nothing uploaded: UpdateGeometry() + Prepare(), whatever is pending
    assert m.device_scene()
    new = M.MythTracer(tb.TWO_WAY)
    new.set_lights(va.LIGHTS)
    new.set_triangle_vertices(idx, moved)
    new.update_geometry()
    assert np.array_equal(m.render(va.CAM, va.W, va.H)["rgb"], new.render(va.CAM, va.W, va.H)["rgb"])
