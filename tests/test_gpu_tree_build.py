"""The octree built on the GPU, on a real MI355X (-m gpu): mt_octree_build / mt_octree_read, mt_scene_create_triangles,
mt_scene_read_tree and the facade's switch (include/mythtracer_hip.h; the kernels are in mythtracer_amd/csrc/mt_build.h).

The bar is identity, no tolerance: every array of the tree equals the host builder's (OctTree::Finalize through the
facade's dump) by bits, frames and planes equal those of a scene made from the host-built description.  The planted
inputs are tests/tree_build_ref.py's, which tests/test_tree_build_cpu.py holds to the host builder without a GPU.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import texture_edit_ref as te  # noqa: E402
import tree_build_ref as tb  # noqa: E402
import vertex_attr_ref as va  # noqa: E402

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding  # noqa: E402

PLANTED = tb.planted()
DEPTH_MESSAGE = "octree depth 65 exceeds MT_MAX_TREE_DEPTH 64"
_HOST = {}


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"


def vertices_of(name, scenes):
    if name in PLANTED:
        return PLANTED[name]
    if name == "grid16":
        return tb.grid16()
    return tb.obj_triangles(M, tb.TWO_WAY if name == "two_way" else scenes[name])


def host_tree(name, scenes):
    """(vertices, the host builder's dump), made once per input."""
    if name not in _HOST:
        v = vertices_of(name, scenes)
        _HOST[name] = (v, tb.host_dump(tb.facade_of(M, v)))
    return _HOST[name]


def device_tree(v, device=0):
    abi = M.hip_abi()
    t, info = abi.octree_build(v, device)
    try:
        out = abi.octree_read(t)
    finally:
        abi.octree_destroy(t)
    return out, info


# ---- (a) planted inputs

@pytest.mark.parametrize("name", sorted(PLANTED) + ["grid16", "two_way", "room"])
def test_device_tree_equals_the_host_builders(name, scenes):
    v, want = host_tree(name, scenes)
    got, info = device_tree(v)
    print("%s: %d triangles, %d nodes, depth %d, %d levels, kernels %.3f ms, call %.3f ms"
          % (name, len(v), info["n_nodes"], info["depth"], info["levels"], info["kernel_ms"], info["total_ms"]))
    assert tb.differences(got, want) == []
    assert (info["n_nodes"], info["depth"], info["levels"]) == (len(want["first_child"]), want["depth"], want["depth"])


def test_read_takes_any_subset_of_the_arrays():
    abi = M.hip_abi()
    v, want = host_tree("shuffled", None)
    t, _ = abi.octree_build(v)
    try:
        a = binding.mt_octree_arrays()
        ids = np.full(len(v), -1, dtype=np.int32)
        a.tri_id = ids.ctypes.data
        abi.check(abi.lib.mt_octree_read(t, C.byref(a)))
        assert (a.n_nodes, a.n_tris, a.depth) == (len(want["first_child"]), len(v), want["depth"])
        assert np.array_equal(ids, want["tri_id"])
        info = binding.mt_build_info()
        abi.check(abi.lib.mt_octree_info(t, C.byref(info)))
        assert info.n_nodes == a.n_nodes and info.kernel_ms > 0.0 and info.total_ms >= info.kernel_ms
        assert abi.lib.mt_octree_info(None, C.byref(info)) == -1 and abi.lib.mt_octree_info(t, None) == -1
        assert abi.lib.mt_octree_read(None, C.byref(a)) == -1 and abi.lib.mt_octree_read(t, None) == -1
    finally:
        abi.octree_destroy(t)
    abi.octree_destroy(None)


# ---- (b) determinism

@pytest.mark.parametrize("name", ["shuffled", "grid16"])
def test_two_builds_give_the_same_bytes(name):
    v = vertices_of(name, None)
    a, _ = device_tree(v)
    b, _ = device_tree(v)
    assert tb.differences(a, b) == []


# ---- (c) depth refusal

def test_depth_refusal_leaves_nothing_behind():
    abi = M.hip_abi()
    v = tb.never_separate()
    for _ in range(2):
        info = binding.mt_build_info()
        assert not abi.lib.mt_octree_build(0, len(v), v.ctypes.data, C.byref(info))
        assert abi.last_error() == DEPTH_MESSAGE
    with pytest.raises(RuntimeError, match=DEPTH_MESSAGE):
        abi.octree_build(v)
    # the next build works
    w, want = host_tree("n1025", None)
    assert tb.differences(device_tree(w)[0], want) == []
    # the facade, switch on: Prepare fails with the same verdict and no tree stands in its place ...
    m = tb.facade_of(M, v)
    m.set_device_tree_build(True)
    with pytest.raises(RuntimeError, match="device tree build failed: " + DEPTH_MESSAGE):
        m.prepare()
    assert len(m.tree()["first_child"]) == 0
    # ... and the host-built tree of the same triangles gets mt_scene_create's own
    with pytest.raises(RuntimeError, match="exceeds MT_MAX_TREE_DEPTH 64"):
        abi.scene_create(tb.facade_of(M, v).flatten())


def test_build_argument_checks_in_their_documented_order():
    abi = M.hip_abi()
    v = PLANTED["n16"]
    for args, msg in (((99, -1, None), "-1 triangles"), ((99, 1, None), "the triangle vertex array is NULL"),
                      ((99, 16, v.ctypes.data), "device 99 outside 0..%d" % (abi.device_count() - 1)),
                      ((-1, 0, None), "device -1 outside 0..%d" % (abi.device_count() - 1))):
        assert not abi.lib.mt_octree_build(*args, None)
        assert abi.last_error() == msg


# ---- (d) mt_scene_create_triangles

def two_way_facade():
    m = M.MythTracer(tb.TWO_WAY)
    return m, dict(cam=va.CAM, lights=va.LIGHTS)


def tiny_facade():
    m = te.build_tiny(M.MythTracer(None))
    return m, dict(cam=te.TINY_CAMERA, lights=te.TINY_LIGHTS)


def add_order(flat):
    """The triangle arrays of a flat description (stream order) in add order, with its materials and textures."""
    ids = flat["tri_id"]
    out = {}
    for k in ("tri_vertex", "tri_normal", "tri_uvw", "tri_material", "tri_line_no"):
        a = np.zeros_like(flat[k])
        a[ids] = flat[k]
        out[k] = a
    out["materials"], out["textures"] = flat["materials"], flat["textures"]
    return out


def look(abi, h, setup):
    """Everything the contract names, from scene h: the tree, a 64 x 48 frame at depth 5 with its stats, the G-buffer's
    prim plane, the getters."""
    W, H = 64, 48
    abi.set_lights(h, setup["lights"])
    sens = binding.sensor(setup["cam"], W, H)
    frame = abi.render_chunk(h, sens, W, H, max_depth=5, debug=True)
    stats = {k: v for k, v in frame["stats"].items() if not k.endswith("_ms")}
    gb = abi.render_gbuffer(h, sens, W, H, channels=["prim", "depth", "material"])
    nt = len(abi.scene_read_tree(h)["tri_id"])
    return dict(tree=abi.scene_read_tree(h), rgb=frame["rgb"], line=frame["line"], point=frame["point"], stats=stats,
                prim=gb["prim"], depth=gb["depth"], material=gb["material"],
                mtl=abi.get_triangle_materials(h, nt), normals=abi.get_triangle_normals(h, nt))


@pytest.mark.parametrize("make", [two_way_facade, tiny_facade])
def test_scene_from_triangles_is_the_host_built_scene(make):
    abi = M.hip_abi()
    m, setup = make()
    flat = m.flatten()
    h_host = abi.scene_create(flat)
    h_dev, info = abi.scene_create_triangles(add_order(flat))
    try:
        want, got = look(abi, h_host, setup), look(abi, h_dev, setup)
    finally:
        abi.scene_destroy(h_host)
        abi.scene_destroy(h_dev)
    print("%s: %d nodes, depth %d; %d rays" % (make.__name__, info["n_nodes"], info["depth"], want["stats"]["rays_primary"]))
    assert info["n_nodes"] == len(flat["node_first_child"]) and info["depth"] == flat["tree_depth"]
    assert tb.differences(got["tree"], want["tree"]) == []
    assert np.array_equal(got["tree"]["tri_id"], flat["tri_id"]) and np.array_equal(tb.bits(got["tree"]["node_aabb"]), tb.bits(flat["node_aabb"]))
    assert (want["prim"] >= 0).any() and (want["line"] >= 0).any()
    for k in ("rgb", "line", "prim", "material", "mtl"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("point", "depth", "normals"):
        assert np.array_equal(tb.bits(got[k]), tb.bits(want[k])), k
    assert got["stats"] == want["stats"]


def test_scene_from_triangles_checks_in_the_documented_order():
    abi = M.hip_abi()
    m, _ = tiny_facade()
    tris = add_order(m.flatten())
    keep = {k: np.ascontiguousarray(tris[k]) for k in ("tri_vertex", "tri_normal", "tri_uvw", "tri_material", "tri_line_no")}
    marr = abi._material_array(tris["materials"])

    def desc(**kw):
        d = binding.mt_triangle_desc()
        d.struct_size, d.abi_version, d.device = C.sizeof(binding.mt_triangle_desc), binding.MT_ABI_VERSION, 0
        d.n_tris, d.n_materials, d.n_textures = len(keep["tri_material"]), len(tris["materials"]), 0
        for k, a in keep.items():
            setattr(d, k, a.ctypes.data)
        d.materials = C.cast(marr, C.c_void_p)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def refused(d, msg):
        assert not abi.lib.mt_scene_create_triangles(None if d is None else C.byref(d), None)
        assert msg in abi.last_error(), abi.last_error()

    refused(None, "desc is NULL")
    refused(desc(struct_size=8, n_tris=-1), "mt_triangle_desc size/version mismatch")
    refused(desc(abi_version=1, n_tris=-1), "mt_triangle_desc size/version mismatch")
    refused(desc(n_materials=-1, tri_normal=None), "negative or empty counts")
    for k in keep:
        refused(desc(**{k: None, "materials": None}), "triangle arrays missing")
    refused(desc(materials=None, device=99), "material/texture arrays missing")
    refused(desc(n_textures=1, device=99), "material/texture arrays missing")
    refused(desc(device=99), "device 99 outside 0..")
    # after the build, the description's own checks are mt_scene_create's: the materials here name textures 0 and 1
    refused(desc(), "texture index")


def test_read_tree_checks():
    abi = M.hip_abi()
    a = binding.mt_octree_arrays()
    assert abi.lib.mt_scene_read_tree(None, C.byref(a)) == -1 and abi.last_error() == "scene is NULL"
    # a scene made without tri_id: one empty node
    keep = [np.zeros(6), np.zeros(3), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)]
    d = binding.mt_scene_desc()
    d.struct_size, d.abi_version, d.n_nodes, d.tree_depth = C.sizeof(binding.mt_scene_desc), binding.MT_ABI_VERSION, 1, 1
    d.node_aabb, d.node_center, d.node_first_child, d.node_prim_begin, d.node_prim_count = (k.ctypes.data for k in keep)
    h = abi.lib.mt_scene_create(C.byref(d))
    assert h, abi.last_error()
    try:
        assert abi.lib.mt_scene_read_tree(h, None) == -1 and abi.last_error() == "the mt_octree_arrays is NULL"
        assert abi.lib.mt_scene_read_tree(h, C.byref(a)) == -1 and abi.last_error() == "the scene was made without tri_id"
    finally:
        abi.scene_destroy(h)
    # ... and with: no triangles, one node
    h, info = abi.scene_create_triangles(dict(tri_vertex=np.zeros((0, 9)), tri_normal=np.zeros((0, 9)), tri_uvw=np.zeros((0, 9)),
                                              tri_material=np.zeros(0, dtype=np.int32), tri_line_no=np.zeros(0, dtype=np.int32)))
    try:
        t = abi.scene_read_tree(h)
        assert info["n_nodes"] == 1 and t["depth"] == 1 and len(t["tri_id"]) == 0 and not t["node_aabb"].any()
    finally:
        abi.scene_destroy(h)


# ---- (e) the facade

def test_switch_on_gives_the_rooms_golden_frame(scenes):
    g = np.load(os.path.join(tb.ROOT, "tests", "golden", "room_240x135.npz"), allow_pickle=False)
    W, H = (int(x) for x in g["image"])
    frames = []
    for on in (True, False):
        m = M.MythTracer(scenes["room"])
        m.set_device_tree_build(on)
        m.set_lights(g["lights"].reshape(-1, 12))
        frames.append(m.render(g["cam"], W, H, chunk=tuple(int(x) for x in g["chunk"]), debug=True))
        if on:
            assert tb.differences(tb.host_dump(m), host_tree("room", scenes)[1]) == []
    on, off = frames
    assert np.array_equal(on["rgb"], g["rgb"])
    assert np.array_equal(on["line"], g["line"]) and np.array_equal(on["point"], g["point"], equal_nan=True)
    assert np.array_equal(on["rgb"], off["rgb"]) and on["counters"] == off["counters"]


def blue_block(m):
    """The add indices and vertices of two_way.obj's blue block (x 170..230, y 0..120, z 250..300)."""
    data, _, _ = m.triangles()
    box = data[:, 27:33]
    inside = ((box[:, :3] >= (170.0, 0.0, 250.0)) & (box[:, 3:] <= (230.0, 120.0, 300.0))).all(axis=1)
    idx = np.nonzero(inside)[0].astype(np.int32)
    assert 2 <= len(idx) < len(data)
    return idx, data[idx, :9].reshape(-1, 3, 3)


def moved_copy(path, idx, vertices):
    """A facade newly loaded with the moved triangles: the .obj's triangles added again, one by one."""
    src = M.MythTracer(path)
    flat = src.flatten()
    tris = add_order(flat)
    tris["tri_vertex"][idx] = vertices.reshape(-1, 9)
    m = M.MythTracer(None)
    for i, mat in enumerate(flat["materials"]):
        v = mat["values"]
        m.add_material("m%d" % i, v[0:3], v[3:6], v[6:9], ns=v[9], refl=v[10], tr=v[11], tf=v[12:15], ni=v[15])
    for i in range(len(tris["tri_material"])):
        m.add_triangle(tris["tri_vertex"][i], tris["tri_normal"][i], tris["tri_uvw"][i], mtl=int(tris["tri_material"][i]),
                       line_no=int(tris["tri_line_no"][i]))
    return m


@pytest.mark.parametrize("on", [False, True])
def test_moved_block_renders_like_a_new_facade(on):
    W, H = va.W, va.H
    m = M.MythTracer(tb.TWO_WAY)
    m.set_device_tree_build(on)
    m.set_lights(va.LIGHTS)
    before = m.render(va.CAM, W, H, debug=True)
    idx, v = blue_block(m)
    moved = v + np.array([-45.0, 10.0, -60.0])
    m.set_triangle_vertices(idx, moved)
    m.update_geometry()
    got = m.render(va.CAM, W, H, debug=True)
    new = moved_copy(tb.TWO_WAY, idx, moved)
    new.set_lights(va.LIGHTS)
    want = new.render(va.CAM, W, H, debug=True)
    assert not np.array_equal(got["rgb"], before["rgb"])
    assert np.array_equal(got["rgb"], want["rgb"]) and np.array_equal(got["line"], want["line"])
    assert np.array_equal(got["point"], want["point"], equal_nan=True) and got["counters"] == want["counters"]
    assert tb.differences(tb.host_dump(m), tb.host_dump(new)) == []
    # two replicas (a device may be listed twice), the whole-image overload
    devices = [0, 1] if M.hip_abi().device_count() >= 2 else [0, 0]
    m.set_devices(devices)
    new.set_devices(devices)
    back = v + np.array([5.0, 0.0, 5.0])
    m.set_triangle_vertices(idx, back)
    m.update_geometry()
    new2 = moved_copy(tb.TWO_WAY, idx, back)
    new2.set_devices(devices)
    new2.set_lights(va.LIGHTS)
    assert np.array_equal(m.render_image(va.CAM, W, H), new2.render_image(va.CAM, W, H))


def test_update_geometry_closes_the_facades_ray_trees():
    m = M.MythTracer(tb.TWO_WAY)
    m.set_lights(va.LIGHTS)
    tree = m.raytree(va.CAM, va.W, va.H)
    idx, v = blue_block(m)
    m.set_triangle_vertices(idx, v + 1.0)
    m.update_geometry()
    with pytest.raises(RuntimeError, match="closed"):
        tree.info
    fresh = m.raytree(va.CAM, va.W, va.H)
    assert fresh.info["n_layers"] >= 1
    fresh.close()
