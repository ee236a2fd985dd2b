"""Vertex normals and texture coordinates edited in place, the parts that need no GPU (include/mythtracer_hip.h,
mt_scene_set_triangle_normals ff. and the attribute edit the two ray-tree material calls take).

a. The symbols exist, the ABI version is still 5, the argument checks that can be reached without a device return
   MT_ERR_ARG and never MT_ERR_HIP, and the facade refuses bad input before it needs a device; its flatten() after
   set_triangle_normals / set_triangle_uvw is the flat description with exactly those triangles replaced.
b. The normal edits of tests/vertex_attr_ref.py, by the oracle alone (tests/raytree_ref.py) on two_way.obj at 96 x 54,
   the bench's lights, depth 5, whole frame and off-grid chunk: the tree of a scene BUILT with each edit has the rays per
   layer vertex_attr_ref.ROWS records; the restated dirty sets, path matching (regrow_ref's with the extra clause) and
   regrow ARE the built tree in every plane -- so a normal moves the normal plane and the reflected subtrees and nothing
   else; and what each edit is there to exercise holds, so that the GPU cases are not vacuous.
c. The uvw edits on texture_edit_ref's tiny scene: no ray count moves, the albedo of a uvw-dirty ray is ambient times
   the texel at the coordinates interpolated again from the stored point, every other plane is the old one, and the
   frame changes exactly where UVW_ROWS says (nowhere for the untextured wall).
"""
import ctypes

import numpy as np
import pytest

import material_edit_ref as me
import orclib
import raytree_ref as rr
import raytree_update_ref as ru
import regrow_ref as rg
import texture_edit_ref as te
import vertex_attr_ref as va

import mythtracer_amd as M
from mythtracer_amd import binding

MT_ERR_ARG, MT_ERR_HIP = -1, -2
W, H = va.W, va.H
SYMBOLS = ("mt_scene_set_triangle_normals", "mt_scene_set_triangle_uvw", "mt_scene_get_triangle_normals",
           "mt_scene_get_triangle_uvw", "mt_raytree_attr_info_last")


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    return native_libs


# ---- a. symbols, argument checks, facade

def test_symbols_and_abi_version():
    abi = M.hip_abi()
    assert binding.MT_ABI_VERSION == 5 == abi.lib.mt_abi_version()
    for name in SYMBOLS:
        assert name in M.HIP_SYMBOLS and getattr(abi.lib, name) is not None
    for name in ("mth_set_triangle_attr", "mth_update_triangle_attributes"):
        assert getattr(M.host_lib(), name) is not None
    for name in ("set_triangle_normals", "set_triangle_uvw", "get_triangle_normals", "get_triangle_uvw", "raytree_attr_info"):
        assert callable(getattr(abi, name))
    for name in ("set_triangle_normals", "set_triangle_uvw", "update_triangle_attributes"):
        assert callable(getattr(binding.MythTracer, name))
    assert callable(binding.RayTree.attr_info)
    assert ctypes.sizeof(binding.mt_raytree_attr_info) == 24


def test_argument_checks_come_before_any_device_call():
    abi = M.hip_abi()
    arr = np.zeros(36)
    for fn in (abi.lib.mt_scene_set_triangle_normals, abi.lib.mt_scene_set_triangle_uvw,
               abi.lib.mt_scene_get_triangle_normals, abi.lib.mt_scene_get_triangle_uvw):
        for p, n in ((arr.ctypes.data, 4), (arr.ctypes.data, 0), (None, 4), (None, 0), (arr.ctypes.data, -1)):
            rc = fn(None, p, n)  # a NULL scene: its message wins over everything about the array
            assert rc == MT_ERR_ARG and rc != MT_ERR_HIP, (rc, abi.last_error())
            assert abi.last_error() == "scene is NULL", abi.last_error()
    info = binding.mt_raytree_attr_info()
    assert abi.lib.mt_raytree_attr_info_last(None, ctypes.byref(info)) == MT_ERR_ARG
    assert abi.last_error() == "the ray tree is NULL"
    assert abi.lib.mt_raytree_attr_info_last(None, None) == MT_ERR_ARG
    assert abi.last_error() == "the ray tree is NULL"
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.set_triangle_normals(None, np.zeros((2, 3, 3)))
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.get_triangle_uvw(None, 3)
    with pytest.raises(RuntimeError, match="ray tree is NULL"):
        abi.raytree_attr_info(None)
    with pytest.raises(ValueError, match="9 doubles per triangle"):
        abi.set_triangle_uvw(None, np.zeros(10))


def test_facade_edits_the_host_triangles_and_refuses_before_it_needs_a_device():
    m = M.MythTracer(rr.TWO_WAY)
    flat = m.flatten()
    n = len(flat["tri_id"])
    with pytest.raises(RuntimeError, match="triangle index %d outside the scene's %d triangles" % (n, n)):
        m.set_triangle_normals([0, n], np.zeros((2, 3, 3)))
    with pytest.raises(RuntimeError, match="triangle index -1 outside"):
        m.set_triangle_uvw([-1], np.zeros((1, 3, 3)))
    with pytest.raises(ValueError, match="2 triangles need 18 doubles"):
        m.set_triangle_uvw([0, 1], np.zeros((1, 3, 3)))
    again = m.flatten()
    for key in ("tri_normal", "tri_uvw"):  # (the refused calls changed no triangle)
        assert ru.same_plane(np.asarray(again[key]), np.asarray(flat[key]))
    orc = orclib.OracleScene(rr.TWO_WAY)
    edit = va.two_way_edit("blue smooth", orc)
    uvw = {3: np.arange(9.0).reshape(3, 3), 0: np.full((3, 3), va.NAN)}
    m.set_triangle_normals(sorted(edit), [edit[i] for i in sorted(edit)])
    m.set_triangle_uvw(sorted(uvw), [uvw[i] for i in sorted(uvw)])
    after = m.flatten()
    assert ru.same_plane(np.asarray(after["tri_normal"], dtype=np.float64).reshape(-1, 9), va.replaced(flat, "tri_normal", edit))
    assert ru.same_plane(np.asarray(after["tri_uvw"], dtype=np.float64).reshape(-1, 9), va.replaced(flat, "tri_uvw", uvw))
    assert len(va.changed_triangles(flat["tri_normal"], after["tri_normal"])) == len(edit)
    for key in flat:
        if key not in ("tri_normal", "tri_uvw", "materials", "textures"):
            assert np.array_equal(np.asarray(after[key]), np.asarray(flat[key])), key


# ---- b. the normal edits, by the oracle alone

@pytest.fixture(scope="module")
def two_way():
    orc = orclib.OracleScene(rr.TWO_WAY)
    orc.set_lights(va.LIGHTS)
    trees = {bool(c): rr.build(orc, va.CAM, W, H, va.LIGHTS, va.DEPTH, chunk=c) for c in (None, va.OFF_GRID)}
    assert trees[False]["n_rays"] == me.TREE_A and trees[True]["n_rays"] == rg.CHUNK_A
    return orc, trees, orc.render(va.CAM, W, H)["rgb"]


def kept_refracted_under_dirty(layers_a, layers_b, src, changed):
    n = 0
    for k in range(len(layers_b) - 1):
        lb, s = layers_b[k], src[k]
        i = np.nonzero((lb["child_refr"] >= 0) & (s >= 0))[0]
        if k < len(layers_a) and len(i):
            d = va.dirty(layers_a[k]["prim"][s[i]], changed)
            n += int((src[k + 1][lb["child_refr"][i]][d] >= 0).sum())
    return n


@pytest.mark.parametrize("name", list(va.NORMAL_EDITS))
def test_normal_edit_by_the_oracle(name, two_way):
    orc_a, trees_a, frame_a = two_way
    edit = va.two_way_edit(name, orc_a)
    changed = sorted(edit)
    assert changed, "the edit reaches no triangle"
    orc_b = va.oracle_with(orc_a, normals=edit)
    orc_b.set_lights(va.LIGHTS)
    frame_b = orc_b.render(va.CAM, W, H)["rgb"]
    moved = int((frame_a != frame_b).any(axis=-1).sum())
    print("%s: triangles %s, %d pixels of the oracle's frame change" % (name, changed, moved))
    assert moved > 0
    data, _, _ = orc_a.triangles()
    normal_now = np.array(data[:, 9:18])
    for i, v in edit.items():
        normal_now[i] = np.asarray(v).reshape(9)
    for chunk in (False, True):
        a = trees_a[chunk]
        b = rr.build(orc_b, va.CAM, W, H, va.LIGHTS, va.DEPTH, chunk=va.OFF_GRID if chunk else None)
        m = va.match(a["layers"], b["layers"], changed, tri="prim")
        got = dict(n_rays=b["n_rays"], traced=m["traced"], blocked=m["blocked"], respawned=m["respawned"],
                   renormaled=m["renormaled"])
        print("%s %s: %s" % (name, "chunk" if chunk else "frame", got))
        assert got == va.ROWS[name][chunk]
        # the frame the restated tree shades to is the oracle's
        cw, ch = (va.OFF_GRID[2], va.OFF_GRID[3]) if chunk else (W, H)
        want = frame_b[va.OFF_GRID[1]:va.OFF_GRID[1] + ch, va.OFF_GRID[0]:va.OFF_GRID[0] + cw] if chunk else frame_b
        assert np.array_equal(rr.shade(orc_b, b, va.LIGHTS, cw, ch), want)
        # the restated regrow IS the built tree, in every plane
        lay = va.regrow(a["layers"], b["layers"], m["src"], data[:, 0:9], normal_now, changed, me.PLANES, tri="prim")
        for k, (g, w) in enumerate(zip(lay, b["layers"])):
            for plane in me.PLANES + ("prim",):
                assert ru.same_plane(np.asarray(g[plane]), np.asarray(w[plane])), (name, chunk, k, plane)
        # what the edit is there to exercise
        dirty = [int(va.dirty(l["prim"], changed).sum()) for l in a["layers"]]
        if name in ("mirror tilt", "pane tilt"):
            assert sum(dirty[1:]) > 0, "no dirty ray below layer 0"
        if name == "pane tilt":
            assert kept_refracted_under_dirty(a["layers"], b["layers"], m["src"], changed) > 0
            assert m["respawned"] > 0
        if name in ("blue smooth", "blue#2 tilt"):
            assert m["blocked"] == 0 and sum(m["traced"]) == 0 and m["renormaled"] > 0
        if name == "mirror tilt" and not chunk:
            assert max(m["traced"]) >= 65, "no traced list crosses the 64-ray item boundary"
            assert m["blocked"] > 0


# ---- c. the uvw edits, by the oracle alone

@pytest.fixture(scope="module")
def tiny():
    orc = te.build_tiny(orclib.OracleScene())
    orc.finalize()
    orc.set_lights(te.TINY_LIGHTS)
    w, h = te.TINY_IMAGE
    tree = rr.build(orc, te.TINY_CAMERA, w, h, te.TINY_LIGHTS, te.TINY_DEPTH)
    assert tree["n_rays"] == va.TINY_A
    return orc, tree, orc.render(te.TINY_CAMERA, w, h, max_level=te.TINY_DEPTH)["rgb"]


@pytest.mark.parametrize("name", list(va.UVW_EDITS))
def test_uvw_edit_by_the_oracle(name, tiny):
    orc_a, a, frame_a = tiny
    w, h = te.TINY_IMAGE
    edit = va.UVW_EDITS[name]()
    changed = sorted(edit)
    orc_b = va.build_tiny(orclib.OracleScene(), uvw=edit)
    orc_b.finalize()
    orc_b.set_lights(te.TINY_LIGHTS)
    b = rr.build(orc_b, te.TINY_CAMERA, w, h, te.TINY_LIGHTS, te.TINY_DEPTH)
    frame_b = orc_b.render(te.TINY_CAMERA, w, h, max_level=te.TINY_DEPTH)["rgb"]
    assert b["n_rays"] == va.TINY_A, "a uvw edit never changes the tree's shape"
    data, _, _ = orc_a.triangles()
    uvw_now = np.array(data[:, 18:27])
    for i, v in edit.items():
        uvw_now[i] = np.asarray(v).reshape(9)
    mats = orc_b.materials()
    texs = te.tiny_textures()
    got = dict(dirty=[], albedo=[], frame=int((frame_a != frame_b).any(axis=-1).sum()))
    for k, (la, lb) in enumerate(zip(a["layers"], b["layers"])):
        d = va.dirty(la["prim"], changed)
        got["dirty"].append(int(d.sum()))
        same = (np.ascontiguousarray(la["albedo"]).view(np.uint64) == np.ascontiguousarray(lb["albedo"]).view(np.uint64)).all(axis=1)
        got["albedo"].append(int((~same).sum()))
        assert not (~same & ~d).any(), "a ray that is not uvw-dirty changed its albedo"
        for plane in me.PLANES + ("prim",):
            if plane != "albedo":
                assert ru.same_plane(np.asarray(la[plane]), np.asarray(lb[plane])), (name, k, plane)
        # the restated albedo of the dirty rays: ambient, times the texel at uvw' where the material has a texture
        i = np.nonzero(d)[0]
        t = la["prim"][i]
        uvw = va.interpolate(data[t, 0:9], uvw_now[t], la["point"][i])
        want = np.array(la["albedo"][i])
        for j, ray in enumerate(i):
            _, values, tex = mats[int(la["material"][ray])]
            want[j] = values[0:3] * (te.color_at(texs[tex], uvw[j, 0], uvw[j, 1])[0] if tex >= 0 else 1.0)
        assert ru.same_plane(want, np.asarray(lb["albedo"][i])), (name, k)
    print("%s: %s" % (name, got))
    assert got == va.UVW_ROWS[name]
    assert (got["frame"] == 0) == (name in va.UVW_ONLY)
