"""Vertex normals and texture coordinates edited in place (mt_scene_set_triangle_normals / _uvw, and what
mt_raytree_update_materials / mt_raytree_regrow_materials make of them for a tree that keeps tri): the edits of the tests,
the builders of the scene VARIANTS that give the truth for them, and the restatement of the dirty sets and of the regrow
-- shared by tests/test_vertex_attr_cpu.py, which pins every number here with the oracle alone, and
tests/test_gpu_vertex_attr.py.  Test infrastructure.

The truth for an edit always comes from a scene BUILT with it, never from the edit call: an OracleScene / MythTracer
filled through add_triangle(v, n, uvw, ...) with the edited arrays, or mt_scene_create on the flat description with
tri_normal / tri_uvw replaced (`built`).

An edit is {AddPrimitive index: (3, 3) array}: the triangle's three normals, or its three texture coordinates.
"""
import numpy as np

import assign_ref as ar
import material_edit_ref as me
import orclib
import raytree_ref as rr
import texture_edit_ref as te

W, H = me.W, me.H
OFF_GRID = me.OFF_GRID
LIGHTS = me.LIGHTS
CAM = rr.CAMERAS["two_way"]
DEPTH = 5
NAN = float("nan")


def _norm(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum())


# ---- normal edits on tests/scenes/two_way.obj

def groups(obj, line_no):
    """The usemtl group of every triangle, by AddPrimitive index (line_no: each triangle's line, by that index)."""
    by_line = {f["line"]: f["group"] for f in ar.faces(obj)}
    return [by_line[int(l)] for l in line_no]


def _of(group, names):
    return [i for i, g in enumerate(group) if g in names]


def _smooth(data, group):
    """blue: smooth normals pointing away from the block's centre"""
    tris = _of(group, ("blue",))
    centre = data[tris, 0:9].reshape(-1, 3).mean(axis=0)
    return {i: np.array([_norm(data[i, 3 * k:3 * k + 3] - centre) for k in range(3)]) for i in tris}


def _tilt_mirror(data, group):
    return {i: np.tile(_norm((0.05, 0.0, -1.0)), (3, 1)) for i in _of(group, ("mirror",))}


def _tilt_pane(data, group):
    out = {}
    for i in _of(group, ("pane",)):
        n = data[i, 9:18].reshape(3, 3)
        axis = np.zeros(3)
        axis[int(np.argmin(np.abs(n[0])))] = 0.05  # (across the normal)
        out[i] = np.array([_norm(n[k] + axis) for k in range(3)])
    return out


def _tilt_blue_second(data, group):
    """one triangle of an object only (two_way's mirror and pane are single triangles: the block is the object that
    has a second one)"""
    i = _of(group, ("blue",))[1]
    n = data[i, 9:18].reshape(3, 3)
    return {i: np.array([_norm(n[k] + np.array([0.05, 0.05, 0.05])) for k in range(3)])}


def _zero_floor(data, group):
    return {i: np.zeros((3, 3)) for i in _of(group, ("floor",))}


NORMAL_EDITS = {
    "blue smooth": _smooth,
    "mirror tilt": _tilt_mirror,
    "pane tilt": _tilt_pane,
    "blue#2 tilt": _tilt_blue_second,
    "floor zero": _zero_floor,
}
# name -> {chunk?: what the restatement says of A -> B at depth 5}: B's rays per layer, the rays traced per layer of B, the
# normal-dirty rays of A with a reflected child (`blocked`: non-zero = mt_raytree_update_materials refuses), the
# reflected children traced because of a dirty parent normal, the kept rays whose normal is rewritten.  False: the whole
# frame, A = material_edit_ref.TREE_A; True: the off-grid chunk, A = regrow_ref.CHUNK_A.  Found once by
# tests/test_vertex_attr_cpu.py with the oracle and held there.
ROWS = {
    "blue smooth": {False: dict(n_rays=[5184, 4353, 1561, 229, 6, 2], traced=[0, 0, 0, 0, 0, 0], blocked=0, respawned=0, renormaled=390),
                    True: dict(n_rays=[2257, 2210, 952, 120, 6, 2], traced=[0, 0, 0, 0, 0, 0], blocked=0, respawned=0, renormaled=170)},
    "mirror tilt": {False: dict(n_rays=[5184, 4353, 1580, 223], traced=[0, 100, 250, 81], blocked=357, respawned=347, renormaled=565),
                    True: dict(n_rays=[2257, 2210, 958, 117], traced=[0, 44, 37, 58], blocked=110, respawned=103, renormaled=268)},
    "pane tilt": {False: dict(n_rays=[5184, 4353, 1659, 215, 1], traced=[0, 631, 412, 48, 1], blocked=869, respawned=866, renormaled=866),
                  True: dict(n_rays=[2257, 2210, 1041, 109], traced=[0, 346, 291, 20], blocked=551, respawned=548, renormaled=548)},
    "blue#2 tilt": {False: dict(n_rays=[5184, 4353, 1561, 229, 6, 2], traced=[0, 0, 0, 0, 0, 0], blocked=0, respawned=0, renormaled=85),
                    True: dict(n_rays=[2257, 2210, 952, 120, 6, 2], traced=[0, 0, 0, 0, 0, 0], blocked=0, respawned=0, renormaled=17)},
    "floor zero": {False: dict(n_rays=[5184, 4353, 1525, 197, 6, 2], traced=[0, 109, 98, 36, 0, 0], blocked=243, respawned=243, renormaled=305),
                   True: dict(n_rays=[2257, 2210, 952, 120, 6, 2], traced=[0, 0, 0, 0, 0, 0], blocked=0, respawned=0, renormaled=4)},
}


def two_way_edit(name, orc_a):
    """The normal edit `name` of the two_way scene loaded in OracleScene `orc_a`."""
    data, _, line = orc_a.triangles()
    return NORMAL_EDITS[name](data, groups(rr.TWO_WAY, line))


def oracle_with(orc_a, normals=None, uvw=None):
    """An OracleScene of orc_a's triangles and materials, added one by one in their order with the edited normals and
    texture coordinates.  Untextured scenes only (two_way)."""
    data, mtl, line = orc_a.triangles()
    mats = orc_a.materials()
    assert all(m[2] < 0 for m in mats), "oracle_with: textured materials are not carried over"
    orc = orclib.OracleScene()
    for name, v, _ in mats:
        orc.add_material(name, v[0:3], v[3:6], v[6:9], ns=v[9], refl=v[10], tr=v[11], tf=v[12:15], ni=v[15])
    for i in range(len(data)):
        n = (normals or {}).get(i, data[i, 9:18])
        t = (uvw or {}).get(i, data[i, 18:27])
        orc.add_triangle(data[i, 0:9], np.asarray(n).reshape(9), np.asarray(t).reshape(9), mtl=int(mtl[i]), line_no=int(line[i]))
    orc.finalize()
    return orc


# ---- uvw edits on texture_edit_ref's tiny scene (AddPrimitive order: floor 0 1, wall 2 3, mirror 4 5, matte 6 7,
# pane 8 9, the NaN-uvw triangle 10, the zero-area one 11)

def _tiny_uvw(i):
    return np.array(te.tiny_triangles()[i][2], dtype=np.float64)


def _swap(t):
    return np.stack([t[:, 1] + 0.25, t[:, 0] + 0.25, t[:, 2]], axis=1)


UVW_EDITS = {
    "floor x2": lambda: {i: _tiny_uvw(i) * 2.0 for i in (0, 1)},
    "wall swap": lambda: {i: _swap(_tiny_uvw(i)) for i in (2, 3)},
    "matte": lambda: {i: _tiny_uvw(i) * 0.5 + np.array([0.125, 0.0, 0.0]) for i in (6, 7)},
    "nan swap": lambda: {10: np.array([[0.1, 0.2, 0.0], [0.9, 0.2, 0.0], [0.5, 0.8, 0.0]]), 0: np.full((3, 3), NAN)},
}
# the tiny scene's rays per layer at TINY_DEPTH (no uvw edit changes them), and per edit the uvw-dirty rays per layer,
# the rays whose albedo changes per layer and the pixels of the frame that change (tests/test_vertex_attr_cpu.py)
TINY_A = [1536, 715, 170]
UVW_ROWS = {
    "floor x2": dict(dirty=[379, 62, 0], albedo=[379, 62, 0], frame=408),
    "wall swap": dict(dirty=[359, 151, 27], albedo=[359, 151, 27], frame=536),
    "matte": dict(dirty=[385, 127, 19], albedo=[0, 0, 0], frame=0),
    "nan swap": dict(dirty=[118, 52, 0], albedo=[118, 52, 0], frame=170),
}
# the edits that change no albedo (an untextured material): only the uvw plane moves
UVW_ONLY = ("matte",)
TINY_CAMERA, TINY_IMAGE, TINY_DEPTH, TINY_LIGHTS = te.TINY_CAMERA, te.TINY_IMAGE, te.TINY_DEPTH, te.TINY_LIGHTS


def build_tiny(scene, normals=None, uvw=None):
    """texture_edit_ref.build_tiny with the edited arrays: the tiny scene BUILT with the edit."""
    real = scene.add_triangle
    count = [0]

    def add_triangle(v, n, t, mtl=-1, line_no=0):
        i = count[0]
        count[0] += 1
        return real(v, (normals or {}).get(i, n), (uvw or {}).get(i, t), mtl=mtl, line_no=line_no)
    scene.add_triangle = add_triangle
    try:
        te.build_tiny(scene)
    finally:
        del scene.add_triangle
    return scene


# ---- the flat description

def replaced(flat, key, edit):
    """flat[key] ("tri_normal" / "tri_uvw", node-stream order, (n, 9)) with the edit applied: what the set takes and
    what the BUILT scene's description holds."""
    out = np.array(flat[key], dtype=np.float64).reshape(-1, 9).copy()
    for s, add in enumerate(flat["tri_id"]):
        if int(add) in edit:
            out[s] = np.asarray(edit[int(add)], dtype=np.float64).reshape(9)
    return out


def built(flat, tri_normal=None, tri_uvw=None):
    """The description of a scene BUILT with the arrays: `flat` with them replaced, nothing else touched."""
    out = dict(flat)
    if tri_normal is not None:
        out["tri_normal"] = np.ascontiguousarray(tri_normal, dtype=np.float64).reshape(np.shape(flat["tri_normal"]))
    if tri_uvw is not None:
        out["tri_uvw"] = np.ascontiguousarray(tri_uvw, dtype=np.float64).reshape(np.shape(flat["tri_uvw"]))
    return out


def changed_triangles(was, now):
    """The triangles whose 9 doubles differ BY THEIR BITS: what tri_attr_stamp_kernel stamps."""
    a = np.ascontiguousarray(was, dtype=np.float64).reshape(-1, 9).view(np.uint64)
    b = np.ascontiguousarray(now, dtype=np.float64).reshape(-1, 9).view(np.uint64)
    return np.nonzero((a != b).any(axis=1))[0]


# ---- the restatement

def interpolate(vertex, attr, point):
    """Triangle::GetNormal / GetUVW (primitive_triangle.cc:27-40 ff.) for n points: barycentric weights by Heron areas,
    every product and sum rounded on its own in mt_shade.h's order.  vertex, attr (n, 9); point (n, 3)."""
    v = np.asarray(vertex, dtype=np.float64).reshape(-1, 3, 3)
    a_ = np.asarray(attr, dtype=np.float64).reshape(-1, 3, 3)
    p = np.asarray(point, dtype=np.float64).reshape(-1, 3)

    def dist(x, y):
        d = x - y
        return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])

    def area(a, b, c):
        s = (a + b + c) / 2.0
        sq = s * (s - a) * (s - b) * (s - c)
        return np.where(sq < 0.0, 0.0, np.sqrt(np.where(sq < 0.0, 0.0, sq)))
    with np.errstate(all="ignore"):
        a, b, c = dist(v[:, 0], v[:, 1]), dist(v[:, 1], v[:, 2]), dist(v[:, 2], v[:, 0])
        p0, p1, p2 = dist(p, v[:, 0]), dist(p, v[:, 1]), dist(p, v[:, 2])
        n0, n1, n2 = area(b, p2, p1), area(c, p0, p2), area(a, p1, p0)
        n = n0 + n1 + n2
        return (a_[:, 0] * n0[:, None] + a_[:, 1] * n1[:, None] + a_[:, 2] * n2[:, None]) / n[:, None]


def dirty(tri, changed):
    """The rays of a layer that sit on a changed triangle: tri (n,) with -1 for a miss, `changed` triangle indices in
    the same numbering."""
    tri = np.asarray(tri)
    return (tri >= 0) & np.isin(tri, np.asarray(changed))


def match(layers_a, layers_b, normal_changed, uvw_changed=(), tri="tri"):
    """regrow_ref.match with the attribute clause: a child of tree B is KEPT when its parent is kept, had a child in
    the same slot in tree A, and (the slot is the refracted one or the parent is not normal-dirty).  Layers are dicts
    with child_refl, child_refr and the triangle plane `tri`.  Returns dict(src per layer of B (-1 = traced), kept,
    traced per layer, renormaled, reuvwed = the kept rays on a changed triangle, respawned = the reflected children traced
    because of a dirty parent normal, blocked = the normal-dirty rays of A with a reflected child)."""
    src = [np.arange(len(layers_b[0][tri]), dtype=np.int64)]
    respawned = 0
    for k in range(len(layers_b) - 1):
        lb = layers_b[k]
        nxt = np.full(len(layers_b[k + 1][tri]), -1, dtype=np.int64)
        kept_dirty = np.zeros(len(lb[tri]), dtype=bool)
        has = src[k] >= 0
        if k < len(layers_a):
            kept_dirty[has] = dirty(layers_a[k][tri][src[k][has]], normal_changed)
        for slot in ("child_refl", "child_refr"):
            i = np.nonzero(lb[slot] >= 0)[0]
            s = src[k][i]
            old = np.full(len(i), -1, dtype=np.int64)
            if k < len(layers_a):
                ok = s >= 0
                old[ok] = layers_a[k][slot][s[ok]]
            if slot == "child_refl":
                respawned += int(((old >= 0) & kept_dirty[i]).sum())
                old[kept_dirty[i]] = -1
            nxt[lb[slot][i]] = old
        src.append(nxt)
    out = dict(src=src, kept=[int((s >= 0).sum()) for s in src], traced=[int((s < 0).sum()) for s in src],
               respawned=respawned, renormaled=0, reuvwed=0)
    for k, s in enumerate(src):
        if k < len(layers_a):
            t = layers_a[k][tri][s[s >= 0]]
            out["renormaled"] += int(dirty(t, normal_changed).sum())
            out["reuvwed"] += int(dirty(t, uvw_changed).sum())
    out["blocked"] = int(sum(int((dirty(l[tri], normal_changed) & (l["child_refl"] >= 0)).sum()) for l in layers_a))
    return out


def regrow(layers_a, layers_b, src, vertex, normal_now, normal_changed, planes, tri="tri"):
    """The layers the call must leave after a NORMAL edit, assembled as the call assembles them: a TRACED ray is B's; a
    KEPT ray takes every plane from A at src, but the normal of a normal-dirty one, which is interpolated again from
    A's stored point; coef and the child indices are B's.  vertex, normal_now: (n_tris, 9) in the numbering of `tri`."""
    out = []
    for k, (lb, s) in enumerate(zip(layers_b, src)):
        lay = {name: np.array(lb[name]) for name in planes}
        lay[tri] = np.array(lb[tri])
        keep = np.nonzero(s >= 0)[0]
        if len(keep):
            la = layers_a[k]
            at = s[keep]
            for name in planes:
                if name in ("coef", "child_refl", "child_refr"):
                    continue
                if name in ("power", "in_shadow"):
                    lay[name][:, keep] = la[name][:, at]
                else:
                    lay[name][keep] = la[name][at]
            lay[tri][keep] = la[tri][at]
            d = np.nonzero(dirty(la[tri][at], normal_changed))[0]
            if len(d):
                t = la[tri][at[d]]
                lay["normal"][keep[d]] = interpolate(vertex[t], normal_now[t], la["point"][at[d]])
        out.append(lay)
    return out
