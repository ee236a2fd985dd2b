"""Triangles given another material in place (mt_scene_set_triangle_materials, the `tri` plane of a ray tree and the
reassignment mt_raytree_update_materials / mt_raytree_regrow_materials take): the reassignments of the tests, the builder
of the scene VARIANTS that give the truth for them, and the restatement of the shadow-visible rule -- shared by
tests/test_assign_cpu.py, which pins every number here with the oracle alone, and tests/test_gpu_assign.py.  Test
infrastructure.

The truth for an assignment always comes from a scene BUILT with it, never from the edit call.  For frames that is the
oracle on a variant .obj whose usemtl lines were rewritten (`variant_obj`), or on a scene added triangle by triangle
(`oracle_with`: "no material" and half a quad have no usemtl spelling that keeps the faces).  For the kernel's planes it
is mt_scene_create on the flat description with tri_material replaced (`reassigned`): a variant .obj's dense material
table is in order of first use and so numbered differently.

A move is (group, face, triangle, target): the faces of the .obj under `usemtl group` -- all of them for face None, else
the face-th of the group --, of each the triangle-th of its fan (None: all), given the material `target` (None: none).
"""
import numpy as np

import material_edit_ref as me
import orclib
import raytree_ref as rr

W, H = me.W, me.H
OFF_GRID = me.OFF_GRID
LIGHTS = me.LIGHTS
CAM = rr.CAMERAS["two_way"]
DEPTHS = (0, 1, 2, 5)
TREE_A = me.TREE_A

# name -> (moves, rays per layer after at depth 5 in the whole frame, may a shadow ray see it by the rule?)
ROWS = {
    "left->right": ([("left", None, None, "right")], [5184, 4353, 1561, 229, 6, 2], False),
    "blue->mirror": ([("blue", None, None, "mirror")], [5184, 4378, 1618, 407, 66, 21], False),
    "mirror->left": ([("mirror", None, None, "left")], [5184, 4353, 1561, 229, 3], False),
    "pane->blue": ([("pane", None, None, "blue")], [5184, 3091, 1012, 167], True),
    "blue->pane": ([("blue", None, None, "pane")], [5184, 4403, 1838, 772, 310, 180], True),
    "ceiling->pane": ([("ceiling", None, None, "pane")], [5184, 4579, 1822, 229, 6, 2], True),
    "blue#2->mirror": ([("blue", 1, None, "mirror")], [5184, 4353, 1561, 292, 48, 7], False),
    "blue#2->pane": ([("blue", 1, None, "pane")], [5184, 4353, 1582, 370, 69, 15], True),
}
SAME_SHAPE = ("left->right",)
# left->right: rays whose albedo changes, per layer
LEFT_RIGHT_ALBEDO = [594, 525, 324, 0, 0, 0]
# the first layer whose ray COUNT differs from A's; for the two blue#2 rows no primary ray sees the face: layer 0 is A's
# bit for bit
FIRST_DIFFERENCE = {"blue#2->mirror": 3, "blue#2->pane": 2, "ceiling->pane": 1}
# no .obj spelling ("no material"): built through add_triangle (oracle_with) and the flat description (kernel); the
# counts are the ones tests/test_assign_cpu.py found and holds
EXTRA = {
    "mirror->none": ([("mirror", None, None, None)], [5184, 4253, 1330, 142], True),
}
# one triangle of a quad only: material_edit_ref.hidden_pane_scene (a floor quad and a pane quad above it, added as two
# triangles each; the camera sees the floor alone) with the SECOND triangle of the floor quad given the pane's material
QUAD_CAMERA, QUAD_SIZE, QUAD_LIGHTS = me.HIDDEN_CAMERA, me.HIDDEN_SIZE, me.HIDDEN_LIGHTS
QUAD_PANE_TR = 0.5
QUAD_TRIANGLE = 1           # AddPrimitive index
QUAD_A = [256]              # rays per layer at depth 5 before ...
QUAD_B = [256, 15]          # ... and after
# room_tex: the red wall given the TEXTURED floor material, in tests/test_gpu_texture_edit.py's ragged chunk
ROOM_TEX_MOVES = [("red", None, None, "floor")]
ROOM_TEX = dict(image=(96, 64), chunk=(5, 3, 61, 45), depth=3, n_lights=2)
ROOM_TEX_A = [2745, 573, 341, 129]
ROOM_TEX_B = [2745, 605, 359, 138]


def faces(obj):
    """The f lines of an .obj in file order: dicts of line (0-based, what the readers record as a triangle's line_no),
    group (the usemtl in force, None before the first) and ordinal (among the group's faces, over the whole file)."""
    out, group, seen = [], None, {}
    for no, text in enumerate(open(obj)):
        words = text.split()
        if not words:
            continue
        if words[0] == "usemtl":
            group = words[1]
        elif words[0] == "f":
            out.append(dict(line=no, group=group, ordinal=seen.get(group, 0)))
            seen[group] = seen.get(group, 0) + 1
    return out


def targets(obj, line_no, moves):
    """{AddPrimitive index: target group or None} of the triangles the moves reach; line_no = every triangle's line, by
    AddPrimitive index (a face's triangles are the ones that carry its line, in their order)."""
    line_no = np.asarray(line_no)
    by_line = {f["line"]: f for f in faces(obj)}
    assert set(line_no.tolist()) <= set(by_line), "a triangle's line is no f line of the .obj"
    out = {}
    for group, face, tri, target in moves:
        hit = False
        for f in by_line.values():
            if f["group"] != group or (face is not None and f["ordinal"] != face):
                continue
            for k, add in enumerate(np.nonzero(line_no == f["line"])[0].tolist()):
                if tri is None or tri == k:
                    out[add] = target
                    hit = True
        assert hit, "the move %r reaches no triangle" % ((group, face, tri, target),)
    return out


def add_order_lines(flat):
    """flat["tri_line_no"] (node-stream order) by AddPrimitive index."""
    out = np.zeros(len(flat["tri_id"]), dtype=np.int64)
    out[flat["tri_id"]] = flat["tri_line_no"]
    return out


def dense_index(flat, obj):
    """{group: its index in flat["materials"]} by the triangles that carry it; None -> -1."""
    group_of = {f["line"]: f["group"] for f in faces(obj)}
    out = {None: -1}
    for s in range(len(flat["tri_id"])):
        g = group_of[int(flat["tri_line_no"][s])]
        m = int(flat["tri_material"][s])
        assert out.setdefault(g, m) == m, "group %s has two materials" % g
    return out


def reassigned(flat, obj, moves):
    """flat["tri_material"] (node-stream order) with the moves applied: what mt_scene_set_triangle_materials takes and what
    the BUILT scene's description holds."""
    index = dense_index(flat, obj)
    to = targets(obj, add_order_lines(flat), moves)
    out = np.array(flat["tri_material"], dtype=np.int32)
    for s, add in enumerate(flat["tri_id"]):
        if int(add) in to:
            out[s] = index[to[int(add)]]
    return out


def built(flat, tri_material):
    """The description of a scene BUILT with the assignment: `flat` with tri_material replaced, nothing else touched."""
    out = dict(flat)
    out["tri_material"] = np.ascontiguousarray(tri_material, dtype=np.int32)
    return out


def variant_obj(obj, moves, out_dir):
    """A copy of `obj` (with its .mtl and textures) whose usemtl lines give every moved face its target: a usemtl line
    goes in front of each face whose material is not the one in force.  Whole faces and named targets only.  Returns
    the copy's path.  (Line numbers move; vertices, faces and their order do not.)"""
    assert all(tri is None and target is not None for _, _, tri, target in moves)
    out = me.variant(obj, {}, out_dir)
    by_line = {f["line"]: f for f in faces(obj)}
    lines, in_force = [], None
    for no, text in enumerate(open(obj)):
        words = text.split()
        if words and words[0] == "usemtl":
            continue  # (restated in front of the faces)
        if no in by_line:
            f = by_line[no]
            want = f["group"]
            for group, face, _, target in moves:
                if group == f["group"] and (face is None or face == f["ordinal"]):
                    want = target
            if want is not None and want != in_force:
                lines.append("usemtl %s\n" % want)
                in_force = want
        lines.append(text)
    with open(out, "w", newline="\n") as f:
        f.write("".join(lines))
    return out


def oracle_with(obj, moves):
    """An OracleScene of `obj`'s triangles, added one by one in their order with the moves applied -- the materials in
    the .obj's oracle's order, so the numbering is the loaded scene's.  Untextured scenes only."""
    src = orclib.OracleScene(obj)
    data, mtl, line = src.triangles()
    mats = src.materials()
    names = [m[0] for m in mats]
    assert all(m[2] < 0 for m in mats), "oracle_with: textured materials are not carried over"
    orc = orclib.OracleScene()
    for name, v, _ in mats:
        assert orc.add_material(name, v[0:3], v[3:6], v[6:9], ns=v[9], refl=v[10], tr=v[11], tf=v[12:15], ni=v[15]) == names.index(name)
    to = targets(obj, line, moves)
    for i in range(len(data)):
        m = int(mtl[i])
        if i in to:
            m = -1 if to[i] is None else names.index(to[i])
        orc.add_triangle(data[i, 0:9], data[i, 9:18], data[i, 18:27], mtl=m, line_no=int(line[i]))
    orc.finalize()
    return orc


def quad_scene(s, reassigned_triangle=False):
    """hidden_pane_scene added to `s` (an OracleScene or a MythTracer); reassigned_triangle: BUILT with triangle
    QUAD_TRIANGLE carrying the pane's material.  Returns (floor, pane), the materials' indices."""
    if not reassigned_triangle:
        return me.hidden_pane_scene(s, QUAD_PANE_TR)
    real = s.add_triangle
    count = [0]

    def add_triangle(v, mtl=-1, line_no=0):
        i = count[0]
        count[0] += 1
        return real(v, mtl=pane[0] if i == QUAD_TRIANGLE else mtl, line_no=line_no)
    # (the pane's index is add_material's second answer: known before the first triangle is added)
    pane = [1]
    s.add_triangle = add_triangle
    try:
        floor, p = me.hidden_pane_scene(s, QUAD_PANE_TR)
    finally:
        del s.add_triangle
    assert p == pane[0]
    return floor, p


def shadow_visible(mats_was, mats_now, pairs):
    """The rule of include/mythtracer_hip.h (mt_scene_set_raytree_tri ff.) restated: `pairs` = (a, b) per changed
    triangle, a its old material in the table `mats_was`, b its new one in `mats_now` (lists of 16 values: ka kd ks ns
    refl tr tf ni; -1 = none).  Doubles compare by their bits."""
    def bits(v):
        return np.asarray(v, dtype=np.float64).tobytes()
    for a, b in pairs:
        if a == b:
            continue
        if a < 0 or b < 0:
            return True
        va, vb = np.asarray(mats_was[a], dtype=np.float64), np.asarray(mats_now[b], dtype=np.float64)
        if bits(va[11]) != bits(vb[11]):
            return True
        if (va[11] != 0.0 or vb[11] != 0.0) and bits(va[12:15]) != bits(vb[12:15]):
            return True
    return False


def changed_pairs(was, now):
    """(a, b) of every entry where two assignments differ."""
    was, now = np.asarray(was), np.asarray(now)
    at = np.nonzero(was != now)[0]
    return list(zip(was[at].tolist(), now[at].tolist()))


def flat_values(flat):
    return [m["values"] for m in flat["materials"]]


def list_rays(n=130):
    """A ray list of n rays, n x 1 (the last wave is partial): every 40th pixel ray of the frame."""
    rays, _ = rr.layer0_rays(CAM, W, H)
    pick = (np.arange(n) * 40 + 7) % len(rays)
    return np.ascontiguousarray(rays[pick])
