"""The material edits of the edit-in-place tests (mt_scene_set_materials, mt_raytree_update_materials), the builder of
the scene VARIANTS that give the truth for them, and the restatement of the update's check pass -- shared by
tests/test_material_edit_cpu.py, which shows with the oracle alone what each edit changes in a stored tree, and
tests/test_gpu_material_edit.py.  Test infrastructure.

The truth for materials B always comes from a scene BUILT with B, never from the edit call: `variant` writes a .mtl with
the edited numbers next to a copy of the .obj.  The edited values are short decimals, so they survive the text round
trip; the flat table of that built scene is what the tests hand to mt_scene_set_materials.

An edit is {material name: {MTL keyword: number or three numbers}} with the keywords Ka Kd Ks Ns Refl Tr Tf Ni.
"""
import os
import shutil

import numpy as np

import lightbuffer_ref as lr
import raytree_ref as rr
import raytree_update_ref as ru

W, H = ru.W, ru.H
OFF_GRID = ru.OFF_GRID
CHUNKS = ru.CHUNKS
LIGHTS = lr.BENCH_LIGHTS
PLANES = ("ray", "in_object", "coef", "point", "normal", "albedo", "material", "power", "in_shadow", "child_refl", "child_refr")

COLOUR = {"left": {"Kd": (0.2, 0.3, 0.9), "Ks": (0.5, 0.5, 0.5), "Ns": 12}, "blue": {"Ka": (0.9, 0.5, 0.25)}}
MIRROR_05 = {"mirror": {"Refl": 0.5}}
PANE_TR = {"pane": {"Tr": 0.5}}
# two_way.obj: edits that keep the tree's shape at depth 5 ...
SAME_SHAPE = {
    "colour": COLOUR,
    "mirror 0.5": MIRROR_05,
    "pane refl": {"pane": {"Refl": 0.5}},
    "floor 0.2": {"floor": {"Refl": 0.2}},
    "pane Tr": PANE_TR,
    "pane Tf": {"pane": {"Tf": (0.5, 0.25, 1.0)}},
    "composite": {**COLOUR, **MIRROR_05, **PANE_TR},
}
# ... and edits that break it
SHAPE_BREAKING = {
    "mirror 0.125": {"mirror": {"Refl": 0.125}},
    "blue refl": {"blue": {"Refl": 0.25}},
    "pane opaque": {"pane": {"Tr": 0}},
}
EDITS = {**SAME_SHAPE, **SHAPE_BREAKING}
# one edit per scene of the scene contract: colours, a mirror, a pane; room_tex: Kd / Ks / Ns and the Ka of a TEXTURED material
SCENE_EDITS = {
    "two_way": SAME_SHAPE["composite"],
    "cornell": {"red": {"Ka": (0.2, 0.3, 0.9), "Kd": (0.2, 0.3, 0.9)}, "white": {"Ks": (0.5, 0.5, 0.5), "Ns": 12},
                "mirror": {"Refl": 0.5}},
    "mini": {"blue": {"Ka": (0.9, 0.5, 0.25)}, "mirror": {"Refl": 0.5}, "glass": {"Tr": 0.5, "Tf": (0.5, 0.25, 1.0)},
             "floor": {"Kd": (0.2, 0.3, 0.9), "Refl": 0.25}},
    "room_tex": {"floor": {"Ka": (0.9, 0.5, 0.25), "Kd": (0.2, 0.3, 0.9), "Ks": (0.5, 0.5, 0.5), "Ns": 12}},
}
# rays per layer of two_way's tree at 96 x 54, the bench's lights, depth 5 (tests/test_material_edit_cpu.py holds it)
TREE_A = [5184, 4353, 1561, 229, 6, 2]
# MTL keyword -> (place in the 16 values ka kd ks ns refl tr tf ni, count)
FIELDS = {"Ka": (0, 3), "Kd": (3, 3), "Ks": (6, 3), "Ns": (9, 1), "Refl": (10, 1), "Tr": (11, 1), "Tf": (12, 3), "Ni": (15, 1)}


def obj_of(scenes, name):
    return ru.obj_of(scenes, name)


def _number(v):
    return repr(float(v)) if float(v) != int(v) else str(int(v))


def edited_mtl(text, edit):
    """The text of a .mtl with `edit` applied: the keyword's line of the material's block replaced, or a new line at the
    end of the block where the material has none."""
    lines = text.split("\n")
    out, current, seen, todo = [], None, set(), {m: dict(f) for m, f in edit.items()}

    def close():
        if current in todo:
            for key, value in todo.pop(current).items():
                if key not in seen:
                    out.append("%s %s" % (key, " ".join(_number(v) for v in np.atleast_1d(value))))

    for line in lines:
        words = line.split()
        if words and words[0] == "newmtl":
            close()
            current, seen = words[1], set()
        elif words and current in todo and words[0] in todo[current]:
            value = todo[current][words[0]]
            line = "%s %s" % (words[0], " ".join(_number(v) for v in np.atleast_1d(value)))
            seen.add(words[0])
        out.append(line)
    if out and out[-1] == "":  # (the block's new lines go before the text's final newline)
        out.pop()
        close()
        out.append("")
    else:
        close()
    assert not todo, "no material named %s" % ", ".join(todo)
    return "\n".join(out)


def variant(obj, edit, out_dir):
    """A scene BUILT with the edited materials: a copy of `obj` in out_dir next to its .mtl with `edit` applied and the
    texture files the .mtl names.  Returns the copy's path."""
    src = os.path.dirname(os.path.abspath(obj))
    os.makedirs(out_dir, exist_ok=True)
    mtllib = [l.split()[1] for l in open(obj) if l.startswith("mtllib ")]
    assert len(mtllib) == 1, mtllib
    out = os.path.join(out_dir, os.path.basename(obj))
    shutil.copyfile(obj, out)
    text = open(os.path.join(src, mtllib[0])).read()
    for line in text.split("\n"):
        words = line.split()
        if words and words[0].startswith("map_"):
            shutil.copyfile(os.path.join(src, words[-1]), os.path.join(out_dir, words[-1]))
    with open(os.path.join(out_dir, mtllib[0]), "w", newline="\n") as f:
        f.write(edited_mtl(text, edit))
    return out


def expected_values(values, fields):
    """A material's 16 values with an edit's fields in place."""
    v = np.array(values, dtype=np.float64)
    for key, value in fields.items():
        at, k = FIELDS[key]
        v[at:at + k] = np.atleast_1d(np.asarray(value, dtype=np.float64))
    return v


def check_variant(mats_a, mats_b, edit):
    """OracleScene.materials() of a scene and of its variant: the variant holds the edit's numbers and nothing else
    moved."""
    assert [m[0] for m in mats_a] == [m[0] for m in mats_b]
    for (name, va, ta), (_, vb, tb) in zip(mats_a, mats_b):
        assert ta == tb
        assert np.array_equal(vb, expected_values(va, edit.get(name, {}))), name
    assert set(edit) <= {m[0] for m in mats_a}


def differing_entries(a, b, plane):
    """Entries of a plane (doubles or bytes, every channel and light counted) that differ between two restated layers,
    NaN = NaN."""
    x, y = np.asarray(a[plane]), np.asarray(b[plane])
    assert x.shape == y.shape, (plane, x.shape, y.shape)
    if x.dtype == np.float64:
        return int(((x.view(np.uint64) != y.view(np.uint64)) & ~(np.isnan(x) & np.isnan(y))).sum())
    return int((x != y).sum())


def diff_table(tree_a, tree_b):
    """{plane: [differing entries per layer]} for the planes that differ at all, of two restated trees of one shape."""
    assert tree_a["n_rays"] == tree_b["n_rays"]
    out = {}
    for plane in PLANES:
        per = [differing_entries(a, b, plane) for a, b in zip(tree_a["layers"], tree_b["layers"])]
        if any(per):
            out[plane] = per
    return out


def check_pass(tree, mats_b):
    """mt::raytree_recoef_kernel restated over a restated tree (materials in the ORACLE's numbering, mats_b =
    OracleScene.materials() of the variant): every ray's coefficient under B carried down the tree, the child conditions
    under B compared with the children the tree has.  dict(count = rays whose conditions differ, first = the lowest
    (layer, ray) among them or None, coef = the new coefficients per layer)."""
    count, first, coefs = 0, None, []
    c = tree["layers"][0]["coef"].copy()
    for k, lay in enumerate(tree["layers"]):
        n = len(c)
        coefs.append(c)
        lit = ~np.isnan(lay["point"][:, 0]) & (lay["material"] >= 0) & (lay["material"] < len(mats_b))
        values = np.array([mats_b[m][1] if l else np.zeros(16) for m, l in zip(lay["material"], lit)]).reshape(n, 16)
        reflectance, transparency = values[:, 10], values[:, 11]
        deeper = k < tree["max_depth"]
        refl = lit & deeper & (reflectance > 0.0) & (c > 0.01) & (lay["in_object"] == 0)
        refr = lit & deeper & (transparency > 0.0)
        bad = np.nonzero((refl != (lay["child_refl"] >= 0)) | (refr != (lay["child_refr"] >= 0)))[0]
        count += len(bad)
        if len(bad) and first is None:
            first = (k, int(bad[0]))
        if k + 1 == len(tree["layers"]):
            break
        nxt = np.zeros(len(tree["layers"][k + 1]["coef"]))
        i = np.nonzero(lay["child_refl"] >= 0)[0]
        nxt[lay["child_refl"][i]] = c[i] * reflectance[i]
        i = np.nonzero(lay["child_refr"] >= 0)[0]
        nxt[lay["child_refr"][i]] = c[i]
        c = nxt
    return dict(count=count, first=first, coef=coefs)


def same_shape(tree_a, tree_b):
    return tree_a["n_rays"] == tree_b["n_rays"] and all(
        np.array_equal(a[p], b[p]) for a, b in zip(tree_a["layers"], tree_b["layers"]) for p in ("child_refl", "child_refr"))


# ---- a pane no ray of the tree hits but a shadow ray crosses, built programmatically
# A floor patch (y = 0), a light above it and a horizontal pane between the two; the camera stands low in front of the
# patch with a narrow view pitched down, so that every ray of it goes down to the floor, into and around the pane's
# shadow, and none up to the pane.
HIDDEN_CAMERA = (50.0, 10.0, -50.0, 5.0, 0.0, 0.0, 40.0)
HIDDEN_SIZE = (32, 8)
HIDDEN_LIGHTS = [(50.0, 100.0, 50.0, 0.1, 0.1, 0.1, 1.0, 1.0, 1.0, 0.5, 0.5, 0.5)]


def hidden_pane_scene(s, pane_tr):
    """Adds the scene to `s` (an OracleScene or a MythTracer: the same add_material / add_triangle); returns
    (floor, pane), the materials' indices as add_material gave them."""
    floor = s.add_material("floor", (0.6, 0.6, 0.55), (0.6, 0.6, 0.55), (0.2, 0.2, 0.2), ns=8.0)
    pane = s.add_material("pane", (0.05, 0.08, 0.08), (0.1, 0.15, 0.15), (0.9, 0.9, 0.9), ns=80.0, tr=pane_tr,
                          tf=(0.9, 0.95, 1.0), ni=1.0)

    def quad(y, x0, x1, z0, z1, mtl, line):
        s.add_triangle([(x0, y, z0), (x1, y, z0), (x1, y, z1)], mtl=mtl, line_no=line)
        s.add_triangle([(x0, y, z0), (x1, y, z1), (x0, y, z1)], mtl=mtl, line_no=line + 1)
    quad(0.0, -100.0, 200.0, 0.0, 300.0, floor, 1)
    quad(50.0, 20.0, 80.0, 20.0, 80.0, pane, 3)
    return floor, pane
