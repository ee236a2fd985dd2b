"""What mt_raytree_regrow_materials (include/mythtracer_hip.h) keeps, traces and drops, restated over two restated trees
-- shared by tests/test_regrow_cpu.py, which pins the numbers with the oracle alone, and tests/test_gpu_regrow.py, which
holds the kernels to them.  Test infrastructure.

The truth for materials B always comes from a scene BUILT with B (material_edit_ref.variant): tree A and tree B are both
raytree_ref.build, on the scene as it is and on the variant.  `match` walks the two trees top-down and gives every ray of
B its index in A's layer of the same depth where its whole path from the pixel exists in A (KEPT), or -1 (TRACED);
`regrow` assembles the tree the call must leave from A's planes at those indices and B's traced rays.
"""
import numpy as np

import material_edit_ref as me

# the five edits of the regrow tests on two_way.obj: material_edit_ref's three shape-breaking ones, one that grows and
# drops subtrees at once while albedo, coef and the light planes of kept rays change, and one that leaves layer 0 alone
EDITS = dict(me.SHAPE_BREAKING)
EDITS["grow and drop"] = {"mirror": {"Refl": 0.125}, "blue": {"Refl": 0.25, "Ka": (0.9, 0.5, 0.25)}, "pane": {"Tr": 0.5}}
EDITS["matte"] = {"floor": {"Refl": 0}, "ceiling": {"Refl": 0}, "left": {"Refl": 0}, "right": {"Refl": 0},
                  "mirror": {"Refl": 0}, "pane": {"Refl": 0, "Tr": 0}}
# which of them a shadow ray can see (a transparency changes): the all-lights re-trace runs
SHADOW_EDITS = ("pane opaque", "grow and drop", "matte")

# A -> B per edit: B's rays per layer, the rays traced per layer of B, the rays dropped per layer of A; the reverse
# direction swaps traced and dropped.  Whole frame, A = material_edit_ref.TREE_A ...
FRAME = {
    "mirror 0.125": ([5184, 4353, 1561, 229, 3], [0, 0, 0, 0, 0], [0, 0, 0, 0, 3, 2]),
    "blue refl": ([5184, 4378, 1618, 407, 60, 12], [0, 25, 57, 178, 54, 10], [0, 0, 0, 0, 0, 0]),
    "pane opaque": ([5184, 3722, 1326, 229, 3, 2], [0, 0, 0, 0, 0, 0], [0, 631, 235, 0, 3, 0]),
    "grow and drop": ([5184, 4378, 1618, 407, 3], [0, 25, 57, 178, 0], [0, 0, 0, 0, 3, 2]),
    "matte": ([5184], [0], [0, 4353, 1561, 229, 6, 2]),
}
# ... and the off-grid chunk (5, 3, 61, 37), A = CHUNK_A
CHUNK_A = [2257, 2210, 952, 120, 6, 2]
CHUNK = {
    "mirror 0.125": ([2257, 2210, 952, 120, 3], [0, 0, 0, 0, 0], [0, 0, 0, 0, 3, 2]),
    "blue refl": ([2257, 2214, 998, 205, 11, 12], [0, 4, 46, 85, 5, 10], [0, 0, 0, 0, 0, 0]),
    "pane opaque": ([2257, 1864, 750, 120, 3, 2], [0, 0, 0, 0, 0, 0], [0, 346, 202, 0, 3, 0]),
    "grow and drop": ([2257, 2214, 998, 205, 3], [0, 4, 46, 85, 0], [0, 0, 0, 0, 3, 2]),
    "matte": ([2257], [0], [0, 2210, 952, 120, 6, 2]),
}


def table(chunk):
    return CHUNK if chunk else FRAME


def shadow_relevant(mats_a, mats_b):
    """mt_raytree_update_materials's rule over two OracleScene.materials() tables: a transparency changed, or the
    transmission filter of a material that is not opaque before and after."""
    for (_, a, _), (_, b, _) in zip(mats_a, mats_b):
        opaque = a[11] == 0.0 and b[11] == 0.0
        if a[11] != b[11] or (not np.array_equal(a[12:15], b[12:15]) and not opaque):
            return True
    return False


def match(tree_a, tree_b, shadow=False):
    """The rays of B path-matched to A.  dict(src = per layer of B the ray's index in A's layer, -1 = traced; kept,
    traced = per layer of B; dropped = per layer of A; rays_secondary, shaded_hits, rays_shadow = what the call counts:
    the traced rays, their hits, their shadow-loop iterations, plus all of B's iterations when `shadow` is set (the
    all-lights re-trace over the whole new tree)."""
    la, lb = tree_a["layers"], tree_b["layers"]
    src = [np.arange(len(lb[0]["ray"]), dtype=np.int64)]
    assert len(la[0]["ray"]) == len(lb[0]["ray"])
    for k in range(len(lb) - 1):
        nxt = np.full(len(lb[k + 1]["ray"]), -1, dtype=np.int64)
        for slot in ("child_refl", "child_refr"):
            i = np.nonzero(lb[k][slot] >= 0)[0]
            s = src[k][i]
            old = np.full(len(i), -1, dtype=np.int64)
            if k < len(la):
                has = s >= 0
                old[has] = la[k][slot][s[has]]
            nxt[lb[k][slot][i]] = old
        src.append(nxt)
    kept = [int((s >= 0).sum()) for s in src]
    traced = [int((s < 0).sum()) for s in src]
    dropped = [n - (kept[k] if k < len(kept) else 0) for k, n in enumerate(tree_a["n_rays"])]
    for k, s in enumerate(src):  # (a kept ray's index is used once)
        assert len(set(s[s >= 0].tolist())) == kept[k]
    new = [np.nonzero(s < 0)[0] for s in src]
    out = dict(src=src, kept=kept, traced=traced, dropped=dropped)
    out["rays_secondary"] = int(sum(traced))
    out["shaded_hits"] = int(sum(int((l["prim"][i] >= 0).sum()) for l, i in zip(lb, new)))
    out["rays_shadow"] = int(sum(int(l["iterations"][:, i].sum()) for l, i in zip(lb, new)))
    if shadow:
        out["rays_shadow"] += tree_b["rays_shadow"]
    return out


def regrow(tree_a, tree_b, src, mats_a, mats_b, shadow):
    """The layers the call must leave, assembled as the call assembles them.  A KEPT ray: ray, in_object, point, normal,
    material and prim from A at src; albedo from A, or B's ambient where the material's ambient changed; the light planes
    from A, or B's when `shadow` (the re-trace); coef from B (the propagation is material_edit_ref.check_pass's subject).
    A TRACED ray: B's.  The child indices are B's.  Returns the list of layer dicts."""
    ambient_changed = np.array([not np.array_equal(a[1][0:3], b[1][0:3]) for a, b in zip(mats_a, mats_b)])
    out = []
    for k, (lb, s) in enumerate(zip(tree_b["layers"], src)):
        lay = {name: np.array(lb[name]) for name in me.PLANES}
        lay["prim"] = np.array(lb["prim"])
        keep = np.nonzero(s >= 0)[0]
        if len(keep):
            la = tree_a["layers"][k]
            at = s[keep]
            for name in ("ray", "in_object", "point", "normal", "material", "prim"):
                lay[name][keep] = la[name][at]
            m = la["material"][at]
            fresh = (m >= 0) & ambient_changed[np.maximum(m, 0)]
            lay["albedo"][keep] = la["albedo"][at]
            for j in np.nonzero(fresh)[0]:
                lay["albedo"][keep[j]] = mats_b[m[j]][1][0:3]
            if not shadow:
                lay["power"][:, keep] = la["power"][:, at]
                lay["in_shadow"][:, keep] = la["in_shadow"][:, at]
        if k == 0:
            lay["pixel"] = np.array(tree_a["layers"][0]["pixel"])
        out.append(lay)
    return out
