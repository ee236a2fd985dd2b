"""What mt_scene_edit_triangles must leave behind, restated in numpy, and the planted edits of the edit tests.

An edit numbers the add order anew -- numpy.delete of the removed indices followed by concatenate of the added triangles
-- and rebuilds the tree over it.  `apply` does that to the add-order arrays of a scene (move_ref.scene_of's form);
`after_edit` gives the mirrors and the generation the scene must hold afterwards, through add order: the per-triangle
mirrors are brought from the old stream order into add order, deleted from and appended to like every other array, and
brought into the new tree's stream order (tree_build_ref.build's, which tests/test_tree_build_cpu.py holds to the host
builder).  `edits()` are the smallest edits at which each part of the call can go wrong, each a small scene in add order
and a chain of (remove list, added vertices) steps; tests/test_edit_triangles_cpu.py checks on the CPU that every planted
edit does to the tree what its name says, so the GPU test cannot pass on an edit that changes nothing.
"""
import numpy as np

import move_ref as mv
import tree_build_ref as tb

W, H, DEPTH = mv.W, mv.H, mv.DEPTH
SHORT, PAD, DEEP_FROM = mv.SHORT, mv.PAD, mv.DEEP_FROM
PER_TRIANGLE = ("tri_vertex", "tri_normal", "tri_uvw", "tri_material", "tri_line_no")
ADDED_MATERIALS = (-1, 0, 3, 1, 2)  # none, the two textured materials of move_ref.MATERIALS, the two plain ones
# the chains that end with the triangles they began with in ANOTHER add order (re-appended triangles have the last indices)
OTHER_ORDER = ("sixteenth_out_and_in", "shuffled")


# ---- the bookkeeping

def added(v, seed=23):
    """The add dict of HipAbi.scene_edit_triangles for the triangles v, or None for none: move_ref.scene_of's normals,
    uvw and line numbers (shifted, so that no added line number is a scene's) and ADDED_MATERIALS in turn."""
    if v is None or len(v) == 0:
        return None
    tris = mv.scene_of(v, seed=seed)
    out = {k: tris[k] for k in PER_TRIANGLE}
    out["tri_material"] = np.array([ADDED_MATERIALS[j % len(ADDED_MATERIALS)] for j in range(len(v))], dtype=np.int32)
    out["tri_line_no"] = (out["tri_line_no"] + 500000 + seed).astype(np.int32)
    return out


def new_order(a, remove, add):
    """numpy.delete followed by concatenate, along the first axis"""
    out = np.delete(np.asarray(a), np.asarray(remove, dtype=np.int64), axis=0)
    return out if add is None else np.concatenate([out, np.asarray(add, dtype=out.dtype).reshape((-1,) + out.shape[1:])])


def apply(tris, remove, add):
    """The add-order arrays of the scene after the edit; materials and textures are the scene's."""
    out = dict(tris)
    for k in PER_TRIANGLE:
        out[k] = new_order(tris[k], remove, None if add is None else add[k])
    return out


def after_edit(state, remove, add):
    """state: dict(tris [add-order arrays], tri_id, tri_mtl, stamp [2 arrays or None] in stream order, geo).  Returns the
    state after the edit; the no-op edit returns the state itself."""
    remove = np.asarray([] if remove is None else remove, dtype=np.int64)
    n_add = 0 if add is None else len(add["tri_material"])
    if len(remove) == 0 and n_add == 0:
        return state
    tris = apply(state["tris"], remove, add)
    tree = tb.build(tris["tri_vertex"].reshape(-1, 3, 3))
    old_id, new_id = np.asarray(state["tri_id"]), tree["tri_id"]

    def mirror(was, fresh):
        if was is None:
            return None
        by_add = np.empty_like(np.asarray(was))
        by_add[old_id] = was  # stream order -> add order
        return new_order(by_add, remove, fresh)[new_id]

    zeros = None if n_add == 0 else np.zeros(n_add, dtype=np.uint32)
    return dict(tris=tris, tri_id=new_id, tri_mtl=mirror(state["tri_mtl"], None if add is None else add["tri_material"]),
                stamp=[mirror(s, zeros) for s in state["stamp"]], geo=state["geo"] + 1, tree=tree)


def state_of(tris):
    """The state of a scene newly made from the add-order arrays tris."""
    tree = tb.build(tris["tri_vertex"].reshape(-1, 3, 3))
    return dict(tris=tris, tri_id=tree["tri_id"], tri_mtl=tris["tri_material"][tree["tri_id"]], stamp=[None, None], geo=0, tree=tree)


def vertices_after(v, steps):
    """[v, the vertices after step 0, after step 1, ...], each (n, 3, 3) in add order"""
    out = [np.asarray(v, dtype=np.float64).reshape(-1, 3, 3)]
    for remove, add_v in steps:
        out.append(new_order(out[-1], remove, add_v))
    return out


# ---- the planted edits: name -> (vertices (n, 3, 3) in add order, [(remove list, added vertices (k, 3, 3) or None), ...])

def edits():
    planted = tb.planted()
    rng = np.random.RandomState(0xed17)
    out = {}
    none = np.zeros(0, dtype=np.int32)

    def idx(*a):
        return np.array(a, dtype=np.int32)

    def in_and_out(v, add_v):
        """appended, then removed again: the added triangles have the last indices"""
        add_v = np.asarray(add_v, dtype=np.float64).reshape(-1, 3, 3)
        return (v, [(none, add_v), (np.arange(len(v), len(v) + len(add_v), dtype=np.int32), None)])

    # one triangle appended into a leaf of 15: the leaf splits, n_nodes grows; removed again: the split disappears
    out["leaf_15_to_16"] = in_and_out(planted["child_gets_15"], [mv._tri((1.5, 1.5, 1.5))])
    # the 16th triangle of a node removed: the node does not split any more; appended again it has the LAST add index, so
    # the stream order differs from the start
    v = np.concatenate([planted["child_gets_15"][:3], [mv._tri((1.5, 1.5, 1.5))], planted["child_gets_15"][3:]])
    out["sixteenth_out_and_in"] = (v, [(idx(3), None), (none, v[[3]])])
    # the root's own list: SHORT -> SHORT + 1 (short list -> long list) and back; PAD -> PAD + 1
    for name, k in (("short_to_long", SHORT), ("long_across_pad", PAD)):
        v = np.concatenate([mv._straddlers(rng, k), mv._off_planes(tb._filler(rng, 24))])
        out[name] = in_and_out(v, [mv._tri((4.0, 6.0, 2.0), 0.3)])
    # the root box grown by an append outside it, shrunk by removing the one far triangle
    base = np.concatenate([[mv._tri((1.0, 1.0, 1.0))], tb._filler(rng, 40)])
    out["root_grows_and_shrinks"] = in_and_out(base, [mv._tri((20.0, 21.0, 22.0))])
    # NaN in v0, NaN in v1 only, +-inf: the planted triangles appended to the ordinary ones of their scene
    for name, rows in (("nan_in_v0", (4, 9)), ("nan_in_v1", (4, 9, 11)), ("plus_inf", (7,)), ("minus_inf", (7,)), ("both_inf", (7, 8))):
        target = planted[name]
        out[name] = in_and_out(np.delete(target, rows, axis=0), target[list(rows)])
    # the corner chain appended: the depth goes from below kDeepFromDepth to at least it, and past 16 (the wide deep
    # layout), then back (the deep layout and the packed stack are chosen anew)
    chain = planted["corner_chain_10"]
    out["chain_deepens"] = in_and_out(chain[24:], chain[:24] * 2.0 * 2.0 ** -3)
    out["chain_past_16"] = in_and_out(chain[24:], chain[:24] * 2.0 * 2.0 ** -6)
    # the forms of the remove list on one scene: index 0, the last index, an unsorted shuffled half, all but one; then
    # remove and add in ONE call brings the scene back: the one survivor out, all 65 in
    v = planted["n65"]
    half = rng.permutation(63)[:32].astype(np.int32)
    assert list(half) != sorted(half)
    out["remove_forms"] = (v, [(idx(0), None), (idx(63), None), (half, None), (rng.permutation(31)[:30].astype(np.int32), None),
                               (idx(0), v)])
    # remove and add in one call: k out and k others in, k out and k + 1 in; then all 64 out and the first 63 in
    v = planted["n63"]
    others = tb._uniform(rng, 11, size=0.05)
    out["swap_in_one_call"] = (v, [(rng.permutation(63)[:5].astype(np.int32), others[:5]),
                                   (rng.permutation(63)[:5].astype(np.int32), others[5:]),
                                   (rng.permutation(64).astype(np.int32), v)])
    # the counts 1 -> 2, 15 -> 16, 16 -> 15, 63 -> 65, 65 -> 1
    v = planted["n65"]
    out["counts"] = (v[:1], [(none, v[1:2]), (none, v[2:15]), (none, v[15:16]), (idx(15), None), (none, v[16:64]),
                             (none, np.concatenate([v[64:65], v[15:16]])), (np.arange(1, 65, dtype=np.int32), None)])
    # 1024 -> 1025 -> 1024
    v = planted["n1025"]
    out["n1024"] = in_and_out(v[:1024], v[1024:])
    # larger triangles, an add order shuffled against space: what the frames with history and the other calls are
    # rendered of -- 100 triangles out and 100 others in, then those out and the first ones in again
    v = planted["shuffled"][:1000]
    gone = rng.permutation(1000)[:100].astype(np.int32)
    new = planted["shuffled"][1000:1100] + 1.5 * (rng.random_sample((100, 1, 3)) - 0.5)
    out["shuffled"] = (v, [(gone, new), (np.arange(900, 1000, dtype=np.int32), v[gone])])
    return out


def never_separate_edit():
    """(vertices, added vertices): 4 + 1 triangles in a root box {0,0,0}-{1,1,1}, and tree_build_ref.never_separate()'s 16
    to append: the build refuses at MT_MAX_TREE_DEPTH."""
    v = np.concatenate([[mv._tri((0.5, 0.5, 0.5), 0.1)] * 4, [[[0.9, 0.9, 0.9], [1.0, 1.0, 1.0], [0.95, 1.0, 0.9]]]])
    return v, tb.never_separate()


def visible_edit():
    """(vertices, remove list, added vertices): 63 triangles large enough to be seen, 5 out and 6 in -- what the test of
    an edit after other edits renders, whose ray tree must hit triangles."""
    rng = np.random.RandomState(0x5ee)
    return tb._uniform(rng, 63, size=4.0), rng.permutation(63)[:5].astype(np.int32), tb._uniform(rng, 6, size=4.0)
