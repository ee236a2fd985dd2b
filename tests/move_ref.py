"""What mt_scene_set_triangle_vertices must leave behind, restated in numpy, and the planted moves of the move tests.

A move rebuilds the tree, so the scene's node-stream order changes from the old tree's tri_id to the new tree's.
`after_move` composes the two permutations by SEARCH-free inverse tables and gives the mirrors and generations the scene
must hold afterwards; the new tree itself is tree_build_ref.build's, which tests/test_tree_build_cpu.py holds to the host
builder.  `moves()` are the smallest moves at which each part of the call can go wrong, each a small scene in add order
and a chain of (listed add indices, their new vertices) steps; tests/test_move_cpu.py checks on the CPU that every
planted move does to the tree what its name says, so the GPU test cannot pass on a move that moves nothing.
"""
import os
import re

import numpy as np

import tree_build_ref as tb

ROOT = tb.ROOT
NAN, INF = float("nan"), float("inf")
W, H, DEPTH = 64, 48, 5


def constant(name):
    """An integer constant of mt_device.h (kHsShortList through its macro's default)."""
    text = open(os.path.join(ROOT, "mythtracer_amd", "csrc", "mt_device.h")).read()
    m = re.search(r"constexpr int %s = (\w+);" % name, text)
    assert m, name
    if m.group(1).isdigit():
        return int(m.group(1))
    d = re.search(r"#define %s (\d+)" % m.group(1), text)
    assert d, m.group(1)
    return int(d.group(1))


SHORT = constant("kHsShortList")
PAD = constant("kLlPad")
DEEP_FROM = constant("kDeepFromDepth")


# ---- the bookkeeping

def compose(old_tri_id, new_tri_id):
    """from[p]: the old stream position of the triangle at the new stream position p."""
    old_tri_id, new_tri_id = np.asarray(old_tri_id), np.asarray(new_tri_id)
    old_pos = np.empty(len(old_tri_id), dtype=np.int64)
    old_pos[old_tri_id] = np.arange(len(old_tri_id))
    return old_pos[new_tri_id]


def changed_triangles(v_live, idx, listed):
    """The listed add indices whose 9 doubles differ from the live ones BY BITS."""
    live = tb.bits(np.asarray(v_live, dtype=np.float64).reshape(-1, 9))
    new = tb.bits(np.asarray(listed, dtype=np.float64).reshape(-1, 9))
    idx = np.asarray(idx, dtype=np.int64)
    return idx[(live[idx] != new).any(axis=1)] if len(idx) else idx


def after_move(state, idx, listed):
    """state: dict(vertex (n, 3, 3) add order, tri_id, tri_mtl, stamp [2 arrays or None] in stream order, geo).  Returns
    the state after the set: a no-op set returns the state itself."""
    if len(changed_triangles(state["vertex"], idx, listed)) == 0:
        return state
    v = np.array(state["vertex"], dtype=np.float64).reshape(-1, 3, 3)
    v[np.asarray(idx, dtype=np.int64)] = np.asarray(listed, dtype=np.float64).reshape(-1, 3, 3)
    tree = tb.build(v)
    src = compose(state["tri_id"], tree["tri_id"])
    return dict(vertex=v, tri_id=tree["tri_id"], tri_mtl=np.asarray(state["tri_mtl"])[src],
                stamp=[None if s is None else np.asarray(s)[src] for s in state["stamp"]], geo=state["geo"] + 1, tree=tree)


# ---- small scenes in add order

MATERIALS = [
    # ka, kd, ks, ns, refl, tr, tf, ni
    dict(values=np.array([0.9, 0.8, 0.7, 0.7, 0.7, 0.7, 0.2, 0.2, 0.2, 8.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]), tex=0),
    dict(values=np.array([0.1, 0.1, 0.1, 0.2, 0.2, 0.2, 0.6, 0.6, 0.6, 32.0, 0.75, 0.0, 0.0, 0.0, 0.0, 1.0]), tex=-1),
    dict(values=np.array([0.05, 0.05, 0.1, 0.1, 0.1, 0.2, 0.4, 0.4, 0.4, 16.0, 0.0, 0.5, 0.9, 0.8, 0.7, 1.3]), tex=-1),
    dict(values=np.array([0.3, 0.4, 0.8, 0.5, 0.5, 0.5, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]), tex=1),
]


def textures():
    rng = np.random.RandomState(0x7e8)
    return [dict(texels=rng.randint(0, 256, (4, 4, 3)).astype(np.uint8)),
            dict(texels=rng.randint(0, 256, (2, 3, 3)).astype(np.uint8))]


def scene_of(v, seed=7):
    """The add-order arrays of a scene over the triangles v: unit normals that differ per vertex, texture coordinates,
    the four materials in turn with every ninth triangle without one, line numbers that are no permutation index."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3, 3)
    n = len(v)
    rng = np.random.RandomState(seed)
    nrm = rng.random_sample((n, 3, 3)) - 0.5 + np.array([0.0, 0.0, -1.0])
    nrm /= np.sqrt((nrm * nrm).sum(axis=2, keepdims=True))
    uvw = rng.random_sample((n, 3, 3)) * 2.0 - 0.5
    uvw[:, :, 2] = 0.0
    mtl = (np.arange(n) % len(MATERIALS)).astype(np.int32)
    mtl[8::9] = -1
    return dict(tri_vertex=v.reshape(-1, 9).copy(), tri_normal=nrm.reshape(-1, 9), tri_uvw=uvw.reshape(-1, 9),
                tri_material=mtl, tri_line_no=(1000 + 3 * np.arange(n)).astype(np.int32), materials=MATERIALS,
                textures=textures())


def with_vertices(tris, v):
    out = dict(tris)
    out["tri_vertex"] = np.asarray(v, dtype=np.float64).reshape(-1, 9).copy()
    return out


def camera_for(v):
    """A camera on the -z side of the finite vertices, looking along +z, that sees their bounding box."""
    p = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    if len(p) == 0:
        p = np.zeros((1, 3))
    lo, hi = np.minimum(p.min(axis=0), 0.0), np.maximum(p.max(axis=0), 0.0)
    c, ext = (lo + hi) / 2.0, max(float((hi - lo).max()), 1.0)
    return (float(c[0]), float(c[1]), float(lo[2] - 0.9 * ext), 0.0, 0.0, 0.0, 75.0)


def expected_hit_pixels(v, width=W):
    """An estimate of the pixels of a `width`-wide frame of camera_for(v) whose primary ray hits a triangle, occlusion
    aside: the triangles' areas projected along z, each over the area of a pixel at its depth (the camera looks along
    +z with 75 degrees across `width` pixels)."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3, 3)
    cam = camera_for(v)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    area = 0.5 * np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])
    depth = v[:, :, 2].mean(axis=1) - cam[2]
    pixel = 2.0 * depth * np.tan(np.radians(cam[6] / 2.0)) / width
    return float((area / (pixel * pixel)).sum())


def lights_for(v):
    cam = camera_for(v)
    return [(cam[0] + 1.0, cam[1] + 3.0, cam[2], 0.1, 0.1, 0.1, 0.8, 0.8, 0.8, 0.5, 0.5, 0.5),
            (cam[0] - 2.0, cam[1] + 1.0, cam[2] + 0.5, 0.05, 0.1, 0.02, 0.5, 0.4, 0.6, 0.3, 0.5, 0.2)]


# ---- the planted moves: name -> (vertices (n, 3, 3) in add order, [(add indices, their new vertices), ...])

def _tri(centre, size=0.2):
    c = np.asarray(centre, dtype=np.float64)
    return c + size * np.array([[-0.5, -0.5, -0.25], [0.5, -0.25, 0.0], [0.0, 0.5, 0.25]])


def _straddlers(rng, n):
    """n small triangles across the plane x = 4 of a root box {0,0,0}-{8,8,8}: they stay in the root."""
    c = np.stack([np.full(n, 4.0), 0.5 + 7.0 * rng.random_sample(n), 0.5 + 7.0 * rng.random_sample(n)], axis=1)
    return np.stack([_tri(p, 0.3) for p in c])


def _off_planes(v):
    """The triangles of v that do not touch the root's centre planes x, y, z = 4: they all leave the root."""
    lo, hi = v.min(axis=1), v.max(axis=1)
    return v[((hi < 4.0) | (lo > 4.0)).all(axis=1)]


def moves():
    planted = tb.planted()
    rng = np.random.RandomState(0x30fe)
    out = {}
    one = np.array([0], dtype=np.int32)

    def there_and_back(v, idx, listed):
        idx = np.asarray(idx, dtype=np.int32)
        return (v, [(idx, np.asarray(listed, dtype=np.float64).reshape(-1, 3, 3)), (idx, v[idx].copy())])

    # a nudge that keeps every triangle in its node: the same tree, new boxes
    base = np.concatenate([[_tri((1.0, 1.0, 1.0))], tb._filler(rng, 40)])
    out["nudge"] = there_and_back(base, one, [base[0] + 1e-3])
    # across the root's centre plane x = 4 into a sibling; onto it, so that the triangle rises to the root
    out["to_sibling"] = there_and_back(base, one, [_tri((7.0, 1.0, 1.0))])
    out["onto_plane"] = there_and_back(base, one, [_tri((4.0, 1.0, 1.0))])
    # the 16th triangle arrives in a leaf of 15: the leaf splits, n_nodes grows; back: the split disappears
    leaf = np.concatenate([[_tri((6.0, 1.0, 1.0))], planted["child_gets_15"]])
    out["leaf_15_to_16"] = there_and_back(leaf, one, [_tri((1.5, 1.5, 1.5))])
    # the root's own list: SHORT -> SHORT + 1 (short list -> long list) and back; PAD -> PAD + 1
    for name, k in (("short_to_long", SHORT), ("long_across_pad", PAD)):
        v = np.concatenate([[_tri((1.0, 1.0, 1.0))], _straddlers(rng, k), _off_planes(tb._filler(rng, 24))])
        out[name] = there_and_back(v, one, [_tri((4.0, 6.0, 2.0), 0.3)])
    # the root box grown, then shrunk
    out["root_grows"] = there_and_back(base, one, [_tri((20.0, 21.0, 22.0))])
    v = base.copy()
    v[0] = _tri((20.0, 21.0, 22.0))
    out["root_shrinks"] = there_and_back(v, one, [_tri((1.0, 1.0, 1.0))])
    # a bound that becomes -0.0; NaN in v0 and in v1 only; +-inf: from an ordinary triangle to the planted one and back
    for name, rows in (("negative_zero", (3, 5)), ("nan_in_v0", (4, 9)), ("nan_in_v1", (4, 9, 11)), ("plus_inf", (7,)),
                       ("minus_inf", (7,)), ("both_inf", (7, 8))):
        target = planted[name]
        v = target.copy()
        for r in rows:
            v[r] = _tri((-2.0, 2.0, 2.0)) if name == "negative_zero" else _tri((2.0, 2.0, 2.0))
        out[name] = there_and_back(v, rows, target[list(rows)])
    # the corner chain: 24 tiny triangles in the root's corner, scaled so that the depth goes from below
    # kDeepFromDepth to at least it and back (the deep layout and the packed stack are chosen anew)
    chain = planted["corner_chain_10"].copy()
    chain[:24] *= 2.0
    idx = np.arange(24, dtype=np.int32)
    out["chain_deepens"] = there_and_back(chain, idx, chain[:24] * 2.0 ** -3)
    out["chain_past_16"] = there_and_back(chain, idx, chain[:24] * 2.0 ** -6)  # (the wide deep layout)
    # the forms of the list on one scene: all triangles, one, a shuffled half; and the triangle counts
    for n in (1, 15, 16, 63, 65, 1025):
        v = planted["n%d" % n]
        jitter = v + 0.3 * (rng.random_sample(v.shape) - 0.5)
        idx = rng.permutation(n)[:max(1, n // 3)].astype(np.int32)
        out["n%d" % n] = (v, [(idx, jitter[idx]), (np.arange(n, dtype=np.int32), v.copy())])
    # larger triangles, an add order shuffled against space: what the frames with history are rendered of
    v = planted["shuffled"]
    idx = rng.permutation(len(v))[:len(v) // 3].astype(np.int32)
    out["shuffled"] = there_and_back(v, idx, v[idx] + 1.5 * (rng.random_sample((len(idx), 1, 3)) - 0.5))
    v = planted["n65"]
    far = v + np.array([0.5, -0.25, 1.0])
    half = rng.permutation(65)[:33].astype(np.int32)
    every = rng.permutation(65).astype(np.int32)
    out["list_forms"] = (v, [(np.arange(65, dtype=np.int32), far), (np.array([64], dtype=np.int32), v[[64]]),
                             (half, v[half]), (every, v[every])])
    return out


def never_separate_move():
    """(vertices, idx, listed): 16 + 4 triangles whose first 16, moved onto one point, never separate
    (tree_build_ref.never_separate): the build refuses at MT_MAX_TREE_DEPTH."""
    rng = np.random.RandomState(0x5e9)
    v = np.concatenate([tb._uniform(rng, 16, side=1.0, size=0.05), [_tri((0.5, 0.5, 0.5), 0.1)] * 4])
    v[16] = [[0.9, 0.9, 0.9], [1.0, 1.0, 1.0], [0.95, 1.0, 0.9]]  # the root box reaches {1, 1, 1}
    return v, np.arange(16, dtype=np.int32), tb.never_separate()
