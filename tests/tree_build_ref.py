"""The octree build restated level by level in numpy, and the planted inputs of the tree-build tests.

`build(v)` follows the rules of mt_octree_build (include/mythtracer_hip.h) the way the GPU builder does: every
triangle keeps a current node, a level is a contiguous range of node indices, the children of a level's splitting nodes
are numbered in the order of their parents, and the stream is a stable sort of (node, add index).  It is NOT a copy of
OctTree::Finalize's loop: tests/test_tree_build_cpu.py holds it to the host builder's dump on every planted input, which
pins what the GPU algorithm rests on -- ascending add index within a node, contiguous levels, the +0.0 and NaN rules of
the boxes.  Everything is compared by bits (`same`).
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_WAY = os.path.join(ROOT, "tests", "scenes", "two_way.obj")
SPLIT = 16
MAX_DEPTH = 64  # MT_MAX_TREE_DEPTH
NAN, INF = float("nan"), float("inf")
KEYS = ("node_aabb", "node_center", "first_child", "prim_begin", "prim_count", "tri_id", "tri_aabb")


class DepthExceeded(Exception):
    pass


def tri_boxes(v):
    """Triangle::CacheAABB: {v0, v0} extended by v1, then v2, with std::min(box, p) / std::max(box, p)."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3, 3)
    lo, hi = v[:, 0].copy(), v[:, 0].copy()
    with np.errstate(invalid="ignore"):
        for k in (1, 2):
            p = v[:, k]
            lo = np.where(p < lo, p, lo)
            hi = np.where(hi < p, p, hi)
    return np.concatenate([lo, hi], axis=1)


def root_box(boxes):
    """OctTree::AddPrimitive's box, order-free: the minimum / maximum over +0.0 and the bounds that are not NaN; a zero
    result is +0.0."""
    out = np.zeros(6)
    for a in range(3):
        lo = boxes[:, a][~np.isnan(boxes[:, a])]
        hi = boxes[:, 3 + a][~np.isnan(boxes[:, 3 + a])]
        if lo.size and lo.min() < 0.0:
            out[a] = lo.min()
        if hi.size and hi.max() > 0.0:
            out[3 + a] = hi.max()
    return out


def _octants(lo, hi, c):
    """(m, 8, 6): the eight children's boxes of m nodes; bit 0 = upper x, bit 1 = upper z, bit 2 = upper y."""
    m = len(lo)
    out = np.zeros((m, 8, 6))
    for k in range(8):
        up = (bool(k & 1), bool(k & 4), bool(k & 2))  # x, y, z
        for a in range(3):
            out[:, k, a] = c[:, a] if up[a] else lo[:, a]
            out[:, k, 3 + a] = hi[:, a] if up[a] else c[:, a]
    return out


def build(v, max_depth=MAX_DEPTH):
    """dict(depth, node_aabb, node_center, first_child, prim_begin, prim_count, tri_id, tri_aabb [add order]) of the
    triangles v (n, 3, 3).  DepthExceeded when a node would have to split at depth max_depth (root = 1)."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3, 3)
    n = len(v)
    boxes = tri_boxes(v)
    aabb = root_box(boxes).reshape(1, 6)
    center = np.zeros((1, 3))
    first_child = np.zeros(1, dtype=np.int64)
    cur = np.zeros(n, dtype=np.int64)
    active = np.ones(n, dtype=bool)
    level_begin, level_n, depth = 0, 1, 1
    with np.errstate(invalid="ignore", over="ignore"):
        for level in range(1, max_depth + 1):
            reached = np.bincount(cur[active] - level_begin, minlength=level_n)
            split = reached >= SPLIT
            if not split.any():
                break
            if level == max_depth:
                raise DepthExceeded("octree depth %d exceeds MT_MAX_TREE_DEPTH %d" % (level + 1, max_depth))
            next_begin = len(aabb)
            nodes = level_begin + np.nonzero(split)[0]  # in index order: the exclusive scan of the flags
            lo, hi = aabb[nodes, :3], aabb[nodes, 3:]
            c = lo + (hi - lo) / 2.0
            center[nodes] = c
            first_child[nodes] = next_begin + 8 * np.arange(len(nodes))
            aabb = np.concatenate([aabb, _octants(lo, hi, c).reshape(-1, 6)])
            center = np.concatenate([center, np.zeros((8 * len(nodes), 3))])
            first_child = np.concatenate([first_child, np.zeros(8 * len(nodes), dtype=np.int64)])
            # every triangle on its way: one level down, or home
            t = np.nonzero(active)[0]
            fc = first_child[cur[t]]
            active[t[fc == 0]] = False
            t, fc = t[fc != 0], fc[fc != 0]
            home = np.full(len(t), -1, dtype=np.int64)
            bl, bh = boxes[t, :3], boxes[t, 3:]
            for k in range(8):
                cb = aabb[fc + k]
                inside = ((bl >= cb[:, :3]) & (bl <= cb[:, 3:]) & (bh >= cb[:, :3]) & (bh <= cb[:, 3:])).all(axis=1)
                home = np.where((home < 0) & inside, k, home)
            active[t[home < 0]] = False
            cur[t[home >= 0]] = fc[home >= 0] + home[home >= 0]
            level_begin, level_n, depth = next_begin, 8 * len(nodes), level + 1
    n_nodes = len(aabb)
    prim_count = np.bincount(cur, minlength=n_nodes)
    return dict(depth=depth, node_aabb=aabb, node_center=center, first_child=first_child.astype(np.int32),
                prim_begin=(np.cumsum(prim_count) - prim_count).astype(np.int32), prim_count=prim_count.astype(np.int32),
                tri_id=np.argsort(cur, kind="stable").astype(np.int32), tri_aabb=boxes)


def facade_of(M, v, **kw):
    """A MythTracer holding the triangles v (n, 3, 3) in that order, unfinalized."""
    m = M.MythTracer(None, **kw)
    for i, t in enumerate(np.asarray(v, dtype=np.float64).reshape(-1, 3, 3)):
        m.add_triangle(t, line_no=i)
    return m


def host_dump(m):
    """The facade's tree (MythTracer.tree(), finalizing with whichever builder it is set to) and its triangles' cached
    boxes, in build()'s form."""
    t = m.tree()
    data, _, _ = m.triangles()
    return dict(depth=t["depth"], node_aabb=t["aabb"], node_center=t["center"], first_child=t["first_child"],
                prim_begin=t["prim_begin"], prim_count=t["prim_count"], tri_id=t["prim_ids"], tri_aabb=data[:, 27:33])


def obj_triangles(M, path):
    """(n, 3, 3) vertices of an .obj in its add order, through the facade's reader."""
    m = M.MythTracer(path)
    data, _, _ = m.triangles()
    return data[:, :9].reshape(-1, 3, 3).copy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def differences(got, want):
    """The names of the arrays (and `depth`) in which two trees differ, by bits."""
    out = [] if int(got["depth"]) == int(want["depth"]) else ["depth %d != %d" % (got["depth"], want["depth"])]
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.dtype != np.float64:
            g, w = g.astype(np.int64), w.astype(np.int64)
        if g.size != w.size or not np.array_equal(bits(g).reshape(-1), bits(w).reshape(-1)):
            out.append("%s (%d vs %d values)" % (k, g.size, w.size))
    return out


# ---- planted inputs: the smallest shapes at which each rule can go wrong

def _small(rng, centre, size, n):
    """n triangles of extent <= size around the points `centre` ((3,) or (n, 3))."""
    return np.asarray(centre, dtype=np.float64).reshape(-1, 1, 3) + size * (rng.random_sample((n, 3, 3)) - 0.5)


def _uniform(rng, n, side=10.0, size=0.2):
    return _small(rng, side * rng.random_sample((n, 3)), size, n)


def _filler(rng, n=20):
    """Small triangles spread over [0, 8]^3, with the cube's far corner reached: the root box is {0,0,0}-{8,8,8}."""
    v = _small(rng, 0.5 + 7.0 * rng.random_sample((n, 3)), 0.25, n)
    v[0] = [[7.5, 7.5, 7.5], [8.0, 8.0, 8.0], [7.75, 8.0, 7.5]]
    return v


def _point(p):
    return np.array([[p, p, p]], dtype=np.float64)


def planted():
    """name -> (n, 3, 3) vertices in add order."""
    rng = np.random.RandomState(0x0c7ee)
    out = {}
    out["n0"] = np.zeros((0, 3, 3))
    for n in (1, 15, 16):
        out["n%d" % n] = _uniform(rng, n)
    # the root reaches from the origin to 8; 15 of 16 in octant 0 (a leaf of 15), one far away
    out["child_gets_15"] = np.concatenate([_small(rng, (1.5, 1.5, 1.5), 1.0, 15),
                                           [[[7.5, 7.5, 7.5], [8.0, 8.0, 8.0], [7.75, 8.0, 7.5]]]])
    # all 16 in [5, 6]^3: the root {0}-{6} splits at 3, child 7 receives exactly 16 and splits again
    out["child_gets_16"] = _small(rng, (5.5, 5.5, 5.5), 1.0, 16)
    # 24 tiny triangles in the corner at the origin of a root box {0}-{8}: child 0, again and again
    out["corner_chain_10"] = np.concatenate([_small(rng, (2.0 ** -8, 2.0 ** -8, 2.0 ** -8), 2.0 ** -9, 24), _filler(rng, 4)])
    # 20 triangles of extent 2^-22 around (8/3, 8/3, 8/3): a cell of size s has its faces s / 3 away from that point, so
    # the cluster stays whole down to cells of 8 x 2^-24 and reaches levels 24 and 25
    out["deep_chain_25"] = np.concatenate([_small(rng, (8.0 / 3, 8.0 / 3, 8.0 / 3), 2.0 ** -22, 20), _filler(rng, 4)])
    # boxes that end exactly on the root's centre plane x = 4, from below and from above; on y and z likewise
    touch = []
    for a in range(3):
        for side in (-1.0, 1.0):
            t = np.array([[1.0, 1.0, 1.0], [1.5, 1.25, 1.0], [1.25, 1.5, 1.5]])
            t[:, a] = [4.0, 4.0 + side * 0.5, 4.0 + side * 0.25]
            touch.append(t)
    out["touching_planes"] = np.concatenate([np.array(touch), _filler(rng)])
    # zero-extent boxes: a point on the plane x = 4, one on the edge x = z = 4, one on the centre itself, one on a
    # grandchild's centre (2, 2, 2) and on the root's corners
    pts = [(4.0, 1.0, 1.0), (4.0, 1.0, 4.0), (4.0, 4.0, 4.0), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0), (8.0, 8.0, 8.0), (6.0, 4.0, 2.0)]
    out["points_on_planes"] = np.concatenate([np.concatenate([_point(p) for p in pts]), _filler(rng),
                                              _small(rng, (1.0, 1.0, 1.0), 0.5, 18)])
    # far inside the positive octant: the root reaches back to the origin
    out["far_positive"] = _small(rng, 100.0 + rng.random_sample((40, 3)), 0.1, 40)
    out["far_negative"] = _small(rng, -100.0 - rng.random_sample((40, 3)), 0.1, 40)
    # -0.0 as the largest bound (everything at or below zero in x) and as the smallest (at or above, in y)
    neg = _uniform(rng, 24)
    neg[:, :, 0] = -np.abs(neg[:, :, 0])
    neg[3, :, 0] = [-0.0, -1.0, -0.0]
    neg[5, :, 1] = [-0.0, 2.0, 1.0]
    neg[:, :, 1] = np.where(neg[:, :, 1] == 0.0, neg[:, :, 1], np.abs(neg[:, :, 1]))
    out["negative_zero"] = neg
    only = _uniform(rng, 20)
    only[:, :, 2] = np.where(rng.random_sample((20, 3)) < 0.5, -0.0, 0.0)  # z: every bound is a zero of either sign
    out["only_zeros_in_z"] = only
    nan0 = _uniform(rng, 30)
    nan0[4, 0, 1] = NAN
    nan0[9, 0] = NAN
    out["nan_in_v0"] = nan0
    nan1 = _uniform(rng, 30)
    nan1[4, 1, 1] = NAN
    nan1[9, 1] = NAN
    nan1[11, 2, 0] = NAN
    out["nan_in_v1"] = nan1
    for name, val in (("plus_inf", INF), ("minus_inf", -INF)):
        inf = _uniform(rng, 30)
        inf[7, 1, 0] = val
        out[name] = inf
    both = _uniform(rng, 30)
    both[7, 1, 0], both[8, 2, 0] = INF, -INF
    out["both_inf"] = both
    # 4^3 cells of 20 triangles each, added in an order shuffled against space
    cells = np.array([(x, y, z) for x in range(4) for y in range(4) for z in range(4)], dtype=np.float64) * 2.0 + 1.0
    grid = _small(rng, np.repeat(cells, 20, axis=0), 0.5, 64 * 20)
    out["shuffled"] = grid[rng.permutation(len(grid))]
    for n in (63, 64, 65, 1023, 1025):
        out["n%d" % n] = _uniform(rng, n, size=0.05)
    return out


def grid16():
    """16^3 cells of 16 small triangles each, cell by cell: a level of 4096 nodes, 65 536 triangles."""
    rng = np.random.RandomState(0x16ced)
    cells = np.array([(x, y, z) for x in range(16) for y in range(16) for z in range(16)], dtype=np.float64) + 0.5
    return _small(rng, np.repeat(cells, 16, axis=0), 0.25, 4096 * 16)


def never_separate():
    """16 triangles that are the same point, the far corner of the root box {0,0,0}-{1,1,1}: a zero-extent box on a
    corner is contained in a child at every level, so they share every node down to any depth."""
    return np.repeat(_point((1.0, 1.0, 1.0)), 16, axis=0)
