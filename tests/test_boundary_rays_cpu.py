"""tests/boundary_rays.py against the oracle alone (no GPU): slab() is the oracle's box test, the generated rays sit
where the fp32 filters decide, and scaling by powers of two is exact.  The floors guard the generator, not a kernel:
they lie below the shares a CPU prototype of the recipe gave (34-37 % accepted in zone, about 28 % rejected in zone,
15-17 % hits of the targeted triangle)."""
import numpy as np
import pytest

import boundary_rays as br

P = range(len(br.PLACEMENTS))


def test_slab_is_the_oracles_box_test():
    """Scenes of ONE triangle, one intersect call per ray: the triangle's filter is counted only after the root's box
    test passed (the root box starts from the origin's point, octtree.h, so it is not the triangle's), and
    Möller-Trumbore only after the triangle's own box test passed (primitive_triangle.cc:83-108).  The two counters are
    slab()'s two verdicts."""
    n_rays = n_accepted = 0
    for p in P:
        c = br.case(p)
        rays_of = {}
        for r in np.nonzero(c["tri"] >= 0)[0][:1200]:
            rays_of.setdefault(int(c["tri"][r]), []).append(int(r))
        for t, rs in rays_of.items():
            o = br.oracle_scene(c["tris"][t:t + 1])
            assert np.array_equal(c["box"][rs[0]], br.tri_boxes(c["tris"][t:t + 1])[0])
            root, _, _ = br.slab(o.root_aabb(), c["rays"][rs, :3], c["rays"][rs, 3:])
            acc, _, _ = br.slab(c["box"][rs], c["rays"][rs, :3], c["rays"][rs, 3:])
            for r, a, b in zip(rs, root, acc):
                got = o.intersect(c["rays"][r])["counters"]
                assert (got["tri_tests"], got["mt_tests"]) == (int(a), int(a and b)), (p, t, r, got)
            assert root[acc].all()
            n_rays += len(rs)
            n_accepted += int(acc.sum())
    print("%d rays, %d accepted" % (n_rays, n_accepted))
    assert n_rays == 3600 and 0.2 < n_accepted / n_rays < 0.8
    assert set(c["step"][np.nonzero(c["tri"] >= 0)[0][:1200]]) == set(range(len(br.LADDER)))


def test_slab_restates_the_nan_rules():
    """std::min / std::max keep their FIRST operand when a comparison with NaN fails: an origin on a min plane with a
    zero direction component passes through NaN, one on a max plane does not (mt_trace.h, degenerate_axis)."""
    box = np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0])
    acc, _, _ = br.slab(box, [[0.0, 5.0, 0.5], [1.0, 5.0, 0.5], [0.5, 5.0, 0.5], [2.0, 5.0, 0.5]],
                        [[0.0, -1.0, 0.1]] * 4)
    o = br.oracle_scene(np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]]]))
    want = [o.intersect([ox, 5.0, 0.5, 0.0, -1.0, 0.1])["counters"]["mt_tests"] for ox in (0.0, 1.0, 0.5, 2.0)]
    assert list(acc.astype(int)) == want


@pytest.mark.parametrize("p", P)
def test_the_scene_is_what_the_filters_need(p):
    c = br.case(p)
    tb = br.tri_boxes(c["tris"])
    inexact = br.inexact_in_fp32(tb).mean()
    flat = ((tb[:, 3:] - tb[:, :3]) == 0.0).any(axis=1).mean()
    counts = c["tree"]["prim_count"]
    print("placement %d: %.1f %% of the box coordinates inexact in fp32, %.1f %% flat boxes, %d nodes, depth %d, "
          "longest list %d" % (p, 100 * inexact, 100 * flat, len(counts), c["tree"]["depth"], counts.max()))
    assert inexact >= 0.6
    assert flat >= 0.2                      # the right triangles
    assert counts.max() >= 64 and (counts[counts > 0] < 16).any()  # long lists (blocks, supers) and short ones
    assert len(counts) >= 200
    # shared planes survive the placement: a lattice has far fewer distinct coordinates than boxes
    assert len(np.unique(tb[:, 0])) <= 80


@pytest.mark.parametrize("p", P)
def test_the_rays_are_where_the_filters_decide(p):
    c = br.case(p)
    n = len(c["rays"])
    assert n == br.N_RAYS and np.isfinite(c["rays"]).all() and (c["rays"][:, 3:] != 0.0).all()
    zone = c["a_zone"] | c["r_zone"]
    hit = c["want"]["line"] >= 0
    own = hit & (c["want"]["line"] == c["tri"])
    by_kind = [zone[c["kind"] == k].mean() for k in range(len(br.KINDS))]
    print("placement %d: accepted in zone %.1f %%, rejected in zone %.1f %%, hit %.1f %%, the targeted triangle "
          "%.1f %%; in zone per kind %s" % (p, 100 * c["a_zone"].mean(), 100 * c["r_zone"].mean(), 100 * hit.mean(),
                                            100 * own.mean(), ["%.0f %%" % (100 * x) for x in by_kind]))
    assert c["a_zone"].mean() >= 0.20
    assert c["r_zone"].mean() >= 0.20
    assert own.mean() >= 0.10
    assert min(by_kind) >= 0.15
    assert 0.2 < hit.mean() < 0.98
    # every step of the ladder decides rays in the zone, on both sides of it
    for s in range(len(br.LADDER)):
        assert c["a_zone"][c["step"] == s].any() and c["r_zone"][c["step"] == s].any(), s
    # waves: runs of 64 of one sign octant in the first part, mixed octants after it
    octant = (c["rays"][:, 3:] < 0) @ np.array([1, 2, 4])
    n_uni = int(c["uniform"].sum())
    assert n_uni % 64 == 0 and n_uni >= n * 3 // 8
    per_wave = octant.reshape(-1, 64)
    assert (per_wave[:n_uni // 64] == per_wave[:n_uni // 64, :1]).all()
    assert len(set(per_wave[:n_uni // 64, 0])) == 8
    assert ((per_wave[n_uni // 64:] != per_wave[n_uni // 64:, :1]).any(axis=1)).all()


def _clear_of_the_det_threshold(tris, rays, shift):
    """Rays for which no determinant the reference can get to evaluate (primitive_triangle.cc:88-93, its operation
    order; only behind the triangle's box test) changes sides of the 1e-8 threshold when it is multiplied by 2^shift.
    (The rounding noise that a zero-area lattice triangle has for a determinant does change sides.)"""
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    tb = br.tri_boxes(tris)
    clear = np.ones(len(rays), dtype=bool)
    for r0 in range(0, len(rays), 256):
        d = rays[r0:r0 + 256, None, 3:]
        pvec = np.stack([d[..., 1] * e2[:, 2] - d[..., 2] * e2[:, 1], d[..., 2] * e2[:, 0] - d[..., 0] * e2[:, 2],
                         d[..., 0] * e2[:, 1] - d[..., 1] * e2[:, 0]], axis=-1)
        det = e1[:, 0] * pvec[..., 0] + e1[:, 1] * pvec[..., 1] + e1[:, 2] * pvec[..., 2]
        small = (det >= -0.00000001) & (det < 0.00000001)
        det2 = det * 2.0 ** shift
        small2 = (det2 >= -0.00000001) & (det2 < 0.00000001)
        tested, _, _ = br.slab(tb[None], rays[r0:r0 + 256, None, :3], d)
        clear[r0:r0 + 256] = ((small == small2) | ~tested).all(axis=1)
    return clear


@pytest.mark.parametrize("k,j", [(60, -55), (-10, 40), (3, 0), (0, 7)])
def test_power_of_two_scaling_is_exact(k, j):
    """Scene and origins times 2^k, directions times 2^j: every slab product scales by 2^(k - j) without a rounding,
    so the traversal is the same; det scales by 2^(2k + j), t by 2^(k - j), the hit point by 2^k.  The GPU tests of the
    filter's preconditions rest on this."""
    c = br.case(0)
    n = 2048
    rays = c["rays"][:n]
    clear = _clear_of_the_det_threshold(c["tris"], rays, 2 * k + j)
    assert clear.mean() > 0.9
    scaled = np.concatenate([rays[:, :3] * 2.0 ** k, rays[:, 3:] * 2.0 ** j], axis=1)
    got = br.oracle_scene(c["tris"] * 2.0 ** k).intersect(scaled)
    want = {key: c["want"][key][:n] for key in ("line", "t", "point")}
    assert np.array_equal(got["line"][clear], want["line"][clear])
    hit = clear & (want["line"] >= 0)
    assert hit.mean() > 0.2
    assert np.array_equal(got["t"][hit], want["t"][hit] * 2.0 ** (k - j))
    assert np.array_equal(got["point"][hit], want["point"][hit] * 2.0 ** k)


def test_the_precondition_rays_reach_the_preconditions():
    """E1-E3 of test_gpu_boundary_rays.py, the part that needs no GPU: M on both sides of 2^120 between and within
    waves; reciprocals beyond fp32's range with M still below 2^120; reciprocals below fp32's normal range."""
    tris, rays, m = br.precondition_m_rays(br.case(0))
    above = (m > 2.0 ** 120).reshape(-1, 64).sum(axis=1)
    assert (m > 2.0 ** 119).all() or (above > 0).any()
    assert (above == 0).sum() >= 4 and (above == 64).sum() >= 4 and (above == 1).sum() >= 4
    assert ((above > 1) & (above < 64)).sum() >= 4
    near = (m > 2.0 ** 119) & (m <= 2.0 ** 121)
    assert near.mean() > 0.7

    tris, rays = br.precondition_big_reciprocal_rays(br.case(2))
    bmax = np.abs(tris).max(axis=(0, 1))
    assert ((bmax + np.abs(rays[:, :3])) < 2.0 ** -8).all()
    inv = np.abs(1.0 / rays[:, 3:])
    m = br.filter_m(bmax, rays[:, :3], rays[:, 3:])
    hole = (m <= 2.0 ** 120) & (inv > 2.0 ** 128).any(axis=1)
    print("E2: %.1f %% of the rays pass the M check with a reciprocal above 2^128" % (100 * hole.mean()))
    assert hole.mean() >= 0.1
    assert (m <= 2.0 ** 120).mean() < 0.9 and ((m <= 2.0 ** 120) & ~hole).mean() >= 0.1

    tris, rays = br.precondition_small_reciprocal_rays(br.case(0))
    inv = np.abs(1.0 / rays[:, 3:])
    assert (inv.max(axis=1) < 2.0 ** -126).mean() >= 0.5 and (inv.min(axis=1) >= 2.0 ** -126).mean() >= 0.1
    assert (inv < 2.0 ** -149).any()
