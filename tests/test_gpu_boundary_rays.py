"""The fp32 filters of the walk (mt_trace.h: Filter32, the block / super / subtree boxes rounded to nearest,
outside_on_axis) on the rays that can prove them wrong, on a real MI355X (-m gpu).

The filters may reject a box but never one the exact test accepts.  They can fail only where the exact slab interval is
almost empty and the fp32 copy of a plane differs from the fp64 plane; tests/boundary_rays.py makes both happen at once
(tests/test_boundary_rays_cpu.py asserts that it does), and goes to the filter's preconditions.  The reference for every
comparison is the oracle: first-hit primitive, distance and hit point bit for bit, and the work counters.  mt_tests is
the sharp one: a triangle whose box was filtered wrongly drops one count even where the triangle itself would have been
missed.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import boundary_rays as br  # noqa: E402

import mythtracer_amd as M  # noqa: E402

PRUNED = ("box_tests", "node_visits", "tri_tests", "mt_tests")
ALL_MODES = (0, 1, 2, 3, 4, 5, 6, 7)


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"


def device_scene(tris):
    m = M.MythTracer()
    for k, v in enumerate(tris):
        m.add_triangle(v, None, mtl=-1, line_no=k)
    return m


def compare(m, rays, want, modes, exact_counters=(1, 2, 4, 7), what="", describe=None):
    """mt_intersect_rays in every mode of `modes` against the oracle's answers `want`, as
    test_random_triangle_soups_all_modes does: line everywhere, t and point bit for bit on hits and NaN on misses,
    mt_tests equal (>= in the automatic mode, which may look behind the reference's early exit), all four work counters
    equal in the modes that skip no subtree.  describe(r), where given, names ray r in the message of a wrong line."""
    abi, h = M.hip_abi(), m.device_scene()
    hit = want["line"] >= 0
    for mode in modes:
        abi.set_traversal_mode(h, mode)
        got = abi.intersect_rays(h, rays)
        tag = (what, mode)
        print("%s mode %d: %d of %d lines differ; mt_tests %d (oracle %d)"
              % (what, mode, int((got["line"] != want["line"]).sum()), len(rays), got["stats"]["mt_tests"],
                 want["counters"]["mt_tests"]))
        wrong = np.nonzero(got["line"] != want["line"])[0]
        assert len(wrong) == 0, (tag, "%d of %d lines wrong" % (len(wrong), len(rays)), "got line %d" % got["line"][wrong[0]],
                                 describe(int(wrong[0])) if describe else "ray %d" % wrong[0])
        assert np.array_equal(got["t"][hit], want["t"][hit]), tag
        assert np.array_equal(got["point"][hit], want["point"][hit]), tag
        assert np.isnan(got["t"][~hit]).all() and np.isnan(got["point"][~hit]).all(), tag
        if mode == 0:
            assert got["stats"]["mt_tests"] >= want["counters"]["mt_tests"], tag
        else:
            assert got["stats"]["mt_tests"] == want["counters"]["mt_tests"], tag
        if mode in exact_counters:
            assert {k: got["stats"][k] for k in PRUNED} == {k: want["counters"][k] for k in PRUNED}, tag
    abi.set_traversal_mode(h, 0)


@pytest.mark.parametrize("p,layout", [(0, 1), (1, 1), (1, 0), (2, 1)])
def test_rays_aimed_at_box_and_triangle_boundaries(p, layout):
    """8192 rays through box corners, box edges, vertices, triangle edges and node centres of a lattice soup at
    coordinates fp32 cannot hold, one direction component nudged by 0, +-2^-52 .. +-2^-18; half of them in waves of one
    sign octant, half in mixed waves (the filter's two forms).  Three quarters of them are decided within twice the
    filter's margin.  The octree of the second placement has 12 levels: both layouts of the deep walk."""
    c = br.case(p)
    assert (c["tree"]["depth"] >= 12) == (p == 1)
    m = device_scene(c["tris"])
    M.hip_abi().set_tuning(m.device_scene(), "DEEP_LAYOUT", float(layout))
    compare(m, c["rays"], c["want"], ALL_MODES, what="placement %d layout %d" % (p, layout))


@pytest.mark.parametrize("per_wave", [1, 3, 8, 9, 64])
def test_zero_component_rays_at_planes_fp32_cannot_hold(per_wave):
    """`per_wave` lanes of every wave run INSIDE an axis plane, at or next to a triangle-box or node plane p that is
    inexact in fp32: at p and its fp64 neighbours, at fl32(p), its fp32 neighbours and their fp64 neighbours, at
    p +- half an fp32 ulp.  The range rule for such rays (outside_on_axis) compares with fp32 copies rounded to
    nearest, widened by one ulp; the other lanes are regular boundary rays."""
    c = br.case(0)
    rays, special = br.zero_component_rays(c, per_wave)
    assert special.reshape(-1, 64).sum(axis=1).tolist() == [per_wave] * (len(rays) // 64)
    assert ((rays[special, 3:] == 0.0).sum(axis=1) == 1).all()
    want = c["oracle"].intersect(rays)
    share = (want["line"][special] >= 0).mean()
    print("%d zero-component rays, %.0f %% of them hit" % (special.sum(), 100 * share))
    assert share >= 0.25
    compare(device_scene(c["tris"]), rays, want, (0, 7, 1, 5), exact_counters=(7,), what="per_wave %d" % per_wave)


def test_filter_precondition_m_around_2_to_the_120():
    """E1.  Scene and origins times 2^60, directions times 2^-50 .. 2^-60: M = (bmax + |o|) |1/d| within a factor of two
    of 2^120, below it for whole waves, above it for whole waves, above it for one lane of a wave (which switches the
    wave's filter off), and mixed."""
    tris, rays, m = br.precondition_m_rays(br.case(0))
    want = br.oracle_scene(tris).intersect(rays)
    assert (want["line"] >= 0).mean() > 0.2
    compare(device_scene(tris), rays, want, ALL_MODES, what="E1")


def test_filter_precondition_reciprocal_beyond_fp32():
    """E2.  bmax + |o| < 2^-8 and direction lengths 2^-120 .. 2^-140: (float)(1/d) is infinite from |1/d| = 2^128 on
    while M can still be below 2^120.  Every determinant is below the triangle test's threshold, nothing is hit; the
    counters are the observable."""
    tris, rays = br.precondition_big_reciprocal_rays(br.case(2))
    want = br.oracle_scene(tris).intersect(rays)
    assert (want["line"] == -1).all() and want["counters"]["mt_tests"] > len(rays)
    compare(device_scene(tris), rays, want, ALL_MODES, what="E2")


def test_filter_precondition_reciprocal_below_fp32_normals():
    """E3.  Scene and origins times 2^60 and direction lengths 2^120 .. 2^150: (float)(1/d) is denormal or zero, its
    error no longer relative, with planes near 2^68."""
    tris, rays = br.precondition_small_reciprocal_rays(br.case(0))
    want = br.oracle_scene(tris).intersect(rays)
    assert (want["line"] >= 0).mean() > 0.2
    compare(device_scene(tris), rays, want, ALL_MODES, what="E3")
