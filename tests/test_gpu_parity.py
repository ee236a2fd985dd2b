"""Parity of the HIP path with the reference, on a real MI355X (-m gpu).

Checker: golden vectors produced by the reference itself (tests/golden/) and
the CPU oracle on the same inputs.  Bars: first-hit primitive, hit point,
distance and all work counters BIT-EXACT; RGB8 within 1 LSB per channel —
`pow` (mythtracer.cc:174) is the one operation whose GPU implementation (ocml)
is not bit-identical to glibc's, every other operation is IEEE-exact fp64 in
the reference's order.  In practice the frames come out identical; the tests
print the differing-pixel count and fail above 0.01 %.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import orclib
from conftest import GOLDEN, CORNELL

pytestmark = pytest.mark.gpu

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding, scenegen, tiling  # noqa: E402

CORNELL_CAM = (50, 50, -120, 0, 0, 0, 60)
CORNELL_LIGHTS = [(50, 90, 50, .3, .3, .3, 1, 1, 1, 1, 1, 1)]
RAY_KEYS = ("rays_primary", "rays_secondary", "rays_shadow")
ALL_KEYS = RAY_KEYS + ("box_tests", "node_visits", "tri_tests", "mt_tests", "shaded_hits")


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"


@pytest.fixture(params=["state_machine", "ray_pool", "hybrid", "auto"], autouse=True)
def engine(request):
    """Every test runs through both frame engines (include/mythtracer_hip.h,
    mt_scene_set_engine) and through the shipping default, the AUTOMATIC choice
    (probe_kernel first frame, the blocks-per-wave switch, cost words handed from
    one engine to the other): the per-lane state machine and the per-wave ray
    pool must give the same pixels, debug buffers and counters.  Selected through
    the API (mt_set_default_engine: scenes created from now on), not through the
    environment."""
    abi = M.hip_abi()
    abi.set_default_engine({"state_machine": 1, "ray_pool": 2, "hybrid": 3, "auto": 0}[request.param])
    yield request.param
    abi.set_default_engine(0)


PRUNED = ("box_tests", "node_visits", "tri_tests", "mt_tests")


def counters_match(got, want):
    """Default traversal mode: every ray count and shaded hit equals the oracle's.
    The four work counters (box / node / triangle-filter / Möller–Trumbore
    evaluations) are the traversal's OWN work there: subtrees a ray provably
    cannot hit are not visited, and the hit-set traversal may look at a node that
    lies behind the reference's early exit (never the other way round: every
    triangle the reference puts through Möller–Trumbore is put through it here).
    Mode 7 reproduces the reference's counts exactly: test_counters_equal_the_oracle."""
    assert {k: v for k, v in got.items() if k not in PRUNED} == {k: v for k, v in want.items() if k not in PRUNED}
    if "mt_tests" in got and "mt_tests" in want:
        assert got["mt_tests"] >= want["mt_tests"], (got, want)


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def assert_rgb_close(got, want, what=""):
    """RGB tolerance: 1 LSB (pow), on at most 0.01 % of the pixels."""
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    n_diff = int((d != 0).any(axis=-1).sum())
    print("%s: %d of %d pixels differ, max |diff| %d" % (what, n_diff, d.shape[0] * d.shape[1], int(d.max(initial=0))))
    assert d.max(initial=0) <= 1, what
    assert n_diff <= max(1, d.shape[0] * d.shape[1] // 10000), what


RENDER_CASES = [("cornell_256", "cornell"), ("cornell_cam2_96x64", "cornell"),
                ("cornell_nolights_64", "cornell"), ("mini_320x180", "mini"),
                ("mini_nomtl_320x180", "mini_nomtl"), ("mini_chunk_101x67", "mini"),
                ("mini_1x1", "mini"), ("room_240x135", "room"),
                ("room_view_back", "room"), ("room_view_floor", "room"), ("room_view_down", "room"),
                ("room_view_axis", "room"),
                # the shadow loop restarts BEYOND an opaque decal 5e-6 behind a pane of glass -- the frame the
                # reference renders has no shadow there (tests/test_oracle_golden.py says why that rules the early-out out)
                ("f2_decal_96x64", "f2_decal"),
                # round 4's two more scenes (profiles/README.md): 770 720 triangles in an octree of 16 levels, made by the
                # reference; the room with map_Ka textures, made by the ORACLE (Texture::GetColorAt: parity unpinned)
                ("loft_240x135", "loft"), ("room_tex_240x135", "room_tex"),
                # the loft with finer shelves: an octree of 20 levels (the third word of the walk's child bytes), reference-made
                ("loft_fine_240x135", "loft_fine")]


@pytest.mark.parametrize("case,scene", RENDER_CASES)
def test_facade_render_matches_reference_golden(case, scene, scenes):
    """MythTracer::RayTrace(WorkChunk*) through the facade vs the reference's output."""
    g = load(case)
    m = M.MythTracer(scenes[scene])
    m.set_lights(g["lights"].reshape(-1, 12))
    W, H = (int(v) for v in g["image"])
    r = m.render(g["cam"], W, H, chunk=tuple(int(v) for v in g["chunk"]), debug=True)
    assert_rgb_close(r["rgb"], g["rgb"], case)
    assert np.array_equal(r["line"], g["line"])
    assert np.array_equal(r["point"], g["point"], equal_nan=True)


@pytest.mark.parametrize("scene,size", [("cornell", (128, 96)), ("mini", (160, 90)), ("room", (96, 54))])
def test_counters_equal_the_oracle(scene, size, scenes):
    """Every IntersectRay / box / triangle / Möller–Trumbore evaluation the
    reference performs is performed, no more, no less."""
    W, H = size
    cam, lights = (CORNELL_CAM, CORNELL_LIGHTS) if scene == "cornell" else (scenegen.ROOM_CAMERA, scenegen.ROOM_LIGHTS)
    m = M.MythTracer(scenes[scene])
    m.set_lights(lights)
    o = orclib.OracleScene(scenes[scene])
    o.set_lights(lights)
    M.hip_abi().set_traversal_mode(m.device_scene(), 7)  # visit every subtree, like the reference
    g, r = m.render(cam, W, H, debug=True), o.render(cam, W, H, debug=True)
    assert g["counters"] == r["counters"]
    assert np.array_equal(g["line"], r["line"])
    assert np.array_equal(g["point"], r["point"], equal_nan=True)
    assert_rgb_close(g["rgb"], r["rgb"], scene)
    M.hip_abi().set_traversal_mode(m.device_scene(), 0)
    g0 = m.render(cam, W, H, debug=True)
    counters_match(g0["counters"], r["counters"])
    assert np.array_equal(g0["rgb"], g["rgb"]) and np.array_equal(g0["line"], g["line"])


@pytest.mark.parametrize("chunk", [(0, 0, 1, 1), (159, 89, 1, 1), (3, 5, 7, 5), (150, 0, 10, 90),
                                   (0, 80, 160, 10), (8, 8, 8, 8), (13, 27, 65, 33)])
def test_ragged_chunks(chunk, scenes):
    m = M.MythTracer(scenes["mini"])
    m.set_lights(scenegen.ROOM_LIGHTS)
    o = orclib.OracleScene(scenes["mini"])
    o.set_lights(scenegen.ROOM_LIGHTS)
    g = m.render(scenegen.ROOM_CAMERA, 160, 90, chunk=chunk, debug=True)
    r = o.render(scenegen.ROOM_CAMERA, 160, 90, chunk=chunk, debug=True)
    assert g["rgb"].shape == (chunk[3], chunk[2], 3)
    assert_rgb_close(g["rgb"], r["rgb"], str(chunk))
    assert np.array_equal(g["line"], r["line"])
    counters_match(g["counters"], r["counters"])


def test_cost_history_scheduling_changes_nothing(scenes):
    """A repeated launch of the same geometry is scheduled from the block costs
    measured in the previous one (one kernel, longest blocks first, some as
    quarters with four lanes per pixel): same image, same counters as the
    first, material-classified launch and as a scene with the history off."""
    abi = M.hip_abi()
    m = M.MythTracer(scenes["mini"])
    h = abi.scene_create(m.flatten())
    try:
        abi.set_lights(h, scenegen.ROOM_LIGHTS)
        sens = binding.sensor(scenegen.ROOM_CAMERA, 320, 180)
        g = load("mini_320x180")
        first = abi.render_chunk(h, sens, 320, 180)
        assert_rgb_close(first["rgb"], g["rgb"], "first launch")
        for i in range(6):  # (blocks change their form -- one unit / four quarters -- between these launches: the forecast's per-block ratio)
            again = abi.render_chunk(h, sens, 320, 180)
            assert np.array_equal(again["rgb"], first["rgb"]), i
            # (which subtrees get skipped depends on the rays that share a wave,
            # so the three pruned counters may differ between schedules)
            counters_match({k: again["stats"][k] for k in ALL_KEYS if k not in PRUNED},
                           {k: first["stats"][k] for k in ALL_KEYS if k not in PRUNED})
        part = abi.render_chunk(h, sens, 320, 180, chunk=(16, 8, 200, 120))  # other geometry: no history
        assert np.array_equal(part["rgb"], first["rgb"][8:128, 16:216])
        part2 = abi.render_chunk(h, sens, 320, 180, chunk=(16, 8, 200, 120))  # ... and now with
        assert np.array_equal(part2["rgb"], part["rgb"])
        abi.set_scheduling(h, False)
        for i in range(2):
            off = abi.render_chunk(h, sens, 320, 180)
            assert np.array_equal(off["rgb"], first["rgb"])
        abi.set_scheduling(h, True)
        abi.set_lights(h, [scenegen.ROOM_LIGHTS[0]] * 6)  # more lights than roles in a quad
        a = abi.render_chunk(h, sens, 320, 180)
        b = abi.render_chunk(h, sens, 320, 180)
        assert np.array_equal(a["rgb"], b["rgb"])
        assert all(a["stats"][k] == b["stats"][k] for k in ALL_KEYS if k not in PRUNED)
        abi.set_lights(h, [])
        a = abi.render_chunk(h, sens, 320, 180)
        b = abi.render_chunk(h, sens, 320, 180)
        assert np.array_equal(a["rgb"], b["rgb"])
    finally:
        abi.scene_destroy(h)


@pytest.mark.parametrize("groups", [1, 3, 64, 256])
def test_work_order_on_any_number_of_workgroups(groups, scenes, engine):
    """The work order of a launch with measured costs (mt_order.h: forecast, counting sort over (region or engine part,
    cost bucket), scatter -- three kernels on MT_TUNE_ORDER_GROUPS workgroups, every thread for its own blocks) with one,
    an odd number, the default and the largest number of workgroups, with one work order per XCD and with one for the
    chip: every unit of every block exactly once -- same pixels and ray counts as the first, unordered launch -- for a
    camera at rest, a moved one (re-projected forecast) and a chunk (another geometry).  (Launches of many tiles:
    test_cost_balanced_tile_ownership.)"""
    abi = M.hip_abi()
    m = M.MythTracer(scenes["room"])
    h = abi.scene_create(m.flatten())
    try:
        abi.set_lights(h, scenegen.ROOM_LIGHTS)
        abi.set_tuning(h, "ORDER_GROUPS", float(groups))
        W, H = 400, 224
        for queues in (2.0, 0.0, 1.0):
            abi.set_tuning(h, "XCD_QUEUES", queues)
            cams = [scenegen.ROOM_CAMERA, scenegen.ROOM_CAMERA, scenegen.ROOM_CAMERA]
            moved = list(scenegen.ROOM_CAMERA); moved[4] += 3.0
            first = {}
            for cam in cams + [moved, moved, scenegen.ROOM_CAMERA]:
                r = abi.render_chunk(h, binding.sensor(cam, W, H), W, H)
                key = tuple(cam)
                if key not in first:
                    first[key] = r  # (no cost history for this camera's first frame after set_tuning: the unordered launch)
                assert np.array_equal(r["rgb"], first[key]["rgb"]), (groups, queues)
                assert {k: r["stats"][k] for k in ALL_KEYS if k not in PRUNED} == {k: first[key]["stats"][k] for k in ALL_KEYS if k not in PRUNED}
            full = first[tuple(scenegen.ROOM_CAMERA)]["rgb"]
            for _ in range(3):
                part = abi.render_chunk(h, binding.sensor(scenegen.ROOM_CAMERA, W, H), W, H, chunk=(40, 16, 301, 150))
                assert np.array_equal(part["rgb"], full[16:166, 40:341]), (groups, queues)
    finally:
        abi.scene_destroy(h)


def test_state_machine_cells_for_blocks_with_zero_component_rays(scenes):
    """A camera on an axis has a pixel column whose primary rays have a zero direction component (exact, lane-serial
    descent: a pass costs with the number of such rays in it).  The state machine hands such blocks out as sixteen 2x2
    cells, four lanes per pixel, when even their quarters would be the launch's longest units (MT_TUNE_SM_CELL_SHARE;
    mt_order.h).  Forced here for every block of the column (and, with a tiny cutting share, quarters for nearly every
    other block): same pixels, debug-free counters and ray counts as the unordered first launch and as the golden."""
    abi = M.hip_abi()
    m = M.MythTracer(scenes["room"])
    h = abi.scene_create(m.flatten())
    try:
        abi.set_engine(h, 1)
        abi.set_lights(h, scenegen.ROOM_LIGHTS)
        g = load("room_240x135")
        W, H = 240, 135   # (odd height, even width: the column x = 120 holds the zero-component rays)
        sens = binding.sensor(scenegen.ROOM_CAMERA, W, H)
        first = abi.render_chunk(h, sens, W, H)
        assert_rgb_close(first["rgb"], g["rgb"], "first launch")
        for share, quad in ((1e-6, 0.05), (1e-6, 0.95), (0.8, 0.95)):
            abi.set_tuning(h, "SM_CELL_SHARE", share)
            abi.set_tuning(h, "QUAD_SHARE", quad)
            for launch in range(4):  # (the first one after set_tuning has no cost history)
                r = abi.render_chunk(h, sens, W, H)
                assert np.array_equal(r["rgb"], first["rgb"]), (share, quad, launch)
                assert {k: r["stats"][k] for k in ALL_KEYS if k not in PRUNED} == {k: first["stats"][k] for k in ALL_KEYS if k not in PRUNED}, (share, quad, launch)
            # a ragged chunk through the column: cells at the clipped edge
            part = abi.render_chunk(h, sens, W, H, chunk=(101, 3, 37, 129))
            part = abi.render_chunk(h, sens, W, H, chunk=(101, 3, 37, 129))
            assert np.array_equal(part["rgb"], first["rgb"][3:132, 101:138]), (share, quad)
    finally:
        abi.scene_destroy(h)


def test_bad_chunks_are_rejected(scenes):
    m = M.MythTracer(scenes["cornell"])
    for chunk in [(-1, 0, 4, 4), (0, 0, 0, 4), (60, 60, 8, 8), (0, 0, 65, 1)]:
        with pytest.raises(RuntimeError):
            m.render(CORNELL_CAM, 64, 64, chunk=chunk)


def test_image_overload(scenes):
    """MythTracer::RayTrace(int, int, Camera*, vector*) == the full-frame chunk."""
    m = M.MythTracer(scenes["cornell"])
    m.set_lights(CORNELL_LIGHTS)
    a = m.render_image(CORNELL_CAM, 96, 80)
    b = m.render(CORNELL_CAM, 96, 80)["rgb"]
    assert np.array_equal(a, b)


@pytest.mark.parametrize("case,scene", [("rays_cornell", "cornell"), ("rays_mini", "mini"), ("rays_room", "room")])
def test_c_abi_intersect_rays_match_reference(case, scene, scenes):
    """mt_scene_create + mt_intersect_rays called directly (no facade in
    between) vs OctTree::IntersectRay of the reference, including axis-parallel
    rays and origins on box planes (the NaN / infinity paths)."""
    g = load(case)
    abi = M.hip_abi()
    flat = M.MythTracer(scenes[scene]).flatten()
    h = abi.scene_create(flat)
    try:
        for mode in (0, 1, 2, 3, 4, 5, 6, 7):
            abi.set_traversal_mode(h, mode)
            r = abi.intersect_rays(h, g["rays"])
            assert np.array_equal(r["line"], g["line"]), mode
            hit = g["line"] >= 0
            assert np.array_equal(r["t"][hit], g["t"][hit]), mode
            assert np.array_equal(r["point"][hit], g["point"][hit]), mode
            assert np.isnan(r["t"][~hit]).all()
    finally:
        abi.scene_destroy(h)


@pytest.mark.parametrize("per_wave", [1, 3, 8, 9, 64])
def test_a_few_rays_with_a_zero_direction_component_per_wave(per_wave, scenes):
    """Rays IN the plane x = 200 of the room (one zero direction component: the exact path behind the hit-set walk),
    `per_wave` of them in every wave of 64, the rest missing the scene: up to eight such lanes have the lists of their
    small nodes scanned together, packed over the wave (scan_small_packed_call); nine and more scan lane by lane.
    Every hit equals the oracle's, in every traversal mode, with the oracle's counters in the un-pruned one."""
    rnd = np.random.RandomState(per_wave)
    n_waves = 6
    rays = np.zeros((64 * n_waves, 6))
    rays[:, :3] = 1.0e6
    rays[:, 3:] = (0.6, 0.64, 0.48)  # away from the scene
    for w in range(n_waves):
        k = w * 64 + rnd.permutation(64)[:per_wave]
        ang = rnd.uniform(-0.7, 0.7, per_wave)
        rays[k, 0] = 200.0
        rays[k, 1] = rnd.choice([120.0, 60.0, 200.0], per_wave)
        rays[k, 2] = rnd.choice([20.0, 200.0], per_wave)
        d = np.stack([np.zeros(per_wave), np.sin(ang), np.cos(ang)], axis=1)
        if w % 2:
            d = d[:, [1, 0, 2]]; rays[k, 0] = rnd.uniform(50.0, 350.0, per_wave); rays[k, 1] = 120.0  # ... or in y = 120
        rays[k, 3:] = d
    o = orclib.OracleScene(scenes["room"])
    want = o.intersect(rays)
    abi = M.hip_abi()
    h = abi.scene_create(M.MythTracer(scenes["room"]).flatten())
    try:
        for mode in (0, 7, 1, 5):
            abi.set_traversal_mode(h, mode)
            r = abi.intersect_rays(h, rays)
            assert np.array_equal(r["line"], want["line"]), mode
            hit = want["line"] >= 0
            assert hit.sum() >= per_wave * n_waves // 2
            assert np.array_equal(r["t"][hit], want["t"][hit]), mode
            assert np.array_equal(r["point"][hit], want["point"][hit]), mode
            if mode == 7:
                for k in ("box_tests", "node_visits", "tri_tests", "mt_tests"):
                    assert r["stats"][k] == want["counters"][k], (k, r["stats"][k], want["counters"][k])
    finally:
        abi.scene_destroy(h)


def test_c_abi_render_direct_and_modes(scenes):
    """mt_render_chunk called directly; all traversal modes give the same image,
    debug buffer, ray counts and Möller–Trumbore counts.  The modes that skip no
    subtree (1, 2, 4, 7) also reproduce the oracle's box / node / triangle test
    counts; the others visit fewer nodes, never more."""
    abi = M.hip_abi()
    m = M.MythTracer(scenes["mini"])
    h = abi.scene_create(m.flatten())
    try:
        abi.set_lights(h, scenegen.ROOM_LIGHTS)
        sens = binding.sensor(scenegen.ROOM_CAMERA, 200, 112)
        o = orclib.OracleScene(scenes["mini"])
        o.set_lights(scenegen.ROOM_LIGHTS)
        w = o.render(scenegen.ROOM_CAMERA, 200, 112, debug=True)
        base = None
        pruned = ("box_tests", "node_visits", "tri_tests")
        for mode in (7, 0, 1, 2, 3, 4, 5, 6, 0):
            abi.set_traversal_mode(h, mode)
            r = abi.render_chunk(h, sens, 200, 112, debug=True)
            key = {k: r["stats"][k] for k in ALL_KEYS}
            if base is None:
                base = (r["rgb"], r["line"], r["point"], key)
                assert_rgb_close(base[0], w["rgb"], "direct")
                assert key == w["counters"] and np.array_equal(base[1], w["line"])
            else:
                assert np.array_equal(r["rgb"], base[0]) and np.array_equal(r["line"], base[1]), mode
                assert np.array_equal(r["point"], base[2], equal_nan=True), mode
                if mode in (1, 2, 4, 7):
                    assert key == base[3], mode
                elif mode == 0:  # the automatic mode's work counters are its own (counters_match)
                    counters_match(key, base[3])
                    assert key["node_visits"] < base[3]["node_visits"], mode
                else:
                    assert all(key[k] == base[3][k] for k in ALL_KEYS if k not in pruned), mode
                    assert all(0 < key[k] <= base[3][k] for k in pruned), mode
                    assert key["node_visits"] < base[3]["node_visits"], mode
    finally:
        abi.scene_destroy(h)


@pytest.mark.parametrize("depth", [0, 1, 2, 4, 5, 7])
def test_recursion_depth_parameter(depth, scenes):
    m = M.MythTracer(scenes["mini"])
    m.set_lights(scenegen.ROOM_LIGHTS)
    m.set_max_level(depth)
    o = orclib.OracleScene(scenes["mini"])
    o.set_lights(scenegen.ROOM_LIGHTS)
    g = m.render(scenegen.ROOM_CAMERA, 128, 72)
    r = o.render(scenegen.ROOM_CAMERA, 128, 72, max_level=depth)
    counters_match(g["counters"], r["counters"])
    assert_rgb_close(g["rgb"], r["rgb"], "depth %d" % depth)


def test_lights_are_reread_every_frame(scenes):
    """main_local.cc:79-110 rewrites scene.lights before every frame."""
    m = M.MythTracer(scenes["cornell"])
    o = orclib.OracleScene(scenes["cornell"])
    for lights in (CORNELL_LIGHTS, [], [(20, 50, 20, .1, .1, .1, .5, .5, .9, 1, 1, 1), (80, 80, 30, 0, 0, 0, .9, .2, .2, .3, .3, .3)],
                   [CORNELL_LIGHTS[0]] * 9):
        m.set_lights(lights)
        o.set_lights(lights)
        g, r = m.render(CORNELL_CAM, 64, 64), o.render(CORNELL_CAM, 64, 64)
        counters_match(g["counters"], r["counters"])
        assert_rgb_close(g["rgb"], r["rgb"], "%d lights" % len(lights))


def _both():
    return M.MythTracer(), orclib.OracleScene()


def _render_both(m, o, cam, W, H, lights):
    m.set_lights(lights)
    o.set_lights(lights)
    g, r = m.render(cam, W, H, debug=True), o.render(cam, W, H, debug=True)
    counters_match(g["counters"], r["counters"])
    assert np.array_equal(g["line"], r["line"])
    assert np.array_equal(g["point"], r["point"], equal_nan=True)
    assert_rgb_close(g["rgb"], r["rgb"])
    return g


@pytest.mark.parametrize("ext,jit,depth,layout", [(0.08, 0.015, 10, 1), (0.04, 0.008, 11, 1), (0.02, 0.004, 12, 1), (0.02, 0.004, 12, 0),
                                                   (0.01, 0.002, 13, 1), (0.01, 0.002, 13, 0),
                                                   (0.005, 0.001, 14, 1), (0.0012, 0.00025, 16, 1), (0.0012, 0.00025, 16, 0),
                                                   (0.0006, 0.00012, 17, 1), (0.0006, 0.00012, 17, 0),
                                                   (0.0003, 0.00006, 18, 1), (0.0003, 0.00006, 18, 0), (0.00004, 0.000008, 21, 1),
                                                   (0.000005, 0.000001, 24, 1), (0.0000025, 0.0000005, 25, 1)])
def test_deep_octrees(ext, jit, depth, layout):
    """A tight cluster of small triangles in a big room makes the octree deep.  Up to 11 levels the hit-set walk keeps
    all its frames in LDS; from 12 levels on the DEEP instantiations of the kernels (layout 1, the default) keep ten
    levels' frames there and the rest -- and the ordered descent's stack -- in global memory, with a third word of
    per-level child bytes for levels 16-23: the walk takes trees of up to 24 levels.  Layout 0 (MT_TUNE_DEEP_LAYOUT off)
    is round 3's: everything in LDS, the walk up to 16 levels; beyond (18 with layout 0, 25 with either) every ray takes
    the ordered descent with its per-lane stack.  Same pixels, hit points and counters as the oracle."""
    rnd = scenegen.SplitMix64(77)
    m, o = _both()
    tris = [[[0, 0, 0], [64, 0, 0], [0, 0, 64]], [[64, 0, 64], [0, 0, 64], [64, 0, 0]]]  # a floor
    for k in range(120):
        c = [20.0 + rnd.rng(0, ext), 3.0 + rnd.rng(0, ext), 30.0 + rnd.rng(0, ext)]
        tris.append([[c[a] + rnd.rng(-jit, jit) for a in range(3)] for _ in range(3)])
    for k in range(200):
        c = [rnd.rng(4, 60), rnd.rng(0.5, 6), rnd.rng(4, 60)]
        tris.append([[c[a] + rnd.rng(-1.5, 1.5) for a in range(3)] for _ in range(3)])
    for s in (m, o):
        s.add_material("a", (.2, .2, .2), (.7, .6, .5), (.3, .3, .3), ns=6, refl=0.2)
        for k, v in enumerate(tris):
            s.add_triangle(v, None, mtl=0, line_no=k)
    assert o.tree()["depth"] == depth
    M.hip_abi().set_tuning(m.device_scene(), "DEEP_LAYOUT", float(layout))
    lights = [(30, 40, 20, .2, .2, .2, .8, .8, .8, .4, .4, .4)]
    _render_both(m, o, (19.0, 8.0, 12.0, 15.0, 0.0, 0.0, 70.0), 96, 64, lights)
    g = _render_both(m, o, (20.0 + ext / 2, 3.0 + ext / 2, 29.9, 0.0, 0.0, 0.0, min(8.0, 800.0 * ext)), 64, 64, lights)  # straight at the cluster
    if ext >= 0.005:  # (the smallest clusters hide behind one of the scattered triangles from this viewpoint)
        assert ((g["line"] >= 2) & (g["line"] < 122)).mean() > 0.2
    else:
        rays = []
        for i in range(256):  # from the +z side through a grid of points inside the cluster
            tgt = [20.0 + ext * (0.1 + 0.8 * (i % 16) / 15.0), 3.0 + ext * (0.1 + 0.8 * (i // 16) / 15.0), 30.0 + ext * 0.5]
            org = [tgt[0] + 0.3 * (i % 5 - 2), tgt[1] + 0.2 * (i % 3), tgt[2] + 2.0]
            rays.append(org + [tgt[a] - org[a] for a in range(3)])
        far = max(2.0, 4e-8 / (jit * jit))  # the triangle test drops |det| < 1e-8: a unit direction never hits triangles
        for i in range(240):                # this small, a direction of this length does (the reference normalises nothing)
            t = tris[2 + i % 120]
            tgt = [(t[0][a] + t[1][a] + t[2][a]) / 3.0 for a in range(3)]
            d = [0.3 * (i % 5 - 2), 1.0, 0.2 * (i % 3 - 1)]
            org = [tgt[a] + far * d[a] for a in range(3)]
            rays.append(org + [tgt[a] - org[a] for a in range(3)])
        rays = np.array(rays)
        want = o.intersect(rays)
        got = M.hip_abi().intersect_rays(m.device_scene(), rays)
        assert np.array_equal(got["line"], want["line"])
        assert np.array_equal(got["point"], want["point"], equal_nan=True)
        assert ((want["line"][256:] >= 2) & (want["line"][256:] < 122)).mean() > 0.3  # rays into the cluster: the deepest levels


def test_reference_octtree_test_scenario():
    """VerStarting/octtree_test.cc:14-73 (with the CacheAABB call it forgot):
    front ray -> tr0, back ray -> tr1, far-away ray -> nothing."""
    m = M.MythTracer()
    m.add_triangle([[1, 1, 0], [1, 0, 0], [0, 0, 0]], line_no=0)
    m.add_triangle([[1, 1, 1], [1, 0, 1], [0, 0, 1]], line_no=1)
    r = m.intersect([[0.9, 0.9, -10, 0, 0, 1], [0.9, 0.9, 10, 0, 0, -1], [5, 5, 5, 0, 0, 1]])
    assert list(r["tri"]) == [0, 1, -1]
    assert r["t"][0] == 10.0 and r["t"][1] == 9.0 and np.isnan(r["t"][2])


def test_empty_scene():
    m, o = _both()
    g = _render_both(m, o, (0, 0, -5, 0, 0, 0, 60), 16, 16, CORNELL_LIGHTS)
    assert not g["rgb"].any() and (g["line"] == -1).all()


def test_ties_degenerates_and_missing_normals():
    """Coincident triangles (equal distance: the LATER one wins, octtree.cc:186-195),
    zero-area triangles (NaN normal -> NaN colour -> 0), triangles without
    normals (N = 0), and more than 16 of them so that the tree splits."""
    m, o = _both()
    mats = [("a", (.8, .2, .2)), ("b", (.2, .8, .2)), ("c", (.2, .2, .8))]
    for s in (m, o):
        for name, c in mats:
            s.add_material(name, c, c, (.3, .3, .3), ns=8)
        n = [[0, 0, -1]] * 3
        k = 0
        for j in range(5):
            for i in range(5):
                quad = [[i * 2.0, j * 2.0, 5], [i * 2.0 + 2, j * 2.0, 5], [i * 2.0, j * 2.0 + 2, 5]]
                s.add_triangle(quad, n, mtl=k % 3, line_no=k)
                s.add_triangle(quad, n, mtl=(k + 1) % 3, line_no=100 + k)  # coincident twin
                k += 1
        s.add_triangle([[1, 1, 4], [1, 1, 4], [1, 1, 4]], n, mtl=0, line_no=900)      # a point
        s.add_triangle([[2, 2, 3], [4, 4, 3], [3, 3, 3]], n, mtl=1, line_no=901)      # a segment
        s.add_triangle([[6, 1, 4.5], [9, 1, 4.5], [6, 4, 4.5]], None, mtl=2, line_no=902)  # no normals
        s.add_triangle([[1, 6, 4.5], [4, 6, 4.5], [1, 9, 4.5]], n, mtl=-1, line_no=903)    # no material
    lights = [(5, 5, -8, .2, .2, .2, .8, .8, .8, .5, .5, .5)]
    g = _render_both(m, o, (5, 5, -6, 0, 0, 0, 80), 96, 96, lights)
    assert (g["line"] >= 100).any()  # twins are visible: the later coincident triangle won


@pytest.mark.parametrize("seed", [1, 2, 3] + list(range(50, 50 + int(os.environ.get("MT_FUZZ_SEEDS", "0")))))
def test_random_triangle_soups_all_modes(seed):
    """Random clustered triangle soups (big straddlers + many small triangles, on
    an integer lattice so that coincident planes, shared edges and exact ties are
    common) against random, axis-parallel, one-zero-component and on-plane rays:
    OctTree::IntersectRay on the GPU in every traversal mode vs the oracle."""
    rnd = scenegen.SplitMix64(1000 + seed)
    m, o = _both()
    tris = []
    for k in range(1500):
        big = k % 37 == 0
        c = [rnd.rng(0, 64) for _ in range(3)]
        ext = 40.0 if big else 3.0
        v = [[float(round(c[a] + rnd.rng(-ext, ext))) for a in range(3)] for _ in range(3)]
        tris.append(v)
    for s in (m, o):
        for k, v in enumerate(tris):
            s.add_triangle(v, None, mtl=-1, line_no=k)
    rays = []
    for i in range(4096):
        org = [rnd.rng(-20, 90) for _ in range(3)]
        kind = i % 8
        if kind == 0:    # axis-parallel
            d = [0.0, 0.0, 0.0]
            d[i // 8 % 3] = 1.0 if (i // 24) % 2 else -1.0
        elif kind == 1:  # exactly one zero component, origin on a lattice plane
            d = [rnd.rng(-1, 1) for _ in range(3)]
            a = i // 8 % 3
            d[a] = 0.0
            org[a] = float(round(org[a]))
        elif kind == 2:  # origin on lattice planes
            org = [float(round(x)) for x in org]
            d = [rnd.rng(-1, 1) for _ in range(3)]
        elif kind == 3:  # lattice origin, diagonal direction with power-of-two ratios: regular rays whose
            #              entry distances into sibling boxes tie exactly (order by index, octtree.cc:213-216)
            org = [float(round(x)) for x in org]
            d = [(1.0 if rnd.rng(0, 1) < 0.5 else -1.0) * (1.0, 2.0, 4.0)[int(rnd.rng(0, 3)) % 3] for _ in range(3)]
        elif kind == 4:  # from one lattice point towards another, no zero component
            org = [float(round(x)) for x in org]
            d = [float(round(rnd.rng(1, 40))) * (1.0 if rnd.rng(0, 1) < 0.5 else -1.0) for _ in range(3)]
        else:
            tgt = [rnd.rng(0, 64) for _ in range(3)]
            d = [tgt[a] - org[a] for a in range(3)]
        n = sum(x * x for x in d) ** 0.5 or 1.0
        rays.append(org + [x / n for x in d])
    rays = np.array(rays)
    want = o.intersect(rays)
    hit = want["line"] >= 0
    assert 0.2 < hit.mean() < 0.98
    abi = M.hip_abi()
    h = m.device_scene()
    for mode in (0, 1, 2, 3, 4, 5, 6, 7):
        abi.set_traversal_mode(h, mode)
        got = abi.intersect_rays(h, rays)
        assert np.array_equal(got["line"], want["line"]), mode
        assert np.array_equal(got["t"][hit], want["t"][hit]), mode
        assert np.array_equal(got["point"][hit], want["point"][hit]), mode
        if mode == 0:  # the automatic mode may look behind the reference's early exit (counters_match)
            assert got["stats"]["mt_tests"] >= want["counters"]["mt_tests"], mode
        else:
            assert got["stats"]["mt_tests"] == want["counters"]["mt_tests"], mode
        if mode in (1, 2, 4, 7):
            assert all(got["stats"][k] == want["counters"][k] for k in PRUNED), mode


def test_transparency_shadow_loop_and_refraction():
    """Stacked glass panes between the floor and the light: the shadow loop
    walks through them (mythtracer.cc:94-156), light power decays below the
    0.001 threshold behind enough panes, refraction recurses with in_object."""
    m, o = _both()
    for s in (m, o):
        s.add_material("floor", (.7, .7, .7), (.7, .7, .7), (.1, .1, .1), ns=5, refl=0.3)
        s.add_material("glass", (.05, .05, .05), (.05, .05, .05), (.6, .6, .6), ns=40, tr=0.25, tf=(.5, .6, .7), ni=1.5)
        s.add_material("dark", (.05, .05, .05), (.05, .05, .05), (.6, .6, .6), ns=40, tr=0.02, tf=(.5, .5, .5), ni=1.5)
        up = [[0, 1, 0]] * 3
        k = 0
        for (x0, z0) in [(-20, -20)]:
            s.add_triangle([[x0, 0, z0], [x0 + 40, 0, z0], [x0, 0, z0 + 40]], up, mtl=0, line_no=k); k += 1
            s.add_triangle([[x0 + 40, 0, z0 + 40], [x0, 0, z0 + 40], [x0 + 40, 0, z0]], up, mtl=0, line_no=k); k += 1
        for i, y in enumerate([2, 3, 4, 5, 6, 7, 8, 9]):
            mt_ = 1 if i < 6 else 2
            w = 10 - i
            s.add_triangle([[-w, y, -w], [w, y, -w], [-w, y, w]], up, mtl=mt_, line_no=k); k += 1
            s.add_triangle([[w, y, w], [-w, y, w], [w, y, -w]], up, mtl=mt_, line_no=k); k += 1
    lights = [(0, 30, 0, .1, .1, .1, 1, 1, 1, 1, 1, 1), (15, 6, -15, 0, 0, 0, .4, .4, .4, .2, .2, .2)]
    g = _render_both(m, o, (0, 14, -30, 22, 0, 0, 70), 128, 96, lights)
    assert g["counters"]["rays_shadow"] > 3 * g["counters"]["shaded_hits"]  # loops iterated
    assert g["counters"]["rays_secondary"] > 0


@pytest.mark.parametrize("seed", [11, 12, 13, 14, 15, 16] + list(range(100, 100 + int(os.environ.get("MT_FUZZ_SEEDS", "0")))))
def test_random_scenes_render_like_the_oracle(seed):
    """Random rooms: a floor and walls, clusters of random triangles (on a lattice:
    shared edges and planes, coincident twins), mirrors, glass and opaque
    materials, one to four lights, a random camera -- rendered with full
    recursion and compared with the oracle pixel for pixel (colour, first-hit
    triangle and hit point).  The traversal that decides every one of these rays
    is the hit-set walk; its candidate rule and its dropping of children are what
    this test is after.  (MT_FUZZ_SEEDS=n adds n more seeds; 1000 were run once -- 4018 cases with the ray soups -- all identical.)"""
    rnd = scenegen.SplitMix64(9000 + seed)
    m, o = _both()
    mats = [("matte", (.3, .3, .3), (.7, .6, .5), (.2, .2, .2), dict(ns=8)),
            ("mirror", (.1, .1, .1), (.2, .2, .2), (.8, .8, .8), dict(ns=60, refl=0.7)),
            ("glass", (.05, .05, .05), (.1, .1, .1), (.6, .6, .6), dict(ns=40, tr=0.4, tf=(.6, .7, .8), ni=1.4)),
            ("both", (.1, .1, .1), (.3, .3, .3), (.5, .5, .5), dict(ns=20, refl=0.4, tr=0.3, tf=(.8, .6, .6), ni=1.2))]
    tris = []
    S = 48.0
    quads = [([0, 0, 0], [S, 0, 0], [0, 0, S], [S, 0, S]), ([0, 0, S], [S, 0, S], [0, S, S], [S, S, S]),
             ([0, 0, 0], [0, 0, S], [0, S, 0], [0, S, S]), ([S, 0, 0], [S, S, 0], [S, 0, S], [S, S, S])]
    for a, b, c, d in quads:  # floor, back wall, side walls, each as a 4 x 4 grid
        for i in range(4):
            for j in range(4):
                def pt(u, v):
                    return [a[k] + (b[k] - a[k]) * u / 4 + (c[k] - a[k]) * v / 4 for k in range(3)]
                tris.append(([pt(i, j), pt(i + 1, j), pt(i, j + 1)], 0 if (i + j) % 3 else 1))
                tris.append(([pt(i + 1, j + 1), pt(i, j + 1), pt(i + 1, j)], 0))
    for cl in range(5):
        c = [rnd.rng(8, 40), rnd.rng(2, 20), rnd.rng(10, 40)]
        ext = rnd.rng(1.5, 6.0)
        mt = int(rnd.rng(0, 4)) % 4
        for k in range(int(rnd.rng(20, 90))):
            p0 = [float(round((c[a] + rnd.rng(-ext, ext)) * 2) / 2) for a in range(3)]
            v = [p0, [p0[a] + float(round(rnd.rng(-2, 2) * 2) / 2) for a in range(3)],
                 [p0[a] + float(round(rnd.rng(-2, 2) * 2) / 2) for a in range(3)]]
            tris.append((v, mt))
            if k % 17 == 0:
                tris.append((v, (mt + 1) % 4))  # a coincident twin with another material
    for s in (m, o):
        for name, ka, kd, ks, kw in mats:
            s.add_material(name, ka, kd, ks, **kw)
        for k, (v, mt) in enumerate(tris):
            s.add_triangle(v, None, mtl=mt, line_no=k)
    lights = [(rnd.rng(4, 44), rnd.rng(25, 45), rnd.rng(4, 44), .1, .1, .1, .7, .7, .7, .5, .5, .5)
              for _ in range(1 + seed % 4)]
    cam = (rnd.rng(10, 38), rnd.rng(6, 30), rnd.rng(-30, -4), rnd.rng(-5, 25), rnd.rng(-25, 25), rnd.rng(-10, 10), rnd.rng(50, 100))
    g = _render_both(m, o, cam, 112, 80, lights)
    assert (g["line"] >= 0).mean() > 0.1 and g["counters"]["rays_secondary"] > 0  # (the camera saw something)
    # Cameras that look straight along z: the centre pixel column and row shoot rays with a zero direction
    # component.  On a lattice plane (triangle boxes and octree planes AT the origin's coordinate: NaN in the
    # reference's slab tests) and off it (the other two axes decide: the culling of DevScene::deg_dirty_*).
    xl = float(round(cam[0] * 2) / 2)
    for x in (xl, xl + 0.125):
        _render_both(m, o, (x, float(round(cam[1])), cam[2], 0.0, 0.0, 0.0, 80.0), 64, 48, lights)


def test_materialless_occluder_is_opaque():
    """The reference dereferences shadow_primitive->mtl unconditionally
    (mythtracer.cc:121) and crashes when a material-less triangle shadows a
    material'd one; product and oracle both define that occluder as opaque."""
    m, o = _both()
    for s in (m, o):
        s.add_material("w", (.8, .8, .8), (.8, .8, .8), (0, 0, 0), ns=1)
        up = [[0, 1, 0]] * 3
        s.add_triangle([[-10, 0, -10], [10, 0, -10], [-10, 0, 10]], up, mtl=0, line_no=1)
        s.add_triangle([[10, 0, 10], [-10, 0, 10], [10, 0, -10]], up, mtl=0, line_no=2)
        s.add_triangle([[-2, 3, -2], [2, 3, -2], [-2, 3, 2]], up, mtl=-1, line_no=3)
    g = _render_both(m, o, (0, 8, -14, 30, 0, 0, 60), 64, 48, [(0, 10, 0, .1, .1, .1, 1, 1, 1, 0, 0, 0)])
    assert g["counters"]["rays_shadow"] > 0


def test_textured_material():
    """map_Ka path: GetUVW + Texture::GetColorAt on the device, RGB8 and f64
    texels.  Checked against the oracle's restatement of texture.cc:11-58,
    which is itself UNPINNED (texture.cc cannot be built without SDL2)."""
    rnd = np.random.RandomState(5)
    tex8 = rnd.randint(0, 256, size=(5, 7, 3)).astype(np.float64) / 255.0
    texf = rnd.rand(4, 4, 3)
    m, o = _both()
    for s in (m, o):
        a = s.add_material("a", (1, 1, 1), (.9, .9, .9), (.1, .1, .1), ns=3)
        b = s.add_material("b", (.9, .8, .7), (.5, .5, .5), (0, 0, 0), ns=1)
        s.set_material_texture(a, s.add_texture("t8", tex8))
        s.set_material_texture(b, s.add_texture("tf", texf))
        n = [[0, 0, -1]] * 3
        s.add_triangle([[-6, -4, 0], [0, -4, 0], [-6, 4, 0]], n, [[-0.5, -0.5, 0], [1.5, 0, 0], [0, 2.5, 0]], mtl=a, line_no=1)
        s.add_triangle([[0, -4, 0], [6, -4, 0], [0, 4, 0]], n, [[0, 0, 0], [1, 0, 0], [0, 1, 0]], mtl=b, line_no=2)
    flat = m.flatten()
    assert sorted(t["texels"].dtype.name for t in flat["textures"]) == ["float64", "uint8"]
    # the materials arrived as given (ka, kd, ks are distinct vectors)
    d, has_tex = m.get_material("b")
    assert has_tex and np.allclose(d[0:3], (.9, .8, .7)) and np.allclose(d[3:6], (.5, .5, .5))
    g = _render_both(m, o, (0, 0, -8, 0, 0, 0, 80), 96, 64, [(0, 0, -6, .4, .4, .4, .7, .7, .7, .2, .2, .2)])
    rgb = g["rgb"]
    assert rgb.max() > 100, "the textured triangles must not be black"
    # the colour depends on the texels: many distinct values on each triangle
    left, right = rgb[:, :48].reshape(-1, 3), rgb[:, 48:].reshape(-1, 3)
    assert len(np.unique(left, axis=0)) > 20 and len(np.unique(right, axis=0)) > 20


def test_axis_aligned_camera_hits_the_nan_paths():
    """Camera on a node plane looking straight down an axis: odd image size puts
    the centre pixel's ray exactly on (0,0,1); 1/0 = inf and 0*inf = NaN in
    the slab tests must behave as in the reference (exact mode)."""
    m = M.MythTracer(CORNELL)
    o = orclib.OracleScene(CORNELL)
    _render_both(m, o, (50, 50, -100, 0, 0, 0, 60), 33, 33, CORNELL_LIGHTS)
    _render_both(m, o, (50, 50, 50, 0, 90, 0, 90), 17, 17, CORNELL_LIGHTS)
    _render_both(m, o, (0, 0, 0, 0, 45, 0, 90), 9, 9, CORNELL_LIGHTS)


def test_big_frames_identical_to_reference(scenes):
    """BASELINE.json sizes: 1280x720 primary-only and 1920x1080 with 3 lights;
    sha256 of the whole frame + of the first-hit line buffer (reference run)."""
    import hashlib
    frames = json.load(open(os.path.join(GOLDEN, "frames.json")))
    for key, scene, (W, H) in [("room_nomtl_1280x720_d5", "room_nomtl", (1280, 720)),
                               ("room_1920x1080_d5", "room", (1920, 1080))]:
        m = M.MythTracer(scenes[scene])
        m.set_lights(scenegen.ROOM_LIGHTS)
        g = m.render(scenegen.ROOM_CAMERA, W, H, debug=True)
        sub = load(key + "_sub16")
        assert np.array_equal(g["line"][::16, ::16], sub["line"])
        assert np.array_equal(g["point"][::16, ::16], sub["point"], equal_nan=True)
        assert_rgb_close(g["rgb"][::16, ::16], sub["rgb"], key)
        assert hashlib.sha256(g["line"].astype("<i4").tobytes()).hexdigest() == frames[key]["line_sha256"]
        # the frame IS the reference's, byte for byte (pow -- the one operation whose implementation differs from glibc's --
        # has not produced a different byte on any frame of three rounds: no tolerance here)
        assert hashlib.sha256(g["rgb"].tobytes()).hexdigest() == frames[key]["sha256"], key


@pytest.mark.parametrize("scale,offset", [(1e-4, 0.0), (3e4, 0.0), (1.0, 2.5e6), (7.0, -9.1e5)])
def test_filters_stay_conservative_at_extreme_coordinates(scale, offset, scenes, tmp_path):
    """The fp32 pre-filter, the block boxes and the subtree boxes work on fp32
    copies of the scene: a scene scaled to 1e-4 / 3e4 of its size or moved
    millions of units from the origin (where fp32 resolves only ~0.25 units)
    must still give exactly the oracle's image, first hits and ray counts, and
    the same as the modes that use none of them."""
    src = open(scenes["mini"]).read().splitlines()
    out = []
    for ln in src:
        if ln.startswith("v "):
            x, y, z = (float(t) for t in ln.split()[1:4])
            out.append("v %.17g %.17g %.17g" % (x * scale + offset, y * scale + offset, z * scale + offset))
        else:
            out.append(ln)
    obj = tmp_path / "mini_moved.obj"
    obj.write_text("\n".join(out) + "\n")
    mtl = os.path.join(os.path.dirname(scenes["mini"]), "mini.mtl")
    if os.path.exists(mtl):
        (tmp_path / "mini.mtl").write_text(open(mtl).read())
    cam = list(scenegen.ROOM_CAMERA)
    cam[:3] = [c * scale + offset for c in cam[:3]]
    lights = [tuple(c * scale + offset for c in l[:3]) + tuple(l[3:]) for l in scenegen.ROOM_LIGHTS]
    m = M.MythTracer(str(obj))
    o = orclib.OracleScene(str(obj))
    m.set_lights(lights)
    o.set_lights(lights)
    g, r = m.render(cam, 160, 90, debug=True), o.render(cam, 160, 90, debug=True)
    assert np.array_equal(g["line"], r["line"])
    assert np.array_equal(g["point"], r["point"], equal_nan=True)
    assert_rgb_close(g["rgb"], r["rgb"], "scale %g offset %g" % (scale, offset))
    counters_match(g["counters"], r["counters"])
    assert (r["line"] >= 0).mean() > 0.5  # the camera still sees the scene
    abi = M.hip_abi()
    for mode in (4, 6, 7):
        abi.set_traversal_mode(m.device_scene(), mode)
        g2 = m.render(cam, 160, 90, debug=True)
        assert np.array_equal(g2["rgb"], g["rgb"]) and np.array_equal(g2["line"], g["line"]), mode


def test_unpacked_stack_frames(scenes):
    """Scenes whose node and triangle indices do not fit one word together use
    20-byte traversal stack frames instead of 16-byte ones; forced here for a
    small scene (mt_scene_set_tuning, MT_TUNE_PACKED_STACK = 0)."""
    g = load("mini_320x180")
    m = M.MythTracer(scenes["mini"])
    M.hip_abi().set_tuning(m.device_scene(), "PACKED_STACK", 0)
    m.set_lights(scenegen.ROOM_LIGHTS)
    a = m.render(scenegen.ROOM_CAMERA, 320, 180, debug=True)
    assert_rgb_close(a["rgb"], g["rgb"], "unpacked frames")
    assert np.array_equal(a["line"], g["line"])
    b = m.render(scenegen.ROOM_CAMERA, 320, 180)  # and through the cost-history path
    assert np.array_equal(b["rgb"], a["rgb"])


def test_4k_frame_contains_the_reference_1080p_frame(scenes):
    """BASELINE configs[4] size (3840x2160, 8 ranks).  Size-independent property:
    Sensor::GetRay (camera.cc:58-69) divides the same corner vectors by W and H,
    so the ray of 4K pixel (2x, 2y) is bit-for-bit the ray of 1080p pixel (x, y)
    (halving and doubling are exact) -- the even pixels of the 4K frame must be
    the reference's 1080p frame.  Rendered as 8 interleaved tile sets and
    blitted, as bench.py --gpus 8 does, and as one launch."""
    import hashlib
    import torch
    frames = json.load(open(os.path.join(GOLDEN, "frames.json")))
    abi = M.hip_abi()
    m = M.MythTracer(scenes["room"])
    m.set_lights(scenegen.ROOM_LIGHTS)
    h = m.device_scene()
    abi.set_lights(h, scenegen.ROOM_LIGHTS)
    W, H, T, world = 3840, 2160, 64, 8
    sens = binding.sensor(scenegen.ROOM_CAMERA, W, H)
    frame = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    for rank in range(world):
        f, s, n = tiling.rank_tiles(W, H, T, T, rank, world)
        slots = torch.zeros(n * tiling.slot_bytes(T, T), dtype=torch.uint8, device="cuda")
        abi.render_tiles_device(h, sens, W, H, T, T, f, s, n, 5, ctypes.c_void_p(slots.data_ptr()))
        abi.blit_tiles_device(h, W, H, T, T, f, s, n, ctypes.c_void_p(slots.data_ptr()),
                              ctypes.c_void_p(frame.data_ptr()))
    torch.cuda.synchronize()
    tiled = frame.cpu().numpy()
    single = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    for _ in range(2):  # the second launch is scheduled from the first one's block costs
        abi.render_chunk_device(h, sens, W, H, (0, 0, W, H), 5, ctypes.c_void_p(single.data_ptr()), None, None)
    torch.cuda.synchronize()
    st = abi.read_stats(h)
    assert np.array_equal(tiled, single.cpu().numpy())
    assert st["rays_primary"] == 2 * W * H + W * H  # two launches + the eight tile sets
    sha = hashlib.sha256(np.ascontiguousarray(tiled[::2, ::2]).tobytes()).hexdigest()
    assert sha == frames["room_1920x1080_d5"]["sha256"]
    # ... and the WHOLE frame is the one the compiled reference rendered at 3840x2160 (tests/golden/make_golden.py
    # --big4k: 185 s on 8 threads): SHA-256 of all 24.9 MB, and two every-16th-pixel sub-samples kept in full so that
    # a mismatch can be located (the second one on odd rows and columns only: pixels the 1080p frame does not hold)
    assert hashlib.sha256(tiled.tobytes()).hexdigest() == frames["room_3840x2160_d5"]["sha256"]
    assert np.array_equal(tiled[::16, ::16], load("room_3840x2160_d5_sub16")["rgb"])
    assert np.array_equal(tiled[11::16, 5::16], load("room_3840x2160_d5_sub16_odd")["rgb"])
    # ... and once more with the tiles dealt out BY COST (what bench.py --gpus 8 does from the second frame on): the
    # eight ranks' cost maps of a frame rendered that way, combined, order the tiles; every rank takes its deal
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    mw, mh = (W + 7) // 8, (H + 7) // 8
    total = tiling.tile_grid(W, H, T, T)[0] * tiling.tile_grid(W, H, T, T)[1]
    order = None
    for frame_no in range(2):
        frame.zero_()
        maps = []
        for rank in range(world):
            n = abi.dealt_tile_count(W, H, T, T, world, rank)
            lst = torch.zeros(n, dtype=torch.int32, device="cuda")
            assert abi.deal_tiles_device(h, vp(order) if order is not None else None, W, H, T, T, world, rank, vp(lst)) == n
            slots = torch.zeros(n * tiling.slot_bytes(T, T), dtype=torch.uint8, device="cuda")
            if order is not None:
                abi.import_costs_device(h, vp(comb), mw, mh)
            abi.render_tile_list_device(h, sens, W, H, T, T, vp(lst), n, 0, 5, vp(slots))
            abi.blit_tile_list_device(h, W, H, T, T, vp(lst), n, vp(slots), vp(frame))
            cm = torch.zeros((mh, mw), dtype=torch.int32, device="cuda")
            abi.export_costs_device(h, vp(cm), mw, mh)
            maps.append(cm)
        torch.cuda.synchronize()
        abi.read_stats(h)
        assert hashlib.sha256(frame.cpu().numpy().tobytes()).hexdigest() == frames["room_3840x2160_d5"]["sha256"], frame_no
        comb = torch.stack(maps).max(dim=0).values.contiguous()
        order = torch.zeros(total, dtype=torch.int32, device="cuda")
        abi.order_tiles_device(h, vp(comb), mw, mh, W, H, T, T, vp(order))
    assert order.cpu().numpy().tolist() != list(range(total))


@pytest.mark.parametrize("scene", ["loft", "room_tex", "loft_fine"])
def test_full_frames_of_the_other_scenes(scene, scenes):
    """1920x1080 of round 4's three more scenes, first frame (no costs) and the two after it, against the SHA-256 of the
    frame the compiled reference rendered (loft, loft_fine) / the oracle rendered (room_tex: textured frames cannot come from the
    reference build here, texture.cc needs SDL2 -- `made_by` in frames.json says so)."""
    import hashlib
    frames = json.load(open(os.path.join(GOLDEN, "frames.json")))
    e = frames[scene + "_1920x1080_d5"]
    abi = M.hip_abi()
    m = M.MythTracer(scenes[scene])
    h = m.device_scene()
    abi.set_lights(h, scenegen.ROOM_LIGHTS)
    sens = binding.sensor(scenegen.ROOM_CAMERA, 1920, 1080)
    for launch in range(3):
        r = abi.render_chunk(h, sens, 1920, 1080)
        sha = hashlib.sha256(r["rgb"].tobytes()).hexdigest()
        print(scene, "launch", launch, sha, "kernel ms", r["stats"]["kernel_ms"])
        assert sha == e["sha256"], launch


@pytest.mark.parametrize("view", ["room_view_back", "room_view_floor"])
def test_big_frames_other_views(view, scenes):
    """Two more 1920x1080 frames (other sign octants; grazing floor reflections)
    against the SHA-256 of the frame the compiled reference rendered, first
    through the material-classified launch, then through the cost-history one."""
    import hashlib
    frames = json.load(open(os.path.join(GOLDEN, "frames.json")))
    e = frames[view + "_1920x1080_d5"]
    abi = M.hip_abi()
    m = M.MythTracer(scenes["room"])
    h = m.device_scene()
    abi.set_lights(h, e["lights"])
    sens = binding.sensor(e["cam"], 1920, 1080)
    for launch in range(3):
        r = abi.render_chunk(h, sens, 1920, 1080)
        sha = hashlib.sha256(r["rgb"].tobytes()).hexdigest()
        print(view, "launch", launch, sha, "kernel ms", r["stats"]["kernel_ms"])
        assert sha == e["sha256"], launch


def test_tiles_and_blit_equal_single_launch(scenes):
    """mt_render_tiles_device + mt_blit_tiles_device: three virtual ranks on one
    GPU reproduce the single-launch frame byte for byte (the multi-GPU path
    minus the RCCL gather, which the gloo test covers)."""
    import torch
    abi = M.hip_abi()
    m = M.MythTracer(scenes["mini"])
    m.set_lights(scenegen.ROOM_LIGHTS)
    h = m.device_scene()
    abi.set_lights(h, scenegen.ROOM_LIGHTS)
    W, H, T = 200, 120, 32
    sens = binding.sensor(scenegen.ROOM_CAMERA, W, H)
    single = m.render(scenegen.ROOM_CAMERA, W, H)["rgb"]
    frame = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    world = 3
    for rank in range(world):
        f, s, n = tiling.rank_tiles(W, H, T, T, rank, world)
        slots = torch.zeros(n * tiling.slot_bytes(T, T), dtype=torch.uint8, device="cuda")
        abi.render_tiles_device(h, sens, W, H, T, T, f, s, n, 5, ctypes.c_void_p(slots.data_ptr()))
        abi.blit_tiles_device(h, W, H, T, T, f, s, n, ctypes.c_void_p(slots.data_ptr()),
                              ctypes.c_void_p(frame.data_ptr()))
    torch.cuda.synchronize()
    abi.read_stats(h)
    assert np.array_equal(frame.cpu().numpy(), single)


def test_smoke_entry():
    import __graft_entry__ as g
    g.smoke()


def test_room_at_recursion_depth_4(scenes):
    """BASELINE.json configs[3]: the room, 3 lights, recursion depth 4
    (MAX_RECURSION_LEVEL is a compile-time 5 in the reference, mythtracer.h:11,
    so the checker is the oracle at max_level 4 -- bit-identical to the
    reference at depth 5 on every golden).  240x135 compared in full with a live
    oracle render; 1920x1080 against the committed oracle fixture (every 16th
    pixel + sha256 of frame and first-hit buffer) and its ray counts."""
    import hashlib
    m = M.MythTracer(scenes["room"])
    m.set_max_level(4)
    o = orclib.OracleScene(scenes["room"])
    m.set_lights(scenegen.ROOM_LIGHTS)
    o.set_lights(scenegen.ROOM_LIGHTS)
    g = m.render(scenegen.ROOM_CAMERA, 240, 135, debug=True)
    r = o.render(scenegen.ROOM_CAMERA, 240, 135, max_level=4, debug=True)
    counters_match(g["counters"], r["counters"])
    assert np.array_equal(g["line"], r["line"]) and np.array_equal(g["point"], r["point"], equal_nan=True)
    assert_rgb_close(g["rgb"], r["rgb"], "room 240x135 depth 4")
    r5 = o.render(scenegen.ROOM_CAMERA, 240, 135, max_level=5)
    assert r5["counters"]["rays_secondary"] > r["counters"]["rays_secondary"]  # the depth matters here
    frames = json.load(open(os.path.join(GOLDEN, "frames.json")))["room_1920x1080_d4"]
    g = m.render(scenegen.ROOM_CAMERA, 1920, 1080, debug=True)
    sub = load("room_1920x1080_d4_sub16")
    assert np.array_equal(g["line"][::16, ::16], sub["line"])
    assert np.array_equal(g["point"][::16, ::16], sub["point"], equal_nan=True)
    assert_rgb_close(g["rgb"][::16, ::16], sub["rgb"], "room 1920x1080 depth 4, every 16th pixel")
    assert hashlib.sha256(g["line"].astype("<i4").tobytes()).hexdigest() == frames["line_sha256"]
    assert {k: g["counters"][k] for k in RAY_KEYS} == frames["rays"]
    sha = hashlib.sha256(g["rgb"].tobytes()).hexdigest()
    print("room depth 4 frame sha256", sha, "oracle", frames["sha256"], "kernel ms", g["kernel_ms"])
    if sha != frames["sha256"]:  # count against the oracle, hold to the pow tolerance
        want = o.render(scenegen.ROOM_CAMERA, 1920, 1080, max_level=4)["rgb"]
        assert hashlib.sha256(want.tobytes()).hexdigest() == frames["sha256"]
        assert_rgb_close(g["rgb"], want, "room 1920x1080 depth 4 (full frame)")


def _build_seam_driver(tmp_path):
    import subprocess
    from mythtracer_amd import build
    exe = str(tmp_path / "seam_driver")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "seam", "seam_driver.cc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(build.HOST, "include"), "-I", build.INC,
                           "-o", exe, src, "-L", build.LIB, "-lmythtracer_host", "-lmythtracer_hip",
                           "-Wl,-rpath," + build.LIB])
    return exe


def test_seam_driver_like_main_local(scenes, tmp_path):
    """The drop-in claim, executed: a C++ program written against the reference's
    API (the calls of main_local.cc:34-35,72-110,122,127-132 and of
    main_net_worker.cc:148-150) is compiled against OUR headers and library,
    run on the GPU, and its raw frame dump is the reference's frame."""
    import hashlib
    import subprocess
    exe = _build_seam_driver(tmp_path)

    def run(obj, W, H, cam, lights, chunk=None):
        out = str(tmp_path / "frame.raw")
        cmd = [exe, obj, str(W), str(H)] + [repr(float(c)) for c in cam] + [str(len(lights))]
        for l in lights:
            cmd += [repr(float(c)) for c in l]
        cmd.append(out)
        if chunk:
            cmd += [str(c) for c in chunk] + [str(tmp_path / "chunk.raw"), str(tmp_path / "chunk.dbg")]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()
        return np.fromfile(out, dtype=np.uint8).reshape(H, W, 3), r.stdout.decode()

    # Cornell 256x256: SURVEY 8c's cross-check hash of the reference's frame
    gold = load("cornell_256")
    img, stdout = run(CORNELL, 256, 256, CORNELL_CAM, CORNELL_LIGHTS, chunk=(37, 21, 101, 67))
    assert hashlib.sha256(img.tobytes()).hexdigest() == "5ed1d7bc14717479bb9312fbc1a709a6e3c0f46acf88302d31d9cd941155d201"
    assert np.array_equal(img, gold["rgb"])
    assert "Triangles: 12" in stdout and "0.000000 0.000000 0.000000 x 100.000000 100.000000 100.000000" in stdout
    # the worker's call on a ragged chunk: PXLS bytes + debug buffer
    crgb = np.fromfile(str(tmp_path / "chunk.raw"), dtype=np.uint8).reshape(67, 101, 3)
    assert np.array_equal(crgb, gold["rgb"][21:21 + 67, 37:37 + 101])
    dbg = np.fromfile(str(tmp_path / "chunk.dbg"), dtype=np.dtype([("line", "<i4"), ("point", "<f8", 3)]))
    assert np.array_equal(dbg["line"].reshape(67, 101), gold["line"][21:21 + 67, 37:37 + 101])
    assert np.array_equal(dbg["point"].reshape(67, 101, 3), gold["point"][21:21 + 67, 37:37 + 101], equal_nan=True)
    # one view of the room (golden made by the reference)
    view = load("room_view_back")
    W, H = (int(v) for v in view["image"])
    img, _ = run(scenes["room"], W, H, view["cam"], view["lights"])
    assert_rgb_close(img, view["rgb"], "seam driver, room_view_back")
    assert np.array_equal(img, view["rgb"])


@pytest.mark.parametrize("pool_cap", [None, 1])
def test_binary_recursion_trees_fill_the_ray_pool(pool_cap):
    """A material that is reflective AND transparent makes every hit spawn two
    child calls (mythtracer.cc:181-189 and :192-225): at depth 7 a pixel's
    recursion tree has up to 255 calls, a block's 16 320 -- far beyond the ray
    pool's 1 024 records per wave, so its depth-first throttle has to work; the
    state machine walks the same trees with its frame stack.  Pixels, debug
    buffer and every ray count must equal the oracle's.  pool_cap = 1: the pool
    is cut down to its minimum (MT_TUNE_POOL_CAP), so that it throttles all
    the time."""
    m, o = _both()
    for s in (m, o):
        s.add_material("both", (.1, .1, .1), (.3, .3, .3), (.4, .4, .4), ns=20, refl=0.8, tr=0.7, tf=(.9, .8, .7), ni=1.3)
        s.add_material("wall", (.6, .5, .4), (.6, .5, .4), (.1, .1, .1), ns=4)
        k = 0
        for i, z in enumerate([10, 14, 18, 22, 26, 30]):  # panes facing the camera, normals towards it
            n = [[0, 0, -1]] * 3
            w = 12 - i
            s.add_triangle([[-w, -w, z], [w, -w, z], [-w, w, z]], n, mtl=0, line_no=k); k += 1
            s.add_triangle([[w, w, z], [-w, w, z], [w, -w, z]], n, mtl=0, line_no=k); k += 1
        n = [[0, 0, -1]] * 3
        s.add_triangle([[-40, -40, 40], [40, -40, 40], [-40, 40, 40]], n, mtl=1, line_no=k); k += 1
        s.add_triangle([[40, 40, 40], [-40, 40, 40], [40, -40, 40]], n, mtl=1, line_no=k); k += 1
        n = [[0, 0, 1]] * 3  # a wall behind the camera catches the mirrored rays
        s.add_triangle([[-40, -40, -20], [40, -40, -20], [-40, 40, -20]], n, mtl=1, line_no=k); k += 1
        s.add_triangle([[40, 40, -20], [-40, 40, -20], [40, -40, -20]], n, mtl=1, line_no=k); k += 1
    lights = [(0, 30, -10, .1, .1, .1, .9, .9, .9, .5, .5, .5), (-20, -5, 5, 0, 0, 0, .4, .4, .4, .2, .2, .2)]
    if pool_cap is not None:
        M.hip_abi().set_tuning(m.device_scene(), "POOL_CAP", pool_cap)
    for depth in (5, 7):
        m.set_max_level(depth)
        m.set_lights(lights)
        o.set_lights(lights)
        g = m.render((0, 0, -5, 0, 0, 0, 70), 64, 48, debug=True)
        r = o.render((0, 0, -5, 0, 0, 0, 70), 64, 48, max_level=depth, debug=True)
        counters_match(g["counters"], r["counters"])
        assert np.array_equal(g["line"], r["line"])
        assert_rgb_close(g["rgb"], r["rgb"], "binary recursion, depth %d" % depth)
        assert g["counters"]["rays_secondary"] > 20 * 64 * 48 * 0.2  # the trees really branch


def test_moving_camera_uses_reprojected_costs(scenes):
    """The animation regime (main_local.cc:51-76: yaw += 2 degrees per frame):
    from the second frame on the work order comes from the previous frame's
    costs, re-projected through the camera change (order_kernel's forecast) -- also with
    a translation and a roll.  The order must not change a pixel: every frame
    equals the oracle's."""
    m = M.MythTracer(scenes["room"])
    o = orclib.OracleScene(scenes["room"])
    m.set_lights(scenegen.ROOM_LIGHTS)
    o.set_lights(scenegen.ROOM_LIGHTS)
    W, H = 320, 180
    cam = list(scenegen.ROOM_CAMERA)
    for f in range(5):
        g = m.render(cam, W, H, debug=True)
        r = o.render(cam, W, H, debug=True)
        assert np.array_equal(g["line"], r["line"]), f
        assert_rgb_close(g["rgb"], r["rgb"], "moving camera, frame %d" % f)
        counters_match(g["counters"], r["counters"])
        cam[4] += 2.0           # yaw
        if f >= 2:
            cam[0] += 7.0       # then the camera also walks and rolls
            cam[5] += 3.0


def test_work_counters_can_be_switched_off(scenes):
    """mt_scene_set_stats(scene, 0): the *_device calls run the kernels built
    without the work counters; same frame, counters stay zero."""
    import torch
    abi = M.hip_abi()
    m = M.MythTracer(scenes["mini"])
    h = abi.scene_create(m.flatten())
    try:
        abi.set_lights(h, scenegen.ROOM_LIGHTS)
        sens = binding.sensor(scenegen.ROOM_CAMERA, 200, 112)
        want = abi.render_chunk(h, sens, 200, 112)
        buf = torch.zeros((112, 200, 3), dtype=torch.uint8, device="cuda")
        abi.read_stats(h)
        for enabled in (False, True):
            abi.set_stats(h, enabled)
            buf.zero_()
            abi.render_chunk_device(h, sens, 200, 112, (0, 0, 200, 112), 5, ctypes.c_void_p(buf.data_ptr()))
            torch.cuda.synchronize()
            st = abi.read_stats(h)
            assert np.array_equal(buf.cpu().numpy(), want["rgb"]), enabled
            rays = sum(st[k] for k in RAY_KEYS)
            assert rays == (sum(want["stats"][k] for k in RAY_KEYS) if enabled else 0), enabled
        # a host call that asks for statistics counts whatever the switch says
        abi.set_stats(h, False)
        again = abi.render_chunk(h, sens, 200, 112)
        # (the work counters of the automatic mode depend on which rays share a wave)
        assert {k: again["stats"][k] for k in ALL_KEYS if k not in PRUNED} == {k: want["stats"][k] for k in ALL_KEYS if k not in PRUNED}
    finally:
        abi.scene_destroy(h)


def test_headline_frame_without_work_counters(scenes, engine):
    """BASELINE configs[2] (room, 1920x1080, 3 lights, depth 5) through
    mt_render_chunk_device with mt_scene_set_stats(scene, 0) -- the kernels
    bench.py times -- against the SHA-256 of the frame the compiled reference
    rendered (tests/golden/frames.json).  Four consecutive frames: a first frame
    without costs, then history-scheduled ones; in the automatic mode that is the
    ray pool (probe_kernel), then the state machine ordered by the pool's cost
    words, then by its own; then a SMALL launch (a 640x360 chunk: fewer than 9
    blocks per resident wave -> ray pool again, twice: probe, then costs) and
    the full frame once more (no usable history after the chunk)."""
    import hashlib
    import torch
    frames = json.load(open(os.path.join(GOLDEN, "frames.json")))
    want = frames["room_1920x1080_d5"]["sha256"]
    abi = M.hip_abi()
    m = M.MythTracer(scenes["room"])
    h = m.device_scene()
    abi.set_lights(h, scenegen.ROOM_LIGHTS)
    W, H = 1920, 1080
    sens = binding.sensor(scenegen.ROOM_CAMERA, W, H)
    buf = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    abi.read_stats(h)
    abi.set_stats(h, False)
    full = None
    for launch in range(4):
        buf.zero_()
        abi.render_chunk_device(h, sens, W, H, (0, 0, W, H), 5, ctypes.c_void_p(buf.data_ptr()))
        torch.cuda.synchronize()
        full = buf.cpu().numpy()
        assert hashlib.sha256(full.tobytes()).hexdigest() == want, (engine, launch)
    small = torch.zeros((360, 640, 3), dtype=torch.uint8, device="cuda")
    for launch in range(2):
        small.zero_()
        abi.render_chunk_device(h, sens, W, H, (700, 500, 640, 360), 5, ctypes.c_void_p(small.data_ptr()))
        torch.cuda.synchronize()
        assert np.array_equal(small.cpu().numpy(), full[500:860, 700:1340]), (engine, launch)
    buf.zero_()
    abi.render_chunk_device(h, sens, W, H, (0, 0, W, H), 5, ctypes.c_void_p(buf.data_ptr()))
    torch.cuda.synchronize()
    assert hashlib.sha256(buf.cpu().numpy().tobytes()).hexdigest() == want
    a, b = abi.kernel_times(h)
    print(engine, "kernel ms per launch:", [round(float(x + y), 2) for x, y in zip(a, b)])
    st = abi.read_stats(h)
    assert sum(st[k] for k in RAY_KEYS) == 0  # counters were off
    abi.set_stats(h, True)


def test_automatic_engine_with_debug_buffers(scenes, engine):
    """Consecutive frames WITH debug buffer and work counters through the
    engine of the fixture -- in the automatic mode: a large launch (state machine
    once costs exist) and a small one (ray pool) alternate, so both branches and
    the hand-over of the cost words run -- each compared with the oracle."""
    abi = M.hip_abi()
    m = M.MythTracer(scenes["mini"])
    h = m.device_scene()
    abi.set_lights(h, scenegen.ROOM_LIGHTS)
    # one workgroup per CU and the switch at 1 block per wave: 320x180 (920 blocks) is "large" for
    # a 256-CU GPU's 1024 resident waves only if the threshold is lowered too
    abi.set_tuning(h, "BLOCKS_PER_CU", 1)
    abi.set_tuning(h, "POOL_BELOW", 0.5)
    o = orclib.OracleScene(scenes["mini"])
    o.set_lights(scenegen.ROOM_LIGHTS)
    big = o.render(scenegen.ROOM_CAMERA, 320, 180, debug=True)
    small = o.render(scenegen.ROOM_CAMERA, 320, 180, chunk=(40, 30, 96, 64), debug=True)
    sens = binding.sensor(scenegen.ROOM_CAMERA, 320, 180)
    for launch in range(6):
        if launch in (3, 4):
            g, w = abi.render_chunk(h, sens, 320, 180, chunk=(40, 30, 96, 64), debug=True), small
        else:
            g, w = abi.render_chunk(h, sens, 320, 180, debug=True), big
        assert_rgb_close(g["rgb"], w["rgb"], "%s launch %d" % (engine, launch))
        assert np.array_equal(g["line"], w["line"]), launch
        assert np.array_equal(g["point"], w["point"], equal_nan=True), launch
        counters_match({k: g["stats"][k] for k in ALL_KEYS}, w["counters"])


@pytest.mark.parametrize("n_lights", [255, 300])
def test_more_lights_than_the_ray_pool_addresses(n_lights, engine):
    """The ray pool addresses 254 lights.  The automatic mode must render such a
    scene anyway (through the state machine, which has no limit); only an
    explicit engine 2 is refused, with MT_ERR_UNSUPPORTED."""
    rnd = np.random.RandomState(n_lights)
    lights = [(float(rnd.uniform(10, 90)), float(rnd.uniform(60, 95)), float(rnd.uniform(10, 90)),
               .001, .001, .001, .004, .004, .004, .002, .002, .002) for _ in range(n_lights)]
    m = M.MythTracer(CORNELL)
    o = orclib.OracleScene(CORNELL)
    m.set_lights(lights)
    o.set_lights(lights)
    if engine == "ray_pool":
        with pytest.raises(RuntimeError, match="254 lights|engine 2"):
            m.render(CORNELL_CAM, 24, 24)
        return
    for frame in range(2):
        g, r = m.render(CORNELL_CAM, 24, 24, debug=True), o.render(CORNELL_CAM, 24, 24, debug=True)
        counters_match(g["counters"], r["counters"])
        assert np.array_equal(g["line"], r["line"])
        assert_rgb_close(g["rgb"], r["rgb"], "%d lights, frame %d" % (n_lights, frame))


def _write_ppm(path, rgb):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(np.ascontiguousarray(rgb, dtype=np.uint8).tobytes())


def test_texture_files_end_to_end(tmp_path, engine):
    """SURVEY f-3 as a whole: image FILE -> decoder -> RGB8 -> mt_texture upload
    -> GetUVW + Texture::GetColorAt in the kernel (texture.cc:60-109,
    mythtracer.cc:59-64).  A generated .mtl names a PPM and a PNG through map_Ka;
    MythTracer::LoadObj reads them with the library's own decoders; the oracle
    loads a twin .mtl whose textures are PPM files of the same pixels (PNG is
    lossless; the oracle reads PPM only).  One triangle carries NaN texture
    coordinates: the reference's colors.at() would throw there (texture.cc:45-52);
    both sides define the colour as NaN -> channel 0.
    PARITY UNPINNED for Texture::GetColorAt itself (texture.cc:11-58): the
    reference's texture.cc needs SDL2, which the image lacks, and the reference
    holds no texture fixture -- GPU and oracle are checked against each other."""
    from PIL import Image
    rnd = np.random.RandomState(77)
    ta = rnd.randint(0, 256, size=(9, 13, 3)).astype(np.uint8)
    tb = rnd.randint(0, 256, size=(16, 16, 3)).astype(np.uint8)
    d_gpu, d_orc = tmp_path / "gpu", tmp_path / "orc"
    d_gpu.mkdir(); d_orc.mkdir()
    _write_ppm(str(d_gpu / "a.ppm"), ta)
    Image.fromarray(tb, "RGB").save(str(d_gpu / "b.png"))
    _write_ppm(str(d_orc / "a.ppm"), ta)
    _write_ppm(str(d_orc / "b.png"), tb)  # the oracle's PPM reader goes by content, the name stays the .mtl's
    # round 4: a PROGRESSIVE JPEG and an Adam7-interlaced 16-bit PNG through map_Ka too (what a 3ds-Max export's textures
    # tend to be); the oracle gets the pixels libjpeg-turbo decodes (through PIL) / the samples' high bytes as PPM
    yy, xx = np.mgrid[0:24, 0:40]
    tc = np.stack([(xx * 6 + yy) % 256, (xx + yy * 9) % 256, (xx * yy) % 256], axis=2).astype(np.uint8)
    Image.fromarray(tc, "RGB").save(str(d_gpu / "c.jpg"), "JPEG", quality=85, progressive=True, subsampling=2)
    assert b"\xff\xc2" in (d_gpu / "c.jpg").read_bytes()
    _write_ppm(str(d_orc / "c.jpg"), np.array(Image.open(str(d_gpu / "c.jpg")).convert("RGB")))
    import test_host_cpu
    td16 = rnd.randint(0, 65536, size=(11, 7, 3))
    (d_gpu / "d.png").write_bytes(test_host_cpu._png(7, 11, 2, td16, [0, 1, 2, 3, 4], 9, depth=16, interlace=1))
    _write_ppm(str(d_orc / "d.png"), (td16 >> 8).astype(np.uint8))
    mtl = ("newmtl pa\nKa 1 1 1\nKd 0.8 0.8 0.8\nKs 0.1 0.1 0.1\nNs 4\nmap_Ka a.ppm\n"
           "newmtl pb\nKa 0.9 0.7 0.8\nKd 0.5 0.5 0.5\nKs 0 0 0\nNs 1\nmap_Ka b.png\n"
           "newmtl pc\nKa 1 1 1\nKd 0.5 0.5 0.5\nKs 0 0 0\nNs 1\nmap_Ka a.ppm\n"
           "newmtl pd\nKa 1 1 1\nKd 0.6 0.6 0.6\nKs 0 0 0\nNs 1\nmap_Ka c.jpg\n"
           "newmtl pe\nKa 1 1 1\nKd 0.6 0.6 0.6\nKs 0 0 0\nNs 1\nmap_Ka d.png\n")
    obj = ("mtllib t.mtl\n"
           "v -6 -4 0\nv 0 -4 0\nv -6 4 0\nv 6 -4 0\nv 0 4 0\nv 6 4 0\nv 0 4.5 0\nv 6 4.5 0\nv 6 8 0\n"
           "vn 0 0 -1\n"
           "vt -0.5 -0.5\nvt 1.5 0\nvt 0 2.5\nvt 0 0\nvt 1 0\nvt 0 1\nvt nan nan\n"
           "usemtl pa\nf 1/1/1 2/2/1 3/3/1 \n"
           "usemtl pb\nf 2/4/1 4/5/1 5/6/1 \n"
           "usemtl pc\nf 7/7/1 8/7/1 9/7/1 \n"
           "v -6 -8 0\nv 0 -8 0\nv -6 -4.5 0\nv 6 -8 0\nv 0 -4.5 0\n"
           "usemtl pd\nf 10/4/1 11/5/1 12/6/1 \n"
           "usemtl pe\nf 11/4/1 13/5/1 14/6/1 \n")
    for d in (d_gpu, d_orc):
        (d / "t.mtl").write_text(mtl)
        (d / "t.obj").write_text(obj)
    m = M.MythTracer(str(d_gpu / "t.obj"))
    o = orclib.OracleScene(str(d_orc / "t.obj"))
    flat = m.flatten()
    assert sorted(t["texels"].dtype.name for t in flat["textures"]) == ["uint8"] * 4  # RGB8 on the device
    assert sorted(t["texels"].shape for t in flat["textures"]) == [(9, 13, 3), (11, 7, 3), (16, 16, 3), (24, 40, 3)]
    cam, lights = (0, 0, -11, 0, 0, 0, 90), [(0, 0, -6, .4, .4, .4, .7, .7, .7, .2, .2, .2)]
    for frame in range(2):
        g = _render_both(m, o, cam, 96, 80, lights)
    rgb, line = g["rgb"], g["line"]
    lines = np.unique(line[line >= 0])
    assert len(lines) == 5
    for ln in [l for l in lines if l != lines[2]]:
        assert len(np.unique(rgb[line == ln], axis=0)) > 20  # the colour follows the texels
    nan_tri = line == lines[2]  # (the third face of the file carries the NaN coordinates)
    assert nan_tri.any() and (rgb[nan_tri] == 0).all()


def test_render_frame_multi_virtual_devices(scenes, engine):
    """mt_render_frame_multi (main_net_master.cc:195-236): N scene
    replicas -- all on GPU 0 here, one per GPU in production -- render their tiles
    (dealt out by number at first, then by cost) of ONE frame side by side, the tile buffers are gathered on the
    first replica's device and blitted; the frame must be byte-identical to the
    single launch, every ray counted once."""
    abi = M.hip_abi()
    m = M.MythTracer(scenes["mini"])
    flat = m.flatten()
    W, H = 330, 190  # ragged edge tiles
    sens = binding.sensor(scenegen.ROOM_CAMERA, W, H)
    hs = [abi.scene_create(flat) for _ in range(4)]
    try:
        for hh in hs:
            abi.set_lights(hh, scenegen.ROOM_LIGHTS)
        single = abi.render_chunk(hs[0], sens, W, H)
        for n in (1, 2, 3, 4):
            for frame in range(2):  # the second one is scheduled from every replica's own costs
                r = abi.render_frame_multi(hs[:n], sens, W, H, 64, 64, 5)
                assert np.array_equal(r["rgb"], single["rgb"]), (n, frame)
                for k in RAY_KEYS + ("shaded_hits",):
                    assert sum(st[k] for st in r["stats"]) == single["stats"][k], (n, k)
                assert all(st["kernel_ms"] > 0 for st in r["stats"])
        # a turning camera: the replicas exchange their block costs after every frame (the next one's re-projected
        # forecast reads all tiles' costs); the order of the work changes no pixel
        cam = list(scenegen.ROOM_CAMERA)
        for frame in range(4):
            cam[4] += 2.0
            s_f = binding.sensor(cam, W, H)
            want = abi.render_chunk(hs[3], s_f, W, H)["rgb"]
            got = abi.render_frame_multi(hs[:3], s_f, W, H, 64, 64, 5, want_stats=False)["rgb"]
            assert np.array_equal(got, want), frame
        r = abi.render_frame_multi(hs, sens, W, H, 256, 256, 5, want_stats=False)  # fewer tiles (2) than replicas
        assert np.array_equal(r["rgb"], single["rgb"])
        # The cross-device branch on ONE device (a one-GPU box): every replica's tiles and cost map go through the gather
        # buffer with hipMemcpyPeerAsync, as they would from another GPU -- its offsets and the blit from it, byte for
        # byte.  (Peer ACCESS between two devices still has not run anywhere: include/mythtracer_hip.h says so.)
        abi.set_tuning(hs[0], "MULTI_FORCE_PEER_COPY", 1.0)
        cam = list(scenegen.ROOM_CAMERA)
        for frame in range(5):  # at rest, at rest (lists kept), then turning
            cam[4] += 0.0 if frame < 2 else 2.0
            s_f = binding.sensor(cam, W, H)
            want = abi.render_chunk(hs[3], s_f, W, H)["rgb"]
            got = abi.render_frame_multi(hs[:3], s_f, W, H, 32, 32, 5, want_stats=False)["rgb"]
            assert np.array_equal(got, want), ("peer copies", frame)
        abi.set_tuning(hs[0], "MULTI_FORCE_PEER_COPY", 0.0)
        abi.set_tuning(hs[0], "MULTI_BALANCE", 0.0)  # tiles by number, every frame
        for frame in range(3):
            cam[4] += 2.0
            s_f = binding.sensor(cam, W, H)
            want = abi.render_chunk(hs[3], s_f, W, H)["rgb"]
            assert np.array_equal(abi.render_frame_multi(hs[:3], s_f, W, H, 64, 64, 5, want_stats=False)["rgb"], want), ("by number", frame)
        abi.set_tuning(hs[0], "MULTI_BALANCE", 1.0)
        with pytest.raises(RuntimeError):
            abi.render_frame_multi([hs[0], hs[0]], sens, W, H)
    finally:
        for hh in hs:
            abi.scene_destroy(hh)


def test_facade_set_devices(scenes, engine):
    """MythTracer::SetDevices({0, 0}): the W x H overload of RayTrace
    (mythtracer.cc:258-278) renders through mt_render_frame_multi -- the drop-in
    a C++ driver written against the facade gets on a multi-GPU node."""
    g = load("mini_320x180")
    m = M.MythTracer(scenes["mini"])
    m.set_devices([0, 0, 0])
    m.set_lights(scenegen.ROOM_LIGHTS)
    for frame in range(2):
        rgb = m.render_image(scenegen.ROOM_CAMERA, 320, 180)
        assert_rgb_close(rgb, g["rgb"], "SetDevices frame %d" % frame)
        assert np.array_equal(rgb, g["rgb"])


def test_cost_map_exchange_between_ranks(scenes, engine):
    """Multi-GPU frames with a moving camera: every rank exports the block costs
    of its tiles into a frame-wide map, the maps are combined (MAX) and imported,
    and the next frame's re-projected forecast reads them
    (mt_scene_export_costs_device / mt_scene_import_costs_device).  Three virtual
    ranks on one GPU, a scene each, five frames of a turning camera: every map
    holds exactly its rank's blocks, and every frame equals the oracle's (the
    order of the work changes no pixel)."""
    import torch
    abi = M.hip_abi()
    m = M.MythTracer(scenes["mini"])
    flat = m.flatten()
    o = orclib.OracleScene(scenes["mini"])
    o.set_lights(scenegen.ROOM_LIGHTS)
    W, H, T, world = 256, 144, 32, 3
    mw, mh = (W + 7) // 8, (H + 7) // 8
    hs = [abi.scene_create(flat) for _ in range(world)]
    try:
        for hh in hs:
            abi.set_lights(hh, scenegen.ROOM_LIGHTS)
        comb = None
        cam = list(scenegen.ROOM_CAMERA)
        for frame_no in range(5):
            sens = binding.sensor(cam, W, H)
            frame = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            maps = []
            for r in range(world):
                f, s, n = tiling.rank_tiles(W, H, T, T, r, world)
                slots = torch.zeros(n * tiling.slot_bytes(T, T), dtype=torch.uint8, device="cuda")
                if comb is not None:
                    abi.import_costs_device(hs[r], ctypes.c_void_p(comb.data_ptr()), mw, mh)
                abi.render_tiles_device(hs[r], sens, W, H, T, T, f, s, n, 5, ctypes.c_void_p(slots.data_ptr()))
                abi.blit_tiles_device(hs[r], W, H, T, T, f, s, n, ctypes.c_void_p(slots.data_ptr()), ctypes.c_void_p(frame.data_ptr()))
                cm = torch.zeros((mh, mw), dtype=torch.int32, device="cuda")
                abi.export_costs_device(hs[r], ctypes.c_void_p(cm.data_ptr()), mw, mh)
                torch.cuda.synchronize()
                abi.read_stats(hs[r])
                own = np.zeros((mh, mw), dtype=bool)
                for j in range(n):
                    x, y, cw, ch = tiling.tile_rect(f + j * s, W, H, T, T)
                    own[y // 8:(y + ch + 7) // 8, x // 8:(x + cw + 7) // 8] = True
                assert np.array_equal(cm.cpu().numpy() != 0, own), (frame_no, r)
                maps.append(cm)
            comb = torch.stack(maps).max(dim=0).values.contiguous()
            assert (comb.cpu().numpy() != 0).all()
            want = o.render(cam, W, H)["rgb"]
            assert_rgb_close(frame.cpu().numpy(), want, "%s frame %d" % (engine, frame_no))
            cam[4] += 2.0
        with pytest.raises(RuntimeError):
            abi.export_costs_device(hs[0], ctypes.c_void_p(comb.data_ptr()), 3, 3)
    finally:
        for hh in hs:
            abi.scene_destroy(hh)


def test_cost_balanced_tile_ownership(scenes, engine):
    """Tiles dealt out by cost (mt_order_tiles_device / mt_deal_tiles_device / mt_render_tile_list_device /
    mt_blit_tile_list_device; the static counterpart of the master's pull queue, main_net_master.cc:62-80): three
    virtual ranks on one GPU, a scene each.  Frame 0 by tile number, from then on by the combined cost map of the
    previous frame -- camera at rest twice (the second time the lists are kept, list_id unchanged: per-slot history),
    then turning (new lists every frame, forecast from the imported map by image position), then at rest again.  The
    device's order and lists equal their numpy restatement (mythtracer_amd/tiling.py), every tile has exactly one
    owner, the summed costs per rank lie closer together than with k mod N, and every frame equals the oracle's."""
    import torch
    abi = M.hip_abi()
    m = M.MythTracer(scenes["mini"])
    flat = m.flatten()
    o = orclib.OracleScene(scenes["mini"])
    o.set_lights(scenegen.ROOM_LIGHTS)
    W, H, T, world = 264, 150, 16, 3  # ragged edge tiles (264 = 16.5 tiles, 150 = 9.4)
    mw, mh = (W + 7) // 8, (H + 7) // 8
    tx, ty = tiling.tile_grid(W, H, T, T)
    total = tx * ty
    hs = [abi.scene_create(flat) for _ in range(world)]
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    try:
        for hh in hs:
            abi.set_lights(hh, scenegen.ROOM_LIGHTS)
        comb, lists, list_id = None, None, 0
        cam = list(scenegen.ROOM_CAMERA)
        plan = ["number", "deal", "keep", "deal", "deal", "deal", "keep"]
        turn = [0.0, 0.0, 0.0, 2.0, 2.0, 2.0, 0.0]
        worst = []
        for frame_no, (what, dyaw) in enumerate(zip(plan, turn)):
            cam[4] += dyaw
            sens = binding.sensor(cam, W, H)
            if what != "keep":
                list_id += 1
                order_d = None
                if what == "deal":
                    order_d = torch.zeros(total, dtype=torch.int32, device="cuda")
                    abi.order_tiles_device(hs[0], vp(comb), mw, mh, W, H, T, T, vp(order_d))
                    want_order = tiling.order_tiles(comb.cpu().numpy().astype(np.uint32), W, H, T, T)
                    assert np.array_equal(order_d.cpu().numpy(), want_order), frame_no
                lists = []
                for r in range(world):
                    lst = torch.full((total,), -7, dtype=torch.int32, device="cuda")
                    n = abi.deal_tiles_device(hs[r], vp(order_d) if order_d is not None else None, W, H, T, T, world, r, vp(lst))
                    assert n == abi.dealt_tile_count(W, H, T, T, world, r) == tiling.dealt_tile_count(total, world, r)
                    got = lst.cpu().numpy()
                    assert (got[n:] == -7).all()
                    assert np.array_equal(got[:n], tiling.deal_tiles(None if order_d is None else want_order, total, world, r))
                    lists.append(lst[:n].contiguous())
                assert sorted(torch.cat(lists).cpu().numpy().tolist()) == list(range(total))
                if what == "deal":  # balance by the map the deal was made from
                    tc = np.array([comb.cpu().numpy()[y // 8:(y + ch + 7) // 8, x // 8:(x + cw + 7) // 8].astype(np.int64).sum()
                                   for (x, y, cw, ch) in (tiling.tile_rect(t, W, H, T, T) for t in range(total))])
                    dealt = np.array([tc[l.cpu().numpy()].sum() for l in lists], dtype=np.float64)
                    modular = np.array([tc[r::world].sum() for r in range(world)], dtype=np.float64)
                    worst.append((dealt.max() / dealt.mean(), modular.max() / modular.mean()))
            frame = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            maps = []
            for r in range(world):
                n = int(lists[r].numel())
                slots = torch.zeros(n * tiling.slot_bytes(T, T), dtype=torch.uint8, device="cuda")
                if comb is not None:
                    abi.import_costs_device(hs[r], vp(comb), mw, mh)
                abi.render_tile_list_device(hs[r], sens, W, H, T, T, vp(lists[r]), n, list_id, 5, vp(slots))
                lists[r] += 0  # (the call copied the list: the caller's buffer may be reused at once)
                abi.blit_tile_list_device(hs[r], W, H, T, T, vp(lists[r]), n, vp(slots), vp(frame))
                cm = torch.zeros((mh, mw), dtype=torch.int32, device="cuda")
                abi.export_costs_device(hs[r], vp(cm), mw, mh)
                torch.cuda.synchronize()
                abi.read_stats(hs[r])
                own = np.zeros((mh, mw), dtype=bool)
                for t in lists[r].cpu().numpy():
                    x, y, cw, ch = tiling.tile_rect(int(t), W, H, T, T)
                    own[y // 8:(y + ch + 7) // 8, x // 8:(x + cw + 7) // 8] = True
                assert np.array_equal(cm.cpu().numpy() != 0, own), (frame_no, r)
                maps.append(cm)
            comb = torch.stack(maps).max(dim=0).values.contiguous()
            assert (comb.cpu().numpy() != 0).all()
            want = o.render(cam, W, H)["rgb"]
            assert_rgb_close(frame.cpu().numpy(), want, "%s frame %d (%s)" % (engine, frame_no, what))
            assert np.array_equal(frame.cpu().numpy(), want)
        print("max / mean of the ranks' summed tile costs, dealt vs k mod N:", ["%.3f vs %.3f" % w for w in worst])
        assert np.mean([w[0] for w in worst]) < np.mean([w[1] for w in worst])
        # argument checks of the new entry points
        with pytest.raises(RuntimeError):
            abi.order_tiles_device(hs[0], vp(comb), 3, 3, W, H, T, T, vp(order_d))
        with pytest.raises(RuntimeError):
            abi.dealt_tile_count(W, H, T, T, 3, 3)
        with pytest.raises(RuntimeError):
            abi.render_tile_list_device(hs[0], sens, W, H, T, T, vp(lists[0]), total + 1, 0, 5, vp(slots))
        # the tuning knobs refuse values the kernels would divide by or overflow on (mt_scene_set_tuning)
        for knob, bad in (("QUAD_SHARE", 0.0), ("HYBRID_WORK1", 0.0), ("POOL_PIECE_WORK1", -1.0), ("POOL_SCRATCH_MB", float("inf")),
                          ("BLEND", 1.5), ("HYBRID_POOL_SHARE", float("nan")), ("ORDER_GROUPS", 0.0), ("ORDER_GROUPS", 257.0), ("SM_CELL_SHARE", 0.0), ("SM_CELL_WORK", -1.0),
                          ("XCD_QUEUES", 3.0)):
            with pytest.raises(RuntimeError):
                abi.set_tuning(hs[0], knob, bad)
    finally:
        for hh in hs:
            abi.scene_destroy(hh)


def test_exact_ties_inside_long_lists(engine):
    """A long list (more than 32 triangles in one node) is scanned through its
    spatially SORTED copy and its hits are folded in whatever order they come,
    by (distance ascending, list position descending) -- which must be the
    reference's "a later equally distant hit replaces the earlier one"
    (octtree.cc:186-195).  Here: 90 coincident copies of two triangles that
    straddle the root's centre (they stay in the root's list), interleaved with
    120 other straddlers, different materials so that the winner shows in the
    pixels, plus small triangles that make the tree split; rays and a rendered
    frame against the oracle."""
    rnd = scenegen.SplitMix64(4242)
    m, o = _both()
    for s in (m, o):
        for k in range(3):
            s.add_material("m%d" % k, (.2 + .3 * k, .9 - .3 * k, .3), (.5, .5, .5), (.1, .1, .1), ns=4)
    tris = []
    n = [[0, 0, -1]] * 3
    for k in range(90):
        tris.append(([[-30, -30, 50], [70, -30, 50], [-30, 70, 50]], k % 3))       # coincident, through the centre
        tris.append(([[70, 70, 50], [-30, 70, 50], [70, -30, 50]], (k + 1) % 3))
        if k % 3 == 0:
            z = 20.0 + float(int(rnd.rng(0, 60)))
            tris.append(([[-20, -20, z], [60, -25, z], [-25, 60, z + 1]], k % 3))  # other straddlers, lattice depths
    for k in range(400):                                                            # small ones: the tree splits
        c = [float(int(rnd.rng(-40, 90))) for _ in range(3)]
        tris.append(([[c[0], c[1], c[2]], [c[0] + 2, c[1], c[2]], [c[0], c[1] + 2, c[2] + 1]], k % 3))
    for s in (m, o):
        for k, (v, mt) in enumerate(tris):
            s.add_triangle(v, n, mtl=mt, line_no=k)
    t = m.tree()
    assert t["prim_count"][0] > 64, "the straddlers must stay in the root's list"
    rays = []
    for i in range(2048):
        org = [float(int(rnd.rng(-20, 60))), float(int(rnd.rng(-20, 60))), -40.0 if i % 2 else 140.0]
        tgt = [float(int(rnd.rng(-10, 50))), float(int(rnd.rng(-10, 50))), 50.0]
        d = [tgt[a] - org[a] for a in range(3)]
        if i % 4 == 0:
            d = [0.0, 0.0, d[2]]  # axis-parallel too (the exact descent on the same lists)
        rays.append(org + d)
    rays = np.array(rays)
    want = o.intersect(rays)
    got = M.hip_abi().intersect_rays(m.device_scene(), rays)
    hit = want["line"] >= 0
    assert hit.mean() > 0.5
    assert np.array_equal(got["line"], want["line"])
    assert np.array_equal(got["t"][hit], want["t"][hit])
    assert (want["line"][hit] >= 170).mean() > 0.3  # late list positions win the ties
    lights = [(20, 20, -60, .2, .2, .2, .8, .8, .8, .3, .3, .3), (30, 10, 160, .1, .1, .1, .6, .6, .6, .2, .2, .2)]
    _render_both(m, o, (20, 20, -70, 0, 0, 0, 70), 128, 96, lights)
    _render_both(m, o, (20, 25, 150, 0, 180, 0, 70), 96, 64, lights)


@pytest.mark.parametrize("extra", [[], ["--regime", "warm", "--engine", "3"]])
def test_bench_line_contract(extra):
    """bench.py as the driver starts it (a child process, one GPU): exit code 0, ONE JSON line with the contract's
    keys, the moving-camera regime as `value`, parity verdicts on the timed frame and the extras, the roofline block
    (counter-derived fields are numbers when profiles/pmc_frame_kernel.json was measured on these kernel sources,
    else null -- never stale)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "6", "--warmup", "2", "--full", "--no-cpu-baseline",
                        "--crop-checks", "2"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["unit"] == "Mray/s" and d["dtype"] == "f64" and d["vs_baseline"] is None
    assert d["parity"] == "frame identical to the reference's" and d["value"] > 100.0
    assert d["value_regime"] == ("warm" if extra else "moving")
    ro = d["roofline"]
    assert ro["bound"] == "valu_issue" and ro["kernel_ms"] > 0 and ro["hbm"]["requested_GBps"] > 0
    assert (ro["frac"] is None) == (ro["achieved"] is None) == (ro["traffic"] is None)
    if ro["frac"] is not None:
        assert 0.2 < ro["frac"] < 1.0 and ro["pmc_source"]["measured_at_commit"]
    ex = d["extras"]
    assert ex["cold_frame_parity"] == ex["warm_same_frame"]["parity"] == ex["counters_on_frame_parity"] == d["parity"]


def test_bench_plain_run_and_output_dump(engine, tmp_path):
    """bench.py without --full (the run repeated for every change): exit code 0, ONE JSON line with the contract's
    keys and none of what --full adds; --steps sets the timed steps; --dump-outputs writes the frame of the last timed
    step (the golden camera's) as float32, and it is the reference's frame.  The plain run counts the rays of each
    distinct camera once and weighs it: its ray counts must equal those of --full's pass over every frame."""
    import hashlib, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    eng = {"state_machine": "1", "ray_pool": "2", "hybrid": "3", "auto": "0"}[engine]

    def run(*extra):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "18", "--warmup", "2",
                            "--engine", eng] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        return json.loads(lines[0])
    d = run("--dump-outputs", str(tmp_path / "out"))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup"):
        assert k in d, k
    for k in ("roofline", "parity", "frame_sha256", "extras", "cpu_baseline", "value_warm"):
        assert k not in d, k
    assert d["steps"] == 18 and d["unit"] == "Mray/s" and d["higher_is_better"] and d["ms_per_step"] > 0
    assert d["value"] > 100.0
    assert sorted(os.listdir(tmp_path / "out")) == ["frame.npy"]
    img = np.load(tmp_path / "out" / "frame.npy")
    assert img.dtype == np.float32 and img.shape == (1080, 1920, 3)
    u8 = img.astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32), img)
    golden = json.load(open(os.path.join(GOLDEN, "frames.json")))["room_1920x1080_d5"]["sha256"]
    assert hashlib.sha256(u8.tobytes()).hexdigest() == golden
    f = run("--full", "--no-extras")
    assert f["parity"] == "frame identical to the reference's"
    assert d["rays_per_frame_mean"] == f["rays_per_frame_mean"] and d["rays_last_frame"] == f["rays_last_frame"]


@pytest.mark.parametrize("n_straddlers", [450, 1100, 6000])
def test_long_lists_of_many_supers(engine, n_straddlers):
    """The walk stages a long list's sorted copy level by level through LDS (scan_long): super boxes in rounds of 16
    (1 024 entries), the block quads of the live supers gathered six at a time, the entry quads of the live blocks two
    buffers deep.  Lists of 8, 18 and 94 supers here (the room scene's longest has 25): thin triangles that straddle the
    root's centre planes all over the box, so that rays of every octant -- mixed within a wave, intersect_rays takes them
    as they come -- find many supers and blocks live at once; distances tie on purpose (lattice coordinates).  Rays and a
    frame against the oracle."""
    rnd = scenegen.SplitMix64(977 + n_straddlers)
    m, o = _both()
    for s in (m, o):
        for k in range(3):
            s.add_material("m%d" % k, (.2 + .3 * k, .9 - .3 * k, .3), (.5, .5, .5), (.1, .1, .1), ns=4)
    tris = []
    n = [[0, 0, -1]] * 3
    for k in range(n_straddlers):  # each crosses one of the centre planes (50): it cannot sink into a child
        a = k % 3
        c = [float(int(rnd.rng(2, 98))) for _ in range(3)]
        c[a] = 50.0
        v0 = list(c); v1 = list(c); v2 = list(c)
        v0[a] -= 1.0 + float(int(rnd.rng(0, 3)))
        v1[a] += 1.0 + float(int(rnd.rng(0, 3)))
        v1[(a + 1) % 3] += 3.0
        v2[(a + 2) % 3] += 3.0
        tris.append(([v0, v1, v2], k % 3))
    for k in range(600):  # small ones in the octants: the tree splits
        c = [float(int(rnd.rng(1, 96))) for _ in range(3)]
        c = [x if abs(x - 50.0) > 4.0 else x + 9.0 for x in c]
        tris.append(([[c[0], c[1], c[2]], [c[0] + 2, c[1], c[2]], [c[0], c[1] + 2, c[2] + 1]], k % 3))
    tris.append(([[0, 0, 0], [1, 0, 0], [0, 1, 0]], 0))
    tris.append(([[100, 100, 100], [99, 100, 100], [100, 99, 100]], 0))
    for s in (m, o):
        for k, (v, mt) in enumerate(tris):
            s.add_triangle(v, n, mtl=mt, line_no=k)
    t = m.tree()
    assert t["prim_count"][0] >= n_straddlers, "the straddlers must stay in the root's list"
    rays = []
    for i in range(4096):
        org = [float(int(rnd.rng(-30, 130))) for _ in range(3)]
        org[i % 3] = -40.0 if (i // 3) % 2 else 140.0
        tgt = [float(int(rnd.rng(5, 95))) for _ in range(3)]
        rays.append(org + [tgt[a] - org[a] for a in range(3)])
    rays = np.array(rays)
    want = o.intersect(rays)
    got = M.hip_abi().intersect_rays(m.device_scene(), rays)
    hit = want["line"] >= 0
    assert hit.mean() > 0.1 and (want["line"][hit] < n_straddlers).mean() > 0.5
    assert np.array_equal(got["line"], want["line"])
    assert np.array_equal(got["t"][hit], want["t"][hit])
    lights = [(20, 20, -60, .2, .2, .2, .8, .8, .8, .3, .3, .3), (130, 110, 160, .1, .1, .1, .6, .6, .6, .2, .2, .2)]
    _render_both(m, o, (-60, 50, -70, 0, 40, 0, 70), 128, 96, lights)


def test_bench_two_ranks_rehearsal():
    """`bench.py --gpus 2` as the driver starts it (no launcher: it starts its own ranks), in the one-GPU rehearsal mode
    (MT_BENCH_EMULATE_RANKS=1: both ranks on GPU 0, gloo on host copies instead of RCCL -- everything else is the code
    of the real N-GPU run): tiles k = r (mod 2) of the 3840x2160 frame with a panning camera, gather, blit, cost-map
    all-reduce; the line must say 2 ranks and a frame identical to the golden one."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MT_BENCH_EMULATE_RANKS="1")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2",
                        "--full", "--no-cpu-baseline", "--no-extras"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_reported_by_backend"] == 2 and d["scaling"] == "strong"
    assert d["parity"].startswith("frame identical to the reference's")  # (the whole 3840x2160 frame: tests/golden/frames.json holds the reference's since round 4)
    assert d["exchange_ms_device"]["cost_map_bytes_all_reduced"] == 4 * ((3840 + 7) // 8) * ((2160 + 7) // 8)
