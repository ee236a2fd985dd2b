"""The lean frame kernel (MT_TUNE_LEAN_KERNEL; mt_render.hip, render_kernel<.., LEAN>): the hit-set walk alone, units it
cannot finish abandoned and rendered by the full kernel in a redo launch behind it.  Every case renders the same
frames with the knob at 0 (the full kernel alone) and compares bytes and ALL work counters with those, and pixels and
ray counts with the oracle.  The block forms are forced (all whole / all quarters / cells on the zero-component
column), so that a frame's units -- and with them the counters that depend on which rays share a wave -- are the same
under every knob value.

Scene: a soup of a few hundred triangles with one mirror and one glass material, 64x48, depth 5, 3 lights."""
import ctypes

import numpy as np
import pytest

import orclib

pytestmark = pytest.mark.gpu

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding, scenegen, tiling  # noqa: E402

W, H, DEPTH = 64, 48, 5
CAM = (21.3, 14.2, -17.9, 9.0, 13.0, 2.0, 75.0)     # every primary ray has three non-zero direction components
CAM_AXIS = (24.0, 12.0, -20.0, 0.0, 0.0, 0.0, 80.0)  # looks along z: pixel column 32 has d.x == 0, pixel row 24 d.y == 0
LIGHTS = [(13.7, 38.1, 9.3, .1, .1, .1, .7, .7, .7, .5, .5, .5),
          (37.9, 33.3, 21.1, .1, .1, .1, .5, .5, .6, .4, .4, .4),
          (22.1, 41.7, 40.9, .05, .05, .05, .4, .4, .3, .3, .3, .3)]
RAY_KEYS = ("rays_primary", "rays_secondary", "rays_shadow", "shaded_hits")
# QUAD_SHARE, SM_CELL_SHARE (mt_order.h): quarters above QUAD_SHARE x an even share of the frame's cost; cells where a
# block with zero-component rays has quarters above SM_CELL_SHARE x that threshold (1e-3 x 1e6: never)
FORMS = {"whole": (1e6, 0.8), "quarters": (1e-3, 1e6), "cells": (1e-6, 1e-6)}


def lean_info(h):
    return M.hip_abi().lean_info(h)


def counters(stats):
    """Every counter of a launch (ray counts, shaded hits, the traversal's own work, bytes, wave steps): not its durations."""
    return {k: v for k, v in stats.items() if not k.endswith("_ms")}


def soup_triangles():
    rnd = scenegen.SplitMix64(4711)
    S = 48.0
    tris = []
    quads = [([0, 0, 0], [S, 0, 0], [0, 0, S], [S, 0, S]), ([0, 0, S], [S, 0, S], [0, S, S], [S, S, S]),
             ([0, 0, 0], [0, 0, S], [0, S, 0], [0, S, S]), ([S, 0, 0], [S, S, 0], [S, 0, S], [S, S, S])]
    for qi, (a, b, c, d) in enumerate(quads):  # floor (partly mirror), back wall, side walls, each a 4 x 4 grid
        for i in range(4):
            for j in range(4):
                def pt(u, v):
                    return [a[k] + (b[k] - a[k]) * u / 4 + (c[k] - a[k]) * v / 4 for k in range(3)]
                tris.append(([pt(i, j), pt(i + 1, j), pt(i, j + 1)], 1 if (qi == 0 and (i + j) % 2 == 0) else 0))
                tris.append(([pt(i + 1, j + 1), pt(i, j + 1), pt(i + 1, j)], 0))
    for cl in range(4):
        c = [rnd.rng(10, 38), rnd.rng(3, 18), rnd.rng(12, 40)]
        ext = rnd.rng(2.0, 6.0)
        mt = (0, 1, 2, 0)[cl]
        for k in range(45):
            p0 = [c[a] + rnd.rng(-ext, ext) for a in range(3)]
            tris.append(([p0, [p0[a] + rnd.rng(-2.5, 2.5) for a in range(3)], [p0[a] + rnd.rng(-2.5, 2.5) for a in range(3)]], mt))
    return tris


MATS = [("matte", (.3, .3, .3), (.7, .6, .5), (.2, .2, .2), dict(ns=8)),
        ("mirror", (.1, .1, .1), (.2, .2, .2), (.8, .8, .8), dict(ns=60, refl=0.7)),
        ("glass", (.05, .05, .05), (.1, .1, .1), (.6, .6, .6), dict(ns=40, tr=0.4, tf=(.6, .7, .8), ni=1.4))]


def fill(s, tris):
    for name, ka, kd, ks, kw in MATS:
        s.add_material(name, ka, kd, ks, **kw)
    for k, (v, mt) in enumerate(tris):
        s.add_triangle(v, None, mtl=mt, line_no=k)


@pytest.fixture(scope="module")
def soup(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"
    m, o = M.MythTracer(), orclib.OracleScene()
    tris = soup_triangles()
    assert 200 <= len(tris) <= 400
    fill(m, tris)
    fill(o, tris)
    return dict(flat=m.flatten(), oracle=o, keep=m, want={})


def oracle_frame(soup, cam, lights, size=(W, H)):
    """The oracle's frame (with hit points), computed once per (camera, lights, size)."""
    key = (tuple(cam), tuple(map(tuple, lights)), size)
    if key not in soup["want"]:
        soup["oracle"].set_lights(lights)
        soup["want"][key] = soup["oracle"].render(cam, size[0], size[1], max_level=DEPTH, debug=True)
    return soup["want"][key]


def new_scene(soup, lights, forms="whole"):
    abi = M.hip_abi()
    h = abi.scene_create(soup["flat"])
    abi.set_engine(h, 1)
    abi.set_lights(h, lights)
    abi.set_tuning(h, "QUAD_SHARE", FORMS[forms][0])
    abi.set_tuning(h, "SM_CELL_SHARE", FORMS[forms][1])
    return h


def frames(h, cam, knob, n=3, chunk=None, size=(W, H)):
    """n frames of one geometry with the knob at `knob`: the first without a cost history (set_tuning forgets it), the
    others with.  Per frame: the render_chunk result and the lean info."""
    abi = M.hip_abi()
    abi.set_tuning(h, "LEAN_KERNEL", float(knob))
    out = []
    for _ in range(n):
        r = abi.render_chunk(h, binding.sensor(cam, size[0], size[1]), size[0], size[1], chunk=chunk, max_depth=DEPTH)
        r["info"] = lean_info(h)
        out.append(r)
    assert out[0]["info"]["lean"] == 0  # (no history yet: primary_kernel and the full kernel)
    return out


def assert_same_as_full(got, full, what):
    """Bytes and every counter of the library (ray counts, shaded hits, the traversal's own work, bytes, wave steps)."""
    assert len(got) == len(full)
    for i, (a, b) in enumerate(zip(got, full)):
        assert np.array_equal(a["rgb"], b["rgb"]), (what, i)
        assert counters(a["stats"]) == counters(b["stats"]), (what, i)


def assert_like_oracle(r, want, chunk=None):
    ref = want["rgb"] if chunk is None else want["rgb"][chunk[1]:chunk[1] + chunk[3], chunk[0]:chunk[0] + chunk[2]]
    assert np.array_equal(r["rgb"], ref)
    if chunk is None:
        assert {k: r["stats"][k] for k in RAY_KEYS} == {k: want["counters"][k] for k in RAY_KEYS}
        assert r["stats"]["mt_tests"] >= want["counters"]["mt_tests"]


@pytest.mark.parametrize("forms", ["whole", "quarters"])
def test_no_irregular_ray(soup, forms):
    """Knob 1 and knob 2 give the frames and counters of knob 0, and nothing is redone."""
    abi = M.hip_abi()
    want = oracle_frame(soup, CAM, LIGHTS)
    h = new_scene(soup, LIGHTS, forms)
    try:
        full = frames(h, CAM, 0)
        assert all(f["info"]["lean"] == 0 for f in full)
        for knob in (1, 2):
            got = frames(h, CAM, knob)
            assert_same_as_full(got, full, (forms, knob))
            for f in got[1:]:
                assert f["info"]["lean"] == 1 and f["info"]["redo_units"] == 0 and f["info"]["handed_over"] == 0, (forms, knob)
                assert f["info"]["units"] == (48 if forms == "whole" else 192)
                assert_like_oracle(f, want)
    finally:
        abi.scene_destroy(h)


@pytest.mark.parametrize("forms", ["whole", "quarters", "cells"])
def test_axis_aligned_camera(soup, forms):
    """One pixel column (and one row) of primary rays with a zero direction component.  Knob 1 picks the full kernel;
    knob 2 abandons those units at pass 0 -- whole blocks, quarters, and the column's cells, which the lean kernel hands
    over unopened -- and the redo launch renders them."""
    abi = M.hip_abi()
    want = oracle_frame(soup, CAM_AXIS, LIGHTS)
    assert want["counters"]["rays_secondary"] > 0
    h = new_scene(soup, LIGHTS, forms)
    try:
        full = frames(h, CAM_AXIS, 0)
        auto = frames(h, CAM_AXIS, 1)
        assert all(f["info"]["lean"] == 0 for f in auto)
        assert_same_as_full(auto, full, (forms, 1))
        forced = frames(h, CAM_AXIS, 2, n=2)  # (two frames: the second lean launch would hand over, test_device_side_handover)
        assert_same_as_full(forced, full[:2], (forms, 2))
        f = forced[1]
        assert f["info"]["lean"] == 1 and f["info"]["handed_over"] == 0
        # blocks of 8 x 8 pixels: block column 4 and block row 3 hold the zero-component rays
        if forms == "whole":
            assert (f["info"]["units"], f["info"]["redo_units"]) == (48, 6 + 8 - 1)
        elif forms == "quarters":  # the quarters that hold column 32 / row 24
            assert (f["info"]["units"], f["info"]["redo_units"]) == (192, 2 * 6 + 2 * 8 - 1)
        else:  # the cells of those 13 blocks unopened, the other 35 blocks' quarters rendered
            assert (f["info"]["units"], f["info"]["redo_units"]) == (13 * 16 + 35 * 4, 13 * 16)
        assert_like_oracle(f, want)
    finally:
        abi.scene_destroy(h)


def secondary_hit(soup, cam, px, py):
    """The hit point of the reflected ray of pixel (px, py), by TraceRayWorker's own expressions (mythtracer.cc:38-74)."""
    o = soup["oracle"]
    sens = orclib.sensor(cam, W, H)
    d = orclib.sensor_ray(sens, px, py)
    first = o.intersect(np.concatenate([sens[0:3], d]))
    P, n = first["point"][0], first["normal"][0]
    if -(n[0] * d[0]) + -(n[1] * d[1]) + -(n[2] * d[2]) < 0.0:
        n = -n
    k = 2 * (n[0] * d[0] + n[1] * d[1] + n[2] * d[2])
    rd = np.array([d[0] - n[0] * k, d[1] - n[1] * k, d[2] - n[2] * k])
    ro = np.array([P[0] + rd[0] * 0.0001, P[1] + rd[1] * 0.0001, P[2] + rd[2] * 0.0001])
    second = o.intersect(np.concatenate([ro, rd]))
    return second["point"][0], int(second["line"][0])


@pytest.mark.parametrize("case", ["one", "three", "block", "level1"])
@pytest.mark.parametrize("forms", ["whole", "quarters"])
def test_irregular_shadow_ray_mid_unit(soup, case, forms):
    """Regular primary rays, but a light whose x is EXACTLY the x of a pixel's hit point: that pixel's shadow ray has
    d.x == 0, passes into its unit.  The unit is abandoned there (pixels it has stored stay) and redone.  One such pixel
    (its last light: the unit has run the other lights' shadow rays by then), three and all 64 of one block (a light
    per pixel), and one whose shading point is the hit of a reflected ray (recursion level 1)."""
    abi = M.hip_abi()
    base = oracle_frame(soup, CAM, LIGHTS)
    tris = soup_triangles()
    mirror = np.array([mt == 1 for _, mt in tris])
    hit = base["line"] >= 0
    lights = [list(l) for l in LIGHTS]
    if case == "level1":
        ys, xs = np.nonzero(hit & mirror[np.maximum(base["line"], 0)])
        assert len(ys) > 0
        for y, x in zip(ys, xs):
            p2, line2 = secondary_hit(soup, CAM, int(x), int(y))
            if line2 >= 0:
                break
        assert line2 >= 0
        lights[2][0] = float(p2[0])
        n_units = None
    else:
        # a block whose 64 pixels all hit something, at an x no other pixel of the frame hits at (hit points on a wall
        # x = const share their x, exactly, by the dozen)
        xs_all, n_all = np.unique(base["point"][..., 0][hit], return_counts=True)
        once = np.isin(base["point"][..., 0], xs_all[n_all == 1]) & hit
        blocks = [(bx, by) for by in range(H // 8) for bx in range(W // 8) if once[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8].all()]
        assert blocks
        bx, by = blocks[len(blocks) // 2]
        pts = base["point"][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8].reshape(64, 3)
        if case == "one":
            lights[2][0] = float(pts[27][0])
        elif case == "three":  # (pixels (1, 1), (6, 3), (6, 7) of the block: three different quarters)
            for li, p in enumerate((9, 30, 62)):
                lights[li][0] = float(pts[p][0])
        else:
            lights = [[float(pts[p][0]), 30.0 + 0.17 * p, 5.0 + 0.61 * p, .01, .01, .01, .02, .02, .02, .02, .02, .02] for p in range(64)]
        n_units = 1 if forms == "whole" else {"one": 1, "three": 3, "block": 4}[case]
    want = oracle_frame(soup, CAM, lights)
    h = new_scene(soup, lights, forms)
    try:
        full = frames(h, CAM, 0)
        got = frames(h, CAM, 1)
        assert_same_as_full(got, full, (case, forms))
        for f in got[1:]:
            assert f["info"]["lean"] == 1 and f["info"]["handed_over"] == 0
            print(case, forms, "units", f["info"]["units"], "redone", f["info"]["redo_units"])
            assert f["info"]["redo_units"] >= 1  # the irregular ray came up
            if n_units is not None:
                assert f["info"]["redo_units"] == n_units
            assert_like_oracle(f, want)
    finally:
        abi.scene_destroy(h)


def test_device_side_handover(soup):
    """A lean launch that abandons more than the guard's share of its units (13 of 48 here) makes the scene's next lean
    launches hand their whole order to the redo launch, decided on the device: the second frame is rendered by the redo
    launch alone."""
    abi = M.hip_abi()
    want = oracle_frame(soup, CAM_AXIS, LIGHTS)
    h = new_scene(soup, LIGHTS, "whole")
    try:
        full = frames(h, CAM_AXIS, 0, n=4)
        got = frames(h, CAM_AXIS, 2, n=4)
        assert_same_as_full(got, full, "handover")
        a, b, c = got[1]["info"], got[2]["info"], got[3]["info"]
        state = lambda i: tuple(i[k] for k in ("lean", "handed_over", "units", "redo_units"))
        assert state(a) == (1, 0, 48, 13)
        assert state(b) == (1, 1, 48, 48)
        assert state(c) == (1, 1, 48, 48)
        assert_like_oracle(got[2], want)
        # a scene whose histories are forgotten starts its lean launches afresh
        again = frames(h, CAM_AXIS, 2, n=2)
        assert (again[1]["info"]["handed_over"], again[1]["info"]["redo_units"]) == (0, 13)
    finally:
        abi.scene_destroy(h)


def test_chunk_smaller_than_the_image(soup):
    abi = M.hip_abi()
    want = oracle_frame(soup, CAM_AXIS, LIGHTS)
    chunk = (13, 5, 37, 30)  # ragged, through column 32 and row 24
    h = new_scene(soup, LIGHTS, "whole")
    try:
        full = frames(h, CAM_AXIS, 0, chunk=chunk)
        got = frames(h, CAM_AXIS, 2, n=2, chunk=chunk)
        assert_same_as_full(got, full[:2], "chunk")
        assert got[1]["info"]["lean"] == 1 and got[1]["info"]["redo_units"] > 0
        assert_like_oracle(got[1], want, chunk)
    finally:
        abi.scene_destroy(h)


def test_tile_list_launch_and_cost_map(soup):
    """A tile-list launch (half of the image's 16 x 16 tiles, kept for three frames) through the lean kernel with abandoned
    units; and the cost map of a frame with abandoned units: every block of the launch present and non-zero, as with
    knob 0 (the cycles themselves are measurements)."""
    import torch
    abi = M.hip_abi()
    want = oracle_frame(soup, CAM_AXIS, LIGHTS)
    T = 16
    tx, ty = tiling.tile_grid(W, H, T, T)
    tiles = [t for t in range(tx * ty) if (t // tx + t % tx) % 2 == 0 or t % tx == 2]
    lst = torch.tensor(tiles, dtype=torch.int32, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    mw, mh = (W + 7) // 8, (H + 7) // 8
    sens = binding.sensor(CAM_AXIS, W, H)
    h = new_scene(soup, LIGHTS, "whole")
    try:
        results = {}
        for knob in (0, 2):
            abi.set_tuning(h, "LEAN_KERNEL", float(knob))
            for frame_no in range(2):
                slots = torch.zeros(len(tiles) * tiling.slot_bytes(T, T), dtype=torch.uint8, device="cuda")
                frame = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
                abi.render_tile_list_device(h, sens, W, H, T, T, vp(lst), len(tiles), 7 + knob, DEPTH, vp(slots))
                abi.blit_tile_list_device(h, W, H, T, T, vp(lst), len(tiles), vp(slots), vp(frame))
                cm = torch.zeros((mh, mw), dtype=torch.int32, device="cuda")
                abi.export_costs_device(h, vp(cm), mw, mh)
                torch.cuda.synchronize()
                info = lean_info(h)
                results[(knob, frame_no)] = (frame.cpu().numpy(), abi.read_stats(h), cm.cpu().numpy(), info)
        own = np.zeros((H, W), dtype=bool)
        for t in tiles:
            x, y, cw, ch = tiling.tile_rect(t, W, H, T, T)
            own[y:y + ch, x:x + cw] = True
        for frame_no in range(2):
            a, b = results[(0, frame_no)], results[(2, frame_no)]
            assert np.array_equal(a[0], b[0]) and counters(a[1]) == counters(b[1]), frame_no
            assert np.array_equal(a[0][own], want["rgb"][own])
            assert np.array_equal(a[2] != 0, own[::8, ::8]) and np.array_equal(b[2] != 0, own[::8, ::8]), frame_no
        info = results[(2, 1)][3]
        assert info["lean"] == 1 and info["handed_over"] == 0 and 0 < info["redo_units"] < info["units"]
        assert results[(0, 1)][3]["lean"] == 0
    finally:
        abi.scene_destroy(h)


@pytest.mark.parametrize("ext,jit,depth", [(0.01, 0.002, 13), (0.0003, 0.00006, 18)])
def test_deep_layouts(ext, jit, depth, native_libs):
    """The DEEP = 1 and DEEP = 2 instantiations (octrees of 12 .. 16 and 17 .. 24 levels: a tight cluster of small
    triangles in a big room, as in test_gpu_parity.test_deep_octrees), looking straight at the cluster along z: regular
    units through the lean kernel, the zero-component column and row abandoned and redone."""
    abi = M.hip_abi()
    rnd = scenegen.SplitMix64(77)
    m, o = M.MythTracer(), orclib.OracleScene()
    tris = [[[0, 0, 0], [64, 0, 0], [0, 0, 64]], [[64, 0, 64], [0, 0, 64], [64, 0, 0]]]
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
    lights = [(30, 40, 20, .2, .2, .2, .8, .8, .8, .4, .4, .4)]
    cam = (20.0 + ext / 2, 3.0 + ext / 2, 29.9, 0.0, 0.0, 0.0, min(8.0, 800.0 * ext))
    o.set_lights(lights)
    want = o.render(cam, 64, 64, max_level=DEPTH)
    h = abi.scene_create(m.flatten())
    try:
        abi.set_engine(h, 1)
        abi.set_lights(h, lights)
        abi.set_tuning(h, "QUAD_SHARE", 1e6)
        full = frames(h, cam, 0, n=2, size=(64, 64))
        got = frames(h, cam, 2, n=2, size=(64, 64))
        assert_same_as_full(got, full, depth)
        f = got[1]
        assert f["info"]["lean"] == 1 and (f["info"]["units"], f["info"]["redo_units"]) == (64, 15)
        assert_like_oracle(f, want)
    finally:
        abi.scene_destroy(h)


def test_knob_values(soup):
    abi = M.hip_abi()
    h = new_scene(soup, LIGHTS)
    try:
        for bad in (-1.0, 0.5, 3.0):
            with pytest.raises(RuntimeError):
                abi.set_tuning(h, "LEAN_KERNEL", bad)
    finally:
        abi.scene_destroy(h)
