"""The work order of a launch (csrc/mt_order.h: order_forecast_kernel, order_count_kernel, order_scatter_kernel;
build_region_table of csrc/mt_queues.h) on cost maps planted word by word and with every tuning knob at the ends of its
range (tests/schedule_inputs.py).  A wrong order leaves the arithmetic intact and loses pixels or renders them twice, so
every frame of every case is compared
  * byte for byte with the first, unordered frame of a newly created scene (same camera, same chunk),
  * with the oracle's frame under the suite's rule for frames that use pow (1 LSB on at most 0.01 % of the pixels),
  * in its ray counters (primary, shadow, secondary rays, shaded hits) with the oracle's: a unit rendered twice paints
    the right pixels and shows only there,
and, where the launch is the lean kernel's, mt_scene_lean_info().units with the count the planted words must give: that
is what proves the words were read.  After a frame the exported cost map is non-zero on exactly the launch's blocks.

Scene: the lean-kernel tests' soup (308 triangles, a mirror and a glass material), 96 x 64, depth 3, two lights."""
import ctypes

import numpy as np
import pytest

import schedule_inputs as si

pytestmark = pytest.mark.gpu

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding, tiling  # noqa: E402

SIZE = (si.W, si.H)
# name -> (engine, MT_TUNE_XCD_QUEUES, MT_TUNE_LEAN_KERNEL)
SETTINGS = {"sm-q0-full": (1, 0, 0), "sm-q0-lean": (1, 0, 2), "sm-q1-full": (1, 1, 0), "sm-q1-lean": (1, 1, 2),
            "sm-q2-full": (1, 2, 0), "sm-q2-lean": (1, 2, 2), "pool": (2, None, None), "hybrid": (3, None, None)}
ENGINES = {"sm": 1, "pool": 2, "hybrid": 3}


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def ctx(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"
    tris, mats = si.scene_description()
    m = M.MythTracer()
    si.fill(m, tris, mats)
    return dict(flat=m.flatten(), keep=m, unordered={})


def new_scene(ctx, engine, xcd=None, lean=None):
    abi = M.hip_abi()
    h = abi.scene_create(ctx["flat"])
    abi.set_engine(h, engine)
    abi.set_lights(h, si.LIGHTS)
    if xcd is not None:
        abi.set_tuning(h, "XCD_QUEUES", float(xcd))
    if lean is not None:
        abi.set_tuning(h, "LEAN_KERNEL", float(lean))
    return h


def forget(h):
    """mt_scene_set_tuning forgets the scene's histories: the next frame is a first frame."""
    M.hip_abi().set_tuning(h, "MULTI_BALANCE", 1.0)


def render(h, cam, size=SIZE, chunk=None):
    abi = M.hip_abi()
    r = abi.render_chunk(h, binding.sensor(si.CAMERAS[cam], size[0], size[1]), size[0], size[1], chunk=chunk, max_depth=si.DEPTH)
    r["info"] = abi.lean_info(h)
    return r


def like_oracle(rgb, stats, cam, size, chunk, what):
    want = si.oracle_frame(cam, size, chunk)
    ok, n_diff, mx = si.rgb_close(rgb, want["rgb"])
    assert ok, (what, "against the oracle: %d pixels differ, max %d" % (n_diff, mx))
    assert {k: stats[k] for k in si.RAY_KEYS} == {k: want["counters"][k] for k in si.RAY_KEYS}, what


def unordered(ctx, cam, size=SIZE, chunk=None):
    """The first frame of a newly created scene: no history, no work order.  Once per (camera, size, chunk)."""
    key = (cam, size, chunk)
    if key not in ctx["unordered"]:
        abi = M.hip_abi()
        h = new_scene(ctx, 1)
        try:
            r = render(h, cam, size, chunk)
        finally:
            abi.scene_destroy(h)
        assert r["info"]["lean"] == 0
        like_oracle(r["rgb"], r["stats"], cam, size, chunk, ("unordered", key))
        ctx["unordered"][key] = r["rgb"]
    return ctx["unordered"][key]


def check_frame(ctx, r, cam, what, size=SIZE, chunk=None):
    assert np.array_equal(r["rgb"], unordered(ctx, cam, size, chunk)), (what, "differs from the unordered frame")
    like_oracle(r["rgb"], r["stats"], cam, size, chunk, what)
    info = r["info"]
    if info["lean"]:
        bw, bh = si.blocks_of(size, chunk)
        assert bw * bh <= info["units"] <= 16 * bw * bh, what  # (order_item holds 16 per block)
        assert info["redo_units"] <= info["units"], what
        if info["handed_over"]:
            assert info["redo_units"] == info["units"], what


def import_map(ctx, h, m):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(m).view(np.int32).copy()).cuda()
    M.hip_abi().import_costs_device(h, vp(d), m.shape[1], m.shape[0])
    return d  # (alive until the launch that reads the scene's copy has been waited for)


def check_export(h, own, what, size=SIZE):
    """mt_scene_export_costs_device into a zeroed map: non-zero on exactly the launch's blocks."""
    import torch
    mw, mh = si.blocks_of(size)
    cm = torch.zeros((mh, mw), dtype=torch.int32, device="cuda")
    M.hip_abi().export_costs_device(h, vp(cm), mw, mh)
    torch.cuda.synchronize()
    assert np.array_equal(cm.cpu().numpy() != 0, own), what


def exportable(chunk):
    """mt_scene_export_costs_device takes launches whose region and tiles lie on the 8-pixel grid."""
    return chunk is None or all(v % 8 == 0 for v in chunk)


def chunk_blocks(chunk, size=SIZE):
    mw, mh = si.blocks_of(size)
    own = np.zeros((mh, mw), dtype=bool)
    x, y, cw, ch = chunk or (0, 0) + size
    own[y // 8:(y + ch + 7) // 8, x // 8:(x + cw + 7) // 8] = True
    return own


def set_shares(h, share):
    if share is not None:
        abi = M.hip_abi()
        abi.set_tuning(h, "QUAD_SHARE", share)
        abi.set_tuning(h, "QUAD_SHARE_MOVING", share)


# ---------------------------------------------------------------------------------------------------------------------
# 1. planted map, translated camera
def planted_sequence(ctx, h, m, share, lean, what, size=SIZE, chunk=None):
    """Frame 0 at the base camera (unordered), the map, frame 1 translated (block b's forecast = its map word), frame 2
    translated again (no map: the scene's own costs, re-projected)."""
    forget(h)
    f0 = render(h, "base", size, chunk)
    assert f0["info"]["lean"] == 0
    check_frame(ctx, f0, "base", (what, 0), size, chunk)
    keep = import_map(ctx, h, m)
    f1 = render(h, "translated", size, chunk)
    check_frame(ctx, f1, "translated", (what, 1), size, chunk)
    assert f1["info"]["lean"] == (1 if lean == 2 else 0), what
    units = None
    if lean == 2:
        units = si.predicted_units(si.planted_words(m, size, chunk), share)
        if units is not None:
            assert f1["info"]["units"] == units, (what, "units of the planted words")
    if exportable(chunk):
        check_export(h, chunk_blocks(chunk, size), (what, "export"), size)
    f2 = render(h, "translated2", size, chunk)
    check_frame(ctx, f2, "translated2", (what, 2), size, chunk)
    del keep
    return units


@pytest.mark.parametrize("share", list(si.SHARES))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_planted_map_translated_camera(ctx, setting, share):
    abi = M.hip_abi()
    engine, xcd, lean = SETTINGS[setting]
    h = new_scene(ctx, engine, xcd, lean)
    try:
        abi.set_tuning(h, "FORECAST_RADIUS", 0.0)
        set_shares(h, si.SHARES[share])
        predicted = 0
        for name, m in si.cost_maps(*si.blocks_of()).items():
            units = planted_sequence(ctx, h, m, si.SHARES[share], lean, (setting, share, name))
            predicted += units is not None
        if lean == 2 and share != "default":
            assert predicted >= 8
    finally:
        abi.scene_destroy(h)


@pytest.mark.parametrize("setting", ["sm-q2-lean", "sm-q1-full", "pool", "hybrid"])
def test_planted_map_ragged_chunk(ctx, setting):
    """A chunk off the 8-pixel grid: block (i, j) of the launch reads the map word of the image block its centre lies in."""
    abi = M.hip_abi()
    engine, xcd, lean = SETTINGS[setting]
    h = new_scene(ctx, engine, xcd, lean)
    try:
        abi.set_tuning(h, "FORECAST_RADIUS", 0.0)
        set_shares(h, 1e-6)
        predicted = 0
        for name, m in si.cost_maps(*si.blocks_of()).items():
            units = planted_sequence(ctx, h, m, 1e-6, lean, (setting, "ragged", name), chunk=si.RAGGED_CHUNK)
            predicted += units is not None
        if lean == 2:
            assert predicted >= 8
    finally:
        abi.scene_destroy(h)


@pytest.mark.parametrize("setting", ["sm-q2-lean", "sm-q1-lean", "pool", "hybrid"])
def test_planted_bucket_edges_on_576_blocks(ctx, setting):
    """Every bucket edge and the value below it (more than 200 distinct buckets), the ramps and a random map at 256 x 144."""
    abi = M.hip_abi()
    engine, xcd, lean = SETTINGS[setting]
    h = new_scene(ctx, engine, xcd, lean)
    try:
        abi.set_tuning(h, "FORECAST_RADIUS", 0.0)
        set_shares(h, 1e-6)
        maps = si.cost_maps(*si.blocks_of(si.BIG))
        assert len(np.unique(si.unit_buckets(maps["bucket_edges"]))) >= 200
        for name in ("bucket_edges", "ramp_down", "random_2", "checker_bit31_1000"):
            units = planted_sequence(ctx, h, maps[name], 1e-6, lean, (setting, "big", name), size=si.BIG)
            assert lean != 2 or name == "bucket_edges" or units is not None
    finally:
        abi.scene_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------
# 2. planted map, from_map: tile-list launches whose list changes with every launch, the axis camera at rest
def list_launch(ctx, h, tiles, list_id, what):
    """One tile-list launch, blitted: (frame, ray counters, lean info)."""
    import torch
    abi = M.hip_abi()
    w, hh = SIZE
    lst = torch.tensor(tiles, dtype=torch.int32, device="cuda")
    slots = torch.zeros(len(tiles) * tiling.slot_bytes(si.T, si.T), dtype=torch.uint8, device="cuda")
    frame = torch.zeros((hh, w, 3), dtype=torch.uint8, device="cuda")
    sens = binding.sensor(si.CAMERAS["axis"], w, hh)
    abi.render_tile_list_device(h, sens, w, hh, si.T, si.T, vp(lst), len(tiles), list_id, si.DEPTH, vp(slots))
    abi.blit_tile_list_device(h, w, hh, si.T, si.T, vp(lst), len(tiles), vp(slots), vp(frame))
    torch.cuda.synchronize()
    info = abi.lean_info(h)
    stats = abi.read_stats(h)
    rgb = frame.cpu().numpy()
    own_px = np.repeat(np.repeat(si.list_blocks(tiles), 8, axis=0), 8, axis=1)
    assert np.array_equal(rgb[own_px], unordered(ctx, "axis")[own_px]), (what, "differs from the unordered frame")
    assert not rgb[~own_px].any(), what
    ok, n_diff, mx = si.rgb_close(rgb[own_px][None], si.oracle_frame("axis")["rgb"][own_px][None])
    assert ok, (what, n_diff, mx)
    assert {k: stats[k] for k in si.RAY_KEYS} == si.oracle_tiles("axis", tiles), what
    if info["lean"]:
        assert info["redo_units"] <= info["units"], what
        if info["handed_over"]:
            assert info["redo_units"] == info["units"], what
    return info


@pytest.mark.parametrize("setting", ["sm-q0-full", "sm-q0-lean", "sm-q2-full", "sm-q2-lean", "pool", "hybrid"])
def test_planted_map_changed_tile_list(ctx, setting):
    abi = M.hip_abi()
    engine, xcd, lean = SETTINGS[setting]
    lists = si.half_lists()
    zb = si.zero_component_blocks(binding.sensor(si.CAMERAS["axis"], si.W, si.H), si.W, si.H)
    h = new_scene(ctx, engine, xcd, lean)
    try:
        set_shares(h, 1e-6)
        abi.set_tuning(h, "SM_CELL_SHARE", 1e-6)
        abi.read_stats(h)
        predicted = 0
        for name, m in si.cost_maps(*si.blocks_of()).items():
            what = (setting, name)
            forget(h)
            info = list_launch(ctx, h, lists[0], 1, (what, 0))  # no history: unordered
            assert info["lean"] == 0
            for k in (1, 2, 3):
                tiles = lists[k % 2]
                own = si.list_blocks(tiles)
                keep = import_map(ctx, h, m)
                info = list_launch(ctx, h, tiles, 1 + k, (what, k))
                del keep
                check_export(h, own, (what, k, "export"))
                if lean != 2:
                    assert info["lean"] == 0
                    continue
                assert info["lean"] == 1, what
                units = si.predicted_units(m[own], 1e-6, cells=zb[own])
                if units is not None:
                    predicted += k == 1
                    assert info["units"] == units, (what, k, "units of the planted words")
                    if not info["handed_over"]:  # the cells are handed to the redo launch unopened
                        assert info["redo_units"] >= 16 * int((zb[own] & (si.cost_of(m[own]) > 0)).sum()), (what, k)
                if name == "all_1":  # every block cut: sixteen units for each one that holds a zero-component ray
                    nz = int(zb[own].sum())
                    assert nz >= 8 and info["units"] == 16 * nz + 4 * (int(own.sum()) - nz)
        if lean == 2:
            assert predicted >= 8
    finally:
        abi.scene_destroy(h)


@pytest.mark.parametrize("setting", ["sm-q0-lean", "sm-q2-lean"])
def test_cells_in_the_first_bucket(ctx, setting):
    """Bucket 0 takes units of 0xf0000000 and more, which a 31-bit cost reaches only through a time factor above 2: the
    cells of the axis camera's column and row under MT_TUNE_SM_CELL_TIME = 1e6, whose expected time (unsigned)(cost x
    1e6) saturates for every cost from 4 295 on.  The unit count shows that those blocks did go out as cells: sixteen
    units each, keyed (region, bucket 0), while the other blocks' quarters and the blocks of cost 0 (bucket 255) keep theirs."""
    abi = M.hip_abi()
    engine, xcd, lean = SETTINGS[setting]
    lists = si.half_lists()
    zb = si.zero_component_blocks(binding.sensor(si.CAMERAS["axis"], si.W, si.H), si.W, si.H)
    maps = si.cost_maps(*si.blocks_of())
    h = new_scene(ctx, engine, xcd, lean)
    try:
        set_shares(h, 1e-6)
        abi.set_tuning(h, "SM_CELL_SHARE", 1e-6)
        abi.set_tuning(h, "SM_CELL_TIME", 1e6)
        abi.read_stats(h)
        for name in ("all_7fffffff", "all_ffffffff", "all_0", "random_1", "one_row"):
            m = maps[name]
            forget(h)
            list_launch(ctx, h, lists[0], 1, (setting, name, 0))
            own = si.list_blocks(lists[1])
            cell_costs = si.cost_of(m[own][zb[own]])
            cell_costs = cell_costs[cell_costs > 0]
            assert len(cell_costs) >= 4 and (si.unit_buckets(cell_costs, 1e6) == 0).all(), name
            keep = import_map(ctx, h, m)
            info = list_launch(ctx, h, lists[1], 2, (setting, name, 1))
            del keep
            assert info["lean"] == 1 and info["units"] == si.predicted_units(m[own], 1e-6, cells=zb[own]), name
            assert info["units"] >= int(own.sum()) + 15 * len(cell_costs)
            check_export(h, own, (setting, name, "export"))
    finally:
        abi.scene_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the knobs at the ends of their ranges
def knob_sequence(ctx, h, what):
    """Three frames at rest (a measured history; MT_TUNE_BLEND acts from the third), one frame turned by 2 degrees, one
    translated frame on the random planted map."""
    for k in range(3):
        check_frame(ctx, render(h, "base"), "base", (what, k))
    check_frame(ctx, render(h, "yaw2"), "yaw2", (what, "yaw2"))
    keep = import_map(ctx, h, si.cost_maps(*si.blocks_of())["random_1"])
    check_frame(ctx, render(h, "translated"), "translated", (what, "planted"))
    del keep
    check_export(h, chunk_blocks(None), (what, "export"))


def pool_declines(engine, knob, end):
    """decide_launch's own rule (mt_capi.hip, pool_fits): engine 2 by request is refused when even the smallest pool --
    64 + 128 + 4 (depth + 1) + 64 records of 160 + 80 lights bytes and 4 lights + 4 bytes of pool entries, per resident
    wave -- does not fit four times MT_TUNE_POOL_SCRATCH_MB.  The launch keeps at least one wave per compute unit
    resident, so with a budget of 1 MB the pool is refused on any device of 47 compute units or more (the MI355X: 256)."""
    if not (engine == 2 and knob == "POOL_SCRATCH_MB"):
        return False
    import torch
    n_l = len(si.LIGHTS)
    floor_cap = 64 + 128 + 4 * (si.DEPTH + 1) + 64
    per_rec = 160 + 80 * n_l + 4 * n_l + 4
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert floor_cap * per_rec * n_cu > 4.0 * end * 1048576.0, "a device this small: the rule's outcome depends on its waves per unit"
    return True


@pytest.mark.parametrize("knob", sorted(si.KNOB_ENDS))
@pytest.mark.parametrize("engine", list(ENGINES))
def test_one_knob_at_each_end(ctx, engine, knob):
    """Engine 2 with MT_TUNE_POOL_SCRATCH_MB = 1 renders nothing: the launch is refused, at once and by name (engine 3
    renders the same launches without a pool, engine 1 does not read the knob)."""
    abi = M.hip_abi()
    for end in si.KNOB_ENDS[knob]:
        h = new_scene(ctx, ENGINES[engine])
        try:
            abi.set_tuning(h, knob, end)
            if pool_declines(ENGINES[engine], knob, end):
                with pytest.raises(RuntimeError, match="scratch budget"):
                    render(h, "base")
            else:
                knob_sequence(ctx, h, (engine, knob, end))
        finally:
            abi.scene_destroy(h)


@pytest.mark.parametrize("end", [0, 1], ids=["low", "high"])
@pytest.mark.parametrize("engine", list(ENGINES))
def test_all_shares_and_factors_at_one_end(ctx, engine, end):
    """Everything in [1e-6, 1e6] at 1e-6 together (every block in sixteen pieces where the engine has them: order_item
    holds exactly 16 per block), then at 1e6 together."""
    abi = M.hip_abi()
    h = new_scene(ctx, ENGINES[engine])
    try:
        for knob in si.UNIT_RANGE:
            abi.set_tuning(h, knob, si.KNOB_ENDS[knob][end])
        knob_sequence(ctx, h, (engine, "all", end))
    finally:
        abi.scene_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------
# 4. degenerate launches with a history
@pytest.mark.parametrize("groups", [1, 256])
@pytest.mark.parametrize("engine", list(ENGINES))
def test_degenerate_chunks_with_a_history(ctx, engine, groups):
    """One pixel, one block, four partial blocks -- four frames each, so that the order kernels run on a history of one
    to four blocks (256 workgroups for 1 .. 4 blocks)."""
    abi = M.hip_abi()
    h = new_scene(ctx, ENGINES[engine])
    try:
        abi.set_tuning(h, "ORDER_GROUPS", float(groups))
        for chunk in si.DEGENERATE_CHUNKS:
            for k in range(4):
                r = render(h, "base", chunk=chunk)
                check_frame(ctx, r, "base", (engine, groups, chunk, k), chunk=chunk)
            if exportable(chunk):
                check_export(h, chunk_blocks(chunk), (engine, groups, chunk, "export"))
    finally:
        abi.scene_destroy(h)


@pytest.mark.parametrize("groups", [1, 3, 256])
def test_576_blocks_on_any_number_of_workgroups(ctx, groups):
    abi = M.hip_abi()
    h = new_scene(ctx, 1, lean=2)
    try:
        abi.set_tuning(h, "ORDER_GROUPS", float(groups))
        set_shares(h, 1e6)
        for k in range(3):
            r = render(h, "base", si.BIG)
            check_frame(ctx, r, "base", (groups, k), si.BIG)
            if k > 0:
                assert r["info"]["lean"] == 1 and r["info"]["units"] == 576
        check_export(h, chunk_blocks(None, si.BIG), (groups, "export"), si.BIG)
    finally:
        abi.scene_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------
# 5. real re-projection moves
@pytest.mark.parametrize("move", ["yaw180", "roll90", "far"])
@pytest.mark.parametrize("engine", list(ENGINES))
def test_reprojection_moves(ctx, engine, move):
    """A camera that sees nothing of the old frame (lambda < 0), one rolled by 90 degrees, one translated far away;
    MT_TUNE_FORECAST_RADIUS 0 and 8, MT_TUNE_FORECAST_STEP at both ends; the scene's own costs, a planted map, and a
    planted map SMALLER than the image's blocks (the bounds branch of the lookup: those blocks count as unseen)."""
    abi = M.hip_abi()
    maps = {"own": None, "map": si.cost_maps(*si.blocks_of())["random_2"], "small": si.cost_maps(5, 3)["random_1"]}
    h = new_scene(ctx, ENGINES[engine], lean=2 if engine == "sm" else None)
    try:
        for radius in (0.0, 8.0):
            abi.set_tuning(h, "FORECAST_RADIUS", radius)
            for step in (1e-6, 1e6):
                abi.set_tuning(h, "FORECAST_STEP", step)
                for name, m in maps.items():
                    what = (engine, move, radius, step, name)
                    forget(h)
                    check_frame(ctx, render(h, "base"), "base", (what, 0))
                    check_frame(ctx, render(h, "base"), "base", (what, 1))
                    keep = import_map(ctx, h, m) if m is not None else None
                    r = render(h, move)
                    check_frame(ctx, r, move, (what, 2))
                    del keep
                    check_export(h, chunk_blocks(None), (what, "export"))
                    if engine == "sm":
                        assert r["info"]["lean"] == 1
    finally:
        abi.scene_destroy(h)
