"""Inputs for the work order of a launch (csrc/mt_order.h, csrc/mt_queues.h) that no measured frame produces: cost maps
planted word by word, every tuning knob at the ends of its range, and the cameras that bring a planted map to the
blocks unchanged.  Fixed seeds, numpy only, no GPU: tests/test_schedule_inputs_cpu.py holds the generators to what
they promise, tests/test_gpu_schedules.py feeds them to the library.  Test infrastructure.

Two public inputs let a test choose every block's forecast word exactly:
  * mt_scene_import_costs_device, then a launch whose camera was only TRANSLATED: start_point, delta_pixel and
    delta_scanline of a sensor are directions (host/src/camera.cc:49-51) and do not change, the re-projection of
    forecast_item is the identity, and with MT_TUNE_FORECAST_RADIUS = 0 block b's forecast is the map word at its
    centre, verbatim (a zero word: "nobody reported it", the unseen guess UNSEEN);
  * the same import, then a tile-list launch whose list differs from the previous launch's (P.from_map): the map word
    at the block's own position, camera at rest, cells allowed.
"""
from __future__ import annotations

import numpy as np

# ---------------------------------------------------------------------------------------------------------------------
# 1. scene, sizes, cameras
W, H, DEPTH = 96, 64, 3          # 12 x 8 blocks
BIG = (256, 144)                 # 32 x 18 = 576 blocks, only where a test says so
T = 16                           # tile side of the list launches: 6 x 4 tiles, 2 x 2 blocks each
RAY_KEYS = ("rays_primary", "rays_secondary", "rays_shadow", "shaded_hits")
UNSEEN = 16000                   # ForecastArgs::unseen (mt_capi.hip, launch_work_order)

# (x, y, z, pitch, yaw, roll, angle of view)
CAMERAS = {
    "base": (21.3, 14.2, -17.9, 9.0, 13.0, 2.0, 75.0),   # every primary ray has three non-zero direction components
    "translated": (21.67, 13.99, -17.75, 9.0, 13.0, 2.0, 75.0),
    "translated2": (21.1, 14.45, -18.2, 9.0, 13.0, 2.0, 75.0),
    "axis": (24.0, 12.0, -20.0, 0.0, 0.0, 0.0, 80.0),    # looks along z: one pixel column has d.x == 0, one row d.y == 0
    "yaw2": (21.3, 14.2, -17.9, 9.0, 15.0, 2.0, 75.0),
    "yaw180": (21.3, 14.2, -17.9, 9.0, 193.0, 2.0, 75.0),  # every new direction unseen (lambda < 0)
    "roll90": (21.3, 14.2, -17.9, 9.0, 13.0, 92.0, 75.0),
    "far": (2021.3, -1985.8, -4017.9, 9.0, 13.0, 2.0, 75.0),  # a translation far outside the scene (the soup is 48 wide)
}
LIGHTS = [(13.7, 38.1, 9.3, .1, .1, .1, .7, .7, .7, .5, .5, .5),
          (37.9, 33.3, 21.1, .1, .1, .1, .5, .5, .6, .4, .4, .4)]
RAGGED_CHUNK = (5, 3, 83, 57)
DEGENERATE_CHUNKS = [(0, 0, 1, 1), (95, 63, 1, 1), (0, 0, 8, 8), (4, 4, 8, 8)]  # the last one: four partial blocks


def scene_description():
    """(triangles, materials) of the lean-kernel tests' soup: 308 triangles, a mirror and a glass material."""
    import test_gpu_lean_kernel as lean  # (imported late: this module itself needs numpy only)
    return lean.soup_triangles(), lean.MATS


def fill(scene, tris, mats):
    for name, ka, kd, ks, kw in mats:
        scene.add_material(name, ka, kd, ks, **kw)
    for k, (v, mt) in enumerate(tris):
        scene.add_triangle(v, None, mtl=mt, line_no=k)


def blocks_of(size=(W, H), chunk=None):
    """(bw, bh) of a launch: the 8 x 8 blocks of its chunk, counted from the chunk's corner."""
    cw, ch = (chunk[2], chunk[3]) if chunk else size
    return (cw + 7) // 8, (ch + 7) // 8


def zero_component_pixels(sensor12, w, h):
    """bool[h, w]: the primary ray start + ds y + dp x (camera.cc:55) has a component that is exactly 0."""
    s = np.asarray(sensor12, dtype=np.float64)
    start, ds, dp = s[3:6], s[6:9], s[9:12]
    y = np.arange(h, dtype=np.float64)[:, None, None]
    x = np.arange(w, dtype=np.float64)[None, :, None]
    d = (start + ds * y) + dp * x
    return (d == 0.0).any(axis=-1)


def zero_component_blocks(sensor12, w, h):
    z = zero_component_pixels(sensor12, w, h)
    bw, bh = (w + 7) // 8, (h + 7) // 8
    out = np.zeros((bh, bw), dtype=bool)
    for by in range(bh):
        for bx in range(bw):
            out[by, bx] = z[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8].any()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 2. the bucket rule (mt_render.hip, cost_bucket; mt_pool.h's pool_cost_bucket is the same rule)
N_BUCKETS = 256


def cost_bucket(c):
    """Descending cost = ascending bucket: 255 for 0, else 255 - (8 octave + the eighth within it)."""
    c = np.asarray(c, dtype=np.uint64)
    safe = np.maximum(c, 1)
    e = np.zeros(c.shape, dtype=np.int64)
    for k in range(1, 32):
        e[safe >= (1 << k)] = k
    shift = np.maximum(e - 3, 0).astype(np.uint64)
    f = np.where(e >= 3, (safe >> shift) & np.uint64(7), 0).astype(np.int64)
    return np.where(c == 0, N_BUCKETS - 1, N_BUCKETS - 1 - (e * 8 + f)).astype(np.int64)


def bucket_edges():
    """Every first value of a bucket with eighths, (8 + f) << (e - 3), e = 3 .. 30 (costs have 31 bits)."""
    return [(8 + f) << (e - 3) for e in range(3, 31) for f in range(8)]


def cost_of(words):
    """The cost a state-machine launch reads from planted forecast words: bit 31 off, a zero word the unseen guess."""
    w = np.asarray(words, dtype=np.uint64)
    return np.where(w == 0, UNSEEN, w & np.uint64(0x7fffffff)).astype(np.uint64)


def unit_buckets(words, time_factor=1.0):
    """Buckets of the units made from `words` when a unit's expected time is cost x time_factor (1: whole blocks;
    kQuarterTime, MT_TUNE_SM_CELL_TIME, MT_TUNE_POOL_PIECE_TIME*: pieces), the float -> unsigned conversion saturating."""
    unit = np.minimum(np.floor(cost_of(words).astype(np.float64) * time_factor), float(2 ** 32 - 1)).astype(np.uint64)
    return cost_bucket(unit)


# ---------------------------------------------------------------------------------------------------------------------
# 3. cost-map patterns
HOT, BIT31 = 0x7fffffff, 0x80000000


def cost_maps(bw, bh):
    """name -> uint32[bh, bw], block b = by * bw + bx."""
    n = bw * bh
    b = np.arange(n, dtype=np.uint64)
    by, bx = np.divmod(np.arange(n), bw)
    checker = (bx + by) % 2 == 0
    out = {}
    for name, word in (("all_0", 0), ("all_1", 1), ("all_7fffffff", HOT), ("all_80000000", BIT31), ("all_ffffffff", 0xffffffff)):
        out[name] = np.full(n, word, dtype=np.uint64)
    for name, at in (("hot_first", 0), ("hot_last", n - 1), ("hot_middle", (bh // 2) * bw + bw // 2)):
        m = np.ones(n, dtype=np.uint64)
        m[at] = HOT
        out[name] = m
    out["checker_1_2p30"] = np.where(checker, 1, 1 << 30)
    out["checker_bit31_1000"] = np.where(checker, BIT31, 1000)
    out["checker_0_1000"] = np.where(checker, 0, 1000)
    out["ramp_up"] = b + 1
    out["ramp_down"] = n - b
    out["octaves"] = np.uint64(1) << (b % np.uint64(31))
    # bucket edges and the value below each: as many edges as fit, spread evenly over the octaves
    edges = bucket_edges()
    take = max(1, min(len(edges), n // 2))
    pick = [edges[int(round(k))] for k in np.linspace(0, len(edges) - 1, take)]
    vals = [v for e in pick for v in (e, e - 1)]
    out["bucket_edges"] = np.array((vals * (n // len(vals) + 1))[:n], dtype=np.uint64)
    # all cost in one place, the other blocks with bit 31 and cost 0: the region cuts coincide, queues stay empty
    for name, where in (("left_column", bx == 0), ("one_row", by == bh // 2), ("corner", (bx == bw - 1) & (by == bh - 1))):
        out[name] = np.where(where, 100000, BIT31)
    for seed in (1, 2):
        out["random_%d" % seed] = np.random.default_rng(seed).integers(0, 2 ** 32, n, dtype=np.uint64)
    return {k: np.asarray(v).astype(np.uint32).reshape(bh, bw) for k, v in out.items()}


PATTERNS = tuple(cost_maps(1, 1))
SHARES = {"low": 1e-6, "default": None, "high": 1e6}   # MT_TUNE_QUAD_SHARE and _MOVING together


def planted_words(cost_map, size=(W, H), chunk=None):
    """uint32[bh, bw]: the map word every block of the launch reads, by the map lookup of forecast_item -- the word at
    (block centre) >> 3 in image coordinates, or 0 outside the map (the bounds branch: unseen).  The centre of a
    partial block at the chunk's right or lower edge lies outside the chunk: forecast_item takes such a position to
    half a pixel inside the edge."""
    cx, cy, cw, ch = chunk if chunk else (0, 0) + tuple(size)
    bw, bh = blocks_of(size, chunk)
    mh, mw = cost_map.shape
    out = np.zeros((bh, bw), dtype=np.uint32)
    for j in range(bh):
        for i in range(bw):
            mx, my = int(min(cx + 8 * i + 4, cx + cw - 0.5)) >> 3, int(min(cy + 8 * j + 4, cy + ch - 0.5)) >> 3
            if mx < mw and my < mh:
                out[j, i] = cost_map[my, mx]
    return out


N_WAVES_MAX = 10 ** 6


def predicted_units(words, share, cells=None):
    """Units of a state-machine launch whose blocks' forecast words are `words`, MT_TUNE_QUAD_SHARE(_MOVING) = share
    and MT_TUNE_QUAD_KEEP at its default -- or None where the count depends on the number of resident waves.
    order_count_kernel cuts a block into quarters iff cost > share x sum / n_waves and cost > 0; the test does not know
    n_waves, so a count is given only where it is the same for every n_waves in [1, N_WAVES_MAX]:
      share = 1e-6: every positive cost above 2e-6 x sum (twice the largest threshold, n_waves = 1: float rounding has
                    room) -> 4 units per block of positive cost, 1 per block of cost 0;
      share = 1e6:  cost x N_WAVES_MAX <= 1e6 x sum always -> 1 unit per block.
    cells (bool, like words; MT_TUNE_SM_CELL_SHARE = 1e-6, camera at rest): the blocks that hold a zero-component ray go
    out as 16 cells where they are cut at all (their condition, 0.45 cost > 1e-6 x the quarters' threshold, is the weaker)."""
    c = cost_of(np.asarray(words).reshape(-1)).astype(object)
    total = sum(c)
    if share == 1e6:
        return len(c)
    if share != 1e-6:
        return None
    positive = [v for v in c if v > 0]
    if any(v * 1000000 <= 2 * total for v in positive):
        return None
    per = np.where(np.asarray(c, dtype=np.float64) > 0, 4, 1)
    if cells is not None:
        per = np.where((per == 4) & np.asarray(cells).reshape(-1), 16, per)
    return int(per.sum())


# ---------------------------------------------------------------------------------------------------------------------
# 4. the knobs at the ends of the ranges mt_scene_set_tuning accepts (mt_capi.hip, its switch)
UNIT_RANGE = ("POOL_PIECE_TIME1", "POOL_PIECE_TIME2", "POOL_PIECE_WORK1", "POOL_PIECE_WORK2", "POOL_CELL_FACTOR",
              "QUAD_SHARE", "QUAD_SHARE_MOVING", "QUAD_KEEP", "QUAD_WORK", "QUAD_WORK_MOVING", "HYBRID_POOL_SHARE",
              "HYBRID_QUAD_SHARE", "SM_CELL_SHARE", "SM_CELL_TIME", "SM_CELL_WORK", "HYBRID_CELL_FACTOR", "HYBRID_WORK1",
              "HYBRID_WORK2", "FORECAST_STEP", "HYBRID_STARTER_SHARE")   # [1e-6, 1e6]
SWITCHES = ("PACKED_STACK", "FORMS", "DEEP_LAYOUT", "MULTI_FORCE_PEER_COPY", "MULTI_BALANCE")
KNOB_ENDS = {k: (1e-6, 1e6) for k in UNIT_RANGE}
KNOB_ENDS.update({k: (0.0, 1.0) for k in SWITCHES})
KNOB_ENDS.update({
    # [0, 1e9], counts: 0 = automatic, 1 = the smallest that acts (the pool's capacity at its floor, one workgroup per
    # CU); the upper end only sizes an allocation (65 535 records per wave) and is left out
    "POOL_CAP": (0.0, 1.0), "BLOCKS_PER_CU": (0.0, 1.0),
    "POOL_BELOW": (0.0, 1e9),            # (the automatic engine's threshold: explicit engines do not read it)
    "POOL_SCRATCH_MB": (1.0,),           # the low end: engine 2 shrinks its pool or declines, engine 3 renders without one
    "BLEND": (0.0, 1.0),
    "FORECAST_RADIUS": (0.0, 8.0),
    "POOL_CUT_SHARE": (-1.0, 1e-6, 1e6),
    "ORDER_GROUPS": (1.0, 256.0),
    "XCD_QUEUES": (0.0, 1.0, 2.0),
    "LEAN_KERNEL": (0.0, 1.0, 2.0),
})


def header_knobs(header_text):
    """The names of enum mt_tune_knob in include/mythtracer_hip.h, in order, up to MT_TUNE_COUNT."""
    import re
    body = header_text[header_text.index("MT_TUNE_POOL_BELOW = 0"):]
    body = re.sub(r"/\*.*?\*/", "", body[:body.index("MT_TUNE_COUNT")], flags=re.S)
    return re.findall(r"MT_TUNE_([A-Z0-9_]+)", body)


# ---------------------------------------------------------------------------------------------------------------------
# 5. tile lists of the from_map launches: two halves of the 6 x 4 tiles, both through the axis camera's column and row
def half_lists(size=(W, H)):
    tx, ty = (size[0] + T - 1) // T, (size[1] + T - 1) // T
    tiles = np.arange(tx * ty)
    even = (tiles % tx + tiles // tx) % 2 == 0
    return [int(t) for t in tiles[even]], [int(t) for t in tiles[~even]]


def tile_rect(t, size=(W, H)):
    tx = (size[0] + T - 1) // T
    x, y = (t % tx) * T, (t // tx) * T
    return x, y, min(T, size[0] - x), min(T, size[1] - y)


def list_blocks(tiles, size=(W, H)):
    """bool[bh, bw]: the blocks of the image that belong to the list's tiles."""
    bw, bh = blocks_of(size)
    own = np.zeros((bh, bw), dtype=bool)
    for t in tiles:
        x, y, cw, ch = tile_rect(t, size)
        own[y // 8:(y + ch + 7) // 8, x // 8:(x + cw + 7) // 8] = True
    return own


# ---------------------------------------------------------------------------------------------------------------------
# 6. expectations: the oracle's frames, once per (camera, size); a chunk's or a tile list's share of them
def rgb_close(got, want):
    """The suite's rule for frames whose materials use pow (tests/test_gpu_parity.py, assert_rgb_close): 1 LSB on at
    most 0.01 % of the pixels, at least one.  -> (ok, differing pixels, max difference)"""
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    n_diff = int((d != 0).any(axis=-1).sum())
    mx = int(d.max(initial=0))
    return mx <= 1 and n_diff <= max(1, d.shape[0] * d.shape[1] // 10000), n_diff, mx


FRAME_CASES = [(cam, (W, H)) for cam in CAMERAS] + [("base", BIG)]
_oracle = {}


def oracle_scene():
    if "scene" not in _oracle:
        import orclib
        tris, mats = scene_description()
        o = orclib.OracleScene()
        fill(o, tris, mats)
        o.set_lights(LIGHTS)
        _oracle["scene"] = o
    return _oracle["scene"]


def oracle_frame(cam, size=(W, H), chunk=None):
    """The oracle's frame of camera `cam` (a name) or of one chunk of it: rgb and counters.  Computed once."""
    key = (cam, size, chunk)
    if key not in _oracle:
        _oracle[key] = oracle_scene().render(CAMERAS[cam], size[0], size[1], chunk=chunk, max_level=DEPTH)
    return _oracle[key]


def oracle_tiles(cam, tiles, size=(W, H)):
    """Ray counters of a tile list: the sum over its tiles (a pixel's rays do not depend on the launch it is in)."""
    total = dict.fromkeys(RAY_KEYS, 0)
    for t in tiles:
        c = oracle_frame(cam, size, tile_rect(t, size))["counters"]
        for k in RAY_KEYS:
            total[k] += c[k]
    return total
