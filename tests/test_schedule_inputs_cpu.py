"""tests/schedule_inputs.py held to its promises (no GPU): the bucket rule and what the patterns reach of it, the
n_waves-independence of every predicted unit count, the translated cameras' sensors, the knob table against the header's
enum, and the oracle's frame for every camera and size tests/test_gpu_schedules.py uses."""
import os
from fractions import Fraction

import numpy as np
import pytest

import schedule_inputs as si
from conftest import ROOT
from mythtracer_amd import binding

BW, BH = si.blocks_of()


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    return native_libs


def bucket_by_definition(c):
    """cost_bucket of mt_render.hip, one value at a time."""
    if c == 0:
        return 255
    e = c.bit_length() - 1
    f = (c >> (e - 3)) & 7 if e >= 3 else 0
    return 255 - (e * 8 + f)


def test_bucket_rule():
    vals = [0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 1000, 0x7fffffff, 0x80000000, 0xefffffff, 0xf0000000, 0xffffffff]
    vals += si.bucket_edges() + [v - 1 for v in si.bucket_edges()]
    got = si.cost_bucket(np.array(vals, dtype=np.uint64))
    assert [int(g) for g in got] == [bucket_by_definition(v) for v in vals]
    assert got.min() == 0 and got.max() == 255
    # descending cost = ascending bucket, and an edge starts a bucket
    order = np.argsort(np.array(vals, dtype=np.uint64), kind="stable")
    assert (np.diff(got[order]) <= 0).all()
    for e in si.bucket_edges():
        assert bucket_by_definition(e) == bucket_by_definition(e - 1) - (1 if e > 8 else 8)  # (below 8: whole octaves)


def test_patterns_and_what_they_reach():
    maps = si.cost_maps(BW, BH)
    assert set(maps) == set(si.PATTERNS) and len(maps) >= 20
    for name, m in maps.items():
        assert m.dtype == np.uint32 and m.shape == (BH, BW), name
        assert np.array_equal(m, si.cost_maps(BW, BH)[name]), name  # fixed seeds
    for name, word in (("all_0", 0), ("all_1", 1), ("all_7fffffff", 0x7fffffff), ("all_80000000", 0x80000000), ("all_ffffffff", 0xffffffff)):
        assert (maps[name] == word).all()
    for name, at in (("hot_first", 0), ("hot_last", BW * BH - 1), ("hot_middle", (BH // 2) * BW + BW // 2)):
        flat = maps[name].reshape(-1)
        assert flat[at] == 0x7fffffff and (np.delete(flat, at) == 1).all()
    assert set(np.unique(maps["checker_bit31_1000"])) == {1000, 0x80000000}
    assert set(np.unique(maps["checker_0_1000"])) == {0, 1000}
    assert set(np.unique(maps["checker_1_2p30"])) == {1, 1 << 30}
    assert (np.diff(maps["ramp_up"].reshape(-1).astype(np.int64)) == 1).all()
    assert (np.diff(maps["ramp_down"].reshape(-1).astype(np.int64)) == -1).all()
    assert set(int(v) for v in maps["octaves"].reshape(-1)) == {1 << k for k in range(31)}
    # cost in one place: one block column / row / block
    for name, n_hot in (("left_column", BH), ("one_row", BW), ("corner", 1)):
        assert int((maps[name] != 0x80000000).sum()) == n_hot
    assert (maps["left_column"][:, 0] == 100000).all() and (maps["one_row"][BH // 2] == 100000).all()
    assert maps["corner"][-1, -1] == 100000
    assert not np.array_equal(maps["random_1"], maps["random_2"])
    assert maps["random_1"].max() >= 0x80000000 and maps["random_1"].min() < 0x08000000

    # ---- buckets.  Bucket 255: cost 0 (bit 31 alone).  Bucket 0 needs a unit of 0xf0000000 or more; a cost has 31
    # bits, so it is reached where a piece's time factor is above 2 (MT_TUNE_SM_CELL_TIME / POOL_PIECE_TIME* towards
    # their upper end, the conversion saturating): the knob-limit cases run the random map under exactly those.
    assert (si.unit_buckets(maps["all_80000000"]) == 255).all()
    assert si.unit_buckets(maps["checker_bit31_1000"]).max() == 255
    assert (si.unit_buckets(maps["all_7fffffff"], 1e6) == 0).all()
    assert si.unit_buckets(maps["random_1"], 1e6).min() == 0 and si.unit_buckets(maps["octaves"], 1e-6).max() == 255
    assert si.unit_buckets(maps["all_ffffffff"]).max() == 8  # (whole blocks: the longest unit a map can ask for)
    # one bucket for every block
    for name in ("all_0", "all_1", "all_7fffffff", "all_80000000", "all_ffffffff"):
        assert len(np.unique(si.unit_buckets(maps[name]))) == 1, name
    # many buckets: 96 blocks hold 48 edges and the 48 values below them; the 576 blocks of the big frame every one
    assert len(np.unique(si.unit_buckets(maps["bucket_edges"]))) >= 90
    big = si.cost_maps(*si.blocks_of(si.BIG))
    assert len(np.unique(si.unit_buckets(big["bucket_edges"]))) >= 200
    assert len(np.unique(si.unit_buckets(big["random_1"]))) >= 30
    # the octaves under the quarters' time factor straddle bucket boundaries differently
    assert len(np.unique(si.unit_buckets(maps["octaves"]))) == 31


def quarters_by_definition(c, total, n_waves, share):
    """order_count_kernel's condition in exact arithmetic."""
    return c > 0 and Fraction(c) > Fraction(total, n_waves) * Fraction(share)


@pytest.mark.parametrize("size,chunk", [((si.W, si.H), None), ((si.W, si.H), si.RAGGED_CHUNK), (si.BIG, None)])
def test_predicted_unit_counts_do_not_depend_on_n_waves(size, chunk):
    mw, mh = si.blocks_of(size)
    maps = si.cost_maps(mw, mh)
    predictable = []
    for name, m in maps.items():
        words = si.planted_words(m, size, chunk)
        assert words.shape == si.blocks_of(size, chunk)[::-1]
        if chunk is None:
            assert np.array_equal(words, m), name
        costs = [int(v) for v in si.cost_of(words.reshape(-1))]
        total = sum(costs)
        n = len(costs)
        assert si.predicted_units(words, 1e6) == n
        for nw in (1, 2, 1000, si.N_WAVES_MAX):
            assert not any(quarters_by_definition(c, total, nw, Fraction(10 ** 6)) for c in costs), (name, nw)
        assert si.predicted_units(words, 0.95) is None
        low = si.predicted_units(words, 1e-6)
        if low is None:
            continue
        predictable.append(name)
        for nw in (1, 2, 1000, si.N_WAVES_MAX):
            units = sum(4 if quarters_by_definition(c, total, nw, Fraction(1, 10 ** 6)) else 1 for c in costs)
            assert units == low, (name, nw)
            # ... with room for the float arithmetic of the kernel: a factor of two at the nearest threshold
            assert all(c == 0 or Fraction(c) > 2 * Fraction(total, nw) * Fraction(1, 10 ** 6) for c in costs)
    print(size, chunk, "predictable:", predictable)
    assert len(predictable) >= 8
    assert "checker_bit31_1000" in predictable and "checker_0_1000" in predictable
    if chunk is None and size == (si.W, si.H):
        want = {"all_0": 384, "all_1": 384, "all_7fffffff": 384, "all_80000000": 96, "all_ffffffff": 384,
                "checker_bit31_1000": 48 * 4 + 48, "checker_0_1000": 384, "ramp_up": 384, "ramp_down": 384,
                "left_column": 8 * 4 + 88, "one_row": 12 * 4 + 84, "corner": 4 + 95}
        for name, units in want.items():
            assert si.predicted_units(maps[name], 1e-6) == units, name
        for name in ("hot_first", "hot_last", "hot_middle", "checker_1_2p30", "octaves"):
            assert si.predicted_units(maps[name], 1e-6) is None, name  # a cost of 1 beside 2^30: quarters or not by n_waves


def test_a_map_smaller_than_the_image():
    small = si.cost_maps(5, 3)["random_1"]
    words = si.planted_words(small)
    assert np.array_equal(words[:3, :5], small) and (words[3:] == 0).all() and (words[:, 5:] == 0).all()
    assert si.predicted_units(np.zeros((BH, BW), dtype=np.uint32), 1e-6) == 4 * BW * BH  # unseen everywhere


def test_translated_cameras_keep_the_sensor_directions():
    base = binding.sensor(si.CAMERAS["base"], si.W, si.H)
    for name in ("translated", "translated2", "far"):
        s = binding.sensor(si.CAMERAS[name], si.W, si.H)
        assert s[3:12].tobytes() == base[3:12].tobytes(), name   # start_point, delta_scanline, delta_pixel: bit-identical
        assert not np.array_equal(s[0:3], base[0:3]), name       # origin
    for name in ("yaw2", "yaw180", "roll90"):
        s = binding.sensor(si.CAMERAS[name], si.W, si.H)
        assert s[3:12].tobytes() != base[3:12].tobytes() and np.array_equal(s[0:3], base[0:3]), name
    # the re-projection of a translated camera is the identity: block centres land in their own block
    big = binding.sensor(si.CAMERAS["base"], *si.BIG)
    assert binding.sensor(si.CAMERAS["translated"], *si.BIG)[3:12].tobytes() == big[3:12].tobytes()


def test_zero_component_rays():
    """The base cameras have none (a re-projected forecast skips old blocks that have); the axis camera has one pixel
    column and one row, through both half-lists of the from_map launches."""
    for name in ("base", "translated", "translated2", "yaw2", "yaw180", "roll90", "far"):
        assert not si.zero_component_pixels(binding.sensor(si.CAMERAS[name], si.W, si.H), si.W, si.H).any(), name
    assert not si.zero_component_pixels(binding.sensor(si.CAMERAS["base"], *si.BIG), *si.BIG).any()
    z = si.zero_component_pixels(binding.sensor(si.CAMERAS["axis"], si.W, si.H), si.W, si.H)
    assert z[:, si.W // 2].all() and z[si.H // 2].all() and int(z.sum()) == si.W + si.H - 1
    zb = si.zero_component_blocks(binding.sensor(si.CAMERAS["axis"], si.W, si.H), si.W, si.H)
    assert int(zb.sum()) == BW + BH - 1
    a, b = si.half_lists()
    assert sorted(a + b) == list(range(24)) and len(a) == len(b) == 12
    for lst in (a, b):
        own = si.list_blocks(lst)
        assert int(own.sum()) == 48 and int((own & zb).sum()) >= 8
    assert not (si.list_blocks(a) & si.list_blocks(b)).any()


def test_knob_table_covers_the_header():
    names = si.header_knobs(open(os.path.join(ROOT, "include", "mythtracer_hip.h")).read())
    assert len(names) == len(binding.TUNE) and set(names) == set(binding.TUNE)
    assert [binding.TUNE[n] for n in names] == list(range(len(names)))  # the binding's numbers are the enum's
    assert set(si.KNOB_ENDS) == set(names)
    for k, ends in si.KNOB_ENDS.items():
        assert len(ends) >= 1 and len(set(ends)) == len(ends), k
    # the ranges of mt_scene_set_tuning's switch, as the table states them
    src = open(os.path.join(ROOT, "mythtracer_amd", "csrc", "mt_capi.hip")).read()
    sw = src[src.index("int mt_scene_set_tuning("):]
    sw = sw[:sw.index("s->tune.v[knob] = value;")]
    unit = sw[:sw.index("value >= 1e-6 && value <= 1e6")]
    assert set(si.header_knobs("MT_TUNE_POOL_BELOW = 0" + unit[unit.index("switch"):] + "MT_TUNE_COUNT")) - {"POOL_BELOW"} == set(si.UNIT_RANGE)
    for text in ("value >= 0.0 && value <= 1e9", "value >= 1.0 && value <= 1e9", "value >= 0.0 && value <= 1.0", "value <= 8.0",
                 "value < 0.0 || (value >= 1e-6 && value <= 1e6)", "value >= 1.0 && value <= (double)kOrdGroupsMax",
                 "value == 0.0 || value == 1.0 || value == 2.0"):
        assert text in sw, text
    assert "kOrdGroupsMax = 256" in open(os.path.join(ROOT, "mythtracer_amd", "csrc", "mt_order.h")).read()


def test_oracle_frames_exist_before_a_gpu_is_touched():
    """Every camera and size of the GPU file, once; what the cases need of them."""
    frames = {}
    for cam, size in si.FRAME_CASES:
        f = si.oracle_frame(cam, size)
        assert f["rgb"].shape == (size[1], size[0], 3)
        assert si.oracle_frame(cam, size) is f  # computed once
        frames[(cam, size)] = f
    small = (si.W, si.H)
    for cam in ("base", "translated", "translated2", "axis", "yaw2", "roll90"):
        c = frames[(cam, small)]["counters"]
        assert c["rays_primary"] == si.W * si.H and c["rays_secondary"] > 0 and c["rays_shadow"] > 0, cam
    assert frames[("base", si.BIG)]["counters"]["rays_secondary"] > 0
    # a translated camera renders another picture (a frame taken for the base camera's would be noticed)
    assert not np.array_equal(frames[("base", small)]["rgb"], frames[("translated", small)]["rgb"])
    assert not np.array_equal(frames[("translated", small)]["rgb"], frames[("translated2", small)]["rgb"])
    # chunks and tile lists: their pixels are the frame's, their ray counts add up to it
    for chunk in [si.RAGGED_CHUNK] + si.DEGENERATE_CHUNKS:
        part = si.oracle_frame("base", small, chunk)
        x, y, cw, ch = chunk
        assert np.array_equal(part["rgb"], frames[("base", small)]["rgb"][y:y + ch, x:x + cw])
    a, b = si.half_lists()
    ca, cb = si.oracle_tiles("axis", a), si.oracle_tiles("axis", b)
    for k in si.RAY_KEYS:
        assert ca[k] + cb[k] == frames[("axis", small)]["counters"][k], k
    ok, n_diff, mx = si.rgb_close(frames[("base", small)]["rgb"], frames[("base", small)]["rgb"])
    assert ok and n_diff == 0 and mx == 0
    assert not si.rgb_close(frames[("base", small)]["rgb"], frames[("translated", small)]["rgb"])[0]
