"""tests/synthetic_inputs.py held to what it promises, and the numpy restatements that tests/test_gpu_synthetic.py holds
the kernels to held to plain Python arithmetic, without a GPU: the planted bitmaps flag the planted blocks and no other;
the planes of the relight test keep pow out of the way of every edge class; tiling.resolve_ss against exact fractions
on the ties pattern; tiling.order_tiles against sorted() over Python integers; tiling.deal_tiles deals every tile once.
"""
from fractions import Fraction

import numpy as np
import pytest

import gbuffer_ref
import lightbuffer_ref as lr
import synthetic_inputs as si
from mythtracer_amd import tiling


# ---- 1
def test_mask_geometries_are_the_block_counts_they_are_chosen_for():
    got = [si.mask_geometry(*g) for g in si.MASK_GEOMETRIES]
    assert [n for _, _, n, _ in got] == si.MASK_BLOCKS
    assert [per for _, _, _, per in got] == [1, 1, 2, 2, 4, 4, 32, 11]
    # 1089 blocks at per = 2: threads 545 .. 1023 own nothing, their i0 is clamped to n
    assert (1089 + 1) // 2 < si.COMPACT_THREADS


@pytest.mark.parametrize("W,H,chunk", si.MASK_GEOMETRIES)
def test_planted_bitmaps_flag_the_planted_blocks(W, H, chunk):
    chunk_, (x0, y0, mw, mh), n, per = si.mask_geometry(W, H, chunk)
    patterns = si.mask_patterns(n, per)
    frames = si.mask_frames(W, H, chunk)
    assert set(frames) == set(patterns) | {"random_bytes"}
    alone = si.isolated_blocks(W, H, chunk)
    assert alone.all() if chunk is None else alone.mean() > 0.95
    tiles_x = (W + 7) // 8
    for name, blocks in patterns.items():
        mask, tiles = tiling.refine_mask(frames[name], W, H, chunk_, 16)
        flagged = np.nonzero(mask.reshape(-1))[0]
        # every planted block is flagged, and a block that is flagged without being planted is the neighbour of one that
        # cannot be flagged alone
        assert np.isin(blocks, flagged).all(), name
        if alone[blocks].all():
            assert np.array_equal(flagged, blocks), name
        assert np.array_equal(tiles, ((y0 + flagged // mw) * tiles_x + x0 + flagged % mw)), name
    assert len(patterns["none"]) == 0 and len(patterns["all"]) == n
    assert abs(len(patterns["random_half"]) - n / 2) < n / 8
    assert len(patterns["every_per_th"]) == (n + per - 1) // per
    run = patterns["run_of_per_across_two_threads"]
    assert len(run) == per and (np.diff(run) == 1).all()
    assert per == 1 or run[0] // per != run[-1] // per  # (two threads' ranges)
    assert patterns["last_thread_first"][0] // per == (n - 1) // per == patterns["last"][0] // per
    assert tiling.refine_mask(frames["random_bytes"], W, H, chunk_, 16)[0].all()


# ---- 2
@pytest.fixture(scope="module")
def shade_rays():
    return {(image, chunk): gbuffer_ref.pixel_rays(si.SHADE_CAMERA, image[0], image[1], chunk) for image, chunk in si.SHADE_CHUNKS}


def restated(rays, n_lights, kind=None):
    gb, lb, classes, lights = si.shade_case(rays, n_lights, kind)
    info = {}
    with np.errstate(all="ignore"):
        rgb = lr.shade(None, gb, lb, lights, materials=si.MATERIALS, hit=gb["hit"], info=info)
    return gb, lb, classes, rgb, info["specular"]


@pytest.mark.parametrize("n_lights", si.SHADE_LIGHT_COUNTS)
def test_planes_keep_pow_out_of_the_way_of_every_edge_class(n_lights, shade_rays):
    """The two construction conditions of the relight test: at most half of the pixels take the specular branch, and
    every edge class has hit pixels that do not -- under the tame lights and under every hostile edit of them."""
    kinds = (None,) + si.HOSTILE_KINDS
    for (image, chunk), rays in shade_rays.items():
        if chunk[2] * chunk[3] < 255 or (chunk == si.SHADE_CHUNKS[-1][1] and image == si.SHADE_IMAGE):
            continue
        for kind in kinds if chunk == si.OFF_GRID else kinds[:1]:
            gb, lb, classes, rgb, spec = restated(rays, n_lights, kind)
            what = (chunk, n_lights, kind)
            assert 0 < spec.sum() <= spec.size // 2, what
            exact = gb["hit"] & ~spec
            for cls in si.EDGE_CLASSES:
                assert (classes[cls] & exact).sum() >= 1, what + (cls,)
                assert (classes[cls] & classes["miss"]).sum() >= 1, what + (cls,)
            d = rays[..., 3:]
            flip = (gb["normal"] * -d).sum(axis=-1) < 0
            assert (flip & exact).sum() > 10 and (~flip & exact).sum() > 10, what
            perp = classes["perpendicular"]
            assert (lr._dot(gb["normal"][perp], -d[perp]) == 0.0).all(), what
            # what the planes are for: a miss is black whatever they hold; a NaN in y or z alone is not a miss
            assert (rgb[classes["miss"]] == 0).all(), what
            assert not spec[classes["miss"]].any()
            grey = (classes["point_nan_y"] | classes["point_nan_z"]) & gb["hit"] & (gb["material"] < 0)
            assert (rgb[grey] > 0).all() or not grey.any()
            if kind is None:
                lit = exact & ~np.isnan(gb["point"]).any(axis=-1)
                assert (rgb[lit] == 255).mean() < 0.25 and (rgb[lit] > 0).mean() > 0.75, what  # (neither saturated nor black)
                print(what, "mean byte of the lit exact pixels %.1f" % rgb[lit].mean())


def test_the_chunk_offset_is_in_the_restated_ray(shade_rays):
    a = restated(shade_rays[si.SHADE_CHUNKS[-2]], 8)[3]
    b = restated(shade_rays[si.SHADE_CHUNKS[-1]], 8)[3]
    assert (a != b).any(axis=-1).mean() > 0.1


def test_shade_with_a_table_is_shade_with_the_oracle_scene(shade_rays):
    """lightbuffer_ref.shade's two forms agree where both are defined: the oracle's material table handed over as
    `materials`, prim >= 0 as `hit`."""
    class Orc:
        def materials(self):
            return [("m%d" % i, v, -1) for i, v in enumerate(si.MATERIALS)]
    rays = shade_rays[si.SHADE_CHUNKS[-2]]
    lights = si.tame_lights(3)
    gb, lb, _ = si.shade_planes(rays, lights)
    gb["material"] = np.where((gb["material"] >= si.N_MATERIALS) | (gb["material"] < 0), -1, gb["material"])
    with np.errstate(all="ignore"):
        a = lr.shade(None, gb, lb, lights, materials=si.MATERIALS, hit=gb["hit"])
        b = lr.shade(Orc(), dict(gb, prim=np.where(gb["hit"], 0, -1)), lb, lights)
    assert np.array_equal(a, b)


# ---- 3
def test_hostile_lights_keep_the_positions_and_change_what_they_say():
    base = np.array(lr.BENCH_LIGHTS)
    for kind in si.HOSTILE_KINDS:
        L = si.hostile_lights(base, kind, which=1, power_value=0.25)
        assert np.array_equal(L[:, :3], base[:, :3]) and L.shape == base.shape
        changed = ~((L == base) | (np.isnan(L) & np.isnan(base)))
        assert changed.any() and (kind == "all_zero" or changed[[0, 2]].sum() == 0)
    assert np.isnan(si.hostile_lights(base, "nan_channel")).sum() == 1
    assert np.isinf(si.hostile_lights(base, "inf_channel")).sum() == 1
    assert si.stored_power_value(np.array([np.nan, 1.0, 1.0, 0.0, 0.36, 0.36, 0.5])) == 0.36
    assert si.stored_power_value(np.array([np.nan, 1.0, 1.0, 0.0])) == 1.0


@pytest.mark.parametrize("name", ["cornell", "two_way"])
def test_restated_shades_are_the_oracle_frames_under_hostile_lights(name, scenes):
    """lightbuffer_ref.shade and raytree_ref.shade over planes and trees made under the tame lights against the oracle's
    own frames under the edited ones, byte for byte: NaN, inf and negative colours included."""
    import orclib
    import raytree_ref as rr
    W, H = 61, 37
    orc = orclib.OracleScene(rr.TWO_WAY if name == "two_way" else scenes[name])
    cam = rr.CAMERAS[name]
    base, which = si.relight_base(name, lr.BENCH_LIGHTS, lr.ONE_LIGHT["cornell"])
    gb = gbuffer_ref.oracle_gbuffer(orc, cam, W, H)
    lb = lr.ref_lightbuffer(orc, gb, base)
    deep = rr.build(orc, cam, W, H, base, 2)
    value = si.stored_power_value(lb["power"][which])
    assert (lb["power"][which] == value).any()
    for kind in si.HOSTILE_KINDS:
        new = si.hostile_lights(base, kind, which=which, power_value=value)
        orc.set_lights(new)
        i0, i2 = {}, {}
        with np.errstate(all="ignore"):
            d0 = lr.shade(orc, gb, lb, new, info=i0)
            t0 = rr.shade(orc, rr.truncated(deep, 0), new, W, H)
            t2 = rr.shade(orc, deep, new, W, H, info=i2)
        assert np.array_equal(d0, orc.render(cam, W, H, max_level=0)["rgb"]), kind
        assert np.array_equal(t0, d0), kind
        assert np.array_equal(t2, orc.render(cam, W, H, max_level=2)["rgb"]), kind
        assert not (i0["specular"] & ~i2["specular"]).any()  # (a tree's pixel takes the branch where its first ray does)
        assert 0 < i2["specular"].sum() < i2["specular"].size // 2, kind
        print(name, kind, "mean byte %.1f / %.1f, specular %d / %d of %d" % (d0.mean(), t2.mean(), i0["specular"].sum(), i2["specular"].sum(), W * H))


# ---- 4
@pytest.mark.parametrize("s", [2, 3, 4])
def test_resolve_ss_against_exact_fractions_on_the_ties(s):
    n = s * s
    a = si.tie_samples(6 * s, 5 * s, s, seed=s)
    got = tiling.resolve_ss(a, s)
    seen = set()
    for y in range(6):
        for x in range(5):
            for c in range(3):
                total = sum(int(a[s * y + j, s * x + i, c]) for j in range(s) for i in range(s))
                seen.add(total % n)
                mean = Fraction(total, n)
                want = int(mean) + (1 if mean - int(mean) >= Fraction(1, 2) else 0)  # the rounded mean, ties up
                assert got[y, x, c] == want == (total + n // 2) // n, (y, x, c)
    assert seen == set(si.tie_residues(n))
    assert s % 2 or set(si.tie_residues(n)) == {n // 2 - 1, n // 2}


@pytest.mark.parametrize("geometry", si.RESOLVE_GEOMETRIES)
def test_resolve_cases_cover_what_they_are_chosen_for(geometry):
    W, H, tw, th = geometry
    tx, ty = tiling.tile_grid(W, H, tw, th)
    if (tw, th) == (8, 8):
        assert tiling.tile_rect(tx - 1, W, H, tw, th)[2] == W % 8 != 0
    forms = si.resolve_forms(tx * ty)
    assert [f[2] is None for f in forms] == [True, True, False, False]
    assert (np.diff(forms[2][3]) < 0).all() and sorted(forms[2][3]) == list(range(tx * ty))
    for pattern in si.RESOLVE_PATTERNS:
        smp, want = si.resolve_case(pattern, geometry, 2, forms[1][3])
        assert smp.size == 4 * want.size == len(forms[1][3]) * 4 * tw * th * 3
        untouched = sum(tw * th * 3 - cw * ch * 3 for _, _, cw, ch in (tiling.tile_rect(int(t), W, H, tw, th) for t in forms[1][3]))
        assert (want == 0xA5).sum() >= untouched
        if pattern == "all_255":
            assert (want != 0xA5).sum() == want.size - untouched and set(np.unique(want)) <= {0xA5, 255}


# ---- 5
def python_order(cost_map, W, H, tw, th):
    """tile_cost_kernel + tile_order_kernel in Python integers: the sum of the map cells a tile's pixels touch, most
    expensive first, ties by tile number."""
    tx, ty = tiling.tile_grid(W, H, tw, th)
    cost = []
    for t in range(tx * ty):
        x0, y0 = (t % tx) * tw, (t // tx) * th
        x1, y1 = min(x0 + tw, W), min(y0 + th, H)
        cost.append(sum(int(cost_map[by][bx]) for by in range(y0 // 8, (y1 - 1) // 8 + 1) for bx in range(x0 // 8, (x1 - 1) // 8 + 1)))
    return sorted(range(tx * ty), key=lambda t: (-cost[t], t)), cost


@pytest.mark.parametrize("geometry", si.ORDER_GEOMETRIES)
def test_order_tiles_against_sorted(geometry):
    W, H, tw, th = geometry
    for kind in si.COST_MAPS:
        m = si.cost_map(kind, geometry)
        want, cost = python_order(m.tolist(), W, H, tw, th)
        assert tiling.order_tiles(m, W, H, tw, th).tolist() == want, kind
        if kind in ("equal", "zero") and W % tw == 0 and H % th == 0 and tw % 8 == 0 and th % 8 == 0:
            assert want == list(range(len(want)))  # (all ties: by tile number)
        if kind == "all_ones_u32" and (tw, th) == (64, 64):
            assert max(cost) >= 2 ** 32
        if kind == "differ_above_bit_32":
            assert m.any() or tw not in (16, 20, 64) or len(cost) < 9, geometry
        if kind == "differ_above_bit_32" and m.any():
            big = sorted(c for c in cost if c)
            assert big == [5, 2 ** 32 + 5, 2 ** 33 + 5]
            low = [t for t in range(len(cost)) if cost[t]]
            assert [cost[t] for t in low] == big and want[:3] == low[::-1]  # (32-bit sums would order them by number)
        if kind == "wider_poisoned":
            assert m.shape == ((H + 7) // 8 + 2, (W + 7) // 8 + 3) and max(cost) < si.POISON


def test_order_geometries_are_the_tile_counts_they_are_chosen_for():
    totals = [int(np.prod(tiling.tile_grid(*g))) for g in si.ORDER_GEOMETRIES]
    assert totals[:4] == [1, 255, 256, 257] and totals[-1] == 2025
    assert {g[2] for g in si.ORDER_GEOMETRIES} >= {5, 12, 16, 20, 64}


@pytest.mark.parametrize("total", [1, 20, 255, 256, 257])
def test_deal_tiles_deals_every_tile_once(total):
    order = np.random.default_rng(total).permutation(total).astype(np.int32)
    for world in si.deal_worlds(total):
        owned = []
        for rank in range(world):
            lst = tiling.deal_tiles(order, total, world, rank)
            assert len(lst) == tiling.dealt_tile_count(total, world, rank)
            owned += lst.tolist()
        assert sorted(owned) == list(range(total)), world
