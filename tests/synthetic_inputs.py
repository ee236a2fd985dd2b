"""Inputs no scene produces, for the kernels that trace nothing: bitmaps for refine_mask_kernel / refine_compact_kernel,
planes for shade_direct_kernel, light colours for both relight kernels, sample slots for resolve_kernel, cost maps for
tile_cost_kernel / tile_order_kernel / deal_tiles_kernel.  Fixed seeds, numpy only, no GPU: tests/test_synthetic_cpu.py
holds the generators to what they promise, tests/test_gpu_synthetic.py feeds them to the kernels.  Test infrastructure.
"""
from __future__ import annotations

import numpy as np

from mythtracer_amd import tiling

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31

# ---------------------------------------------------------------------------------------------------------------------
# 1. block masks past refine_compact_kernel's 1024 threads (csrc/mt_adaptive.h: thread t owns `per` flags)
COMPACT_THREADS = 1024
# (image_w, image_h, chunk or None): 1023 / 1024 / 1025 blocks; 1089 (per 2, the upper threads empty); 4095; 4096 (per 4,
# every thread full); 32 400 (per 32); a chunk of the 1080p image (11 214 blocks: mask_x0, mask_y0 and tiles_x matter)
MASK_GEOMETRIES = [(8184, 8, None), (8192, 8, None), (8200, 8, None), (264, 264, None), (520, 504, None),
                   (512, 512, None), (1920, 1080, None), (1920, 1080, (3, 5, 1000, 700))]
MASK_BLOCKS = [1023, 1024, 1025, 1089, 4095, 4096, 32400, 11214]
FLAT, DEVIATING = 100, 200  # a flat frame's byte and the planted pixel's: 100 apart, far above threshold 16


def mask_geometry(W, H, chunk):
    """(chunk, (mask_x0, mask_y0, mask_w, mask_h), n_blocks, per)"""
    chunk = chunk or (0, 0, W, H)
    x0, y0, mw, mh = tiling.chunk_blocks(chunk)
    n = mw * mh
    return chunk, (x0, y0, mw, mh), n, (n + COMPACT_THREADS - 1) // COMPACT_THREADS


def mask_patterns(n, per, seed=1):
    """name -> the chunk-local numbers of the blocks to flag (sorted int64), for n blocks of which a thread owns per."""
    rng = np.random.default_rng(seed)
    last_thread = (n - 1) // per  # the last thread that owns a block
    t = max(0, min(COMPACT_THREADS // 2, last_thread - 2))  # a thread in the middle with a full successor
    run0 = t * per + (per + 1) // 2
    out = {
        "none": [],
        "all": range(n),
        "first": [0],
        "last": [n - 1],
        # the last non-empty thread: its last block is block n - 1, its first one and its predecessor's last one are
        # the two sides of the boundary below it
        "last_thread_first": [last_thread * per],
        "last_full_thread_last": [last_thread * per - 1] if last_thread > 0 else [n - 1],
        "every_per_th": range(0, n, per),
        "every_per_th_last": range(per - 1, n, per),
        "run_of_per_across_two_threads": range(run0, min(run0 + per, n)),
        "random_half": np.nonzero(rng.random(n) < 0.5)[0],
    }
    return {k: np.array(sorted(v), dtype=np.int64) for k, v in out.items()}


def planted_pixel(b, W, H, chunk):
    """The chunk-local (x, y) of the pixel that flags chunk-local block b: (8 bx + 3, 8 by + 3) of the image where the
    chunk holds it, else the chunk's pixel of that block nearest to it."""
    chunk, (x0, y0, mw, mh), _, _ = mask_geometry(W, H, chunk)
    cx, cy, cw, ch = chunk
    b = np.asarray(b, dtype=np.int64)
    bx, by = x0 + b % mw, y0 + b // mw
    px = np.clip(8 * bx + 3, np.maximum(cx, 8 * bx), np.minimum(cx + cw - 1, 8 * bx + 7))
    py = np.clip(8 * by + 3, np.maximum(cy, 8 * by), np.minimum(cy + ch - 1, 8 * by + 7))
    return px - cx, py - cy


def planted_frame(blocks, W, H, chunk):
    """A flat chunk bitmap with one deviating pixel per listed block."""
    _, _, cw, ch = chunk or (0, 0, W, H)
    f = np.full((ch, cw, 3), FLAT, dtype=np.uint8)
    if len(blocks):
        x, y = planted_pixel(blocks, W, H, chunk)
        f[y, x, 0] = DEVIATING
    return f


def isolated_blocks(W, H, chunk):
    """Which chunk-local blocks can be flagged alone: the planted pixel's neighbours inside the chunk lie in its block
    (every block of a whole image at least 8 high and wide; not a block of which the chunk holds one row or column)."""
    chunk, (x0, y0, mw, mh), n, _ = mask_geometry(W, H, chunk)
    cx, cy, cw, ch = chunk
    b = np.arange(n)
    x, y = planted_pixel(b, W, H, chunk)
    ok = np.ones(n, dtype=bool)
    for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        nx, ny = x + dx, y + dy
        inside = (nx >= 0) & (nx < cw) & (ny >= 0) & (ny < ch)
        same = ((nx + cx) // 8 == (x + cx) // 8) & ((ny + cy) // 8 == (y + cy) // 8)
        ok &= ~inside | same
    return ok


def mask_frames(W, H, chunk, seed=1):
    """name -> the chunk's bitmap: the planted patterns and random bytes."""
    _, _, n, per = mask_geometry(W, H, chunk)
    frames = {k: planted_frame(v, W, H, chunk) for k, v in mask_patterns(n, per, seed).items()}
    _, _, cw, ch = chunk or (0, 0, W, H)
    frames["random_bytes"] = np.random.default_rng(seed + 1).integers(0, 256, (ch, cw, 3), dtype=np.uint8)
    return frames


# ---------------------------------------------------------------------------------------------------------------------
# 2. planes for shade_direct_kernel (csrc/mt_lightbuffer.h)
# the material table: ka kd ks ns refl tr tf ni (mythtracer_amd/binding.py, scene_create)
def _mat(ka, kd, ks, ns):
    return np.array(list(ka) + list(kd) + list(ks) + [ns, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0], dtype=np.float64)


MATERIALS = np.stack([
    _mat((0.5, 0.5, 0.5), (0.6, 0.5, 0.4), (0.5, 0.4, 0.3), 0.0),     # pow(x, 0) = 1
    _mat((0.5, 0.5, 0.5), (0.3, 0.6, 0.5), (0.3, 0.5, 0.4), 1.0),     # pow(x, 1) = x
    _mat((0.5, 0.5, 0.5), (0.5, 0.3, 0.6), (0.4, 0.3, 0.5), 0.5),
    _mat((0.5, 0.5, 0.5), (0.4, 0.4, 0.4), (0.9, 0.8, 0.7), 200.0),
    _mat((0.5, 0.5, 0.5), (0.2, 0.5, 0.3), (1.0, 1.0, 1.0), 1000.0),
    _mat((0.5, 0.5, 0.5), (0.5, 0.5, 0.5), (0.0, 0.0, 0.0), 10.0),    # zero specular
    _mat((0.5, 0.5, 0.5), (1.5, 2.0, 1.25), (0.2, 0.2, 0.2), 10.0),   # diffuse above 1
    _mat((0.5, 0.5, 0.5), (0.0, 0.0, 0.0), (0.3, 0.3, 0.3), 10.0),    # zero diffuse
])
N_MATERIALS = len(MATERIALS)

SHADE_IMAGE = (96, 54)
SHADE_CAMERA = (50.0, 50.0, -120.0, 0.0, 0.0, 0.0, 100.0)
OFF_GRID = (5, 3, 61, 37)
# (image, chunk): one pixel; one row around the 256-thread launch boundary; the off-grid chunk and the same planes at
# the image's origin
SHADE_CHUNKS = [((1, 1), (0, 0, 1, 1)), ((255, 1), (0, 0, 255, 1)), ((256, 1), (0, 0, 256, 1)), ((257, 1), (0, 0, 257, 1)),
                (SHADE_IMAGE, OFF_GRID), (SHADE_IMAGE, (0, 0, 61, 37))]
SHADE_LIGHT_COUNTS = (1, 8, 9)  # kShadeArgLights = 8: nine lights are read from device memory
# the edge classes of the planes; every one of them (and both sides of the normal flip, which the generator leaves to
# chance) must have hit pixels that do not take the specular branch
EDGE_CLASSES = ("perpendicular", "point_nan_y", "point_nan_z", "point_at_light",
                "material_minus_1", "material_n", "material_int_max", "material_int_min",
                "power_zero", "power_around_ambient", "power_negative", "power_nan", "power_inf",
                "in_shadow_0", "in_shadow_1", "in_shadow_255", "in_shadow_2",
                "albedo_zero", "albedo_above_1", "albedo_negative")


def tame_lights(n, seed=7):
    """n lights at random places; colours positive, the sum over the lights around 1."""
    rng = np.random.default_rng(seed)
    L = np.zeros((n, 12))
    L[:, 0:3] = rng.uniform(-100.0, 200.0, (n, 3))
    L[:, 3:6] = rng.uniform(0.3, 0.9, (n, 3)) / n
    L[:, 6:9] = rng.uniform(1.0, 2.0, (n, 3)) / n
    L[:, 9:12] = rng.uniform(0.5, 1.0, (n, 3)) / n
    return L


def shade_planes(rays, lights, seed=11):
    """Planes for a chunk whose pixel rays are `rays` (ch, cw, 6) under `lights` (n, 12): (gb, lb, classes).
    gb: rays, point, normal, albedo (ch, cw, 3), material (ch, cw) int32, hit (ch, cw) = point[0] is not NaN;
    lb: power (n, ch, cw, 3), in_shadow (n, ch, cw) uint8; classes: name -> (ch, cw) bool for EDGE_CLASSES and "miss".
    A pixel is random first -- a unit normal on either side of the ray, a valid material, power in [0, 1], in_shadow 0 or
    1 --; then every third pixel is dealt one edge class in turn, and of a class's pixels in turn one is left as it is,
    one gets in_shadow 1 for every light (so that it cannot take the specular branch: pow is then not in its way) and
    one becomes a miss on top (NaN in point[0]: black whatever the other planes hold)."""
    ch, cw = rays.shape[:2]
    n, n_l = ch * cw, len(lights)
    L = np.asarray(lights, dtype=np.float64).reshape(n_l, 12)
    rng = np.random.default_rng(seed)
    d = rays[..., 3:].reshape(n, 3)
    point = rng.uniform(-50.0, 150.0, (n, 3))
    normal = rng.normal(size=(n, 3))
    normal /= np.sqrt((normal * normal).sum(axis=1))[:, None]
    albedo = rng.uniform(0.0, 1.0, (n, 3))
    material = rng.integers(0, N_MATERIALS, n).astype(np.int32)
    power = rng.uniform(0.0, 1.0, (n_l, n, 3))
    in_shadow = rng.integers(0, 2, (n_l, n)).astype(np.uint8)
    classes = {name: np.zeros(n, dtype=bool) for name in EDGE_CLASSES + ("miss",)}
    dealt = np.arange(0, n, 3) if n >= 3 * 3 * len(EDGE_CLASSES) else np.arange(n)
    for k, i in enumerate(dealt):
        name = EDGE_CLASSES[k % len(EDGE_CLASSES)]
        variant = (k // len(EDGE_CLASSES)) % 3
        li = (k // (3 * len(EDGE_CLASSES))) % n_l
        classes[name][i] = True
        if variant >= 1 and not name.startswith("in_shadow"):
            in_shadow[:, i] = 1
        if name == "perpendicular":
            # not a unit vector, but dot(normal, -direction) = -(dy dx) + dx dy is +0.0 exactly: no flip, and the
            # reflected ray is the ray itself, refl_dot = -|d|^2 < 0
            normal[i] = (d[i, 1], -d[i, 0], 0.0)
        elif name == "point_nan_y":
            point[i, 1] = np.nan
        elif name == "point_nan_z":
            point[i, 2] = np.nan
        elif name == "point_at_light":
            point[i] = L[li, 0:3]
        elif name.startswith("material"):
            material[i] = {"minus_1": -1, "n": N_MATERIALS, "int_max": INT32_MAX, "int_min": INT32_MIN}[name[9:]]
        elif name == "power_zero":
            power[:, i] = 0.0
        elif name == "power_around_ambient":  # below in x, equal in y, above in z: of every light's own ambient
            power[:, i] = L[:, 3:6] + np.array([-0.01, 0.0, 0.01])
        elif name == "power_negative":
            power[:, i] = -power[:, i] - 0.25
        elif name == "power_nan":
            power[li, i, k % 3] = np.nan
        elif name == "power_inf":
            power[li, i, k % 3] = np.inf
        elif name.startswith("in_shadow"):
            in_shadow[:, i] = int(name[10:])
            if variant >= 1:  # (in_shadow is the class: the normal keeps the pixel off the specular branch instead)
                normal[i] = (d[i, 1], -d[i, 0], 0.0) / np.sqrt(d[i, 0] * d[i, 0] + d[i, 1] * d[i, 1])
        elif name == "albedo_zero":
            albedo[i] = 0.0
        elif name == "albedo_above_1":
            albedo[i] += 1.0
        elif name == "albedo_negative":
            albedo[i] = -albedo[i] - 0.1
        if variant == 2:
            point[i, 0] = np.nan
            classes["miss"][i] = True
    # misses among the ordinary pixels too
    plain = np.setdiff1d(np.arange(n), dealt)
    extra = plain[::11]
    point[extra, 0] = np.nan
    classes["miss"][extra] = True
    gb = dict(rays=rays, point=point.reshape(ch, cw, 3), normal=normal.reshape(ch, cw, 3), albedo=albedo.reshape(ch, cw, 3),
              material=material.reshape(ch, cw), hit=~np.isnan(point[:, 0]).reshape(ch, cw))
    lb = dict(power=power.reshape(n_l, ch, cw, 3), in_shadow=in_shadow.reshape(n_l, ch, cw))
    return gb, lb, {k: v.reshape(ch, cw) for k, v in classes.items()}


# ---------------------------------------------------------------------------------------------------------------------
# 3. light colours no scene file holds; positions untouched
HOSTILE_KINDS = ("all_zero", "ambient_above_1", "negative_diffuse", "specular_1e6", "nan_channel", "inf_channel",
                 "ambient_equals_power")


def relight_base(name, bench, one):
    """The lights a scene's planes and trees are made under, and the light whose colours the edits change: the cornell
    box under its one light inside the box (the bench's three stand outside it), every other scene under the bench's,
    the middle one edited."""
    lights = one if name == "cornell" else bench
    return lights, len(lights) // 2


def stored_power_value(power):
    """A value the power plane holds for the ambient_equals_power edit: a finite one strictly inside (0, 1) where a
    transparent occluder left one, else the most frequent finite value."""
    v = np.asarray(power).reshape(-1)
    v = v[np.isfinite(v)]
    inside = v[(v > 0.0) & (v < 1.0)]
    values, counts = np.unique(inside if len(inside) else v, return_counts=True)
    return float(values[np.argmax(counts)])


def hostile_lights(lights, kind, which=None, power_value=1.0):
    """The light set with the colours of light `which` (default: the last one) edited -- all_zero: of every light."""
    L = np.array(lights, dtype=np.float64).reshape(-1, 12).copy()
    i = len(L) - 1 if which is None else which
    if kind == "all_zero":
        L[:, 3:] = 0.0
    elif kind == "ambient_above_1":
        L[i, 3:6] = (1.5, 1.25, 2.0)
    elif kind == "negative_diffuse":
        L[i, 6:9] = (-0.5, -1.0, -0.25)
    elif kind == "specular_1e6":
        L[i, 9:12] = 1e6
    elif kind == "nan_channel":
        L[i, 7] = np.nan
    elif kind == "inf_channel":
        L[i, 6] = np.inf
    elif kind == "ambient_equals_power":
        L[i, 3:6] = power_value
    else:
        raise ValueError(kind)
    return L


def shade_case(rays, n_lights, kind=None):
    """The planes of a chunk made under the tame lights, and the lights to relight them with -- the tame ones, or those
    with the last light's colours edited (ambient_equals_power: to a value its power plane holds): (gb, lb, classes,
    lights)."""
    tame = tame_lights(n_lights)
    gb, lb, classes = shade_planes(rays, tame)
    if kind is None:
        return gb, lb, classes, tame
    return gb, lb, classes, hostile_lights(tame, kind, power_value=stored_power_value(lb["power"][-1]))


# ---------------------------------------------------------------------------------------------------------------------
# 4. sample slots for resolve_kernel<S> (csrc/mt_resolve.h)
# (image_w, image_h, tile_w, tile_h): 8 x 8 tiles whose edge tiles are 1 .. 7 pixels wide (a head only, a head and a
# tail, rows shorter than the head; 11 and 13 rows: the rows of a slot start at every alignment); 5 x 3; 32 x 32
RESOLVE_GEOMETRIES = [(17 + k, 11 + 2 * (k & 1), 8, 8) for k in range(7)] + [(23, 10, 5, 3), (101, 67, 32, 32)]
RESOLVE_PATTERNS = ("random", "zeros", "all_255", "ties", "column_255", "byte_column_255")


def tie_residues(n):
    """The sums mod n on both sides of the rounding of (sum + n // 2) // n: n // 2 - 1 and n // 2 (even n: down, up),
    and for odd n also (n + 1) // 2, the first residue that rounds up."""
    return sorted({n // 2 - 1, n // 2, (n + 1) // 2})


def tie_samples(sh, sw, s, seed):
    """uint8 [sh][sw][3], sh and sw multiples of s, every s x s block's channel sum = n q + r, r in tie_residues(n)."""
    rng = np.random.default_rng(seed)
    n = s * s
    h, w = sh // s, sw // s
    res = np.array(tie_residues(n))
    q = rng.integers(0, 255, (h, w, 3))
    total = n * q + res[rng.integers(0, len(res), (h, w, 3))]
    # spread the sum over the n samples: equal shares, the remainder one each, then shifts between neighbours
    v = np.repeat((total // n)[..., None], n, axis=-1) + (np.arange(n) < (total % n)[..., None])
    for k in range(n - 1):
        room = np.minimum(v[..., k], 255 - v[..., k + 1])
        move = (rng.random(room.shape) * (room + 1)).astype(np.int64)
        v[..., k] -= move
        v[..., k + 1] += move
    v = rng.permuted(v, axis=-1)
    assert v.min() >= 0 and v.max() <= 255 and np.array_equal(v.sum(axis=-1), total)
    # v[y][x][c][j s + i] -> sample (s y + j, s x + i, c)
    return v.reshape(h, w, 3, s, s).transpose(0, 3, 1, 4, 2).reshape(sh, sw, 3).astype(np.uint8)


def resolve_samples(pattern, sh, sw, s, seed):
    """The sample bitmap uint8 [sh][sw][3] of one tile."""
    rng = np.random.default_rng(seed)
    if pattern == "random":
        return rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    if pattern == "zeros":
        return np.zeros((sh, sw, 3), dtype=np.uint8)
    if pattern == "all_255":
        return np.full((sh, sw, 3), 255, dtype=np.uint8)
    if pattern == "ties":
        return tie_samples(sh, sw, s, seed)
    a = np.zeros((sh, sw * 3), dtype=np.uint8)
    if pattern == "column_255":  # one sample column of every pixel, all channels
        a = a.reshape(sh, sw, 3)
        a[:, seed % s::s] = 255
        return a
    if pattern == "byte_column_255":  # every fourth byte of a sample row: one 16-bit field full, its neighbours empty
        a[:, seed % 4::4] = 255
        return a.reshape(sh, sw, 3)
    raise ValueError(pattern)


def resolve_case(pattern, geometry, s, tiles, seed=5):
    """Sample slots for the listed tiles of the OUTPUT image, slot j = tile tiles[j]: (samples uint8 flat, want uint8
    flat with 0xA5 in every byte the resolve must not touch)."""
    W, H, tw, th = geometry
    smp = np.zeros(len(tiles) * tiling.slot_bytes(s * tw, s * th), dtype=np.uint8)
    want = np.full(len(tiles) * tiling.slot_bytes(tw, th), 0xA5, dtype=np.uint8)
    for j, t in enumerate(tiles):
        _, _, cw, ch = tiling.tile_rect(int(t), W, H, tw, th)
        a = resolve_samples(pattern, s * ch, s * cw, s, seed + 31 * int(t))
        smp[j * tiling.slot_bytes(s * tw, s * th):][:a.size] = a.reshape(-1)
        want[j * tiling.slot_bytes(tw, th):][:cw * ch * 3] = tiling.resolve_ss(a, s).reshape(-1)
    return smp, want


def resolve_forms(total, seed=3):
    """The tile selections of a resolve: (first_tile, tile_stride, list or None, tiles) -- strided from 0, strided from 1
    by 2, a descending list, a shuffled list of half the tiles."""
    rng = np.random.default_rng(seed)
    out = [(0, 1, None, np.arange(total))]
    if total >= 2:
        out.append((1, 2, None, np.arange(1, total, 2)))
    out.append((0, 1, np.arange(total - 1, -1, -1, dtype=np.int32), None))
    out.append((0, 1, rng.permutation(total)[:max(1, total // 2)].astype(np.int32), None))
    return [(f, st, lst, lst if tiles is None else tiles) for f, st, lst, tiles in out]


# ---------------------------------------------------------------------------------------------------------------------
# 5. cost maps for tile_cost_kernel / tile_order_kernel / deal_tiles_kernel (csrc/mt_render.hip)
# (image_w, image_h, tile_w, tile_h): 1 tile; 255 / 256 / 257 (the 256-thread workgroup of the order kernel); ragged
# images under tiles of 5, 12, 16, 20 and 64 (5, 12 and 20: neighbouring tiles share map blocks); 2025 tiles
ORDER_GEOMETRIES = [(37, 21, 64, 64), (2040, 8, 8, 8), (2048, 8, 8, 8), (2056, 8, 8, 8), (203, 131, 5, 5),
                    (264, 150, 12, 12), (101, 67, 16, 16), (333, 177, 20, 20), (300, 200, 64, 64), (101, 67, 12, 20),
                    (223, 223, 5, 5)]
COST_MAPS = ("equal", "zero", "two_values", "all_ones_u32", "differ_above_bit_32", "random_u32", "wider_poisoned")
POISON = 0xFFFFFFFF


def cost_map(kind, geometry, seed=9):
    """uint32 [map_h][map_w] for the image of `geometry`; wider_poisoned: three columns and two rows more than the image
    needs, full of POISON."""
    W, H, tw, th = geometry
    mw, mh = (W + 7) // 8, (H + 7) // 8
    rng = np.random.default_rng(seed)
    if kind == "equal":
        return np.full((mh, mw), 1000, dtype=np.uint32)
    if kind == "zero":
        return np.zeros((mh, mw), dtype=np.uint32)
    if kind == "two_values":
        return np.where(rng.random((mh, mw)) < 0.5, 7, 90000).astype(np.uint32)
    if kind == "all_ones_u32":
        return np.full((mh, mw), 0xFFFFFFFF, dtype=np.uint32)
    if kind == "random_u32":
        return rng.integers(0, 2 ** 32, (mh, mw), dtype=np.uint64).astype(np.uint32)
    if kind == "wider_poisoned":
        m = np.full((mh + 2, mw + 3), POISON, dtype=np.uint32)
        m[:mh, :mw] = rng.integers(0, 2 ** 20, (mh, mw), dtype=np.uint64).astype(np.uint32)
        return m
    if kind == "differ_above_bit_32":
        # sums 5, 2^32 + 5 and 2 * 2^32 + 5 (and 0 elsewhere) in the first map cell(s) that only ONE tile sums -- the
        # cheapest in the lowest tile number: the low 32 bits alone order them by number, i.e. the wrong way round
        m = np.zeros((mh, mw), dtype=np.uint32)
        tx, ty = tiling.tile_grid(W, H, tw, th)
        owners = np.zeros((mh, mw), dtype=np.int32)
        first = {}
        for t in range(tx * ty):
            x0, y0, cw, ch = tiling.tile_rect(t, W, H, tw, th)
            owners[y0 >> 3:((y0 + ch - 1) >> 3) + 1, x0 >> 3:((x0 + cw - 1) >> 3) + 1] += 1
        for t in range(tx * ty):
            x0, y0, cw, ch = tiling.tile_rect(t, W, H, tw, th)
            ys, xs = np.nonzero(owners[y0 >> 3:((y0 + ch - 1) >> 3) + 1, x0 >> 3:((x0 + cw - 1) >> 3) + 1] == 1)
            first[t] = [((y0 >> 3) + y, (x0 >> 3) + x) for y, x in zip(ys[:3], xs[:3])]
        # (tiles of one map cell -- 8 x 8 -- cannot hold such sums: the map stays zero)
        three = [t for t in first if len(first[t]) >= 3]
        two = [t for t in first if len(first[t]) >= 2 and three and t < three[-1]]
        one = [t for t in first if len(first[t]) >= 1 and two and t < two[len(two) // 2]]
        if one:
            picks = [one[0], two[len(two) // 2], three[-1]]
            for t, cells in zip(picks, ([5], [0xFFFFFFFF, 6], [0xFFFFFFFF, 0xFFFFFFFF, 7])):
                for (y, x), v in zip(first[t], cells):
                    m[y, x] = v
        return m
    raise ValueError(kind)


def deal_worlds(total):
    return (1, 2, 3, 8, 16, total + 3)
