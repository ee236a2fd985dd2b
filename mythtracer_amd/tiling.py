"""Tile bookkeeping for multi-GPU frames.

Mirrors the master's work split in the reference: the frame is cut into
tile_w x tile_h WorkChunks in row-major order, edge tiles clipped
(VerStarting/main_net_master.cc:195-221 GenerateWork), each rendered with the
full-image sensor and blitted back by (chunk_y + j) * image_width + chunk_x + i
(main_net_master.cc:223-236 BlitWorkChunk).  Here tile k belongs to rank
k mod world_size, so that expensive image regions are spread over all GPUs.

The device-side equivalents are mt_render_tiles_device / mt_blit_tiles_device
of the C ABI; this module is the host-side description of the same layout (and
a numpy blit used by the CPU tests of the distributed path).
"""
from __future__ import annotations

import numpy as np


def tile_grid(image_w: int, image_h: int, tile_w: int, tile_h: int):
    """(tiles_x, tiles_y)."""
    return (image_w + tile_w - 1) // tile_w, (image_h + tile_h - 1) // tile_h


def tile_rect(k: int, image_w: int, image_h: int, tile_w: int, tile_h: int):
    """(x, y, w, h) of tile k, clipped to the image like GenerateWork does."""
    tx, _ = tile_grid(image_w, image_h, tile_w, tile_h)
    x0, y0 = (k % tx) * tile_w, (k // tx) * tile_h
    return x0, y0, min(tile_w, image_w - x0), min(tile_h, image_h - y0)


def rank_tiles(image_w: int, image_h: int, tile_w: int, tile_h: int, rank: int, world: int):
    """(first_tile, tile_stride, n_tiles) of one rank: tiles rank, rank+world, ..."""
    tx, ty = tile_grid(image_w, image_h, tile_w, tile_h)
    total = tx * ty
    n = 0 if rank >= total else (total - rank + world - 1) // world
    return rank, world, n


def max_tiles_per_rank(image_w, image_h, tile_w, tile_h, world):
    return rank_tiles(image_w, image_h, tile_w, tile_h, 0, world)[2]


def dealt_position(q: int, world: int, rank: int) -> int:
    """Position, in the cost order of the tiles, of the tile rank `rank` holds in round q: the rounds change
    direction (0 1 .. N-1, N-1 .. 1 0, ...) -- mt_order_tiles_device / deal_tiles_kernel of the C ABI."""
    return q * world + ((world - 1 - rank) if (q & 1) else rank)


def dealt_tile_count(n_tiles: int, world: int, rank: int) -> int:
    n = 0
    for q in (n_tiles // world - 1, n_tiles // world):
        if q >= 0 and dealt_position(q, world, rank) < n_tiles:
            n = q + 1
    return n


def order_tiles(cost_map: np.ndarray, image_w: int, image_h: int, tile_w: int, tile_h: int) -> np.ndarray:
    """Tiles by summed block cost, most expensive first, ties by tile number (numpy restatement of
    tile_cost_kernel + tile_order_kernel; cost_map = uint32 [map_h][map_w], one word per 8x8 block)."""
    tx, ty = tile_grid(image_w, image_h, tile_w, tile_h)
    cost = np.zeros(tx * ty, dtype=np.uint64)
    for t in range(tx * ty):
        x0, y0, cw, ch = tile_rect(t, image_w, image_h, tile_w, tile_h)
        cost[t] = cost_map[y0 >> 3:((y0 + ch - 1) >> 3) + 1, x0 >> 3:((x0 + cw - 1) >> 3) + 1].astype(np.uint64).sum()
    return np.lexsort((np.arange(tx * ty), -cost.astype(np.int64))).astype(np.int32)


def deal_tiles(order, n_tiles: int, world: int, rank: int) -> np.ndarray:
    """The rank's tile list in slot order (order None: by tile number)."""
    n = dealt_tile_count(n_tiles, world, rank)
    pos = np.array([dealt_position(q, world, rank) for q in range(n)], dtype=np.int64)
    return (pos if order is None else np.asarray(order)[pos]).astype(np.int32)


def blit_tile_list(image: np.ndarray, tiles: np.ndarray, tile_w: int, tile_h: int, tile_list) -> None:
    """BlitWorkChunk for a buffer whose slot j holds tile tile_list[j] (numpy, host)."""
    image_h, image_w, _ = image.shape
    sb = slot_bytes(tile_w, tile_h)
    flat = np.asarray(tiles, dtype=np.uint8).reshape(-1)
    for j, t in enumerate(tile_list):
        x0, y0, cw, ch = tile_rect(int(t), image_w, image_h, tile_w, tile_h)
        image[y0:y0 + ch, x0:x0 + cw] = flat[j * sb: j * sb + cw * ch * 3].reshape(ch, cw, 3)


def slot_bytes(tile_w: int, tile_h: int) -> int:
    return tile_w * tile_h * 3


def blit_tiles(image: np.ndarray, tiles: np.ndarray, tile_w: int, tile_h: int,
               first_tile: int, tile_stride: int, n_tiles: int) -> None:
    """BlitWorkChunk for a buffer of tile slots (numpy, host).  `tiles` is a
    flat uint8 array of n_tiles slots of tile_w*tile_h*3 bytes; slot j holds
    the chunk-local row-major bitmap of tile first_tile + j*tile_stride."""
    image_h, image_w, _ = image.shape
    sb = slot_bytes(tile_w, tile_h)
    flat = np.asarray(tiles, dtype=np.uint8).reshape(-1)
    for j in range(n_tiles):
        x0, y0, cw, ch = tile_rect(first_tile + j * tile_stride, image_w, image_h, tile_w, tile_h)
        chunk = flat[j * sb: j * sb + cw * ch * 3].reshape(ch, cw, 3)
        image[y0:y0 + ch, x0:x0 + cw] = chunk


def resolve_ss(samples: np.ndarray, s: int) -> np.ndarray:
    """A supersampled frame from its sample frame (numpy restatement of resolve_kernel, csrc/mt_resolve.h):
    samples = uint8 [s H][s W][C]; output byte (y, x, c) = (sum + n // 2) // n with n = s * s and sum = the n sample
    bytes (s y + j, s x + i, c), 0 <= i, j < s -- the rounded mean, ties up, in integer arithmetic."""
    a = np.asarray(samples)
    if a.dtype != np.uint8 or a.ndim != 3:
        raise ValueError("samples must be a uint8 array [height][width][channels]")
    if not 1 <= int(s) <= 4:
        raise ValueError("supersampling factor %r outside 1 .. 4" % (s,))
    s = int(s)
    sh, sw, c = a.shape
    if sh % s or sw % s:
        raise ValueError("sample frame %dx%d is not a multiple of %d" % (sw, sh, s))
    n = s * s
    total = a.reshape(sh // s, s, sw // s, s, c).astype(np.uint32).sum(axis=(1, 3))
    return ((total + n // 2) // n).astype(np.uint8)


# ---- adaptive supersampling (include/mythtracer_hip.h, mt_render_chunk_adaptive ff.; csrc/mt_adaptive.h)
def chunk_blocks(chunk):
    """The blocks of a chunk -- those of the IMAGE's 8 x 8 grid that hold a chunk pixel: (mask_x0, mask_y0, mask_w,
    mask_h)."""
    cx, cy, cw, ch = chunk
    x0, y0 = cx // 8, cy // 8
    return x0, y0, (cx + cw - 1) // 8 - x0 + 1, (cy + ch - 1) // 8 - y0 + 1


def refine_mask(plain_rgb: np.ndarray, image_w: int, image_h: int, chunk=None, threshold: int = 16):
    """Which blocks of a chunk does an adaptive frame supersample?  plain_rgb = the chunk's plain frame, uint8
    [chunk_h][chunk_w][3].  Two horizontal or vertical neighbours inside the chunk are contrasty when they differ by
    more than `threshold` in a channel; a block is refined iff a pixel of a contrasty pair lies in it.  Returns (mask
    bool [mask_h][mask_w], the refined blocks' tile numbers by * ceil(image_w / 8) + bx, int32 ascending)."""
    cx, cy, cw, ch = chunk if chunk else (0, 0, image_w, image_h)
    f = np.asarray(plain_rgb)
    if f.dtype != np.uint8 or f.shape != (ch, cw, 3):
        raise ValueError("plain_rgb must be the chunk's uint8 [%d][%d][3] bitmap" % (ch, cw))
    if not 0 <= int(threshold) <= 255:
        raise ValueError("threshold %r outside 0 .. 255" % (threshold,))
    f = f.astype(np.int16)
    hot = np.zeros((ch, cw), dtype=bool)  # pixels of contrasty pairs
    h = np.abs(f[:, 1:] - f[:, :-1]).max(axis=2) > int(threshold)
    hot[:, 1:] |= h
    hot[:, :-1] |= h
    v = np.abs(f[1:] - f[:-1]).max(axis=2) > int(threshold)
    hot[1:] |= v
    hot[:-1] |= v
    x0, y0, mw, mh = chunk_blocks((cx, cy, cw, ch))
    mask = np.zeros((mh, mw), dtype=bool)
    ys, xs = np.nonzero(hot)
    mask[(ys + cy) // 8 - y0, (xs + cx) // 8 - x0] = True
    my, mx = np.nonzero(mask)
    tiles = ((my + y0) * ((image_w + 7) // 8) + mx + x0).astype(np.int32)
    return mask, tiles


def compose_adaptive(plain_rgb: np.ndarray, ss_rgb: np.ndarray, mask: np.ndarray, chunk) -> np.ndarray:
    """The adaptive frame of a chunk: the supersampled frame's bytes where the pixel's block is refined, the plain
    frame's elsewhere.  mask as refine_mask returns it for `chunk`."""
    cx, cy, cw, ch = chunk
    x0, y0, mw, mh = chunk_blocks(chunk)
    m = np.asarray(mask, dtype=bool)
    if m.shape != (mh, mw):
        raise ValueError("mask must be [%d][%d] for this chunk" % (mh, mw))
    by = (np.arange(ch) + cy) // 8 - y0
    bx = (np.arange(cw) + cx) // 8 - x0
    px = m[by[:, None], bx[None, :]]
    return np.where(px[:, :, None], np.asarray(ss_rgb), np.asarray(plain_rgb)).astype(np.uint8)


# ---- the ray-tree buffer (include/mythtracer_hip.h, mt_raytree_create ff.; csrc/mt_raytree.h)
def raytree_layer0_order(chunk_w: int, chunk_h: int) -> np.ndarray:
    """The order of a ray tree's layer 0 (numpy restatement of raytree_layer0_index, csrc/mt_raytree.h): entry i = the
    chunk-local row-major pixel index of ray i.  The 8 x 8 blocks of the CHUNK in row-major order, within a block its
    pixels in row-major order; a block cut by the chunk's right or bottom edge holds only its pixels, so the list has
    chunk_w * chunk_h entries.  A fixed function of (chunk_w, chunk_h)."""
    if chunk_w <= 0 or chunk_h <= 0:
        raise ValueError("chunk %dx%d is empty" % (chunk_w, chunk_h))
    out = []
    for by in range(0, chunk_h, 8):
        ys = np.arange(by, min(by + 8, chunk_h))
        for bx in range(0, chunk_w, 8):
            xs = np.arange(bx, min(bx + 8, chunk_w))
            out.append((ys[:, None] * chunk_w + xs[None, :]).reshape(-1))
    return np.concatenate(out).astype(np.int32)
