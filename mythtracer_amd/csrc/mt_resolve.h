// mt_resolve.h — supersampled frames: the s x s box filter that turns a frame of samples into a frame of pixels
// (include/mythtracer_hip.h, mt_render_chunk_ss ff.).  No reference counterpart: the reference renders one ray per
// pixel (mythtracer.cc:292-305); a sample frame is its frame at s W x s H, and output byte (x, y, c) is
//   (sum of the s*s sample bytes (s x + i, s y + j, c) + s*s/2) / (s*s)   in unsigned integer arithmetic.
//
// Layout: a buffer of tile slots as mt_render_tiles_device writes it.  Slot j holds tile t(j) of the OUTPUT image's
// tile_w x tile_h grid, edge-clipped to cw x ch, as a chunk-local row-major RGB8 bitmap at out + j tile_w tile_h 3;
// its samples are the same tile of the sample image's (s tile_w) x (s tile_h) grid, clipped to s cw x s ch, at
// samples + j (s tile_w)(s tile_h) 3.  A chunk is the one tile of an image of its own size.
//
// The kernel is memory-bound (3 s*s bytes in, 3 out per pixel).  A thread makes four consecutive pixels of a row --
// twelve bytes, three dwords -- from s sample rows of 12 s bytes.  Rows start at multiples of 3 bytes only, so a row
// is cut into a head of 0 .. 3 pixels up to the first pixel whose output byte address is a multiple of 4 (pixel p of a
// row at byte address R lies at R + 3 p: aligned when p = R mod 4), groups of four pixels from there, and a tail of
// 0 .. 3 pixels.  Head and tail go byte by byte (resolve_pixel); a group stores three aligned dwords and reads every
// sample row as aligned dwords around its 12 s bytes, shifted into place (resolve_group).
#pragma once
#include <stdint.h>

namespace mt {

struct ResolveArgs {
  int image_w, image_h;  // OUTPUT image
  int tile_w, tile_h, tiles_x;
  int first_tile, tile_stride, n_tiles;
  const int32_t *tile_list;  // nullable: slot j holds tile tile_list[j], else first_tile + j tile_stride
  int rows;                  // rows of a slot that can hold pixels: min(tile_h, image_h)
  int units;                 // work units per row: groups a row can hold at most + head + tail
  const uint8_t *samples;
  uint8_t *out;
};

// one output pixel: `in` = its first sample in the first of its S sample rows, in_pitch = bytes per sample row
template <int S>
__device__ inline void resolve_pixel(const uint8_t *in, size_t in_pitch, uint8_t *out) {
  constexpr unsigned N = S * S;
  for (int c = 0; c < 3; c++) {
    unsigned sum = 0;
    for (int j = 0; j < S; j++) {
      for (int i = 0; i < S; i++) sum += in[(size_t)j * in_pitch + i * 3 + c];
    }
    out[c] = (uint8_t)((sum + N / 2) / N);
  }
}

// four output pixels at a dword-aligned `out`: 12 S sample bytes per sample row from `in` (any alignment)
template <int S>
__device__ inline void resolve_group(const uint8_t *in, size_t in_pitch, uint8_t *out) {
  constexpr unsigned N = S * S;
  constexpr int W = 3 * S;  // dwords of samples per row
  // column sums over the S rows, two 16-bit fields per word (at most 4 x 255 each): bytes 0 and 2 of dword k in ev[k],
  // bytes 1 and 3 in od[k]
  uint32_t ev[W], od[W];
#pragma unroll
  for (int k = 0; k < W; k++) ev[k] = od[k] = 0;
#pragma unroll
  for (int j = 0; j < S; j++) {
    const uint8_t *row = in + (size_t)j * in_pitch;
    const unsigned mis = (unsigned)((uintptr_t)row & 3);
    const uint32_t *a = (const uint32_t *)(row - mis);  // the aligned dwords that hold row[0 .. 12 S)
    uint32_t raw[W + 1];
#pragma unroll
    for (int k = 0; k < W; k++) raw[k] = a[k];
    raw[W] = mis != 0 ? a[W] : 0;  // (holds sample bytes of this group only when mis != 0: never read otherwise)
#pragma unroll
    for (int k = 0; k < W; k++) {
      const uint32_t w = (uint32_t)((((uint64_t)raw[k + 1] << 32) | raw[k]) >> (8 * mis));  // row[4 k .. 4 k + 4)
      ev[k] += w & 0x00ff00ffu;
      od[k] += (w >> 8) & 0x00ff00ffu;
    }
  }
  uint32_t o[3] = {0, 0, 0};
#pragma unroll
  for (int b = 0; b < 12; b++) {  // output byte b = pixel b / 3, channel b % 3
    unsigned sum = 0;
#pragma unroll
    for (int i = 0; i < S; i++) {
      const int off = ((b / 3) * S + i) * 3 + b % 3;  // byte of the sample row
      const uint32_t v = (off & 1) ? od[off >> 2] : ev[off >> 2];
      sum += (v >> ((off & 2) * 8)) & 0xffffu;
    }
    o[b >> 2] |= ((sum + N / 2) / N) << ((b & 3) * 8);
  }
  uint32_t *dst = (uint32_t *)out;
  dst[0] = o[0];
  dst[1] = o[1];
  dst[2] = o[2];
}

// work unit `idx` of the launch: (slot, row, unit of the row); unit 0 = the head, 1 = the tail, 2 + g = group g
template <int S>
__device__ inline void resolve_unit(const ResolveArgs &A, unsigned idx) {
  const unsigned u = idx % (unsigned)A.units;
  const unsigned ly = (idx / (unsigned)A.units) % (unsigned)A.rows;
  const unsigned j = idx / (unsigned)A.units / (unsigned)A.rows;
  const int tile = A.tile_list != nullptr ? A.tile_list[j] : A.first_tile + (int)j * A.tile_stride;
  const int x0 = (tile % A.tiles_x) * A.tile_w, y0 = (tile / A.tiles_x) * A.tile_h;
  const int cw = min(A.tile_w, A.image_w - x0), ch = min(A.tile_h, A.image_h - y0);
  if (cw <= 0 || (int)ly >= ch) return;  // (a tile number outside the image, from a caller's list: nothing to do)
  const size_t in_pitch = (size_t)cw * S * 3;
  uint8_t *out_row = A.out + (size_t)j * A.tile_w * A.tile_h * 3 + (size_t)ly * cw * 3;
  const uint8_t *in_row = A.samples + (size_t)j * A.tile_w * A.tile_h * 3 * S * S + (size_t)ly * S * in_pitch;
  const int head = min(cw, (int)((uintptr_t)out_row & 3));
  const int groups = (cw - head) / 4;
  int p0, p1;  // this unit's pixels of the row
  if (u == 0) {
    p0 = 0; p1 = head;
  } else if (u == 1) {
    p0 = head + 4 * groups; p1 = cw;
  } else {
    if ((int)(u - 2) >= groups) return;
    p0 = head + 4 * (int)(u - 2);
    resolve_group<S>(in_row + (size_t)p0 * S * 3, in_pitch, out_row + (size_t)p0 * 3);
    return;
  }
  for (int p = p0; p < p1; p++) resolve_pixel<S>(in_row + (size_t)p * S * 3, in_pitch, out_row + (size_t)p * 3);
}

template <int S>
__global__ void __launch_bounds__(256) resolve_kernel(ResolveArgs A, unsigned total) {
  for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    resolve_unit<S>(A, idx);
  }
}

}  // namespace mt
