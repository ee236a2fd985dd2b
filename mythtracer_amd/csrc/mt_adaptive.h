// mt_adaptive.h — adaptive supersampling (include/mythtracer_hip.h, mt_render_chunk_adaptive ff.): supersample only the
// 8 x 8 blocks of the IMAGE's grid in which neighbouring pixels of the plain frame differ.  No reference counterpart;
// the definition is integer arithmetic on bytes the library already makes (mythtracer_amd/tiling.py restates it:
// refine_mask, compose_adaptive).
//
//   refine_mask_kernel     one wave per block of the chunk, one lane per pixel: the flag "some horizontal or vertical
//                          pair of chunk pixels with a pixel in this block differs by more than `threshold` in a channel"
//   refine_compact_kernel  one workgroup: the flagged blocks' tile numbers in ascending order (a scan, not atomics:
//                          the same frame gives the same list), their count, and a hash of the list that does not
//                          depend on thread order -- a sum over j of mix(j, list[j])
//   refine_resolve_kernel  slot j of the refinement launch's samples (tile list[j] of the sample image's 8 S x 8 S grid,
//                          clipped to the image) box-filtered -- resolve_pixel of mt_resolve.h, the same arithmetic --
//                          over the chunk's bitmap at the block's place, clipped to the chunk
//
// All three go byte by byte: a block's rows are 24 bytes at any alignment, and the kernels move a few hundred KB at
// most next to launches of milliseconds (DESIGN.md section 3.9 has the times).
#pragma once
#include <stdint.h>

#include "mt_resolve.h"

namespace mt {

struct RefineArgs {
  int chunk_x, chunk_y, chunk_w, chunk_h;
  int tiles_x;                      // blocks per row of the IMAGE: a block's tile number is by tiles_x + bx
  int mask_x0, mask_y0, mask_w, mask_h;  // the chunk's blocks
  int threshold;
  const uint8_t *rgb;               // the chunk's bitmap, chunk-local row-major RGB8
  uint8_t *flags;                   // [mask_w mask_h] 0 / 1
  uint8_t *mask_out;                // nullable: the caller's copy of the flags
};

constexpr int kRefineCompactThreads = 1024;

// the word at refine_compact_kernel's `ctl`: what the host reads back
struct RefineCtl {
  uint32_t count, pad;
  uint64_t hash;
};

// pixel (x, y) of the chunk's bitmap as 0x00BBGGRR
__device__ inline uint32_t refine_load_px(const RefineArgs &A, int x, int y) {
  const uint8_t *p = A.rgb + ((size_t)y * (size_t)A.chunk_w + (size_t)x) * 3;
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

__device__ inline bool refine_contrasty(uint32_t a, uint32_t b, int threshold) {
  int m = 0;
  for (int c = 0; c < 3; c++) {
    const int d = (int)((a >> (8 * c)) & 0xffu) - (int)((b >> (8 * c)) & 0xffu);
    m = max(m, d < 0 ? -d : d);
  }
  return m > threshold;
}

__global__ void __launch_bounds__(256) refine_mask_kernel(RefineArgs A) {
  const int lane = (int)(threadIdx.x & 63u);
  const unsigned n_blocks = (unsigned)A.mask_w * (unsigned)A.mask_h;
  const unsigned waves = gridDim.x * (blockDim.x >> 6);
  for (unsigned b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); b < n_blocks; b += waves) {  // (wave-uniform)
    const int bx = A.mask_x0 + (int)(b % (unsigned)A.mask_w), by = A.mask_y0 + (int)(b / (unsigned)A.mask_w);
    // this lane's pixel in chunk coordinates; a block at the chunk's border has lanes outside the chunk
    const int lx = lane & 7, ly = lane >> 3;
    const int x = bx * 8 + lx - A.chunk_x, y = by * 8 + ly - A.chunk_y;
    const bool in = x >= 0 && x < A.chunk_w && y >= 0 && y < A.chunk_h;
    const uint32_t v = in ? refine_load_px(A, x, y) : 0u;
    // the right and lower neighbours inside the block come from their lanes; all 64 lanes take part in the exchange
    const uint32_t from_right = (uint32_t)__shfl((int)v, (lane + 1) & 63, 64);
    const uint32_t from_below = (uint32_t)__shfl((int)v, (lane + 8) & 63, 64);
    bool hit = false;
    if (in) {
      if (x + 1 < A.chunk_w) hit |= refine_contrasty(v, lx < 7 ? from_right : refine_load_px(A, x + 1, y), A.threshold);
      if (y + 1 < A.chunk_h) hit |= refine_contrasty(v, ly < 7 ? from_below : refine_load_px(A, x, y + 1), A.threshold);
      // the halo on the other two sides: pairs whose other pixel lies in the block to the left / above
      if (lx == 0 && x > 0) hit |= refine_contrasty(v, refine_load_px(A, x - 1, y), A.threshold);
      if (ly == 0 && y > 0) hit |= refine_contrasty(v, refine_load_px(A, x, y - 1), A.threshold);
    }
    const bool any = __ballot(hit) != 0ull;
    if (lane == 0) {
      A.flags[b] = any ? 1 : 0;
      if (A.mask_out != nullptr) A.mask_out[b] = any ? 1 : 0;
    }
  }
}

__device__ inline uint64_t refine_mix(uint64_t j, uint64_t tile) {  // (splitmix64's finaliser)
  uint64_t z = j * 0x9e3779b97f4a7c15ull + tile + 0x632be59bd9b4e019ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// One workgroup of kRefineCompactThreads: thread t owns the flags [t per, (t + 1) per); an exclusive scan of the
// threads' counts gives each its place in the list.
__global__ void __launch_bounds__(kRefineCompactThreads) refine_compact_kernel(RefineArgs A, int32_t *list, uint32_t *count_out,
                                                                                RefineCtl *ctl) {
  __shared__ uint32_t s_count[kRefineCompactThreads];
  __shared__ uint64_t s_hash[kRefineCompactThreads];
  const unsigned t = threadIdx.x;
  const unsigned n = (unsigned)A.mask_w * (unsigned)A.mask_h;
  const unsigned per = (n + kRefineCompactThreads - 1) / kRefineCompactThreads;
  const unsigned i0 = min(t * per, n), i1 = min(i0 + per, n);
  uint32_t mine = 0;
  for (unsigned i = i0; i < i1; i++) mine += A.flags[i];
  s_count[t] = mine;
  __syncthreads();
  // inclusive scan (Hillis-Steele) over the threads' counts
  for (unsigned d = 1; d < kRefineCompactThreads; d <<= 1) {
    const uint32_t add = t >= d ? s_count[t - d] : 0u;
    __syncthreads();
    s_count[t] += add;
    __syncthreads();
  }
  uint32_t j = s_count[t] - mine;
  uint64_t h = 0;
  for (unsigned i = i0; i < i1; i++) {
    if (A.flags[i] == 0) continue;
    const int tile = (A.mask_y0 + (int)(i / (unsigned)A.mask_w)) * A.tiles_x + A.mask_x0 + (int)(i % (unsigned)A.mask_w);
    list[j] = tile;
    h += refine_mix(j, (uint64_t)(uint32_t)tile);
    j++;
  }
  s_hash[t] = h;
  __syncthreads();
  for (unsigned d = kRefineCompactThreads / 2; d > 0; d >>= 1) {
    if (t < d) s_hash[t] += s_hash[t + d];
    __syncthreads();
  }
  if (t == 0) {
    const uint32_t total = s_count[kRefineCompactThreads - 1];
    if (count_out != nullptr) *count_out = total;
    ctl->count = total;
    ctl->pad = 0;
    ctl->hash = s_hash[0];
  }
}

struct RefineResolveArgs {
  int image_w, image_h;  // OUTPUT image
  int chunk_x, chunk_y, chunk_w, chunk_h;
  int tiles_x;
  int n_slots;
  const int32_t *list;     // slot j holds the samples of block list[j]
  const uint8_t *samples;  // slots of 8 S x 8 S samples, edge blocks clipped to the image
  uint8_t *rgb;            // the chunk's bitmap
};

// one lane per pixel of a block, four blocks per workgroup
template <int S>
__global__ void __launch_bounds__(256) refine_resolve_kernel(RefineResolveArgs A) {
  const unsigned total = (unsigned)A.n_slots * 64u;
  for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const unsigned j = idx >> 6;
    const int lx = (int)(idx & 7u), ly = (int)((idx >> 3) & 7u);
    const int tile = A.list[j];
    const int x0 = (tile % A.tiles_x) * 8, y0 = (tile / A.tiles_x) * 8;
    const int cw = min(8, A.image_w - x0), ch = min(8, A.image_h - y0);  // the block within the image: the slot's layout
    if (lx >= cw || ly >= ch) continue;
    const int x = x0 + lx - A.chunk_x, y = y0 + ly - A.chunk_y;
    if (x < 0 || x >= A.chunk_w || y < 0 || y >= A.chunk_h) continue;  // rendered, but not this chunk's pixel
    const size_t in_pitch = (size_t)cw * S * 3;
    const uint8_t *in = A.samples + (size_t)j * (size_t)(64 * S * S * 3) + (size_t)ly * S * in_pitch + (size_t)lx * S * 3;
    resolve_pixel<S>(in, in_pitch, A.rgb + ((size_t)y * (size_t)A.chunk_w + (size_t)x) * 3);
  }
}

}  // namespace mt
