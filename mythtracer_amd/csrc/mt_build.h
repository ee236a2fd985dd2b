// mt_build.h -- the octree built on the GPU from triangles in ADD order (mt_octree_build): node for node and bit for bit
// the tree OctTree::Finalize builds on the host (host/src/octtree.cc, the reference's AttemptSplit).
//
// A node's split depends only on its box and on the NUMBER of triangles that reached it; the partition into children is
// stable and the root's list is 0 .. n-1, so every node's final list is in ascending add index.  The whole tree is
// therefore fixed by (a) the node each triangle ends in and (b) the breadth-first numbering of the nodes:
//   build_tri_box_kernel   a thread per triangle: its box (Triangle::CacheAABB), and the root box by integer atomics on
//                          an order-preserving encoding of the doubles (OctTree::AddPrimitive's rules restated)
//   build_root_kernel      node 0
//   per level (one host round trip: the number of nodes that split):
//     [rocPRIM exclusive scan of `reached >= 16` over the level's nodes: a level is a contiguous range of indices]
//     build_split_kernel   a thread per node of the level: centre, first_child, the eight children's boxes
//     build_descend_kernel a thread per triangle: the FIRST child whose box fully contains the triangle's box, or stay;
//                          the children's `reached` counters by integer atomicAdd, one per wave and child
//   build_finish_kernel    a thread per triangle: its final node as the sort key, the nodes' prim_count
//   [rocPRIM exclusive scan of prim_count -> prim_begin; rocPRIM stable radix sort of (node, add index) -> tri_id]
// Nothing depends on the order in which atomics arrive: they only add integers or take integer minima / maxima.
// Every fp64 expression is the host builder's, in its order (-ffp-contract=off as everywhere).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace mt {

constexpr int kBuildSplit = 16;      // OctTree::SPLIT_BOUNDARY
constexpr int kBuildThreads = 256;

// the tree while it grows: arrays of `capacity` nodes (the host grows them before a level's children are written)
struct BuildTree {
  double *aabb;        // [n][6] min xyz, max xyz
  double *center;      // [n][3], zero for a node that does not split
  int32_t *first_child;
  int32_t *reached;    // triangles that reached the node
  int32_t *prim_count; // triangles that end in it (build_finish_kernel)
};

// a double as a 64-bit key whose unsigned order is the doubles' (-0.0 below +0.0; not for NaN)
__device__ __forceinline__ unsigned long long build_key(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double build_unkey(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
  return __longlong_as_double((long long)u);
}
// the key of +0.0: what root_key[0..5] hold before build_tri_box_kernel
constexpr unsigned long long kBuildKeyZero = 0x8000000000000000ull;

// std::min(a, b) / std::max(a, b) with the host's operand order: b only where the comparison holds (a NaN in b never
// enters, a NaN in a stays)
__device__ __forceinline__ double build_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double build_max(double a, double b) { return a < b ? b : a; }

// Triangle::CacheAABB for triangle i of vertex[n][9] -> tri_aabb[n][6]; OctTree::AddPrimitive's root box into
// root_key[6].  The root starts as {0,0,0}-{0,0,0} (+0.0) and takes std::min(root, box.min) / std::max(root, box.max):
// a NaN bound never enters, and a bound that comes out as zero is the initial +0.0 (neither -0.0 < +0.0 nor
// +0.0 < -0.0 holds); every other tie is between equal bits.  So the result is the minimum / maximum over +0.0 and
// the bounds that are not NaN, with a zero result restated as +0.0 (build_root_kernel): order-free.
__global__ __launch_bounds__(kBuildThreads) void build_tri_box_kernel(const double *__restrict__ vertex, uint32_t n,
                                                                       double *__restrict__ tri_aabb,
                                                                       unsigned long long *__restrict__ root_key) {
  __shared__ unsigned long long red[6][kBuildThreads];
  const uint32_t i = blockIdx.x * kBuildThreads + threadIdx.x;
  unsigned long long key[6] = {kBuildKeyZero, kBuildKeyZero, kBuildKeyZero, kBuildKeyZero, kBuildKeyZero, kBuildKeyZero};
  if (i < n) {
    const double *v = vertex + (size_t)i * 9;
    double lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
      lo[a] = hi[a] = v[a];
      lo[a] = build_min(lo[a], v[3 + a]);
      hi[a] = build_max(hi[a], v[3 + a]);
      lo[a] = build_min(lo[a], v[6 + a]);
      hi[a] = build_max(hi[a], v[6 + a]);
      tri_aabb[(size_t)i * 6 + a] = lo[a];
      tri_aabb[(size_t)i * 6 + 3 + a] = hi[a];
      if (lo[a] == lo[a]) key[a] = build_key(lo[a]);
      if (hi[a] == hi[a]) key[3 + a] = build_key(hi[a]);
    }
  }
  for (int q = 0; q < 6; q++) red[q][threadIdx.x] = key[q];
  __syncthreads();
  for (int step = kBuildThreads / 2; step > 0; step >>= 1) {
    if ((int)threadIdx.x < step) {
      for (int q = 0; q < 3; q++) {
        const unsigned long long a = red[q][threadIdx.x], b = red[q][threadIdx.x + step];
        red[q][threadIdx.x] = b < a ? b : a;
        const unsigned long long c = red[3 + q][threadIdx.x], d = red[3 + q][threadIdx.x + step];
        red[3 + q][threadIdx.x] = c < d ? d : c;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) atomicMin(&root_key[threadIdx.x], red[threadIdx.x][0]);
  else if (threadIdx.x < 6) atomicMax(&root_key[threadIdx.x], red[threadIdx.x][0]);
}

// node 0: the root box out of its keys, reached by all n triangles
__global__ void build_root_kernel(BuildTree T, const unsigned long long *__restrict__ root_key, int32_t n_tris) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  for (int q = 0; q < 6; q++) {
    const double v = build_unkey(root_key[q]);
    T.aabb[q] = v == 0.0 ? 0.0 : v;
  }
  for (int a = 0; a < 3; a++) T.center[a] = 0.0;
  T.first_child[0] = 0;
  T.reached[0] = n_tris;
  T.prim_count[0] = 0;
}

// `reached >= 16` as 0 / 1: the scan's input
struct BuildSplits {
  __host__ __device__ int32_t operator()(int32_t reached) const { return reached >= kBuildSplit ? 1 : 0; }
};

// The nodes level_begin + j, j < level_n, that split: Node::CalcCenter, first_child = next_begin + 8 x (the splitting
// nodes of the level before it: split_before[j]), and the eight children as Octant() makes them -- bit 0 = upper x,
// bit 1 = upper z, bit 2 = upper y -- with no centre, no child and nothing reached yet.  The host has made room for
// next_begin + 8 x (the level's splits) nodes.
__global__ __launch_bounds__(kBuildThreads) void build_split_kernel(BuildTree T, int32_t level_begin, int32_t level_n,
                                                                     const int32_t *__restrict__ split_before,
                                                                     int32_t next_begin) {
  const int32_t j = (int32_t)(blockIdx.x * kBuildThreads + threadIdx.x);
  if (j >= level_n) return;
  const int32_t node = level_begin + j;
  if (T.reached[node] < kBuildSplit) return;
  double lo[3], hi[3], c[3];
  for (int a = 0; a < 3; a++) {
    lo[a] = T.aabb[(size_t)node * 6 + a];
    hi[a] = T.aabb[(size_t)node * 6 + 3 + a];
    c[a] = lo[a] + (hi[a] - lo[a]) / 2.0;
    T.center[(size_t)node * 3 + a] = c[a];
  }
  const int32_t first = next_begin + 8 * split_before[j];
  T.first_child[node] = first;
  for (int k = 0; k < 8; k++) {
    const bool up[3] = {(k & 1) != 0, (k & 4) != 0, (k & 2) != 0};  // x, y, z
    const size_t kid = (size_t)first + (size_t)k;
    for (int a = 0; a < 3; a++) {
      T.aabb[kid * 6 + a] = up[a] ? c[a] : lo[a];
      T.aabb[kid * 6 + 3 + a] = up[a] ? hi[a] : c[a];
      T.center[kid * 3 + a] = 0.0;
    }
    T.first_child[kid] = 0;
    T.reached[kid] = 0;
    T.prim_count[kid] = 0;
  }
}

// One level down for every triangle that is still on its way (cur[i] >= 0: the node it has reached, a node of the
// current level; ~node once it has found its home).  In a node that split it goes to the FIRST child k = 0 .. 7 whose
// box FullyContains its box -- closed intervals, p >= min && p <= max, so any NaN means not contained --, else it
// stays.  The children's boxes are the parent's bounds and centre, selected as build_split_kernel selects them.
// `reached` of the children: one atomicAdd per wave and child (the lanes of a wave mostly share their node).
__global__ __launch_bounds__(kBuildThreads) void build_descend_kernel(BuildTree T, const double *__restrict__ tri_aabb,
                                                                       int32_t *__restrict__ cur, uint32_t n) {
  const uint32_t i = blockIdx.x * kBuildThreads + threadIdx.x;
  int32_t to = -1;  // the child this lane's triangle moves to
  if (i < n) {
    const int32_t node = cur[i];
    if (node >= 0) {
      const int32_t first = T.first_child[node];
      if (first != 0) {
        double lo[3], hi[3], c[3], bl[3], bh[3];
        for (int a = 0; a < 3; a++) {
          lo[a] = T.aabb[(size_t)node * 6 + a];
          hi[a] = T.aabb[(size_t)node * 6 + 3 + a];
          c[a] = T.center[(size_t)node * 3 + a];
          bl[a] = tri_aabb[(size_t)i * 6 + a];
          bh[a] = tri_aabb[(size_t)i * 6 + 3 + a];
        }
        for (int k = 0; k < 8 && to < 0; k++) {
          const bool up[3] = {(k & 1) != 0, (k & 4) != 0, (k & 2) != 0};
          bool inside = true;
          for (int a = 0; a < 3; a++) {
            const double mn = up[a] ? c[a] : lo[a], mx = up[a] ? hi[a] : c[a];
            inside = inside && (bl[a] >= mn && bl[a] <= mx) && (bh[a] >= mn && bh[a] <= mx);
          }
          if (inside) to = first + k;
        }
      }
      cur[i] = to >= 0 ? to : ~node;
    }
  }
  // (every lane of the wave gets here)
  const int lane = (int)(threadIdx.x & 63u);
  unsigned long long todo = __ballot(to >= 0);
  for (int round = 0; round < 64 && todo != 0ull; round++) {
    const int leader = __ffsll((long long)todo) - 1;
    const int32_t key = __shfl(to, leader);
    const unsigned long long same = __ballot(to == key);
    if (lane == leader) atomicAdd(&T.reached[key], (int32_t)__popcll(same));
    todo &= ~same;
  }
}

// the node each triangle ends in as the sort's key, the add index as its value, and the nodes' prim_count
__global__ __launch_bounds__(kBuildThreads) void build_finish_kernel(BuildTree T, const int32_t *__restrict__ cur, uint32_t n,
                                                                      uint32_t *__restrict__ key, int32_t *__restrict__ value) {
  const uint32_t i = blockIdx.x * kBuildThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t c = cur[i];
  const int32_t node = c < 0 ? ~c : c;
  key[i] = (uint32_t)node;
  value[i] = (int32_t)i;
  atomicAdd(&T.prim_count[node], 1);
}

// ---- triangles moved in place (mt_scene_set_triangle_vertices): the scene's per-triangle arrays live in node-stream
// order and the scene keeps no host copy of them, so the new tree's input is made, and the arrays are re-ordered, here.
//   move_unscatter_kernel  a thread per OLD stream position q: the live vertices to an ADD-order staging array through
//                          the old tri_id, and the inverse permutation old_pos[add index] = q
//   move_overwrite_kernel  a thread per listed triangle: its 9 doubles compared BY BITS with the staged ones, written
//                          where they differ; the changed triangles counted (one integer atomicAdd per wave)
//   [the build above, from the staging array]
//   move_regather_kernel   a thread per NEW stream position p: everything of triangle a = new_tri_id[p] into new arrays
// Every index read from memory is checked against n before it is used: a thread whose index is out of range writes
// nothing (the host has checked that both tri_id are permutations; the kernels do not rely on it).

__global__ __launch_bounds__(kBuildThreads) void move_unscatter_kernel(const double *__restrict__ live_vertex,
                                                                        const int32_t *__restrict__ old_tri_id, uint32_t n,
                                                                        double *__restrict__ staged,
                                                                        int32_t *__restrict__ old_pos) {
  const uint32_t q = blockIdx.x * kBuildThreads + threadIdx.x;
  if (q >= n) return;
  const uint32_t a = (uint32_t)old_tri_id[q];
  if (a >= n) return;
  for (int k = 0; k < 9; k++) staged[(size_t)a * 9 + k] = live_vertex[(size_t)q * 9 + k];
  old_pos[a] = (int32_t)q;
}

__global__ __launch_bounds__(kBuildThreads) void move_overwrite_kernel(const int32_t *__restrict__ add_idx,
                                                                        const double *__restrict__ vertices, uint32_t n_idx,
                                                                        uint32_t n_tris, double *__restrict__ staged,
                                                                        unsigned int *__restrict__ changed) {
  const uint32_t i = blockIdx.x * kBuildThreads + threadIdx.x;
  bool differs = false;
  if (i < n_idx) {
    const uint32_t a = (uint32_t)add_idx[i];
    if (a < n_tris) {
      double v[9];
      for (int k = 0; k < 9; k++) {
        v[k] = vertices[(size_t)i * 9 + k];
        differs = differs || __double_as_longlong(v[k]) != __double_as_longlong(staged[(size_t)a * 9 + k]);
      }
      if (differs) {
        for (int k = 0; k < 9; k++) staged[(size_t)a * 9 + k] = v[k];
      }
    }
  }
  // (every lane of the wave gets here)
  const unsigned long long any = __ballot(differs);
  if (any != 0ull && (int)(threadIdx.x & 63u) == __ffsll((long long)any) - 1) atomicAdd(changed, (unsigned int)__popcll(any));
}

// the per-triangle arrays of a scene in stream order; a stamp plane that does not exist is nullptr on both sides
struct MoveArrays {
  double *vertex, *normal, *uvw, *aabb;  // 9, 9, 9, 6 per triangle
  int32_t *mtl, *line;
  uint32_t *stamp[2];
};

// was: the old arrays (read), now: the new ones (written; now.aabb has room for n boxes).  staged: the vertices in add
// order; box_add: the build's tri_aabb, add order.
__global__ __launch_bounds__(kBuildThreads) void move_regather_kernel(MoveArrays was, MoveArrays now,
                                                                       const double *__restrict__ staged,
                                                                       const double *__restrict__ box_add,
                                                                       const int32_t *__restrict__ new_tri_id,
                                                                       const int32_t *__restrict__ old_pos, uint32_t n) {
  const uint32_t p = blockIdx.x * kBuildThreads + threadIdx.x;
  if (p >= n) return;
  const uint32_t a = (uint32_t)new_tri_id[p];
  if (a >= n) return;
  const uint32_t q = (uint32_t)old_pos[a];
  if (q >= n) return;
  for (int k = 0; k < 9; k++) {
    now.vertex[(size_t)p * 9 + k] = staged[(size_t)a * 9 + k];
    now.normal[(size_t)p * 9 + k] = was.normal[(size_t)q * 9 + k];
    now.uvw[(size_t)p * 9 + k] = was.uvw[(size_t)q * 9 + k];
  }
  for (int k = 0; k < 6; k++) now.aabb[(size_t)p * 6 + k] = box_add[(size_t)a * 6 + k];
  now.mtl[p] = was.mtl[q];
  now.line[p] = was.line[q];
  for (int w = 0; w < 2; w++) {
    if (now.stamp[w] != nullptr) now.stamp[w][p] = was.stamp[w][q];
  }
}

// ---- triangles added and removed in place (mt_scene_edit_triangles): the COUNT changes, so the add order is numbered
// anew -- the survivors densely in their old relative order, then the added triangles -- and a triangle's attributes
// come from one of two sources.
//   edit_mark_kernel      a thread per listed remove index: keep[a] = 0 over a plane preset to 1
//   [rocPRIM exclusive scan of keep -> new_add: integer addition; its total is the survivor count n_keep]
//   edit_stage_kernel     a thread per OLD stream position q: a kept triangle's live vertices to staged[new_add[a]] and
//                         src[new_add[a]] = q; a thread per added triangle j: staged[n_keep + j], src[n_keep + j] = ~j
//   [the build above, from the staging array, with the new count]
//   edit_regather_kernel  a thread per NEW stream position p: everything of triangle a' = new_tri_id[p] into new arrays,
//                         the attributes from the old arrays at src[a'] or from the uploaded add arrays at ~src[a']
// src is preset to kEditNoSource, which is neither a position nor a ~j: a thread that meets it writes nothing.  As in the
// move kernels every index read from memory is checked against its bound before it is used, and no thread writes a place
// that another thread writes (remove indices are listed at most once and all write the same 0).

constexpr int32_t kEditNoSource = INT32_MIN;

__global__ __launch_bounds__(kBuildThreads) void edit_mark_kernel(const int32_t *__restrict__ remove_idx, uint32_t n_remove,
                                                                   uint32_t n_old, int32_t *__restrict__ keep) {
  const uint32_t i = blockIdx.x * kBuildThreads + threadIdx.x;
  if (i >= n_remove) return;
  const uint32_t a = (uint32_t)remove_idx[i];
  if (a >= n_old) return;
  keep[a] = 0;
}

// threads 0 .. n_old - 1: the old stream positions; threads n_old .. n_old + n_add - 1: the added triangles.  staged and
// src have room for n_keep + n_add triangles.
__global__ __launch_bounds__(kBuildThreads) void edit_stage_kernel(const double *__restrict__ live_vertex,
                                                                    const int32_t *__restrict__ old_tri_id,
                                                                    const int32_t *__restrict__ keep,
                                                                    const int32_t *__restrict__ new_add, uint32_t n_old,
                                                                    uint32_t n_keep, const double *__restrict__ add_vertex,
                                                                    uint32_t n_add, double *__restrict__ staged,
                                                                    int32_t *__restrict__ src) {
  const unsigned long long t = (unsigned long long)blockIdx.x * kBuildThreads + threadIdx.x;
  if (t < n_old) {
    const uint32_t q = (uint32_t)t;
    const uint32_t a = (uint32_t)old_tri_id[q];
    if (a >= n_old || keep[a] == 0) return;
    const uint32_t to = (uint32_t)new_add[a];
    if (to >= n_keep) return;
    for (int k = 0; k < 9; k++) staged[(size_t)to * 9 + k] = live_vertex[(size_t)q * 9 + k];
    src[to] = (int32_t)q;
  } else if (t - n_old < n_add) {
    const uint32_t j = (uint32_t)(t - n_old);
    const size_t to = (size_t)n_keep + j;
    for (int k = 0; k < 9; k++) staged[to * 9 + k] = add_vertex[(size_t)j * 9 + k];
    src[to] = ~(int32_t)j;
  }
}

// the added triangles' attributes as the caller gave them, on the device, in the order given
struct EditAdds {
  const double *normal, *uvw;  // 9, 9 per triangle
  const int32_t *mtl, *line;
};

// was: the old arrays, n_old triangles (read); add: the added triangles' attributes, n_add of them (read); now: the new
// arrays, n triangles (written; now.aabb has room for n boxes).  staged, box_add, src: in the NEW add order.
__global__ __launch_bounds__(kBuildThreads) void edit_regather_kernel(MoveArrays was, EditAdds add, MoveArrays now,
                                                                       const double *__restrict__ staged,
                                                                       const double *__restrict__ box_add,
                                                                       const int32_t *__restrict__ new_tri_id,
                                                                       const int32_t *__restrict__ src, uint32_t n,
                                                                       uint32_t n_old, uint32_t n_add) {
  const uint32_t p = blockIdx.x * kBuildThreads + threadIdx.x;
  if (p >= n) return;
  const uint32_t a = (uint32_t)new_tri_id[p];
  if (a >= n) return;
  const int32_t from = src[a];
  const bool added = from < 0;
  const uint32_t at = added ? (uint32_t)~from : (uint32_t)from;  // (kEditNoSource: 2^31 - 1, below no count)
  if (at >= (added ? n_add : n_old)) return;
  const double *normal = added ? add.normal : was.normal, *uvw = added ? add.uvw : was.uvw;
  for (int k = 0; k < 9; k++) {
    now.vertex[(size_t)p * 9 + k] = staged[(size_t)a * 9 + k];
    now.normal[(size_t)p * 9 + k] = normal[(size_t)at * 9 + k];
    now.uvw[(size_t)p * 9 + k] = uvw[(size_t)at * 9 + k];
  }
  for (int k = 0; k < 6; k++) now.aabb[(size_t)p * 6 + k] = box_add[(size_t)a * 6 + k];
  now.mtl[p] = added ? add.mtl[at] : was.mtl[at];
  now.line[p] = added ? add.line[at] : was.line[at];
  for (int w = 0; w < 2; w++) {
    if (now.stamp[w] != nullptr) now.stamp[w][p] = added ? 0u : was.stamp[w][at];
  }
}

}  // namespace mt
