// mt_layout.h — what the host derives from a flattened scene (mt_scene_desc) before anything is uploaded: the checks
// that let the kernels index it without bounds checks, and every array the hit-set walk reads (mt_device.h), with the
// paddings its scans look ahead into.  Host only and free of HIP calls: mt_capi.hip uploads a SceneLayout as it stands,
// and tests/native/layout_check.cc checks one without a GPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "mt_device.h"
#include "mt_shadow_bound.h"

namespace mt {

// Why a desc is refused: the MT_ERR_* code and the text for mt_last_error.
struct LayoutError {
  int code = MT_OK;
  std::string msg;
};

inline bool refuse(LayoutError *err, int code, const char *fmt, ...) {
  char text[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(text, sizeof text, fmt, ap);
  va_end(ap);
  err->code = code;
  err->msg = text;
  return false;
}

// a texture's size and format (mt_scene_create, mt_scene_set_texture)
inline bool check_texture(const mt_texture &t, int i, LayoutError *err) {
  if (t.width <= 0 || t.height <= 0 || t.width > 30000 || t.height > 30000 || !t.texels ||
      (t.format != MT_TEX_RGB8 && t.format != MT_TEX_F64)) {
    return refuse(err, MT_ERR_ARG, "texture %d: bad size/format", i);
  }
  return true;
}

// True when the kernels may index the scene unchecked; else false and *err.  depth_of: every node's level, root = 1.
inline bool check_scene_desc(const mt_scene_desc &d, std::vector<int> *depth_of, int *max_depth, LayoutError *err) {
  if (d.struct_size != sizeof(mt_scene_desc) || d.abi_version != MT_ABI_VERSION) {
    return refuse(err, MT_ERR_ARG, "mt_scene_desc size/version mismatch (%u/%u, want %zu/%d)",
                  d.struct_size, d.abi_version, sizeof(mt_scene_desc), MT_ABI_VERSION);
  }
  if (d.n_nodes < 1 || d.n_tris < 0 || d.n_materials < 0 || d.n_textures < 0) {
    return refuse(err, MT_ERR_ARG, "negative or empty counts");
  }
  if (!d.node_aabb || !d.node_center || !d.node_first_child || !d.node_prim_begin || !d.node_prim_count) {
    return refuse(err, MT_ERR_ARG, "node arrays missing");
  }
  if (d.n_tris > 0 && (!d.tri_vertex || !d.tri_normal || !d.tri_uvw || !d.tri_aabb || !d.tri_material ||
                       !d.tri_line_no)) {
    return refuse(err, MT_ERR_ARG, "triangle arrays missing");
  }
  if ((d.n_materials > 0 && !d.materials) || (d.n_textures > 0 && !d.textures)) {
    return refuse(err, MT_ERR_ARG, "material/texture arrays missing");
  }
  // --- structural validation: the kernel indexes all of this unchecked.
  const int nn = d.n_nodes;
  depth_of->assign((size_t)nn, 0);
  std::vector<int> &depth = *depth_of;
  depth[0] = 1;
  *max_depth = 1;
  long long prim_total = 0;
  for (int i = 0; i < nn; i++) {
    const int fc = d.node_first_child[i];
    const int pb = d.node_prim_begin[i], pc = d.node_prim_count[i];
    if (pb < 0 || pc < 0 || (long long)pb + pc > d.n_tris) {
      return refuse(err, MT_ERR_ARG, "node %d: primitive range [%d,+%d) outside 0..%d", i, pb, pc, d.n_tris);
    }
    prim_total += pc;
    if (depth[i] == 0) return refuse(err, MT_ERR_ARG, "node %d is not reachable in BFS order", i);
    if (fc != 0) {
      if (fc <= i || (long long)fc + 8 > nn) {
        return refuse(err, MT_ERR_ARG, "node %d: first_child %d invalid (n_nodes %d)", i, fc, nn);
      }
      for (int k = 0; k < 8; k++) {
        if (depth[fc + k] != 0) return refuse(err, MT_ERR_ARG, "node %d has two parents", fc + k);
        depth[fc + k] = depth[i] + 1;
      }
      if (depth[i] + 1 > *max_depth) *max_depth = depth[i] + 1;
    }
  }
  if (prim_total != d.n_tris) {
    return refuse(err, MT_ERR_ARG, "nodes reference %lld primitives, scene has %d", prim_total, d.n_tris);
  }
  if (*max_depth > MT_MAX_TREE_DEPTH) {
    return refuse(err, MT_ERR_UNSUPPORTED, "octree depth %d exceeds MT_MAX_TREE_DEPTH %d", *max_depth,
                  MT_MAX_TREE_DEPTH);
  }
  for (int i = 0; i < d.n_tris; i++) {
    const int m = d.tri_material[i];
    if (m < -1 || m >= d.n_materials) {
      return refuse(err, MT_ERR_ARG, "triangle %d: material index %d outside -1..%d", i, m, d.n_materials - 1);
    }
  }
  for (int i = 0; i < d.n_materials; i++) {
    const int t = d.materials[i].tex;
    if (t < -1 || t >= d.n_textures) {
      return refuse(err, MT_ERR_ARG, "material %d: texture index %d outside -1..%d", i, t, d.n_textures - 1);
    }
  }
  for (int i = 0; i < d.n_textures; i++) {
    if (!check_texture(d.textures[i], i, err)) return false;
  }
  return true;
}

// One vector per array of DevScene that the host derives (the name of the DevScene member where it differs).
struct SceneLayout {
  std::vector<NodeRec> recs;        // nodes
  std::vector<float> groups;        // grp_aabb32
  std::vector<float> supers;        // sup_aabb32
  std::vector<float> subs;          // sub_aabb32
  std::vector<HsRec> hsr;           // hs_rec
  std::vector<float> sl_box;        // sl_box32
  std::vector<int32_t> ll_tri;
  std::vector<double> ll_exact;
  std::vector<float> ll_box_q, ll_grp_q, ll_sup_q;
  std::vector<double> tri_aabb;
  std::vector<float> tri_aabb32;
  double bmax[3] = {0.0, 0.0, 0.0};
  bool regular = false;             // scene_regular
  ShadowBound shadow{1.0f, 0.0f, 0.0f, 0};  // sb (mt_shadow_bound.h): on = 0 unless the scene is eligible
  int max_depth = 0;                // tree_depth
};

// ---- boxes of six: lo xyz, hi xyz

// The box of an empty set: every ray misses it, and a union that starts from it is the union of the rest.
constexpr double kInvertedBox[6] = {3.0e38, 3.0e38, 3.0e38, -3.0e38, -3.0e38, -3.0e38};
static_assert((float)3.0e38 == 3.0e38f, "the fp32 inverted box is the rounded fp64 one");

template <typename T>
inline void box_invert(T *u) {
  for (int k = 0; k < 6; k++) u[k] = (T)kInvertedBox[k];
}

// u becomes the union of u and the n boxes at b
template <typename T>
inline void box_union(T *u, const T *b, size_t n = 1) {
  for (size_t j = 0; j < n; j++, b += 6) {
    for (int k = 0; k < 3; k++) {
      u[k] = std::min(u[k], b[k]);
      u[3 + k] = std::max(u[3 + k], b[3 + k]);
    }
  }
}

// Appends the n boxes at `boxes`, rounded to fp32, as quads in the layout of DevScene::sl_box32: per four boxes
// kSlQuadFloats floats = per axis [lo x 4][hi x 4][lo x 4], the last quad filled up with inverted boxes.
template <typename T>
inline void append_quads(const T *boxes, size_t n, std::vector<float> *out) {
  const size_t at = out->size();
  out->resize(at + ((n + 3) / 4) * (size_t)kSlQuadFloats, 0.0f);
  for (size_t i = 0; i < ((n + 3) / 4) * 4; i++) {
    for (int a = 0; a < 3; a++) {
      const float lo = i < n ? (float)boxes[i * 6 + a] : (float)kInvertedBox[a];
      const float hi = i < n ? (float)boxes[i * 6 + 3 + a] : (float)kInvertedBox[3 + a];
      float *q = out->data() + at + (i / 4) * kSlQuadFloats + (size_t)a * 12 + (i & 3);
      q[0] = lo;
      q[4] = hi;
      q[8] = lo;
    }
  }
}

// ---- the arrays, one family each

inline void derive_node_records(const mt_scene_desc &d, const std::vector<int> &depth_of, std::vector<NodeRec> *recs) {
  recs->resize((size_t)d.n_nodes);
  for (int i = 0; i < d.n_nodes; i++) {
    NodeRec &r = (*recs)[(size_t)i];
    memset(&r, 0, sizeof r);
    for (int k = 0; k < 3; k++) {
      r.lo[k] = d.node_aabb[i * 6 + k];
      r.hi[k] = d.node_aabb[i * 6 + 3 + k];
      r.c[k] = d.node_center[i * 3 + k];
    }
    r.first_child = d.node_first_child[i];
    r.prim_begin = d.node_prim_begin[i];
    r.prim_count = d.node_prim_count[i];
    r.level = depth_of[(size_t)i] - 1;
  }
}

// Block boxes (mt_device.h kGroupTris): union of the fp64 boxes of each block of kGroupTris consecutive stream
// triangles, then rounded to fp32 exactly like the per-triangle copies (the filter's margin covers it).
// Second level (mt_device.h kSuperBlocks): one fp32 union box per kSuperBlocks consecutive blocks, for the long lists.
inline void derive_block_boxes(const mt_scene_desc &d, std::vector<float> *groups, std::vector<float> *supers) {
  for (int t0 = 0; t0 < d.n_tris; t0 += kGroupTris) {
    const int e = std::min(t0 + kGroupTris, d.n_tris);
    double u[6];
    for (int k = 0; k < 6; k++) u[k] = d.tri_aabb[(size_t)t0 * 6 + k];
    box_union(u, d.tri_aabb + (size_t)(t0 + 1) * 6, (size_t)(e - t0 - 1));
    for (int k = 0; k < 6; k++) groups->push_back((float)u[k]);
  }
  const size_t nblk = groups->size() / 6;
  for (size_t b = 0; b < nblk; b += kSuperBlocks) {
    float u[6];
    for (int k = 0; k < 6; k++) u[k] = (*groups)[b * 6 + k];
    box_union(u, groups->data() + (b + 1) * 6, std::min(b + (size_t)kSuperBlocks, nblk) - b - 1);
    for (int k = 0; k < 6; k++) supers->push_back(u[k]);
  }
  supers->resize(supers->size() + 8 * 6, 0.0f);  // look-ahead padding
  groups->resize(groups->size() + 8 * 6, 0.0f);  // the scan looks four boxes ahead
}

// Subtree boxes (mt_trace.h tight_keep_mask): union of the fp64 boxes of all triangles stored in a node or below it,
// rounded to fp32 like the others.  Breadth-first order: children have larger indices than their parent.  An empty
// subtree gets an inverted box, which every ray misses.  Sets NodeRec::child_mask.
inline void derive_subtree_boxes(const mt_scene_desc &d, std::vector<NodeRec> *recs, std::vector<float> *subs) {
  const int nn = d.n_nodes;
  subs->assign((size_t)nn * 6 + 8 * 6, 0.0f);
  std::vector<double> sb((size_t)nn * 6);
  for (int i = nn - 1; i >= 0; i--) {
    double *u = &sb[(size_t)i * 6];
    NodeRec &r = (*recs)[(size_t)i];
    box_invert(u);
    if (r.prim_count > 0) box_union(u, d.tri_aabb + (size_t)r.prim_begin * 6, (size_t)r.prim_count);
    if (r.first_child != 0) {
      box_union(u, &sb[(size_t)r.first_child * 6], 8);
      int mask = 0;
      for (int c = 0; c < 8; c++) {
        const double *b = &sb[(size_t)(r.first_child + c) * 6];
        if (b[0] <= b[3]) mask |= 1 << c;  // an empty subtree keeps the inverted box
      }
      r.child_mask = mask;
    }
    for (int k = 0; k < 6; k++) (*subs)[(size_t)i * 6 + k] = (float)u[k];
  }
}

// Records of the hit-set traversal (mt_device.h HsRec), one more than nodes (the last all zero), and the short lists'
// boxes as quads (DevScene::sl_box32).  ll_begin is -1 here: derive_long_lists sets it.
inline void derive_hit_set_records(const mt_scene_desc &d, const std::vector<NodeRec> &recs,
                                   const std::vector<float> &subs, std::vector<HsRec> *hsr,
                                   std::vector<float> *sl_box) {
  const int nn = d.n_nodes;
  hsr->resize((size_t)nn + 1);
  memset(hsr->data(), 0, hsr->size() * sizeof(HsRec));
  for (int i = 0; i < nn; i++) {
    HsRec &h = (*hsr)[(size_t)i];
    const NodeRec &r = recs[(size_t)i];
    h.first_child = r.first_child;
    h.prim_begin = r.prim_begin;
    h.prim_count = r.prim_count;
    h.child_mask = r.first_child != 0 ? (r.child_mask & 0xff) : 0;
    for (int c = 0; c < 8; c++) {
      const float *kid = r.first_child != 0 ? &subs[(size_t)(r.first_child + c) * 6] : nullptr;
      for (int a = 0; a < 3; a++) {
        h.kid[a][c] = h.kid[a][16 + c] = kid ? kid[a] : (float)kInvertedBox[a];
        h.kid[a][8 + c] = kid ? kid[3 + a] : (float)kInvertedBox[3 + a];
      }
    }
    double u[6];
    box_invert(u);
    if (r.prim_count > 0) box_union(u, d.tri_aabb + (size_t)r.prim_begin * 6, (size_t)r.prim_count);
    for (int a = 0; a < 3; a++) {
      h.own[a][0] = h.own[a][2] = (float)u[a];
      h.own[a][1] = (float)u[3 + a];
    }
    h.sl_begin = h.ll_begin = -1;
    if (r.prim_count >= 1 && r.prim_count <= kHsShortList) {
      h.sl_begin = (int32_t)(sl_box->size() / kSlQuadFloats);
      append_quads(d.tri_aabb + (size_t)r.prim_begin * 6, (size_t)r.prim_count, sl_box);
    }
    for (int k = 0; k < 3; k++) {
      h.planes[k] = r.lo[k];
      h.planes[3 + k] = r.c[k];
      h.planes[6 + k] = r.hi[k];
    }
  }
  sl_box->resize(sl_box->size() + 2 * kSlQuadFloats, 0.0f);  // (the copies are whole 16-byte pieces; never empty)
}

// The triangles [pb, pb + pc) in the order of a median-split tree over their boxes' centres, cut on the longest axis of
// the centres' extent at a multiple of 64 (16 below 64) entries, so that 16 consecutive entries -- one block box --
// and 64 -- one super box -- are spatial neighbours.
inline void sort_long_list(const mt_scene_desc &d, int pb, int pc, std::vector<int32_t> *order_out) {
  std::vector<int32_t> &order = *order_out;
  order.resize((size_t)pc);
  for (int k = 0; k < pc; k++) order[(size_t)k] = pb + k;
  // iterative median split over [lo, hi) of `order`
  std::vector<std::pair<int, int>> todo{{0, pc}};
  while (!todo.empty()) {
    const int lo = todo.back().first, hi = todo.back().second;
    todo.pop_back();
    const int n = hi - lo;
    if (n <= 16) continue;
    double cmin[3] = {1e300, 1e300, 1e300}, cmax[3] = {-1e300, -1e300, -1e300};
    for (int k = lo; k < hi; k++) {
      const double *b = d.tri_aabb + (size_t)order[(size_t)k] * 6;
      for (int a = 0; a < 3; a++) {
        const double c = b[a] * 0.5 + b[3 + a] * 0.5;
        cmin[a] = std::min(cmin[a], c);
        cmax[a] = std::max(cmax[a], c);
      }
    }
    int ax = 0;
    for (int a = 1; a < 3; a++) {
      if (cmax[a] - cmin[a] > cmax[ax] - cmin[ax]) ax = a;
    }
    const int unit = n > 64 ? 64 : 16;
    int left = ((n / 2 + unit - 1) / unit) * unit;
    if (left >= n) left = n - (n % unit ? n % unit : unit);
    if (left <= 0 || left >= n) continue;
    auto key = [&](int32_t t) {
      const double *b = d.tri_aabb + (size_t)t * 6;
      return b[ax] * 0.5 + b[3 + ax] * 0.5;
    };
    std::nth_element(order.begin() + lo, order.begin() + lo + left, order.begin() + hi,
                     [&](int32_t x, int32_t y) { const double kx = key(x), ky = key(y); return kx < ky || (kx == ky && x < y); });
    todo.push_back({lo, lo + left});
    todo.push_back({lo + left, hi});
  }
}

// Spatially sorted copies of the long lists (DevScene::ll_*), every list padded to a multiple of kLlPad: the triangle
// of every entry (-1: padding), its fp64 box and vertices (zeros), and in ll_box its fp32 box (inverted).
inline void derive_long_lists(const mt_scene_desc &d, std::vector<HsRec> *hsr, std::vector<int32_t> *ll_tri,
                              std::vector<double> *ll_exact, std::vector<float> *ll_box) {
  std::vector<int32_t> order;
  for (int i = 0; i < d.n_nodes; i++) {
    HsRec &h = (*hsr)[(size_t)i];
    const int pc = h.prim_count;
    if (pc <= kHsShortList) continue;
    sort_long_list(d, h.prim_begin, pc, &order);
    h.ll_begin = (int32_t)ll_tri->size();
    const int padded = ((pc + kLlPad - 1) / kLlPad) * kLlPad;
    for (int k = 0; k < padded; k++) {
      if (k < pc) {
        const int32_t t = order[(size_t)k];
        ll_tri->push_back(t);
        for (int q = 0; q < 6; q++) ll_box->push_back((float)d.tri_aabb[(size_t)t * 6 + q]);
        for (int q = 0; q < 6; q++) ll_exact->push_back(d.tri_aabb[(size_t)t * 6 + q]);
        for (int q = 0; q < 9; q++) ll_exact->push_back(d.tri_vertex[(size_t)t * 9 + q]);
      } else {
        ll_tri->push_back(-1);
        for (int q = 0; q < 6; q++) ll_box->push_back((float)kInvertedBox[q]);
        for (int q = 0; q < 15; q++) ll_exact->push_back(0.0);
      }
    }
  }
  ll_tri->resize(ll_tri->size() + 64, -1);  // (never empty)
  ll_exact->resize(ll_exact->size() + 15, 0.0);
}

// One union box per `per` consecutive boxes of src; padding (inverted) boxes do not count.
inline std::vector<float> box_unions(const std::vector<float> &src, size_t per) {
  std::vector<float> dst;
  const size_t n = src.size() / 6;
  for (size_t b = 0; b < n; b += per) {
    float u[6];
    box_invert(u);
    for (size_t j = b; j < std::min(b + per, n); j++) {
      if (!(src[j * 6] <= src[j * 6 + 3])) continue;  // padding (inverted)
      box_union(u, &src[j * 6]);
    }
    dst.insert(dst.end(), u, u + 6);
  }
  return dst;
}

// The long lists' three levels as quads for the walk's per-lane reads (DevScene::ll_*_q; layout of sl_box32): the
// entries' boxes, a union per 16 entries (block) and per 64 (super), each followed by one quad of zeros.
inline void derive_long_list_quads(const std::vector<float> &ll_box, SceneLayout *L) {
  const std::vector<float> ll_grp = box_unions(ll_box, 16), ll_sup = box_unions(ll_grp, 4);
  const std::vector<float> *src[3] = {&ll_box, &ll_grp, &ll_sup};
  std::vector<float> *dst[3] = {&L->ll_box_q, &L->ll_grp_q, &L->ll_sup_q};
  for (int k = 0; k < 3; k++) {
    append_quads(src[k]->data(), src[k]->size() / 6, dst[k]);
    dst[k]->resize(dst[k]->size() + kSlQuadFloats, 0.0f);
  }
}

// The triangles' boxes with the scans' look-ahead behind them, their fp32 copy, and the largest |coordinate| per axis.
inline void derive_triangle_boxes(const mt_scene_desc &d, SceneLayout *L) {
  const size_t nt = (size_t)d.n_tris;
  // The scan loop looks two boxes ahead (mt_trace.h): pad the stream.
  L->tri_aabb.assign(nt * 6 + 4 * 6, 0.0);
  if (nt) memcpy(L->tri_aabb.data(), d.tri_aabb, nt * 6 * sizeof(double));
  // fp32 copy for the conservative pre-filter (mt_trace.h Filter32); padded by 8 boxes because that loop looks four
  // boxes ahead.
  L->tri_aabb32.assign(nt * 6 + 64 * 6, 0.0f);  // (padding: the look-ahead of the scans; the hit-set traversal copies whole 16-byte pieces)
  double bmax[3] = {0.0, 0.0, 0.0};
  for (size_t i = 0; i < nt * 6; i++) {
    L->tri_aabb32[i] = (float)L->tri_aabb[i];
    const double a = std::fabs(L->tri_aabb[i]);
    if (a > bmax[i % 3]) bmax[i % 3] = a;
  }
  // Never below 2^-7: make_filter32's check M = (bmax + |o|) |1/d| <= 2^120 then bounds |1/d| by 2^127 as well, the
  // range in which its fp32 copy is finite (mt_trace.h, Filter32's preconditions).
  for (int k = 0; k < 3; k++) L->bmax[k] = std::max(bmax[k], 0x1p-7);
}

inline bool all_finite(const double *p, size_t n) {
  for (size_t i = 0; i < n; i++) {
    if (!std::isfinite(p[i])) return false;
  }
  return true;
}

// Is the min/max-instruction path admissible for this scene?  All coordinates finite, boxes ordered, an inner node's
// centre inside its box.
inline bool scene_regular(const mt_scene_desc &d) {
  const int nn = d.n_nodes;
  bool regular = all_finite(d.node_aabb, (size_t)nn * 6) && all_finite(d.node_center, (size_t)nn * 3) &&
                 all_finite(d.tri_aabb, (size_t)d.n_tris * 6);
  for (int i = 0; regular && i < nn; i++) {
    for (int k = 0; k < 3; k++) {
      const double lo = d.node_aabb[i * 6 + k], hi = d.node_aabb[i * 6 + 3 + k];
      const double c = d.node_center[i * 3 + k];
      if (!(lo <= hi)) regular = false;
      if (d.node_first_child[i] != 0 && !(lo <= c && c <= hi)) regular = false;
    }
  }
  for (int i = 0; regular && i < d.n_tris; i++) {
    for (int k = 0; k < 3; k++) {
      if (!(d.tri_aabb[i * 6 + k] <= d.tri_aabb[i * 6 + 3 + k])) regular = false;
    }
  }
  return regular;
}

// Everything of a checked desc (check_scene_desc, which gives depth_of) that the kernels read besides the caller's
// own arrays.
inline void derive_layout(const mt_scene_desc &d, const std::vector<int> &depth_of, SceneLayout *out) {
  SceneLayout &L = *out;
  L = SceneLayout();
  L.regular = scene_regular(d);
  L.max_depth = *std::max_element(depth_of.begin(), depth_of.end());
  derive_node_records(d, depth_of, &L.recs);
  derive_block_boxes(d, &L.groups, &L.supers);
  derive_subtree_boxes(d, &L.recs, &L.subs);
  derive_hit_set_records(d, L.recs, L.subs, &L.hsr, &L.sl_box);
  std::vector<float> ll_box;
  derive_long_lists(d, &L.hsr, &L.ll_tri, &L.ll_exact, &ll_box);
  derive_long_list_quads(ll_box, &L);
  derive_triangle_boxes(d, &L);
  if (L.regular) {
    const ShadowBoundInput in{d.n_nodes, d.n_tris, d.node_aabb, d.node_center, d.node_first_child, d.node_prim_begin,
                              d.node_prim_count, d.tri_vertex, d.tri_aabb};
    L.shadow = shadow_bound_for(in);
  }
}

}  // namespace mt
