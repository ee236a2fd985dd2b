// mt_move.h — the host bookkeeping of mt_scene_set_triangle_vertices (mt_capi.hip): the checks on the list of moved
// triangles, and what the scene's host mirrors become when the node-stream order changes from the old tree's to the new
// tree's.  Host only and free of HIP calls: tests/native/move_check.cc checks it without a GPU.
//
// Orders: a tri_id maps a STREAM position to the triangle's ADD index (mt_scene_desc::tri_id).  A move rebuilds the tree,
// so the same add indices come in another stream order.  With old_pos = the inverse of the old tri_id,
//   from[p] = old_pos[new_tri_id[p]]
// is the OLD stream position of the triangle that now sits at position p: what move_regather_kernel (mt_build.h) reads
// its per-triangle attributes through, and what the mirrors below are permuted by.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "mythtracer_hip.h"

namespace mt {

// Why a move is refused: the MT_ERR_* code and the text for mt_last_error.
struct MoveError {
  int code = MT_OK;
  std::string msg;
};

inline bool move_refuse(MoveError *err, int code, const char *fmt, ...) {
  char text[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(text, sizeof text, fmt, ap);
  va_end(ap);
  err->code = code;
  err->msg = text;
  return false;
}

// mt_scene_set_triangle_vertices's checks after "scene NULL", in the header's order, all MT_ERR_ARG: a scene made without
// tri_id; n_idx negative or greater than n_tris; add_idx or vertices NULL with n_idx > 0; an index outside
// 0 .. n_tris - 1; an index listed twice.
inline bool check_move_list(bool have_tri_id, int n_tris, const int32_t *add_idx, int n_idx, const void *vertices,
                            MoveError *err) {
  if (!have_tri_id) return move_refuse(err, MT_ERR_ARG, "the scene was made without tri_id");
  if (n_idx < 0 || n_idx > n_tris) {
    return move_refuse(err, MT_ERR_ARG, "%d listed triangles for a scene of %d", n_idx, n_tris);
  }
  if (n_idx > 0 && !add_idx) return move_refuse(err, MT_ERR_ARG, "the index list is NULL");
  if (n_idx > 0 && !vertices) return move_refuse(err, MT_ERR_ARG, "the vertex array is NULL");
  for (int i = 0; i < n_idx; i++) {
    if (add_idx[i] < 0 || add_idx[i] >= n_tris) {
      return move_refuse(err, MT_ERR_ARG, "entry %d: add index %d outside 0..%d", i, add_idx[i], n_tris - 1);
    }
  }
  std::vector<bool> seen((size_t)n_tris, false);
  for (int i = 0; i < n_idx; i++) {
    if (seen[(size_t)add_idx[i]]) return move_refuse(err, MT_ERR_ARG, "add index %d is listed twice", add_idx[i]);
    seen[(size_t)add_idx[i]] = true;
  }
  return true;
}

// mt_scene_get_triangle_vertices's checks after "scene NULL"
inline bool check_move_get(bool have_tri_id, int scene_tris, const void *out, int n_tris, MoveError *err) {
  if (!have_tri_id) return move_refuse(err, MT_ERR_ARG, "the scene was made without tri_id");
  if (n_tris != scene_tris) return move_refuse(err, MT_ERR_ARG, "%d triangles for a scene made with %d", n_tris, scene_tris);
  if (n_tris > 0 && !out) return move_refuse(err, MT_ERR_ARG, "the output array is NULL");
  return true;
}

// from[p] = old stream position of the triangle at new stream position p.  False (MT_ERR_ARG) unless both arrays are
// permutations of 0 .. n - 1 -- which a tree built over the scene's own triangles always gives.
inline bool compose_move(const int32_t *old_tri_id, const int32_t *new_tri_id, size_t n, std::vector<int32_t> *from,
                         MoveError *err) {
  std::vector<int32_t> old_pos(n, -1);
  for (size_t q = 0; q < n; q++) {
    const int32_t a = old_tri_id[q];
    if (a < 0 || (size_t)a >= n || old_pos[(size_t)a] >= 0) {
      return move_refuse(err, MT_ERR_ARG, "the old tri_id is no permutation (position %zu: %d)", q, a);
    }
    old_pos[(size_t)a] = (int32_t)q;
  }
  from->assign(n, -1);
  std::vector<bool> seen(n, false);
  for (size_t p = 0; p < n; p++) {
    const int32_t a = new_tri_id[p];
    if (a < 0 || (size_t)a >= n || seen[(size_t)a]) {
      return move_refuse(err, MT_ERR_ARG, "the new tri_id is no permutation (position %zu: %d)", p, a);
    }
    seen[(size_t)a] = true;
    (*from)[p] = old_pos[(size_t)a];
  }
  return true;
}

// a per-triangle mirror in the new order; an EMPTY mirror (a stamp plane no set has made yet: every stamp is 0) stays empty
template <typename T>
inline std::vector<T> permute_mirror(const std::vector<T> &was, const std::vector<int32_t> &from) {
  std::vector<T> now;
  if (was.empty()) return now;
  now.resize(from.size());
  for (size_t p = 0; p < from.size(); p++) now[p] = was[(size_t)from[p]];
  return now;
}

// The scene's mirrors after a move: the new tri_id, the assignment and the two attribute stamp planes, all in the new
// stream order.  Built aside; the caller swaps them in once nothing can fail any more.
struct MovedMirrors {
  std::vector<int32_t> tri_id;
  std::vector<int32_t> tri_mtl;
  std::vector<uint32_t> stamp[2];
};

inline bool move_mirrors(const std::vector<int32_t> &old_tri_id, const int32_t *new_tri_id, const std::vector<int32_t> &tri_mtl,
                         const std::vector<uint32_t> stamp[2], MovedMirrors *out, std::vector<int32_t> *from, MoveError *err) {
  const size_t n = old_tri_id.size();
  if (tri_mtl.size() != n || (!stamp[0].empty() && stamp[0].size() != n) || (!stamp[1].empty() && stamp[1].size() != n)) {
    return move_refuse(err, MT_ERR_ARG, "the mirrors do not have the scene's %zu triangles", n);
  }
  if (!compose_move(old_tri_id.data(), new_tri_id, n, from, err)) return false;
  out->tri_id.assign(new_tri_id, new_tri_id + n);
  out->tri_mtl = permute_mirror(tri_mtl, *from);
  for (int w = 0; w < 2; w++) out->stamp[w] = permute_mirror(stamp[w], *from);
  return true;
}

}  // namespace mt
