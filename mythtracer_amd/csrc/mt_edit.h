// mt_edit.h — the host bookkeeping of mt_scene_edit_triangles (mt_capi.hip): the argument checks in the header's order,
// where every triangle of the edited scene comes from, and the scene's host mirrors in the new count and the new stream
// order.  Host only and free of HIP calls, like mt_move.h: tests/native/edit_check.cc checks it without a GPU.
//
// Orders: an edit numbers the ADD order anew.  The survivors come first, in their old relative order and densely --
// new index = old index - the number of removed indices below it --, then the n_add new triangles in the order given
// (numpy.delete followed by concatenate).  The tree is built over that order, so with old_pos the inverse of the old
// tri_id,
//   src[p] = old_pos[old add index of new_tri_id[p]]   for a survivor: its OLD stream position, >= 0
//   src[p] = ~j                                        for the added triangle j: negative
// is where the triangle at the new stream position p takes its attributes from -- what edit_regather_kernel (mt_build.h)
// reads through, and what the mirrors below are made by.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "mt_move.h"

namespace mt {

// the add arrays of mt_scene_edit_triangles; only add_material's values are read here
struct EditAdd {
  int n = 0;
  const void *vertex = nullptr, *normal = nullptr, *uvw = nullptr;
  const int32_t *material = nullptr;
  const void *line_no = nullptr;
};

// mt_scene_edit_triangles's checks after "scene NULL", in the header's order, all MT_ERR_ARG: a scene made without
// tri_id; a scene of zero triangles; n_remove negative or greater than n_tris; n_add negative; remove_idx NULL with
// n_remove > 0; a missing add array with n_add > 0 (vertex, normal, uvw, material, line_no); a remove index outside
// 0 .. n_tris - 1; a remove index listed twice; a resulting count below 1 or above what an int32 holds; an add_material
// outside -1 .. n_materials - 1.
inline bool check_edit_args(bool have_tri_id, int n_tris, const int32_t *remove_idx, int n_remove, const EditAdd &add,
                            int n_materials, MoveError *err) {
  if (!have_tri_id) return move_refuse(err, MT_ERR_ARG, "the scene was made without tri_id");
  if (n_tris < 1) return move_refuse(err, MT_ERR_ARG, "a scene of %d triangles cannot be edited", n_tris);
  if (n_remove < 0 || n_remove > n_tris) {
    return move_refuse(err, MT_ERR_ARG, "%d triangles to remove from a scene of %d", n_remove, n_tris);
  }
  if (add.n < 0) return move_refuse(err, MT_ERR_ARG, "%d triangles to add", add.n);
  if (n_remove > 0 && !remove_idx) return move_refuse(err, MT_ERR_ARG, "the remove list is NULL");
  if (add.n > 0) {
    if (!add.vertex) return move_refuse(err, MT_ERR_ARG, "the added triangles' vertex array is NULL");
    if (!add.normal) return move_refuse(err, MT_ERR_ARG, "the added triangles' normal array is NULL");
    if (!add.uvw) return move_refuse(err, MT_ERR_ARG, "the added triangles' uvw array is NULL");
    if (!add.material) return move_refuse(err, MT_ERR_ARG, "the added triangles' material array is NULL");
    if (!add.line_no) return move_refuse(err, MT_ERR_ARG, "the added triangles' line_no array is NULL");
  }
  for (int i = 0; i < n_remove; i++) {
    if (remove_idx[i] < 0 || remove_idx[i] >= n_tris) {
      return move_refuse(err, MT_ERR_ARG, "entry %d: remove index %d outside 0..%d", i, remove_idx[i], n_tris - 1);
    }
  }
  std::vector<bool> seen((size_t)n_tris, false);
  for (int i = 0; i < n_remove; i++) {
    if (seen[(size_t)remove_idx[i]]) return move_refuse(err, MT_ERR_ARG, "remove index %d is listed twice", remove_idx[i]);
    seen[(size_t)remove_idx[i]] = true;
  }
  const long long count = (long long)n_tris - (long long)n_remove + (long long)add.n;
  if (count < 1 || count > 0x7fffffffll) {
    return move_refuse(err, MT_ERR_ARG, "the edit leaves %lld triangles: a scene holds 1..%d", count, 0x7fffffff);
  }
  for (int j = 0; j < add.n; j++) {
    const int m = add.material[j];
    if (m < -1 || m >= n_materials) {
      return move_refuse(err, MT_ERR_ARG, "triangle %d: material index %d outside -1..%d", j, m, n_materials - 1);
    }
  }
  return true;
}

// src[p] for every new stream position p (above).  False (MT_ERR_ARG) unless the old tri_id is a permutation of
// 0 .. n_old - 1, the remove list holds indices of that range at most once, and the new tri_id is a permutation of
// 0 .. n_new - 1 with n_new = n_old - n_remove + n_add.
inline bool compose_edit(const int32_t *old_tri_id, size_t n_old, const int32_t *remove_idx, size_t n_remove, size_t n_add,
                         const int32_t *new_tri_id, size_t n_new, std::vector<int32_t> *src, MoveError *err) {
  if (n_remove > n_old || n_new != n_old - n_remove + n_add) {
    return move_refuse(err, MT_ERR_ARG, "%zu - %zu + %zu triangles are not %zu", n_old, n_remove, n_add, n_new);
  }
  std::vector<int32_t> old_pos(n_old, -1);
  for (size_t q = 0; q < n_old; q++) {
    const int32_t a = old_tri_id[q];
    if (a < 0 || (size_t)a >= n_old || old_pos[(size_t)a] >= 0) {
      return move_refuse(err, MT_ERR_ARG, "the old tri_id is no permutation (position %zu: %d)", q, a);
    }
    old_pos[(size_t)a] = (int32_t)q;
  }
  std::vector<bool> removed(n_old, false);
  for (size_t i = 0; i < n_remove; i++) {
    const int32_t a = remove_idx[i];
    if (a < 0 || (size_t)a >= n_old || removed[(size_t)a]) {
      return move_refuse(err, MT_ERR_ARG, "the remove list is no list of distinct triangles (entry %zu: %d)", i, a);
    }
    removed[(size_t)a] = true;
  }
  const size_t n_keep = n_old - n_remove;
  std::vector<int32_t> by_add(n_new);  // new add index -> source
  size_t next = 0;
  for (size_t a = 0; a < n_old; a++) {
    if (!removed[a]) by_add[next++] = old_pos[a];
  }
  for (size_t j = 0; j < n_add; j++) by_add[n_keep + j] = ~(int32_t)j;
  src->assign(n_new, 0);
  std::vector<bool> seen(n_new, false);
  for (size_t p = 0; p < n_new; p++) {
    const int32_t a = new_tri_id[p];
    if (a < 0 || (size_t)a >= n_new || seen[(size_t)a]) {
      return move_refuse(err, MT_ERR_ARG, "the new tri_id is no permutation (position %zu: %d)", p, a);
    }
    seen[(size_t)a] = true;
    (*src)[p] = by_add[(size_t)a];
  }
  return true;
}

// a per-triangle mirror in the new count and order: a survivor's entry, or `fresh` for an added triangle; an EMPTY
// mirror (a stamp plane no set has made yet) stays empty
template <typename T, typename Fresh>
inline std::vector<T> edit_mirror(const std::vector<T> &was, const std::vector<int32_t> &src, Fresh fresh) {
  std::vector<T> now;
  if (was.empty()) return now;
  now.resize(src.size());
  for (size_t p = 0; p < src.size(); p++) now[p] = src[p] >= 0 ? was[(size_t)src[p]] : fresh((size_t)~src[p]);
  return now;
}

// The scene's mirrors after an edit, built aside like a move's (MovedMirrors): the new tri_id, the assignment -- a NEW
// vector, the ray trees share the old one -- with the added triangles' materials, and the two stamp planes, where an
// added triangle's stamp is 0.
inline bool edit_mirrors(const std::vector<int32_t> &old_tri_id, const int32_t *remove_idx, size_t n_remove, size_t n_add,
                         const int32_t *add_material, const int32_t *new_tri_id, size_t n_new,
                         const std::vector<int32_t> &tri_mtl, const std::vector<uint32_t> stamp[2], MovedMirrors *out,
                         std::vector<int32_t> *src, MoveError *err) {
  const size_t n = old_tri_id.size();
  if (tri_mtl.size() != n || (!stamp[0].empty() && stamp[0].size() != n) || (!stamp[1].empty() && stamp[1].size() != n)) {
    return move_refuse(err, MT_ERR_ARG, "the mirrors do not have the scene's %zu triangles", n);
  }
  if (!compose_edit(old_tri_id.data(), n, remove_idx, n_remove, n_add, new_tri_id, n_new, src, err)) return false;
  out->tri_id.assign(new_tri_id, new_tri_id + n_new);
  out->tri_mtl.resize(n_new);  // (never empty: a scene has an assignment)
  for (size_t p = 0; p < n_new; p++) {
    out->tri_mtl[p] = (*src)[p] >= 0 ? tri_mtl[(size_t)(*src)[p]] : add_material[(size_t)~(*src)[p]];
  }
  for (int w = 0; w < 2; w++) out->stamp[w] = edit_mirror(stamp[w], *src, [](size_t) { return 0u; });
  return true;
}

}  // namespace mt
