// move_check.cc — mt_move.h without a GPU: the index-list refusals of mt_scene_set_triangle_vertices in their order,
// and the permutation of the scene's host mirrors from (old tri_id, new tri_id), against brute-force restatements
// written out here (searches, not inverse tables).  Driven by tests/test_move_cpu.py, which builds it with the address
// and undefined-behaviour sanitizers.  Exit status 0 = every check held; else the failing cases on stderr.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mt_move.h"

using namespace mt;

namespace {

int g_failures = 0;
std::string g_case;

#define CHECK(cond, ...)                                          \
  do {                                                            \
    if (!(cond)) {                                                \
      if (g_failures++ < 40) {                                    \
        fprintf(stderr, "FAIL [%s] %s: ", g_case.c_str(), #cond); \
        fprintf(stderr, __VA_ARGS__);                             \
        fprintf(stderr, "\n");                                    \
      }                                                           \
      return;                                                     \
    }                                                             \
  } while (0)

uint32_t g_rng = 2463534242u;
uint32_t next(uint32_t mod) {  // a fixed integer generator
  g_rng = g_rng * 1664525u + 1013904223u;
  return (g_rng >> 8) % mod;
}

std::vector<int32_t> identity(size_t n) {
  std::vector<int32_t> v(n);
  for (size_t i = 0; i < n; i++) v[i] = (int32_t)i;
  return v;
}
std::vector<int32_t> reversed(size_t n) {
  std::vector<int32_t> v(n);
  for (size_t i = 0; i < n; i++) v[i] = (int32_t)(n - 1 - i);
  return v;
}
std::vector<int32_t> shuffled(size_t n) {
  std::vector<int32_t> v = identity(n);
  for (size_t i = n; i > 1; i--) std::swap(v[i - 1], v[next((uint32_t)i)]);
  return v;
}

// ---- the refusals: each case breaks one rule and, where it can, every LATER rule too, so that the order shows
void refusals() {
  g_case = "refusals";
  const int32_t ok[3] = {2, 0, 1}, outside[3] = {2, 7, 2}, negative[3] = {-1, 0, 0}, twice[3] = {1, 0, 1};
  const double v[27] = {};
  struct Case {
    const char *name;
    bool have_tri_id;
    int n_tris;
    const int32_t *idx;
    int n_idx;
    const void *vertices;
    const char *want;  // nullptr: accepted
  };
  const Case cases[] = {
      {"accepted", true, 3, ok, 3, v, nullptr},
      {"accepted, empty list and NULL arrays", true, 3, nullptr, 0, nullptr, nullptr},
      {"accepted, no triangles", true, 0, nullptr, 0, nullptr, nullptr},
      {"accepted, one of three", true, 3, ok, 1, v, nullptr},
      {"no tri_id (and everything after it wrong)", false, 3, nullptr, -1, nullptr, "the scene was made without tri_id"},
      {"negative count (and NULL arrays)", true, 3, nullptr, -1, nullptr, "-1 listed triangles for a scene of 3"},
      {"more than n_tris (and NULL arrays)", true, 2, nullptr, 3, nullptr, "3 listed triangles for a scene of 2"},
      {"NULL list (and NULL vertices)", true, 3, nullptr, 3, nullptr, "the index list is NULL"},
      {"NULL vertices (and an index outside)", true, 3, outside, 3, nullptr, "the vertex array is NULL"},
      {"outside (and one twice)", true, 3, outside, 3, v, "entry 1: add index 7 outside 0..2"},
      {"negative index (and one twice)", true, 3, negative, 3, v, "entry 0: add index -1 outside 0..2"},
      {"twice", true, 3, twice, 3, v, "add index 1 is listed twice"},
  };
  for (const Case &c : cases) {
    g_case = std::string("refusals: ") + c.name;
    MoveError err;
    const bool accepted = check_move_list(c.have_tri_id, c.n_tris, c.idx, c.n_idx, c.vertices, &err);
    if (c.want == nullptr) {
      CHECK(accepted, "refused with '%s'", err.msg.c_str());
      CHECK(err.code == MT_OK, "code %d", err.code);
    } else {
      CHECK(!accepted, "accepted");
      CHECK(err.code == MT_ERR_ARG, "code %d", err.code);
      CHECK(err.msg == c.want, "'%s', want '%s'", err.msg.c_str(), c.want);
    }
  }
  // the getter
  struct Get {
    const char *name;
    bool have_tri_id;
    int scene_tris, n_tris;
    const void *out;
    const char *want;
  };
  const Get gets[] = {
      {"get accepted", true, 3, 3, v, nullptr},
      {"get accepted, none", true, 0, 0, nullptr, nullptr},
      {"get no tri_id (and everything after it wrong)", false, 3, 2, nullptr, "the scene was made without tri_id"},
      {"get count (and NULL)", true, 3, 2, nullptr, "2 triangles for a scene made with 3"},
      {"get NULL", true, 3, 3, nullptr, "the output array is NULL"},
  };
  for (const Get &c : gets) {
    g_case = std::string("refusals: ") + c.name;
    MoveError err;
    const bool accepted = check_move_get(c.have_tri_id, c.scene_tris, c.out, c.n_tris, &err);
    if (c.want == nullptr) {
      CHECK(accepted, "refused with '%s'", err.msg.c_str());
    } else {
      CHECK(!accepted, "accepted");
      CHECK(err.code == MT_ERR_ARG, "code %d", err.code);
      CHECK(err.msg == c.want, "'%s', want '%s'", err.msg.c_str(), c.want);
    }
  }
}

// ---- the permutation: every mirror entry follows its triangle's ADD index, found here by search
void permutation(const char *name, const std::vector<int32_t> &old_id, const std::vector<int32_t> &new_id, bool stamp0, bool stamp1) {
  g_case = std::string("permutation: ") + name + " n=" + std::to_string(old_id.size()) + (stamp0 ? " s0" : "") + (stamp1 ? " s1" : "");
  const size_t n = old_id.size();
  std::vector<int32_t> mtl(n);
  std::vector<uint32_t> stamp[2];
  for (size_t q = 0; q < n; q++) mtl[q] = (int32_t)next(7) - 1;
  if (stamp0) {
    stamp[0].resize(n);
    for (size_t q = 0; q < n; q++) stamp[0][q] = next(5);
  }
  if (stamp1) {
    stamp[1].resize(n);
    for (size_t q = 0; q < n; q++) stamp[1][q] = 0xfffffff0u + next(16);
  }
  const std::vector<int32_t> mtl_was = mtl, old_was = old_id;
  const std::vector<uint32_t> stamp_was[2] = {stamp[0], stamp[1]};
  MovedMirrors out;
  std::vector<int32_t> from;
  MoveError err;
  CHECK(move_mirrors(old_id, new_id.data(), mtl, stamp, &out, &from, &err), "refused: %s", err.msg.c_str());
  CHECK(mtl == mtl_was && old_id == old_was && stamp[0] == stamp_was[0] && stamp[1] == stamp_was[1], "an input was written");
  CHECK(out.tri_id == new_id, "tri_id is not the new one");
  CHECK(from.size() == n && out.tri_mtl.size() == n, "sizes %zu %zu", from.size(), out.tri_mtl.size());
  CHECK(out.stamp[0].size() == (stamp0 ? n : 0) && out.stamp[1].size() == (stamp1 ? n : 0), "an empty stamp plane must stay empty");
  for (size_t p = 0; p < n; p++) {
    size_t q = n;  // the old position of the triangle at p, by search
    for (size_t k = 0; k < n; k++) {
      if (old_id[k] == new_id[p]) q = k;
    }
    CHECK(q < n, "add index %d not found", new_id[p]);
    CHECK(from[p] == (int32_t)q, "from[%zu] = %d, want %zu", p, from[p], q);
    CHECK(out.tri_mtl[p] == mtl[q], "tri_mtl[%zu]", p);
    if (stamp0) CHECK(out.stamp[0][p] == stamp[0][q], "stamp0[%zu]", p);
    if (stamp1) CHECK(out.stamp[1][p] == stamp[1][q], "stamp1[%zu]", p);
  }
}

void not_permutations() {
  g_case = "not permutations";
  MoveError err;
  std::vector<int32_t> from;
  const int32_t good[4] = {3, 1, 0, 2}, twice[4] = {3, 1, 1, 2}, outside[4] = {3, 1, 4, 2}, negative[4] = {3, -1, 0, 2};
  CHECK(compose_move(good, good, 4, &from, &err), "refused");
  for (size_t p = 0; p < 4; p++) CHECK(from[p] == (int32_t)p, "a tri_id composed with itself is the identity");
  for (const int32_t *bad : {twice, outside, negative}) {
    CHECK(!compose_move(bad, good, 4, &from, &err) && err.code == MT_ERR_ARG, "a bad old tri_id was accepted");
    CHECK(!compose_move(good, bad, 4, &from, &err) && err.code == MT_ERR_ARG, "a bad new tri_id was accepted");
  }
  // mirrors of another size
  MovedMirrors out;
  const std::vector<int32_t> id = identity(4);
  const std::vector<uint32_t> none[2] = {{}, {}}, short_plane[2] = {{1u, 2u, 3u}, {}};
  CHECK(!move_mirrors(id, id.data(), std::vector<int32_t>(3, 0), none, &out, &from, &err), "a short assignment was accepted");
  CHECK(!move_mirrors(id, id.data(), std::vector<int32_t>(4, 0), short_plane, &out, &from, &err), "a short stamp plane was accepted");
}

}  // namespace

int main() {
  refusals();
  for (size_t n : {(size_t)0, (size_t)1, (size_t)15, (size_t)16, (size_t)17, (size_t)1025}) {
    for (int planes = 0; planes < 4; planes++) {
      const bool s0 = (planes & 1) != 0, s1 = (planes & 2) != 0;
      permutation("identity -> identity", identity(n), identity(n), s0, s1);
      permutation("identity -> reversal", identity(n), reversed(n), s0, s1);
      permutation("reversal -> identity", reversed(n), identity(n), s0, s1);
      permutation("shuffle -> shuffle", shuffled(n), shuffled(n), s0, s1);
      const std::vector<int32_t> same = shuffled(n);
      permutation("shuffle -> itself", same, same, s0, s1);
    }
  }
  not_permutations();
  if (g_failures) {
    fprintf(stderr, "%d checks failed\n", g_failures);
    return 1;
  }
  printf("all checks held\n");
  return 0;
}
