// edit_check.cc — mt_edit.h without a GPU: the refusals of mt_scene_edit_triangles in their order, and where every
// triangle of an edited scene comes from (compose_edit) with the resized mirrors (edit_mirrors), against brute-force
// restatements written out here (searches and counting, not inverse tables).  Driven by
// tests/test_edit_triangles_cpu.py, which builds it with the address and undefined-behaviour sanitizers.  Exit status
// 0 = every check held; else the failing cases on stderr.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mt_edit.h"

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

std::vector<int32_t> shuffled(size_t n) {
  std::vector<int32_t> v(n);
  for (size_t i = 0; i < n; i++) v[i] = (int32_t)i;
  for (size_t i = n; i > 1; i--) std::swap(v[i - 1], v[next((uint32_t)i)]);
  return v;
}

// ---- the refusals: each case breaks one rule and, where it can, every LATER rule too, so that the order shows
void refusals() {
  const int32_t ok[2] = {2, 0}, outside[3] = {2, 7, 2}, negative[3] = {-1, 0, 0}, twice[3] = {1, 0, 1}, all[3] = {0, 1, 2};
  const int32_t mtl_ok[2] = {-1, 3}, mtl_high[2] = {0, 4}, mtl_low[2] = {-2, 9};
  const double v[18] = {};
  struct Case {
    const char *name;
    bool have_tri_id;
    int n_tris;
    const int32_t *remove;
    int n_remove;
    EditAdd add;
    const char *want;  // nullptr: accepted
  };
  const auto adds = [&](int n, const void *vertex, const void *normal, const void *uvw, const int32_t *material, const void *line) {
    EditAdd a;
    a.n = n;
    a.vertex = vertex;
    a.normal = normal;
    a.uvw = uvw;
    a.material = material;
    a.line_no = line;
    return a;
  };
  const EditAdd none = adds(0, nullptr, nullptr, nullptr, nullptr, nullptr), two = adds(2, v, v, v, mtl_ok, v);
  const Case cases[] = {
      {"accepted", true, 3, ok, 2, two, nullptr},
      {"accepted, the no-op", true, 3, nullptr, 0, none, nullptr},
      {"accepted, all out and two in", true, 3, all, 3, two, nullptr},
      {"accepted, all but one out", true, 3, ok, 2, none, nullptr},
      {"accepted, only added", true, 1, nullptr, 0, two, nullptr},
      {"no tri_id (and everything after it wrong)", false, 0, nullptr, -1, adds(-1, nullptr, nullptr, nullptr, nullptr, nullptr),
       "the scene was made without tri_id"},
      {"no triangles (and counts wrong)", true, 0, nullptr, -1, adds(-1, nullptr, nullptr, nullptr, nullptr, nullptr),
       "a scene of 0 triangles cannot be edited"},
      {"negative n_remove (and n_add negative)", true, 3, nullptr, -1, adds(-1, nullptr, nullptr, nullptr, nullptr, nullptr),
       "-1 triangles to remove from a scene of 3"},
      {"n_remove above n_tris (and n_add negative)", true, 3, nullptr, 4, adds(-2, nullptr, nullptr, nullptr, nullptr, nullptr),
       "4 triangles to remove from a scene of 3"},
      {"negative n_add (and NULL list)", true, 3, nullptr, 2, adds(-2, nullptr, nullptr, nullptr, nullptr, nullptr),
       "-2 triangles to add"},
      {"NULL remove list (and NULL add arrays)", true, 3, nullptr, 2, adds(2, nullptr, nullptr, nullptr, nullptr, nullptr),
       "the remove list is NULL"},
      {"NULL vertex (and the rest NULL, index outside)", true, 3, outside, 3, adds(2, nullptr, nullptr, nullptr, nullptr, nullptr),
       "the added triangles' vertex array is NULL"},
      {"NULL normal", true, 3, outside, 3, adds(2, v, nullptr, nullptr, nullptr, nullptr), "the added triangles' normal array is NULL"},
      {"NULL uvw", true, 3, outside, 3, adds(2, v, v, nullptr, nullptr, nullptr), "the added triangles' uvw array is NULL"},
      {"NULL material", true, 3, outside, 3, adds(2, v, v, v, nullptr, nullptr), "the added triangles' material array is NULL"},
      {"NULL line_no", true, 3, outside, 3, adds(2, v, v, v, mtl_high, nullptr), "the added triangles' line_no array is NULL"},
      {"outside (and one twice, a bad material)", true, 3, outside, 3, adds(2, v, v, v, mtl_high, v),
       "entry 1: remove index 7 outside 0..2"},
      {"negative index (and one twice)", true, 3, negative, 3, adds(2, v, v, v, mtl_high, v), "entry 0: remove index -1 outside 0..2"},
      {"twice (and a bad material)", true, 3, twice, 3, adds(2, v, v, v, mtl_high, v), "remove index 1 is listed twice"},
      {"nothing left", true, 3, all, 3, none, "the edit leaves 0 triangles: a scene holds 1..2147483647"},
      {"too many (and a bad material)", true, 3, ok, 2, adds(0x7fffffff, v, v, v, mtl_high, v),
       "the edit leaves 2147483648 triangles: a scene holds 1..2147483647"},
      {"material too high", true, 3, ok, 2, adds(2, v, v, v, mtl_high, v), "triangle 1: material index 4 outside -1..3"},
      {"material too low", true, 3, ok, 2, adds(2, v, v, v, mtl_low, v), "triangle 0: material index -2 outside -1..3"},
  };
  for (const Case &c : cases) {
    g_case = std::string("refusals: ") + c.name;
    MoveError err;
    const bool accepted = check_edit_args(c.have_tri_id, c.n_tris, c.remove, c.n_remove, c.add, 4, &err);
    if (c.want == nullptr) {
      CHECK(accepted, "refused with '%s'", err.msg.c_str());
      CHECK(err.code == MT_OK, "code %d", err.code);
    } else {
      CHECK(!accepted, "accepted");
      CHECK(err.code == MT_ERR_ARG, "code %d", err.code);
      CHECK(err.msg == c.want, "'%s', want '%s'", err.msg.c_str(), c.want);
    }
  }
}

// ---- where the triangles come from: the new add order by counting, the old positions by search
void composition(const char *name, size_t n_old, const std::vector<int32_t> &remove, size_t n_add, bool stamp0, bool stamp1) {
  g_case = std::string("composition: ") + name + " n=" + std::to_string(n_old) + " -" + std::to_string(remove.size()) + " +" +
           std::to_string(n_add) + (stamp0 ? " s0" : "") + (stamp1 ? " s1" : "");
  const size_t n_new = n_old - remove.size() + n_add;
  if (n_new == 0) return;  // (refused by the argument checks)
  const std::vector<int32_t> old_id = shuffled(n_old), new_id = shuffled(n_new);
  std::vector<int32_t> mtl(n_old), add_mtl(n_add);
  std::vector<uint32_t> stamp[2];
  for (size_t q = 0; q < n_old; q++) mtl[q] = (int32_t)next(7) - 1;
  for (size_t j = 0; j < n_add; j++) add_mtl[j] = 100 + (int32_t)j;
  if (stamp0) {
    stamp[0].resize(n_old);
    for (size_t q = 0; q < n_old; q++) stamp[0][q] = 1u + next(5);
  }
  if (stamp1) {
    stamp[1].resize(n_old);
    for (size_t q = 0; q < n_old; q++) stamp[1][q] = 0xfffffff0u + next(15);
  }
  const std::vector<int32_t> mtl_was = mtl, old_was = old_id, remove_was = remove;
  const std::vector<uint32_t> stamp_was[2] = {stamp[0], stamp[1]};
  MovedMirrors out;
  std::vector<int32_t> src, alone;
  MoveError err;
  CHECK(edit_mirrors(old_id, remove.data(), remove.size(), n_add, add_mtl.data(), new_id.data(), n_new, mtl, stamp, &out, &src, &err),
        "refused: %s", err.msg.c_str());
  CHECK(compose_edit(old_id.data(), n_old, remove.data(), remove.size(), n_add, new_id.data(), n_new, &alone, &err), "refused: %s",
        err.msg.c_str());
  CHECK(alone == src, "compose_edit alone differs from edit_mirrors'");
  CHECK(mtl == mtl_was && old_id == old_was && remove == remove_was && stamp[0] == stamp_was[0] && stamp[1] == stamp_was[1],
        "an input was written");
  CHECK(out.tri_id == new_id, "tri_id is not the new one");
  CHECK(src.size() == n_new && out.tri_mtl.size() == n_new, "sizes %zu %zu", src.size(), out.tri_mtl.size());
  CHECK(out.stamp[0].size() == (stamp0 ? n_new : 0) && out.stamp[1].size() == (stamp1 ? n_new : 0),
        "an empty stamp plane must stay empty, another has the new count");
  const size_t n_keep = n_old - remove.size();
  std::vector<int32_t> survivors;
  for (size_t a = 0; a < n_old; a++) {
    if (std::find(remove.begin(), remove.end(), (int32_t)a) == remove.end()) survivors.push_back((int32_t)a);
  }
  CHECK(survivors.size() == n_keep, "%zu survivors, want %zu", survivors.size(), n_keep);
  for (size_t p = 0; p < n_new; p++) {
    const size_t a_new = (size_t)new_id[p];
    if (a_new >= n_keep) {  // an added triangle
      const size_t j = a_new - n_keep;
      CHECK(src[p] == ~(int32_t)j, "src[%zu] = %d, want ~%zu", p, src[p], j);
      CHECK(out.tri_mtl[p] == add_mtl[j], "tri_mtl[%zu] of an added triangle", p);
      if (stamp0) CHECK(out.stamp[0][p] == 0u, "stamp0[%zu] of an added triangle", p);
      if (stamp1) CHECK(out.stamp[1][p] == 0u, "stamp1[%zu] of an added triangle", p);
      continue;
    }
    const size_t a_old = (size_t)survivors[a_new];  // numpy.delete: the a_new-th old add index that is not listed
    size_t q = n_old;
    for (size_t k = 0; k < n_old; k++) {
      if ((size_t)old_id[k] == a_old) q = k;
    }
    CHECK(q < n_old, "add index %zu not found", a_old);
    CHECK(src[p] == (int32_t)q, "src[%zu] = %d, want %zu", p, src[p], q);
    CHECK(out.tri_mtl[p] == mtl[q], "tri_mtl[%zu]", p);
    if (stamp0) CHECK(out.stamp[0][p] == stamp[0][q], "stamp0[%zu]", p);
    if (stamp1) CHECK(out.stamp[1][p] == stamp[1][q], "stamp1[%zu]", p);
  }
}

void not_composable() {
  g_case = "not composable";
  MoveError err;
  std::vector<int32_t> src;
  const int32_t good[4] = {3, 1, 0, 2}, twice[4] = {3, 1, 1, 2}, outside[4] = {3, 1, 4, 2}, negative[4] = {3, -1, 0, 2};
  const int32_t rm[1] = {2}, rm_twice[2] = {2, 2}, rm_out[1] = {4}, new5[5] = {4, 0, 3, 1, 2}, new3[3] = {2, 0, 1};
  CHECK(compose_edit(good, 4, nullptr, 0, 0, good, 4, &src, &err), "refused");
  for (size_t p = 0; p < 4; p++) CHECK(src[p] == (int32_t)p, "nothing removed, nothing added, one tri_id: the identity");
  CHECK(compose_edit(good, 4, rm, 1, 2, new5, 5, &src, &err), "refused");
  CHECK(compose_edit(good, 4, rm, 1, 0, new3, 3, &src, &err), "refused");
  for (const int32_t *bad : {twice, outside, negative}) {
    CHECK(!compose_edit(bad, 4, nullptr, 0, 0, good, 4, &src, &err) && err.code == MT_ERR_ARG, "a bad old tri_id was accepted");
    CHECK(!compose_edit(good, 4, nullptr, 0, 0, bad, 4, &src, &err) && err.code == MT_ERR_ARG, "a bad new tri_id was accepted");
  }
  CHECK(!compose_edit(good, 4, rm_twice, 2, 1, new3, 3, &src, &err), "a remove list with a repeat was accepted");
  CHECK(!compose_edit(good, 4, rm_out, 1, 0, new3, 3, &src, &err), "a remove index outside was accepted");
  CHECK(!compose_edit(good, 4, rm, 1, 0, good, 4, &src, &err), "a new tri_id of another count was accepted");
  CHECK(!compose_edit(good, 4, rm, 1, 2, new3, 3, &src, &err), "a new tri_id of another count was accepted");
  // mirrors of another size
  MovedMirrors out;
  const std::vector<int32_t> id = {0, 1, 2, 3};
  const std::vector<uint32_t> none[2] = {{}, {}}, short_plane[2] = {{1u, 2u, 3u}, {}};
  CHECK(!edit_mirrors(id, nullptr, 0, 0, nullptr, id.data(), 4, std::vector<int32_t>(3, 0), none, &out, &src, &err),
        "a short assignment was accepted");
  CHECK(!edit_mirrors(id, nullptr, 0, 0, nullptr, id.data(), 4, std::vector<int32_t>(4, 0), short_plane, &out, &src, &err),
        "a short stamp plane was accepted");
}

}  // namespace

int main() {
  refusals();
  for (size_t n : {(size_t)1, (size_t)2, (size_t)15, (size_t)16, (size_t)17, (size_t)1025}) {
    const std::vector<int32_t> order = shuffled(n);  // removal lists are its prefixes: unsorted
    for (size_t n_remove : {(size_t)0, (size_t)1, n / 2, n - 1}) {
      const std::vector<int32_t> remove(order.begin(), order.begin() + (long)n_remove);
      for (size_t n_add : {(size_t)0, (size_t)1, (size_t)65}) {
        const int planes = (int)((n + n_remove + n_add) % 4);  // every combination of planes comes by
        composition("shuffled", n, remove, n_add, (planes & 1) != 0, (planes & 2) != 0);
      }
    }
    // index 0 and the last index alone, and all planes at once
    composition("first", n, {0}, 1, true, true);
    composition("last", n, {(int32_t)(n - 1)}, 1, true, true);
    composition("no planes", n, {(int32_t)(n - 1)}, 65, false, false);
  }
  not_composable();
  if (g_failures) {
    fprintf(stderr, "%d checks failed\n", g_failures);
    return 1;
  }
  printf("all checks held\n");
  return 0;
}
