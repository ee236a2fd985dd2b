// layout_check.cc — mt_layout.h without a GPU: small scenes built in memory, check_scene_desc's refusals word for
// word, and every array of derive_layout against brute-force restatements written out here (nothing below calls the
// header's helpers).  Driven by tests/test_layout_cpu.py, which builds it with the address and undefined-behaviour
// sanitizers.  Exit status 0 = every check held; else the failing cases on stderr.
//   layout_check          run the checks
//   layout_check --hash   one FNV-1a value per array and scene (to compare two versions of the derivation by hand)
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "mt_layout.h"

using namespace mt;

namespace {

int g_failures = 0;
std::string g_case;

#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      if (g_failures++ < 40) {                                  \
        fprintf(stderr, "FAIL [%s] %s: ", g_case.c_str(), #cond); \
        fprintf(stderr, __VA_ARGS__);                           \
        fprintf(stderr, "\n");                                  \
      }                                                         \
      return;                                                   \
    }                                                           \
  } while (0)

// ---- scenes

struct Scene {
  std::string name;
  std::vector<double> node_aabb, node_center;
  std::vector<int32_t> first_child, prim_begin, prim_count;
  std::vector<double> tri_vertex, tri_normal, tri_uvw, tri_aabb;
  std::vector<int32_t> tri_material, tri_line_no;
  std::vector<mt_material> materials;
  std::vector<mt_texture> textures;
  uint32_t rng = 12345u;

  int n_nodes() const { return (int)first_child.size(); }
  int n_tris() const { return (int)tri_material.size(); }

  uint32_t next(uint32_t mod) {  // a fixed integer generator
    rng = rng * 1664525u + 1013904223u;
    return (rng >> 8) % mod;
  }
  int add_node(const double lo[3], const double hi[3]) {
    for (int k = 0; k < 3; k++) node_aabb.push_back(lo[k]);
    for (int k = 0; k < 3; k++) node_aabb.push_back(hi[k]);
    for (int k = 0; k < 3; k++) node_center.push_back(lo[k] * 0.5 + hi[k] * 0.5);
    first_child.push_back(0);
    prim_begin.push_back(0);
    prim_count.push_back(0);
    return n_nodes() - 1;
  }
  // the eight octants of node i become the next eight nodes (bit 0 = x high, bit 1 = z high, bit 2 = y high)
  int split(int i) {
    const int fc = n_nodes();
    for (int c = 0; c < 8; c++) {
      double lo[3], hi[3];
      const int high[3] = {c & 1, (c >> 2) & 1, (c >> 1) & 1};
      for (int k = 0; k < 3; k++) {
        const double a = node_aabb[(size_t)i * 6 + k], b = node_aabb[(size_t)i * 6 + 3 + k], m = node_center[(size_t)i * 3 + k];
        lo[k] = high[k] ? m : a;
        hi[k] = high[k] ? b : m;
      }
      add_node(lo, hi);
    }
    first_child[(size_t)i] = fc;
    return fc;
  }
  // n triangles appended to the stream as node i's list: boxes of tenths (not fp32 numbers), extents 0.1 .. 0.5,
  // every seventh a coincident copy of the one before it; flat: no extent in x
  void fill(int i, int n, bool flat = false) {
    prim_begin[(size_t)i] = n_tris();
    prim_count[(size_t)i] = n;
    for (int k = 0; k < n; k++) {
      double b[6];
      if (k % 7 == 6) {
        memcpy(b, &tri_aabb[tri_aabb.size() - 6], sizeof b);
      } else {
        for (int a = 0; a < 3; a++) {
          b[a] = 0.1 * (double)next(1200) + 0.001 * (double)(n_tris() % 89);
          b[3 + a] = b[a] + 0.1 * (double)(1 + next(5));
        }
      }
      if (flat) b[3] = b[0];
      tri_aabb.insert(tri_aabb.end(), b, b + 6);
      const double v[9] = {b[0], b[1], b[2], b[3], b[1], b[5], b[0], b[4], b[2] * 0.5 + b[5] * 0.5};
      tri_vertex.insert(tri_vertex.end(), v, v + 9);
      for (int q = 0; q < 9; q++) tri_normal.push_back(q % 3 == 2 ? 1.0 : 0.0);
      for (int q = 0; q < 9; q++) tri_uvw.push_back(0.125 * q);
      tri_material.push_back(-1);
      tri_line_no.push_back(n_tris());
    }
  }
  mt_scene_desc desc() const {
    mt_scene_desc d;
    memset(&d, 0, sizeof d);
    d.struct_size = sizeof d;
    d.abi_version = MT_ABI_VERSION;
    d.n_nodes = n_nodes();
    d.n_tris = n_tris();
    d.n_materials = (int)materials.size();
    d.n_textures = (int)textures.size();
    d.node_aabb = node_aabb.data();
    d.node_center = node_center.data();
    d.node_first_child = first_child.data();
    d.node_prim_begin = prim_begin.data();
    d.node_prim_count = prim_count.data();
    if (n_tris() > 0) {
      d.tri_vertex = tri_vertex.data();
      d.tri_normal = tri_normal.data();
      d.tri_uvw = tri_uvw.data();
      d.tri_aabb = tri_aabb.data();
      d.tri_material = tri_material.data();
      d.tri_line_no = tri_line_no.data();
    }
    d.materials = materials.empty() ? nullptr : materials.data();
    d.textures = textures.empty() ? nullptr : textures.data();
    return d;
  }
};

Scene new_scene(const std::string &name) {
  Scene s;
  s.name = name;
  const double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {128.0, 128.0, 128.0};
  s.add_node(lo, hi);
  return s;
}

// A root with eight children: the root's list of l at stream position 0, child 0's of l2 at l, fillers in children 3,
// 5 and 7; the other children's subtrees are empty.
Scene pair_scene(int l, int l2) {
  Scene s = new_scene("pair " + std::to_string(l) + " " + std::to_string(l2));
  const int fc = s.split(0);
  s.fill(0, l);
  s.fill(fc, l2);
  s.fill(fc + 3, 2);
  s.fill(fc + 5, 5);
  s.fill(fc + 7, 3);
  return s;
}

// Three levels: child 1 is an inner node whose children are all empty; child 3's children hold a short and a long list;
// child 7's only triangle is flat.
Scene deep_scene() {
  Scene s = new_scene("three levels");
  const int fc = s.split(0);
  const int empty_kids = s.split(fc + 1);
  (void)empty_kids;
  const int kids = s.split(fc + 3);
  s.fill(0, 5);
  s.fill(fc + 2, 2);
  s.fill(fc + 7, 1, true);
  s.fill(kids + 1, 3);
  s.fill(kids + 3, 40);
  return s;
}

// A long list that starts at a stream position that is no multiple of 16, behind two short ones.
Scene unaligned_scene() {
  Scene s = new_scene("unaligned");
  const int fc = s.split(0);
  s.fill(0, 5);
  s.fill(fc, 7);
  s.fill(fc + 1, 40);
  s.fill(fc + 6, 33);
  return s;
}

// The layout's boundaries (tests/list_lengths.py), every long length with a short partner in both orders and every
// short length with a long one; a few pairs without a long list and with two.
std::vector<std::pair<int, int>> length_pairs() {
  const int shorts[] = {0, 1, 3, 4, 5, 15, 16, 17, 31, 32}, longs[] = {33, 63, 64, 65, 255, 256, 257, 1793};
  std::set<std::pair<int, int>> out;
  for (int i = 0; i < 8; i++) {
    out.insert({longs[i], shorts[i % 10]});
    out.insert({shorts[i % 10], longs[i]});
  }
  for (int j = 0; j < 10; j++) {
    out.insert({longs[(j + 3) % 8], shorts[j]});
    out.insert({shorts[j], longs[(j + 3) % 8]});
    out.insert({shorts[j], shorts[(j + 3) % 10]});
  }
  out.insert({0, 0});
  out.insert({257, 65});
  out.insert({33, 257});
  out.insert({1793, 256});
  return std::vector<std::pair<int, int>>(out.begin(), out.end());
}

std::vector<Scene> all_scenes() {
  std::vector<Scene> out;
  for (const auto &p : length_pairs()) out.push_back(pair_scene(p.first, p.second));
  out.push_back(deep_scene());
  out.push_back(new_scene("no triangles"));
  out.push_back(unaligned_scene());
  return out;
}

// ---- the restatements

const float kBig = 3.0e38f;

template <typename T>
bool same_bits(T a, T b) {
  return memcmp(&a, &b, sizeof a) == 0;
}

template <typename T>
bool all_equal(const std::vector<T> &v, size_t from, size_t to, T want) {
  if (to > v.size()) return false;
  for (size_t i = from; i < to; i++) {
    if (!same_bits(v[i], want)) return false;
  }
  return true;
}

struct Box {
  double v[6] = {3.0e38, 3.0e38, 3.0e38, -3.0e38, -3.0e38, -3.0e38};
  bool empty = true;
  void add(const double *b) {
    for (int k = 0; k < 3; k++) {
      if (b[k] < v[k]) v[k] = b[k];
      if (b[3 + k] > v[3 + k]) v[3 + k] = b[3 + k];
    }
    empty = false;
  }
  // the six floats at p are this box rounded (or the inverted box, if nothing was added)
  bool is(const float *p) const {
    for (int k = 0; k < 6; k++) {
      if (!same_bits(p[k], empty ? (k < 3 ? kBig : -kBig) : (float)v[k])) return false;
    }
    return true;
  }
};

struct FBox {  // the same over fp32 boxes
  float v[6] = {kBig, kBig, kBig, -kBig, -kBig, -kBig};
  void add(const float *b) {
    for (int k = 0; k < 3; k++) {
      if (b[k] < v[k]) v[k] = b[k];
      if (b[3 + k] > v[3 + k]) v[3 + k] = b[3 + k];
    }
  }
};

// box i of a quad array: [lo x 4][hi x 4][lo x 4] per axis and four boxes
bool quad_is(const std::vector<float> &q, size_t first_quad, size_t i, const float want[6]) {
  const size_t at = (first_quad + i / 4) * 36 + (i & 3);
  if (at + 2 * 12 + 8 >= q.size()) return false;
  for (int a = 0; a < 3; a++) {
    if (!same_bits(q[at + a * 12], want[a]) || !same_bits(q[at + a * 12 + 4], want[3 + a]) ||
        !same_bits(q[at + a * 12 + 8], want[a])) {
      return false;
    }
  }
  return true;
}

const float kInv[6] = {kBig, kBig, kBig, -kBig, -kBig, -kBig};

// all triangles in the subtree of node i, by descent
void collect(const Scene &s, int i, Box *box) {
  for (int t = s.prim_begin[(size_t)i]; t < s.prim_begin[(size_t)i] + s.prim_count[(size_t)i]; t++) box->add(&s.tri_aabb[(size_t)t * 6]);
  if (s.first_child[(size_t)i] != 0) {
    for (int c = 0; c < 8; c++) collect(s, s.first_child[(size_t)i] + c, box);
  }
}

int level_of(const Scene &s, int i) {  // root = 0, by looking for the parent
  int level = 0;
  while (i != 0) {
    int parent = -1;
    for (int p = 0; p < s.n_nodes(); p++) {
      if (s.first_child[(size_t)p] != 0 && i >= s.first_child[(size_t)p] && i < s.first_child[(size_t)p] + 8) parent = p;
    }
    i = parent;
    level++;
  }
  return level;
}

void check_sizes_and_padding(const Scene &s, const SceneLayout &L) {
  const size_t nn = (size_t)s.n_nodes(), nt = (size_t)s.n_tris();
  const size_t nblk = (nt + 15) / 16, nsup = (nblk + kSuperBlocks - 1) / kSuperBlocks;
  size_t sl_quads = 0, entries = 0;
  for (size_t i = 0; i < nn; i++) {
    const size_t c = (size_t)s.prim_count[i];
    if (c >= 1 && c <= 32) sl_quads += (c + 3) / 4;
    if (c > 32) entries += (c + 255) / 256 * 256;
  }
  CHECK(L.recs.size() == nn, "%zu", L.recs.size());
  CHECK(L.groups.size() == nblk * 6 + 8 * 6, "%zu", L.groups.size());
  CHECK(L.supers.size() == nsup * 6 + 8 * 6, "%zu", L.supers.size());
  CHECK(L.subs.size() == nn * 6 + 8 * 6, "%zu", L.subs.size());
  CHECK(L.hsr.size() == nn + 1, "%zu", L.hsr.size());
  CHECK(L.sl_box.size() == (sl_quads + 2) * 36, "%zu", L.sl_box.size());
  CHECK(L.ll_tri.size() == entries + 64, "%zu", L.ll_tri.size());
  CHECK(L.ll_exact.size() == entries * 15 + 15, "%zu", L.ll_exact.size());
  CHECK(L.ll_box_q.size() == (entries / 4 + 1) * 36, "%zu", L.ll_box_q.size());
  CHECK(L.ll_grp_q.size() == ((entries / 16 + 3) / 4 + 1) * 36, "%zu", L.ll_grp_q.size());
  CHECK(L.ll_sup_q.size() == ((entries / 64 + 3) / 4 + 1) * 36, "%zu", L.ll_sup_q.size());
  CHECK(L.tri_aabb.size() == nt * 6 + 4 * 6, "%zu", L.tri_aabb.size());
  CHECK(L.tri_aabb32.size() == nt * 6 + 64 * 6, "%zu", L.tri_aabb32.size());
  CHECK(all_equal(L.groups, nblk * 6, L.groups.size(), 0.0f), "groups' padding");
  CHECK(all_equal(L.supers, nsup * 6, L.supers.size(), 0.0f), "supers' padding");
  CHECK(all_equal(L.subs, nn * 6, L.subs.size(), 0.0f), "subs' padding");
  CHECK(all_equal(L.sl_box, sl_quads * 36, L.sl_box.size(), 0.0f), "sl_box's padding");
  CHECK(all_equal(L.ll_tri, entries, L.ll_tri.size(), (int32_t)-1), "ll_tri's padding");
  CHECK(all_equal(L.ll_exact, entries * 15, L.ll_exact.size(), 0.0), "ll_exact's padding");
  CHECK(all_equal(L.ll_box_q, L.ll_box_q.size() - 36, L.ll_box_q.size(), 0.0f), "ll_box_q's padding");
  CHECK(all_equal(L.ll_grp_q, L.ll_grp_q.size() - 36, L.ll_grp_q.size(), 0.0f), "ll_grp_q's padding");
  CHECK(all_equal(L.ll_sup_q, L.ll_sup_q.size() - 36, L.ll_sup_q.size(), 0.0f), "ll_sup_q's padding");
  CHECK(all_equal(L.tri_aabb, nt * 6, L.tri_aabb.size(), 0.0), "tri_aabb's padding");
  CHECK(all_equal(L.tri_aabb32, nt * 6, L.tri_aabb32.size(), 0.0f), "tri_aabb32's padding");
  const std::vector<unsigned char> zero(sizeof(HsRec), 0);
  CHECK(memcmp(&L.hsr[nn], zero.data(), sizeof(HsRec)) == 0, "hsr[n_nodes] is not all zero");
}

void check_stream_boxes(const Scene &s, const SceneLayout &L) {
  const size_t nt = (size_t)s.n_tris(), nblk = (nt + 15) / 16;
  for (size_t b = 0; b < nblk; b++) {
    Box u;
    for (size_t t = 16 * b; t < std::min(16 * b + 16, nt); t++) u.add(&s.tri_aabb[t * 6]);
    CHECK(u.is(&L.groups[b * 6]), "block %zu", b);
  }
  for (size_t sp = 0; sp * kSuperBlocks < nblk; sp++) {
    Box u;
    for (size_t t = 16 * kSuperBlocks * sp; t < std::min(16 * kSuperBlocks * (sp + 1), nt); t++) u.add(&s.tri_aabb[t * 6]);
    CHECK(u.is(&L.supers[sp * 6]), "super %zu", sp);
  }
  double bmax[3] = {0x1p-7, 0x1p-7, 0x1p-7};
  for (size_t i = 0; i < nt * 6; i++) {
    CHECK(same_bits(L.tri_aabb[i], s.tri_aabb[i]), "tri_aabb[%zu]", i);
    CHECK(same_bits(L.tri_aabb32[i], (float)s.tri_aabb[i]), "tri_aabb32[%zu]", i);
    if (std::fabs(s.tri_aabb[i]) > bmax[i % 3]) bmax[i % 3] = std::fabs(s.tri_aabb[i]);
  }
  for (int k = 0; k < 3; k++) CHECK(same_bits(L.bmax[k], bmax[k]), "bmax[%d] %g, want %g", k, L.bmax[k], bmax[k]);
}

void check_nodes(const Scene &s, const SceneLayout &L) {
  int ll_at = 0, sl_at = 0, deepest = 0;
  for (int i = 0; i < s.n_nodes(); i++) {
    const size_t z = (size_t)i;
    const NodeRec &r = L.recs[z];
    const HsRec &h = L.hsr[z];
    const int fc = s.first_child[z], pb = s.prim_begin[z], pc = s.prim_count[z];
    deepest = std::max(deepest, level_of(s, i) + 1);
    CHECK(r.first_child == fc && r.prim_begin == pb && r.prim_count == pc && r.level == level_of(s, i) && r.pad1 == 0, "node %d's record", i);
    CHECK(h.first_child == fc && h.prim_begin == pb && h.prim_count == pc && h.pad0 == 0 && h.pad1[0] == 0 && h.pad1[1] == 0, "node %d's HsRec", i);
    for (int k = 0; k < 3; k++) {
      const double lo = s.node_aabb[z * 6 + k], hi = s.node_aabb[z * 6 + 3 + k], c = s.node_center[z * 3 + k];
      CHECK(same_bits(r.lo[k], lo) && same_bits(r.hi[k], hi) && same_bits(r.c[k], c), "node %d's planes", i);
      CHECK(same_bits(h.planes[k], lo) && same_bits(h.planes[3 + k], c) && same_bits(h.planes[6 + k], hi), "node %d's HsRec planes", i);
    }
    Box sub, own;
    collect(s, i, &sub);
    CHECK(sub.is(&L.subs[z * 6]), "node %d's subtree box", i);
    CHECK((L.subs[z * 6] > L.subs[z * 6 + 3]) == sub.empty, "node %d: inverted iff empty", i);
    int mask = 0;
    for (int c = 0; c < 8; c++) {
      Box kid;
      if (fc != 0) collect(s, fc + c, &kid);
      if (!kid.empty) mask |= 1 << c;
      const float *want = fc != 0 ? &L.subs[(size_t)(fc + c) * 6] : kInv;
      CHECK(fc == 0 || kid.is(want), "node %d child %d", i, c);
      for (int a = 0; a < 3; a++) {
        CHECK(same_bits(h.kid[a][c], want[a]) && same_bits(h.kid[a][8 + c], want[3 + a]) && same_bits(h.kid[a][16 + c], want[a]),
              "node %d: kid row %d, child %d", i, a, c);
      }
    }
    CHECK(r.child_mask == mask && h.child_mask == mask, "node %d: child_mask %x / %x, want %x", i, r.child_mask, h.child_mask, mask);
    for (int t = pb; t < pb + pc; t++) own.add(&s.tri_aabb[(size_t)t * 6]);
    float o[6];
    for (int a = 0; a < 3; a++) {
      o[a] = h.own[a][0];
      o[3 + a] = h.own[a][1];
      CHECK(same_bits(h.own[a][2], h.own[a][0]), "node %d: own row %d", i, a);
    }
    CHECK(own.is(o), "node %d's own box", i);
    // the short list's quads
    if (pc >= 1 && pc <= 32) {
      CHECK(h.sl_begin == sl_at, "node %d: sl_begin %d, want %d", i, h.sl_begin, sl_at);
      for (int e = 0; e < (pc + 3) / 4 * 4; e++) {
        float want[6];
        for (int k = 0; k < 6; k++) want[k] = e < pc ? (float)s.tri_aabb[(size_t)(pb + e) * 6 + k] : kInv[k];
        CHECK(quad_is(L.sl_box, (size_t)sl_at, (size_t)e, want), "node %d: short-list entry %d", i, e);
      }
      sl_at += (pc + 3) / 4;
    } else {
      CHECK(h.sl_begin == -1, "node %d: sl_begin %d", i, h.sl_begin);
    }
    // the long list's sorted copy
    if (pc > 32) {
      CHECK(h.ll_begin == ll_at && ll_at % 256 == 0, "node %d: ll_begin %d, want %d", i, h.ll_begin, ll_at);
      const int padded = (pc + 255) / 256 * 256;
      std::set<int32_t> seen;
      for (int e = 0; e < padded; e++) {
        const int32_t t = L.ll_tri[(size_t)(ll_at + e)];
        const double *x = &L.ll_exact[(size_t)(ll_at + e) * 15];
        if (e >= pc) {
          CHECK(t == -1, "node %d: padding entry %d is %d", i, e, t);
          for (int q = 0; q < 15; q++) CHECK(same_bits(x[q], 0.0), "node %d: padding entry %d's ll_exact", i, e);
          continue;
        }
        CHECK(t >= pb && t < pb + pc && seen.insert(t).second, "node %d: entry %d is %d: no permutation", i, e, t);
        for (int q = 0; q < 6; q++) CHECK(same_bits(x[q], s.tri_aabb[(size_t)t * 6 + q]), "node %d: entry %d's box", i, e);
        for (int q = 0; q < 9; q++) CHECK(same_bits(x[6 + q], s.tri_vertex[(size_t)t * 9 + q]), "node %d: entry %d's vertices", i, e);
      }
      ll_at += padded;
    } else {
      CHECK(h.ll_begin == -1, "node %d: ll_begin %d", i, h.ll_begin);
    }
  }
  CHECK(L.max_depth == deepest, "max_depth %d, want %d", L.max_depth, deepest);
}

// the three levels of quads over the sorted copy, from ll_tri alone
void check_long_list_quads(const Scene &s, const SceneLayout &L) {
  const size_t entries = L.ll_tri.size() - 64;
  std::vector<float> box(entries * 6);
  for (size_t e = 0; e < entries; e++) {
    const int32_t t = L.ll_tri[e];
    for (int k = 0; k < 6; k++) box[e * 6 + k] = t >= 0 ? (float)s.tri_aabb[(size_t)t * 6 + k] : kInv[k];
    CHECK(quad_is(L.ll_box_q, 0, e, &box[e * 6]), "entry %zu's quad", e);
  }
  for (size_t per : {(size_t)16, (size_t)64}) {
    const std::vector<float> &q = per == 16 ? L.ll_grp_q : L.ll_sup_q;
    const size_t n = entries / per;
    for (size_t b = 0; b < (n + 3) / 4 * 4; b++) {
      FBox u;
      for (size_t e = b * per; e < std::min((b + 1) * per, entries); e++) {
        if (L.ll_tri[e] >= 0) u.add(&box[e * 6]);
      }
      CHECK(quad_is(q, 0, b, u.v), "union %zu of %zu entries", b, per);
    }
  }
}

void check_layout(const Scene &s) {
  g_case = s.name;
  const mt_scene_desc d = s.desc();
  std::vector<int> depth_of;
  int max_depth = 0;
  LayoutError err;
  CHECK(check_scene_desc(d, &depth_of, &max_depth, &err), "refused: %s", err.msg.c_str());
  SceneLayout L;
  derive_layout(d, depth_of, &L);
  CHECK(L.max_depth == max_depth, "max_depth %d / %d", L.max_depth, max_depth);
  CHECK(L.regular, "not regular");
  const int before = g_failures;
  check_sizes_and_padding(s, L);
  if (g_failures != before) return;  // (the other checks index by these sizes)
  check_stream_boxes(s, L);
  check_nodes(s, L);
  check_long_list_quads(s, L);
}

// ---- scene_regular

bool regular_of(const Scene &s) {
  const mt_scene_desc d = s.desc();
  std::vector<int> depth_of;
  int max_depth = 0;
  LayoutError err;
  if (!check_scene_desc(d, &depth_of, &max_depth, &err)) {
    fprintf(stderr, "FAIL [%s] refused: %s\n", g_case.c_str(), err.msg.c_str());
    g_failures++;
    return false;
  }
  SceneLayout L;
  derive_layout(d, depth_of, &L);
  return L.regular;
}

void check_regular() {
  const Scene base = pair_scene(5, 3);
  const double nan = std::nan(""), inf = INFINITY;
  struct Edit { const char *what; int array; size_t index; double value; bool regular; };
  // array 0 node_aabb, 1 node_center, 2 tri_aabb.  Node 0 is inner, node 2 a leaf; lo of the root is 0, hi 128.
  const Edit edits[] = {
      {"unchanged", 2, 0, base.tri_aabb[0], true},
      {"NaN in node_aabb", 0, 6 * 2 + 1, nan, false},
      {"inf in node_aabb", 0, 6 * 2 + 4, inf, false},
      {"NaN in node_center", 1, 3 * 2 + 1, nan, false},
      {"-inf in node_center", 1, 3 * 2, -inf, false},
      {"NaN in tri_aabb", 2, 6 * 4 + 2, nan, false},
      {"inf in tri_aabb", 2, 6 * 4 + 5, inf, false},
      {"lo > hi in a node box", 0, 6 * 2 + 0, 1000.0, false},
      {"lo > hi in a triangle box", 2, 6 * 7 + 1, 1000.0, false},
      {"centre above an inner node's box", 1, 2, 129.0, false},
      {"centre below an inner node's box", 1, 0, -1.0, false},
      {"centre outside a leaf's box", 1, 3 * 2 + 1, 1000.0, true},
  };
  for (const Edit &e : edits) {
    g_case = std::string("regular: ") + e.what;
    Scene s = base;
    (e.array == 0 ? s.node_aabb : e.array == 1 ? s.node_center : s.tri_aabb)[e.index] = e.value;
    CHECK(regular_of(s) == e.regular, "want %d", (int)e.regular);
  }
}

// ---- check_scene_desc's refusals

void expect_refusal(const char *what, const mt_scene_desc &d, int code, const std::string &msg) {
  g_case = std::string("refusal: ") + what;
  std::vector<int> depth_of;
  int max_depth = 0;
  LayoutError err;
  CHECK(!check_scene_desc(d, &depth_of, &max_depth, &err), "accepted");
  CHECK(err.code == code && err.msg == msg, "%d \"%s\", want %d \"%s\"", err.code, err.msg.c_str(), code, msg.c_str());
}

std::string text(const char *fmt, size_t a, int b) {
  char buf[256];
  snprintf(buf, sizeof buf, fmt, a, b);
  return buf;
}

void check_refusals() {
  const Scene base = pair_scene(5, 3);  // 9 nodes, 18 triangles
  mt_scene_desc d = base.desc();
  d.struct_size -= 8;
  expect_refusal("struct size", d, MT_ERR_ARG,
                 "mt_scene_desc size/version mismatch (" + std::to_string(sizeof d - 8) + "/" + std::to_string(MT_ABI_VERSION) +
                     text(", want %zu/%d)", sizeof d, MT_ABI_VERSION));
  d = base.desc();
  d.abi_version += 1;
  expect_refusal("abi version", d, MT_ERR_ARG,
                 "mt_scene_desc size/version mismatch (" + std::to_string(sizeof d) + "/" + std::to_string(MT_ABI_VERSION + 1) +
                     text(", want %zu/%d)", sizeof d, MT_ABI_VERSION));
  d = base.desc();
  d.n_nodes = 0;
  expect_refusal("n_nodes 0", d, MT_ERR_ARG, "negative or empty counts");
  d = base.desc();
  d.n_tris = -1;
  expect_refusal("n_tris -1", d, MT_ERR_ARG, "negative or empty counts");
  d = base.desc();
  d.node_prim_count = nullptr;
  expect_refusal("node arrays", d, MT_ERR_ARG, "node arrays missing");
  d = base.desc();
  d.node_aabb = nullptr;
  expect_refusal("node_aabb", d, MT_ERR_ARG, "node arrays missing");
  d = base.desc();
  d.tri_uvw = nullptr;
  expect_refusal("triangle arrays", d, MT_ERR_ARG, "triangle arrays missing");
  d = base.desc();
  d.tri_line_no = nullptr;
  expect_refusal("tri_line_no", d, MT_ERR_ARG, "triangle arrays missing");
  d = base.desc();
  d.n_materials = 1;
  expect_refusal("materials", d, MT_ERR_ARG, "material/texture arrays missing");
  d = base.desc();
  d.n_textures = 2;
  expect_refusal("textures", d, MT_ERR_ARG, "material/texture arrays missing");

  Scene s = base;
  s.prim_count[8] = 4;  // (the last list: 3 at 15)
  expect_refusal("primitive range", s.desc(), MT_ERR_ARG, "node 8: primitive range [15,+4) outside 0..18");
  s = base;
  s.prim_begin[3] = -1;
  expect_refusal("negative prim_begin", s.desc(), MT_ERR_ARG, "node 3: primitive range [-1,+0) outside 0..18");
  s = base;
  s.first_child[0] = 0;
  expect_refusal("unreachable", s.desc(), MT_ERR_ARG, "node 1 is not reachable in BFS order");
  s = deep_scene();  // 25 nodes: 0 -> 1..8, 2 -> 9..16, 4 -> 17..24
  s.first_child[4] = 4;
  expect_refusal("first_child = i", s.desc(), MT_ERR_ARG, "node 4: first_child 4 invalid (n_nodes 25)");
  s.first_child[4] = 3;
  expect_refusal("first_child < i", s.desc(), MT_ERR_ARG, "node 4: first_child 3 invalid (n_nodes 25)");
  s.first_child[4] = 18;
  expect_refusal("first_child + 8 > n_nodes", s.desc(), MT_ERR_ARG, "node 4: first_child 18 invalid (n_nodes 25)");
  s.first_child[4] = 16;
  expect_refusal("two parents", s.desc(), MT_ERR_ARG, "node 16 has two parents");
  s = base;
  s.prim_count[6] = 4;
  expect_refusal("prim_total", s.desc(), MT_ERR_ARG, "nodes reference 17 primitives, scene has 18");

  s = new_scene("depth");  // a chain: the first child of every level splits again
  for (int level = 1, i = 0; level < MT_MAX_TREE_DEPTH + 1; level++) i = s.split(i);
  expect_refusal("depth", s.desc(), MT_ERR_UNSUPPORTED,
                 "octree depth " + std::to_string(MT_MAX_TREE_DEPTH + 1) + " exceeds MT_MAX_TREE_DEPTH " + std::to_string(MT_MAX_TREE_DEPTH));

  s = base;
  s.tri_material[7] = -2;
  expect_refusal("material -2", s.desc(), MT_ERR_ARG, "triangle 7: material index -2 outside -1..-1");
  s = base;
  s.materials.resize(2);
  memset(s.materials.data(), 0, 2 * sizeof(mt_material));
  s.materials[0].tex = s.materials[1].tex = -1;
  s.tri_material[9] = 2;
  expect_refusal("material n_materials", s.desc(), MT_ERR_ARG, "triangle 9: material index 2 outside -1..1");
  s.tri_material[9] = 1;
  s.materials[1].tex = 0;
  expect_refusal("texture index", s.desc(), MT_ERR_ARG, "material 1: texture index 0 outside -1..-1");
  s.materials[1].tex = -2;
  expect_refusal("texture index -2", s.desc(), MT_ERR_ARG, "material 1: texture index -2 outside -1..-1");
  const unsigned char texels[12] = {0};
  s.materials[1].tex = 1;
  s.textures = {mt_texture{2, 2, MT_TEX_RGB8, 0, texels}, mt_texture{2, 0, MT_TEX_RGB8, 0, texels}};
  expect_refusal("texture height", s.desc(), MT_ERR_ARG, "texture 1: bad size/format");
  s.textures[1] = mt_texture{2, 2, 7, 0, texels};
  expect_refusal("texture format", s.desc(), MT_ERR_ARG, "texture 1: bad size/format");
  s.textures[1] = mt_texture{2, 2, MT_TEX_RGB8, 0, texels};
  s.textures[0].texels = nullptr;
  expect_refusal("texture texels", s.desc(), MT_ERR_ARG, "texture 0: bad size/format");
  s.textures[0] = mt_texture{30001, 2, MT_TEX_F64, 0, texels};
  expect_refusal("texture width", s.desc(), MT_ERR_ARG, "texture 0: bad size/format");

  // ... and what passes: that scene with its textures mended, a tree of exactly MT_MAX_TREE_DEPTH levels, the least desc
  g_case = "accepted";
  std::vector<int> depth_of;
  int max_depth = 0;
  LayoutError err;
  s.textures[0] = mt_texture{2, 2, MT_TEX_RGB8, 0, texels};
  CHECK(check_scene_desc(s.desc(), &depth_of, &max_depth, &err) && max_depth == 2, "materials and textures: %s", err.msg.c_str());
  s = new_scene("depth");
  for (int level = 1, i = 0; level < MT_MAX_TREE_DEPTH; level++) i = s.split(i);
  CHECK(check_scene_desc(s.desc(), &depth_of, &max_depth, &err) && max_depth == MT_MAX_TREE_DEPTH, "deepest tree: %s", err.msg.c_str());
  s = new_scene("least");
  CHECK(check_scene_desc(s.desc(), &depth_of, &max_depth, &err), "least desc: %s", err.msg.c_str());
  CHECK(max_depth == 1 && depth_of == std::vector<int>{1}, "least desc: max_depth %d", max_depth);
}

// ---- --hash

template <typename T>
unsigned long long fnv(const T *p, size_t n) {
  unsigned long long h = 1469598103934665603ull;
  const unsigned char *b = (const unsigned char *)p;
  for (size_t i = 0; i < n * sizeof(T); i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

template <typename T>
void print_hash(const char *name, const std::vector<T> &v) {
  printf("  %-10s %8zu %016llx\n", name, v.size(), fnv(v.data(), v.size()));
}

void print_hashes(const Scene &s) {
  const mt_scene_desc d = s.desc();
  std::vector<int> depth_of;
  int max_depth = 0;
  LayoutError err;
  if (!check_scene_desc(d, &depth_of, &max_depth, &err)) {
    printf("%s: refused: %s\n", s.name.c_str(), err.msg.c_str());
    return;
  }
  SceneLayout L;
  derive_layout(d, depth_of, &L);
  printf("%s\n", s.name.c_str());
  print_hash("recs", L.recs);
  print_hash("groups", L.groups);
  print_hash("supers", L.supers);
  print_hash("subs", L.subs);
  print_hash("hsr", L.hsr);
  print_hash("sl_box", L.sl_box);
  print_hash("ll_tri", L.ll_tri);
  print_hash("ll_exact", L.ll_exact);
  print_hash("ll_box_q", L.ll_box_q);
  print_hash("ll_grp_q", L.ll_grp_q);
  print_hash("ll_sup_q", L.ll_sup_q);
  print_hash("tri_aabb", L.tri_aabb);
  print_hash("tri_aabb32", L.tri_aabb32);
  printf("  bmax %016llx regular %d max_depth %d\n", fnv(L.bmax, 3), (int)L.regular, L.max_depth);
}

}  // namespace

#ifndef LAYOUT_CHECK_NO_MAIN
int main(int argc, char **argv) {
  const std::vector<Scene> scenes = all_scenes();
  if (argc > 1 && strcmp(argv[1], "--hash") == 0) {
    for (const Scene &s : scenes) print_hashes(s);
    return 0;
  }
  for (const Scene &s : scenes) check_layout(s);
  check_regular();
  check_refusals();
  if (g_failures) {
    fprintf(stderr, "%d check(s) failed\n", g_failures);
    return 1;
  }
  printf("layout_check: %zu scenes, all checks held\n", scenes.size());
  return 0;
}
#endif
