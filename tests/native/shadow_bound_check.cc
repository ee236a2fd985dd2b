// shadow_bound_check.cc — mt_shadow_bound.h without a GPU.  Driven by tests/test_shadow_bound_cpu.py, which builds it
// with the address and undefined-behaviour sanitizers and hands it scene dumps (format: read_scene below).
//
//   (a) no arguments needed (every coordinate of a pair stays within kSbMaxCoord, asserted): the two facts the bound's derivation rests on, on adversarial triangle/ray pairs.  The
//       reference's Moeller-Trumbore in the project's fp64 order (mt_trace.h moller_trumbore_v, copied operation by
//       operation) against long double geometry: a REPORTED hit's distance lies within a (Dt + 2 t*) of the exact
//       plane parameter t* (F1), the exact point within r of the triangle's box (F2), and so the distance is not below
//       the box's exact entry distance minus sigma(t) (H).  Then mu's inequality as the issue states it, for the per-ray
//       mu = tmax - L: a triangle whose exact box entry distance exceeds L + mu is not reported with t <= L + mu / 2.
//   (b) per scene dump: a plain recursive port of the reference's traversal (octtree.cc:169-257 on the flattened tree)
//       runs every shadow iteration twice, once with the walk's bound emptying subtrees and own lists (the kernel's
//       fp32 arithmetic: Filter32 restated for the host, shadow_l32 and shadow_tmax32 as they are), once without: the
//       loop must take the same branch of mythtracer.cc:109-118 in both, and wherever the unbounded hit has t <= L both hits must be the same
//       triangle at the same distance, bit for bit.  Iterations whose bounded run meets the tie of DESIGN 3.1.3 are
//       repeated unbounded by the kernel: counted here (at most one in a hundred, but in the scene planted to have them, which
//       must have some), and compared after that repetition.
// Exit status 0 and "all checks held" = every check held; else the failing cases on stderr.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mt_layout.h"
#include "mt_shadow_bound.h"

using namespace mt;

namespace {

int g_failures = 0;
#define CHECK(cond, ...)                              \
  do {                                                \
    if (!(cond)) {                                    \
      if (g_failures++ < 40) {                        \
        fprintf(stderr, "FAIL %s: ", #cond);          \
        fprintf(stderr, __VA_ARGS__);                 \
        fprintf(stderr, "\n");                        \
      }                                               \
    }                                                 \
  } while (0)

uint64_t g_rng = 88172645463325252ull;
double uniform() {  // [0, 1)
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  return (double)(g_rng >> 11) * 0x1p-53;
}
double between(double lo, double hi) { return lo + (hi - lo) * uniform(); }

// primitive_triangle.cc:110-142 in the project's order of operations (no FMA: built with -ffp-contract=off)
bool moller_trumbore(const double *v, const double *o, const double *d, double *t_out) {
  const double v0x = v[0], v0y = v[1], v0z = v[2];
  const double e1x = v[3] - v0x, e1y = v[4] - v0y, e1z = v[5] - v0z;
  const double e2x = v[6] - v0x, e2y = v[7] - v0y, e2z = v[8] - v0z;
  const double px = d[1] * e2z - d[2] * e2y;
  const double py = d[2] * e2x - d[0] * e2z;
  const double pz = d[0] * e2y - d[1] * e2x;
  const double det = px * e1x + py * e1y + pz * e1z;
  if (det >= -0.00000001 && det < 0.00000001) return false;
  const double inv_det = 1.0 / det;
  const double tx = o[0] - v0x, ty = o[1] - v0y, tz = o[2] - v0z;
  const double u = (px * tx + py * ty + pz * tz) * inv_det;
  if (u < 0.0 || u > 1.0) return false;
  const double qx = ty * e1z - tz * e1y;
  const double qy = tz * e1x - tx * e1z;
  const double qz = tx * e1y - ty * e1x;
  const double vv = (qx * d[0] + qy * d[1] + qz * d[2]) * inv_det;
  if (vv < 0.0 || u + vv > 1.0) return false;
  const double dist = (qx * e2x + qy * e2y + qz * e2z) * inv_det;
  if (dist < 0.0) return false;
  *t_out = dist;
  return true;
}

typedef long double ld;

// exact (long double) parameter at which the line meets the triangle's plane; false when parallel
bool plane_parameter(const double *v, const double *o, const double *d, ld *t) {
  const ld e1[3] = {(ld)v[3] - v[0], (ld)v[4] - v[1], (ld)v[5] - v[2]};
  const ld e2[3] = {(ld)v[6] - v[0], (ld)v[7] - v[1], (ld)v[8] - v[2]};
  const ld n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const ld nd = n[0] * d[0] + n[1] * d[1] + n[2] * d[2];
  if (nd == 0) return false;
  *t = (n[0] * ((ld)v[0] - o[0]) + n[1] * ((ld)v[1] - o[1]) + n[2] * ((ld)v[2] - o[2])) / nd;
  return true;
}

void box_of(const double *v, double *b) {
  for (int a = 0; a < 3; a++) {
    b[a] = std::min(v[a], std::min(v[3 + a], v[6 + a]));
    b[3 + a] = std::max(v[a], std::max(v[3 + a], v[6 + a]));
  }
}

// exact entry parameter of the LINE into the box's three slabs (max of the near planes' parameters)
ld box_entry(const double *b, const double *o, const double *d) {
  ld e = -INFINITY;
  for (int a = 0; a < 3; a++) {
    const ld t0 = ((ld)b[a] - o[a]) / d[a], t1 = ((ld)b[3 + a] - o[a]) / d[a];
    e = std::max(e, std::min(t0, t1));
  }
  return e;
}

struct Pairs {
  long tried = 0, reported = 0;
  double worst_f1 = 0, worst_f2 = 0, worst_h = 0;  // observed slop over its bound
};

// One pair under test.  extent: the scene box's diagonal this pair is imagined in (all its points lie within it).
void check_pair(const double *v, const double *o, const double *d, double longest_edge, const double *scene_box,
                Pairs *P) {
  P->tried++;
  double t;
  if (!moller_trumbore(v, o, d, &t)) return;
  P->reported++;
  const ShadowSlop s = shadow_slop(longest_edge, scene_box);
  ld ts;
  if (!plane_parameter(v, o, d, &ts)) {
    CHECK(false, "a hit was reported for a line exactly parallel to the plane");
    return;
  }
  // F1
  const double f1 = (double)fabsl((ld)t - ts), f1_bound = s.a * (s.dt + 2.0 * (double)fabsl(ts));
  CHECK(f1 <= f1_bound, "F1: |t - t*| = %.3g above a (Dt + 2 t*) = %.3g (t %.17g)", f1, f1_bound, t);
  if (f1_bound > 0) P->worst_f1 = std::max(P->worst_f1, f1 / f1_bound);
  // F2: distance of the exact point from the triangle's box, largest axis excess
  double b[6];
  box_of(v, b);
  double out = 0;
  for (int a = 0; a < 3; a++) {
    const ld p = (ld)o[a] + ts * d[a];
    out = std::max(out, (double)std::max((ld)b[a] - p, p - (ld)b[3 + a]));
  }
  CHECK(out <= s.r, "F2: the exact point lies %.3g outside the box, r = %.3g", out, s.r);
  if (s.r > 0) P->worst_f2 = std::max(P->worst_f2, out / s.r);
  // H, and mu's inequality for this ray
  const double imax = std::max(std::fabs(1.0 / d[0]), std::max(std::fabs(1.0 / d[1]), std::fabs(1.0 / d[2])));
  const double sigma = s.r * imax + s.a * (s.dt + 2.0 * t);
  const double entry = (double)box_entry(b, o, d);
  CHECK(t >= entry - sigma, "H: t = %.17g below the box's entry %.17g - sigma %.3g", t, entry, sigma);
  if (sigma > 0 && entry > t) P->worst_h = std::max(P->worst_h, (entry - t) / sigma);
  // mu(L) = tmax - L with tmax = (L + 3 a Dt + 3 r imax) / (1 - 6 a): were the entry beyond L + mu for some L >= 0, the
  // hit must not come with t <= L + mu / 2.  The largest L with entry > L + mu(L) is where they are equal.
  const double k = 1.0 / (1.0 - 6.0 * s.a), c = (3.0 * s.a * s.dt + 3.0 * s.r * imax) * k;  // tmax = k L + c
  const double L = (entry - c) / k;  // entry = tmax(L)
  if (L >= 0) {
    const double mu = entry - L;
    CHECK(t > L + mu / 2.0, "mu: a hit at t = %.17g <= L + mu / 2 = %.17g + %.3g behind a box entered at L + mu = %.17g", t, L,
          mu / 2.0, entry);
  }
}

void unit(double *d) {
  const double n = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  for (int a = 0; a < 3; a++) d[a] /= n;
}

void adversarial_pairs() {
  Pairs P;
  const double scales[] = {1.0, 40.0, 340.0};  // longest edges up to the eligibility limit (a <= 1/64: E <= 342)
  // coordinates up to the eligibility limit kSbMaxCoord = 2^40 (one ulp there is 2^-12), the scene box around them
  const double offsets[] = {0.0, 600.0, 0x1p30, kSbMaxCoord - 2048.0};
  for (double E : scales) {
    for (double off : offsets) {
      const double ext = std::max(1000.0, std::min(2.2 * off, kSbMaxCoord));
      const double scene_box[6] = {-ext, -ext, -ext, ext, ext, ext};
      for (int it = 0; it < 6000; it++) {
        // a triangle of longest edge <= E: general, or a sliver (third vertex almost on the first edge)
        double v[9];
        const bool sliver = it % 3 == 1;
        for (int a = 0; a < 3; a++) v[a] = off + between(-100, 100);
        double e1[3] = {between(-1, 1), between(-1, 1), between(-1, 1)};
        unit(e1);
        const double l1 = E * between(0.3, 0.7);
        double e2[3] = {between(-1, 1), between(-1, 1), between(-1, 1)};
        unit(e2);
        for (int a = 0; a < 3; a++) {
          v[3 + a] = v[a] + l1 * e1[a];
          v[6 + a] = sliver ? v[a] + 0.5 * l1 * e1[a] + 1e-3 * E * e2[a] : v[a] + E * between(0.2, 0.29) * (e1[a] + e2[a]);
        }
        const double f1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]}, f2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
        double n[3] = {f1[1] * f2[2] - f1[2] * f2[1], f1[2] * f2[0] - f1[0] * f2[2], f1[0] * f2[1] - f1[1] * f2[0]};
        const double area2 = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (!(area2 > 0)) continue;
        unit(n);
        // a target point: inside, on an edge, or just outside the triangle (what a sloppy u, v lets through)
        const double bu = between(-0.02, 1.02), bv = between(-0.02, 1.02 - std::max(bu, 0.0));
        double target[3];
        for (int a = 0; a < 3; a++) target[a] = v[a] + bu * f1[a] + bv * f2[a];
        // a direction: an in-plane unit vector plus a normal share that puts det = 2 area (n . d) where wanted --
        // just outside the threshold on either side, a few thresholds, or a plain transversal ray
        double w[3] = {between(-1, 1), between(-1, 1), between(-1, 1)};
        const double wn = w[0] * n[0] + w[1] * n[1] + w[2] * n[2];
        for (int a = 0; a < 3; a++) w[a] -= wn * n[a];
        unit(w);
        const int kind = it % 5;
        const double want_det = kind == 0 ? 1.0000001e-8 : kind == 1 ? -1.0000001e-8 : kind == 2 ? between(1e-8, 1e-6)
                                : kind == 3 ? -between(1e-8, 1e-5) : area2 * between(-1, 1);
        const double nd = std::max(-0.99, std::min(0.99, want_det / area2));
        double d[3];
        for (int a = 0; a < 3; a++) d[a] = std::sqrt(1.0 - nd * nd) * w[a] + nd * n[a];
        unit(d);
        if (d[0] == 0.0 || d[1] == 0.0 || d[2] == 0.0) continue;  // (the walk does not take such rays)
        // the origin: t* behind the target along the ray, t* at the values the issue lists around a light distance L
        const double Lr = between(0.5, 500.0);
        const double mu = 3.0 * shadow_slop(E, scene_box).a * shadow_slop(E, scene_box).dt;
        const double ts_choices[] = {Lr, Lr * (1 + 3 * 0x1p-52), Lr * (1 - 3 * 0x1p-52), Lr + 1e-5, Lr - 1e-5,
                                     Lr + mu * (1 + 1e-9), Lr + mu * (1 - 1e-9), Lr + 0.5 * mu, between(0, 800)};
        const double ts = ts_choices[(it / 5) % 9];
        double o[3];
        for (int a = 0; a < 3; a++) o[a] = target[a] - ts * d[a];
        bool inside = true;  // every point of the pair within the scene box, which is within the eligibility limit
        for (int a = 0; a < 3; a++) {
          inside = inside && std::fabs(o[a]) <= ext;
          for (int j = 0; j < 3; j++) inside = inside && std::fabs(v[j * 3 + a]) <= ext;
        }
        if (!inside || ext > kSbMaxCoord) continue;
        check_pair(v, o, d, E, scene_box, &P);
      }
    }
  }
  printf("(a) %ld pairs, %ld reported; worst observed slop over its bound: F1 %.3g, F2 %.3g, H %.3g\n", P.tried, P.reported,
         P.worst_f1, P.worst_f2, P.worst_h);
  CHECK(P.reported > P.tried / 20, "too few of the pairs are reported hits: %ld of %ld", P.reported, P.tried);
}

// ---- (b) ------------------------------------------------------------------------------------------------------------

struct Scene {
  int n_nodes = 0, n_tris = 0, n_lights = 0, w = 0, h = 0, max_level = 0;
  std::vector<double> node_aabb, node_center;
  std::vector<int32_t> first_child, prim_begin, prim_count;
  std::vector<double> vertex, normal, aabb;  // per stream triangle 9, 9, 6
  std::vector<double> reflectance, transparency;  // per stream triangle (its material's; -1 = no material)
  std::vector<double> lights;  // 3 per light
  double sensor[12];  // origin, start point, delta scanline, delta pixel
  // mt_layout.h's: fp32 union boxes of every node's subtree and own list, bmax
  std::vector<float> sub32, own32;
  double bmax[3];
  ShadowBound sb;
  std::string name;
};

template <typename T>
bool read_vec(FILE *f, std::vector<T> *v, size_t n) {
  v->resize(n);
  return n == 0 || fread(v->data(), sizeof(T), n, f) == n;
}

// int32 x 6: n_nodes, n_tris, n_lights, w, h, max_level; then the arrays in the order of the members above
bool read_scene(const char *path, Scene *s) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  int32_t head[6];
  bool ok = fread(head, 4, 6, f) == 6;
  if (ok) {
    s->n_nodes = head[0]; s->n_tris = head[1]; s->n_lights = head[2]; s->w = head[3]; s->h = head[4]; s->max_level = head[5];
    ok = s->n_nodes > 0 && s->n_tris > 0 && s->n_nodes < (1 << 24) && s->n_tris < (1 << 24) && s->n_lights >= 0 && s->n_lights < 64;
  }
  const size_t nn = ok ? (size_t)s->n_nodes : 0, nt = ok ? (size_t)s->n_tris : 0;
  ok = ok && read_vec(f, &s->node_aabb, nn * 6) && read_vec(f, &s->node_center, nn * 3) && read_vec(f, &s->first_child, nn) &&
       read_vec(f, &s->prim_begin, nn) && read_vec(f, &s->prim_count, nn) && read_vec(f, &s->vertex, nt * 9) &&
       read_vec(f, &s->normal, nt * 9) && read_vec(f, &s->aabb, nt * 6) && read_vec(f, &s->reflectance, nt) &&
       read_vec(f, &s->transparency, nt) && read_vec(f, &s->lights, (size_t)s->n_lights * 3) &&
       fread(s->sensor, 8, 12, f) == 12;
  fclose(f);
  if (!ok) return false;
  for (size_t i = 0; i < nn; i++) {  // what the recursion indexes unchecked
    const int fc = s->first_child[i], pb = s->prim_begin[i], pc = s->prim_count[i];
    if (pb < 0 || pc < 0 || (size_t)pb + (size_t)pc > nt || (fc != 0 && (fc <= (int)i || (size_t)fc + 8 > nn))) return false;
  }
  return true;
}

// What the kernels read, from the project's own derivation (mt_layout.h derive_layout): the fp32 union boxes of every
// node's subtree (DevScene::sub_aabb32, which HsRec::kid repeats per parent) and own list (HsRec::own), bmax, the bound.
void derive(Scene *s) {
  const size_t nn = (size_t)s->n_nodes, nt = (size_t)s->n_tris;
  std::vector<int32_t> zeros(nt, 0);
  mt_scene_desc d;
  memset(&d, 0, sizeof d);
  d.struct_size = sizeof d;
  d.abi_version = MT_ABI_VERSION;
  d.n_nodes = s->n_nodes;
  d.n_tris = s->n_tris;
  d.node_aabb = s->node_aabb.data();
  d.node_center = s->node_center.data();
  d.node_first_child = s->first_child.data();
  d.node_prim_begin = s->prim_begin.data();
  d.node_prim_count = s->prim_count.data();
  d.tri_vertex = s->vertex.data();
  d.tri_normal = s->normal.data();
  d.tri_uvw = s->normal.data();  // (stand-in: no derived array reads it)
  d.tri_aabb = s->aabb.data();
  d.tri_material = zeros.data();
  d.tri_line_no = zeros.data();
  std::vector<int> depth_of(nn, 0);  // (read_scene checked the links: children lie behind their parent)
  depth_of[0] = 1;
  for (size_t i = 0; i < nn; i++) {
    for (int c = 0; s->first_child[i] != 0 && c < 8; c++) depth_of[(size_t)s->first_child[i] + c] = depth_of[i] + 1;
  }
  SceneLayout L;
  derive_layout(d, depth_of, &L);
  s->sub32.assign(L.subs.begin(), L.subs.begin() + nn * 6);
  s->own32.resize(nn * 6);
  for (size_t i = 0; i < nn; i++) {
    for (int a = 0; a < 3; a++) {
      s->own32[i * 6 + a] = L.hsr[i].own[a][0];
      s->own32[i * 6 + 3 + a] = L.hsr[i].own[a][1];
    }
  }
  for (int k = 0; k < 3; k++) s->bmax[k] = L.bmax[k];
  s->sb = L.shadow;
  const ShadowBoundInput in{s->n_nodes, s->n_tris, s->node_aabb.data(), s->node_center.data(), s->first_child.data(),
                            s->prim_begin.data(), s->prim_count.data(), s->vertex.data(), s->aabb.data()};
  const char *why = "";
  const ShadowBound again = shadow_bound_for(in, &why);
  CHECK(memcmp(&again, &s->sb, sizeof again) == 0, "%s: derive_layout's bound is not shadow_bound_for's", s->name.c_str());
  printf("(b) %s: %d nodes, %d triangles; bound %s%s: 1 + rho = %.9g, mu = %.6g, kappa = %.6g\n", s->name.c_str(), s->n_nodes,
         s->n_tris, s->sb.on ? "on" : "OFF: ", why, (double)s->sb.rho1, (double)s->sb.mu, (double)s->sb.kappa);
}

struct Ray {
  double o[3], d[3], i[3];
  // the walk's fp32 filter (mt_trace.h make_filter32) and bound
  float I[3], Cn[3];
  bool f32_ok;
  float tmax;  // +inf: unbounded
  bool tie;    // the bounded run met the tie the kernel answers kTraceRedo for
  bool counted;  // a shadow iteration: its node visits are counted
};

float f32_pred(float f) { return std::nextafterf(f, -INFINITY); }

void make_ray(const Scene &s, const double *o, const double *d, Ray *r) {
  r->f32_ok = true;
  for (int k = 0; k < 3; k++) {
    r->o[k] = o[k]; r->d[k] = d[k]; r->i[k] = 1.0 / d[k];
    const double M = (s.bmax[k] + std::fabs(o[k])) * std::fabs(r->i[k]);
    r->f32_ok = r->f32_ok && (M <= 0x1p120) && std::fabs(r->i[k]) >= 0x1p-126 && std::isfinite(r->i[k]);
    const double E = M * 0x1p-21 + 0x1p-100;
    const double c = -(o[k] * r->i[k]) - E;
    r->I[k] = (float)r->i[k];
    float f = (float)c;
    if ((double)f > c) f = f32_pred(f);
    r->Cn[k] = f;
  }
  r->tmax = INFINITY;
  r->tie = false;
  r->counted = false;
}

// the walk's conservative entry distance of an fp32 box (near_far_may_hit's lo0)
float entry32(const float *b, const Ray &r) {
  float lo = 0.0f;
  for (int k = 0; k < 3; k++) lo = std::fmax(lo, std::fmaf(std::signbit(r.i[k]) ? b[3 + k] : b[k], r.I[k], r.Cn[k]));
  return lo;
}

bool slab(const double *b, const Ray &r, double *dist) {  // octtree.cc:138-167 / primitive_triangle.cc:85-108
  const double t1 = (b[0] - r.o[0]) * r.i[0], t2 = (b[3] - r.o[0]) * r.i[0];
  const double t3 = (b[1] - r.o[1]) * r.i[1], t4 = (b[4] - r.o[1]) * r.i[1];
  const double t5 = (b[2] - r.o[2]) * r.i[2], t6 = (b[5] - r.o[2]) * r.i[2];
  const double tmax = std::min({std::max(t1, t2), std::max(t3, t4), std::max(t5, t6)});
  if (tmax < 0.0) return false;
  const double tmin = std::max({std::min(t1, t2), std::min(t3, t4), std::min(t5, t6)});
  if (tmin > tmax) return false;
  *dist = tmin;
  return true;
}
bool slab_degenerate(const double *b, const Ray &r) {
  const double t1 = (b[0] - r.o[0]) * r.i[0], t2 = (b[3] - r.o[0]) * r.i[0];
  const double t3 = (b[1] - r.o[1]) * r.i[1], t4 = (b[4] - r.o[1]) * r.i[1];
  const double t5 = (b[2] - r.o[2]) * r.i[2], t6 = (b[5] - r.o[2]) * r.i[2];
  return std::min({std::max(t1, t2), std::max(t3, t4), std::max(t5, t6)}) ==
         std::max({std::min(t1, t2), std::min(t3, t4), std::min(t5, t6)});
}

long g_visits[2] = {0, 0};  // node visits, unbounded and bounded
bool g_tie_handling = true;  // --without-tie-handling: the bounded run decides ties like everything else (must FAIL on the tie scene)
long g_ties[2] = {0, 0};    // tie events of either kind

// Node::PrimitiveIntersectRay, octtree.cc:169-257.  With r.tmax finite, subtrees and own lists the walk would skip are
// empty.  Returns the triangle or -1.
int node_intersect(const Scene &s, int node, Ray &r, double *dist) {
  const bool bounded = r.tmax < INFINITY;
  if (r.counted) g_visits[bounded ? 1 : 0]++;
  int best = -1;
  double best_t = 0.0;
  const bool own_skipped = bounded && entry32(&s.own32[(size_t)node * 6], r) > r.tmax;
  for (int t = s.prim_begin[node]; !own_skipped && t < s.prim_begin[node] + s.prim_count[node]; t++) {
    double bd, tt;
    if (!slab(&s.aabb[(size_t)t * 6], r, &bd)) continue;
    if (!moller_trumbore(&s.vertex[(size_t)t * 9], r.o, r.d, &tt)) continue;
    if (best >= 0 && tt > best_t) continue;
    best = t;
    best_t = tt;
  }
  const int fc = s.first_child[node];
  if (fc != 0) {
    int order[8], n = 0;
    double key[8];
    for (int c = 0; c < 8; c++) {
      double dd;
      if (!slab(&s.node_aabb[(size_t)(fc + c) * 6], r, &dd)) continue;
      int at = n++;  // std::sort on at most eight elements is an insertion sort: stable
      while (at > 0 && dd < key[at - 1]) { key[at] = key[at - 1]; order[at] = order[at - 1]; at--; }
      key[at] = dd;
      order[at] = c;
    }
    for (int k = 0; k < n; k++) {
      const int child = fc + order[k];
      if (bounded && entry32(&s.sub32[(size_t)child * 6], r) > r.tmax) continue;  // emptied: "nothing found"
      double tt;
      const int p = node_intersect(s, child, r, &tt);
      if (p < 0) continue;
      if (bounded && g_tie_handling && slab_degenerate(&s.node_aabb[(size_t)child * 6], r)) { r.tie = true; g_ties[0]++; }  // (offer(): tmin == tmax)
      if (best >= 0 && tt > best_t) continue;
      best = p;
      best_t = tt;
      // (offer(): a bounded lane keeps the children at its candidate's key, so that none that is entered and left at one
      // parameter goes unseen; their results change nothing)
      for (int k2 = k + 1; bounded && g_tie_handling && k2 < n && key[k2] == key[k]; k2++) {
        const int tied = fc + order[k2];
        if (entry32(&s.sub32[(size_t)tied * 6], r) > r.tmax) continue;
        double t2;
        g_ties[1]++;
        if (node_intersect(s, tied, r, &t2) >= 0 && slab_degenerate(&s.node_aabb[(size_t)tied * 6], r)) { r.tie = true; g_ties[0]++; }
      }
      break;
    }
  }
  if (best < 0) return -1;
  *dist = best_t;
  return best;
}

int intersect(const Scene &s, Ray &r, double *dist) {  // OctTree::IntersectRay, octtree.cc:26-40
  double dd;
  if (!slab(&s.node_aabb[0], r, &dd)) return -1;
  return node_intersect(s, 0, r, dist);
}

struct Tally {
  long iterations = 0, near_hits = 0, far_or_none = 0, redone = 0;
};

double dist3(const double *a, const double *b) {
  return std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
}

// One iteration of the shadow loop, both ways.  Returns the unbounded result (the reference's).
int shadow_iteration(const Scene &s, const double *start, const double *dir, const double *light, double *t_out,
                     Tally *T) {
  double o[3];
  for (int k = 0; k < 3; k++) o[k] = start[k] + dir[k] * 0.00001;
  const double L = dist3(start, light);
  Ray a, b;
  make_ray(s, o, dir, &a);
  make_ray(s, o, dir, &b);
  a.counted = b.counted = true;
  double ta = 0, tb = 0;
  const int pa = intersect(s, a, &ta);
  int pb = pa;
  tb = ta;
  T->iterations++;
  const bool regular = a.f32_ok && std::isfinite(L) && dir[0] != 0.0 && dir[1] != 0.0 && dir[2] != 0.0;
  if (s.sb.on && regular) {
    const double d2 = (o[0] - light[0]) * (o[0] - light[0]) + (o[1] - light[1]) * (o[1] - light[1]) + (o[2] - light[2]) * (o[2] - light[2]);
    b.tmax = shadow_tmax32(s.sb, shadow_l32(d2), std::fmax(std::fmax(std::fabs(b.I[0]), std::fabs(b.I[1])), std::fabs(b.I[2])));
    pb = intersect(s, b, &tb);
    if (b.tie) {  // kTraceRedo: the same ray without a bound
      T->redone++;
      b.tmax = INFINITY;
      b.counted = false;
      pb = intersect(s, b, &tb);
    }
  }
  // mythtracer.cc:109-118: 0 = nothing found, 1 = behind the light, 2 = an occluder within the light's distance
  const int branch_a = pa < 0 ? 0 : (ta > L ? 1 : 2), branch_b = pb < 0 ? 0 : (tb > L ? 1 : 2);
  CHECK((branch_a == 2) == (branch_b == 2), "%s: the loop takes branch %d unbounded and %d bounded (L %.17g, t %.17g / %.17g)",
        s.name.c_str(), branch_a, branch_b, L, ta, tb);
  if (branch_a == 2) {
    T->near_hits++;
    CHECK(pa == pb && memcmp(&ta, &tb, 8) == 0, "%s: hit %d at %.17g unbounded, %d at %.17g bounded (L %.17g)", s.name.c_str(),
          pa, ta, pb, tb, L);
  } else {
    T->far_or_none++;
  }
  *t_out = ta;
  return pa;
}

void normalize(double *v) {
  const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  for (int k = 0; k < 3; k++) v[k] /= n;
}

// TraceRayWorker's control flow (mythtracer.cc:16-230) without its colours: which rays are shot, and from where.  The
// normal is interpolated with plain barycentric weights (the rays differ from a render's in the last bits; the set of
// situations is the render's).
void trace(const Scene &s, const double *o, const double *d, int level, bool in_object, double coef, Tally *T) {
  Ray r;
  make_ray(s, o, d, &r);
  double t;
  const int p = intersect(s, r, &t);
  if (p < 0) return;
  if (s.transparency[(size_t)p] < 0.0) return;  // no material: no lights
  double pt[3], nn[3];
  for (int k = 0; k < 3; k++) pt[k] = o[k] + d[k] * t;
  {
    const double *v = &s.vertex[(size_t)p * 9], *n = &s.normal[(size_t)p * 9];
    const double e1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]}, e2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
    const double q[3] = {pt[0] - v[0], pt[1] - v[1], pt[2] - v[2]};
    const double d11 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], d12 = e1[0] * e2[0] + e1[1] * e2[1] + e1[2] * e2[2];
    const double d22 = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2];
    const double q1 = q[0] * e1[0] + q[1] * e1[1] + q[2] * e1[2], q2 = q[0] * e2[0] + q[1] * e2[1] + q[2] * e2[2];
    const double den = d11 * d22 - d12 * d12;
    const double bu = den != 0 ? (d22 * q1 - d12 * q2) / den : 0, bv = den != 0 ? (d11 * q2 - d12 * q1) / den : 0;
    for (int k = 0; k < 3; k++) nn[k] = n[k] * (1 - bu - bv) + n[3 + k] * bu + n[6 + k] * bv;
    if (!(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2] > 0)) {  // (a file without normals)
      nn[0] = e1[1] * e2[2] - e1[2] * e2[1]; nn[1] = e1[2] * e2[0] - e1[0] * e2[2]; nn[2] = e1[0] * e2[1] - e1[1] * e2[0];
    }
    normalize(nn);
    if (-(nn[0] * d[0] + nn[1] * d[1] + nn[2] * d[2]) < 0) { nn[0] = -nn[0]; nn[1] = -nn[1]; nn[2] = -nn[2]; }
  }
  for (int li = 0; li < s.n_lights; li++) {
    const double *light = &s.lights[(size_t)li * 3];
    double ld_[3] = {light[0] - pt[0], light[1] - pt[1], light[2] - pt[2]};
    normalize(ld_);
    double start[3] = {pt[0], pt[1], pt[2]};
    double power = 1.0;
    bool through = false;
    for (int guard = 0; guard < 64; guard++) {
      double st;
      const int sp = shadow_iteration(s, start, ld_, light, &st, T);
      if (sp < 0) break;
      if (st > dist3(start, light)) break;
      const double tr = s.transparency[(size_t)sp] < 0 ? 0.0 : s.transparency[(size_t)sp];
      if (tr == 0.0) break;
      if (!through) power *= tr;
      through = !through;
      double so[3];
      for (int k = 0; k < 3; k++) so[k] = start[k] + ld_[k] * 0.00001;
      for (int k = 0; k < 3; k++) start[k] = (so[k] + ld_[k] * st) + ld_[k] * 0.0000001;
      const double a2 = (pt[0] - start[0]) * (pt[0] - start[0]) + (pt[1] - start[1]) * (pt[1] - start[1]) + (pt[2] - start[2]) * (pt[2] - start[2]);
      const double b2 = (pt[0] - light[0]) * (pt[0] - light[0]) + (pt[1] - light[1]) * (pt[1] - light[1]) + (pt[2] - light[2]) * (pt[2] - light[2]);
      if (a2 > b2) break;
      if (power <= 0.001) break;
    }
  }
  const double refl = s.reflectance[(size_t)p], tr = s.transparency[(size_t)p];
  if (level < s.max_level && refl > 0.0 && coef > 0.01 && !in_object) {
    const double dn = 2 * (d[0] * nn[0] + d[1] * nn[1] + d[2] * nn[2]);
    double rd[3] = {d[0] - nn[0] * dn, d[1] - nn[1] * dn, d[2] - nn[2] * dn}, ro[3];
    for (int k = 0; k < 3; k++) ro[k] = pt[k] + rd[k] * 0.0001;
    trace(s, ro, rd, level + 1, in_object, coef * refl, T);
  }
  if (level < s.max_level && tr > 0.0) {
    double rd[3] = {d[0], d[1], d[2]}, ro[3];
    normalize(rd);
    for (int k = 0; k < 3; k++) ro[k] = pt[k] + rd[k] * 0.00001;
    trace(s, ro, rd, level + 1, !in_object, coef, T);
  }
}

void scene_rays(const char *path) {
  Scene s;
  s.name = path;
  if (!read_scene(path, &s)) {
    CHECK(false, "cannot read the scene dump %s", path);
    return;
  }
  const size_t slash = s.name.find_last_of('/');
  if (slash != std::string::npos) s.name = s.name.substr(slash + 1);
  derive(&s);
  const bool expect_on = s.name.find("poking") == std::string::npos;
  CHECK((s.sb.on != 0) == expect_on, "%s: the bound is %s", s.name.c_str(), s.sb.on ? "on" : "off");
  Tally T;
  g_visits[0] = g_visits[1] = g_ties[0] = g_ties[1] = 0;
  const double *S = s.sensor;
  for (int y = 0; y < s.h; y++) {
    for (int x = 0; x < s.w; x++) {
      double d[3];
      for (int k = 0; k < 3; k++) d[k] = S[3 + k] + S[6 + k] * (double)y + S[9 + k] * (double)x;
      normalize(d);
      trace(s, S, d, 0, false, 1.0, &T);
    }
  }
  printf("(b) %s: %ld shadow iterations (%ld with an occluder within the light's distance, %ld without), %ld repeated unbounded\n",
         s.name.c_str(), T.iterations, T.near_hits, T.far_or_none, T.redone);
  printf("(b) %s: the shadow iterations' node visits: %ld unbounded, %ld bounded (%.3f); ties: %ld children with a hit entered at one parameter, %ld children seen at a candidate's key\n", s.name.c_str(),
         g_visits[0], g_visits[1], (double)g_visits[1] / (double)g_visits[0], g_ties[0], g_ties[1]);
  CHECK(T.iterations > 1000 && T.near_hits > 0 && T.far_or_none > 0, "%s: the rays do not cover both outcomes", s.name.c_str());
  if (s.name.find("tie") != std::string::npos && g_tie_handling) {
    CHECK(T.redone > 0 && g_ties[0] > 0, "%s: no iteration met a tie that brought a hit: the scene does not test the repetition", s.name.c_str());
  }
  else CHECK(T.redone * 100 <= T.iterations, "%s: %ld of %ld iterations repeated", s.name.c_str(), T.redone, T.iterations);
}

}  // namespace

int main(int argc, char **argv) {
  adversarial_pairs();
  for (int i = 1; i < argc; i++) {
    if (std::string(argv[i]) == "--without-tie-handling") g_tie_handling = false;
    else scene_rays(argv[i]);
  }
  if (g_failures) {
    fprintf(stderr, "%d checks failed\n", g_failures);
    return 1;
  }
  printf("all checks held\n");
  return 0;
}
