// mt_shadow_bound.h — how far an iteration of the shadow loop (mythtracer.cc:94-156) has to look.
//
// Free of HIP calls: scene creation computes a ShadowBound on the host (mt_layout.h), the frame kernels evaluate
// shadow_l32 and shadow_tmax32 per lane, and tests/native/shadow_bound_check.cc checks both without a GPU.
//
// The loop's iteration from `start` towards a light asks for the reference's traversal result (prim, t) and then only
// looks at "prim == nullptr" and "t > L", L = start.Distance(light.position) (mythtracer.cc:101-118).  The hit-set walk
// (mt_trace.h) may therefore skip, for that one ray, every subtree and every own list whose union box the ray enters
// beyond
//
//     tmax = L (1 + rho) + mu + kappa * imax,      imax = max |1 / d_k| over the ray's direction d,
//
// provided the scene is ELIGIBLE (below).  DESIGN.md section 3.1.3 proves that the walk's result is then the
// reference's whenever the reference's has t <= L, and is "none" or has t > L otherwise.  The proof needs two facts
// about a hit that the reference's Triangle::IntersectRay (primitive_triangle.cc:110-142) REPORTS at distance t for a
// triangle with box B; this header derives them and the three constants.
//
// ---- the arithmetic's slop.  u = 2^-53, |d| <= 1 + 2^-40 (a normalised direction), tau = 1e-8 (the determinant's
// threshold, :118), E = the scene's longest triangle edge, Dt >= |origin - vertex| for every ray origin the shadow loop
// can produce (a hit point of the scene, 1e-5 along the ray: the scene box's diagonal and a little).  Every value
// below is a 3 x 3 determinant evaluated as cross product, then dot product, without FMA: a cross product's component
// fl(fl(a b) - fl(c e)) is off by at most 3 u (|a b| + |c e|) (two products, one difference; the inputs e1, e2, tvec
// carry one rounding of their own), a dot product of three terms adds 4 u |x| |y|.  With the 2-norm of the component-wise
// bound at most sqrt(3) |x| |y| that is, to first order,
//     |det - det*|  <= 10 u |d| |e1| |e2|          |Nt - Nt*| <= 11 u |tvec| |e1| |e2|     (Nt = e2 . qvec)
//     |Nu - Nu*|    <= 10 u |d| |e2| |tvec|        |Nv - Nv*| <= 10 u |d| |tvec| |e1|
// (starred: the exact value for the same fp64 inputs), and each quotient carries 2 u more.  12 u below pays for the
// second order.  A reported hit has |det| >= tau, so with
//     a = 12 u E^2 / tau
// (F1) |t - t*| <= a (Dt + 2 t*), t* = the parameter at which the ray meets the triangle's plane: from
//      t - t* = (Nt - Nt*) / det - t* (det - det*) / det;
// (F2) the point o + t* d lies within r = 4 a (Dt + 2 E) of the triangle, hence of B: its exact barycentric coordinates
//      differ from the computed, accepted ones by at most du, dv <= 10 u E (Dt + 2 E) / tau (|u*|, |v*| <= 2), and
//      moving the point back into the triangle costs at most (du + dv) * 2 E.
// F2 is what a distance bound must not forget: a grazing ray (|det| just outside the threshold) can be "hit" at a point
// beside the triangle, EARLIER than it enters B.  A point of the ray within r of B has a parameter not below the entry
// into B widened by r, and max_k (n_k - r |1/d_k|) >= max_k n_k - r imax for the slab distances n_k.  So with
//     sigma(t) = r imax + a (Dt + 2 t):
// (H)  a hit reported at t for a triangle whose box lies in a box S has t >= entry(S) - sigma(t),
//      and t <= exit(S) + sigma(t) in the same way.
// The proof spends sigma three times (a skipped hit, and a hop over two neighbouring cells), so it wants
//     tmax - 3 sigma(tmax) >= L    <=    tmax = (L + 3 a Dt + 3 r imax) / (1 - 6 a),
// which is the form above with rho = 6 a / (1 - 6 a), mu = 3 a Dt (1 + rho), kappa = 3 r (1 + rho).  On top of that:
//   * the caller measures L from the ray's origin, 1e-5 |d| behind `start`: mu gets 2e-5 more;
//   * the walk compares a conservative fp32 value that is not above the fp64 slab distances (Filter32), which are the
//     exact ones up to a factor 1 +- 2^-51; shadow_tmax32 evaluates in fp32 (square root within 1 ulp, three roundings):
//     all three constants are multiplied by 1 + 2^-18 and rounded up to fp32.
// In the `room` scene (E = 50: the mirror panel) a = 3.3e-4: rho = 0.002, mu = 0.6, kappa = 2.4 scene units.
//
// ---- eligibility, decided once per scene (shadow_bound_for).  (H) is used for subtrees, own lists and CELLS: a
// node's cell is the octant of its parent's nine planes (the root's: its box), which is what the walk and the
// reference test a child against.  So: all coordinates finite and at most 2^40; every inner node's centre inside its
// box; every child's own box IS its octant; every triangle's vertices lie in its box and its box in its owner's cell
// (the cells nest, so in every ancestor's too); a <= 1/64; mu finite and at most the scene's diagonal.  A scene that
// fails gets on = 0 and traces as before.  A non-finite L or direction gives a non-finite or NaN tmax: no skipping
// (every comparison with it is false).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MT_SB_HD __host__ __device__
#else
#define MT_SB_HD
#endif

namespace mt {

struct ShadowBound {
  float rho1;   // 1 + rho
  float mu;
  float kappa;
  int32_t on;   // 0: the scene gets no bound
};

// smallest fp32 not below a finite double
MT_SB_HD inline float sb_f32_not_below(double c) {
  float f = (float)c;
  if ((double)f < c) {
    uint32_t b;
    memcpy(&b, &f, 4);
    if ((b & 0x7fffffffu) == 0u) b = 0x00000001u;
    else b = (b & 0x80000000u) ? b - 1u : b + 1u;
    memcpy(&f, &b, 4);
  }
  return f;
}

// What the caller hands to the walk: L in fp32 from the SQUARED distance between the ray's origin and the light (not
// below the exact value but for the square root's last bit, which the constants' margin pays) ...
MT_SB_HD inline float shadow_l32(double dist2) { return sqrtf(sb_f32_not_below(dist2)); }
// ... and what the walk makes of it where 1 / d is at hand: imax = max |1 / d_k|, fp32
MT_SB_HD inline float shadow_tmax32(const ShadowBound &b, float l32, float imax) {
  return (l32 * b.rho1 + b.mu) + b.kappa * imax;
}

// The description's arrays that the bound reads (mt_scene_desc's, without the header).
struct ShadowBoundInput {
  int n_nodes, n_tris;
  const double *node_aabb, *node_center;
  const int32_t *node_first_child, *node_prim_begin, *node_prim_count;
  const double *tri_vertex, *tri_aabb;
};

constexpr double kSbTau = 0.00000001;  // primitive_triangle.cc:118
constexpr double kSbMaxCoord = 0x1p40;

// The exact-arithmetic constants (before the fp32 margins): a, r, Dt from the longest edge and the root box.
struct ShadowSlop {
  double a, r, dt, diag;
};
inline ShadowSlop shadow_slop(double longest_edge, const double *root_box) {
  ShadowSlop s;
  double d2 = 0.0;
  for (int k = 0; k < 3; k++) d2 += (root_box[3 + k] - root_box[k]) * (root_box[3 + k] - root_box[k]);
  s.diag = std::sqrt(d2) * (1.0 + 0x1p-30);
  s.dt = s.diag + 1e-3;
  s.a = 12.0 * 0x1p-53 * longest_edge * longest_edge / kSbTau;
  s.r = 4.0 * s.a * (s.dt + 2.0 * longest_edge);
  return s;
}

// octant k of the box (lo, hi) split at c: child index bits 0 = x high, 1 = z high, 2 = y high (octtree.cc:61-100)
inline void sb_octant(const double *lo, const double *c, const double *hi, int k, double *out) {
  const bool high[3] = {(k & 1) != 0, (k & 4) != 0, (k & 2) != 0};
  for (int a = 0; a < 3; a++) {
    out[a] = high[a] ? c[a] : lo[a];
    out[3 + a] = high[a] ? hi[a] : c[a];
  }
}

// The scene's bound, or on = 0.  `why` (optional) names the first condition that failed.
inline ShadowBound shadow_bound_for(const ShadowBoundInput &d, const char **why = nullptr) {
  ShadowBound off{1.0f, 0.0f, 0.0f, 0};
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  auto no = [&](const char *w) { *why = w; return off; };
  if (d.n_nodes < 1 || d.n_tris < 1) return no("no triangles");
  auto sane = [](const double *p, size_t n) {
    for (size_t i = 0; i < n; i++) {
      if (!(std::fabs(p[i]) <= kSbMaxCoord)) return false;
    }
    return true;
  };
  if (!sane(d.node_aabb, (size_t)d.n_nodes * 6) || !sane(d.node_center, (size_t)d.n_nodes * 3) ||
      !sane(d.tri_aabb, (size_t)d.n_tris * 6) || !sane(d.tri_vertex, (size_t)d.n_tris * 9)) {
    return no("a coordinate is not finite or beyond 2^40");
  }
  double e2max = 0.0;
  for (int t = 0; t < d.n_tris; t++) {
    const double *v = d.tri_vertex + (size_t)t * 9, *b = d.tri_aabb + (size_t)t * 6;
    for (int a = 0; a < 3; a++) {
      if (!(b[a] <= b[3 + a])) return no("a triangle's box is inverted");
      for (int j = 0; j < 3; j++) {
        if (!(b[a] <= v[j * 3 + a] && v[j * 3 + a] <= b[3 + a])) return no("a triangle's vertex lies outside its box");
      }
    }
    for (int j = 0; j < 3; j++) {
      const double *p = v + j * 3, *q = v + ((j + 1) % 3) * 3;
      const double l2 = (p[0] - q[0]) * (p[0] - q[0]) + (p[1] - q[1]) * (p[1] - q[1]) + (p[2] - q[2]) * (p[2] - q[2]);
      if (l2 > e2max) e2max = l2;
    }
  }
  // cells: the root's is its box; a child's is the octant of the parent's planes, and must be the child's own box
  for (int i = 0; i < d.n_nodes; i++) {
    const double *bx = d.node_aabb + (size_t)i * 6, *c = d.node_center + (size_t)i * 3;
    for (int a = 0; a < 3; a++) {
      if (!(bx[a] <= bx[3 + a])) return no("a node's box is inverted");
    }
    const int pb = d.node_prim_begin[i], pc = d.node_prim_count[i];
    for (int t = pb; t < pb + pc; t++) {
      const double *b = d.tri_aabb + (size_t)t * 6;
      for (int a = 0; a < 3; a++) {
        if (!(bx[a] <= b[a] && b[3 + a] <= bx[3 + a])) return no("a triangle's box pokes out of its node's cell");
      }
    }
    const int fc = d.node_first_child[i];
    if (fc == 0) continue;
    for (int a = 0; a < 3; a++) {
      if (!(bx[a] <= c[a] && c[a] <= bx[3 + a])) return no("a node's centre lies outside its box");
    }
    for (int k = 0; k < 8; k++) {
      double o[6];
      sb_octant(bx, c, bx + 3, k, o);
      if (memcmp(o, d.node_aabb + (size_t)(fc + k) * 6, sizeof o) != 0) return no("a child's box is not its octant");
    }
  }
  const ShadowSlop s = shadow_slop(std::sqrt(e2max) * (1.0 + 0x1p-30), d.node_aabb);
  if (!(s.a <= 1.0 / 64.0)) return no("the longest edge makes the arithmetic's slop too large");
  const double rho = 6.0 * s.a / (1.0 - 6.0 * s.a);
  const double m32 = 1.0 + 0x1p-18;
  const double mu = (3.0 * s.a * s.dt * (1.0 + rho) + 2e-5 * (1.0 + rho)) * m32;
  const double kappa = 3.0 * s.r * (1.0 + rho) * m32;
  if (!std::isfinite(mu) || !std::isfinite(kappa) || !(mu <= s.diag)) return no("mu exceeds the scene's diagonal");
  ShadowBound b;
  b.rho1 = sb_f32_not_below((1.0 + rho) * m32);
  b.mu = sb_f32_not_below(mu);
  b.kappa = sb_f32_not_below(kappa);
  b.on = 1;
  return b;
}

}  // namespace mt
