// mt_raytree.h — the ray-tree buffer: the whole call tree of TraceRayWorker (mythtracer.cc:13-228) for every pixel of a
// chunk, traced once and stored layer by layer, so that the full-depth frame under edited light COLOURS is arithmetic
// over the stored tree (include/mythtracer_hip.h, mt_raytree_create ff.).  Nothing in the shape of the recursion depends
// on a light's colour: :181-184 and :192 read level, the material's reflectance and transparency, the reflection
// coefficient and in_object; the rays, their hits and the shadow loops read geometry, materials and light POSITIONS.
//
// Layer 0 holds one ray per chunk pixel (Sensor::GetRay), layer k + 1 the child rays of layer k in parent order, a
// parent's reflected ray before its refracted one.  Per ray: origin and direction as handed to IntersectRay, in_object,
// coef, the G-buffer planes point / normal (unflipped) / albedo / material, per light power and in_shadow
// (mt_lightbuffer.h's meaning, planes [n_lights][n_rays]), the two child indices into the next layer (-1 = none), and
// in layer 0 the chunk-local pixel index.  A tree made while mt_scene_set_raytree_uvw is on also keeps the G-buffer
// plane uvw: the one thing a texture edit needs to restate the albedo without tracing a ray.  A tree made while
// mt_scene_set_raytree_tri is on keeps tri, the stream index of the triangle each ray hit: the one thing a REASSIGNMENT
// (mt_scene_set_triangle_materials) needs to restate the ray's material, raytree_effective_material below.
//
//   raytree_primary_kernel  layer 0's ray list from the sensor, in raytree_layer0_index's order (8x8 blocks of the
//                           chunk, row-major; a block clipped by the chunk's edge holds only its pixels, row-major:
//                           the list has no holes).  mythtracer_amd/tiling.py restates it (raytree_layer0_order).
//   raytree_trace_kernel    lightbuffer_kernel's execution model over a ray LIST: a work item is 64 consecutive rays.
//                           Each lane loads its ray, traces it, writes the planes (write_gbuffer_planes), runs the
//                           lights' shadow loops -- lightbuffer_kernel's loop body restated, that kernel is as it was --
//                           and leaves the two child conditions in a byte per ray.
//   raytree_compact_kernel  one workgroup, refine_compact_kernel's scan: the child conditions become indices into the
//                           next layer, in order; the count goes to the host, which sizes the next layer by it.
//   raytree_spawn_kernel    one thread per parent: the child rays of :68-74 and :208-218 with the in_object and coef the
//                           recursive call receives (:186-187, :222-223), in the frame kernels' arithmetic.
//   raytree_shade_kernel    one thread per ray, one launch per layer, bottom-up: the direct term as shade_direct_kernel
//                           states it (from the stored direction instead of the sensor), + colour[child_refl] *
//                           reflectance (:185-188), + colour[child_refr] * transmission_filter * transparency
//                           (:220-224); layer 0 ends in V3DtoRGB at the ray's pixel.
//   raytree_update_kernel   a moved light: the listed lights' planes of ALL layers again from the stored point and
//                           material planes, one launch (a work item is 64 rays of one layer x one listed light).
// fp64 in the reference's order of operations (-ffp-contract=off), so a shaded tree is mt_render_chunk's frame byte for
// byte.
#pragma once
#include "mt_lightbuffer.h"

namespace mt {

// One layer's planes on the device (n rays).  `color` and `spawn` are the tree's own scratch.
struct RayTreeLayer {
  double *ray;         // [n][6] origin, direction
  double *coef;        // [n]
  double *point, *normal, *albedo;  // [n][3]
  double *power;       // [n_lights][n][3]
  double *color;       // [n][3] the shade's per-ray colour
  int32_t *material;   // [n]
  int32_t *child_refl, *child_refr;  // [n]
  int32_t *pixel;      // [n], layer 0 only
  uint8_t *in_object;  // [n]
  uint8_t *in_shadow;  // [n_lights][n]
  uint8_t *spawn;      // [n] bit 0: a reflected child, bit 1: a refracted child
  double *uvw;         // [n][3] Triangle::GetUVW(point), NaN on a miss; nullptr: the tree keeps none (mt_scene_set_raytree_uvw)
  int32_t *tri;        // [n] the stream index of the triangle hit, -1 on a miss; nullptr: the tree keeps none (mt_scene_set_raytree_tri)
};

// The material of stored ray i while a reassignment is pending (tri_mtl = the scene's CURRENT assignment, read through
// the layer's tri plane), else -- tri_mtl == nullptr -- what the material plane holds.
__device__ __forceinline__ int raytree_effective_material(const RayTreeLayer &L, const int32_t *tri_mtl, size_t i) {
  if (tri_mtl == nullptr) return L.material[i];
  const int tri = L.tri[i];
  return tri < 0 ? -1 : tri_mtl[tri];
}

// ---- edited vertex attributes (include/mythtracer_hip.h, mt_scene_set_triangle_normals / _uvw) ----
// tri_attr_stamp_kernel  one thread per triangle: the staged array's 9 doubles against the live array's BY THEIR BITS;
//                        a triangle that differs is copied into the live array and gets `generation` in its stamp.
//                        found[0] += the changed triangles, found[1] = min(the lowest changed index): one atomic pair per
//                        wave that has any.  At launch found = {0, 0xffffffff}.
struct TriAttrStampArgs {
  const double *staged;  // [n_tris][9]
  double *live;          // [n_tris][9]
  uint32_t *stamp;       // [n_tris]
  uint32_t n_tris;
  uint32_t generation;
  unsigned int *found;   // [2]
};

__global__ __launch_bounds__(256) void tri_attr_stamp_kernel(TriAttrStampArgs A) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)A.n_tris) return;
  const unsigned long long *a = (const unsigned long long *)(A.staged + i * 9);
  unsigned long long *b = (unsigned long long *)(A.live + i * 9);
  unsigned long long v[9];
  bool differ = false;
  for (int k = 0; k < 9; k++) {
    v[k] = a[k];
    differ = differ || v[k] != b[k];
  }
  if (differ) {
    for (int k = 0; k < 9; k++) b[k] = v[k];
    A.stamp[i] = A.generation;
  }
  const unsigned long long changed = __ballot(differ);
  if (differ && (int)__lane_id() == __ffsll((long long)changed) - 1) {  // (the wave's lowest changed triangle)
    atomicAdd(A.found, (unsigned)__popcll(changed));
    atomicMin(A.found + 1, (unsigned)i);
  }
}

// What a stored tree needs to follow an attribute edit: the scene's stamp planes and live arrays, and the generations of
// the tree's snapshot.  A stamp pointer is nullptr while no triangle carries a stamp newer than the snapshot: nothing of
// that attribute is dirty.  Only trees that keep tri get a non-null one.
struct RayTreeAttr {
  const uint32_t *normal_stamp, *uvw_stamp;  // [n_tris]
  uint32_t normal_gen, uvw_gen;              // the snapshot's
  const double *tri_vertex, *tri_normal, *tri_uvw;
  unsigned long long *count;                 // kRayTreeAttr* words (below); nullptr where a kernel counts nothing
};
enum { kRayTreeAttrBlocked = 0, kRayTreeAttrFirst = 1, kRayTreeAttrNormal = 2, kRayTreeAttrUVW = 3,
       kRayTreeAttrRespawned = 4, kRayTreeAttrWords = 5 };

__device__ __forceinline__ bool raytree_normal_dirty(const RayTreeAttr &T, const RayTreeLayer &L, size_t i) {
  if (T.normal_stamp == nullptr) return false;
  const int tri = L.tri[i];
  return tri >= 0 && T.normal_stamp[tri] > T.normal_gen;
}
__device__ __forceinline__ bool raytree_uvw_dirty(const RayTreeAttr &T, const RayTreeLayer &L, size_t i) {
  if (T.uvw_stamp == nullptr) return false;
  const int tri = L.tri[i];
  return tri >= 0 && T.uvw_stamp[tri] > T.uvw_gen;
}
// Triangle::GetNormal / GetUVW at the stored point of ray i of L, write_gbuffer_planes's expressions in its order
__device__ __forceinline__ V3 raytree_attr_at(const RayTreeAttr &T, const double *attr, const RayTreeLayer &L, size_t i) {
  const size_t tri = (size_t)L.tri[i];
  const Bary w = barycentric(T.tri_vertex + tri * 9, v3_load(L.point + i * 3));
  return interpolate(attr + tri * 9, w);
}
// one atomic per wave: *at += the lanes of the wave that are here with `flag` set
__device__ __forceinline__ void raytree_wave_count(unsigned long long *at, bool flag) {
  const unsigned long long b = __ballot(flag);
  if (flag && (int)__lane_id() == __ffsll((long long)b) - 1) atomicAdd(at, (unsigned long long)__popcll(b));
}

// index of chunk pixel (x, y) in layer 0's list
__host__ __device__ inline size_t raytree_layer0_index(int x, int y, int chunk_w, int chunk_h) {
  const int bx = x >> 3, by = y >> 3;
  const int bh = chunk_h - by * 8 < 8 ? chunk_h - by * 8 : 8;
  const int bw = chunk_w - bx * 8 < 8 ? chunk_w - bx * 8 : 8;
  return (size_t)by * 8 * (size_t)chunk_w + (size_t)bx * 8 * (size_t)bh + (size_t)((y & 7) * bw + (x & 7));
}

struct RayTreePrimaryArgs {
  mt_sensor sensor;
  int32_t chunk_x, chunk_y, chunk_w, chunk_h;
  RayTreeLayer L;
};

__global__ __launch_bounds__(256) void raytree_primary_kernel(RayTreePrimaryArgs A) {
  const size_t npx = (size_t)A.chunk_w * (size_t)A.chunk_h;
  const size_t px = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (px >= npx) return;
  const int lx = (int)(px % (size_t)A.chunk_w), ly = (int)(px / (size_t)A.chunk_w);
  const size_t i = raytree_layer0_index(lx, ly, A.chunk_w, A.chunk_h);
  // Sensor::GetRay, camera.cc:65-69
  const V3 d = v3_load(A.sensor.start_point) + (v3_load(A.sensor.delta_scanline) * (double)(A.chunk_y + ly)) +
               (v3_load(A.sensor.delta_pixel) * (double)(A.chunk_x + lx));
  const V3 rd = normalized(d);
  double *r = A.L.ray + i * 6;
  r[0] = A.sensor.origin[0]; r[1] = A.sensor.origin[1]; r[2] = A.sensor.origin[2];
  r[3] = rd.x; r[4] = rd.y; r[5] = rd.z;
  A.L.coef[i] = 1.0;
  A.L.in_object[i] = 0;
  A.L.pixel[i] = (int32_t)px;
}

struct RayTreeTraceArgs {
  RayTreeLayer L;
  uint32_t n_rays;
  uint32_t n_items;              // ceil(n_rays / 64)
  int32_t secondary;             // layer >= 1: the rays count as secondary
  int32_t may_spawn;             // layer < max_depth
  unsigned long long *counters;  // ST_COUNT
  unsigned int *work_counter;    // zero at launch
};

template <bool STATS, int DEEP>
__global__ __launch_bounds__(256, MT_WAVES_PER_SIMD) void raytree_trace_kernel(DevScene S, RayTreeTraceArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave_in_block = threadIdx.x >> 6;
  WaveStack stk;
  stk.bind(smem, wave_in_block, S.tree_depth, S.pack_shift, DEEP != 0);
  const MT_CONST mt_material *mtls = as_const(S.mtls);
  const MT_CONST mt_light *lights = as_const(S.lights);
  LaneStats st;
  st.clear();
  GBufferPlanes planes{};
  planes.point = A.L.point; planes.normal = A.L.normal; planes.albedo = A.L.albedo; planes.material = A.L.material;
  planes.uvw = A.L.uvw;  // (nullable, wave-uniform: write_gbuffer_planes computes it exactly as for the textured albedo)
  const size_t n = (size_t)A.n_rays;
  // every iteration of a shadow loop crosses another surface
  const int iteration_bound = S.n_tris + 2;
  bool failed = false;
  while (!failed) {
    const unsigned item = fetch_work(A.work_counter, lane);
    if (item >= A.n_items) break;
    const size_t i = (size_t)item * 64 + (size_t)lane;
    const bool want = i < n;
    V3 org = v3(0, 0, 0), rd = v3(0, 0, 1);
    if (want) {
      org = v3_load(A.L.ray + i * 6);
      rd = v3_load(A.L.ray + i * 6 + 3);
      if (STATS) st.v[ST_BYTES_VECTOR] += 48u;
    }
    const TraceOut to = trace_wave<STATS, DEEP>(S.self, stk.base, lane, want, org.x, org.y, org.z, rd.x, rd.y, rd.z);
    add_trace_stats<STATS>(st, to);
    if (to.status != DEV_OK) {
      if (lane == 0) atomicMax(A.counters + ST_STATUS, (unsigned long long)to.status);
      break;
    }
    V3 Pt = v3(0, 0, 0);
    bool lit = false;  // does the reference enter the light loop for this ray?
    if (want) {
      const PrimaryHit h = write_gbuffer_planes<STATS>(S, planes, i, org, rd, to, st, true);
      if (STATS && A.secondary) {  // (write_gbuffer_planes counted a primary ray)
        st.v[ST_RAYS_PRIMARY]--;
        st.v[ST_RAYS_SECONDARY]++;
      }
      lit = to.prim >= 0 && h.mtl >= 0;
      if (lit) Pt = h.point;
      if (A.L.tri != nullptr) A.L.tri[i] = to.prim >= 0 ? to.prim : -1;  // (nullable, wave-uniform)
      // the child conditions, :181-184 and :192 (level < max_depth is the layer's: wave-uniform)
      unsigned spawn = 0;
      if (lit && A.may_spawn) {
        const MT_CONST mt_material *m = mtls + h.mtl;
        const bool in_object = A.L.in_object[i] != 0;
        if (m->reflectance > 0.0 && A.L.coef[i] > 0.01 && !in_object) spawn |= 1u;
        if (m->transparency > 0.0) spawn |= 2u;
      }
      A.L.spawn[i] = (uint8_t)spawn;
    }
    for (int li = 0; li < S.n_lights && !failed; li++) {
      const MT_CONST mt_light *lt = lights + li;
      const V3 lpos = v3(lt->position[0], lt->position[1], lt->position[2]);
      // from here to the stores: lightbuffer_kernel's light loop body, the same operations in the same order
      V3 start = Pt, lp = v3(1.0, 1.0, 1.0);  // :90, :94
      bool in_shadow = false, traversing = false, running = lit;
      V3 ro = Pt, ld = v3(0, 0, 1);
      if (lit) {
        ld = normalized(lpos - Pt);  // light_direction, :79-80
        ro = Pt + (ld * 0.00001);    // :95-99
      }
      int iterations = 0;
      while (__ballot(running) != 0ull) {
        const TraceOut so = trace_wave<STATS, DEEP>(S.self, stk.base, lane, running, ro.x, ro.y, ro.z, ld.x, ld.y, ld.z);
        add_trace_stats<STATS>(st, so);
        if (so.status != DEV_OK || ++iterations > iteration_bound) {
          if (lane == 0) {
            atomicMax(A.counters + ST_STATUS, (unsigned long long)(so.status != DEV_OK ? so.status : DEV_ERR_PIXEL_BOUND));
          }
          failed = true;
          break;
        }
        if (running) {  // one iteration of the shadow loop, mythtracer.cc:94-156 (as mt_render.hip states it)
          if (STATS) {
            st.v[ST_RAYS_SHADOW]++;
            st.v[ST_BYTES_VECTOR] += 96u + 4u + 32u;  // light, occluder's material index and transparency
          }
          const int prim = so.prim;
          const double t = so.t;
          if (prim < 0) {
            running = false;  // :109-112
          } else {
            const double light_distance = distance(start, lpos);  // :101-102
            if (t > light_distance) {
              running = false;  // :115-118
            } else {
              // :121 dereferences shadow_primitive->mtl unconditionally; defined as opaque (mt_render.hip)
              const int sm = S.tri_mtl[prim];
              const double s_tr = sm >= 0 ? mtls[sm].transparency : 0.0;
              if (s_tr == 0.0) {
                lp = v3(0, 0, 0);
                in_shadow = true;
                running = false;
              } else {
                if (!traversing) {  // :129-132
                  const MT_CONST mt_material *smm = mtls + sm;
                  const V3 tf = v3(smm->transmission_filter[0], smm->transmission_filter[1],
                                   smm->transmission_filter[2]);
                  lp = lp * (tf * s_tr);
                }
                traversing = !traversing;
                const V3 sp = ro + ld * t;
                start = sp + (ld * 0.0000001);  // :137
                if (sqr_distance(Pt, start) > sqr_distance(Pt, lpos)) {
                  running = false;  // :141-145
                } else if (lp.x <= 0.001 && lp.y <= 0.001 && lp.z <= 0.001) {
                  lp = v3(0, 0, 0);  // :149-155
                  in_shadow = true;
                  running = false;
                } else {
                  ro = start + (ld * 0.00001);  // next iteration, :95-99
                }
              }
            }
          }
        }
      }
      if (want && !failed) {
        const size_t at = (size_t)li * n + i;
        const double nan = __builtin_nan("");
        store3(A.L.power, at, lit ? lp : v3(nan, nan, nan));
        A.L.in_shadow[at] = lit ? (in_shadow ? 1 : 0) : 255;
        if (STATS) st.v[ST_BYTES_VECTOR] += 24u + 1u;
      }
    }
    flush_item_stats<STATS>(st, A.counters, lane);
  }
}

constexpr int kRayTreeCompactThreads = 1024;

// One workgroup of kRayTreeCompactThreads: thread t owns the rays [t per, (t + 1) per); an exclusive scan of the threads'
// child counts gives each its place in the next layer (refine_compact_kernel's scan: the same layer gives the same
// order).  Writes both child indices of every ray and the next layer's ray count -- 64 bits: it is the host that
// refuses 2^31 or more.
__global__ void __launch_bounds__(kRayTreeCompactThreads) raytree_compact_kernel(RayTreeLayer L, uint32_t n,
                                                                                 unsigned long long *count_out) {
  __shared__ unsigned long long s_count[kRayTreeCompactThreads];
  const unsigned t = threadIdx.x;
  const unsigned per = (n + kRayTreeCompactThreads - 1) / kRayTreeCompactThreads;
  const unsigned i0 = min(t * per, n), i1 = min(i0 + per, n);
  unsigned long long mine = 0;
  for (unsigned i = i0; i < i1; i++) {
    const unsigned f = L.spawn[i];
    mine += (f & 1u) + (f >> 1);
  }
  s_count[t] = mine;
  __syncthreads();
  // inclusive scan (Hillis-Steele) over the threads' counts
  for (unsigned d = 1; d < kRayTreeCompactThreads; d <<= 1) {
    const unsigned long long add = t >= d ? s_count[t - d] : 0ull;
    __syncthreads();
    s_count[t] += add;
    __syncthreads();
  }
  const unsigned long long total = s_count[kRayTreeCompactThreads - 1];
  if (t == 0) *count_out = total;
  if (total >= 0x80000000ull) return;  // no index of such a layer fits: the host fails the call
  int32_t j = (int32_t)(s_count[t] - mine);
  for (unsigned i = i0; i < i1; i++) {
    const unsigned f = L.spawn[i];
    L.child_refl[i] = (f & 1u) ? j++ : -1;
    L.child_refr[i] = (f & 2u) ? j++ : -1;
  }
}

struct RayTreeSpawnArgs {
  RayTreeLayer parent, child;
  uint32_t n_parent;
  const mt_material *mtls;
};

__global__ __launch_bounds__(256) void raytree_spawn_kernel(RayTreeSpawnArgs A) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)A.n_parent) return;
  const int cr = A.parent.child_refl[i], ct = A.parent.child_refr[i];
  if (cr < 0 && ct < 0) return;
  const V3 dir = v3_load(A.parent.ray + i * 6 + 3);
  const V3 Pt = v3_load(A.parent.point + i * 3);
  const double coef = A.parent.coef[i];
  const bool in_object = A.parent.in_object[i] != 0;
  if (cr >= 0) {
    V3 Nn = v3_load(A.parent.normal + i * 3);  // as GetNormal returned it, :38
    if (dot(Nn, -dir) < 0.0) Nn = -Nn;         // :42-45
    const V3 Rd = dir - Nn * (2 * dot(dir, Nn));  // :68-69
    const V3 ro = Pt + (Rd * 0.0001);             // :70-74
    double *r = A.child.ray + (size_t)cr * 6;
    r[0] = ro.x; r[1] = ro.y; r[2] = ro.z; r[3] = Rd.x; r[4] = Rd.y; r[5] = Rd.z;
    A.child.coef[cr] = coef * A.mtls[A.parent.material[i]].reflectance;  // :187
    A.child.in_object[cr] = in_object ? 1 : 0;
  }
  if (ct >= 0) {
    const V3 rdir = normalized(dir);  // :208-212 (direction unchanged, re-normalised)
    const V3 ro = Pt + rdir * 0.00001;
    double *r = A.child.ray + (size_t)ct * 6;
    r[0] = ro.x; r[1] = ro.y; r[2] = ro.z; r[3] = rdir.x; r[4] = rdir.y; r[5] = rdir.z;
    A.child.coef[ct] = coef;                    // :223
    A.child.in_object[ct] = in_object ? 0 : 1;  // :222
  }
}

struct RayTreeShadeArgs {
  RayTreeLayer L;
  const double *child_color;  // the next layer's colours; nullptr: this is the deepest layer
  uint32_t n_rays;
  int32_t n_lights;
  const mt_material *mtls;
  const mt_light *d_lights;   // ARG_LIGHTS = false
  uint8_t *out_rgb;           // layer 0: chunk-local row-major RGB8; else nullptr
  mt_light lights[kShadeArgLights];  // ARG_LIGHTS = true
};

template <bool ARG_LIGHTS>
__global__ __launch_bounds__(256) void raytree_shade_kernel(RayTreeShadeArgs A) {
  const size_t n = (size_t)A.n_rays;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  V3 color = v3(0, 0, 0);
  const V3 Pt = v3_load(A.L.point + i * 3);
  if (Pt.x == Pt.x) {  // (a miss: background, mythtracer.cc:23-31)
    const V3 dir = v3_load(A.L.ray + i * 6 + 3);
    V3 Nn = v3_load(A.L.normal + i * 3);  // as GetNormal returned it, :38
    const V3 towards_camera = -dir;
    double normal_ray_dot = dot(Nn, towards_camera);
    if (normal_ray_dot < 0.0) {  // :42-45
      Nn = -Nn;
      normal_ray_dot = dot(Nn, towards_camera);
    }
    const int mtl = A.L.material[i];
    if (mtl < 0) {  // :49-52
      normal_ray_dot = (normal_ray_dot + 1.0) * 0.5;
      color = v3(normal_ray_dot, normal_ray_dot, normal_ray_dot);
    } else {
      const mt_material *m = A.mtls + mtl;
      const V3 surf = v3_load(A.L.albedo + i * 3);            // :58-64
      const V3 Rd = dir - Nn * (2 * dot(dir, Nn));            // :68-69
      const double refl_dot = dot(Rd, towards_camera);        // :170
      const V3 kd = v3(m->diffuse[0], m->diffuse[1], m->diffuse[2]);
      for (int li = 0; li < A.n_lights; li++) {
        const mt_light *lt = ARG_LIGHTS ? A.lights + li : A.d_lights + li;
        const V3 lpos = v3(lt->position[0], lt->position[1], lt->position[2]);
        const V3 amb = v3(lt->ambient[0], lt->ambient[1], lt->ambient[2]);
        const V3 ld = normalized(lpos - Pt);                  // :79-80
        color = color + amb * surf;                           // :83-84
        const size_t at = (size_t)li * n + i;
        V3 lp = v3_load(A.L.power + at * 3);
        lp.x = std_max(lp.x, amb.x);                          // :159-161
        lp.y = std_max(lp.y, amb.y);
        lp.z = std_max(lp.z, amb.z);
        const V3 ldiff = v3(lt->diffuse[0], lt->diffuse[1], lt->diffuse[2]);
        color = color + kd * surf * dot(ld, Nn) * ldiff * lp;  // :163-167
        if (A.L.in_shadow[at] == 0 && refl_dot > 0) {         // :169-177
          const V3 ks = v3(m->specular[0], m->specular[1], m->specular[2]);
          const V3 ls = v3(lt->specular[0], lt->specular[1], lt->specular[2]);
          color = color + ks * surf * ::pow(refl_dot, m->specular_exp) * ls;
        }
      }
      const int cr = A.L.child_refl[i], ct = A.L.child_refr[i];
      if (cr >= 0) color = color + v3_load(A.child_color + (size_t)cr * 3) * m->reflectance;  // :185-188
      if (ct >= 0) {                                                                          // :220-224
        const V3 tf = v3(m->transmission_filter[0], m->transmission_filter[1], m->transmission_filter[2]);
        color = color + v3_load(A.child_color + (size_t)ct * 3) * tf * m->transparency;
      }
    }
  }
  if (A.out_rgb != nullptr) {
    uint8_t *o = A.out_rgb + (size_t)A.L.pixel[i] * 3;
    o[0] = channel_to_u8(color.x);  // V3DtoRGB, :235-241
    o[1] = channel_to_u8(color.y);
    o[2] = channel_to_u8(color.z);
  } else {
    store3(A.L.color, i, color);
  }
}

// raytree_update_kernel: the planes of the LISTED lights again in EVERY layer, from the stored hits -- a layer's `point`
// and `material` planes hold, bit for bit, the two things a shadow loop takes from the ray's trace, and no ray, hit or
// child index of the tree depends on a light.  No sensor, no primary or secondary trace_wave; the planes of the other
// lights and everything else in the tree are not touched.  The listed lights' loops of all layers are independent, so
// they all go out in ONE launch: a work item is 64 consecutive rays of one layer x one listed light, so that the few
// items of the deep layers share the chip with layer 0's.  Within a light, place j belongs to layer l when it lies
// between l's first_item and the next layer's; the items are handed out light-major and within a light from the LAST
// place down (j = items_per_light - 1 - item % items_per_light): the deepest layers, whose waves mix rays of many
// blocks and whose loops are the long ones, start first and layer 0's many coherent items fill in behind them
// (measured against layer 0 first; the order changes no bit of the result).  A wave finds its layer
// from the wave-uniform j.  A ray's loop runs when point[0] is not NaN and 0 <= material < n_materials; every other
// ray of the layer gets NaN / 255.  raytree_trace_kernel's light loop body restated, that kernel is as it was.
struct RayTreeUpdateLayer {
  const double *point;      // [n][3]
  const int32_t *material;  // [n]
  double *power;            // [n_lights][n][3], plane l written for listed l only
  uint8_t *in_shadow;       // [n_lights][n]
  uint32_t n_rays;
  uint32_t first_item;      // of this layer within one light's items
};

struct RayTreeUpdateArgs {
  RayTreeUpdateLayer layer[MT_MAX_RECURSION + 1];
  int32_t n_layers;
  int32_t n_materials;
  uint32_t items_per_light;          // sum over the layers of ceil(n_rays / 64)
  uint32_t n_items;                  // items_per_light x listed lights
  const int32_t *d_idx;              // the list when it has more than kUpdateArgLights entries, else nullptr
  int32_t idx[kUpdateArgLights];
  unsigned long long *counters;      // ST_COUNT
  unsigned int *work_counter;        // zero at launch
};

template <bool STATS, int DEEP>
__global__ __launch_bounds__(256, MT_WAVES_PER_SIMD) void raytree_update_kernel(DevScene S, RayTreeUpdateArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave_in_block = threadIdx.x >> 6;
  WaveStack stk;
  stk.bind(smem, wave_in_block, S.tree_depth, S.pack_shift, DEEP != 0);
  const MT_CONST mt_material *mtls = as_const(S.mtls);
  const MT_CONST mt_light *lights = as_const(S.lights);
  LaneStats st;
  st.clear();
  // every iteration of a shadow loop crosses another surface
  const int iteration_bound = S.n_tris + 2;
  bool failed = false;
  while (!failed) {
    const unsigned item = fetch_work(A.work_counter, lane);
    if (item >= A.n_items) break;
    const unsigned k = item / A.items_per_light, j = A.items_per_light - 1u - item % A.items_per_light;  // (wave-uniform)
    const int li = A.d_idx != nullptr ? A.d_idx[k] : A.idx[k];
    int layer = 0;
    while (layer + 1 < A.n_layers && j >= A.layer[layer + 1].first_item) layer++;
    const RayTreeUpdateLayer L = A.layer[layer];
    const size_t n = (size_t)L.n_rays;
    const size_t i = (size_t)(j - L.first_item) * 64 + (size_t)lane;
    const bool want = i < n;
    V3 Pt = v3(0, 0, 0);
    bool lit = false;
    if (want) {
      const V3 p = v3_load(L.point + i * 3);
      const int mtl = L.material[i];
      lit = p.x == p.x && mtl >= 0 && mtl < A.n_materials;
      if (lit) Pt = p;
      if (STATS) st.v[ST_BYTES_VECTOR] += 24u + 4u;
    }
    const MT_CONST mt_light *lt = lights + li;
    const V3 lpos = v3(lt->position[0], lt->position[1], lt->position[2]);
    // from here to the stores: raytree_trace_kernel's light loop body, the same operations in the same order
    V3 start = Pt, lp = v3(1.0, 1.0, 1.0);  // :90, :94
    bool in_shadow = false, traversing = false, running = lit;
    V3 ro = Pt, ld = v3(0, 0, 1);
    if (lit) {
      ld = normalized(lpos - Pt);  // light_direction, :79-80
      ro = Pt + (ld * 0.00001);    // :95-99
    }
    int iterations = 0;
    while (__ballot(running) != 0ull) {
      const TraceOut so = trace_wave<STATS, DEEP>(S.self, stk.base, lane, running, ro.x, ro.y, ro.z, ld.x, ld.y, ld.z);
      add_trace_stats<STATS>(st, so);
      if (so.status != DEV_OK || ++iterations > iteration_bound) {
        if (lane == 0) {
          atomicMax(A.counters + ST_STATUS, (unsigned long long)(so.status != DEV_OK ? so.status : DEV_ERR_PIXEL_BOUND));
        }
        failed = true;
        break;
      }
      if (running) {  // one iteration of the shadow loop, mythtracer.cc:94-156 (as mt_render.hip states it)
        if (STATS) {
          st.v[ST_RAYS_SHADOW]++;
          st.v[ST_BYTES_VECTOR] += 96u + 4u + 32u;  // light, occluder's material index and transparency
        }
        const int prim = so.prim;
        const double t = so.t;
        if (prim < 0) {
          running = false;  // :109-112
        } else {
          const double light_distance = distance(start, lpos);  // :101-102
          if (t > light_distance) {
            running = false;  // :115-118
          } else {
            // :121 dereferences shadow_primitive->mtl unconditionally; defined as opaque (mt_render.hip)
            const int sm = S.tri_mtl[prim];
            const double s_tr = sm >= 0 ? mtls[sm].transparency : 0.0;
            if (s_tr == 0.0) {
              lp = v3(0, 0, 0);
              in_shadow = true;
              running = false;
            } else {
              if (!traversing) {  // :129-132
                const MT_CONST mt_material *smm = mtls + sm;
                const V3 tf = v3(smm->transmission_filter[0], smm->transmission_filter[1],
                                 smm->transmission_filter[2]);
                lp = lp * (tf * s_tr);
              }
              traversing = !traversing;
              const V3 sp = ro + ld * t;
              start = sp + (ld * 0.0000001);  // :137
              if (sqr_distance(Pt, start) > sqr_distance(Pt, lpos)) {
                running = false;  // :141-145
              } else if (lp.x <= 0.001 && lp.y <= 0.001 && lp.z <= 0.001) {
                lp = v3(0, 0, 0);  // :149-155
                in_shadow = true;
                running = false;
              } else {
                ro = start + (ld * 0.00001);  // next iteration, :95-99
              }
            }
          }
        }
      }
    }
    if (want && !failed) {
      const size_t at = (size_t)li * n + i;
      const double nan = __builtin_nan("");
      store3(L.power, at, lit ? lp : v3(nan, nan, nan));
      L.in_shadow[at] = lit ? (in_shadow ? 1 : 0) : 255;
      if (STATS) st.v[ST_BYTES_VECTOR] += 24u + 1u;
    }
    flush_item_stats<STATS>(st, A.counters, lane);
  }
}

#define MT_INSTANTIATE_RT_UPDATE(DEEP_)                                                      \
  template __global__ void raytree_update_kernel<true, DEEP_>(DevScene, RayTreeUpdateArgs);  \
  template __global__ void raytree_update_kernel<false, DEEP_>(DevScene, RayTreeUpdateArgs);
MT_INSTANTIATE_RT_UPDATE(0)
MT_INSTANTIATE_RT_UPDATE(1)
MT_INSTANTIATE_RT_UPDATE(2)
#undef MT_INSTANTIATE_RT_UPDATE

#define MT_INSTANTIATE_RT(DEEP_)                                                          \
  template __global__ void raytree_trace_kernel<true, DEEP_>(DevScene, RayTreeTraceArgs);  \
  template __global__ void raytree_trace_kernel<false, DEEP_>(DevScene, RayTreeTraceArgs);
MT_INSTANTIATE_RT(0)
MT_INSTANTIATE_RT(1)
MT_INSTANTIATE_RT(2)
#undef MT_INSTANTIATE_RT
template __global__ void raytree_shade_kernel<true>(RayTreeShadeArgs);
template __global__ void raytree_shade_kernel<false>(RayTreeShadeArgs);

// ---- a tree over the CALLER's rays (include/mythtracer_hip.h, mt_raytree_create_rays ff.) ----
// raytree_rays_kernel  layer 0 from a ray list instead of the sensor: raytree_primary_kernel's shape with the rays read
//                      from memory.  The list counts as a list_w x list_h chunk: caller's ray p goes to place
//                      raytree_layer0_index(p % list_w, p / list_w, list_w, list_h) (p itself when list_h == 1) and
//                      pixel = p.  A ray the walk must never see -- a number that is not finite, the direction
//                      (0, 0, 0), an in_object byte above 1, a coef that is not finite -- is counted in bad[0] and
//                      its index kept in bad[1] when it is the lowest (atomicAdd / atomicMin); the host reads the two
//                      words before the first raytree_trace_kernel launch and launches none when bad[0] != 0.
// raytree_color_kernel the shade's layer-0 colours, as raytree_shade_kernel leaves them in L.color when out_rgb is
//                      nullptr, to the rays' places of the caller's [n][3] doubles: out[pixel[i]] = color[i].
struct RayTreeRaysArgs {
  const double *ray;         // [n][6], the caller's order
  const uint8_t *in_object;  // [n] or nullptr = all 0
  const double *coef;        // [n] or nullptr = all 1.0
  int32_t list_w, list_h;
  RayTreeLayer L;
  unsigned int *bad;         // [2] at launch: 0, 0xffffffff
};

// neither an infinity nor a NaN (by the exponent's bits: no compiler flag has a say)
__device__ inline bool raytree_finite(double v) {
  return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

__global__ __launch_bounds__(256) void raytree_rays_kernel(RayTreeRaysArgs A) {
  const size_t n = (size_t)A.list_w * (size_t)A.list_h;
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const double *src = A.ray + p * 6;
  const double r0 = src[0], r1 = src[1], r2 = src[2], r3 = src[3], r4 = src[4], r5 = src[5];
  const unsigned in_object = A.in_object != nullptr ? A.in_object[p] : 0u;
  const double coef = A.coef != nullptr ? A.coef[p] : 1.0;
  const bool finite = raytree_finite(r0) && raytree_finite(r1) && raytree_finite(r2) && raytree_finite(r3) &&
                      raytree_finite(r4) && raytree_finite(r5);
  const bool zero = r3 == 0.0 && r4 == 0.0 && r5 == 0.0;
  if (!finite || zero || in_object > 1u || !raytree_finite(coef)) {
    atomicAdd(A.bad, 1u);
    atomicMin(A.bad + 1, (unsigned)p);  // (n < 2^31)
    return;
  }
  const size_t i = raytree_layer0_index((int)(p % (size_t)A.list_w), (int)(p / (size_t)A.list_w), A.list_w, A.list_h);
  double *r = A.L.ray + i * 6;
  r[0] = r0; r[1] = r1; r[2] = r2; r[3] = r3; r[4] = r4; r[5] = r5;
  A.L.coef[i] = coef;
  A.L.in_object[i] = (uint8_t)in_object;
  A.L.pixel[i] = (int32_t)p;
}

__global__ __launch_bounds__(256) void raytree_color_kernel(const double *color, const int32_t *pixel, uint32_t n_rays,
                                                            double *out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n_rays) return;
  store3(out, (size_t)pixel[i], v3_load(color + i * 3));
}

// ---- edited materials (include/mythtracer_hip.h, mt_raytree_update_materials) ----
// What a stored tree holds that depends on a material: albedo (the material's ambient), coef (products of reflectance
// along the path), the child conditions (reflectance, transparency, coef) and the light planes.  The last are
// raytree_update_kernel's, unchanged; the first three are these two kernels', plain grids, one thread per ray.
// raytree_recoef_kernel    the CHECK pass, one launch per layer, top-down.  The ray's coefficient c under the new
//                          materials is coef[i] in layer 0 (nothing above it) and, deeper, what its parent's thread
//                          left in color[i][0] -- the shade's scratch plane: one shade OR one update in flight per
//                          tree.  The two child conditions exactly as raytree_trace_kernel evaluates them, from the NEW
//                          materials, c, in_object[i], may_spawn and lit (point[i][0] not NaN, 0 <= material[i] <
//                          n_materials), are compared with child_refl[i] >= 0 and child_refr[i] >= 0: a mismatch in
//                          either direction adds one to mismatch[0] and offers (layer << 32 | i) to mismatch[1]
//                          (atomicMin).  Where the TREE has a child, its new coefficient goes to the child's scratch
//                          with raytree_spawn_kernel's expressions.  Writes nothing but scratch and the two words.
// raytree_recommit_kernel  the COMMIT, one launch per layer that has something to take: coef[i] = the scratch's
//                          coefficient (copy_coef: layers >= 1 after a clean check), and albedo[i] = the new ambient for
//                          the rays whose material's byte in `albedo_changed` is set -- what write_gbuffer_planes
//                          stores for an untextured material, no arithmetic; times the texel at the ray's stored uvw
//                          where the material has a texture (retextured_albedo, mt_gbuffer.h: a tree that keeps uvw;
//                          the host lets no textured material's byte through for a tree that does not).
// A pending REASSIGNMENT (tri_mtl != nullptr, a tree that keeps tri): both kernels read raytree_effective_material in the
// material plane's place; the commit also writes it into the material plane, and restates the albedo of every ray whose
// material moved as well -- NaN for "no material", what write_gbuffer_planes stores.
struct RayTreeRecoefArgs {
  RayTreeLayer L;
  double *child_scratch;         // the next layer's color plane, nullptr: there is no next layer
  const mt_material *mtls;       // the scene's CURRENT materials
  const int32_t *tri_mtl;        // the scene's CURRENT assignment while a reassignment is pending, else nullptr
  uint32_t n_rays;
  int32_t n_materials;
  int32_t layer;
  int32_t may_spawn;             // layer < max_depth
  unsigned long long *mismatch;  // [2] at the first layer's launch: 0, ~0
};

__global__ __launch_bounds__(256) void raytree_recoef_kernel(RayTreeRecoefArgs A) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)A.n_rays) return;
  const double c = A.layer == 0 ? A.L.coef[i] : A.L.color[i * 3];
  const double p0 = A.L.point[i * 3];
  const int mtl = raytree_effective_material(A.L, A.tri_mtl, i);
  const bool lit = p0 == p0 && mtl >= 0 && mtl < A.n_materials;
  const int cr = A.L.child_refl[i], ct = A.L.child_refr[i];
  // the child conditions, :181-184 and :192, as raytree_trace_kernel states them
  unsigned spawn = 0;
  double reflectance = 0.0;
  if (lit && A.may_spawn) {
    const mt_material *m = A.mtls + mtl;
    const bool in_object = A.L.in_object[i] != 0;
    reflectance = m->reflectance;
    if (m->reflectance > 0.0 && c > 0.01 && !in_object) spawn |= 1u;
    if (m->transparency > 0.0) spawn |= 2u;
  }
  const unsigned has = (cr >= 0 ? 1u : 0u) | (ct >= 0 ? 2u : 0u);
  if (spawn != has) {
    atomicAdd(A.mismatch, 1ull);
    atomicMin(A.mismatch + 1, ((unsigned long long)(unsigned)A.layer << 32) | (unsigned long long)i);
  }
  if (A.child_scratch != nullptr) {
    // (a child of a ray that is not lit cannot exist; `reflectance` is then 0 and nothing is stored)
    if (cr >= 0) A.child_scratch[(size_t)cr * 3] = c * reflectance;  // :187
    if (ct >= 0) A.child_scratch[(size_t)ct * 3] = c;                // :223
  }
}

struct RayTreeRecommitArgs {
  RayTreeLayer L;
  const mt_material *mtls;        // the scene's CURRENT materials
  const DevTexture *texs;         // and its CURRENT textures
  const uint8_t *albedo_changed;  // [n_materials], nullptr: no albedo to rewrite for a material's own sake
  const int32_t *tri_mtl;         // the scene's CURRENT assignment while a reassignment is pending, else nullptr
  uint32_t n_rays;
  int32_t n_materials;
  int32_t copy_coef;
};

// the albedo of a stored ray whose material is now `mtl`: retextured_albedo, NaN for "no material"
__device__ __forceinline__ V3 raytree_restated_albedo(const mt_material *mtls, const DevTexture *texs, int mtl,
                                                      const double *uvw, size_t i) {
  const double nan = __builtin_nan("");
  return mtl >= 0 ? retextured_albedo(mtls + mtl, texs, uvw, i) : v3(nan, nan, nan);
}

__global__ __launch_bounds__(256) void raytree_recommit_kernel(RayTreeRecommitArgs A) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)A.n_rays) return;
  if (A.copy_coef) A.L.coef[i] = A.L.color[i * 3];
  const int was = A.L.material[i];
  const int mtl = raytree_effective_material(A.L, A.tri_mtl, i);
  if (mtl != was) {
    A.L.material[i] = mtl;
    store3(A.L.albedo, i, raytree_restated_albedo(A.mtls, A.texs, mtl, A.L.uvw, i));
  } else if (A.albedo_changed != nullptr && mtl >= 0 && mtl < A.n_materials && A.albedo_changed[mtl] != 0) {
    store3(A.L.albedo, i, retextured_albedo(A.mtls + mtl, A.texs, A.L.uvw, i));
  }
}

// ---- edited vertex attributes in a stored tree (include/mythtracer_hip.h, mt_raytree_attr_info_last ff.) ----
// raytree_attr_check_kernel  part of the CHECK pass, one launch per layer while normal stamps are pending: counts the
//                            normal-dirty rays that have a reflected child (count[Blocked]) and offers
//                            (layer << 32 | i) to count[First].  Such a child's ray depends on the edited normal: an
//                            update refuses, a regrow traces it.  Writes nothing but the two words.
// raytree_reattr_kernel      part of the COMMIT, one launch per layer, behind raytree_recommit_kernel (the material plane
//                            holds the effective material by then): normal' to the normal plane of a normal-dirty ray;
//                            uvw' to the uvw plane (where kept) and the albedo restated from uvw' for a uvw-dirty one.
//                            Counts both kinds.  Plain grids, one thread per ray.
struct RayTreeReattrArgs {
  RayTreeLayer L;
  RayTreeAttr attr;
  const mt_material *mtls;  // the scene's CURRENT materials
  const DevTexture *texs;   // and its CURRENT textures
  uint32_t n_rays;
  int32_t layer;
};

__global__ __launch_bounds__(256) void raytree_attr_check_kernel(RayTreeReattrArgs A) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)A.n_rays) return;
  const bool blocked = A.L.child_refl[i] >= 0 && raytree_normal_dirty(A.attr, A.L, i);
  raytree_wave_count(A.attr.count + kRayTreeAttrBlocked, blocked);
  if (blocked) atomicMin(A.attr.count + kRayTreeAttrFirst, ((unsigned long long)(unsigned)A.layer << 32) | (unsigned long long)i);
}

// the albedo of a stored ray with material `mtl` (-1: none) at texture coordinates `uvw`
__device__ __forceinline__ V3 raytree_albedo_at(const mt_material *mtls, const DevTexture *texs, int mtl, V3 uvw) {
  const double c[3] = {uvw.x, uvw.y, uvw.z};
  const double nan = __builtin_nan("");
  return mtl >= 0 ? retextured_albedo(mtls + mtl, texs, c, 0) : v3(nan, nan, nan);
}

__global__ __launch_bounds__(256) void raytree_reattr_kernel(RayTreeReattrArgs A) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)A.n_rays) return;
  const bool nd = raytree_normal_dirty(A.attr, A.L, i), ud = raytree_uvw_dirty(A.attr, A.L, i);
  if (nd) store3(A.L.normal, i, raytree_attr_at(A.attr, A.attr.tri_normal, A.L, i));
  if (ud) {
    const V3 uvw = raytree_attr_at(A.attr, A.attr.tri_uvw, A.L, i);
    if (A.L.uvw != nullptr) store3(A.L.uvw, i, uvw);
    store3(A.L.albedo, i, raytree_albedo_at(A.mtls, A.texs, A.L.material[i], uvw));
  }
  raytree_wave_count(A.attr.count + kRayTreeAttrNormal, nd);
  raytree_wave_count(A.attr.count + kRayTreeAttrUVW, ud);
}

// ---- edited materials that change the tree's shape (include/mythtracer_hip.h, mt_raytree_regrow_materials) ----
// The NEW tree is built layer by layer, top-down, next to the old one.  A ray of the new tree is KEPT when its path from
// the pixel exists in the old tree -- every ray of layer 0; a child whose parent is kept and had a child in the same
// slot -- and TRACED otherwise.  Every new layer k carries src[i]: the ray's index in the OLD layer k, -1 for a traced
// ray (layer 0: src = nullptr, meaning src[i] = i).  A kept ray takes everything that depends on no material from the
// old tree; a traced ray goes through the unchanged raytree_trace_kernel in a dense temporary layer.  Per layer k, over
// plain 256-thread grids (the scans are raytree_compact_kernel's, unchanged):
//   raytree_regrow_flags_kernel    one thread per ray: the spawn byte of a KEPT ray from the NEW materials, the ray's new
//                                  coef, in_object, may_spawn and lit-ness -- raytree_trace_kernel's expressions, with
//                                  lit as raytree_recoef_kernel states it.  A traced ray has its byte from its trace.
//   (raytree_compact_kernel)       the spawn bytes become layer k's child indices and layer k + 1's ray count.
//   raytree_regrow_link_kernel     one thread per parent, per child slot: the old child index -- the old parent's, where
//                                  the parent is kept and had that child -- goes to src of layer k + 1; the child's coef
//                                  with raytree_spawn_kernel's expressions under the new materials; a child WITHOUT an
//                                  old index also gets its ray and in_object, raytree_spawn_kernel's expressions again.
//                                  The child's spawn byte becomes 1 for "to be traced", 0 for kept:
//   (raytree_compact_kernel)       run over layer k + 1 itself, it leaves every traced ray's place in the dense list in
//                                  child_refl (-1 for a kept ray; child_refr is all -1) and the list's length in the
//                                  count.  The order is the layer's, so a work item is 64 consecutive traced rays.  The
//                                  places live in child_refl until layer k + 1's own compaction overwrites them.
//   raytree_regrow_copy_kernel     one thread per kept ray of layer k + 1, by the destination index: ray, in_object,
//                                  point, normal, material, every light's power and in_shadow from the old layer at
//                                  src; uvw and tri too where the tree keeps them; albedo too, or the new ambient (times
//                                  the texel at the OLD layer's uvw at src) where the material's byte in albedo_changed
//                                  is set or a pending reassignment moved the ray's material (raytree_recommit_kernel's
//                                  rule).
//   raytree_regrow_gather_kernel   ray, coef and in_object of the traced rays to their places in the temporary layer;
//   (raytree_trace_kernel)         over the temporary layer, secondary = 1, may_spawn = (k + 1 < max_depth);
//   raytree_regrow_scatter_kernel  point, normal, albedo, material, power, in_shadow, spawn and (where kept) uvw and tri
//                                  back to the new layer.
// A pending NORMAL edit (RayTreeAttr, a tree that keeps tri) adds one reason for a child to be traced rather than kept: the
// link kernel gives the reflected child of a KEPT normal-dirty parent no old index and spawns it from the parent's
// effective normal (layer 0's normal plane waits for the commit); the refracted child keeps its index.  The copy kernel
// restates normal, uvw and albedo of kept dirty rays by raytree_reattr_kernel's rule.
// That regrouping the traced rays changes no bit is the ray-list contract: layer k handed in as an n x 1 list gives the
// tree's layers k onwards.  None of these kernels writes a plane of the OLD tree.
struct RayTreeRegrowFlagsArgs {
  RayTreeLayer L;
  const int32_t *src;       // nullptr: layer 0, every ray is kept
  const mt_material *mtls;  // the scene's CURRENT materials
  const int32_t *tri_mtl;   // layer 0 while a reassignment is pending (its material plane waits for the commit), else nullptr
  uint32_t n_rays;
  int32_t n_materials;
  int32_t may_spawn;        // layer < max_depth
};

__global__ __launch_bounds__(256) void raytree_regrow_flags_kernel(RayTreeRegrowFlagsArgs A) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)A.n_rays) return;
  if (A.src != nullptr && A.src[i] < 0) return;  // (traced: raytree_trace_kernel left its byte)
  const double p0 = A.L.point[i * 3];
  const int mtl = raytree_effective_material(A.L, A.tri_mtl, i);
  const bool lit = p0 == p0 && mtl >= 0 && mtl < A.n_materials;
  // the child conditions, :181-184 and :192, as raytree_trace_kernel states them
  unsigned spawn = 0;
  if (lit && A.may_spawn) {
    const mt_material *m = A.mtls + mtl;
    const bool in_object = A.L.in_object[i] != 0;
    if (m->reflectance > 0.0 && A.L.coef[i] > 0.01 && !in_object) spawn |= 1u;
    if (m->transparency > 0.0) spawn |= 2u;
  }
  A.L.spawn[i] = (uint8_t)spawn;
}

struct RayTreeRegrowLinkArgs {
  RayTreeLayer parent, child;                      // layers k and k + 1 of the NEW tree
  const int32_t *parent_src;                       // nullptr: layer 0
  const int32_t *old_child_refl, *old_child_refr;  // of the OLD layer k
  int32_t *child_src;                              // [the child layer's rays]
  const mt_material *mtls;                         // the scene's CURRENT materials
  const int32_t *tri_mtl;                          // as RayTreeRegrowFlagsArgs has it: the parent is layer 0, else nullptr
  uint32_t n_parent;
  // a pending normal edit: the reflected child of a KEPT normal-dirty parent is not kept -- it is spawned from the
  // parent's effective normal and traced (counted in count[Respawned])
  RayTreeAttr attr;
};

__global__ __launch_bounds__(256) void raytree_regrow_link_kernel(RayTreeRegrowLinkArgs A) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)A.n_parent) return;
  const int cr = A.parent.child_refl[i], ct = A.parent.child_refr[i];
  if (cr < 0 && ct < 0) return;
  const int s = A.parent_src != nullptr ? A.parent_src[i] : (int)i;
  int ocr = s >= 0 ? A.old_child_refl[s] : -1;
  const int oct = s >= 0 ? A.old_child_refr[s] : -1;
  // (a traced parent's normal plane comes from the current attributes already)
  const bool renormal = s >= 0 && raytree_normal_dirty(A.attr, A.parent, i);
  if (renormal) {
    raytree_wave_count(A.attr.count + kRayTreeAttrRespawned, cr >= 0 && ocr >= 0);
    ocr = -1;
  }
  const V3 dir = v3_load(A.parent.ray + i * 6 + 3);
  const V3 Pt = v3_load(A.parent.point + i * 3);
  const double coef = A.parent.coef[i];
  const bool in_object = A.parent.in_object[i] != 0;
  if (cr >= 0) {
    A.child_src[cr] = ocr;
    A.child.spawn[cr] = ocr < 0 ? 1 : 0;
    A.child.coef[cr] = coef * A.mtls[raytree_effective_material(A.parent, A.tri_mtl, i)].reflectance;  // :187
    if (ocr < 0) {  // raytree_spawn_kernel's reflected child
      // as GetNormal returned it, :38 (layer 0's normal plane waits for the commit: the effective normal)
      V3 Nn = renormal ? raytree_attr_at(A.attr, A.attr.tri_normal, A.parent, i) : v3_load(A.parent.normal + i * 3);
      if (dot(Nn, -dir) < 0.0) Nn = -Nn;         // :42-45
      const V3 Rd = dir - Nn * (2 * dot(dir, Nn));  // :68-69
      const V3 ro = Pt + (Rd * 0.0001);             // :70-74
      double *r = A.child.ray + (size_t)cr * 6;
      r[0] = ro.x; r[1] = ro.y; r[2] = ro.z; r[3] = Rd.x; r[4] = Rd.y; r[5] = Rd.z;
      A.child.in_object[cr] = in_object ? 1 : 0;
    }
  }
  if (ct >= 0) {
    A.child_src[ct] = oct;
    A.child.spawn[ct] = oct < 0 ? 1 : 0;
    A.child.coef[ct] = coef;  // :223
    if (oct < 0) {  // raytree_spawn_kernel's refracted child
      const V3 rdir = normalized(dir);  // :208-212 (direction unchanged, re-normalised)
      const V3 ro = Pt + rdir * 0.00001;
      double *r = A.child.ray + (size_t)ct * 6;
      r[0] = ro.x; r[1] = ro.y; r[2] = ro.z; r[3] = rdir.x; r[4] = rdir.y; r[5] = rdir.z;
      A.child.in_object[ct] = in_object ? 0 : 1;  // :222
    }
  }
}

struct RayTreeRegrowCopyArgs {
  RayTreeLayer from, to;          // the OLD layer and the new one
  const int32_t *src;             // [n_to]
  uint32_t n_from, n_to;
  int32_t n_lights;
  int32_t n_materials;
  const mt_material *mtls;        // the scene's CURRENT materials
  const DevTexture *texs;         // and its CURRENT textures
  const uint8_t *albedo_changed;  // [n_materials], nullptr: no albedo to rewrite for a material's own sake
  const int32_t *tri_mtl;         // the scene's CURRENT assignment while a reassignment is pending, else nullptr
  RayTreeAttr attr;               // pending attribute edits: raytree_reattr_kernel's rule for the kept rays (counted)
};

__global__ __launch_bounds__(256) void raytree_regrow_copy_kernel(RayTreeRegrowCopyArgs A) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= (size_t)A.n_to) return;
  const int src = A.src[j];
  if (src < 0) return;
  const size_t s = (size_t)src, n_from = (size_t)A.n_from, n_to = (size_t)A.n_to;
  store3(A.to.ray, j * 2, v3_load(A.from.ray + s * 6));
  store3(A.to.ray, j * 2 + 1, v3_load(A.from.ray + s * 6 + 3));
  A.to.in_object[j] = A.from.in_object[s];
  store3(A.to.point, j, v3_load(A.from.point + s * 3));
  const bool nd = raytree_normal_dirty(A.attr, A.from, s), ud = raytree_uvw_dirty(A.attr, A.from, s);
  store3(A.to.normal, j, nd ? raytree_attr_at(A.attr, A.attr.tri_normal, A.from, s) : v3_load(A.from.normal + s * 3));
  const int was = A.from.material[s];
  const int mtl = raytree_effective_material(A.from, A.tri_mtl, s);
  A.to.material[j] = mtl;
  if (A.to.tri != nullptr) A.to.tri[j] = A.from.tri[s];
  if (A.attr.count != nullptr) {
    raytree_wave_count(A.attr.count + kRayTreeAttrNormal, nd);
    raytree_wave_count(A.attr.count + kRayTreeAttrUVW, ud);
  }
  if (!ud && A.to.uvw != nullptr) store3(A.to.uvw, j, v3_load(A.from.uvw + s * 3));
  if (ud) {  // uvw' in the stored uvw's place, for the plane and for the albedo whatever else changed
    const V3 uvw = raytree_attr_at(A.attr, A.attr.tri_uvw, A.from, s);
    if (A.to.uvw != nullptr) store3(A.to.uvw, j, uvw);
    store3(A.to.albedo, j, raytree_albedo_at(A.mtls, A.texs, mtl, uvw));
  } else if (mtl != was) {
    store3(A.to.albedo, j, raytree_restated_albedo(A.mtls, A.texs, mtl, A.from.uvw, s));
  } else if (A.albedo_changed != nullptr && mtl >= 0 && mtl < A.n_materials && A.albedo_changed[mtl] != 0) {
    store3(A.to.albedo, j, retextured_albedo(A.mtls + mtl, A.texs, A.from.uvw, s));
  } else {
    store3(A.to.albedo, j, v3_load(A.from.albedo + s * 3));
  }
  for (int li = 0; li < A.n_lights; li++) {
    store3(A.to.power, (size_t)li * n_to + j, v3_load(A.from.power + ((size_t)li * n_from + s) * 3));
    A.to.in_shadow[(size_t)li * n_to + j] = A.from.in_shadow[(size_t)li * n_from + s];
  }
}

struct RayTreeRegrowListArgs {
  RayTreeLayer L, tmp;  // the new layer (child_refl = the traced rays' places in tmp, -1 = kept) and the dense list
  uint32_t n_rays;      // of L
  uint32_t n_list;      // of tmp
  int32_t n_lights;
};

__global__ __launch_bounds__(256) void raytree_regrow_gather_kernel(RayTreeRegrowListArgs A) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= (size_t)A.n_rays) return;
  const int place = A.L.child_refl[j];
  if (place < 0) return;
  const size_t p = (size_t)place;
  store3(A.tmp.ray, p * 2, v3_load(A.L.ray + j * 6));
  store3(A.tmp.ray, p * 2 + 1, v3_load(A.L.ray + j * 6 + 3));
  A.tmp.coef[p] = A.L.coef[j];
  A.tmp.in_object[p] = A.L.in_object[j];
}

__global__ __launch_bounds__(256) void raytree_regrow_scatter_kernel(RayTreeRegrowListArgs A) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= (size_t)A.n_rays) return;
  const int place = A.L.child_refl[j];
  if (place < 0) return;
  const size_t p = (size_t)place, n = (size_t)A.n_rays, m = (size_t)A.n_list;
  store3(A.L.point, j, v3_load(A.tmp.point + p * 3));
  store3(A.L.normal, j, v3_load(A.tmp.normal + p * 3));
  store3(A.L.albedo, j, v3_load(A.tmp.albedo + p * 3));
  A.L.material[j] = A.tmp.material[p];
  if (A.L.uvw != nullptr) store3(A.L.uvw, j, v3_load(A.tmp.uvw + p * 3));
  if (A.L.tri != nullptr) A.L.tri[j] = A.tmp.tri[p];
  for (int li = 0; li < A.n_lights; li++) {
    store3(A.L.power, (size_t)li * n + j, v3_load(A.tmp.power + ((size_t)li * m + p) * 3));
    A.L.in_shadow[(size_t)li * n + j] = A.tmp.in_shadow[(size_t)li * m + p];
  }
  A.L.spawn[j] = A.tmp.spawn[p];
}

}  // namespace mt
