// mt_gbuffer.h — the primary-hit G-buffer: what the first call of TraceRayWorker (mythtracer.cc:18-64) knows about
// a pixel before it looks at a light, written out as planes instead of being folded into a colour.
//
// Per pixel, the frame kernels' own arithmetic in their own order (mt_render.hip, sm_engine, stage 1): Sensor::GetRay
// (camera.cc:65-69), OctTree::IntersectRay from the camera origin (trace_wave), and on a hit
//   depth     t, the Moeller-Trumbore distance along the normalised ray
//   point     origin + direction t                               (primitive_triangle.cc:141)
//   normal    Triangle::GetNormal(point): Heron-area weights      (primitive_triangle.cc:27-60)
//   uvw       Triangle::GetUVW(point), the same weights           (primitive_triangle.cc:62-79)
//   albedo    material.ambient, times Texture::GetColorAt(u, v) where the material has a texture (mythtracer.cc:58-64)
//   prim      the AddPrimitive index of the triangle (mt_scene_desc::tri_id)
//   line_no   Primitive::debug_line_no
//   material  index into mt_scene_desc::materials, -1 = the triangle has none (then albedo = NaN)
// The normal is what GetNormal RETURNS: it is NOT flipped towards the camera (mythtracer.cc:42-45 does that to its
// own copy afterwards).  No lights, no recursion.  A miss: NaN in the f64 planes, -1 in the int planes.  NaN texture
// coordinates (degenerate triangle): albedo = what texture_color_at defines for them (NaN).
//
// Execution model: primary_kernel's.  Persistent waves pull 8x8-pixel blocks of the chunk from one counter, one lane
// per pixel -- a wave's 64 rays are neighbours, which is what the wave-synchronous walk is fast on -- and blocks cut by
// the right or bottom edge run with inactive lanes.  Persistent rather than one wave per block: the grid, the LDS
// size and the per-wave global areas of the DEEP layouts are then the frame kernels' (configure_launch, ensure_deep),
// whatever the chunk's size -- a grid of one wave per block would need a DEEP area per BLOCK (32 400 of them at 1080p).
// Every plane is optional (nullptr): the pointers are kernel arguments, hence wave-uniform (SGPRs), and what no
// requested plane needs is not computed -- only the trace itself always runs.  Included behind mt_render.hip
// (fetch_work, flush_item_stats).
#pragma once
#include "mt_shade.h"

namespace mt {

// The planes, all optional; `tri_id` (stream index -> AddPrimitive index) is read for `prim` only.
struct GBufferPlanes {
  double *depth, *point, *normal, *uvw, *albedo;  // 1, 3, 3, 3, 3 doubles per pixel
  int32_t *prim, *line_no, *material;
  const int32_t *tri_id;
};

struct GBufferArgs {
  mt_sensor sensor;
  int32_t chunk_x, chunk_y, chunk_w, chunk_h;  // in image coordinates; the planes are chunk-local row-major
  int32_t blocks_x;                            // 8x8 blocks per row of the chunk
  uint32_t n_items;                            // blocks of the chunk
  GBufferPlanes planes;
  unsigned long long *counters;                // ST_COUNT
  unsigned int *work_counter;                  // zero at launch
};

__device__ __forceinline__ void store3(double *plane, size_t px, V3 v) {
  double *o = plane + px * 3;
  o[0] = v.x; o[1] = v.y; o[2] = v.z;
}

// What a pixel's primary trace found, as far as a caller of write_gbuffer_planes asked for it
struct PrimaryHit {
  V3 point;  // origin + direction t (NaN on a miss, or when neither a plane nor the caller needs it)
  int mtl;   // the triangle's material, -1 = none / miss / not needed
};

// One pixel's planes from its primary trace `to` (ray origin + rd t): the part of the G-buffer after the trace, shared
// by gbuffer_kernel and lightbuffer_kernel (mt_lightbuffer.h).  What no requested plane needs is not computed;
// need_hit: the caller wants point and material whatever the planes say.
template <bool STATS>
__device__ __forceinline__ PrimaryHit write_gbuffer_planes(const DevScene &S, const GBufferPlanes &A, size_t px, V3 origin,
                                                           V3 rd, const TraceOut &to, LaneStats &st, bool need_hit) {
  const MT_CONST mt_material *mtls = as_const(S.mtls);
  // which intermediate values does some requested plane need?  (wave-uniform)
  const bool want_albedo = A.albedo != nullptr;
  const bool want_mtl = A.material != nullptr || want_albedo || need_hit;
  const bool want_uvw = A.uvw != nullptr;
  const bool want_bary = A.normal != nullptr || want_uvw || want_albedo;  // (albedo: textured materials only, per lane)
  const V3 nan3 = v3(__builtin_nan(""), __builtin_nan(""), __builtin_nan(""));
  const int prim = to.prim;
  const bool hit = prim >= 0;
  if (STATS) {
    st.v[ST_RAYS_PRIMARY]++;
    if (hit) st.v[ST_SHADED_HITS]++;
  }
  if (A.depth) A.depth[px] = hit ? to.t : __builtin_nan("");
  if (A.line_no) A.line_no[px] = hit ? S.tri_line[prim] : -1;
  if (A.prim) A.prim[px] = hit ? A.tri_id[prim] : -1;
  V3 Pt = nan3, Nn = nan3, uvw = nan3, surf = nan3;
  int mtl = -1;
  if (hit) {
    if (A.point != nullptr || want_bary || need_hit) Pt = origin + rd * to.t;  // primitive_triangle.cc:141
    if (want_mtl) mtl = S.tri_mtl[prim];
    const bool textured = want_albedo && mtl >= 0 && mtls[mtl].tex >= 0;
    if (A.normal != nullptr || want_uvw || textured) {
      const Bary w = barycentric(S.tri_vertex + (size_t)prim * 9, Pt);
      if (A.normal) Nn = interpolate(S.tri_normal + (size_t)prim * 9, w);  // GetNormal; no flip
      if (want_uvw || textured) uvw = interpolate(S.tri_uvw + (size_t)prim * 9, w);
      if (STATS) st.v[ST_BYTES_VECTOR] += 72u + (A.normal ? 72u : 0u) + ((want_uvw || textured) ? 72u : 0u);
    }
    if (want_albedo && mtl >= 0) {  // mythtracer.cc:58-64
      const MT_CONST mt_material *m = mtls + mtl;
      surf = v3(m->ambient[0], m->ambient[1], m->ambient[2]);
      if (textured) surf = surf * texture_color_at(S.texs[m->tex], uvw.x, uvw.y);
    }
  }
  if (A.point) store3(A.point, px, Pt);
  if (A.normal) store3(A.normal, px, Nn);
  if (A.uvw) store3(A.uvw, px, uvw);
  if (A.albedo) store3(A.albedo, px, surf);
  if (A.material) A.material[px] = mtl;
  if (STATS) {
    st.v[ST_BYTES_VECTOR] += (A.depth ? 8u : 0u) + (A.point ? 24u : 0u) + (A.normal ? 24u : 0u) + (A.uvw ? 24u : 0u) +
                             (A.albedo ? 24u : 0u) + (A.prim ? 4u : 0u) + (A.line_no ? 4u : 0u) + (A.material ? 4u : 0u);
  }
  return PrimaryHit{Pt, mtl};
}

template <bool STATS, int DEEP>
__global__ __launch_bounds__(256, MT_WAVES_PER_SIMD) void gbuffer_kernel(DevScene S, GBufferArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave_in_block = threadIdx.x >> 6;
  WaveStack stk;
  stk.bind(smem, wave_in_block, S.tree_depth, S.pack_shift, DEEP != 0);
  LaneStats st;
  st.clear();
  const V3 cam_origin = v3_load(A.sensor.origin);
  const V3 s_start = v3_load(A.sensor.start_point);
  const V3 s_ds = v3_load(A.sensor.delta_scanline);
  const V3 s_dp = v3_load(A.sensor.delta_pixel);
  for (;;) {
    const unsigned item = fetch_work(A.work_counter, lane);
    if (item >= A.n_items) break;
    const int lx = (int)(item % (unsigned)A.blocks_x) * 8 + (lane & 7);
    const int ly = (int)(item / (unsigned)A.blocks_x) * 8 + (lane >> 3);
    const bool want = lx < A.chunk_w && ly < A.chunk_h;
    const size_t px = (size_t)ly * (size_t)A.chunk_w + (size_t)lx;
    V3 rd = v3(0, 0, 1);
    if (want) {  // Sensor::GetRay, camera.cc:65-69
      const V3 d = s_start + (s_ds * (double)(A.chunk_y + ly)) + (s_dp * (double)(A.chunk_x + lx));
      rd = normalized(d);
    }
    const TraceOut to = trace_wave<STATS, DEEP>(S.self, stk.base, lane, want, cam_origin.x, cam_origin.y, cam_origin.z,
                                                rd.x, rd.y, rd.z);
    add_trace_stats<STATS>(st, to);
    if (to.status != DEV_OK) {
      if (lane == 0) atomicMax(A.counters + ST_STATUS, (unsigned long long)to.status);
      break;
    }
    if (want) (void)write_gbuffer_planes<STATS>(S, A.planes, px, cam_origin, rd, to, st, false);
    flush_item_stats<STATS>(st, A.counters, lane);
  }
}

// ---- edited textures (include/mythtracer_hip.h, mt_scene_set_texture ff.) ----
// A texture touches exactly one stored quantity, the albedo, and that is arithmetic over a stored uvw: the rule of
// write_gbuffer_planes above (mythtracer.cc:58-64), the same expressions in the same order, from memory instead of from
// the trace.  Shared by gbuffer_retexture_kernel, raytree_recommit_kernel and raytree_regrow_copy_kernel
// (mt_raytree.h).  `uvw` may be nullptr where no material the caller lets through has a texture.
__device__ __forceinline__ V3 retextured_albedo(const mt_material *m, const DevTexture *texs, const double *uvw, size_t i) {
  V3 surf = v3(m->ambient[0], m->ambient[1], m->ambient[2]);
  if (m->tex >= 0 && uvw != nullptr) {
    const V3 c = v3_load(uvw + i * 3);
    surf = surf * texture_color_at(texs[m->tex], c.x, c.y);
  }
  return surf;
}

// gbuffer_retexture_kernel: the albedo plane of a stored G-buffer again under the scene's CURRENT materials and
// textures, from its material and uvw planes -- no sensor, no traversal, a plain grid, one thread per pixel.  A material
// outside 0 .. n_materials - 1 (a miss, "no material", or anything else a caller's plane may hold) gets NaN, what
// write_gbuffer_planes stores for a miss.
struct GBufferRetextureArgs {
  const int32_t *material;  // [n]
  const double *uvw;        // [n][3]; nullptr: no current material has a texture
  double *albedo;           // [n][3]
  const mt_material *mtls;
  const DevTexture *texs;
  unsigned long long n;
  int32_t n_materials;
};

__global__ __launch_bounds__(256) void gbuffer_retexture_kernel(GBufferRetextureArgs A) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)A.n) return;
  const int mtl = A.material[i];
  const double nan = __builtin_nan("");
  V3 surf = v3(nan, nan, nan);
  if (mtl >= 0 && mtl < A.n_materials) surf = retextured_albedo(A.mtls + mtl, A.texs, A.uvw, i);
  store3(A.albedo, i, surf);
}

#define MT_INSTANTIATE_GB(DEEP_)                                                    \
  template __global__ void gbuffer_kernel<true, DEEP_>(DevScene, GBufferArgs);      \
  template __global__ void gbuffer_kernel<false, DEEP_>(DevScene, GBufferArgs);
MT_INSTANTIATE_GB(0)
MT_INSTANTIATE_GB(1)
MT_INSTANTIATE_GB(2)
#undef MT_INSTANTIATE_GB

}  // namespace mt
