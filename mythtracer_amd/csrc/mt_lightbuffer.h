// mt_lightbuffer.h — the direct-light buffer and the deferred relight pass: the part of TraceRayWorker between the
// G-buffer (mt_gbuffer.h) and the recursion (mythtracer.cc:66-177), cut where geometry ends and light colours begin.
//
// lightbuffer_kernel: per pixel and light, the shadow loop of mythtracer.cc:90-156 -- from the primary hit towards the
// light, through every transparent occluder -- with the frame kernels' arithmetic (mt_render.hip, sm_engine, the
// MODE_SHADOW branch of stage 1), and what it leaves behind:
//   power      light_power when the loop ends, BEFORE :159-161 raise it to light.ambient
//   in_shadow  0 = lit, 1 = in_shadow, 255 = the reference never enters the light loop for this pixel (a miss, or a
//              hit on a triangle without a material, :23-31 and :49-52); power is NaN there
// An occluder without a material is opaque, as in the frame kernels.  Both depend on geometry, materials and the light's
// POSITION only.  Planes: power [n_lights][chunk_h][chunk_w][3] doubles, in_shadow [n_lights][chunk_h][chunk_w] bytes.
// The G-buffer planes of the same primary trace come from the same launch if asked for (write_gbuffer_planes).
//
// Execution model: gbuffer_kernel's (persistent waves, 8x8 blocks from one counter, one lane per pixel).  After the
// primary trace_wave the wave walks the lights one after the other (wave-uniform loop); within a light every lane
// runs its own shadow loop, one trace_wave per iteration with want = "this lane's loop is still running", until no
// lane wants.  start point, light power and the traversing flag live in registers: there is no recursion, so nothing
// is parked.
//
// lightbuffer_update_kernel: the same loops for a LIST of lights from a stored G-buffer's point and material planes,
// without the primary trace: what a moved light costs.  The loop body is restated there, lightbuffer_kernel is as it was.
//
// shade_direct_kernel: mythtracer.cc:38-177 for one pixel from the stored planes -- point, unflipped normal, albedo,
// material (G-buffer), power and in_shadow (light buffer) -- and a list of lights whose colours may have changed
// since: no traversal, one thread per pixel, fp64 in the reference's order of operations (this translation unit is
// built with -ffp-contract=off), so that the bytes are those of a frame at max_depth = 0.
#pragma once
#include "mt_gbuffer.h"

namespace mt {

struct LightBufferArgs {
  mt_sensor sensor;
  int32_t chunk_x, chunk_y, chunk_w, chunk_h;
  int32_t blocks_x;
  uint32_t n_items;
  GBufferPlanes planes;          // all optional
  double *power;                 // optional
  uint8_t *in_shadow;            // optional
  unsigned long long *counters;  // ST_COUNT
  unsigned int *work_counter;    // zero at launch
};

template <bool STATS, int DEEP>
__global__ __launch_bounds__(256, MT_WAVES_PER_SIMD) void lightbuffer_kernel(DevScene S, LightBufferArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave_in_block = threadIdx.x >> 6;
  WaveStack stk;
  stk.bind(smem, wave_in_block, S.tree_depth, S.pack_shift, DEEP != 0);
  const MT_CONST mt_material *mtls = as_const(S.mtls);
  const MT_CONST mt_light *lights = as_const(S.lights);
  LaneStats st;
  st.clear();
  const V3 cam_origin = v3_load(A.sensor.origin);
  const V3 s_start = v3_load(A.sensor.start_point);
  const V3 s_ds = v3_load(A.sensor.delta_scanline);
  const V3 s_dp = v3_load(A.sensor.delta_pixel);
  const size_t npx = (size_t)A.chunk_w * (size_t)A.chunk_h;
  // every iteration of a shadow loop crosses another surface
  const int iteration_bound = S.n_tris + 2;
  bool failed = false;
  while (!failed) {
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
    V3 Pt = v3(0, 0, 0);
    bool lit = false;  // does the reference enter the light loop for this pixel?
    if (want) {
      const PrimaryHit h = write_gbuffer_planes<STATS>(S, A.planes, px, cam_origin, rd, to, st, true);
      lit = to.prim >= 0 && h.mtl >= 0;
      if (lit) Pt = h.point;
    }
    for (int li = 0; li < S.n_lights && !failed; li++) {
      const MT_CONST mt_light *lt = lights + li;
      const V3 lpos = v3(lt->position[0], lt->position[1], lt->position[2]);
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
        const size_t at = (size_t)li * npx + px;
        if (A.power) {
          const double nan = __builtin_nan("");
          store3(A.power, at, lit ? lp : v3(nan, nan, nan));
        }
        if (A.in_shadow) A.in_shadow[at] = lit ? (in_shadow ? 1 : 0) : 255;
        if (STATS) st.v[ST_BYTES_VECTOR] += (A.power ? 24u : 0u) + (A.in_shadow ? 1u : 0u);
      }
    }
    flush_item_stats<STATS>(st, A.counters, lane);
  }
}

// lightbuffer_update_kernel: the planes of the LISTED lights again, from the stored primary hits -- the G-buffer's
// `point` and `material` planes hold, bit for bit, the two things a shadow loop takes from the primary trace.  No
// sensor, no primary trace_wave; the planes of the other lights are not touched.  A work item is one 8x8 block of the
// chunk x one listed light (item = k n_blocks + block: neighbouring items are neighbouring blocks of one light), so
// that one light on a small chunk still fills the chip.  A pixel's loop runs when point[0] is not NaN and
// 0 <= material < n_materials (the plane is the caller's; the index itself is never read with); every other pixel
// of the chunk gets NaN / 255.  Lit pixels are NOT compacted across blocks: the walk is wave-synchronous and lives on
// the coherence of an 8x8 block's rays.
constexpr int kUpdateArgLights = 8;  // indices that travel with the launch; more in device memory

struct LightUpdateArgs {
  int32_t chunk_w, chunk_h;
  int32_t blocks_x;
  uint32_t n_blocks;                 // 8x8 blocks of the chunk
  uint32_t n_items;                  // n_blocks x listed lights
  const double *point;               // G-buffer planes of the chunk
  const int32_t *material;
  int32_t n_materials;
  double *power;                     // optional; [n_lights][chunk_h][chunk_w][3], plane l written for listed l only
  uint8_t *in_shadow;                // optional
  const int32_t *d_idx;              // the list when it has more than kUpdateArgLights entries, else nullptr
  int32_t idx[kUpdateArgLights];
  unsigned long long *counters;      // ST_COUNT
  unsigned int *work_counter;        // zero at launch
};

template <bool STATS, int DEEP>
__global__ __launch_bounds__(256, MT_WAVES_PER_SIMD) void lightbuffer_update_kernel(DevScene S, LightUpdateArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave_in_block = threadIdx.x >> 6;
  WaveStack stk;
  stk.bind(smem, wave_in_block, S.tree_depth, S.pack_shift, DEEP != 0);
  const MT_CONST mt_material *mtls = as_const(S.mtls);
  const MT_CONST mt_light *lights = as_const(S.lights);
  LaneStats st;
  st.clear();
  const size_t npx = (size_t)A.chunk_w * (size_t)A.chunk_h;
  const int iteration_bound = S.n_tris + 2;
  bool failed = false;
  for (;;) {
    const unsigned item = fetch_work(A.work_counter, lane);
    if (item >= A.n_items) break;
    const unsigned k = item / A.n_blocks, block = item % A.n_blocks;  // (wave-uniform)
    const int li = A.d_idx != nullptr ? A.d_idx[k] : A.idx[k];
    const int lx = (int)(block % (unsigned)A.blocks_x) * 8 + (lane & 7);
    const int ly = (int)(block / (unsigned)A.blocks_x) * 8 + (lane >> 3);
    const bool want = lx < A.chunk_w && ly < A.chunk_h;
    const size_t px = (size_t)ly * (size_t)A.chunk_w + (size_t)lx;
    V3 Pt = v3(0, 0, 0);
    bool lit = false;
    if (want) {
      const V3 p = v3_load(A.point + px * 3);
      const int mtl = A.material[px];
      lit = p.x == p.x && mtl >= 0 && mtl < A.n_materials;
      if (lit) Pt = p;
      if (STATS) st.v[ST_BYTES_VECTOR] += 24u + 4u;
    }
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
    if (failed) break;
    if (want) {
      const size_t at = (size_t)li * npx + px;
      if (A.power) {
        const double nan = __builtin_nan("");
        store3(A.power, at, lit ? lp : v3(nan, nan, nan));
      }
      if (A.in_shadow) A.in_shadow[at] = lit ? (in_shadow ? 1 : 0) : 255;
      if (STATS) st.v[ST_BYTES_VECTOR] += (A.power ? 24u : 0u) + (A.in_shadow ? 1u : 0u);
    }
    flush_item_stats<STATS>(st, A.counters, lane);
  }
}

// The lights of a relight: up to kShadeArgLights travel as a kernel argument, more in device memory.
constexpr int kShadeArgLights = 8;

struct ShadeDirectArgs {
  mt_sensor sensor;
  int32_t chunk_x, chunk_y, chunk_w, chunk_h;
  const double *point, *normal, *albedo;  // G-buffer planes, 3 doubles per pixel
  const int32_t *material;
  const double *power;                    // light buffer, [n_lights][chunk_h][chunk_w][3]
  const uint8_t *in_shadow;               // [n_lights][chunk_h][chunk_w]
  const mt_material *mtls;
  int32_t n_materials;                    // a material index outside 0 .. n_materials - 1 counts as "no material"
  const mt_light *d_lights;               // ARG_LIGHTS = false
  int32_t n_lights;
  uint8_t *out_rgb;                       // chunk-local row-major RGB8
  mt_light lights[kShadeArgLights];       // ARG_LIGHTS = true
};

template <bool ARG_LIGHTS>
__global__ __launch_bounds__(256) void shade_direct_kernel(ShadeDirectArgs A) {
  const size_t npx = (size_t)A.chunk_w * (size_t)A.chunk_h;
  const size_t px = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (px >= npx) return;
  const int lx = (int)(px % (size_t)A.chunk_w), ly = (int)(px / (size_t)A.chunk_w);
  uint8_t *o = A.out_rgb + px * 3;
  const V3 Pt = v3_load(A.point + px * 3);
  if (Pt.x != Pt.x) {  // a miss: background, mythtracer.cc:23-31
    o[0] = 0; o[1] = 0; o[2] = 0;
    return;
  }
  // Sensor::GetRay, camera.cc:65-69
  const V3 d = v3_load(A.sensor.start_point) + (v3_load(A.sensor.delta_scanline) * (double)(A.chunk_y + ly)) +
               (v3_load(A.sensor.delta_pixel) * (double)(A.chunk_x + lx));
  const V3 dir = normalized(d);
  V3 Nn = v3_load(A.normal + px * 3);  // as GetNormal returned it, :38
  const V3 towards_camera = -dir;
  double normal_ray_dot = dot(Nn, towards_camera);
  if (normal_ray_dot < 0.0) {  // :42-45
    Nn = -Nn;
    normal_ray_dot = dot(Nn, towards_camera);
  }
  // (the plane is the caller's: an index the scene does not have -- a G-buffer of another scene -- must not be read with)
  const int mtl = A.material[px];
  V3 color = v3(0, 0, 0);
  if (mtl < 0 || mtl >= A.n_materials) {  // :49-52
    normal_ray_dot = (normal_ray_dot + 1.0) * 0.5;
    color = v3(normal_ray_dot, normal_ray_dot, normal_ray_dot);
  } else {
    const mt_material *m = A.mtls + mtl;
    const V3 surf = v3_load(A.albedo + px * 3);             // :58-64
    const V3 Rd = dir - Nn * (2 * dot(dir, Nn));            // :68-69
    const double refl_dot = dot(Rd, towards_camera);        // :170
    const V3 kd = v3(m->diffuse[0], m->diffuse[1], m->diffuse[2]);
    for (int li = 0; li < A.n_lights; li++) {
      const mt_light *lt = ARG_LIGHTS ? A.lights + li : A.d_lights + li;
      const V3 lpos = v3(lt->position[0], lt->position[1], lt->position[2]);
      const V3 amb = v3(lt->ambient[0], lt->ambient[1], lt->ambient[2]);
      const V3 ld = normalized(lpos - Pt);                  // :79-80
      color = color + amb * surf;                           // :83-84
      const size_t at = (size_t)li * npx + px;
      V3 lp = v3_load(A.power + at * 3);
      lp.x = std_max(lp.x, amb.x);                          // :159-161
      lp.y = std_max(lp.y, amb.y);
      lp.z = std_max(lp.z, amb.z);
      const V3 ldiff = v3(lt->diffuse[0], lt->diffuse[1], lt->diffuse[2]);
      color = color + kd * surf * dot(ld, Nn) * ldiff * lp;  // :163-167
      if (A.in_shadow[at] == 0 && refl_dot > 0) {           // :169-177
        const V3 ks = v3(m->specular[0], m->specular[1], m->specular[2]);
        const V3 ls = v3(lt->specular[0], lt->specular[1], lt->specular[2]);
        color = color + ks * surf * ::pow(refl_dot, m->specular_exp) * ls;
      }
    }
  }
  o[0] = channel_to_u8(color.x);  // V3DtoRGB, :235-241
  o[1] = channel_to_u8(color.y);
  o[2] = channel_to_u8(color.z);
}

#define MT_INSTANTIATE_LB(DEEP_)                                                         \
  template __global__ void lightbuffer_kernel<true, DEEP_>(DevScene, LightBufferArgs);   \
  template __global__ void lightbuffer_kernel<false, DEEP_>(DevScene, LightBufferArgs);  \
  template __global__ void lightbuffer_update_kernel<true, DEEP_>(DevScene, LightUpdateArgs);   \
  template __global__ void lightbuffer_update_kernel<false, DEEP_>(DevScene, LightUpdateArgs);
MT_INSTANTIATE_LB(0)
MT_INSTANTIATE_LB(1)
MT_INSTANTIATE_LB(2)
#undef MT_INSTANTIATE_LB
template __global__ void shade_direct_kernel<true>(ShadeDirectArgs);
template __global__ void shade_direct_kernel<false>(ShadeDirectArgs);

}  // namespace mt
