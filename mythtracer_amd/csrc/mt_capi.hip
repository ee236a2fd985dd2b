// mt_capi.hip — host side of libmythtracer_hip.so: the C ABI declared in
// include/mythtracer_hip.h.  Validates the flattened scene (so that the kernel
// can index it without bounds checks), keeps it resident in HBM and launches
// the kernels of mt_render.hip.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <limits>
#include <utility>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unistd.h>
#include <vector>

// Single translation unit: the kernels are compiled together with their host
// side so that no relocatable device code is needed.
#include "mt_render.hip"
#include "mt_resolve.h"
#include "mt_adaptive.h"
#include "mt_gbuffer.h"
#include "mt_lightbuffer.h"
#include "mt_raytree.h"
#include "mt_build.h"
#include "mt_layout.h"
#include "mt_host_tree.h"
#include "mt_move.h"
#include "mt_edit.h"

using namespace mt;

namespace {

thread_local char g_err[1024] = "";

int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

int fail(const LayoutError &err) { return fail(err.code, "%s", err.msg.c_str()); }
int fail(const MoveError &err) { return fail(err.code, "%s", err.msg.c_str()); }

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(MT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),    \
                  __FILE__, __LINE__);                                                  \
  } while (0)


// MT_OK or return the MT_ERR_* of `expr`
#define MT_TRY(expr)                                                                    \
  do {                                                                                  \
    const int rc_ = (expr);                                                             \
    if (rc_ != MT_OK) return rc_;                                                       \
  } while (0)

// The text g_err holds now, to fail with again after a clean-up that may overwrite it (a destroy, a configure, a fail
// that quotes it)
struct KeptError {
  const std::string text = g_err;
  int fail_again(int rc) const { return fail(rc, "%s", text.c_str()); }
};

// hipMalloc of `bytes` (at least one) for `what`: an allocation that does not fit is MT_ERR_NOMEM, *p is NULL then
int device_malloc(void **p, size_t bytes, const char *what) {
  const hipError_t e = hipMalloc(p, bytes ? bytes : 1);
  if (e == hipSuccess) return MT_OK;
  (void)hipGetLastError();
  *p = nullptr;
  if (e == hipErrorOutOfMemory) return fail(MT_ERR_NOMEM, "no room for the %zu bytes of %s", bytes, what);
  return fail(MT_ERR_HIP, "hipMalloc of %zu bytes for %s failed: %s", bytes, what, hipGetErrorString(e));
}

// A move-only list of device allocations, freed with it.  Whatever alloc() and upload() hand out belongs to the list;
// ownership changes hands by swapping whole lists or single slots (the k-th allocation made is slot k), never by
// copying a pointer.
class DeviceAllocs {
  std::vector<void *> p_;

 public:
  DeviceAllocs() = default;
  DeviceAllocs(const DeviceAllocs &) = delete;
  DeviceAllocs &operator=(const DeviceAllocs &) = delete;
  DeviceAllocs(DeviceAllocs &&o) noexcept { p_.swap(o.p_); }
  ~DeviceAllocs() { free_all(); }
  void free_all() {
    for (void *q : p_) (void)hipFree(q);
    p_.clear();
  }
  void swap(DeviceAllocs &o) noexcept { p_.swap(o.p_); }
  void swap_slot(size_t slot, DeviceAllocs &o, size_t o_slot) { std::swap(p_.at(slot), o.p_.at(o_slot)); }
  // `count` elements (at least one) of new device memory; *out is const T * where only kernels read it, T * where its
  // owner writes it
  template <typename T, typename P>
  int alloc(size_t count, const char *what, P *out) {
    p_.reserve(p_.size() + 1);  // (no push_back that throws with the allocation in hand)
    void *d = nullptr;
    MT_TRY(device_malloc(&d, (count ? count : 1) * sizeof(T), what));
    p_.push_back(d);
    *out = (T *)d;
    return MT_OK;
  }
  // ... filled from `count` elements of `host`
  template <typename T, typename P>
  int upload(const T *host, size_t count, const char *what, P *out) {
    T *d = nullptr;
    MT_TRY(alloc<T>(count, what, &d));
    if (count) HIP_TRY(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
    *out = d;
    return MT_OK;
  }
  template <typename T, typename P>
  int upload(const std::vector<T> &host, const char *what, P *out) {
    return upload(host.data(), host.size(), what, out);
  }
};

constexpr size_t kLdsBudget = 160 * 1024;

// A growable scratch buffer that owns its allocation: device memory, or page-locked host memory (HOST).  It only grows
// -- a request above the capacity reallocates, at least 1 byte -- and is freed with its owner.
template <typename T, bool HOST = false>
struct Buf {
  T *p = nullptr;
  size_t bytes = 0;
  Buf() = default;
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
  ~Buf() {
    if (p) (void)(HOST ? hipHostFree(p) : hipFree(p));
  }
  operator T *() const { return p; }
  void swap(Buf &o) {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
  }
  int ensure(size_t need, unsigned host_flags = hipHostMallocDefault) {
    if (bytes >= need && p) return MT_OK;
    void **ptr = (void **)&p;
    if (p) HIP_TRY(HOST ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    bytes = 0;
    if (HOST) HIP_TRY(hipHostMalloc(ptr, need ? need : 1, host_flags));
    else HIP_TRY(hipMalloc(ptr, need ? need : 1));
    bytes = need;
    return MT_OK;
  }
};

// Tuning constants of the work order and of the engine choice, with the values the sweeps of DESIGN.md section 5
// settled on.  Changed through mt_scene_set_tuning only (tests, experiment scripts): the library reads no
// environment variable on the launch path.  (A -DMT_DEBUG_KNOBS build additionally reads its DUMP facilities --
// item cycles, unit counts, heartbeat, time line -- from the environment, once, in mt_scene_create.)
struct Tuning {
  double v[MT_TUNE_COUNT];
  Tuning() {
    for (double &x : v) x = 0.0;
    v[MT_TUNE_POOL_BELOW] = 9.0;          // blocks per resident wave below which a launch is taken to be tail-bound
    v[MT_TUNE_POOL_CAP] = 0.0;            // 0 = default capacity of a wave's ray pool
    v[MT_TUNE_PACKED_STACK] = 1.0;
    v[MT_TUNE_BLOCKS_PER_CU] = 0.0;       // 0 = as many as fit
    v[MT_TUNE_FORECAST_RADIUS] = -1.0;    // < 0 = 1 block, 2 when the origin moved
    v[MT_TUNE_BLEND] = 0.9;
    v[MT_TUNE_FORMS] = 1.0;
    v[MT_TUNE_POOL_CUT_SHARE] = -1.0;     // < 0 = 1.0 with history, 0.3 without
    v[MT_TUNE_POOL_PIECE_TIME1] = 0.35; v[MT_TUNE_POOL_PIECE_TIME2] = 0.12;
    v[MT_TUNE_POOL_PIECE_WORK1] = 1.1;  v[MT_TUNE_POOL_PIECE_WORK2] = 3.0;
    v[MT_TUNE_POOL_CELL_FACTOR] = 1.0;  // (round 4, swept on the panning 4K frame at N = 8: 3.0 / 2.0 / 1.5 / 1.2 / 1.0 / 0.85 / 0.7 / 0.5 -> 3.39 / 3.41 / 3.37 / 3.35 / 3.20 / 3.11 / 3.29 / 4.37 ms for the slowest rank; with HYBRID_WORK2 2.6: 3.06)
    v[MT_TUNE_QUAD_SHARE] = 0.95; v[MT_TUNE_QUAD_SHARE_MOVING] = 0.7;
    v[MT_TUNE_QUAD_KEEP] = 1.0;
    v[MT_TUNE_QUAD_WORK] = 1.7;   v[MT_TUNE_QUAD_WORK_MOVING] = 1.5;
    v[MT_TUNE_POOL_SCRATCH_MB] = 4096.0;  // automatic mode: above this the state machine renders (explicit engine 2: the cap shrinks)
    // hybrid launches: blocks above POOL_SHARE of an even split go to the ray pool in pieces, blocks above QUAD_SHARE to
    // the state machine as quarters with four lanes per pixel (swept on one rank's share of the 4K frame at N = 8,
    // scripts/hybrid_sweep.py: 0.8 / 0.9 / 1.0 / 1.15 / 1.3 -> slowest rank 3.90 / 3.65 / 3.65 / 3.72 / 3.92 ms; with the
    // quarters' threshold below the pool's the state machine's 1.7x work per quartered block comes back: +0.3 ms)
    v[MT_TUNE_HYBRID_POOL_SHARE] = 1.3;   // (swept with HYBRID_CELL_FACTOR at N = 8, panning: (1.0, 1.0) 3.03 ms, (1.3, 0.85) 2.88: fewer blocks through the pool as quarters, the cells' threshold where it was)
    v[MT_TUNE_HYBRID_CELL_FACTOR] = 0.85;
    v[MT_TUNE_HYBRID_QUAD_SHARE] = 1.0;
    v[MT_TUNE_FORECAST_STEP] = 8.0;       // pixels between the old-image positions a re-projected forecast takes its maximum over
    v[MT_TUNE_HYBRID_WORK1] = 1.3; v[MT_TUNE_HYBRID_WORK2] = 2.6;  // pool quarters / cells: summed cost over the state machine's whole-block cost
    v[MT_TUNE_HYBRID_STARTER_SHARE] = 0.33;  // hybrid launches: state-machine units above this share of an even split start with the launch (hybrid_kernel)
    v[MT_TUNE_DEEP_LAYOUT] = 1.0;
    v[MT_TUNE_MULTI_FORCE_PEER_COPY] = 0.0;
    v[MT_TUNE_MULTI_BALANCE] = 1.0;
    v[MT_TUNE_SM_CELL_SHARE] = 0.8;  // (x the quarters' cutting threshold; blocks with zero-component rays only: mt_order.h)
    v[MT_TUNE_SM_CELL_TIME] = 0.2;
    v[MT_TUNE_SM_CELL_WORK] = 3.0;
    v[MT_TUNE_ORDER_GROUPS] = (double)kOrdGroups;  // workgroups of the work-order kernels (mt_order.h)
    v[MT_TUNE_XCD_QUEUES] = 2.0;  // one work order per XCD over a 4 x 2 grid of regions of equal forecast cost (L2 hit rate 0.82 -> 0.92 room, 0.66 -> 0.82 loft)
    v[MT_TUNE_LEAN_KERNEL] = 1.0;  // the lean frame kernel where decide_launch finds its conditions met (0 never, 2 whatever the primary rays)
  }
};

// The lean frame kernel's guard (order_forecast_kernel): when a lean launch abandoned more than this share of its
// units, the scene's next kLeanHandoverFrames lean launches hand their whole order to the redo launch.  An abandoned
// unit costs the passes it ran before the ray the walk cannot take came up -- half of the unit when such rays come
// anywhere in it -- on top of its redo, which costs what the unit costs without a lean kernel: with a share f of the
// units abandoned the frame pays 0.5 f and gains g (1 - f), g being what the lean kernel saves on a unit it finishes.
// Break-even at f = g / (0.5 + g) = 0.07 for the g = 3.7 % measured on the room's panning frame (LABBOOK section D);
// the guard stays on the safe side of it.
constexpr float kLeanRedoShare = 0.04f;

// process-wide default of mt_scene_set_engine for scenes created from now on (mt_set_default_engine)
std::atomic<int> g_default_engine{0};

// The forecast state of a scene: what decide_launch, size_buffers and launch_render keep from one launch for the next
// -- the measured block costs, the geometry, camera and engine they belong to, and the buffers of the work order made
// from them.  A launch of another geometry starts it over, so two geometries that alternate each need their own: a
// scene has two banks.  Bank 0 serves every call; bank 1, allocated on first use, only the refinement launch of an
// adaptive chunk (mt_render_chunk_adaptive), which alternates with that chunk's plain launch.
struct ForecastBank {
  // cost feedback (schedule_kernel): valid for launches of the same geometry
  Buf<unsigned int> d_item_cost;       // [n_items]
  Buf<unsigned int> d_item_forecast;   // [n_items]
  Buf<unsigned int> d_item_forms;      // [2 n_items] cost of a block as one unit / as four quarters (forecast_kernel)
  Buf<unsigned char> d_item_form;      // [n_items] hybrid launches: how each block was rendered (hybrid_schedule_kernel)
  Buf<unsigned int> d_item_unit;
  Buf<unsigned short> d_item_cell;
  Buf<unsigned int> d_order_item;      // [4 n_items]
  Buf<signed char> d_order_sub;        // [4 n_items]
  Buf<unsigned int> d_redo_item;       // the lean frame kernel's abandoned units, sized like the order (first lean launch)
  Buf<signed char> d_redo_sub;
  // tile-list launches (mt_render_tile_list_device): the launch's own copy of the list, and tile -> slot (last_P
  // points at them)
  Buf<int32_t> d_tile_list;
  Buf<int32_t> d_tile_slot;
  mt_sensor cost_sensor{};                // camera of the launch that measured the costs
  unsigned long long cost_signature = 0;  // 0 = no history
  int forecasts_in_a_row = 0;  // launches with this geometry and camera whose work order came from a forecast
  int last_engine = 0;         // engine of the previous launch (cost histories are per engine)
  bool last_history = false;   // LaunchPlan::history of the previous launch
  RenderParams last_P{};       // geometry of the last launch (mt_scene_export_costs_device)
  bool last_P_valid = false;
  unsigned long long launches = 0;                 // launches of this bank so far
  unsigned long long cost_map_for_launch = ~0ull;  // the scene's cost map describes the frame of launch number ... (`launches` then)
  mt_sensor irr_sensor{};      // the sensor `irr_sensor_has` was found for (image irr_w x irr_h)
  int irr_w = 0, irr_h = 0, irr_sensor_has = 0;
  bool irr_sensor_valid = false;
};

// The scene's own, writable view of the per-triangle arrays that DevScene shows the kernels as const (the edit calls
// write them, a move regathers them)
struct TriArrays {
  double *vertex = nullptr, *normal = nullptr, *uvw = nullptr;  // DevScene::tri_vertex, tri_normal, tri_uvw
  int32_t *mtl = nullptr, *line = nullptr;                      // DevScene::tri_mtl, tri_line
};

}  // namespace

struct mt_scene {
  int device = 0;
  DevScene dev{};
  // The scene's uploads.  geo: the 13 arrays derived from the geometry (upload_derived) and the five of `tri`; a move
  // builds a new one aside and swaps it in whole.  tables: texture i's texels in slot i, then the materials and the
  // texture table; mt_scene_set_texture swaps slot i.
  DeviceAllocs geo, tables;
  TriArrays tri;
  mt_material *mtls = nullptr;  // dev.mtls and dev.texs for the scene's own writes
  DevTexture *texs = nullptr;
  Buf<mt_light> d_lights;
  Buf<unsigned long long> d_counters;
  Buf<unsigned int> d_work;
  Buf<unsigned int> d_queues;  // kQueueWords: the per-XCD work orders' counters and bounds (RenderParams::queues)
  Buf<unsigned int> d_order_ctl;  // kOrdWords: the work-order kernels' sums, histograms, grids (zero at creation, never reset by the host)
  Buf<unsigned int> d_order_whist; // [kOrdGroupsMax][kOrdKeysMax]
  unsigned order_epoch = 0;             // work orders of this scene so far (order_forecast_kernel, order_count_kernel, order_scatter_kernel)
  DevScene dev_uploaded;                // what d_dev holds
  int32_t shadow_bound_knob = 1;        // MT_TUNE_SHADOW_BOUND (DevScene::sb_knob)
  bool dev_uploaded_valid = false;
  Buf<double> d_frames;            // throughput engine: recursion frames
  Buf<int32_t> d_hit_prim;         // launch 1 -> launch 2 hand-off (per pixel)
  Buf<double> d_hit_t;
  Buf<unsigned int> d_class_list;  // [3][n_items]
  Buf<char> d_pool;                // latency engine: ray pool scratch of every wave (mt_pool.h)
  int engine = 0;                  // 0 = automatic, 1 = throughput (state machine), 2 = latency (ray pool)
  ForecastBank bank0;                   // every call's forecast state ...
  std::unique_ptr<ForecastBank> bank1;  // ... but the refinement launch's of an adaptive chunk (first use)
  void forget_histories() {  // other settings, other order: start from a first frame
    bank0.cost_signature = 0;
    if (bank1) bank1->cost_signature = 0;
    lean_fresh = true;
  }
  // The lean frame kernel (render_kernel<.., LEAN>): its device words (d_work + kLeanCtl) start afresh with the next
  // lean launch; what the last launch was (mt_scene_lean_info); the event between the lean and the redo launch.
  bool lean_fresh = true;
  bool last_lean = false;
  long long last_lean_slot = -1;  // ev_k row of the last lean launch
  bool use_history = true;
  Buf<uint8_t> d_rgb;
  Buf<uint8_t> d_samples;  // supersampled chunks: the sample frame on its way to resolve_kernel (mt_resolve.h)
  Buf<mt_debug_px> d_debug;
  // adaptive chunks (mt_adaptive.h), allocated on first use: the chunk's block flags, the refined blocks' list, count
  // and hash on the device and in pinned memory, the host call's mask, the events around the call's synchronisation
  Buf<uint8_t> d_ad_flags;
  Buf<int32_t> d_ad_list;
  Buf<RefineCtl> d_ad_ctl;
  Buf<RefineCtl, true> h_ad_ctl;
  Buf<uint8_t> d_ad_mask;
  hipEvent_t ev_ad[2] = {};
  std::vector<mt_light> lights_host;  // what d_lights holds
  int waves_per_block = 4;
  int deep = 0;                    // which DEEP instantiations of the kernels: 0, 1, 2 (mt_device.h, deep_layout)
  Buf<char> d_deep;                // their per-wave areas
  size_t lds_bytes = 0;
  int grid_blocks = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // per-launch kernel timing (mt_scene_kernel_times): [i][0] before the primary
  // kernel, [1] between the two kernels, [2] after the render kernel (a lean launch: after its redo launch; [3] between
  // the two)
  static constexpr int kTimedLaunches = 64;
  hipEvent_t ev_k[kTimedLaunches][4] = {};
  unsigned long long launches_timed = 0, launches_read = 0;
  int n_cu = 0;
  bool stats_enabled = true;
  Buf<unsigned long long, true> hb_host;  // MT_DEBUG_HEARTBEAT: pinned, device-visible
  Buf<unsigned long long> d_prof;         // -DMT_PROF build: phase cycle sums
  Buf<DevScene> d_dev;                    // device copy of `dev` (DevScene::self)
  Tuning tune;
  // multi-GPU frames with a moving camera: every rank's costs of the previous frame (mt_scene_import_costs_device)
  Buf<unsigned int> d_cost_map;
  int cost_map_w = 0, cost_map_h = 0;
  int tree_depth_levels = 0, n_tris_total = 0, n_nodes_total = 0;  // for MT_TUNE_PACKED_STACK
  // -DMT_DEBUG_KNOBS builds only (read from the environment once, in mt_scene_create)
  std::string dbg_item_cycles, dbg_timeline;
  int dbg_print_units = 0;
  // mt_render_frame_multi: this scene's tile buffer and stream, the frame + gathered tiles on the first scene's GPU
  Buf<uint8_t> d_multi_tiles;
  Buf<uint8_t> d_multi_gather;
  Buf<uint8_t> d_multi_frame;
  hipStream_t multi_stream = nullptr;
  hipEvent_t multi_done = nullptr;
  Buf<unsigned int> d_multi_map;    // this replica's block costs / the combined map on its way back
  Buf<unsigned int> d_multi_maps;   // first replica: all replicas' maps
  hipEvent_t multi_comb_done = nullptr;
  // mt_render_chunk (host buffers): page-locked staging for the frame on its way to the caller's buffer (copied in
  // pieces, each piece's host copy under the next piece's DMA), pinned words for the counters
  Buf<uint8_t, true> h_stage;
  static constexpr int kStagePieces = 16;
  hipEvent_t ev_stage[kStagePieces] = {};
  Buf<unsigned long long, true> h_counters;
  // mt_render_gbuffer (mt_gbuffer.h): stream index -> AddPrimitive index (mt_scene_desc::tri_id; kept OUTSIDE DevScene:
  // only gbuffer_kernel reads it; uploaded by the first call that wants the `prim` plane, like everything else here
  // allocated on first use: a scene that never makes a G-buffer has the allocations it had without the feature), the
  // kernel's work counter, the host call's planes and the events of its staged copies
  std::vector<int32_t> tri_id_host;
  Buf<int32_t> d_tri_id;
  bool have_tri_id = false;
  Buf<unsigned int> d_gb_work;
  Buf<double> d_gb_f64[5];
  Buf<int32_t> d_gb_i32[3];
  std::vector<hipEvent_t> ev_gb;
  // mt_render_lightbuffer / mt_shade_direct (mt_lightbuffer.h), allocated on first use: the host calls' light-buffer
  // planes, and the lights of a relight with more than kShadeArgLights of them
  Buf<double> d_lb_power;
  Buf<uint8_t> d_lb_shadow;
  Buf<mt_light> d_shade_lights;
  Buf<int32_t> d_update_idx;  // mt_update_lightbuffer: a list of more than kUpdateArgLights light indices
  int n_materials = 0;  // of dev.mtls (shade_direct_kernel checks the caller's material plane against it)
  // mt_scene_set_materials: what dev.mtls holds, how often it has changed since mt_scene_create, and the texture count
  // a material's `tex` is checked against
  std::vector<mt_material> mtls_host;
  unsigned long long mtl_generation = 0;
  int n_textures = 0;
  // mt_scene_set_texture: what dev.texs holds (the texels are device pointers: the scene keeps no host copy of them) and
  // how often each texture has been set since mt_scene_create; mt_scene_set_raytree_uvw's switch
  std::vector<DevTexture> texs_host;
  std::vector<unsigned long long> tex_generation;
  int raytree_uvw = 0;
  // mt_scene_set_triangle_materials: what dev.tri_mtl holds (shared with the ray trees' snapshots: a set replaces the
  // vector, it never writes into it) and how often it has changed since mt_scene_create; mt_scene_set_raytree_tri's switch
  std::shared_ptr<const std::vector<int32_t>> tri_mtl_host;
  unsigned long long asg_generation = 0;
  int raytree_tri = 0;
  // mt_scene_set_triangle_normals ([0]) / _uvw ([1]), allocated by the first set: the staging buffer and
  // tri_attr_stamp_kernel's two words, shared; per attribute the stamp plane, its host mirror (empty: every stamp is 0)
  // and the generation.  No host copy of the attributes themselves.
  Buf<double> d_attr_stage;
  Buf<unsigned int> d_attr_found;
  Buf<uint32_t> d_attr_stamp[2];
  std::vector<uint32_t> attr_stamp_host[2];
  uint32_t attr_generation[2] = {0, 0};
  // mt_scene_set_triangle_vertices, mt_scene_edit_triangles: how often the geometry has changed since mt_scene_create (a
  // ray tree of an older geometry is refused for good), and the wall times of the last move's or edit's parts
  // (mt_scene_move_times_last)
  unsigned long long geo_generation = 0;
  bool tri_id_checked = false;  // tri_id_host was found to be a permutation (the first set; a move keeps it one)
  double move_ms[MT_MOVE_TIMES] = {};
  // mt_order_tiles_device: summed block costs per tile
  Buf<unsigned long long> d_tile_cost;
  // mt_render_frame_multi, cost-balanced ownership: this replica's order and list; on the first replica every replica's list
  Buf<int32_t> d_multi_order;
  Buf<int32_t> d_multi_list;
  Buf<int32_t> d_multi_lists;
  unsigned long long multi_geom = 0;      // geometry (image, tiles, depth, replicas) the state below belongs to
  unsigned long long multi_list_id = 0;   // changes whenever the tiles are dealt out anew
  bool multi_have_map = false;            // d_multi_map holds the combined costs of the previous frame of multi_geom
  int multi_frames_at_rest = 0;
  int multi_rank = -1;
  mt_sensor multi_sensor{};
};

namespace {

// `kernel` over a flat range of n elements, one thread each in workgroups of 256; returns the launch's status
template <typename... Params, typename... Args>
hipError_t launch_flat(void (*kernel)(Params...), size_t n, hipStream_t stream, Args &&...args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, static_cast<Params>(args)...);
  return hipGetLastError();
}

// tiles of tile_w x tile_h over an image of image_w x image_h
long long tile_count(int image_w, int image_h, int tile_w, int tile_h) {
  return (long long)((image_w + tile_w - 1) / tile_w) * ((image_h + tile_h - 1) / tile_h);
}

// FNV-1a over a list of integers, never 0 (0 = no signature)
unsigned long long fnv1a(std::initializer_list<long long> key) {
  unsigned long long h = 1469598103934665603ull;
  for (long long v : key) h = (h ^ (unsigned long long)v) * 1099511628211ull;
  return h != 0 ? h : 1;
}

// 16-byte traversal stack frames when "first child" and "best triangle + 1" share one word: a quarter less LDS per
// wave.  The shift of the packed word, or 0 where the two do not fit in 32 bits.
int pack_shift_for(int n_tris, int n_nodes) {
  int tri_bits = 1;
  while (tri_bits < 31 && ((long long)n_tris + 1) > (1ll << tri_bits)) tri_bits++;
  int node_bits = 1;
  while (node_bits < 31 && (long long)n_nodes > (1ll << node_bits)) node_bits++;
  return tri_bits + node_bits <= 32 ? tri_bits : 0;
}

// The kernels of one deep layout D = 0, 1, 2 (mt_device.h, deep_layout); the frame kernels by [STATS]
using SceneKernel = void (*)(DevScene, RenderParams);
struct LayoutKernels {
  SceneKernel render[2], primary[2], pool[2], hybrid[2], probe;
  void (*intersect)(DevScene, int, const double *, int *, int *, double *, double *, unsigned long long *);
  void (*gbuffer[2])(DevScene, GBufferArgs);
  void (*lightbuffer[2])(DevScene, LightBufferArgs);
  void (*lightbuffer_update[2])(DevScene, LightUpdateArgs);
  void (*raytree_trace[2])(DevScene, RayTreeTraceArgs);
  void (*raytree_update[2])(DevScene, RayTreeUpdateArgs);
  SceneKernel lean[2];  // render_kernel<.., LEAN>
};
template <int D>
LayoutKernels layout_kernels() {
  return {{render_kernel<false, D>, render_kernel<true, D>}, {primary_kernel<false, D>, primary_kernel<true, D>},
          {pool_kernel<false, D>, pool_kernel<true, D>}, {hybrid_kernel<false, D>, hybrid_kernel<true, D>},
          probe_kernel<D>, intersect_kernel<D>, {gbuffer_kernel<false, D>, gbuffer_kernel<true, D>},
          {lightbuffer_kernel<false, D>, lightbuffer_kernel<true, D>},
          {lightbuffer_update_kernel<false, D>, lightbuffer_update_kernel<true, D>},
          {raytree_trace_kernel<false, D>, raytree_trace_kernel<true, D>},
          {raytree_update_kernel<false, D>, raytree_update_kernel<true, D>},
          {render_kernel<false, D, true>, render_kernel<true, D, true>}};
}
const LayoutKernels &kernels_of(int deep) {
  static const LayoutKernels k[3] = {layout_kernels<0>(), layout_kernels<1>(), layout_kernels<2>()};
  return k[deep];
}

// Launch geometry: workgroups of 4 waves -- or of 2 or 1 where that puts more waves on a CU: a deep octree's traversal
// frames (27 KB per wave at 16 levels) let one 4-wave workgroup fill two thirds of the LDS and leave room for a fifth
// wave only as a workgroup of its own.
int configure_launch(mt_scene *s) {
  s->deep = s->tune.v[MT_TUNE_DEEP_LAYOUT] != 0.0 ? deep_layout(s->dev.tree_depth) : 0;
  const size_t per_wave = wave_stack_bytes(s->dev.tree_depth, s->dev.pack_shift != 0, s->deep != 0);
  if (per_wave > kLdsBudget) {
    return fail(MT_ERR_UNSUPPORTED, "octree depth %d needs %zu B of LDS per wave (> %zu)",
                s->dev.tree_depth, per_wave, kLdsBudget);
  }
  // The attribute is per function AND per device: keep it, for every device, at the largest size any scene
  // of this process needs there (a shallower scene must not lower it; scenes may be created from several threads).
  auto set_attribute = [&](size_t bytes) -> int {
    static std::mutex mu;
    static std::map<int, size_t> lds_attr;  // device -> bytes set
    std::lock_guard<std::mutex> lock(mu);
    size_t &have = lds_attr[s->device];
    if (bytes > have) {
      constexpr hipFuncAttribute kLdsAttr = hipFuncAttributeMaxDynamicSharedMemorySize;
      for (int d = 0; d < 3; d++) {
        const LayoutKernels &k = kernels_of(d);
        for (const SceneKernel *f : {k.render, k.primary, k.pool, k.hybrid, k.lean}) {
          for (int st = 0; st < 2; st++) HIP_TRY(hipFuncSetAttribute((const void *)f[st], kLdsAttr, (int)bytes));
        }
        HIP_TRY(hipFuncSetAttribute((const void *)k.probe, kLdsAttr, (int)bytes));
        HIP_TRY(hipFuncSetAttribute((const void *)k.intersect, kLdsAttr, (int)bytes));
        for (int st = 0; st < 2; st++) HIP_TRY(hipFuncSetAttribute((const void *)k.gbuffer[st], kLdsAttr, (int)bytes));
        for (int st = 0; st < 2; st++) HIP_TRY(hipFuncSetAttribute((const void *)k.lightbuffer[st], kLdsAttr, (int)bytes));
        for (int st = 0; st < 2; st++) {
          HIP_TRY(hipFuncSetAttribute((const void *)k.lightbuffer_update[st], kLdsAttr, (int)bytes));
        }
      }
      have = bytes;
    }
    return MT_OK;
  };
  int best_wpb = 0, best_per_cu = 0;
  for (int wpb = 4; wpb >= 1; wpb >>= 1) {
    if (per_wave * wpb > kLdsBudget) continue;
    MT_TRY(set_attribute(per_wave * wpb));
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)kernels_of(s->deep).render[1], wpb * 64, per_wave * wpb));
    if (per_cu < 1) per_cu = 1;
    if (per_cu * wpb > 16) per_cu = 16 / wpb;  // more waves only add divergence state
    if (per_cu * wpb > best_per_cu * best_wpb) {  // (ties: the larger workgroup, tried first)
      best_wpb = wpb;
      best_per_cu = per_cu;
    }
  }
  int per_cu = best_per_cu;
  s->waves_per_block = best_wpb;
  s->lds_bytes = per_wave * best_wpb;
  {  // occupancy experiments
    const int v = (int)s->tune.v[MT_TUNE_BLOCKS_PER_CU];
    if (v >= 1 && v < per_cu) per_cu = v;
  }
  s->grid_blocks = s->n_cu * per_cu;
  return MT_OK;
}

// the per-wave global areas of the DEEP instantiations, for a launch of `waves` waves
int ensure_deep(mt_scene *s, size_t waves) {
  if (!s->deep) return MT_OK;
  const size_t stride = (wave_deep_bytes(s->dev.tree_depth) + 255) & ~(size_t)255;
  MT_TRY(s->d_deep.ensure(stride * waves));
  s->dev.deep_base = s->d_deep;
  s->dev.deep_stride = stride;
  return MT_OK;
}

// Did the frame of sensor `o` have pixels whose primary rays have a zero direction component?  Found on the host,
// exactly: per scanline and component the direction is r + dp x with r = start + ds y (the kernels' own expression,
// Sensor::GetRay), zero for at most the pixels next to -r / dp -- a whole column or row for a camera on an axis,
// isolated pixels for one with roll or pitch.  Those blocks' costs are skipped by a re-projected forecast
// (forecast_kernel).
int has_zero_component_pixel(const mt_sensor &o, int image_w, int image_h) {
  for (int k = 0; k < 3; k++) {
    for (int y = 0; y < image_h; y++) {
      const double r = o.start_point[k] + o.delta_scanline[k] * (double)y;
      if (o.delta_pixel[k] == 0.0 || !std::isfinite(r / o.delta_pixel[k])) {
        if (r + o.delta_pixel[k] * 0.0 == 0.0) return 1;
        continue;
      }
      const double x0 = std::nearbyint(-r / o.delta_pixel[k]);
      for (int dx = -1; dx <= 1; dx++) {
        const double x = x0 + dx;
        if (x >= 0.0 && x < (double)image_w && r + o.delta_pixel[k] * x == 0.0) return 1;
      }
    }
  }
  return 0;
}

// What a launch does, decided from its geometry and the scene's history (decide_launch, no HIP call)
struct LaunchPlan {
  unsigned long long sig = 0;  // the launch's geometry: costs measured by a launch with the same one are a history
  bool from_map = false;       // the history is the frame-wide cost map imported since the previous launch
  bool history = false;        // the work order comes from a history (else from probe_kernel / primary_kernel)
  int engine = 0;              // 1 state machine, 2 ray pool, 3 hybrid
  long long pool_cap = 0;      // ray pool: records per wave
  size_t pool_stride = 0;      // ... and bytes per wave
  int reproject = 0, radius = 0;  // forecast_kernel: the camera moved since the costs were measured
  float blend = 0.0f;
  int old_irr = 0, new_irr = 0;   // zero-component pixels in the frame that measured the costs / in this one
  bool lean = false;              // the frame kernel is render_kernel<.., LEAN>, with a redo launch of the full one behind it
};

int decide_launch(mt_scene *s, ForecastBank &B, const RenderParams &P, const mt_sensor *sensor, bool debug, const int32_t *d_list,
                  unsigned long long list_id, size_t waves, LaunchPlan &L) {
  const int image_w = P.image_w, image_h = P.image_h, max_depth = P.max_depth;
  // The block costs of the previous launch are a valid forecast when that
  // launch had the same geometry (an animation frame, main_local.cc:79-110, or a
  // repeated benchmark step) -- whichever engine measured them.  Then the blocks
  // are handed out longest first, the longest in pieces.  Otherwise: the ray
  // pool forecasts from 1/16 of the primary rays (probe_kernel); the state
  // machine classifies the blocks by material in a launch of its own
  // (primary_kernel).
  L.sig = fnv1a({image_w, image_h, P.region_x, P.region_y, P.region_w, P.region_h, P.tile_w, P.tile_h, P.first_tile,
                 P.tile_stride, P.n_tiles, max_depth, s->dev.n_lights, d_list ? 1 : 0, d_list ? (long long)list_id : 0});
  // (a tile list promises to be the previous launch's list by its non-zero list_id only)
  bool have_costs = s->use_history && B.cost_signature == L.sig && !(d_list != nullptr && list_id == 0);
  // A list launch with ANOTHER list (the tiles were dealt out anew): the slots' cost words belong to other tiles, but the
  // frame-wide map imported since the previous launch has every block's cost by image position.
  const bool map_ready = s->d_cost_map != nullptr && B.cost_map_for_launch == B.launches &&
                         s->cost_map_w >= (image_w + 7) / 8 && s->cost_map_h >= (image_h + 7) / 8;
  L.from_map = s->use_history && d_list != nullptr && !have_costs && map_ready && B.last_P_valid &&
               (P.tile_w & 7) == 0 && (P.tile_h & 7) == 0 && (P.region_x & 7) == 0 && (P.region_y & 7) == 0 &&
               B.last_P.image_w == image_w && B.last_P.image_h == image_h && B.last_P.max_depth == max_depth;
  if (L.from_map) have_costs = true;
  // ---- which engine?  Both compute every pixel with the same operations in the
  // same order (tests render through both).  The state machine (one lane per
  // pixel, its context in registers) has the lower cost per ray and is the
  // default; the ray pool has the shorter chain of dependent passes per pixel
  // and takes over when a launch is bound by its longest work unit rather than
  // by its amount of work, i.e. when there are few blocks per wave (a rank's
  // share of a multi-GPU frame, a small chunk).
  int engine = s->engine;
  const bool engine_auto = engine != 1 && engine != 2 && engine != 3;
  // Ray pool: records per wave.  64 * (2^(max_depth+1) - 1) is every call of every pixel's recursion tree at once;
  // beyond kPoolCapMax the kernel's throttle keeps the pool within the capacity (depth first).  A record grows with
  // the number of lights (160 + 80 n bytes), so the capacity shrinks with it -- down to the floor the throttle needs
  // -- to keep the scratch of all resident waves within MT_TUNE_POOL_SCRATCH_MB.
  const int n_l = s->dev.n_lights;
  constexpr int kPoolMaxLights = 254;  // a pool entry has 8 bits for (light + 1)
  bool pool_fits = n_l <= kPoolMaxLights, pool_roomy = pool_fits;
  if (pool_fits) {
    constexpr long long kPoolCapMax = 1024;
    const long long all = 64ll * ((2ll << max_depth) - 1);
    const long long floor_cap = 64 + 128 + 4ll * (max_depth + 1) + 64;
    long long pool_cap = all < kPoolCapMax ? all : kPoolCapMax;
    const size_t rec_bytes = (size_t)(kRecFixed + kLightSlot * n_l) * sizeof(double);
    const size_t per_rec = rec_bytes + (size_t)(n_l > 0 ? n_l : 1) * 4 + 4;
    const double budget = s->tune.v[MT_TUNE_POOL_SCRATCH_MB] * 1048576.0;
    const long long fit = (long long)(budget / ((double)per_rec * (double)(waves ? waves : 1)));
    if (pool_cap > fit) {  // automatic mode: such a launch goes to the state machine; engine 2 by request: a smaller pool
      pool_roomy = false;
      pool_cap = fit;
    }
    if ((long long)s->tune.v[MT_TUNE_POOL_CAP] > 0) pool_cap = (long long)s->tune.v[MT_TUNE_POOL_CAP];  // tests: force the depth-first throttle
    if (pool_cap > 65535) pool_cap = 65535;  // a pool entry holds the record number in 16 bits
    if (pool_cap < floor_cap) {
      pool_fits = (double)floor_cap * (double)per_rec * (double)(waves ? waves : 1) <= 4.0 * budget;
      pool_cap = floor_cap;
    }
    L.pool_cap = pool_cap;
    L.pool_stride = ((size_t)pool_cap * per_rec + 255) & ~(size_t)255;
  }
  if (engine_auto) {
    // blocks per wave below which a launch is taken to be tail-bound (one rank's share of the 4K frame
    // at N = 8 has 7.9 per wave: ray pool 4.4 ms, state machine 4.7; at N = 4, 15.8: 7.3 against 6.6)
    const float per_wave = (float)s->tune.v[MT_TUNE_POOL_BELOW];
    // ... and the first frame of a geometry: without measured costs the order
    // of the work is a guess, and the pool's short pixel chains forgive a bad
    // guess (12 ms against the state machine's 14.5 on the 1080p frame).
    // The state machine has no limit on lights or scratch: it takes what the pool cannot hold.
    // With measured costs such a launch goes to the HYBRID kernel (engine 3): only its longest blocks go through the
    // pool, in pieces; the rest keeps the state machine's cost per ray (one rank's share of the 4K frame at N = 8:
    // 3.63 ms against the pool's 3.88 and the state machine's 4.36; at N = 4 the state machine alone is ahead, 5.71
    // against 5.80).  It has no debug-buffer path: such launches stay with the pool.
    const bool small = (float)P.n_items < per_wave * (float)waves;
    engine = !(pool_fits && pool_roomy) ? 1 : (!have_costs ? 2 : (small ? (!debug ? 3 : 2) : 1));
  }
  // Engine 3 (hybrid: the longest blocks through the ray pool in pieces, the rest through the state machine, one
  // kernel) needs measured costs to tell the two kinds apart and has no debug-buffer path; a launch without either
  // is rendered by the ray pool (or the state machine where the pool does not fit).
  if (engine == 3 && !(have_costs && pool_fits && !debug)) engine = pool_fits ? 2 : 1;
  if (engine == 2 && !pool_fits) {
    return fail(MT_ERR_UNSUPPORTED, "the ray pool (engine 2) holds at most %d lights within its scratch budget; "
                "%d were set -- engine 0 (automatic) or 1 renders such scenes", kPoolMaxLights, n_l);
  }
  L.engine = engine;
  L.history = have_costs && (engine == 2 || !debug);  // (hybrid: both hold, see above)
  if (!L.history) return MT_OK;
  // (kept per sensor: a camera at rest is looked at once)
  if (!B.irr_sensor_valid || memcmp(&B.irr_sensor, sensor, sizeof(mt_sensor)) != 0 || B.irr_w != image_w || B.irr_h != image_h) {
    B.irr_sensor = *sensor; B.irr_w = image_w; B.irr_h = image_h;
    B.irr_sensor_has = has_zero_component_pixel(*sensor, image_w, image_h);
    B.irr_sensor_valid = true;
  }
  L.new_irr = B.irr_sensor_has;
  // Has the camera moved since the costs were measured?  Then forecast_kernel
  // re-projects them (radius 1 block; 2 when the origin moved too: parallax).
  if (memcmp(&B.cost_sensor, sensor, sizeof(mt_sensor)) != 0) {
    L.old_irr = has_zero_component_pixel(B.cost_sensor, image_w, image_h);
    L.reproject = 1;
    L.radius = memcmp(B.cost_sensor.origin, sensor->origin, sizeof sensor->origin) != 0 ? 2 : 1;
    if (s->tune.v[MT_TUNE_FORECAST_RADIUS] >= 0.0) L.radius = (int)s->tune.v[MT_TUNE_FORECAST_RADIUS];
  }
  if (!L.reproject && !L.from_map && B.forecasts_in_a_row > 0) {
    // swept (scripts/blend_sweep.py, state machine, 64 frames): 0 -> every other frame 6 % slower (mean 7.09 ms), 0.5 -> one
    // in three (7.03), 0.9 -> one in eight (7.01); a frozen forecast (1.0) repeats its frame time to 0.2 % (scripts/alternation.py)
    // (a running mean of the measurements first -- 1/2, 2/3, ... -- so that the first frames' costs, measured under a
    // guessed order, do not linger)
    const float cap = (float)s->tune.v[MT_TUNE_BLEND];
    L.blend = std::min(cap, (float)B.forecasts_in_a_row / (float)(B.forecasts_in_a_row + 1));
  }
  // ---- which frame kernel?  The lean one (the hit-set walk alone; units it cannot finish are redone by the full kernel
  // behind it) where nothing but the walk is expected to run: a state-machine launch with a cost history, traversal mode
  // 0, a scene within the walk's limits (trace_wave's own conditions), no debug facility -- and no pixel whose primary
  // ray has a zero direction component: those units are the frame's longest (a pixel column on the golden camera), and
  // started only behind the lean launch they would double the frame.  MT_TUNE_LEAN_KERNEL = 2 waives the last condition.
  const int lean_knob = (int)s->tune.v[MT_TUNE_LEAN_KERNEL];
  const int hs_depth = s->deep >= 2 ? kHsMaxDepthDeep : kHsMaxDepth;
  L.lean = lean_knob != 0 && L.engine == 1 && (s->engine == 0 || s->engine == 1) && &B == &s->bank0 &&
           s->dev.force_mode == 0 && s->dev.scene_regular != 0 && s->dev.tree_depth <= hs_depth &&
           s->dev.n_tris < (1 << 28) && s->dev.bmax[0] <= 0x1p200 && s->dev.bmax[1] <= 0x1p200 && s->dev.bmax[2] <= 0x1p200 &&
           !s->hb_host && s->dbg_item_cycles.empty() && s->dbg_print_units == 0 && s->dev.prof == nullptr &&
           (lean_knob == 2 || !L.new_irr);
  return MT_OK;
}

// The buffers a launch of plan L needs, and P's pointers to them
int size_buffers(mt_scene *s, ForecastBank &B, const LaunchPlan &L, const int32_t *d_list, size_t waves, RenderParams &P) {
  const size_t n = P.n_items;
  MT_TRY(B.d_item_cost.ensure(n * 4));
  MT_TRY(B.d_item_forecast.ensure(n * 4));
  MT_TRY(B.d_item_forms.ensure(n * 8));
  MT_TRY(B.d_order_item.ensure(n * 64));
  MT_TRY(B.d_order_sub.ensure(n * 16));
  MT_TRY(B.d_item_form.ensure(n));
  MT_TRY(B.d_item_unit.ensure(n * 4));
  P.item_cost = B.d_item_cost;
  P.item_forecast = B.d_item_forecast;
  P.item_whole = B.d_item_forms;
  P.item_qsum = B.d_item_forms + P.n_items;
  if (s->tune.v[MT_TUNE_FORMS] == 0.0) P.item_whole = P.item_qsum = nullptr;
  P.order_item = B.d_order_item;
  P.order_sub = B.d_order_sub;
  P.n_work = s->d_work + 7;
  if (L.lean) {
    MT_TRY(B.d_redo_item.ensure(n * 64));
    MT_TRY(B.d_redo_sub.ensure(n * 16));
    P.redo_item = B.d_redo_item;
    P.redo_sub = B.d_redo_sub;
    P.lean_ctl = s->d_work + kLeanCtl;
  }
  // the combined cost map of all ranks, if one was imported after the previous launch (else nullptr: own costs only)
  P.cost_map = B.cost_map_for_launch == B.launches ? s->d_cost_map.p : nullptr;
  P.cost_map_w = s->cost_map_w;
  P.cost_map_h = s->cost_map_h;
  if (L.from_map) P.item_whole = P.item_qsum = nullptr;  // (the two measured forms of a block are kept per slot)
  if (d_list != nullptr && P.n_tiles > 0) {
    MT_TRY(B.d_tile_list.ensure((size_t)P.n_tiles * 4));
    MT_TRY(B.d_tile_slot.ensure((size_t)tile_count(P.region_w, P.region_h, P.tile_w, P.tile_h) * 4));
    P.tile_list = B.d_tile_list;
    P.tile_slot = B.d_tile_slot;
  }
  if (L.engine == 2 || L.engine == 3) {
    MT_TRY(s->d_pool.ensure(L.pool_stride * waves));
    P.pool_scratch = s->d_pool;
    P.pool_stride = L.pool_stride;
    P.pool_cap = (int)L.pool_cap;
    P.prio_units = (unsigned)(s->n_cu * 4);  // one per SIMD
  }
  if (L.engine != 2) {
    const size_t slots_px = (size_t)P.n_tiles * (size_t)P.tile_w * (size_t)P.tile_h;
    MT_TRY(s->d_frames.ensure(waves * ((size_t)(P.max_depth > 0 ? P.max_depth : 1) * kFrameSlots + kParkSlots) * 64 * sizeof(double)));
    MT_TRY(s->d_hit_prim.ensure(slots_px * sizeof(int32_t)));
    MT_TRY(s->d_hit_t.ensure(slots_px * sizeof(double)));
    MT_TRY(s->d_class_list.ensure(3 * n * sizeof(unsigned int)));
    P.frames = s->d_frames;
    P.hit_prim = s->d_hit_prim;
    P.hit_t = s->d_hit_t;
    P.class_list = s->d_class_list;
    P.class_count = s->d_work + 4;  // d_work: [0..1] work counters, [4..6] class counts
  }
  if (n == 0) return MT_OK;  // (nothing is launched)
  P.order_ctl = s->d_order_ctl;
  P.order_whist = s->d_order_whist;
  P.item_unit = B.d_item_unit;
  // one work order per XCD: state-machine launches with a cost history only (the other engines keep the one order)
  // (measured and left out: first frames through the ray pool -- room 8.4 -> 8.9 ms, loft 19.7 -> 20.9: the probe's guess
  // balances the regions too roughly, and such a frame ends with its longest units either way --; the state machine's
  // part of hybrid launches, i.e. a rank's share of a frame -- mean of eight ranks' 4K shares 2.71 -> 2.77 ms)
  P.queues = (s->tune.v[MT_TUNE_XCD_QUEUES] != 0.0 && L.history && L.engine == 1) ? s->d_queues.p : nullptr;
  if (P.queues) {
    MT_TRY(B.d_item_cell.ensure(n * 2));
    P.item_cell = B.d_item_cell;
  }
  // (the probe's grid follows the number of blocks: 16 of them per wave)
  const size_t block = (size_t)s->waves_per_block * 64;
  const size_t probe_waves = (4 * n + block - 1) / block * s->waves_per_block;
  return ensure_deep(s, std::max(waves, probe_waves));
}

// the three kernels of the work order (mt_order.h) of kind KIND: 0 state machine, 1 hybrid, 2 ray pool
template <int KIND>
void launch_order(const RenderParams &P, const ForecastArgs &fa, const OrderArgs &oa, int groups, hipStream_t stream) {
  hipLaunchKernelGGL(order_forecast_kernel<KIND>, dim3(groups), dim3(kOrdThreads), 0, stream, P, fa, oa);
  hipLaunchKernelGGL(order_count_kernel<KIND>, dim3(groups), dim3(kOrdThreads), 0, stream, P, oa);
  hipLaunchKernelGGL(order_scatter_kernel<KIND>, dim3(groups), dim3(kOrdThreads), 0, stream, P, oa);
}

// The work order of a launch with a cost history, or of the ray pool's first frame (from probe_kernel's forecast)
void launch_work_order(mt_scene *s, ForecastBank &B, const LaunchPlan &L, const RenderParams &P, hipStream_t stream) {
  const double *tv = s->tune.v;
  const int last = B.last_engine;  // (the engine that measured the costs)
  const bool pool = L.engine == 2, hybrid = L.engine == 3;
  // blocks above this share of an even split are cut into quarters; a re-projected forecast (moving camera) is
  // cut more eagerly -- it is a neighbourhood maximum of stale costs (swept, scripts/quad_sweep.py: repeated frame
  // 0.6 / 0.8 / 1.0 -> 7.18 / 6.84 / 7.28 ms, moving camera 6.69 / 7.20 / 9.89; with work 1.5: share 0.7 -> 6.40)
  // (with the per-block ratio of the two forms' costs -- forecast_kernel -- the repeated frame no longer alternates,
  // and re-swept: 0.8 / 0.9 / 0.95 / 1.0 / 1.05 / 1.1 -> 6.67 / 6.49 / 6.47 / 6.46 / 6.56 / 6.93 ms)
  const float quad_share = (float)tv[L.reproject ? MT_TUNE_QUAD_SHARE_MOVING : MT_TUNE_QUAD_SHARE];  // 0.7 / 0.95
  // work of a block rendered as quarters / rendered whole (swept with the share): 1.5 / 1.7
  const float quad_work = (float)tv[L.reproject ? MT_TUNE_QUAD_WORK_MOVING : MT_TUNE_QUAD_WORK];
  // the ray pool: blocks above cut_share of an even split of the frame are handed out in pieces; a forecast is cut more
  // eagerly (own_costs: granularity in bits 30-31)
  SchedParams sp{L.history ? 1.0f : 0.3f, {1.0f, (float)tv[MT_TUNE_POOL_PIECE_TIME1], (float)tv[MT_TUNE_POOL_PIECE_TIME2]},
                 {1.0f, (float)tv[MT_TUNE_POOL_PIECE_WORK1], (float)tv[MT_TUNE_POOL_PIECE_WORK2]},
                 (float)tv[MT_TUNE_POOL_CELL_FACTOR], (!L.from_map && (!L.history || last == 2)) ? 1 : 0};
  if (tv[MT_TUNE_POOL_CUT_SHARE] >= 0.0) sp.cut_share = (float)tv[MT_TUNE_POOL_CUT_SHARE];
  // How forecast_kernel reads the measured costs -- per engine, side by side (the state machine and the hybrid kernel
  // always have a history):
  //   pool  the cost words carry the ray pool's granularity
  //   w1    cost of a block's quarters over the block's whole cost, w2 the same for its cells
  ForecastArgs fa{B.cost_sensor, L.reproject, L.radius,
                  pool ? ((L.history && (last == 1 || last == 3)) ? 0 : 1) : (last == 2 ? 1 : 0),
                  pool ? ((L.history && last == 1) ? 1.7f : sp.piece_work[1]) : (last == 2 ? 1.1f : quad_work),
                  pool ? sp.piece_work[2] : 3.0f,
                  16000u, L.blend, (L.history && last == 3) ? B.d_item_form.p : nullptr, (float)tv[MT_TUNE_HYBRID_WORK1],
                  (float)tv[MT_TUNE_HYBRID_WORK2], (float)tv[MT_TUNE_FORECAST_STEP], (float)tv[MT_TUNE_SM_CELL_WORK],
                  L.old_irr, L.new_irr};
  OrderArgs oa{};
  oa.n_waves = s->grid_blocks * s->waves_per_block;
  oa.epoch = s->order_epoch++;
  const int groups = std::max(1, std::min((int)tv[MT_TUNE_ORDER_GROUPS], kOrdGroupsMax));
  if (pool) {
    oa.sp = sp;
    launch_order<2>(P, fa, oa, groups, stream);
  } else if (hybrid) {
    const float k = L.reproject ? (float)(tv[MT_TUNE_QUAD_SHARE_MOVING] / tv[MT_TUNE_QUAD_SHARE]) : 1.0f;  // a re-projected forecast is cut more eagerly
    oa.quad_share = k * (float)tv[MT_TUNE_HYBRID_QUAD_SHARE];
    oa.pool_share = k * (float)tv[MT_TUNE_HYBRID_POOL_SHARE];
    oa.piece_time1 = (float)tv[MT_TUNE_POOL_PIECE_TIME1];
    oa.piece_time2 = (float)tv[MT_TUNE_POOL_PIECE_TIME2];
    oa.cell_factor = (float)tv[MT_TUNE_HYBRID_CELL_FACTOR];
    oa.form_out = B.d_item_form;
    oa.starter_share = (float)tv[MT_TUNE_HYBRID_STARTER_SHARE];
    oa.max_starters = (unsigned)std::min(s->grid_blocks, (int)(0.25 * s->grid_blocks * s->waves_per_block));
    launch_order<1>(P, fa, oa, groups, stream);
  } else {
    oa.quad_share = quad_share;
    // ... and stay so above this fraction of that threshold (1 = no hysteresis: swept, scripts/quad_sweep.py --
    // settings that steady the repeated frame cost the moving camera 50 %)
    oa.quad_keep = (float)tv[MT_TUNE_QUAD_KEEP];
    oa.cell_share = (float)tv[MT_TUNE_SM_CELL_SHARE];
    // (cells only on MEASURED costs: a re-projected forecast of such a block is a guess -- thirty times a mean block --
    // that cannot tell the loft's column, 1.4 frames long as quarters, from the room's, 0.87: room panning +0.5 % with
    // the guess trusted, loft -2 %)
    oa.new_irr = L.reproject ? 0 : L.new_irr;
    oa.cell_time = (float)tv[MT_TUNE_SM_CELL_TIME];
    oa.queue_mode = (int)tv[MT_TUNE_XCD_QUEUES];
    oa.lean = L.lean ? (s->lean_fresh ? 2 : 1) : 0;
    oa.lean_share = kLeanRedoShare;
    if (L.lean) s->lean_fresh = false;
    launch_order<0>(P, fa, oa, groups, stream);
  }
}

// Everything a launch puts on its stream.  Events: [0] -> [1] forecast / classification + work order; [1] -> [2] the
// frame kernel.
int launch_kernels(mt_scene *s, ForecastBank &B, const LaunchPlan &L, const RenderParams &P, const int32_t *d_list, hipStream_t stream) {
  if (P.tile_list) {
    const int tiles_total = (int)tile_count(P.region_w, P.region_h, P.tile_w, P.tile_h);
    HIP_TRY(hipMemcpyAsync(B.d_tile_list, d_list, (size_t)P.n_tiles * 4, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(launch_flat(tile_slot_kernel, (size_t)tiles_total, stream, B.d_tile_list.p, P.n_tiles, B.d_tile_slot.p, tiles_total, 0));
    HIP_TRY(launch_flat(tile_slot_kernel, (size_t)P.n_tiles, stream, B.d_tile_list.p, P.n_tiles, B.d_tile_slot.p, tiles_total, 1));
  }
  // (launches with a work order: order_forecast_kernel zeroes the counters on its way)
  if (!L.history && L.engine != 2) HIP_TRY(hipMemsetAsync(s->d_work, 0, 16 * sizeof(unsigned), stream));
  if (!s->dev_uploaded_valid || memcmp(&s->dev_uploaded, &s->dev, sizeof(DevScene)) != 0) {  // (nearly never: the scene description changes with the lights, the traversal mode, the layout)
    HIP_TRY(hipMemcpyAsync(s->d_dev, &s->dev, sizeof(DevScene), hipMemcpyHostToDevice, stream));
    memcpy(&s->dev_uploaded, &s->dev, sizeof(DevScene));
    s->dev_uploaded_valid = true;
  }
  hipEvent_t *ek = s->ev_k[s->launches_timed % mt_scene::kTimedLaunches];
  for (int i = 0; i < (L.lean ? 4 : 3); i++) {
    if (!ek[i]) HIP_TRY(hipEventCreate(&ek[i]));
  }
  HIP_TRY(hipEventRecord(ek[0], stream));
  // (the two measurements of a block belong to ONE camera, geometry and set of lights)
  if (B.forecasts_in_a_row == 0) HIP_TRY(hipMemsetAsync(B.d_item_forms, 0, (size_t)P.n_items * 8, stream));
  const dim3 grid(s->grid_blocks), block(s->waves_per_block * 64);
  const LayoutKernels &k = kernels_of(s->deep);
  const int stats = s->stats_enabled ? 1 : 0;
  if (L.engine == 2 && !L.history) {
    hipLaunchKernelGGL(k.probe, dim3((4 * P.n_items + block.x - 1) / block.x), block, s->lds_bytes, stream, s->dev, P);
    HIP_TRY(hipGetLastError());
  }
  if (L.engine == 2 || L.history) launch_work_order(s, B, L, P, stream);
  else hipLaunchKernelGGL(k.primary[stats], grid, block, s->lds_bytes, stream, s->dev, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ek[1], stream));
  const SceneKernel *frame = L.engine == 2 ? k.pool : (L.engine == 3 ? k.hybrid : (L.lean ? k.lean : k.render));
  hipLaunchKernelGGL(frame[stats], grid, block, s->lds_bytes, stream, s->dev, P);
  s->last_lean = L.lean;
  if (L.lean) {
    // The redo launch: the full kernel over the units the lean one abandoned -- one order for the chip, its count and
    // its unit counter among the lean words (zeroed by order_forecast_kernel).  Mostly empty: every wave fetches once.
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ek[3], stream));
    s->last_lean_slot = (long long)(s->launches_timed % mt_scene::kTimedLaunches);
    RenderParams R = P;
    R.order_item = P.redo_item;
    R.order_sub = P.redo_sub;
    R.n_work = P.lean_ctl + kLeanRedoCount;
    R.work_counter = P.lean_ctl;  // (the frame kernel counts through work_counter[1] = kLeanRedoCounter)
    R.queues = nullptr;
    R.from_primary = 0;
    hipLaunchKernelGGL(k.render[stats], grid, block, s->lds_bytes, stream, s->dev, R);
  }
  HIP_TRY(hipEventRecord(ek[2], stream));
  HIP_TRY(hipGetLastError());
  return MT_OK;
}

// -DMT_DEBUG_KNOBS facilities, after a launch: the work order's unit count, the per-item cycle dump (d_item), the
// heartbeat watchdog
int debug_after_launch(mt_scene *s, const RenderParams &P, const unsigned long long *d_item, hipStream_t stream) {
  if (s->dbg_print_units) {  // how many work units did the order have?
    if (s->dbg_print_units == 2) {  // without synchronising: kept in a ring, printed every 16th launch
      static unsigned *ring = nullptr;
      static unsigned long long n = 0;
      if (!ring) HIP_TRY(hipMalloc((void **)&ring, 16 * sizeof(unsigned)));
      HIP_TRY(hipMemcpyAsync(ring + (n % 16), s->d_work + 7, sizeof(unsigned), hipMemcpyDeviceToDevice, stream));
      if (++n % 16 == 0) {
        unsigned host[16];
        HIP_TRY(hipMemcpy(host, ring, sizeof host, hipMemcpyDeviceToHost));
        fprintf(stderr, "[mt units]");
        for (int i = 0; i < 16; i++) fprintf(stderr, " %u", host[i]);
        fprintf(stderr, "\n");
      }
    } else {  // (synchronises!)
      unsigned nw = 0;
      HIP_TRY(hipMemcpy(&nw, s->d_work + 7, sizeof nw, hipMemcpyDeviceToHost));
      fprintf(stderr, "[mt units] %u units for %u blocks\n", nw, P.n_items);
    }
  }
  if (d_item) {  // dump per-item durations (synchronises!)
    std::vector<unsigned long long> host((size_t)P.n_items * 16 * 2 * 4);
    HIP_TRY(hipMemcpy(host.data(), d_item, host.size() * 8, hipMemcpyDeviceToHost));
    if (FILE *f = fopen(s->dbg_item_cycles.c_str(), "wb")) {
      fwrite(host.data(), 8, host.size(), f);
      fclose(f);
    }
  }
  if (s->hb_host) {
    // Debug mode: watch the launch from the host and report where it is stuck.
    const auto t0 = std::chrono::steady_clock::now();
    while (hipStreamQuery(stream) == hipErrorNotReady) {
      const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (sec > 10.0) {
        fprintf(stderr, "[mt heartbeat] kernel still running after %.0f s\n", sec);
        int hist[8] = {0};
        const int nw = s->grid_blocks * s->waves_per_block;
        for (int w = 0; w < nw; w++) {
          const unsigned long long *h = s->hb_host + (size_t)w * 4;
          hist[h[0] & 7]++;
          if ((h[0] & 255) != 5 && (h[0] & 255) != 0) {
            fprintf(stderr, "  wave %d: stage %llu arg %llu exec@fetch %llx alive %llx exec %llx\n", w, h[0] & 255,
                    h[0] >> 8, h[1], h[2], h[3]);
          }
        }
        fprintf(stderr, "  stage histogram:");
        for (int i = 0; i < 8; i++) fprintf(stderr, " %d:%d", i, hist[i]);
        fprintf(stderr, "\n");
        fflush(stderr);
        _exit(86);
      }
    }
  }
  return MT_OK;
}

int launch_render(mt_scene *s, const mt_sensor *sensor, int image_w, int image_h, int rx, int ry,
                  int rw, int rh, int tile_w, int tile_h, int first_tile, int tile_stride,
                  int n_tiles, int max_depth, uint8_t *d_rgb, mt_debug_px *d_debug,
                  hipStream_t stream, const int32_t *d_list = nullptr, unsigned long long list_id = 0,
                  ForecastBank *bank = nullptr) {
  ForecastBank &B = bank ? *bank : s->bank0;
  if (max_depth < 0 || max_depth > MT_MAX_RECURSION) {
    return fail(MT_ERR_ARG, "max_depth %d outside [0, %d]", max_depth, MT_MAX_RECURSION);
  }
  RenderParams P{};
  P.sensor = *sensor;
  P.image_w = image_w;
  P.image_h = image_h;
  P.region_x = rx; P.region_y = ry; P.region_w = rw; P.region_h = rh;
  P.tile_w = tile_w; P.tile_h = tile_h;
  P.tiles_x = (rw + tile_w - 1) / tile_w;
  P.first_tile = first_tile; P.tile_stride = tile_stride; P.n_tiles = n_tiles;
  P.blocks_x = (tile_w + 7) / 8;
  P.blocks_y = (tile_h + 7) / 8;
  P.max_depth = max_depth;
  const unsigned long long items = (unsigned long long)n_tiles * P.blocks_x * P.blocks_y;
  if (items > 0xfffffff0ull) return fail(MT_ERR_ARG, "too many work items (%llu)", items);
  P.n_items = (unsigned)items;
  P.out_rgb = d_rgb;
  P.out_debug = d_debug;
  P.counters = s->d_counters;
  P.work_counter = s->d_work;
  const size_t waves = (size_t)s->grid_blocks * s->waves_per_block;
  LaunchPlan L;
  MT_TRY(decide_launch(s, B, P, sensor, d_debug != nullptr, d_list, list_id, waves, L));
  P.from_primary = L.history ? 0 : 1;
  P.from_map = L.from_map ? 1 : 0;
  MT_TRY(size_buffers(s, B, L, d_list, waves, P));
  if (P.n_items == 0) return MT_OK;
  Buf<unsigned long long> item_cycles;  // -DMT_DEBUG_KNOBS: MT_DEBUG_ITEM_CYCLES
  if (!s->dbg_item_cycles.empty()) {
    MT_TRY(item_cycles.ensure((size_t)P.n_items * 16 * 16 * 4));
    HIP_TRY(hipMemset(item_cycles, 0, (size_t)P.n_items * 16 * 16 * 4));
    P.item_cycles = item_cycles;
  }
  MT_TRY(launch_kernels(s, B, L, P, d_list, stream));
  // the scene's bookkeeping.  (A forecast made from the OTHER engine's costs -- the frame after a first frame -- does
  // not count: the next one starts the running mean with this engine's own measurement.)
  B.forecasts_in_a_row = (L.history && !L.reproject && !L.from_map && B.last_engine == L.engine) ? B.forecasts_in_a_row + 1 : 0;
  s->launches_timed++;
  B.launches++;
  B.last_history = L.history;
  B.last_P = P;
  B.last_P_valid = true;
  B.cost_signature = (d_list != nullptr && list_id == 0) ? 0 : L.sig;  // the costs now in d_item_cost belong to this geometry and engine
  B.last_engine = L.engine;
  B.cost_sensor = *sensor;
  return debug_after_launch(s, P, item_cycles, stream);
}

int check_status(const unsigned long long *c) {
  if (c[ST_STATUS] == DEV_OK) return MT_OK;
  return fail(MT_ERR_INTERNAL, "device loop bound tripped (code %llu): kernel logic error", c[ST_STATUS]);
}

void fill_stats(const unsigned long long *c, mt_stats *st) {
  st->rays_primary = c[ST_RAYS_PRIMARY];
  st->rays_secondary = c[ST_RAYS_SECONDARY];
  st->rays_shadow = c[ST_RAYS_SHADOW];
  st->box_tests = c[ST_BOX_TESTS];
  st->node_visits = c[ST_NODE_VISITS];
  st->tri_tests = c[ST_TRI_TESTS];
  st->mt_tests = c[ST_MT_TESTS];
  st->shaded_hits = c[ST_SHADED_HITS];
  st->wave_node_steps = c[ST_WAVE_NODE_STEPS];
  st->wave_tri_steps = c[ST_WAVE_TRI_STEPS];
  st->bytes_scalar = c[ST_BYTES_SCALAR];
  st->bytes_vector = c[ST_BYTES_VECTOR];
}

// The frame of a host entry point -- a call that comes back with its results, and its mt_stats, on the host: what such
// a call does around its launches.  From construction (after the argument checks) to destruction the scene counts when
// the caller asked for `stats`, whatever mt_scene_set_stats says; every way out of the call restores the switch.
// Between the two: begin -- the scene's work counters cleared, or left alone by a call that has none, and the first of
// the call's two events --, the launches, then the pieces of the way back in the caller's order: mark_end,
// counters_home, and close, which waits for the stream, checks the device status and fills `stats`.  Everything is
// queued on the null stream.  (mt_octree_build has no scene yet: a frame without one has no counters and no stats, only
// the two events and the wait.)
struct HostCall {
  mt_scene *const s;
  mt_stats *const stats;
  hipEvent_t &ev0, &ev1;  // (references: a tree's two events are created inside its first call)
  const std::chrono::steady_clock::time_point w0 = std::chrono::steady_clock::now();
  const bool counters_were;
  const hipStream_t stream = nullptr;
  bool begun = false;     // ev0 is on the stream: close waits, kernel_ms is ev0 .. ev1
  bool counters = false;  // the call has work counters: h_counters is checked and reported
  HostCall(mt_scene *scene, mt_stats *st, hipEvent_t &e0, hipEvent_t &e1)
      : s(scene), stats(st), ev0(e0), ev1(e1), counters_were(scene != nullptr && scene->stats_enabled) {
    if (stats && s) s->stats_enabled = true;  // the caller asked for them
  }
  ~HostCall() {
    if (s) s->stats_enabled = counters_were;
  }
  HostCall(const HostCall &) = delete;
  HostCall &operator=(const HostCall &) = delete;
  int clear_counters() {
    MT_TRY(s->h_counters.ensure(ST_COUNT * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(s->d_counters, 0, ST_COUNT * sizeof(unsigned long long), stream));
    counters = true;
    return MT_OK;
  }
  int begin(bool with_counters) {
    if (with_counters) MT_TRY(clear_counters());
    HIP_TRY(hipEventRecord(ev0, stream));
    begun = true;
    return MT_OK;
  }
  int mark_end() {
    HIP_TRY(hipEventRecord(ev1, stream));
    return MT_OK;
  }
  // the counters are queued for the pinned words and cleared behind the copy
  int counters_home() {
    HIP_TRY(hipMemcpyAsync(s->h_counters, s->d_counters, ST_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemsetAsync(s->d_counters, 0, ST_COUNT * sizeof(unsigned long long), stream));
    return MT_OK;
  }
  // `stats` from what has arrived: the counters in h_counters, kernel_ms between the two events, total_ms since w0
  int report() {
    if (!stats) return MT_OK;
    memset(stats, 0, sizeof *stats);
    if (counters) fill_stats(s->h_counters, stats);
    if (begun) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
      stats->kernel_ms = ms;
    }
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    return MT_OK;
  }
  int close() {
    if (begun) HIP_TRY(hipStreamSynchronize(stream));
    if (counters) MT_TRY(check_status(s->h_counters));
    return report();
  }
};

int check_image_args(const mt_scene *s, const mt_sensor *sensor, int image_w, int image_h) {
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  if (!sensor) return fail(MT_ERR_ARG, "sensor is NULL");
  if (image_w <= 0 || image_h <= 0 || image_w > 100000 || image_h > 100000) {
    return fail(MT_ERR_ARG, "image size %dx%d out of range", image_w, image_h);
  }
  return MT_OK;
}

// the arguments of a tiled launch: first_tile + k tile_stride, k < n_tiles
int check_tiling(const mt_scene *s, const mt_sensor *sensor, int image_w, int image_h, int tile_w, int tile_h,
                 int first_tile, int tile_stride, int n_tiles) {
  MT_TRY(check_image_args(s, sensor, image_w, image_h));
  if (tile_w <= 0 || tile_h <= 0 || first_tile < 0 || tile_stride <= 0 || n_tiles < 0) {
    return fail(MT_ERR_ARG, "bad tiling arguments");
  }
  return MT_OK;
}

// ... and are those tiles of the image?
int check_tile_selection(int image_w, int image_h, int tile_w, int tile_h, int first_tile, int tile_stride, int n_tiles) {
  const long long tiles_total = tile_count(image_w, image_h, tile_w, tile_h);
  if (n_tiles > 0 && (long long)first_tile + (long long)(n_tiles - 1) * tile_stride >= tiles_total) {
    return fail(MT_ERR_ARG, "tile selection exceeds the %lld tiles of the image", tiles_total);
  }
  return MT_OK;
}

// WorkChunk::DeserializeInput's constraints, mythtracer.cc:358-371
int check_chunk(int image_w, int image_h, int chunk_x, int chunk_y, int chunk_w, int chunk_h) {
  if (chunk_x < 0 || chunk_y < 0 || chunk_w <= 0 || chunk_h <= 0 ||
      (long long)chunk_x + chunk_w > image_w || (long long)chunk_y + chunk_h > image_h) {
    return fail(MT_ERR_ARG, "chunk %d,%d %dx%d outside image %dx%d", chunk_x, chunk_y, chunk_w,
                chunk_h, image_w, image_h);
  }
  return MT_OK;
}

// ---- supersampled frames (mt_resolve.h) ----
// The factor and the sample grid it makes of the OUTPUT image: checked before anything else, the scene included.
int check_ss(int ss, int image_w, int image_h) {
  if (ss < 1 || ss > 4) return fail(MT_ERR_ARG, "ss %d outside [1, 4]", ss);
  if (image_w <= 0 || image_h <= 0 || (long long)ss * image_w > 100000 || (long long)ss * image_h > 100000) {
    return fail(MT_ERR_ARG, "image size %dx%d with ss %d: sample grid %lldx%lld out of range", image_w, image_h, ss,
                (long long)ss * image_w, (long long)ss * image_h);
  }
  return MT_OK;
}

// The scene's sample buffer, grown on demand.  A frame that does not fit fails: never a lower factor instead.
int ensure_samples(mt_scene *s, size_t bytes) {
  if (s->d_samples.ensure(bytes) == MT_OK) return MT_OK;
  (void)hipGetLastError();
  return fail(MT_ERR_NOMEM, "no room for the %zu-byte sample buffer: %s", bytes, KeptError().text.c_str());
}

// resolve_kernel over n_tiles slots of the OUTPUT image's tile grid (a chunk: its one tile)
int launch_resolve(int ss, int image_w, int image_h, int tile_w, int tile_h, int first_tile, int tile_stride,
                   const int32_t *d_list, int n_tiles, const uint8_t *d_samples, uint8_t *d_out, hipStream_t stream) {
  ResolveArgs A{};
  A.image_w = image_w; A.image_h = image_h;
  A.tile_w = tile_w; A.tile_h = tile_h;
  A.tiles_x = (image_w + tile_w - 1) / tile_w;
  A.first_tile = first_tile; A.tile_stride = tile_stride; A.n_tiles = n_tiles;
  A.tile_list = d_list;
  A.rows = std::min(tile_h, image_h);
  A.units = std::min(tile_w, image_w) / 4 + 2;
  A.samples = d_samples;
  A.out = d_out;
  const unsigned long long total = (unsigned long long)n_tiles * A.rows * A.units;
  if (total > 0x7fffffffull) return fail(MT_ERR_ARG, "too many pixels to resolve in one launch (%llu units)", total);
  if (total == 0) return MT_OK;
  const dim3 grid((unsigned)std::min<unsigned long long>((total + 255) / 256, 4096)), block(256);
  switch (ss) {
    case 2: hipLaunchKernelGGL(resolve_kernel<2>, grid, block, 0, stream, A, (unsigned)total); break;
    case 3: hipLaunchKernelGGL(resolve_kernel<3>, grid, block, 0, stream, A, (unsigned)total); break;
    case 4: hipLaunchKernelGGL(resolve_kernel<4>, grid, block, 0, stream, A, (unsigned)total); break;
    default: return fail(MT_ERR_ARG, "ss %d has no resolve kernel", ss);
  }
  HIP_TRY(hipGetLastError());
  return MT_OK;
}

// The two halves of a chunk call with host output around its launches.  begin: the scene's buffers for npx pixels,
// cleared counters, the first event.
int begin_host_chunk(HostCall &call, size_t npx, bool debug) {
  mt_scene *s = call.s;
  MT_TRY(s->d_rgb.ensure(npx * 3));
  if (debug) MT_TRY(s->d_debug.ensure(npx * sizeof(mt_debug_px)));
  MT_TRY(s->h_stage.ensure(npx * 3));
  for (hipEvent_t &e : s->ev_stage) {
    if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  return call.begin(true);
}

// finish: the chunk in s->d_rgb (and s->d_debug) reaches the caller, with the counters and times of the launches.
// How the frame reaches the caller's (pageable) buffer, measured on the box (scripts/ubench/d2h_paths.hip, 6.2 MB of
// a 1080p frame / 24.9 MB of a 4K one): plain hipMemcpy 1.17 / 1.22 ms; a page-locked staging buffer + memcpy 0.42 /
// 1.72 (the memcpy alone 0.30 / 1.28); registering the caller's buffer per call 0.82 / 1.22 (the registration 0.7);
// a copy into memory that IS registered 0.12 / 0.45 -- but keeping a caller's buffer registered across calls is not
// safe (a vector freed and allocated again at the same address would receive its frame in the OLD pages).  So: the
// staging buffer, in pieces, every piece's memcpy under the next piece's DMA: about the memcpy's time.
int finish_host_chunk(HostCall &call, size_t npx, uint8_t *out_rgb, mt_debug_px *out_debug) {
  mt_scene *s = call.s;
  const hipStream_t stream = call.stream;
  const size_t out_bytes = npx * 3;
  MT_TRY(call.mark_end());
  // everything that comes back is queued behind the kernels: the counters (device status), the frame in pieces
  MT_TRY(call.counters_home());
  const int n_pieces = out_bytes < (1u << 20) ? 1 : (out_bytes < (8u << 20) ? 4 : mt_scene::kStagePieces);
  const size_t piece = ((out_bytes + n_pieces - 1) / n_pieces + 4095) & ~(size_t)4095;
  for (int k = 0; k < n_pieces; k++) {
    const size_t off = (size_t)k * piece;
    if (off < out_bytes) {
      HIP_TRY(hipMemcpyAsync(s->h_stage + off, s->d_rgb + off, std::min(piece, out_bytes - off), hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipEventRecord(s->ev_stage[k], stream));
  }
  if (out_debug) {
    HIP_TRY(hipMemcpyAsync(out_debug, s->d_debug, npx * sizeof(mt_debug_px), hipMemcpyDeviceToHost, stream));
  }
  for (int k = 0; k < n_pieces; k++) {
    const size_t off = (size_t)k * piece;
    HIP_TRY(hipEventSynchronize(s->ev_stage[k]));
    if (k == 0 && check_status(s->h_counters) != MT_OK) {  // (the counters came first: no frame of a failed launch)
      (void)hipStreamSynchronize(stream);
      return check_status(s->h_counters);
    }
    if (off < out_bytes) memcpy(out_rgb + off, s->h_stage + off, std::min(piece, out_bytes - off));
  }
  return call.close();
}

}  // namespace

extern "C" {

const char *mt_last_error(void) { return g_err; }
int mt_abi_version(void) { return MT_ABI_VERSION; }

int mt_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return fail(MT_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
  return n;
}

void mt_scene_destroy(mt_scene *s) {
  if (!s) return;
  (void)hipSetDevice(s->device);  // (the uploads and the buffers are freed with the scene)
  for (hipEvent_t e : s->ev_stage) {
    if (e) (void)hipEventDestroy(e);
  }
  for (hipEvent_t e : s->ev_gb) (void)hipEventDestroy(e);
  if (s->multi_comb_done) (void)hipEventDestroy(s->multi_comb_done);
  if (s->multi_stream) (void)hipStreamDestroy(s->multi_stream);
  if (s->multi_done) (void)hipEventDestroy(s->multi_done);
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  for (hipEvent_t e : s->ev_ad) {
    if (e) (void)hipEventDestroy(e);
  }
  for (auto &tri : s->ev_k) {
    for (hipEvent_t e : tri) {
      if (e) (void)hipEventDestroy(e);
    }
  }
  delete s;
}

// a texture's size and format (mt_scene_create, mt_scene_set_texture)
static int check_texture(const mt_texture &t, int i) {
  LayoutError err;
  return mt::check_texture(t, i, &err) ? MT_OK : fail(err);
}

// The arrays of a SceneLayout (mt_layout.h) in new allocations of `geo`, and what else of *dev the layout decides.  The
// one place that knows which arrays a layout has: scene creation and a move both come through here.
static int upload_derived(const SceneLayout &L, DeviceAllocs &geo, DevScene *dev) {
  MT_TRY(geo.upload(L.groups, "the block boxes", &dev->grp_aabb32));
  MT_TRY(geo.upload(L.supers, "the super boxes", &dev->sup_aabb32));
  MT_TRY(geo.upload(L.subs, "the subtree boxes", &dev->sub_aabb32));
  MT_TRY(geo.upload(L.hsr, "the walk's records", &dev->hs_rec));
  MT_TRY(geo.upload(L.ll_tri, "the long lists", &dev->ll_tri));
  MT_TRY(geo.upload(L.ll_exact, "the long lists", &dev->ll_exact));
  MT_TRY(geo.upload(L.ll_box_q, "the long lists' boxes", &dev->ll_box_q));
  MT_TRY(geo.upload(L.ll_grp_q, "the long lists' boxes", &dev->ll_grp_q));
  MT_TRY(geo.upload(L.ll_sup_q, "the long lists' boxes", &dev->ll_sup_q));
  MT_TRY(geo.upload(L.sl_box, "the short lists' boxes", &dev->sl_box32));
  MT_TRY(geo.upload(L.recs, "the node records", &dev->nodes));
  MT_TRY(geo.upload(L.tri_aabb, "the triangles' boxes", &dev->tri_aabb));
  MT_TRY(geo.upload(L.tri_aabb32, "the triangles' boxes", &dev->tri_aabb32));
  for (int k = 0; k < 3; k++) dev->bmax[k] = L.bmax[k];
  dev->tree_depth = L.max_depth;
  dev->scene_regular = L.regular ? 1 : 0;
  dev->sb = L.shadow;  // (sb_knob stays the scene's)
  return MT_OK;
}

// dev's per-triangle pointers are the scene's own `tri`
static void show_tri_arrays(const TriArrays &tri, DevScene *dev) {
  dev->tri_vertex = tri.vertex;
  dev->tri_normal = tri.normal;
  dev->tri_uvw = tri.uvw;
  dev->tri_mtl = tri.mtl;
  dev->tri_line = tri.line;
}

// The derived arrays (mt_layout.h) and the caller's own reach the device; the host keeps what the edit calls mirror.
static int upload_layout(mt_scene *s, const mt_scene_desc *d, const SceneLayout &L) {
  HIP_TRY(hipSetDevice(d->device));
  s->device = d->device;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, d->device));
  s->n_cu = prop.multiProcessorCount;

  MT_TRY(upload_derived(L, s->geo, &s->dev));
  const size_t nt = (size_t)d->n_tris;
  MT_TRY(s->geo.upload(d->tri_vertex, nt * 9, "the triangles' vertices", &s->tri.vertex));
  MT_TRY(s->geo.upload(d->tri_normal, nt * 9, "the triangles' normals", &s->tri.normal));
  MT_TRY(s->geo.upload(d->tri_uvw, nt * 9, "the triangles' uvw", &s->tri.uvw));
  MT_TRY(s->geo.upload(d->tri_material, nt, "the triangles' materials", &s->tri.mtl));
  s->tri_mtl_host = std::make_shared<const std::vector<int32_t>>(d->tri_material, d->tri_material + nt);
  MT_TRY(s->geo.upload(d->tri_line_no, nt, "the triangles' line numbers", &s->tri.line));
  show_tri_arrays(s->tri, &s->dev);
  if (d->tri_id != nullptr) {  // (mt_render_gbuffer's `prim` plane; not part of DevScene)
    s->tri_id_host.assign(d->tri_id, d->tri_id + nt);
    s->have_tri_id = true;
  }
  std::vector<DevTexture> texs((size_t)d->n_textures);
  for (int i = 0; i < d->n_textures; i++) {  // (first: texture i's texels are slot i of `tables`)
    const mt_texture &t = d->textures[i];
    const size_t texel_bytes = (t.format == MT_TEX_RGB8 ? 3 : 24);
    const uint8_t *dev_texels = nullptr;
    MT_TRY(s->tables.upload((const uint8_t *)t.texels, (size_t)t.width * t.height * texel_bytes,
                            ("texture " + std::to_string(i)).c_str(), &dev_texels));
    texs[i] = DevTexture{dev_texels, t.width, t.height, t.format, 0};
  }
  MT_TRY(s->tables.upload(d->materials, (size_t)d->n_materials, "the materials", &s->mtls));
  s->dev.mtls = s->mtls;
  s->n_materials = d->n_materials;
  s->n_textures = d->n_textures;
  if (d->n_materials > 0) s->mtls_host.assign(d->materials, d->materials + d->n_materials);
  MT_TRY(s->tables.upload(texs, "the texture table", &s->texs));
  s->dev.texs = s->texs;
  s->texs_host = texs;
  s->tex_generation.assign(texs.size(), 0ull);
  s->dev.n_tris = d->n_tris;
  s->dev.n_nodes = d->n_nodes;
  s->dev.force_mode = 0;
  s->dev.pack_shift = pack_shift_for(d->n_tris, d->n_nodes);  // (MT_TUNE_PACKED_STACK = 0 switches it off)
  s->dev.sb_knob = s->shadow_bound_knob;
  s->dev.n_lights = 0;
  s->dev.lights = nullptr;
  return MT_OK;
}

// What every launch of the scene needs besides the scene: counters, work words, queues, events, the device's DevScene.
static int init_launch_state(mt_scene *s) {
  MT_TRY(s->d_counters.ensure(ST_COUNT * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(s->d_counters, 0, ST_COUNT * sizeof(unsigned long long)));
  MT_TRY(s->d_work.ensure((kLeanCtl + 8) * sizeof(unsigned)));  // 16 words of counters, 8 of the lean frame kernel's
  HIP_TRY(hipMemset(s->d_work, 0, (kLeanCtl + 8) * sizeof(unsigned)));
  MT_TRY(s->d_queues.ensure(kQueueWords * sizeof(unsigned)));
  MT_TRY(s->d_order_ctl.ensure(kOrdWords * sizeof(unsigned)));
  HIP_TRY(hipMemset(s->d_order_ctl, 0, kOrdWords * sizeof(unsigned)));
  MT_TRY(s->d_order_whist.ensure((size_t)kOrdGroupsMax * kOrdKeysMax * sizeof(unsigned)));
  HIP_TRY(hipEventCreate(&s->ev0));
  HIP_TRY(hipEventCreate(&s->ev1));
  MT_TRY(mt_scene_set_lights(s, nullptr, 0));
  s->dev.hb = nullptr;
  s->dev.prof = nullptr;
  MT_TRY(s->d_dev.ensure(sizeof(DevScene)));
  s->dev.self = s->d_dev;
#ifdef MT_PROF
  // (behind the phase sums: a time line of one wave, -DMT_PROF builds only -- kProfTimeline stamps)
  MT_TRY(s->d_prof.ensure((PROF_COUNT + 1 + kProfTimeline) * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(s->d_prof, 0, (PROF_COUNT + 1 + kProfTimeline) * sizeof(unsigned long long)));
  s->dev.prof = s->d_prof;
#endif
#ifdef MT_DEBUG_KNOBS
  if (const char *e = getenv("MT_DEBUG_ITEM_CYCLES")) s->dbg_item_cycles = e;
  if (const char *e = getenv("MT_DEBUG_TIMELINE")) s->dbg_timeline = e;
  if (const char *e = getenv("MT_DEBUG_PRINT_UNITS")) s->dbg_print_units = atoi(e);
  const bool heartbeat = getenv("MT_DEBUG_HEARTBEAT") != nullptr;
#else
  const bool heartbeat = false;
#endif
  if (heartbeat) {
    MT_TRY(s->hb_host.ensure(65536 * sizeof(unsigned long long), hipHostMallocMapped));
    memset(s->hb_host, 0, 65536 * sizeof(unsigned long long));
    void *dp = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&dp, s->hb_host, 0));
    s->dev.hb = (volatile unsigned long long *)dp;
  }
  return configure_launch(s);
}

// A bad desc is refused before any HIP call (mt_layout.h: the checks and every derived array).
static int scene_create_impl(mt_scene *s, const mt_scene_desc *d) {
  std::vector<int> depth_of;
  int max_depth = 0;
  LayoutError err;
  if (!check_scene_desc(*d, &depth_of, &max_depth, &err)) return fail(err);
  SceneLayout L;
  derive_layout(*d, depth_of, &L);
  MT_TRY(upload_layout(s, d, L));
  return init_launch_state(s);
}

mt_scene *mt_scene_create(const mt_scene_desc *d) {
  if (!d) {
    fail(MT_ERR_ARG, "desc is NULL");
    return nullptr;
  }
  mt_scene *s = new mt_scene();
  s->engine = g_default_engine.load();
  if (scene_create_impl(s, d) != MT_OK) {
    mt_scene_destroy(s);
    return nullptr;
  }
  return s;
}

int mt_scene_set_lights(mt_scene *s, const mt_light *lights, int n) {
  if (!s || n < 0 || (n > 0 && !lights)) return fail(MT_ERR_ARG, "bad lights argument");
  HIP_TRY(hipSetDevice(s->device));
  MT_TRY(s->d_lights.ensure((size_t)(n > 8 ? n : 8) * sizeof(mt_light)));
  // The reference's drivers push the same lights again before every frame (main_local.cc:79-110): what the device
  // holds already is not uploaded again.  Other lights, other costs: the damped forecast starts over (the old costs
  // remain its first guess).
  if ((size_t)n != s->lights_host.size() || s->dev.lights != s->d_lights ||
      (n && memcmp(s->lights_host.data(), lights, (size_t)n * sizeof(mt_light)) != 0)) {
    if (n) HIP_TRY(hipMemcpy(s->d_lights, lights, (size_t)n * sizeof(mt_light), hipMemcpyHostToDevice));
    s->lights_host.assign(lights, lights + n);
    s->bank0.forecasts_in_a_row = 0;
    if (s->bank1) s->bank1->forecasts_in_a_row = 0;
  }
  s->dev.lights = s->d_lights;
  s->dev.n_lights = n;
  return MT_OK;
}

// checked before any device call, in the order of the header
static int check_materials_args(const mt_scene *s, const void *materials, int n) {
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  if (n != s->n_materials) return fail(MT_ERR_ARG, "%d materials for a scene made with %d", n, s->n_materials);
  if (n > 0 && !materials) return fail(MT_ERR_ARG, "the material array is NULL");
  return MT_OK;
}

int mt_scene_set_materials(mt_scene *s, const mt_material *materials, int n) {
  MT_TRY(check_materials_args(s, materials, n));
  for (int i = 0; i < n; i++) {
    const int t = materials[i].tex;
    if (t < -1 || t >= s->n_textures) {
      return fail(MT_ERR_ARG, "material %d: texture index %d outside -1..%d", i, t, s->n_textures - 1);
    }
  }
  if (n == 0 || memcmp(s->mtls_host.data(), materials, (size_t)n * sizeof(mt_material)) == 0) return MT_OK;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipDeviceSynchronize());  // no kernel of an earlier call reads the table while it changes
  HIP_TRY(hipMemcpy(s->mtls, materials, (size_t)n * sizeof(mt_material), hipMemcpyHostToDevice));
  s->mtls_host.assign(materials, materials + n);
  s->mtl_generation++;
  return MT_OK;
}

int mt_scene_get_materials(const mt_scene *s, mt_material *out, int n) {
  MT_TRY(check_materials_args(s, out, n));
  if (n > 0) memcpy(out, s->mtls_host.data(), (size_t)n * sizeof(mt_material));
  return MT_OK;
}

// checked before any device call, in the order of the header
static int check_texture_index(const mt_scene *s, int index) {
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  if (index < 0 || index >= s->n_textures) {
    return fail(MT_ERR_ARG, "texture index %d outside 0..%d", index, s->n_textures - 1);
  }
  return MT_OK;
}

int mt_scene_set_texture(mt_scene *s, int index, const mt_texture *tex) {
  MT_TRY(check_texture_index(s, index));
  if (!tex) return fail(MT_ERR_ARG, "the mt_texture is NULL");
  MT_TRY(check_texture(*tex, index));
  HIP_TRY(hipSetDevice(s->device));
  const size_t bytes = (size_t)tex->width * (size_t)tex->height * (tex->format == MT_TEX_RGB8 ? 3 : 24);
  // the new texels next to the old ones, in a list of their own: until the entry is patched the scene is what it was
  DeviceAllocs aside;
  uint8_t *fresh = nullptr;
  MT_TRY(aside.alloc<uint8_t>(bytes, ("texture " + std::to_string(index)).c_str(), &fresh));
  const DevTexture entry{fresh, tex->width, tex->height, tex->format, 0};
  // (hipDeviceSynchronize: no kernel of an earlier call reads the entry or the old texels while they change)
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(fresh, tex->texels, bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(s->texs + index, &entry, sizeof entry, hipMemcpyHostToDevice) != hipSuccess) {
    return fail(MT_ERR_HIP, "uploading texture %d failed: %s", index, hipGetErrorString(hipGetLastError()));
  }
  s->tables.swap_slot((size_t)index, aside, 0);  // (the old texels are freed with `aside`)
  s->texs_host[(size_t)index] = entry;
  s->tex_generation[(size_t)index]++;
  s->mtl_generation++;  // every ray tree of the scene is stale, as after a material edit
  return MT_OK;
}

int mt_scene_get_texture_info(const mt_scene *s, int index, mt_texture *out) {
  MT_TRY(check_texture_index(s, index));
  if (!out) return fail(MT_ERR_ARG, "the mt_texture is NULL");
  const DevTexture &t = s->texs_host[(size_t)index];
  out->width = t.width;
  out->height = t.height;
  out->format = t.format;
  out->texels = nullptr;  // (no host copy is kept)
  return MT_OK;
}

int mt_scene_set_raytree_uvw(mt_scene *s, int keep) {
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  if (keep != 0 && keep != 1) return fail(MT_ERR_ARG, "keep must be 0 or 1");
  s->raytree_uvw = keep;
  return MT_OK;
}

// checked before any device call, in the order of the header
static int check_triangle_materials_args(const mt_scene *s, const void *tri_material, int n) {
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  if (n != s->dev.n_tris) return fail(MT_ERR_ARG, "%d triangles for a scene made with %d", n, s->dev.n_tris);
  if (n > 0 && !tri_material) return fail(MT_ERR_ARG, "the triangle material array is NULL");
  return MT_OK;
}

int mt_scene_set_triangle_materials(mt_scene *s, const int32_t *tri_material, int n) {
  MT_TRY(check_triangle_materials_args(s, tri_material, n));
  for (int i = 0; i < n; i++) {
    const int m = tri_material[i];
    if (m < -1 || m >= s->n_materials) {
      return fail(MT_ERR_ARG, "triangle %d: material index %d outside -1..%d", i, m, s->n_materials - 1);
    }
  }
  if (n == 0 || memcmp(s->tri_mtl_host->data(), tri_material, (size_t)n * sizeof(int32_t)) == 0) return MT_OK;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipDeviceSynchronize());  // no kernel of an earlier call reads the array while it changes
  HIP_TRY(hipMemcpy(s->tri.mtl, tri_material, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
  s->tri_mtl_host = std::make_shared<const std::vector<int32_t>>(tri_material, tri_material + n);
  s->asg_generation++;
  s->mtl_generation++;  // every ray tree of the scene is stale, as after a material edit
  return MT_OK;
}

int mt_scene_get_triangle_materials(const mt_scene *s, int32_t *out, int n) {
  MT_TRY(check_triangle_materials_args(s, out, n));
  if (n > 0) memcpy(out, s->tri_mtl_host->data(), (size_t)n * sizeof(int32_t));
  return MT_OK;
}

namespace {

const char *const kAttrName[2] = {"normal", "uvw"};

// checked before any device call, in the order of the header
int check_triangle_attr_args(const mt_scene *s, const void *attr, int n, int which) {
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  if (n != s->dev.n_tris) return fail(MT_ERR_ARG, "%d triangles for a scene made with %d", n, s->dev.n_tris);
  if (n > 0 && !attr) return fail(MT_ERR_ARG, "the triangle %s array is NULL", kAttrName[which]);
  return MT_OK;
}

// the status of a Buf::ensure for an attribute set: what does not fit is MT_ERR_NOMEM (nothing of the scene has changed
// by then)
int attr_nomem(int rc, size_t bytes, const char *what) {
  if (rc == MT_OK) return MT_OK;
  (void)hipGetLastError();
  return fail(MT_ERR_NOMEM, "no room for the %zu bytes of %s: %s", bytes, what, KeptError().text.c_str());
}

// mt_scene_set_triangle_normals (which = 0) / _uvw (1): the array staged on the device, tri_attr_stamp_kernel, and --
// only when a triangle changed -- the stamp plane's way home and the generations
int set_triangle_attr(mt_scene *s, const double *attr, int n, int which) {
  MT_TRY(check_triangle_attr_args(s, attr, n, which));
  if (n == 0) return MT_OK;
  if (s->attr_generation[which] == 0xffffffffu) {  // (the stamps are 32 bits wide)
    return fail(MT_ERR_UNSUPPORTED, "the scene's %s generation is used up (2^32 - 1 sets that changed a triangle): a new "
                                    "scene is needed", kAttrName[which]);
  }
  const size_t nt = (size_t)n;
  HostCall call(s, nullptr, s->ev0, s->ev1);
  HIP_TRY(hipSetDevice(s->device));
  // everything that may not fit comes first: until the kernel runs the scene is exactly what it was
  MT_TRY(attr_nomem(s->d_attr_stage.ensure(nt * 72), nt * 72, "the staged triangle attributes"));
  MT_TRY(attr_nomem(s->d_attr_found.ensure(2 * sizeof(unsigned int)), 2 * sizeof(unsigned int), "the attribute set's count"));
  const bool first_set = s->d_attr_stamp[which].p == nullptr;
  MT_TRY(attr_nomem(s->d_attr_stamp[which].ensure(nt * sizeof(uint32_t)), nt * sizeof(uint32_t), "the triangles' stamp plane"));
  if (first_set) HIP_TRY(hipMemset(s->d_attr_stamp[which], 0, nt * sizeof(uint32_t)));  // (generation 0: creation)
  try {
    s->attr_stamp_host[which].resize(nt, 0u);
  } catch (const std::bad_alloc &) {
    return fail(MT_ERR_NOMEM, "no room for the %zu bytes of the stamp plane's host mirror", nt * sizeof(uint32_t));
  }
  HIP_TRY(hipDeviceSynchronize());  // no kernel of an earlier call reads the array while it changes
  const hipStream_t stream = call.stream;
  HIP_TRY(hipMemcpyAsync(s->d_attr_stage, attr, nt * 72, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetAsync(s->d_attr_found, 0, sizeof(unsigned int), stream));
  HIP_TRY(hipMemsetAsync(s->d_attr_found + 1, 0xff, sizeof(unsigned int), stream));
  MT_TRY(call.begin(false));
  TriAttrStampArgs A{};
  A.staged = s->d_attr_stage;
  A.live = which == 0 ? s->tri.normal : s->tri.uvw;
  A.stamp = s->d_attr_stamp[which];
  A.n_tris = (uint32_t)n;
  A.generation = s->attr_generation[which] + 1u;
  A.found = s->d_attr_found;
  HIP_TRY(launch_flat(tri_attr_stamp_kernel, nt, stream, A));
  MT_TRY(call.mark_end());
  unsigned int found[2] = {0u, 0u};
  HIP_TRY(hipMemcpyAsync(found, s->d_attr_found, sizeof found, hipMemcpyDeviceToHost, stream));
  MT_TRY(call.close());  // (waits for the stream)
  if (found[0] == 0) return MT_OK;
  HIP_TRY(hipMemcpy(s->attr_stamp_host[which].data(), s->d_attr_stamp[which], nt * sizeof(uint32_t), hipMemcpyDeviceToHost));
  s->attr_generation[which]++;
  s->mtl_generation++;  // every ray tree of the scene is stale, as after a material edit
  return MT_OK;
}

int get_triangle_attr(mt_scene *s, double *out, int n, int which) {
  MT_TRY(check_triangle_attr_args(s, out, n, which));
  if (n == 0) return MT_OK;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipMemcpy(out, which == 0 ? s->dev.tri_normal : s->dev.tri_uvw, (size_t)n * 72, hipMemcpyDeviceToHost));
  return MT_OK;
}

}  // namespace

int mt_scene_set_triangle_normals(mt_scene *s, const double *tri_normal, int n) { return set_triangle_attr(s, tri_normal, n, 0); }
int mt_scene_set_triangle_uvw(mt_scene *s, const double *tri_uvw, int n) { return set_triangle_attr(s, tri_uvw, n, 1); }
int mt_scene_get_triangle_normals(mt_scene *s, double *out, int n) { return get_triangle_attr(s, out, n, 0); }
int mt_scene_get_triangle_uvw(mt_scene *s, double *out, int n) { return get_triangle_attr(s, out, n, 1); }

int mt_scene_set_raytree_tri(mt_scene *s, int keep) {
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  if (keep != 0 && keep != 1) return fail(MT_ERR_ARG, "keep must be 0 or 1");
  s->raytree_tri = keep;
  return MT_OK;
}

int mt_scene_set_traversal_mode(mt_scene *s, int mode) {
  if (!s || mode < 0 || mode > 7) return fail(MT_ERR_ARG, "mode must be 0..7");
  s->dev.force_mode = mode;
  return MT_OK;
}

int mt_scene_set_scheduling(mt_scene *s, int use_cost_history) {
  if (!s || (use_cost_history != 0 && use_cost_history != 1)) return fail(MT_ERR_ARG, "bad scheduling argument");
  s->use_history = use_cost_history != 0;
  s->forget_histories();
  return MT_OK;
}

int mt_scene_set_stats(mt_scene *s, int enabled) {
  if (!s || (enabled != 0 && enabled != 1)) return fail(MT_ERR_ARG, "bad stats argument");
  s->stats_enabled = enabled != 0;
  return MT_OK;
}

int mt_scene_set_engine(mt_scene *s, int engine) {
  if (!s || engine < 0 || engine > 3) return fail(MT_ERR_ARG, "engine must be 0 (automatic), 1, 2 or 3");
  s->engine = engine;
  s->forget_histories();
  return MT_OK;
}

int mt_set_default_engine(int engine) {
  if (engine < 0 || engine > 3) return fail(MT_ERR_ARG, "engine must be 0 (automatic), 1, 2 or 3");
  g_default_engine.store(engine);
  return MT_OK;
}

int mt_scene_set_tuning(mt_scene *s, int knob, double value) {
  if (s && knob == MT_TUNE_SHADOW_BOUND) {  // (not one of the launch constants in tune.v: a word of the scene description)
    if (!(value == 0.0 || value == 1.0 || value == 2.0)) return fail(MT_ERR_ARG, "shadow bound: 0 (never), 1 (launches without work counters) or 2 (always)");
    s->shadow_bound_knob = s->dev.sb_knob = (int32_t)value;
    s->forget_histories();  // other block costs: start from a first frame
    return MT_OK;
  }
  if (!s || knob < 0 || knob >= MT_TUNE_COUNT || !std::isfinite(value)) return fail(MT_ERR_ARG, "bad tuning argument");
  // The kernels divide by the work factors and scale an even share by the shares: those must be positive (and small
  // enough for their products to stay finite in float); counts and budgets must not be negative or beyond what the
  // conversions to integers hold.
  switch (knob) {
    case MT_TUNE_POOL_PIECE_TIME1: case MT_TUNE_POOL_PIECE_TIME2: case MT_TUNE_POOL_PIECE_WORK1: case MT_TUNE_POOL_PIECE_WORK2:
    case MT_TUNE_POOL_CELL_FACTOR: case MT_TUNE_QUAD_SHARE: case MT_TUNE_QUAD_SHARE_MOVING: case MT_TUNE_QUAD_KEEP:
    case MT_TUNE_QUAD_WORK: case MT_TUNE_QUAD_WORK_MOVING: case MT_TUNE_HYBRID_POOL_SHARE: case MT_TUNE_HYBRID_QUAD_SHARE:
    case MT_TUNE_SM_CELL_SHARE: case MT_TUNE_SM_CELL_TIME: case MT_TUNE_SM_CELL_WORK: case MT_TUNE_HYBRID_CELL_FACTOR:
    case MT_TUNE_HYBRID_WORK1: case MT_TUNE_HYBRID_WORK2: case MT_TUNE_FORECAST_STEP: case MT_TUNE_HYBRID_STARTER_SHARE:
      if (!(value >= 1e-6 && value <= 1e6)) return fail(MT_ERR_ARG, "tuning knob %d must lie in [1e-6, 1e6]", knob);
      break;
    case MT_TUNE_POOL_BELOW: case MT_TUNE_POOL_CAP: case MT_TUNE_BLOCKS_PER_CU:
      if (!(value >= 0.0 && value <= 1e9)) return fail(MT_ERR_ARG, "tuning knob %d must lie in [0, 1e9]", knob);
      break;
    case MT_TUNE_POOL_SCRATCH_MB:
      if (!(value >= 1.0 && value <= 1e9)) return fail(MT_ERR_ARG, "the ray pool's scratch budget must lie in [1, 1e9] MB");
      break;
    case MT_TUNE_BLEND:
      if (!(value >= 0.0 && value <= 1.0)) return fail(MT_ERR_ARG, "the forecast's damping must lie in [0, 1]");
      break;
    case MT_TUNE_FORECAST_RADIUS:
      if (!(value <= 8.0)) return fail(MT_ERR_ARG, "the forecast's radius must be at most 8 blocks (< 0 = automatic)");
      break;
    case MT_TUNE_POOL_CUT_SHARE:
      if (!(value < 0.0 || (value >= 1e-6 && value <= 1e6))) return fail(MT_ERR_ARG, "the pool's cutting share must be negative (automatic) or lie in [1e-6, 1e6]");
      break;
    case MT_TUNE_ORDER_GROUPS:
      if (!(value >= 1.0 && value <= (double)kOrdGroupsMax)) return fail(MT_ERR_ARG, "the work-order kernel runs on 1 .. %d workgroups", kOrdGroupsMax);
      break;
    case MT_TUNE_XCD_QUEUES:
      if (!(value == 0.0 || value == 1.0 || value == 2.0)) return fail(MT_ERR_ARG, "XCD queues: 0 (off), 1 (stripes) or 2 (grid)");
      break;
    case MT_TUNE_LEAN_KERNEL:
      if (!(value == 0.0 || value == 1.0 || value == 2.0)) return fail(MT_ERR_ARG, "lean frame kernel: 0 (never), 1 (automatic) or 2 (forced)");
      break;
    default: break;  // switches: any finite value (0 / non-zero)
  }
  s->tune.v[knob] = value;
  s->forget_histories();  // other constants, other order: start from a first frame
  if (knob == MT_TUNE_PACKED_STACK || knob == MT_TUNE_BLOCKS_PER_CU || knob == MT_TUNE_DEEP_LAYOUT) {
    if (knob == MT_TUNE_PACKED_STACK) s->dev.pack_shift = value != 0.0 ? pack_shift_for(s->dev.n_tris, s->dev.n_nodes) : 0;
    HIP_TRY(hipSetDevice(s->device));
    return configure_launch(s);
  }
  return MT_OK;
}

int mt_scene_export_costs_device(mt_scene *s, void *d_map, int map_w, int map_h, void *stream) {
  if (!s || !d_map || map_w <= 0 || map_h <= 0) return fail(MT_ERR_ARG, "bad cost map arguments");
  if (!s->bank0.last_P_valid) return fail(MT_ERR_ARG, "no launch to export the costs of");
  const RenderParams &P = s->bank0.last_P;
  if (map_w < (P.image_w + 7) / 8 || map_h < (P.image_h + 7) / 8 || (P.tile_w & 7) || (P.tile_h & 7) || (P.region_x & 7) || (P.region_y & 7)) {
    return fail(MT_ERR_ARG, "cost map smaller than the image's 8x8 blocks, or tiles not on the 8-pixel grid");
  }
  HIP_TRY(hipSetDevice(s->device));
  if (P.n_items == 0) return MT_OK;
  const double *tv = s->tune.v;
  const bool hy = s->bank0.last_engine == 3;
  HIP_TRY(launch_flat(export_costs_kernel, (size_t)P.n_items, (hipStream_t)stream, P, s->bank0.last_engine,
                      (float)(hy ? tv[MT_TUNE_HYBRID_WORK1] : tv[MT_TUNE_POOL_PIECE_WORK1]),
                      (float)(hy ? tv[MT_TUNE_HYBRID_WORK2] : tv[MT_TUNE_POOL_PIECE_WORK2]), (float)tv[MT_TUNE_SM_CELL_WORK],
                      (const unsigned char *)s->bank0.d_item_form, (unsigned *)d_map, map_w, map_h));
  return MT_OK;
}

int mt_scene_import_costs_device(mt_scene *s, const void *d_map, int map_w, int map_h, void *stream) {
  if (!s || !d_map || map_w <= 0 || map_h <= 0) return fail(MT_ERR_ARG, "bad cost map arguments");
  HIP_TRY(hipSetDevice(s->device));
  const size_t bytes = (size_t)map_w * (size_t)map_h * sizeof(unsigned);
  MT_TRY(s->d_cost_map.ensure(bytes));
  HIP_TRY(hipMemcpyAsync(s->d_cost_map, d_map, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  s->cost_map_w = map_w;
  s->cost_map_h = map_h;
  s->bank0.cost_map_for_launch = s->bank0.launches;  // valid for the NEXT launch only
  return MT_OK;
}

int mt_scene_read_stats(mt_scene *s, mt_stats *st) {
  if (!s || !st) return fail(MT_ERR_ARG, "NULL argument");
  HIP_TRY(hipSetDevice(s->device));
  unsigned long long c[ST_COUNT];
  HIP_TRY(hipMemcpy(c, s->d_counters, sizeof c, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(s->d_counters, 0, sizeof c));
  memset(st, 0, sizeof *st);
  fill_stats(c, st);
#ifdef MT_PROF
  {
    unsigned long long pr[PROF_COUNT];
    HIP_TRY(hipMemcpy(pr, s->d_prof, sizeof pr, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(s->d_prof, 0, sizeof pr));
    if (const char *tl = s->dbg_timeline.empty() ? nullptr : s->dbg_timeline.c_str()) {  // dump and reset the time line
      std::vector<unsigned long long> host(1 + kProfTimeline);
      HIP_TRY(hipMemcpy(host.data(), s->d_prof + PROF_COUNT, host.size() * 8, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemset(s->d_prof + PROF_COUNT, 0, host.size() * 8));
      if (FILE *f = fopen(tl, "wb")) {
        fwrite(host.data(), 8, host.size(), f);
        fclose(f);
      }
    }
    static const char *names[PROF_COUNT] = {"trace_cycles", "scan_raypar_cycles", "scan_transposed_cycles",
                                            "children_unwind_cycles", "n_raypar_scans", "n_transposed_scans",
                                            "n_transposed_chunks", "n_raypar_tris", "n_traces", "lane_phase_cycles",
                                            "scan_m2f", "scan_m2", "scan_m1", "scan_m0", "n_m2f", "n_m2", "n_m1", "n_m0",
                                            "tris_m2f", "tris_m1", "tris_transposed", "g_groups", "g_live", "g_ranges", "g_range_tris", "nin_sum", "nin_lt8", "nin_lt24", "want_sum",
                                            "grp_mask_t", "grp_ranges_t", "tr_blocks_t", "tr_tris_t", "tr_bcast_t", "tr_rays", "m2f_call_t",
                                            "hs_rec_t", "hs_big_t", "hs_small_t", "hs_trans_t", "hs_kids_t", "hs_ret_t", "hs_close_t", "hs_n_enter", "hs_n_big", "hs_n_small", "hs_n_empty", "hs_n_trans", "hs_n_ret", "hs_n_rethit", "hs_lanes", "hs_big_tris", "hs_small_tris"};
    fprintf(stderr, "[mt prof]");
    for (int i = 0; i < PROF_COUNT; i++) fprintf(stderr, " %s=%llu", names[i], pr[i]);
    fprintf(stderr, "\n");
  }
#endif
  return check_status(c);
}

int mt_scene_kernel_times(mt_scene *s, int max_n, double *primary_ms, double *render_ms) {
  if (!s || max_n < 0 || (max_n > 0 && (!primary_ms || !render_ms))) {
    return fail(MT_ERR_ARG, "bad kernel_times arguments");
  }
  HIP_TRY(hipSetDevice(s->device));
  unsigned long long first = s->launches_read;
  if (s->launches_timed - first > (unsigned long long)mt_scene::kTimedLaunches) {
    first = s->launches_timed - mt_scene::kTimedLaunches;  // older ones were overwritten
  }
  if (s->launches_timed - first > (unsigned long long)max_n) first = s->launches_timed - max_n;
  int n = 0;
  for (unsigned long long i = first; i < s->launches_timed; i++, n++) {
    hipEvent_t *ek = s->ev_k[i % mt_scene::kTimedLaunches];
    HIP_TRY(hipEventSynchronize(ek[2]));
    float a = 0, b = 0;
    HIP_TRY(hipEventElapsedTime(&a, ek[0], ek[1]));
    HIP_TRY(hipEventElapsedTime(&b, ek[1], ek[2]));
    primary_ms[n] = a;
    render_ms[n] = b;
  }
  s->launches_read = s->launches_timed;
  return n;
}

int mt_scene_lean_info(mt_scene *s, mt_lean_info *out) {
  if (!s || !out) return fail(MT_ERR_ARG, "NULL argument");
  memset(out, 0, sizeof *out);
  HIP_TRY(hipSetDevice(s->device));
  out->lean = s->last_lean ? 1 : 0;
  if (!s->last_lean || s->last_lean_slot < 0) return MT_OK;
  HIP_TRY(hipDeviceSynchronize());
  unsigned w[8];
  HIP_TRY(hipMemcpy(w, s->d_work + kLeanCtl, sizeof w, hipMemcpyDeviceToHost));
  out->redo_units = w[kLeanRedoCount];
  out->units = w[kLeanUnits];
  out->handed_over = w[kLeanHandover] != 0u ? 1 : 0;
  hipEvent_t *ek = s->ev_k[s->last_lean_slot];
  float a = 0, b = 0;
  HIP_TRY(hipEventElapsedTime(&a, ek[1], ek[3]));
  HIP_TRY(hipEventElapsedTime(&b, ek[3], ek[2]));
  out->lean_ms = a;
  out->redo_ms = b;
  return MT_OK;
}

int mt_render_chunk_device(mt_scene *s, const mt_sensor *sensor, int image_w, int image_h,
                           int chunk_x, int chunk_y, int chunk_w, int chunk_h, int max_depth,
                           void *d_rgb, void *d_debug, void *stream) {
  MT_TRY(check_image_args(s, sensor, image_w, image_h));
  MT_TRY(check_chunk(image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h));
  if (!d_rgb) return fail(MT_ERR_ARG, "d_rgb is NULL");
  HIP_TRY(hipSetDevice(s->device));
  return launch_render(s, sensor, image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h, chunk_w,
                       chunk_h, 0, 1, 1, max_depth, (uint8_t *)d_rgb, (mt_debug_px *)d_debug,
                       (hipStream_t)stream);
}

int mt_render_tiles_device(mt_scene *s, const mt_sensor *sensor, int image_w, int image_h,
                           int tile_w, int tile_h, int first_tile, int tile_stride, int n_tiles,
                           int max_depth, void *d_rgb, void *stream) {
  MT_TRY(check_tiling(s, sensor, image_w, image_h, tile_w, tile_h, first_tile, tile_stride, n_tiles));
  MT_TRY(check_tile_selection(image_w, image_h, tile_w, tile_h, first_tile, tile_stride, n_tiles));
  if (!d_rgb && n_tiles > 0) return fail(MT_ERR_ARG, "d_rgb is NULL");
  HIP_TRY(hipSetDevice(s->device));
  return launch_render(s, sensor, image_w, image_h, 0, 0, image_w, image_h, tile_w, tile_h,
                       first_tile, tile_stride, n_tiles, max_depth, (uint8_t *)d_rgb, nullptr,
                       (hipStream_t)stream);
}

int mt_blit_tiles_device(mt_scene *s, int image_w, int image_h, int tile_w, int tile_h,
                         int first_tile, int tile_stride, int n_tiles, const void *d_tiles,
                         void *d_image, void *stream) {
  if (!s || !d_tiles || !d_image || image_w <= 0 || image_h <= 0 || tile_w <= 0 || tile_h <= 0 ||
      first_tile < 0 || tile_stride <= 0 || n_tiles < 0) {
    return fail(MT_ERR_ARG, "bad blit arguments");
  }
  MT_TRY(check_tile_selection(image_w, image_h, tile_w, tile_h, first_tile, tile_stride, n_tiles));
  if (n_tiles == 0) return MT_OK;
  HIP_TRY(hipSetDevice(s->device));
  hipLaunchKernelGGL(blit_tiles_kernel, dim3(1024), dim3(256), 0, (hipStream_t)stream, image_w,
                     image_h, tile_w, tile_h, (image_w + tile_w - 1) / tile_w, first_tile, tile_stride, n_tiles, (const int32_t *)nullptr,
                     (const uint8_t *)d_tiles, (uint8_t *)d_image);
  HIP_TRY(hipGetLastError());
  return MT_OK;
}

int mt_order_tiles_device(mt_scene *s, const void *d_cost_map, int map_w, int map_h, int image_w, int image_h,
                          int tile_w, int tile_h, void *d_order, void *stream) {
  if (!s || !d_cost_map || !d_order || map_w <= 0 || map_h <= 0 || image_w <= 0 || image_h <= 0 || tile_w <= 0 || tile_h <= 0 ||
      image_w > 100000 || image_h > 100000) {
    return fail(MT_ERR_ARG, "bad tile order arguments");
  }
  if (map_w < (image_w + 7) / 8 || map_h < (image_h + 7) / 8) return fail(MT_ERR_ARG, "cost map smaller than the image's 8x8 blocks");
  const int tiles_x = (image_w + tile_w - 1) / tile_w;
  const long long total = tile_count(image_w, image_h, tile_w, tile_h);
  if (total > (1ll << 20)) return fail(MT_ERR_ARG, "too many tiles to order (%lld)", total);
  HIP_TRY(hipSetDevice(s->device));
  MT_TRY(s->d_tile_cost.ensure((size_t)total * 8));
  const int n = (int)total;
  HIP_TRY(launch_flat(tile_cost_kernel, (size_t)n, (hipStream_t)stream, (const unsigned *)d_cost_map, map_w, map_h, image_w,
                      image_h, tile_w, tile_h, tiles_x, n, s->d_tile_cost.p));
  HIP_TRY(launch_flat(tile_order_kernel, (size_t)n, (hipStream_t)stream, s->d_tile_cost.p, n, (int32_t *)d_order));
  return MT_OK;
}

int mt_dealt_tile_count(int image_w, int image_h, int tile_w, int tile_h, int world, int rank) {
  if (image_w <= 0 || image_h <= 0 || tile_w <= 0 || tile_h <= 0 || world < 1 || rank < 0 || rank >= world) {
    return fail(MT_ERR_ARG, "bad tile count arguments");
  }
  const long long total = tile_count(image_w, image_h, tile_w, tile_h);
  if (total > 0x7fffffffll) return fail(MT_ERR_ARG, "too many tiles");
  return dealt_tile_count((int)total, world, rank);
}

int mt_deal_tiles_device(mt_scene *s, const void *d_order, int image_w, int image_h, int tile_w, int tile_h, int world,
                         int rank, void *d_list, void *stream) {
  if (!s || !d_list) return fail(MT_ERR_ARG, "bad deal arguments");
  const int n = mt_dealt_tile_count(image_w, image_h, tile_w, tile_h, world, rank);
  if (n <= 0) return n;
  const int total = (int)tile_count(image_w, image_h, tile_w, tile_h);
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(launch_flat(deal_tiles_kernel, (size_t)n, (hipStream_t)stream, (const int32_t *)d_order, total, world, rank, n,
                      (int32_t *)d_list));
  return n;
}

int mt_render_tile_list_device(mt_scene *s, const mt_sensor *sensor, int image_w, int image_h, int tile_w, int tile_h,
                               const void *d_list, int n_tiles, uint64_t list_id, int max_depth, void *d_rgb,
                               void *stream) {
  MT_TRY(check_tiling(s, sensor, image_w, image_h, tile_w, tile_h, 0, 1, n_tiles));
  const long long tiles_total = tile_count(image_w, image_h, tile_w, tile_h);
  if (n_tiles > tiles_total) return fail(MT_ERR_ARG, "%d tiles listed, the image has %lld", n_tiles, tiles_total);
  if (n_tiles > 0 && (!d_rgb || !d_list)) return fail(MT_ERR_ARG, "d_rgb or d_list is NULL");
  HIP_TRY(hipSetDevice(s->device));
  return launch_render(s, sensor, image_w, image_h, 0, 0, image_w, image_h, tile_w, tile_h, 0, 1, n_tiles, max_depth,
                       (uint8_t *)d_rgb, nullptr, (hipStream_t)stream, n_tiles > 0 ? (const int32_t *)d_list : nullptr,
                       (unsigned long long)list_id);
}

int mt_blit_tile_list_device(mt_scene *s, int image_w, int image_h, int tile_w, int tile_h, const void *d_list,
                             int n_tiles, const void *d_tiles, void *d_image, void *stream) {
  if (!s || !d_tiles || !d_image || !d_list || image_w <= 0 || image_h <= 0 || tile_w <= 0 || tile_h <= 0 || n_tiles < 0) {
    return fail(MT_ERR_ARG, "bad blit arguments");
  }
  if (n_tiles == 0) return MT_OK;
  HIP_TRY(hipSetDevice(s->device));
  hipLaunchKernelGGL(blit_tiles_kernel, dim3(1024), dim3(256), 0, (hipStream_t)stream, image_w, image_h, tile_w, tile_h,
                     (image_w + tile_w - 1) / tile_w, 0, 1, n_tiles, (const int32_t *)d_list, (const uint8_t *)d_tiles,
                     (uint8_t *)d_image);
  HIP_TRY(hipGetLastError());
  return MT_OK;
}

int mt_render_chunk(mt_scene *s, const mt_sensor *sensor, int image_w, int image_h, int chunk_x,
                    int chunk_y, int chunk_w, int chunk_h, int max_depth, uint8_t *out_rgb,
                    mt_debug_px *out_debug, mt_stats *stats) {
  if (!out_rgb) return fail(MT_ERR_ARG, "out_rgb is NULL");
  MT_TRY(check_image_args(s, sensor, image_w, image_h));
  HostCall call(s, stats, s->ev0, s->ev1);
  HIP_TRY(hipSetDevice(s->device));
  const size_t npx = (size_t)(chunk_w > 0 ? chunk_w : 0) * (size_t)(chunk_h > 0 ? chunk_h : 0);
  MT_TRY(begin_host_chunk(call, npx, out_debug != nullptr));
  MT_TRY(mt_render_chunk_device(s, sensor, image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h, max_depth, s->d_rgb,
                                out_debug ? s->d_debug.p : nullptr, call.stream));
  MT_TRY(finish_host_chunk(call, npx, out_rgb, out_debug));
#ifdef MT_PROF
  {  // (the phase profile is printed by mt_scene_read_stats)
    mt_stats dummy;
    (void)mt_scene_read_stats(s, &dummy);
  }
#endif
  return MT_OK;
}

// ---- supersampled frames: the sample frame is an ordinary launch at ss image_w x ss image_h, resolve_kernel
// (mt_resolve.h) makes the pixels.  `sensor` is the sensor of the SAMPLE grid. ----
int mt_render_chunk_ss_device(mt_scene *s, const mt_sensor *sensor, int image_w, int image_h, int chunk_x, int chunk_y,
                              int chunk_w, int chunk_h, int ss, int max_depth, void *d_rgb, void *stream) {
  MT_TRY(check_ss(ss, image_w, image_h));
  if (ss == 1) {
    return mt_render_chunk_device(s, sensor, image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h, max_depth, d_rgb,
                                  nullptr, stream);
  }
  MT_TRY(check_image_args(s, sensor, ss * image_w, ss * image_h));
  MT_TRY(check_chunk(image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h));
  if (!d_rgb) return fail(MT_ERR_ARG, "d_rgb is NULL");
  HIP_TRY(hipSetDevice(s->device));
  MT_TRY(ensure_samples(s, (size_t)chunk_w * chunk_h * 3 * ss * ss));
  MT_TRY(mt_render_chunk_device(s, sensor, ss * image_w, ss * image_h, ss * chunk_x, ss * chunk_y, ss * chunk_w,
                                ss * chunk_h, max_depth, s->d_samples, nullptr, stream));
  return launch_resolve(ss, chunk_w, chunk_h, chunk_w, chunk_h, 0, 1, nullptr, 1, s->d_samples, (uint8_t *)d_rgb,
                        (hipStream_t)stream);
}

int mt_render_chunk_ss(mt_scene *s, const mt_sensor *sensor, int image_w, int image_h, int chunk_x, int chunk_y,
                       int chunk_w, int chunk_h, int ss, int max_depth, uint8_t *out_rgb, mt_stats *stats) {
  MT_TRY(check_ss(ss, image_w, image_h));
  if (ss == 1) {
    return mt_render_chunk(s, sensor, image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h, max_depth, out_rgb, nullptr,
                           stats);
  }
  MT_TRY(check_image_args(s, sensor, ss * image_w, ss * image_h));
  if (!out_rgb) return fail(MT_ERR_ARG, "out_rgb is NULL");
  MT_TRY(check_chunk(image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h));
  HostCall call(s, stats, s->ev0, s->ev1);
  HIP_TRY(hipSetDevice(s->device));
  const size_t npx = (size_t)chunk_w * chunk_h;
  MT_TRY(begin_host_chunk(call, npx, false));
  MT_TRY(mt_render_chunk_ss_device(s, sensor, image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h, ss, max_depth, s->d_rgb,
                                   call.stream));
  return finish_host_chunk(call, npx, out_rgb, nullptr);
}

int mt_resolve_tiles_device(mt_scene *s, int image_w, int image_h, int tile_w, int tile_h, int first_tile,
                            int tile_stride, const void *d_list, int n_tiles, int ss, const void *d_samples,
                            void *d_tiles, void *stream) {
  MT_TRY(check_ss(ss, image_w, image_h));
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  if (tile_w <= 0 || tile_h <= 0 || first_tile < 0 || tile_stride <= 0 || n_tiles < 0) {
    return fail(MT_ERR_ARG, "bad tiling arguments");
  }
  if ((long long)ss * tile_w > 100000 || (long long)ss * tile_h > 100000) {
    return fail(MT_ERR_ARG, "tile size %dx%d with ss %d out of range", tile_w, tile_h, ss);
  }
  if (d_list == nullptr) {
    MT_TRY(check_tile_selection(image_w, image_h, tile_w, tile_h, first_tile, tile_stride, n_tiles));
  } else if (n_tiles > tile_count(image_w, image_h, tile_w, tile_h)) {
    return fail(MT_ERR_ARG, "%d tiles listed, the image has %lld", n_tiles, tile_count(image_w, image_h, tile_w, tile_h));
  }
  if (n_tiles == 0) return MT_OK;
  if (!d_samples || !d_tiles) return fail(MT_ERR_ARG, "d_samples or d_tiles is NULL");
  if (d_samples == d_tiles) return ss == 1 ? MT_OK : fail(MT_ERR_ARG, "d_samples and d_tiles are the same buffer");
  HIP_TRY(hipSetDevice(s->device));
  if (ss == 1) {  // the samples are the pixels
    HIP_TRY(hipMemcpyAsync(d_tiles, d_samples, (size_t)n_tiles * tile_w * tile_h * 3, hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
    return MT_OK;
  }
  return launch_resolve(ss, image_w, image_h, tile_w, tile_h, d_list ? 0 : first_tile, d_list ? 1 : tile_stride,
                        (const int32_t *)d_list, n_tiles, (const uint8_t *)d_samples, (uint8_t *)d_tiles,
                        (hipStream_t)stream);
}

// ---- adaptive supersampling (mt_adaptive.h): the plain launch, the blocks whose pixels differ, a tile-list launch of
// those blocks' samples on the scene's second forecast bank, the resolve over the plain frame ----
namespace {

// the blocks of a chunk (include/mythtracer_hip.h) and the kernels' arguments for them
RefineArgs refine_args(int image_w, int chunk_x, int chunk_y, int chunk_w, int chunk_h, int threshold) {
  RefineArgs A{};
  A.chunk_x = chunk_x; A.chunk_y = chunk_y; A.chunk_w = chunk_w; A.chunk_h = chunk_h;
  A.tiles_x = (image_w + 7) / 8;
  A.mask_x0 = chunk_x / 8;
  A.mask_y0 = chunk_y / 8;
  A.mask_w = (chunk_x + chunk_w - 1) / 8 - A.mask_x0 + 1;
  A.mask_h = (chunk_y + chunk_h - 1) / 8 - A.mask_y0 + 1;
  A.threshold = threshold;
  return A;
}

int check_threshold(int threshold) {
  if (threshold < 0 || threshold > 255) return fail(MT_ERR_ARG, "threshold %d outside [0, 255]", threshold);
  return MT_OK;
}

int check_image_size(int image_w, int image_h) {
  if (image_w <= 0 || image_h <= 0 || image_w > 100000 || image_h > 100000) {
    return fail(MT_ERR_ARG, "image size %dx%d out of range", image_w, image_h);
  }
  return MT_OK;
}

// refine_mask_kernel + refine_compact_kernel: flags in s->d_ad_flags (and d_mask), the list in d_list, count and hash
// in s->d_ad_ctl (the count in d_count too)
int launch_refine_mask(mt_scene *s, RefineArgs A, const uint8_t *d_rgb, uint8_t *d_mask, int32_t *d_list,
                       uint32_t *d_count, hipStream_t stream) {
  const size_t n_blocks = (size_t)A.mask_w * (size_t)A.mask_h;
  MT_TRY(s->d_ad_flags.ensure(n_blocks));
  MT_TRY(s->d_ad_ctl.ensure(sizeof(RefineCtl)));
  A.rgb = d_rgb;
  A.flags = s->d_ad_flags;
  A.mask_out = d_mask;
  const unsigned grid = (unsigned)std::min<size_t>((n_blocks + 3) / 4, 8192);
  hipLaunchKernelGGL(refine_mask_kernel, dim3(grid), dim3(256), 0, stream, A);
  hipLaunchKernelGGL(refine_compact_kernel, dim3(1), dim3(kRefineCompactThreads), 0, stream, A, d_list, d_count, s->d_ad_ctl.p);
  HIP_TRY(hipGetLastError());
  return MT_OK;
}

int launch_refine_resolve(int ss, const RefineArgs &M, int image_w, int image_h, const int32_t *d_list, int n_slots,
                          const uint8_t *d_samples, uint8_t *d_rgb, hipStream_t stream) {
  RefineResolveArgs A{};
  A.image_w = image_w; A.image_h = image_h;
  A.chunk_x = M.chunk_x; A.chunk_y = M.chunk_y; A.chunk_w = M.chunk_w; A.chunk_h = M.chunk_h;
  A.tiles_x = M.tiles_x;
  A.n_slots = n_slots;
  A.list = d_list;
  A.samples = d_samples;
  A.rgb = d_rgb;
  const dim3 grid((unsigned)std::min((n_slots + 3) / 4, 8192)), block(256);
  switch (ss) {
    case 2: hipLaunchKernelGGL(refine_resolve_kernel<2>, grid, block, 0, stream, A); break;
    case 3: hipLaunchKernelGGL(refine_resolve_kernel<3>, grid, block, 0, stream, A); break;
    case 4: hipLaunchKernelGGL(refine_resolve_kernel<4>, grid, block, 0, stream, A); break;
    default: return fail(MT_ERR_ARG, "ss %d has no resolve kernel", ss);
  }
  HIP_TRY(hipGetLastError());
  return MT_OK;
}

// The checks of the adaptive calls, before any device call: ss and the sample grid, threshold, the output pointer,
// image and chunk, the scene, the sensors.
int check_adaptive_args(const mt_scene *s, const mt_sensor *sensor, const mt_sensor *sensor_ss, int image_w, int image_h,
                        int chunk_x, int chunk_y, int chunk_w, int chunk_h, int ss, int threshold, const void *rgb,
                        const char *rgb_name) {
  MT_TRY(check_ss(ss, image_w, image_h));
  MT_TRY(check_threshold(threshold));
  if (!rgb) return fail(MT_ERR_ARG, "%s is NULL", rgb_name);
  MT_TRY(check_image_size(image_w, image_h));
  MT_TRY(check_chunk(image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h));
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  if (!sensor) return fail(MT_ERR_ARG, "sensor is NULL");
  if (ss > 1 && !sensor_ss) return fail(MT_ERR_ARG, "sensor_ss is NULL (the sensor of the sample grid, needed with ss > 1)");
  return MT_OK;
}

// The composed call on checked arguments.  *synced: events ev_ad[0] .. ev_ad[1] enclose the stream's idle time.
int render_adaptive(mt_scene *s, const mt_sensor *sensor, const mt_sensor *sensor_ss, int image_w, int image_h,
                    int chunk_x, int chunk_y, int chunk_w, int chunk_h, int ss, int threshold, int max_depth,
                    uint8_t *d_rgb, uint8_t *d_mask, mt_adaptive_info *info, hipStream_t stream, bool *synced) {
  *synced = false;
  const RefineArgs M = refine_args(image_w, chunk_x, chunk_y, chunk_w, chunk_h, threshold);
  const size_t n_blocks = (size_t)M.mask_w * (size_t)M.mask_h;
  mt_adaptive_info I{(int32_t)n_blocks, 0, 0, 0};
  MT_TRY(launch_render(s, sensor, image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h, chunk_w, chunk_h, 0, 1, 1,
                       max_depth, d_rgb, nullptr, stream));
  I.plain_history = s->bank0.last_history ? 1 : 0;
  if (ss == 1) {  // the plain call
    if (d_mask) HIP_TRY(hipMemsetAsync(d_mask, 0, n_blocks, stream));
    if (info) *info = I;
    return MT_OK;
  }
  MT_TRY(s->d_ad_list.ensure(n_blocks * sizeof(int32_t)));
  MT_TRY(s->h_ad_ctl.ensure(sizeof(RefineCtl)));
  for (hipEvent_t &e : s->ev_ad) {
    if (!e) HIP_TRY(hipEventCreate(&e));
  }
  MT_TRY(launch_refine_mask(s, M, d_rgb, d_mask, s->d_ad_list, nullptr, stream));
  // how many blocks, and which list: the one synchronisation of the call (a launch sizes its buffers on the host)
  HIP_TRY(hipMemcpyAsync(s->h_ad_ctl, s->d_ad_ctl, sizeof(RefineCtl), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipEventRecord(s->ev_ad[0], stream));
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipEventRecord(s->ev_ad[1], stream));
  *synced = true;
  const RefineCtl ctl = *s->h_ad_ctl.p;
  if ((size_t)ctl.count > n_blocks) return fail(MT_ERR_INTERNAL, "%u refined blocks of %zu: kernel logic error", ctl.count, n_blocks);
  I.n_refined = (int32_t)ctl.count;
  if (ctl.count > 0) {
    MT_TRY(ensure_samples(s, (size_t)ctl.count * 64 * 3 * ss * ss));
    if (!s->bank1) s->bank1.reset(new ForecastBank());
    MT_TRY(launch_render(s, sensor_ss, ss * image_w, ss * image_h, 0, 0, ss * image_w, ss * image_h, 8 * ss, 8 * ss, 0, 1,
                         (int)ctl.count, max_depth, s->d_samples, nullptr, stream, s->d_ad_list,
                         (unsigned long long)ctl.hash | 1ull, s->bank1.get()));
    I.refine_history = s->bank1->last_history ? 1 : 0;
    MT_TRY(launch_refine_resolve(ss, M, image_w, image_h, s->d_ad_list, (int)ctl.count, s->d_samples, d_rgb, stream));
  }
  if (info) *info = I;
  return MT_OK;
}

}  // namespace

int mt_refine_mask_device(mt_scene *s, int image_w, int image_h, int chunk_x, int chunk_y, int chunk_w, int chunk_h,
                          int threshold, const void *d_rgb, void *d_mask, void *d_list, void *d_count, void *stream) {
  MT_TRY(check_threshold(threshold));
  if (!d_rgb || !d_list || !d_count) return fail(MT_ERR_ARG, "d_rgb, d_list or d_count is NULL");
  MT_TRY(check_image_size(image_w, image_h));
  MT_TRY(check_chunk(image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h));
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  HIP_TRY(hipSetDevice(s->device));
  return launch_refine_mask(s, refine_args(image_w, chunk_x, chunk_y, chunk_w, chunk_h, threshold), (const uint8_t *)d_rgb,
                            (uint8_t *)d_mask, (int32_t *)d_list, (uint32_t *)d_count, (hipStream_t)stream);
}

int mt_render_chunk_adaptive_device(mt_scene *s, const mt_sensor *sensor, const mt_sensor *sensor_ss, int image_w,
                                    int image_h, int chunk_x, int chunk_y, int chunk_w, int chunk_h, int ss, int threshold,
                                    int max_depth, void *d_rgb, void *d_mask, mt_adaptive_info *info, void *stream) {
  MT_TRY(check_adaptive_args(s, sensor, sensor_ss, image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h, ss, threshold,
                             d_rgb, "d_rgb"));
  HIP_TRY(hipSetDevice(s->device));
  bool synced = false;
  return render_adaptive(s, sensor, sensor_ss, image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h, ss, threshold,
                         max_depth, (uint8_t *)d_rgb, (uint8_t *)d_mask, info, (hipStream_t)stream, &synced);
}

int mt_render_chunk_adaptive(mt_scene *s, const mt_sensor *sensor, const mt_sensor *sensor_ss, int image_w, int image_h,
                             int chunk_x, int chunk_y, int chunk_w, int chunk_h, int ss, int threshold, int max_depth,
                             uint8_t *out_rgb, uint8_t *out_mask, mt_adaptive_info *info, mt_stats *stats) {
  MT_TRY(check_adaptive_args(s, sensor, sensor_ss, image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h, ss, threshold,
                             out_rgb, "out_rgb"));
  HostCall call(s, stats, s->ev0, s->ev1);
  HIP_TRY(hipSetDevice(s->device));
  const size_t npx = (size_t)chunk_w * chunk_h;
  const RefineArgs M = refine_args(image_w, chunk_x, chunk_y, chunk_w, chunk_h, threshold);
  const size_t n_blocks = (size_t)M.mask_w * (size_t)M.mask_h;
  MT_TRY(begin_host_chunk(call, npx, false));
  if (out_mask) MT_TRY(s->d_ad_mask.ensure(n_blocks));
  bool synced = false;
  MT_TRY(render_adaptive(s, sensor, sensor_ss, image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h, ss, threshold, max_depth,
                         s->d_rgb, out_mask ? s->d_ad_mask.p : nullptr, info, call.stream, &synced));
  if (out_mask) HIP_TRY(hipMemcpyAsync(out_mask, s->d_ad_mask, n_blocks, hipMemcpyDeviceToHost, call.stream));
  MT_TRY(finish_host_chunk(call, npx, out_rgb, nullptr));
  if (stats && synced) {  // (the stream idled between these two while the host read the count)
    float idle = 0;
    HIP_TRY(hipEventElapsedTime(&idle, s->ev_ad[0], s->ev_ad[1]));
    stats->kernel_ms = std::max(0.0, stats->kernel_ms - (double)idle);
  }
  return MT_OK;
}

// ---- the primary-hit G-buffer (mt_gbuffer.h): one kernel next to the frame kernels.  Nothing here reads or writes
// what decide_launch looks at (cost history, signatures, launch counts, events of mt_scene_kernel_times). ----
namespace {

constexpr int kGbPlanes = 8;
// the planes of an mt_gbuffer in declaration order, and a pixel's bytes in each
void gb_planes(const mt_gbuffer &g, void *out[kGbPlanes]) {
  void *p[kGbPlanes] = {g.depth, g.point, g.normal, g.uvw, g.albedo, g.prim, g.line_no, g.material};
  for (int i = 0; i < kGbPlanes; i++) out[i] = p[i];
}
constexpr size_t kGbPixelBytes[kGbPlanes] = {8, 24, 24, 24, 24, 4, 4, 4};

// Checked before any device call; the order lets a caller without a device reach every message.
int check_gbuffer_args(const mt_scene *s, const mt_sensor *sensor, int image_w, int image_h, int chunk_x, int chunk_y,
                       int chunk_w, int chunk_h, const mt_gbuffer *out) {
  if (!out) return fail(MT_ERR_ARG, "the mt_gbuffer is NULL");
  void *p[kGbPlanes];
  gb_planes(*out, p);
  bool any = false;
  for (void *q : p) any = any || q != nullptr;
  if (!any) return fail(MT_ERR_ARG, "no plane of the mt_gbuffer is set");
  if (image_w <= 0 || image_h <= 0 || image_w > 100000 || image_h > 100000) {
    return fail(MT_ERR_ARG, "image size %dx%d out of range", image_w, image_h);
  }
  MT_TRY(check_chunk(image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h));
  MT_TRY(check_image_args(s, sensor, image_w, image_h));
  if (out->prim != nullptr && !s->have_tri_id) {
    return fail(MT_ERR_UNSUPPORTED, "the scene was created without mt_scene_desc::tri_id: no prim plane");
  }
  return MT_OK;
}

// What every kernel of persistent waves next to the frame kernels needs before its launch of `items` work items: the
// work counter (zeroed by the stream), the DEEP areas, the scene description on the device.  Returns the grid in *grid.
int prepare_persistent_launch(mt_scene *s, unsigned long long items, unsigned *grid, hipStream_t stream) {
  MT_TRY(s->d_gb_work.ensure(64));
  MT_TRY(ensure_deep(s, (size_t)s->grid_blocks * s->waves_per_block));
  if (!s->dev_uploaded_valid || memcmp(&s->dev_uploaded, &s->dev, sizeof(DevScene)) != 0) {  // (as launch_kernels)
    HIP_TRY(hipMemcpyAsync(s->d_dev, &s->dev, sizeof(DevScene), hipMemcpyHostToDevice, stream));
    memcpy(&s->dev_uploaded, &s->dev, sizeof(DevScene));
    s->dev_uploaded_valid = true;
  }
  HIP_TRY(hipMemsetAsync(s->d_gb_work, 0, sizeof(unsigned), stream));
  *grid = (unsigned)std::min<unsigned long long>((unsigned long long)s->grid_blocks,
                                                 (items + s->waves_per_block - 1) / s->waves_per_block);
  return MT_OK;
}

// What gbuffer_kernel and lightbuffer_kernel share on the host: the chunk's blocks, the device-side planes (`d`
// nullable: none), and prepare_persistent_launch.  Args = GBufferArgs or LightBufferArgs.  Returns the grid in *grid.
extern "C++" {  // (this file's functions sit inside one extern "C" block; a template needs C++ linkage)
template <typename Args>
int prepare_block_launch(mt_scene *s, const mt_sensor *sensor, int chunk_x, int chunk_y, int chunk_w, int chunk_h,
                         const mt_gbuffer *d, Args &A, unsigned *grid, hipStream_t stream) {
  A.sensor = *sensor;
  A.chunk_x = chunk_x; A.chunk_y = chunk_y; A.chunk_w = chunk_w; A.chunk_h = chunk_h;
  A.blocks_x = (chunk_w + 7) / 8;
  const unsigned long long items = (unsigned long long)A.blocks_x * (unsigned long long)((chunk_h + 7) / 8);
  if (items > 0xfffffff0ull) return fail(MT_ERR_ARG, "too many work items (%llu)", items);
  A.n_items = (unsigned)items;
  if (d != nullptr) {
    A.planes.depth = d->depth; A.planes.point = d->point; A.planes.normal = d->normal; A.planes.uvw = d->uvw;
    A.planes.albedo = d->albedo; A.planes.prim = d->prim; A.planes.line_no = d->line_no; A.planes.material = d->material;
    if (d->prim != nullptr && s->d_tri_id == nullptr) {  // first use (synchronous, once per scene)
      MT_TRY(s->d_tri_id.ensure(s->tri_id_host.size() * sizeof(int32_t)));
      HIP_TRY(hipMemcpy(s->d_tri_id, s->tri_id_host.data(), s->tri_id_host.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
  }
  MT_TRY(prepare_persistent_launch(s, items, grid, stream));
  A.planes.tri_id = s->d_tri_id;
  A.counters = s->d_counters;
  A.work_counter = s->d_gb_work;
  return MT_OK;
}
}  // extern "C++"

// gbuffer_kernel over the chunk, planes = device pointers
int launch_gbuffer(mt_scene *s, const mt_sensor *sensor, int chunk_x, int chunk_y, int chunk_w, int chunk_h,
                   const mt_gbuffer &d, hipStream_t stream) {
  GBufferArgs A{};
  unsigned grid = 0;
  MT_TRY(prepare_block_launch(s, sensor, chunk_x, chunk_y, chunk_w, chunk_h, &d, A, &grid, stream));
  hipLaunchKernelGGL(kernels_of(s->deep).gbuffer[s->stats_enabled ? 1 : 0], dim3(grid), dim3(s->waves_per_block * 64),
                     s->lds_bytes, stream, s->dev, A);
  HIP_TRY(hipGetLastError());
  return MT_OK;
}

// The host calls' way back: planes in device buffers reach the caller through the page-locked staging buffer in
// pieces of at most 4 MB, every piece's memcpy under the next piece's DMA (finish_host_chunk's path).  The counters
// travel first: no planes of a failed launch.  h_stage must hold staged_bytes(planes); ends with the stream idle and
// the call closed.
struct PlaneCopy { void *host; const void *dev; size_t bytes; };

size_t staged_bytes(const std::vector<PlaneCopy> &planes) {
  size_t total = 0;
  for (const PlaneCopy &p : planes) total += (p.bytes + 4095) & ~(size_t)4095;
  return total;
}

int planes_to_host(HostCall &call, const std::vector<PlaneCopy> &planes) {
  mt_scene *s = call.s;
  const hipStream_t stream = call.stream;
  MT_TRY(call.counters_home());
  struct Piece { uint8_t *dst; size_t off, bytes; };
  std::vector<Piece> pieces;
  constexpr size_t kPiece = 4u << 20;
  size_t at = 0;
  for (const PlaneCopy &p : planes) {
    for (size_t o = 0; o < p.bytes; o += kPiece) {
      const size_t n = std::min(kPiece, p.bytes - o);
      HIP_TRY(hipMemcpyAsync(s->h_stage + at + o, (const uint8_t *)p.dev + o, n, hipMemcpyDeviceToHost, stream));
      while (s->ev_gb.size() <= pieces.size()) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        s->ev_gb.push_back(e);
      }
      HIP_TRY(hipEventRecord(s->ev_gb[pieces.size()], stream));
      pieces.push_back({(uint8_t *)p.host + o, at + o, n});
    }
    at += (p.bytes + 4095) & ~(size_t)4095;
  }
  for (size_t k = 0; k < pieces.size(); k++) {
    HIP_TRY(hipEventSynchronize(s->ev_gb[k]));
    if (k == 0 && check_status(s->h_counters) != MT_OK) {
      (void)hipStreamSynchronize(stream);
      return check_status(s->h_counters);
    }
    memcpy(pieces[k].dst, s->h_stage + pieces[k].off, pieces[k].bytes);
  }
  return call.close();
}

// Scene-owned device buffers for the planes of `host` that are set (the host calls): the device-side mt_gbuffer in
// *d, and one PlaneCopy per plane appended to *copies.
int scene_planes(mt_scene *s, const mt_gbuffer &host_gb, size_t npx, mt_gbuffer *d, std::vector<PlaneCopy> *copies) {
  void *host[kGbPlanes], *dev[kGbPlanes] = {};
  gb_planes(host_gb, host);
  for (int i = 0; i < kGbPlanes; i++) {
    if (!host[i]) continue;
    if (i < 5) { MT_TRY(s->d_gb_f64[i].ensure(npx * kGbPixelBytes[i])); dev[i] = s->d_gb_f64[i].p; }
    else { MT_TRY(s->d_gb_i32[i - 5].ensure(npx * kGbPixelBytes[i])); dev[i] = s->d_gb_i32[i - 5].p; }
    copies->push_back({host[i], dev[i], npx * kGbPixelBytes[i]});
  }
  *d = mt_gbuffer{(double *)dev[0], (double *)dev[1], (double *)dev[2], (double *)dev[3], (double *)dev[4],
                  (int32_t *)dev[5], (int32_t *)dev[6], (int32_t *)dev[7]};
  return MT_OK;
}

}  // namespace

int mt_render_gbuffer_device(mt_scene *s, const mt_sensor *sensor, int image_w, int image_h, int chunk_x, int chunk_y,
                             int chunk_w, int chunk_h, const mt_gbuffer *d_out, void *stream) {
  MT_TRY(check_gbuffer_args(s, sensor, image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h, d_out));
  HIP_TRY(hipSetDevice(s->device));
  return launch_gbuffer(s, sensor, chunk_x, chunk_y, chunk_w, chunk_h, *d_out, (hipStream_t)stream);
}

// The host call: the requested planes in buffers the scene owns, then to the caller (planes_to_host).
int mt_render_gbuffer(mt_scene *s, const mt_sensor *sensor, int image_w, int image_h, int chunk_x, int chunk_y,
                      int chunk_w, int chunk_h, const mt_gbuffer *out, mt_stats *stats) {
  MT_TRY(check_gbuffer_args(s, sensor, image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h, out));
  HostCall call(s, stats, s->ev0, s->ev1);
  HIP_TRY(hipSetDevice(s->device));
  const size_t npx = (size_t)chunk_w * (size_t)chunk_h;
  std::vector<PlaneCopy> copies;
  mt_gbuffer d{};
  MT_TRY(scene_planes(s, *out, npx, &d, &copies));
  MT_TRY(s->h_stage.ensure(staged_bytes(copies)));
  MT_TRY(call.begin(true));
  MT_TRY(launch_gbuffer(s, sensor, chunk_x, chunk_y, chunk_w, chunk_h, d, call.stream));
  MT_TRY(call.mark_end());
  return planes_to_host(call, copies);
}

// ---- the direct-light buffer and the relight pass (mt_lightbuffer.h).  Like the G-buffer calls, nothing here reads
// or writes what decide_launch looks at. ----
namespace {

bool any_gb_plane(const mt_gbuffer *g) {
  if (!g) return false;
  void *p[kGbPlanes];
  gb_planes(*g, p);
  for (void *q : p) {
    if (q != nullptr) return true;
  }
  return false;
}

// Checked before any device call, in the order of the header: lb / gb pointers, image and chunk, scene, sensor, lights.
int check_lightbuffer_args(const mt_scene *s, const mt_sensor *sensor, int image_w, int image_h, int chunk_x, int chunk_y,
                           int chunk_w, int chunk_h, const mt_gbuffer *gb, const mt_lightbuffer *lb) {
  if (!lb) return fail(MT_ERR_ARG, "the mt_lightbuffer is NULL");
  if (!lb->power && !lb->in_shadow) return fail(MT_ERR_ARG, "no plane of the mt_lightbuffer is set");
  if (image_w <= 0 || image_h <= 0 || image_w > 100000 || image_h > 100000) {
    return fail(MT_ERR_ARG, "image size %dx%d out of range", image_w, image_h);
  }
  MT_TRY(check_chunk(image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h));
  MT_TRY(check_image_args(s, sensor, image_w, image_h));
  if (s->dev.n_lights == 0 && !any_gb_plane(gb)) {
    return fail(MT_ERR_ARG, "no lights are set and no G-buffer plane is requested: nothing to render");
  }
  if (gb && gb->prim != nullptr && !s->have_tri_id) {
    return fail(MT_ERR_UNSUPPORTED, "the scene was created without mt_scene_desc::tri_id: no prim plane");
  }
  return MT_OK;
}

// lightbuffer_kernel over the chunk, planes = device pointers
int launch_lightbuffer(mt_scene *s, const mt_sensor *sensor, int chunk_x, int chunk_y, int chunk_w, int chunk_h,
                       const mt_gbuffer *d_gb, const mt_lightbuffer &d_lb, hipStream_t stream) {
  LightBufferArgs A{};
  unsigned grid = 0;
  MT_TRY(prepare_block_launch(s, sensor, chunk_x, chunk_y, chunk_w, chunk_h, d_gb, A, &grid, stream));
  A.power = d_lb.power;
  A.in_shadow = d_lb.in_shadow;
  hipLaunchKernelGGL(kernels_of(s->deep).lightbuffer[s->stats_enabled ? 1 : 0], dim3(grid), dim3(s->waves_per_block * 64),
                     s->lds_bytes, stream, s->dev, A);
  HIP_TRY(hipGetLastError());
  return MT_OK;
}

int check_shade_args(const mt_scene *s, const mt_sensor *sensor, int image_w, int image_h, int chunk_x, int chunk_y,
                     int chunk_w, int chunk_h, const mt_gbuffer *gb, const mt_lightbuffer *lb, const mt_light *lights,
                     int n_lights, const void *rgb) {
  if (!lb) return fail(MT_ERR_ARG, "the mt_lightbuffer is NULL");
  if (!lb->power || !lb->in_shadow) return fail(MT_ERR_ARG, "the relight pass needs both planes of the mt_lightbuffer");
  if (!gb) return fail(MT_ERR_ARG, "the mt_gbuffer is NULL");
  if (!gb->point || !gb->normal || !gb->albedo || !gb->material) {
    return fail(MT_ERR_ARG, "the relight pass needs the point, normal, albedo and material planes of the mt_gbuffer");
  }
  if (!rgb) return fail(MT_ERR_ARG, "the output bitmap is NULL");
  if (image_w <= 0 || image_h <= 0 || image_w > 100000 || image_h > 100000) {
    return fail(MT_ERR_ARG, "image size %dx%d out of range", image_w, image_h);
  }
  MT_TRY(check_chunk(image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h));
  MT_TRY(check_image_args(s, sensor, image_w, image_h));
  if (n_lights < 0 || (n_lights > 0 && !lights)) return fail(MT_ERR_ARG, "bad lights argument");
  return MT_OK;
}

// shade_direct_kernel over the chunk, everything but `lights` = device pointers
int launch_shade_direct(mt_scene *s, const mt_sensor *sensor, int chunk_x, int chunk_y, int chunk_w, int chunk_h,
                        const mt_gbuffer &d_gb, const mt_lightbuffer &d_lb, const mt_light *lights, int n_lights,
                        uint8_t *d_rgb, hipStream_t stream) {
  ShadeDirectArgs A{};
  A.sensor = *sensor;
  A.chunk_x = chunk_x; A.chunk_y = chunk_y; A.chunk_w = chunk_w; A.chunk_h = chunk_h;
  A.point = d_gb.point; A.normal = d_gb.normal; A.albedo = d_gb.albedo; A.material = d_gb.material;
  A.power = d_lb.power; A.in_shadow = d_lb.in_shadow;
  A.mtls = s->dev.mtls;
  A.n_materials = s->n_materials;
  A.n_lights = n_lights;
  A.out_rgb = d_rgb;
  const bool in_args = n_lights <= kShadeArgLights;
  if (in_args) {
    for (int i = 0; i < n_lights; i++) A.lights[i] = lights[i];
  } else {
    MT_TRY(s->d_shade_lights.ensure((size_t)n_lights * sizeof(mt_light)));
    HIP_TRY(hipMemcpyAsync(s->d_shade_lights, lights, (size_t)n_lights * sizeof(mt_light), hipMemcpyHostToDevice, stream));
    A.d_lights = s->d_shade_lights;
  }
  const size_t npx = (size_t)chunk_w * (size_t)chunk_h;
  const size_t blocks = (npx + 255) / 256;
  if (blocks > 0x7fffffffull) return fail(MT_ERR_ARG, "too many pixels (%zu)", npx);
  hipLaunchKernelGGL(in_args ? shade_direct_kernel<true> : shade_direct_kernel<false>, dim3((unsigned)blocks), dim3(256), 0,
                     stream, A);
  HIP_TRY(hipGetLastError());
  return MT_OK;
}

// mt_update_lightbuffer[_device]: checked before any device call, in the order of the header.
int check_update_args(const mt_scene *s, int chunk_w, int chunk_h, const mt_gbuffer *gb, const int32_t *light_idx,
                      int n_idx, const mt_lightbuffer *lb) {
  if (!lb) return fail(MT_ERR_ARG, "the mt_lightbuffer is NULL");
  if (!lb->power && !lb->in_shadow) return fail(MT_ERR_ARG, "no plane of the mt_lightbuffer is set");
  if (!gb) return fail(MT_ERR_ARG, "the mt_gbuffer is NULL");
  if (!gb->point || !gb->material) {
    return fail(MT_ERR_ARG, "the light-buffer update needs the point and material planes of the mt_gbuffer");
  }
  if (chunk_w <= 0 || chunk_h <= 0 || chunk_w > 100000 || chunk_h > 100000) {
    return fail(MT_ERR_ARG, "chunk size %dx%d out of range", chunk_w, chunk_h);
  }
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  if (n_idx <= 0 || !light_idx) return fail(MT_ERR_ARG, "bad light index list");
  for (int i = 0; i < n_idx; i++) {
    if (light_idx[i] < 0 || light_idx[i] >= s->dev.n_lights) {
      return fail(MT_ERR_ARG, "light index %d outside the scene's %d lights", light_idx[i], s->dev.n_lights);
    }
  }
  // (no index is listed twice: at most n_lights entries are compared)
  std::vector<bool> seen((size_t)s->dev.n_lights, false);
  for (int i = 0; i < n_idx; i++) {
    if (seen[(size_t)light_idx[i]]) return fail(MT_ERR_ARG, "light index %d is listed twice", light_idx[i]);
    seen[(size_t)light_idx[i]] = true;
  }
  return MT_OK;
}

// lightbuffer_update_kernel over the chunk x the listed lights; planes = device pointers, light_idx = host array
int launch_lightbuffer_update(mt_scene *s, int chunk_w, int chunk_h, const mt_gbuffer &d_gb, const int32_t *light_idx,
                              int n_idx, const mt_lightbuffer &d_lb, hipStream_t stream) {
  LightUpdateArgs A{};
  A.chunk_w = chunk_w; A.chunk_h = chunk_h;
  A.blocks_x = (chunk_w + 7) / 8;
  const unsigned long long blocks = (unsigned long long)A.blocks_x * (unsigned long long)((chunk_h + 7) / 8);
  const unsigned long long items = blocks * (unsigned long long)n_idx;
  if (items > 0xfffffff0ull) return fail(MT_ERR_ARG, "too many work items (%llu)", items);
  A.n_blocks = (unsigned)blocks;
  A.n_items = (unsigned)items;
  A.point = d_gb.point; A.material = d_gb.material;
  A.n_materials = s->n_materials;
  A.power = d_lb.power; A.in_shadow = d_lb.in_shadow;
  if (n_idx <= kUpdateArgLights) {
    for (int i = 0; i < n_idx; i++) A.idx[i] = light_idx[i];
  } else {
    MT_TRY(s->d_update_idx.ensure((size_t)n_idx * sizeof(int32_t)));
    HIP_TRY(hipMemcpyAsync(s->d_update_idx, light_idx, (size_t)n_idx * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    A.d_idx = s->d_update_idx;
  }
  unsigned grid = 0;
  MT_TRY(prepare_persistent_launch(s, items, &grid, stream));
  A.counters = s->d_counters;
  A.work_counter = s->d_gb_work;
  hipLaunchKernelGGL(kernels_of(s->deep).lightbuffer_update[s->stats_enabled ? 1 : 0], dim3(grid),
                     dim3(s->waves_per_block * 64), s->lds_bytes, stream, s->dev, A);
  HIP_TRY(hipGetLastError());
  return MT_OK;
}

}  // namespace

int mt_render_lightbuffer_device(mt_scene *s, const mt_sensor *sensor, int image_w, int image_h, int chunk_x, int chunk_y,
                                 int chunk_w, int chunk_h, const mt_gbuffer *d_gb, const mt_lightbuffer *d_lb,
                                 void *stream) {
  MT_TRY(check_lightbuffer_args(s, sensor, image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h, d_gb, d_lb));
  HIP_TRY(hipSetDevice(s->device));
  return launch_lightbuffer(s, sensor, chunk_x, chunk_y, chunk_w, chunk_h, d_gb, *d_lb, (hipStream_t)stream);
}

int mt_render_lightbuffer(mt_scene *s, const mt_sensor *sensor, int image_w, int image_h, int chunk_x, int chunk_y,
                          int chunk_w, int chunk_h, const mt_gbuffer *gb, const mt_lightbuffer *lb, mt_stats *stats) {
  MT_TRY(check_lightbuffer_args(s, sensor, image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h, gb, lb));
  HostCall call(s, stats, s->ev0, s->ev1);
  HIP_TRY(hipSetDevice(s->device));
  const size_t npx = (size_t)chunk_w * (size_t)chunk_h;
  const size_t n_l = (size_t)s->dev.n_lights;
  std::vector<PlaneCopy> copies;
  mt_gbuffer d{};
  if (gb) MT_TRY(scene_planes(s, *gb, npx, &d, &copies));
  mt_lightbuffer dl{};
  if (lb->power && n_l > 0) {
    MT_TRY(s->d_lb_power.ensure(n_l * npx * 24));
    dl.power = s->d_lb_power;
    copies.push_back({lb->power, dl.power, n_l * npx * 24});
  }
  if (lb->in_shadow && n_l > 0) {
    MT_TRY(s->d_lb_shadow.ensure(n_l * npx));
    dl.in_shadow = s->d_lb_shadow;
    copies.push_back({lb->in_shadow, dl.in_shadow, n_l * npx});
  }
  MT_TRY(s->h_stage.ensure(staged_bytes(copies)));
  MT_TRY(call.begin(true));
  MT_TRY(launch_lightbuffer(s, sensor, chunk_x, chunk_y, chunk_w, chunk_h, gb ? &d : nullptr, dl, call.stream));
  MT_TRY(call.mark_end());
  return planes_to_host(call, copies);
}

int mt_shade_direct_device(mt_scene *s, const mt_sensor *sensor, int image_w, int image_h, int chunk_x, int chunk_y,
                           int chunk_w, int chunk_h, const mt_gbuffer *d_gb, const mt_lightbuffer *d_lb,
                           const mt_light *lights, int n_lights, void *d_rgb, void *stream) {
  MT_TRY(check_shade_args(s, sensor, image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h, d_gb, d_lb, lights, n_lights,
                          d_rgb));
  HIP_TRY(hipSetDevice(s->device));
  return launch_shade_direct(s, sensor, chunk_x, chunk_y, chunk_w, chunk_h, *d_gb, *d_lb, lights, n_lights,
                             (uint8_t *)d_rgb, (hipStream_t)stream);
}

// The host form: the six planes go up into buffers the scene owns, the bitmap comes back.
int mt_shade_direct(mt_scene *s, const mt_sensor *sensor, int image_w, int image_h, int chunk_x, int chunk_y,
                    int chunk_w, int chunk_h, const mt_gbuffer *gb, const mt_lightbuffer *lb, const mt_light *lights,
                    int n_lights, uint8_t *out_rgb, mt_stats *stats) {
  MT_TRY(check_shade_args(s, sensor, image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h, gb, lb, lights, n_lights,
                          out_rgb));
  HostCall call(s, stats, s->ev0, s->ev1);
  HIP_TRY(hipSetDevice(s->device));
  const size_t npx = (size_t)chunk_w * (size_t)chunk_h;
  const size_t n_l = (size_t)n_lights;
  const hipStream_t stream = call.stream;
  MT_TRY(s->d_gb_f64[1].ensure(npx * 24));
  MT_TRY(s->d_gb_f64[2].ensure(npx * 24));
  MT_TRY(s->d_gb_f64[4].ensure(npx * 24));
  MT_TRY(s->d_gb_i32[2].ensure(npx * 4));
  MT_TRY(s->d_lb_power.ensure(n_l * npx * 24));
  MT_TRY(s->d_lb_shadow.ensure(n_l * npx));
  MT_TRY(s->d_rgb.ensure(npx * 3));
  mt_gbuffer d{};
  d.point = s->d_gb_f64[1]; d.normal = s->d_gb_f64[2]; d.albedo = s->d_gb_f64[4]; d.material = s->d_gb_i32[2];
  const mt_lightbuffer dl{s->d_lb_power, s->d_lb_shadow};
  HIP_TRY(hipMemcpyAsync(d.point, gb->point, npx * 24, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d.normal, gb->normal, npx * 24, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d.albedo, gb->albedo, npx * 24, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d.material, gb->material, npx * 4, hipMemcpyHostToDevice, stream));
  if (n_l > 0) {
    HIP_TRY(hipMemcpyAsync(dl.power, lb->power, n_l * npx * 24, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(dl.in_shadow, lb->in_shadow, n_l * npx, hipMemcpyHostToDevice, stream));
  }
  MT_TRY(call.begin(false));  // (no ray, no traversal: every work counter is zero)
  MT_TRY(launch_shade_direct(s, sensor, chunk_x, chunk_y, chunk_w, chunk_h, d, dl, lights, n_lights, s->d_rgb, stream));
  MT_TRY(call.mark_end());
  HIP_TRY(hipMemcpyAsync(out_rgb, s->d_rgb, npx * 3, hipMemcpyDeviceToHost, stream));
  return call.close();
}

int mt_update_lightbuffer_device(mt_scene *s, int chunk_w, int chunk_h, const mt_gbuffer *d_gb, const int32_t *light_idx,
                                 int n_idx, const mt_lightbuffer *d_lb, void *stream) {
  MT_TRY(check_update_args(s, chunk_w, chunk_h, d_gb, light_idx, n_idx, d_lb));
  HIP_TRY(hipSetDevice(s->device));
  return launch_lightbuffer_update(s, chunk_w, chunk_h, *d_gb, light_idx, n_idx, *d_lb, (hipStream_t)stream);
}

// The host form: point and material go up into the scene's G-buffer buffers; the planes of the LISTED lights are
// computed at their places in the scene's light-buffer buffers and only they come back (planes_to_host) -- nothing of
// the caller's other planes travels in either direction.
int mt_update_lightbuffer(mt_scene *s, int chunk_w, int chunk_h, const mt_gbuffer *gb, const int32_t *light_idx, int n_idx,
                          const mt_lightbuffer *lb, mt_stats *stats) {
  MT_TRY(check_update_args(s, chunk_w, chunk_h, gb, light_idx, n_idx, lb));
  HostCall call(s, stats, s->ev0, s->ev1);
  HIP_TRY(hipSetDevice(s->device));
  const size_t npx = (size_t)chunk_w * (size_t)chunk_h;
  const size_t n_l = (size_t)s->dev.n_lights;
  const hipStream_t stream = call.stream;
  MT_TRY(s->d_gb_f64[1].ensure(npx * 24));
  MT_TRY(s->d_gb_i32[2].ensure(npx * 4));
  mt_gbuffer d{};
  d.point = s->d_gb_f64[1]; d.material = s->d_gb_i32[2];
  mt_lightbuffer dl{};
  std::vector<PlaneCopy> copies;
  if (lb->power) {
    MT_TRY(s->d_lb_power.ensure(n_l * npx * 24));
    dl.power = s->d_lb_power;
  }
  if (lb->in_shadow) {
    MT_TRY(s->d_lb_shadow.ensure(n_l * npx));
    dl.in_shadow = s->d_lb_shadow;
  }
  for (int i = 0; i < n_idx; i++) {
    const size_t l = (size_t)light_idx[i];
    if (lb->power) copies.push_back({lb->power + l * npx * 3, dl.power + l * npx * 3, npx * 24});
    if (lb->in_shadow) copies.push_back({lb->in_shadow + l * npx, dl.in_shadow + l * npx, npx});
  }
  MT_TRY(s->h_stage.ensure(staged_bytes(copies)));
  HIP_TRY(hipMemcpyAsync(d.point, gb->point, npx * 24, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d.material, gb->material, npx * 4, hipMemcpyHostToDevice, stream));
  MT_TRY(call.begin(true));
  MT_TRY(launch_lightbuffer_update(s, chunk_w, chunk_h, d, light_idx, n_idx, dl, stream));
  MT_TRY(call.mark_end());
  return planes_to_host(call, copies);
}

// ---- edited textures and the deferred path (mt_gbuffer.h, gbuffer_retexture_kernel): stateless, like
// mt_update_lightbuffer ----
namespace {

// mt_retexture_gbuffer[_device]: checked before any device call, in the order of the header.
int check_retexture_args(const mt_scene *s, int chunk_w, int chunk_h, const mt_gbuffer *gb) {
  if (!gb) return fail(MT_ERR_ARG, "the mt_gbuffer is NULL");
  if (!gb->material || !gb->albedo) {
    return fail(MT_ERR_ARG, "the retexture needs the material and albedo planes of the mt_gbuffer");
  }
  if (!gb->uvw && s) {
    for (size_t i = 0; i < s->mtls_host.size(); i++) {
      if (s->mtls_host[i].tex >= 0) {
        return fail(MT_ERR_ARG, "material %d has a texture: the retexture needs the uvw plane of the mt_gbuffer", (int)i);
      }
    }
  }
  if (chunk_w <= 0 || chunk_h <= 0 || chunk_w > 100000 || chunk_h > 100000) {
    return fail(MT_ERR_ARG, "chunk size %dx%d out of range", chunk_w, chunk_h);
  }
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  return MT_OK;
}

// gbuffer_retexture_kernel over the chunk's pixels; planes = device pointers
int launch_gbuffer_retexture(mt_scene *s, size_t npx, const mt_gbuffer &d_gb, hipStream_t stream) {
  GBufferRetextureArgs A{};
  A.material = d_gb.material; A.uvw = d_gb.uvw; A.albedo = d_gb.albedo;
  A.mtls = s->dev.mtls;
  A.texs = s->dev.texs;
  A.n = npx;
  A.n_materials = s->n_materials;
  HIP_TRY(launch_flat(gbuffer_retexture_kernel, npx, stream, A));
  return MT_OK;
}

}  // namespace

int mt_retexture_gbuffer_device(mt_scene *s, int chunk_w, int chunk_h, const mt_gbuffer *d_gb, void *stream) {
  MT_TRY(check_retexture_args(s, chunk_w, chunk_h, d_gb));
  HIP_TRY(hipSetDevice(s->device));
  return launch_gbuffer_retexture(s, (size_t)chunk_w * (size_t)chunk_h, *d_gb, (hipStream_t)stream);
}

// The host form: material and uvw go up into the scene's G-buffer buffers, only the albedo comes back.
int mt_retexture_gbuffer(mt_scene *s, int chunk_w, int chunk_h, const mt_gbuffer *gb, mt_stats *stats) {
  MT_TRY(check_retexture_args(s, chunk_w, chunk_h, gb));
  HostCall call(s, stats, s->ev0, s->ev1);
  HIP_TRY(hipSetDevice(s->device));
  const size_t npx = (size_t)chunk_w * (size_t)chunk_h;
  const hipStream_t stream = call.stream;
  MT_TRY(s->d_gb_i32[2].ensure(npx * 4));
  MT_TRY(s->d_gb_f64[4].ensure(npx * 24));
  mt_gbuffer d{};
  d.material = s->d_gb_i32[2]; d.albedo = s->d_gb_f64[4];
  HIP_TRY(hipMemcpyAsync(d.material, gb->material, npx * 4, hipMemcpyHostToDevice, stream));
  if (gb->uvw) {
    MT_TRY(s->d_gb_f64[3].ensure(npx * 24));
    d.uvw = s->d_gb_f64[3];
    HIP_TRY(hipMemcpyAsync(d.uvw, gb->uvw, npx * 24, hipMemcpyHostToDevice, stream));
  }
  MT_TRY(call.begin(false));  // (no ray, no traversal: every work counter is zero)
  MT_TRY(launch_gbuffer_retexture(s, npx, d, stream));
  MT_TRY(call.mark_end());
  HIP_TRY(hipMemcpyAsync(gb->albedo, d.albedo, npx * 24, hipMemcpyDeviceToHost, stream));
  return call.close();
}

// ---- the ray-tree buffer (mt_raytree.h).  Like the G-buffer and light-buffer calls, nothing here reads or writes what
// decide_launch looks at. ----
struct mt_raytree {
  mt_scene *scene = nullptr;
  mt_raytree_desc info{};
  mt_sensor sensor{};
  void *alloc[MT_MAX_RECURSION + 1] = {};  // one allocation per layer
  RayTreeLayer layer[MT_MAX_RECURSION + 1] = {};
  unsigned long long *d_count = nullptr;   // the compaction's answer
  uint8_t *d_rgb = nullptr;                // the host shade's bitmap (first use)
  double *d_out_color = nullptr;           // the host shade's colours (first use)
  unsigned int *d_bad = nullptr;           // a ray-list tree: raytree_rays_kernel's count and lowest index of refused rays
  // mt_raytree_update_materials: the materials the planes are valid for (the scene's at creation or at the last
  // successful update) and the scene's generation then; raytree_recoef_kernel's two words and raytree_recommit_kernel's
  // byte per material (first use)
  std::vector<mt_material> mtls;
  unsigned long long mtl_generation = 0;
  // the scene's generation of every texture then (mt_scene_set_texture), and whether the layers have a uvw plane: the
  // scene's mt_scene_set_raytree_uvw switch when the tree was made
  std::vector<unsigned long long> tex_generation;
  bool keep_uvw = false;
  // the scene's assignment then (mt_scene_set_triangle_materials: the scene's own vector of that time, shared) with its
  // generation, and whether the layers have a tri plane: the scene's mt_scene_set_raytree_tri switch when the tree was made
  std::shared_ptr<const std::vector<int32_t>> tri_mtl;
  unsigned long long asg_generation = 0;
  bool keep_tri = false;
  // the scene's two attribute generations then (mt_scene_set_triangle_normals / _uvw), the kernels' kRayTreeAttrWords
  // counts (first use) and what the last update or regrow made of them (mt_raytree_attr_info_last)
  uint32_t attr_generation[2] = {0, 0};
  unsigned long long geo_generation = 0;  // the scene's geometry generation at creation (mt_scene_set_triangle_vertices)
  unsigned long long *d_attr_count = nullptr;
  mt_raytree_attr_info attr_last{};
  unsigned long long *d_mismatch = nullptr;
  uint8_t *d_albedo_changed = nullptr;
  // mt_raytree_regrow_materials (first use, grown when a call needs more): `src` of the new layers k and k + 1 in turn,
  // layer 0's child indices and spawn bytes while the new tree is built aside, the temporary layer of the traced rays
  int32_t *d_src[2] = {};
  void *d_regrow0 = nullptr, *d_tmp = nullptr;
  size_t src_cap[2] = {}, regrow0_cap = 0, tmp_cap = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_layer[MT_MAX_RECURSION + 1][2] = {};
};

namespace {

// One allocation holds a layer's planes, each at a multiple of 256 bytes: the planes of layer k with n rays and n_l
// lights laid out from `base` (nullptr: only the size is wanted).  Returns the bytes.  The uvw plane of a tree that
// keeps one comes last, [n][3] doubles at a multiple of 256 bytes: without it a layer is laid out as it always was.
// The tri plane of a tree that keeps one comes behind that, [n] int32, unpadded too.
size_t raytree_carve_layer(void *base, size_t n_l, int k, size_t n, bool keep_uvw, bool keep_tri, RayTreeLayer *out) {
  struct Part { void **at; size_t bytes; };
  RayTreeLayer &L = *out;
  const Part parts[] = {
      {(void **)&L.ray, n * 48}, {(void **)&L.coef, n * 8}, {(void **)&L.point, n * 24}, {(void **)&L.normal, n * 24},
      {(void **)&L.albedo, n * 24}, {(void **)&L.power, n_l * n * 24}, {(void **)&L.color, n * 24},
      {(void **)&L.material, n * 4}, {(void **)&L.child_refl, n * 4}, {(void **)&L.child_refr, n * 4},
      {(void **)&L.pixel, k == 0 ? n * 4 : 0}, {(void **)&L.in_object, n}, {(void **)&L.in_shadow, n_l * n},
      {(void **)&L.spawn, n}};
  size_t at = 0;
  for (const Part &p : parts) {
    if (base != nullptr) *p.at = (char *)base + at;
    at += (p.bytes + 255) & ~(size_t)255;
  }
  if (k != 0) L.pixel = nullptr;
  // (behind the last padded plane, itself unpadded: the layer grows by exactly 24 bytes per ray)
  L.uvw = keep_uvw && base != nullptr ? (double *)((char *)base + at) : nullptr;
  if (keep_uvw) at += n * 24;
  // (at a multiple of 8 bytes either way: the layer grows by exactly 4 bytes per ray)
  L.tri = keep_tri && base != nullptr ? (int32_t *)((char *)base + at) : nullptr;
  if (keep_tri) at += n * 4;
  return at;
}

int raytree_alloc_layer(mt_raytree *t, int k, size_t n) {
  const size_t n_l = (size_t)t->info.n_lights;
  RayTreeLayer &L = t->layer[k];
  const size_t total = raytree_carve_layer(nullptr, n_l, k, n, t->keep_uvw, t->keep_tri, &L);
  char what[64];
  snprintf(what, sizeof what, "layer %d of the ray tree (%zu rays)", k, n);
  MT_TRY(device_malloc(&t->alloc[k], total, what));
  (void)raytree_carve_layer(t->alloc[k], n_l, k, n, t->keep_uvw, t->keep_tri, &L);
  t->info.bytes += total;
  t->info.n_rays[k] = (int64_t)n;
  t->info.n_layers = k + 1;
  return MT_OK;
}

int check_raytree_create_args(const mt_scene *s, const mt_sensor *sensor, int image_w, int image_h, int chunk_x,
                              int chunk_y, int chunk_w, int chunk_h, int max_depth) {
  if (image_w <= 0 || image_h <= 0 || image_w > 100000 || image_h > 100000) {
    return fail(MT_ERR_ARG, "image size %dx%d out of range", image_w, image_h);
  }
  MT_TRY(check_chunk(image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h));
  MT_TRY(check_image_args(s, sensor, image_w, image_h));
  if (max_depth < 0 || max_depth > MT_MAX_RECURSION) {
    return fail(MT_ERR_ARG, "max_depth %d outside [0, %d]", max_depth, MT_MAX_RECURSION);
  }
  return MT_OK;
}

// mt_raytree_create_rays[_device]: checked before any device call, in the order of the header.
int check_raytree_rays_args(const mt_scene *s, const mt_ray_list *rays, int max_depth, bool on_host) {
  if (!rays || !rays->ray) return fail(MT_ERR_ARG, "the ray list is NULL");
  if (rays->list_w < 1 || rays->list_h < 1) {
    return fail(MT_ERR_ARG, "ray list size %dx%d out of range", rays->list_w, rays->list_h);
  }
  const long long n = (long long)rays->list_w * (long long)rays->list_h;
  if (n >= 0x80000000ll) return fail(MT_ERR_ARG, "layer 0 of the ray tree would have %lld rays (2^31 or more)", n);
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  if (max_depth < 0 || max_depth > MT_MAX_RECURSION) {
    return fail(MT_ERR_ARG, "max_depth %d outside [0, %d]", max_depth, MT_MAX_RECURSION);
  }
  if (!on_host) return MT_OK;
  // the content of the list: what raytree_rays_kernel refuses, found before anything is copied
  long long bad = 0, first = -1;
  for (long long p = 0; p < n; p++) {
    const double *r = rays->ray + p * 6;
    bool ok = std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2]) && std::isfinite(r[3]) &&
              std::isfinite(r[4]) && std::isfinite(r[5]) && !(r[3] == 0.0 && r[4] == 0.0 && r[5] == 0.0);
    if (rays->in_object && rays->in_object[p] > 1) ok = false;
    if (rays->coef && !std::isfinite(rays->coef[p])) ok = false;
    if (!ok && bad++ == 0) first = p;
  }
  if (bad) return fail(MT_ERR_ARG, "%lld rays of the list cannot be traced, the first at index %lld", bad, first);
  return MT_OK;
}

// a tree made before the scene's triangles were moved is refused for good: its tri plane and hit points belong to the
// old geometry (checked directly before the stale-materials check; the tree is left untouched)
int check_raytree_geometry(const mt_raytree *t) {
  if (t->geo_generation != t->scene->geo_generation) {
    return fail(MT_ERR_ARG, "the scene's triangles were moved after the ray tree was made (mt_scene_set_triangle_vertices): "
                            "its hits belong to the old geometry; destroy the tree and make a new one");
  }
  return MT_OK;
}

// a tree whose scene's materials were edited since it was made or last updated is stale (the last check of every
// call that shades or re-traces it)
int check_raytree_fresh(const mt_raytree *t) {
  MT_TRY(check_raytree_geometry(t));
  if (t->mtl_generation != t->scene->mtl_generation) {
    return fail(MT_ERR_ARG, "the scene's materials were edited after the ray tree was made: mt_raytree_update_materials "
                            "or a new tree is needed");
  }
  return MT_OK;
}

int check_raytree_shade_args(const mt_raytree *t, const mt_light *lights, int n_lights, const void *out,
                             const char *no_output = "the output bitmap is NULL") {
  if (!out) return fail(MT_ERR_ARG, "%s", no_output);
  if (!t) return fail(MT_ERR_ARG, "the ray tree is NULL");
  if (n_lights < 0 || (n_lights > 0 && !lights)) return fail(MT_ERR_ARG, "bad lights argument");
  if (n_lights != t->info.n_lights) {
    return fail(MT_ERR_ARG, "%d lights for a ray tree made with %d", n_lights, t->info.n_lights);
  }
  return check_raytree_fresh(t);
}

// mt_raytree_update_lights[_device]: checked before any device call, in the order of the header.
int check_raytree_update_args(const mt_raytree *t, const int32_t *light_idx, int n_idx) {
  if (!t) return fail(MT_ERR_ARG, "the ray tree is NULL");
  if (n_idx <= 0 || !light_idx) return fail(MT_ERR_ARG, "bad light index list");
  const int n_lights = t->info.n_lights;
  if (t->scene->dev.n_lights != n_lights) {
    return fail(MT_ERR_ARG, "the scene has %d lights, the ray tree was made with %d", t->scene->dev.n_lights, n_lights);
  }
  for (int i = 0; i < n_idx; i++) {
    if (light_idx[i] < 0 || light_idx[i] >= n_lights) {
      return fail(MT_ERR_ARG, "light index %d outside the ray tree's %d lights", light_idx[i], n_lights);
    }
  }
  // (no index is listed twice: at most n_lights entries are compared)
  std::vector<bool> seen((size_t)n_lights, false);
  for (int i = 0; i < n_idx; i++) {
    if (seen[(size_t)light_idx[i]]) return fail(MT_ERR_ARG, "light index %d is listed twice", light_idx[i]);
    seen[(size_t)light_idx[i]] = true;
  }
  return check_raytree_fresh(t);
}

// raytree_update_kernel over all layers x the listed lights, one launch; light_idx = host array
int launch_raytree_update(mt_raytree *t, const int32_t *light_idx, int n_idx, hipStream_t stream) {
  mt_scene *s = t->scene;
  RayTreeUpdateArgs A{};
  unsigned long long per_light = 0;
  for (int k = 0; k < t->info.n_layers; k++) {
    const RayTreeLayer &L = t->layer[k];
    RayTreeUpdateLayer &U = A.layer[k];
    U.point = L.point; U.material = L.material; U.power = L.power; U.in_shadow = L.in_shadow;
    U.n_rays = (uint32_t)t->info.n_rays[k];
    U.first_item = (uint32_t)per_light;  // (a layer has fewer than 2^31 rays: 17 layers stay below 2^32 items)
    per_light += ((unsigned long long)t->info.n_rays[k] + 63) / 64;
  }
  const unsigned long long items = per_light * (unsigned long long)n_idx;
  if (items > 0xfffffff0ull) return fail(MT_ERR_ARG, "too many work items (%llu)", items);
  A.n_layers = t->info.n_layers;
  A.n_materials = s->n_materials;
  A.items_per_light = (unsigned)per_light;
  A.n_items = (unsigned)items;
  if (n_idx <= kUpdateArgLights) {
    for (int i = 0; i < n_idx; i++) A.idx[i] = light_idx[i];
  } else {
    MT_TRY(s->d_update_idx.ensure((size_t)n_idx * sizeof(int32_t)));
    HIP_TRY(hipMemcpyAsync(s->d_update_idx, light_idx, (size_t)n_idx * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    A.d_idx = s->d_update_idx;
  }
  unsigned grid = 0;
  MT_TRY(prepare_persistent_launch(s, items, &grid, stream));
  A.counters = s->d_counters;
  A.work_counter = s->d_gb_work;
  hipLaunchKernelGGL(kernels_of(s->deep).raytree_update[s->stats_enabled ? 1 : 0], dim3(grid),
                     dim3(s->waves_per_block * 64), s->lds_bytes, stream, s->dev, A);
  HIP_TRY(hipGetLastError());
  return MT_OK;
}

// the counters so far, checked: no further layer after a tripped bound
int raytree_read_counters(mt_scene *s, hipStream_t stream) {
  HIP_TRY(hipMemcpyAsync(s->h_counters, s->d_counters, ST_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return check_status(s->h_counters);
}

// Layer 0 of a ray-list tree: the caller's rays (host or device pointers in `rays`) through raytree_rays_kernel.
// Synchronises: no tracing kernel is launched before the kernel's count of refused rays has been read.
int raytree_import_rays(mt_raytree *t, const mt_ray_list *rays, bool on_device, hipStream_t stream) {
  const size_t n = (size_t)t->info.chunk_w * (size_t)t->info.chunk_h;
  MT_TRY(device_malloc((void **)&t->d_bad, 2 * sizeof(unsigned int), "the ray tree's count of refused rays"));
  RayTreeRaysArgs A{};
  A.ray = rays->ray; A.in_object = rays->in_object; A.coef = rays->coef;
  void *staged = nullptr;
  if (!on_device) {  // one allocation: the rays, the coefficients, the in_object bytes
    MT_TRY(device_malloc(&staged, n * 48 + n * 8 + n, "the caller's ray list"));
    char *at = (char *)staged;
    A.ray = (const double *)at;
    A.coef = rays->coef ? (const double *)(at + n * 48) : nullptr;
    A.in_object = rays->in_object ? (const uint8_t *)(at + n * 56) : nullptr;
  }
  const auto release = [&](int rc) {
    if (staged) (void)hipFree(staged);
    return rc;
  };
  if (!on_device) {
    if (hipMemcpyAsync((void *)A.ray, rays->ray, n * 48, hipMemcpyHostToDevice, stream) != hipSuccess ||
        (A.coef && hipMemcpyAsync((void *)A.coef, rays->coef, n * 8, hipMemcpyHostToDevice, stream) != hipSuccess) ||
        (A.in_object && hipMemcpyAsync((void *)A.in_object, rays->in_object, n, hipMemcpyHostToDevice, stream) != hipSuccess)) {
      return release(fail(MT_ERR_HIP, "copying the ray list to the device failed: %s", hipGetErrorString(hipGetLastError())));
    }
  }
  A.list_w = t->info.chunk_w; A.list_h = t->info.chunk_h;
  A.L = t->layer[0];
  A.bad = t->d_bad;
  unsigned int bad[2] = {0u, 0xffffffffu};
  hipError_t e = hipMemsetAsync(t->d_bad, 0, sizeof(unsigned int), stream);
  if (e == hipSuccess) e = hipMemsetAsync(t->d_bad + 1, 0xff, sizeof(unsigned int), stream);
  if (e == hipSuccess) e = launch_flat(raytree_rays_kernel, n, stream, A);
  if (e == hipSuccess) e = hipMemcpyAsync(bad, t->d_bad, sizeof bad, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return release(fail(MT_ERR_HIP, "importing the ray list failed: %s", hipGetErrorString(e)));
  if (bad[0] != 0) {
    return release(fail(MT_ERR_ARG, "%u rays of the list cannot be traced, the first at index %u", bad[0], bad[1]));
  }
  return release(MT_OK);
}

// raytree_trace_kernel over the n rays of L as rays of the tree's layer k (a layer of the tree, or a dense list of some of
// its rays), between that layer's two events
int launch_raytree_trace(mt_raytree *t, const RayTreeLayer &L, size_t n, int k, hipStream_t stream) {
  mt_scene *s = t->scene;
  RayTreeTraceArgs A{};
  A.L = L;
  A.n_rays = (uint32_t)n;
  A.n_items = (uint32_t)((n + 63) / 64);
  A.secondary = k > 0 ? 1 : 0;
  A.may_spawn = k < t->info.max_depth ? 1 : 0;
  unsigned grid = 0;
  MT_TRY(prepare_persistent_launch(s, A.n_items, &grid, stream));
  A.counters = s->d_counters;
  A.work_counter = s->d_gb_work;
  if (!t->ev_layer[k][0]) HIP_TRY(hipEventCreate(&t->ev_layer[k][0]));
  if (!t->ev_layer[k][1]) HIP_TRY(hipEventCreate(&t->ev_layer[k][1]));
  HIP_TRY(hipEventRecord(t->ev_layer[k][0], stream));
  hipLaunchKernelGGL(kernels_of(s->deep).raytree_trace[s->stats_enabled ? 1 : 0], dim3(grid), dim3(s->waves_per_block * 64),
                     s->lds_bytes, stream, s->dev, A);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(t->ev_layer[k][1], stream));
  return MT_OK;
}

// Layer after layer: trace, compact, (host: size the next layer), spawn.  Layer 0 comes from the tree's sensor, or from
// `rays` (a ray-list tree; on_device: its pointers are device pointers).
// a new tree of scene s with what the scene's switches and lights say now; the caller sets its geometry and depth
mt_raytree *raytree_new(mt_scene *s) {
  mt_raytree *t = new mt_raytree();
  t->scene = s;
  t->keep_uvw = s->raytree_uvw != 0;
  t->keep_tri = s->raytree_tri != 0;
  t->info.n_lights = s->dev.n_lights;
  t->geo_generation = s->geo_generation;
  return t;
}

// the tree's snapshot of what its planes are valid for: the scene's materials, textures and assignment as they are now
void raytree_snapshot(mt_raytree *t) {
  const mt_scene *s = t->scene;
  t->mtls = s->mtls_host;
  t->mtl_generation = s->mtl_generation;
  t->tex_generation = s->tex_generation;
  t->tri_mtl = s->tri_mtl_host;
  t->asg_generation = s->asg_generation;
  t->attr_generation[0] = s->attr_generation[0];
  t->attr_generation[1] = s->attr_generation[1];
}

int raytree_build(mt_raytree *t, const mt_ray_list *rays, bool on_device, mt_stats *stats) {
  mt_scene *s = t->scene;
  HostCall call(s, stats, t->ev0, t->ev1);
  const hipStream_t stream = call.stream;
  const mt_raytree_desc &I = t->info;
  const size_t npx = (size_t)I.chunk_w * (size_t)I.chunk_h;
  if (npx >= 0x80000000ull) return fail(MT_ERR_UNSUPPORTED, "layer 0 of the ray tree would have %zu rays (2^31 or more)", npx);
  HIP_TRY(hipEventCreate(&t->ev0));
  HIP_TRY(hipEventCreate(&t->ev1));
  MT_TRY(device_malloc((void **)&t->d_count, sizeof(unsigned long long), "the ray tree's child count"));
  MT_TRY(raytree_alloc_layer(t, 0, npx));
  MT_TRY(call.begin(true));
  if (rays) {
    MT_TRY(raytree_import_rays(t, rays, on_device, stream));
  } else {
    RayTreePrimaryArgs A{};
    A.sensor = t->sensor;
    A.chunk_x = I.chunk_x; A.chunk_y = I.chunk_y; A.chunk_w = I.chunk_w; A.chunk_h = I.chunk_h;
    A.L = t->layer[0];
    HIP_TRY(launch_flat(raytree_primary_kernel, npx, stream, A));
  }
  for (int k = 0;; k++) {
    const size_t n = (size_t)I.n_rays[k];
    MT_TRY(launch_raytree_trace(t, t->layer[k], n, k, stream));
    if (k == I.max_depth) {  // no ray of the deepest layer has a child
      HIP_TRY(hipMemsetAsync(t->layer[k].child_refl, 0xff, n * 4, stream));
      HIP_TRY(hipMemsetAsync(t->layer[k].child_refr, 0xff, n * 4, stream));
      break;
    }
    hipLaunchKernelGGL(raytree_compact_kernel, dim3(1), dim3(kRayTreeCompactThreads), 0, stream, t->layer[k], (uint32_t)n,
                       t->d_count);
    HIP_TRY(hipGetLastError());
    unsigned long long children = 0;
    HIP_TRY(hipMemcpyAsync(&children, t->d_count, sizeof children, hipMemcpyDeviceToHost, stream));
    MT_TRY(raytree_read_counters(s, stream));  // (synchronises: `children` has arrived)
    if (children == 0) break;
    if (children >= 0x80000000ull) {
      return fail(MT_ERR_UNSUPPORTED, "layer %d of the ray tree would have %llu rays (2^31 or more)", k + 1, children);
    }
    MT_TRY(raytree_alloc_layer(t, k + 1, (size_t)children));
    RayTreeSpawnArgs SA{};
    SA.parent = t->layer[k];
    SA.child = t->layer[k + 1];
    SA.n_parent = (uint32_t)n;
    SA.mtls = s->dev.mtls;
    HIP_TRY(launch_flat(raytree_spawn_kernel, n, stream, SA));
  }
  MT_TRY(call.mark_end());
  MT_TRY(raytree_read_counters(s, stream));  // (the last layer's status, checked before the counters are cleared)
  HIP_TRY(hipMemsetAsync(s->d_counters, 0, ST_COUNT * sizeof(unsigned long long), stream));
  for (int k = 0; k < I.n_layers; k++) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, t->ev_layer[k][0], t->ev_layer[k][1]));
    t->info.trace_ms[k] = ms;
  }
  raytree_snapshot(t);
  return call.report();
}

// raytree_shade_kernel over the layers, deepest first; d_rgb, d_color = device pointers, either may be nullptr: layer 0
// goes to the bitmap, or to its own colour plane and from there to d_color (raytree_color_kernel), or both
int launch_raytree_shade(mt_raytree *t, const mt_light *lights, int n_lights, uint8_t *d_rgb, double *d_color,
                         hipStream_t stream) {
  mt_scene *s = t->scene;
  RayTreeShadeArgs A{};
  A.n_lights = n_lights;
  A.mtls = s->dev.mtls;
  const bool in_args = n_lights <= kShadeArgLights;
  if (in_args) {
    for (int i = 0; i < n_lights; i++) A.lights[i] = lights[i];
  } else {
    MT_TRY(s->d_shade_lights.ensure((size_t)n_lights * sizeof(mt_light)));
    HIP_TRY(hipMemcpyAsync(s->d_shade_lights, lights, (size_t)n_lights * sizeof(mt_light), hipMemcpyHostToDevice, stream));
    A.d_lights = s->d_shade_lights;
  }
  void (*const shade)(RayTreeShadeArgs) = in_args ? raytree_shade_kernel<true> : raytree_shade_kernel<false>;
  for (int k = t->info.n_layers - 1; k >= 0; k--) {
    const size_t n = (size_t)t->info.n_rays[k];
    A.L = t->layer[k];
    A.child_color = k + 1 < t->info.n_layers ? t->layer[k + 1].color : nullptr;
    A.n_rays = (uint32_t)n;
    A.out_rgb = nullptr;
    if (k > 0 || d_color != nullptr) HIP_TRY(launch_flat(shade, n, stream, A));
    if (k == 0 && d_color != nullptr) {
      HIP_TRY(launch_flat(raytree_color_kernel, n, stream, (const double *)A.L.color, (const int32_t *)A.L.pixel,
                          (uint32_t)n, d_color));
    }
    if (k == 0 && d_rgb != nullptr) {
      A.out_rgb = d_rgb;
      HIP_TRY(launch_flat(shade, n, stream, A));
    }
  }
  return MT_OK;
}

}  // namespace

void mt_raytree_destroy(mt_raytree *t) {
  if (!t) return;
  (void)hipSetDevice(t->scene->device);
  (void)hipDeviceSynchronize();
  for (void *p : t->alloc) {
    if (p) (void)hipFree(p);
  }
  if (t->d_count) (void)hipFree(t->d_count);
  if (t->d_rgb) (void)hipFree(t->d_rgb);
  if (t->d_out_color) (void)hipFree(t->d_out_color);
  if (t->d_bad) (void)hipFree(t->d_bad);
  if (t->d_mismatch) (void)hipFree(t->d_mismatch);
  if (t->d_attr_count) (void)hipFree(t->d_attr_count);
  if (t->d_albedo_changed) (void)hipFree(t->d_albedo_changed);
  for (int32_t *p : t->d_src) {
    if (p) (void)hipFree(p);
  }
  if (t->d_regrow0) (void)hipFree(t->d_regrow0);
  if (t->d_tmp) (void)hipFree(t->d_tmp);
  if (t->ev0) (void)hipEventDestroy(t->ev0);
  if (t->ev1) (void)hipEventDestroy(t->ev1);
  for (auto &e : t->ev_layer) {
    if (e[0]) (void)hipEventDestroy(e[0]);
    if (e[1]) (void)hipEventDestroy(e[1]);
  }
  delete t;
}

mt_raytree *mt_raytree_create(mt_scene *s, const mt_sensor *sensor, int image_w, int image_h, int chunk_x, int chunk_y,
                              int chunk_w, int chunk_h, int max_depth, mt_stats *stats) {
  if (check_raytree_create_args(s, sensor, image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h, max_depth) != MT_OK) {
    return nullptr;
  }
  if (hipSetDevice(s->device) != hipSuccess) {
    (void)fail(MT_ERR_HIP, "hipSetDevice(%d) failed", s->device);
    return nullptr;
  }
  mt_raytree *t = raytree_new(s);
  t->sensor = *sensor;
  t->info.image_w = image_w; t->info.image_h = image_h;
  t->info.chunk_x = chunk_x; t->info.chunk_y = chunk_y; t->info.chunk_w = chunk_w; t->info.chunk_h = chunk_h;
  t->info.max_depth = max_depth;
  const int rc = raytree_build(t, nullptr, false, stats);
  if (rc != MT_OK) {
    const KeptError why;
    mt_raytree_destroy(t);
    (void)why.fail_again(rc);
    return nullptr;
  }
  return t;
}

namespace {

// *out = the tree, or nullptr with the error's code returned
int raytree_create_rays(mt_scene *s, const mt_ray_list *rays, int max_depth, mt_stats *stats, bool on_device,
                        mt_raytree **out) {
  *out = nullptr;
  MT_TRY(check_raytree_rays_args(s, rays, max_depth, !on_device));
  if (hipSetDevice(s->device) != hipSuccess) return fail(MT_ERR_HIP, "hipSetDevice(%d) failed", s->device);
  mt_raytree *t = raytree_new(s);
  t->info.image_w = t->info.chunk_w = rays->list_w;
  t->info.image_h = t->info.chunk_h = rays->list_h;
  t->info.max_depth = max_depth;
  t->info.from_rays = 1;
  const int rc = raytree_build(t, rays, on_device, stats);
  if (rc != MT_OK) {
    const KeptError why;
    mt_raytree_destroy(t);
    return why.fail_again(rc);
  }
  *out = t;
  return MT_OK;
}

}  // namespace

mt_raytree *mt_raytree_create_rays(mt_scene *s, const mt_ray_list *rays, int max_depth, mt_stats *stats) {
  mt_raytree *t = nullptr;
  (void)raytree_create_rays(s, rays, max_depth, stats, false, &t);
  return t;
}

mt_raytree *mt_raytree_create_rays_device(mt_scene *s, const mt_ray_list *d_rays, int max_depth, mt_stats *stats) {
  mt_raytree *t = nullptr;
  (void)raytree_create_rays(s, d_rays, max_depth, stats, true, &t);
  return t;
}

int mt_raytree_info(const mt_raytree *t, mt_raytree_desc *out) {
  if (!t) return fail(MT_ERR_ARG, "the ray tree is NULL");
  if (!out) return fail(MT_ERR_ARG, "the mt_raytree_desc is NULL");
  *out = t->info;
  return MT_OK;
}

int mt_raytree_read_layer(mt_raytree *t, int layer, const mt_raytree_layer *out) {
  if (!t) return fail(MT_ERR_ARG, "the ray tree is NULL");
  if (layer < 0 || layer >= t->info.n_layers) {
    return fail(MT_ERR_ARG, "layer %d outside the ray tree's %d layers", layer, t->info.n_layers);
  }
  if (!out) return fail(MT_ERR_ARG, "the mt_raytree_layer is NULL");
  if (out->pixel != nullptr && layer != 0) return fail(MT_ERR_ARG, "only layer 0 has a pixel plane");
  HIP_TRY(hipSetDevice(t->scene->device));
  const RayTreeLayer &L = t->layer[layer];
  const size_t n = (size_t)t->info.n_rays[layer], n_l = (size_t)t->info.n_lights;
  const PlaneCopy copies[] = {
      {out->ray, L.ray, n * 48}, {out->in_object, L.in_object, n}, {out->coef, L.coef, n * 8},
      {out->point, L.point, n * 24}, {out->normal, L.normal, n * 24}, {out->albedo, L.albedo, n * 24},
      {out->material, L.material, n * 4}, {out->power, L.power, n_l * n * 24}, {out->in_shadow, L.in_shadow, n_l * n},
      {out->child_refl, L.child_refl, n * 4}, {out->child_refr, L.child_refr, n * 4}, {out->pixel, L.pixel, n * 4}};
  for (const PlaneCopy &c : copies) {
    if (c.host != nullptr && c.bytes > 0) HIP_TRY(hipMemcpy(c.host, c.dev, c.bytes, hipMemcpyDeviceToHost));
  }
  return MT_OK;
}

int mt_raytree_keeps_uvw(const mt_raytree *t) {
  if (!t) return fail(MT_ERR_ARG, "the ray tree is NULL");
  return t->keep_uvw ? 1 : 0;
}

int mt_raytree_read_uvw(mt_raytree *t, int layer, double *out_uvw) {
  if (!t) return fail(MT_ERR_ARG, "the ray tree is NULL");
  if (layer < 0 || layer >= t->info.n_layers) {
    return fail(MT_ERR_ARG, "layer %d outside the ray tree's %d layers", layer, t->info.n_layers);
  }
  if (!out_uvw) return fail(MT_ERR_ARG, "the uvw output is NULL");
  if (!t->keep_uvw) {
    return fail(MT_ERR_ARG, "the ray tree keeps no uvw: it was made with mt_scene_set_raytree_uvw at 0");
  }
  HIP_TRY(hipSetDevice(t->scene->device));
  const size_t n = (size_t)t->info.n_rays[layer];
  if (n > 0) HIP_TRY(hipMemcpy(out_uvw, t->layer[layer].uvw, n * 24, hipMemcpyDeviceToHost));
  return MT_OK;
}

int mt_raytree_keeps_tri(const mt_raytree *t) {
  if (!t) return fail(MT_ERR_ARG, "the ray tree is NULL");
  return t->keep_tri ? 1 : 0;
}

int mt_raytree_read_tri(mt_raytree *t, int layer, int32_t *out_tri) {
  if (!t) return fail(MT_ERR_ARG, "the ray tree is NULL");
  if (layer < 0 || layer >= t->info.n_layers) {
    return fail(MT_ERR_ARG, "layer %d outside the ray tree's %d layers", layer, t->info.n_layers);
  }
  if (!out_tri) return fail(MT_ERR_ARG, "the tri output is NULL");
  if (!t->keep_tri) {
    return fail(MT_ERR_ARG, "the ray tree keeps no tri: it was made with mt_scene_set_raytree_tri at 0");
  }
  HIP_TRY(hipSetDevice(t->scene->device));
  const size_t n = (size_t)t->info.n_rays[layer];
  if (n > 0) HIP_TRY(hipMemcpy(out_tri, t->layer[layer].tri, n * 4, hipMemcpyDeviceToHost));
  return MT_OK;
}

int mt_raytree_shade_device(mt_raytree *t, const mt_light *lights, int n_lights, void *d_rgb, void *stream) {
  MT_TRY(check_raytree_shade_args(t, lights, n_lights, d_rgb));
  HIP_TRY(hipSetDevice(t->scene->device));
  return launch_raytree_shade(t, lights, n_lights, (uint8_t *)d_rgb, nullptr, (hipStream_t)stream);
}

int mt_raytree_shade_colors_device(mt_raytree *t, const mt_light *lights, int n_lights, void *d_color, void *stream) {
  MT_TRY(check_raytree_shade_args(t, lights, n_lights, d_color, "the output colours are NULL"));
  HIP_TRY(hipSetDevice(t->scene->device));
  return launch_raytree_shade(t, lights, n_lights, nullptr, (double *)d_color, (hipStream_t)stream);
}

namespace {

// the host forms of the shade: bytes, colours or both, whichever is not NULL
int raytree_shade_host(mt_raytree *t, const mt_light *lights, int n_lights, uint8_t *out_rgb, double *out_color,
                       mt_stats *stats) {
  HostCall call(t->scene, stats, t->ev0, t->ev1);
  HIP_TRY(hipSetDevice(t->scene->device));
  const size_t npx = (size_t)t->info.chunk_w * (size_t)t->info.chunk_h;
  const hipStream_t stream = call.stream;
  if (out_rgb && !t->d_rgb) MT_TRY(device_malloc((void **)&t->d_rgb, npx * 3, "the ray tree's bitmap"));
  if (out_color && !t->d_out_color) MT_TRY(device_malloc((void **)&t->d_out_color, npx * 24, "the ray tree's colours"));
  MT_TRY(call.begin(false));  // (no ray, no traversal: every work counter is zero)
  MT_TRY(launch_raytree_shade(t, lights, n_lights, out_rgb ? t->d_rgb : nullptr, out_color ? t->d_out_color : nullptr, stream));
  MT_TRY(call.mark_end());
  if (out_rgb) HIP_TRY(hipMemcpyAsync(out_rgb, t->d_rgb, npx * 3, hipMemcpyDeviceToHost, stream));
  if (out_color) HIP_TRY(hipMemcpyAsync(out_color, t->d_out_color, npx * 24, hipMemcpyDeviceToHost, stream));
  return call.close();
}

}  // namespace

int mt_raytree_shade_colors(mt_raytree *t, const mt_light *lights, int n_lights, double *out_color, mt_stats *stats) {
  MT_TRY(check_raytree_shade_args(t, lights, n_lights, out_color, "the output colours are NULL"));
  return raytree_shade_host(t, lights, n_lights, nullptr, out_color, stats);
}

int mt_raytree_shade(mt_raytree *t, const mt_light *lights, int n_lights, uint8_t *out_rgb, mt_stats *stats) {
  MT_TRY(check_raytree_shade_args(t, lights, n_lights, out_rgb));
  return raytree_shade_host(t, lights, n_lights, out_rgb, nullptr, stats);
}

int mt_trace_rays(mt_scene *s, const mt_ray_list *rays, int max_depth, double *out_color, uint8_t *out_rgb,
                  mt_stats *stats) {
  if (!out_color && !out_rgb) return fail(MT_ERR_ARG, "out_color and out_rgb are both NULL");
  const auto w0 = std::chrono::steady_clock::now();
  mt_stats made{};
  mt_raytree *t = nullptr;
  MT_TRY(raytree_create_rays(s, rays, max_depth, stats ? &made : nullptr, false, &t));
  const std::vector<mt_light> lights = s->lights_host;  // the scene's current lights
  mt_stats shaded{};
  const int rc = raytree_shade_host(t, lights.data(), (int)lights.size(), out_rgb, out_color, stats ? &shaded : nullptr);
  const KeptError why;
  mt_raytree_destroy(t);
  if (rc != MT_OK) return why.fail_again(rc);
  if (stats) {
    *stats = made;
    stats->kernel_ms = made.kernel_ms + shaded.kernel_ms;
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
  }
  return MT_OK;
}

int mt_raytree_update_lights_device(mt_raytree *t, const int32_t *light_idx, int n_idx, void *stream) {
  MT_TRY(check_raytree_update_args(t, light_idx, n_idx));
  HIP_TRY(hipSetDevice(t->scene->device));
  return launch_raytree_update(t, light_idx, n_idx, (hipStream_t)stream);
}

// The host form: the tree's planes are where they are; only the counters come back.
int mt_raytree_update_lights(mt_raytree *t, const int32_t *light_idx, int n_idx, mt_stats *stats) {
  MT_TRY(check_raytree_update_args(t, light_idx, n_idx));
  mt_scene *s = t->scene;
  HostCall call(s, stats, t->ev0, t->ev1);
  HIP_TRY(hipSetDevice(s->device));
  MT_TRY(call.begin(true));
  MT_TRY(launch_raytree_update(t, light_idx, n_idx, call.stream));
  MT_TRY(call.mark_end());
  MT_TRY(call.counters_home());
  return call.close();
}

namespace {

bool same_bits(const double *a, const double *b, int n) { return memcmp(a, b, (size_t)n * sizeof(double)) == 0; }

// what the edit from `was` to `now` asks of a stored tree
struct MaterialDiff {
  bool shape = false;    // a reflectance or transparency changed: the check pass
  bool shadow = false;   // a shadow ray may see the change: the light planes again
  bool albedo = false;   // some ambient changed
  int textured = -1;     // the first textured material whose ambient or tex changed
  std::vector<uint8_t> albedo_changed;
  // a pending reassignment (mt_scene_set_triangle_materials): the triangles whose material differs from the tree's
  // snapshot, the first of them, and the first whose NEW material has a texture (with that material)
  long long reassigned = 0;
  int first_reassigned = -1, textured_tri = -1, textured_tri_mtl = -1;
  // pending attribute edits (mt_scene_set_triangle_normals / _uvw): some triangle's stamp is newer than the tree's snapshot
  bool normals = false, uvws = false;
};

// the kernels' view of the pending attribute edits D of tree t (mt_raytree.h, RayTreeAttr)
RayTreeAttr raytree_attr_args(const mt_raytree *t, const MaterialDiff &D) {
  const mt_scene *s = t->scene;
  RayTreeAttr T{};
  if (D.normals) T.normal_stamp = s->d_attr_stamp[0];
  if (D.uvws) T.uvw_stamp = s->d_attr_stamp[1];
  T.normal_gen = t->attr_generation[0];
  T.uvw_gen = t->attr_generation[1];
  T.tri_vertex = s->dev.tri_vertex;
  T.tri_normal = s->dev.tri_normal;
  T.tri_uvw = s->dev.tri_uvw;
  T.count = t->d_attr_count;
  return T;
}

// raytree_reattr_kernel (or, check = true, raytree_attr_check_kernel) over the n rays of layer k
hipError_t launch_raytree_reattr(const mt_raytree *t, const MaterialDiff &D, const RayTreeLayer &L, size_t n, int k, bool check,
                                 hipStream_t stream) {
  RayTreeReattrArgs A{};
  A.L = L;
  A.attr = raytree_attr_args(t, D);
  A.mtls = t->scene->dev.mtls;
  A.texs = t->scene->dev.texs;
  A.n_rays = (uint32_t)n;
  A.layer = k;
  return launch_flat(check ? raytree_attr_check_kernel : raytree_reattr_kernel, n, stream, A);
}

// CHANGED of the assignment `was` -> `now`, and whether a shadow ray may see it: a = the old material under the tree's
// constants `mtls_was`, b = the new one under the scene's `mtls_now`
void diff_assignment(const std::vector<int32_t> &was, const std::vector<int32_t> &now, const std::vector<mt_material> &mtls_was,
                     const std::vector<mt_material> &mtls_now, MaterialDiff *out) {
  MaterialDiff &D = *out;
  for (size_t i = 0; i < now.size(); i++) {
    const int a = was[i], b = now[i];
    if (a == b) continue;
    if (D.reassigned++ == 0) D.first_reassigned = (int)i;
    if (b >= 0 && mtls_now[(size_t)b].tex >= 0 && D.textured_tri < 0) {
      D.textured_tri = (int)i;
      D.textured_tri_mtl = b;
    }
    if (a < 0 || b < 0) {  // a ray on it enters or leaves the light loop
      D.shadow = true;
      continue;
    }
    const mt_material &ma = mtls_was[(size_t)a], &mb = mtls_now[(size_t)b];
    const bool opaque = ma.transparency == 0.0 && mb.transparency == 0.0;  // (the shadow loop's own test)
    if (!same_bits(&ma.transparency, &mb.transparency, 1) ||
        (!opaque && !same_bits(ma.transmission_filter, mb.transmission_filter, 3))) {
      D.shadow = true;
    }
  }
  if (D.reassigned != 0) D.shape = true;  // the check pass decides
}

void diff_materials(const std::vector<mt_material> &was, const std::vector<mt_material> &now, MaterialDiff *out) {
  MaterialDiff &D = *out;
  D.albedo_changed.assign(now.size(), 0);
  for (size_t i = 0; i < now.size(); i++) {
    const mt_material &a = was[i], &b = now[i];
    if (!same_bits(a.ambient, b.ambient, 3) || a.tex != b.tex) {
      D.albedo = true;
      D.albedo_changed[i] = 1;
      if ((a.tex >= 0 || b.tex >= 0) && D.textured < 0) D.textured = (int)i;
    }
    const bool refl = !same_bits(&a.reflectance, &b.reflectance, 1);
    const bool tr = !same_bits(&a.transparency, &b.transparency, 1);
    if (refl || tr) D.shape = true;
    const bool opaque = a.transparency == 0.0 && b.transparency == 0.0;  // (the shadow loop's own test)
    if (tr || (!same_bits(a.transmission_filter, b.transmission_filter, 3) && !opaque)) D.shadow = true;
  }
}

// scratch of a tree that only grows: at least `bytes` at *p
int raytree_scratch(void **p, size_t *cap, size_t bytes, const char *what) {
  if (*p != nullptr && *cap >= bytes) return MT_OK;
  if (*p != nullptr) {
    (void)hipFree(*p);  // (waits for whatever still reads it)
    *p = nullptr;
    *cap = 0;
  }
  MT_TRY(device_malloc(p, bytes, what));
  *cap = bytes;
  return MT_OK;
}

// D.albedo_changed in the tree's byte per material on the device (made on first use)
int raytree_upload_albedo_changed(mt_raytree *t, const MaterialDiff &D, hipStream_t stream) {
  const size_t n_mtl = (size_t)t->scene->n_materials;
  if (!t->d_albedo_changed) {
    MT_TRY(device_malloc((void **)&t->d_albedo_changed, n_mtl, "the ray tree's material flags"));
  }
  HIP_TRY(hipMemcpyAsync(t->d_albedo_changed, D.albedo_changed.data(), n_mtl, hipMemcpyHostToDevice, stream));
  return MT_OK;
}

// raytree_recommit_kernel's arguments for the n rays of layer L under the edit D
RayTreeRecommitArgs raytree_recommit_args(const mt_raytree *t, const MaterialDiff &D, const RayTreeLayer &L, size_t n,
                                          int copy_coef) {
  const mt_scene *s = t->scene;
  RayTreeRecommitArgs A{};
  A.L = L;
  A.mtls = s->dev.mtls;
  A.texs = s->dev.texs;
  A.albedo_changed = D.albedo ? t->d_albedo_changed : nullptr;
  A.tri_mtl = D.reassigned != 0 ? s->dev.tri_mtl : nullptr;
  A.n_rays = (uint32_t)n;
  A.n_materials = s->n_materials;
  A.copy_coef = copy_coef;
  return A;
}

// mt_raytree_regrow_materials after a check pass that found mismatches: the new tree under the scene's current
// materials, built layer by layer next to the old one (mt_raytree.h, "edited materials that change the tree's shape"),
// then swapped in.  Until the swap only scratch and the new allocations are written: a failure before it leaves every
// plane of the tree as it was.  The scene's counters are zero at entry (HostCall::clear_counters) and hold the tracing
// launches' sums at exit.
int raytree_regrow(mt_raytree *t, const MaterialDiff &D, mt_raytree_regrow_info *info, hipStream_t stream) {
  mt_scene *s = t->scene;
  mt_raytree_desc &I = t->info;
  const int n_mtl = s->n_materials;
  const size_t n_l = (size_t)I.n_lights;
  const int old_layers = I.n_layers;
  // a pending reassignment: layer 0's material plane waits for the commit, the copy kernel restates the kept rays'
  const int32_t *tri_mtl_now = D.reassigned != 0 ? s->dev.tri_mtl : nullptr;
  // pending attribute edits: the link kernel respawns the reflected children of kept normal-dirty parents, the copy
  // kernel restates the kept rays' planes, layer 0's wait for the commit
  const RayTreeAttr attr = raytree_attr_args(t, D);
  void *alloc[MT_MAX_RECURSION + 1] = {};  // the new layers >= 1, aside
  RayTreeLayer NL[MT_MAX_RECURSION + 1] = {};
  size_t n_new[MT_MAX_RECURSION + 1] = {}, n_traced[MT_MAX_RECURSION + 1] = {};
  const auto release = [&](int rc) {
    for (void *p : alloc) {
      if (p) (void)hipFree(p);
    }
    return rc;
  };
  // layer 0 stays where it is; its child indices and spawn bytes are built in scratch and its albedo waits for the commit
  const size_t n0 = (size_t)I.n_rays[0];
  const size_t idx_bytes = (n0 * 4 + 255) & ~(size_t)255;
  MT_TRY(raytree_scratch(&t->d_regrow0, &t->regrow0_cap, 2 * idx_bytes + n0, "the ray tree's regrow scratch of layer 0"));
  NL[0] = t->layer[0];
  NL[0].child_refl = (int32_t *)t->d_regrow0;
  NL[0].child_refr = (int32_t *)((char *)t->d_regrow0 + idx_bytes);
  NL[0].spawn = (uint8_t *)t->d_regrow0 + 2 * idx_bytes;
  n_new[0] = n0;
  if (D.albedo) MT_TRY(raytree_upload_albedo_changed(t, D, stream));
  int new_layers = 0;
  for (int k = 0;; k++) {
    const size_t n = n_new[k];
    const int32_t *src = k == 0 ? nullptr : t->d_src[k & 1];
    {
      RayTreeRegrowFlagsArgs A{};
      A.L = NL[k];
      A.src = src;
      A.mtls = s->dev.mtls;
      A.tri_mtl = k == 0 ? tri_mtl_now : nullptr;
      A.n_rays = (uint32_t)n;
      A.n_materials = n_mtl;
      A.may_spawn = k < I.max_depth ? 1 : 0;
      if (launch_flat(raytree_regrow_flags_kernel, n, stream, A) != hipSuccess) {
        return release(fail(MT_ERR_HIP, "launching the regrow's flags kernel failed"));
      }
    }
    new_layers = k + 1;
    if (k == I.max_depth) {  // no ray of the deepest layer has a child
      if (hipMemsetAsync(NL[k].child_refl, 0xff, n * 4, stream) != hipSuccess ||
          hipMemsetAsync(NL[k].child_refr, 0xff, n * 4, stream) != hipSuccess) {
        return release(fail(MT_ERR_HIP, "clearing the deepest layer's child indices failed"));
      }
      break;
    }
    hipLaunchKernelGGL(raytree_compact_kernel, dim3(1), dim3(kRayTreeCompactThreads), 0, stream, NL[k], (uint32_t)n,
                       t->d_count);
    unsigned long long children = 0;
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(&children, t->d_count, sizeof children, hipMemcpyDeviceToHost, stream) != hipSuccess) {
      return release(fail(MT_ERR_HIP, "the regrow's compaction of layer %d failed", k));
    }
    // (synchronises: `children` has arrived; a tripped bound in layer k's tracing launch ends the call here)
    if (const int rc = raytree_read_counters(s, stream)) return release(rc);
    if (children == 0) break;
    if (children >= 0x80000000ull) {
      return release(fail(MT_ERR_UNSUPPORTED, "layer %d of the ray tree would have %llu rays (2^31 or more)", k + 1, children));
    }
    const size_t n1 = (size_t)children;
    n_new[k + 1] = n1;
    const size_t total = raytree_carve_layer(nullptr, n_l, k + 1, n1, t->keep_uvw, t->keep_tri, &NL[k + 1]);
    char what[64];
    snprintf(what, sizeof what, "layer %d of the ray tree (%zu rays)", k + 1, n1);
    if (const int rc = device_malloc(&alloc[k + 1], total, what)) return release(rc);
    (void)raytree_carve_layer(alloc[k + 1], n_l, k + 1, n1, t->keep_uvw, t->keep_tri, &NL[k + 1]);
    const int to = (k + 1) & 1;
    if (const int rc = raytree_scratch((void **)&t->d_src[to], &t->src_cap[to], n1 * 4, "the ray tree's regrow indices")) {
      return release(rc);
    }
    {
      RayTreeRegrowLinkArgs A{};
      A.parent = NL[k];
      A.child = NL[k + 1];
      A.parent_src = src;
      // (past the old tree's last layer every parent is a traced ray: src < 0, the old indices are not read)
      A.old_child_refl = k < old_layers ? t->layer[k].child_refl : nullptr;
      A.old_child_refr = k < old_layers ? t->layer[k].child_refr : nullptr;
      A.child_src = t->d_src[to];
      A.mtls = s->dev.mtls;
      A.tri_mtl = k == 0 ? tri_mtl_now : nullptr;
      A.n_parent = (uint32_t)n;
      A.attr = attr;
      if (launch_flat(raytree_regrow_link_kernel, n, stream, A) != hipSuccess) {
        return release(fail(MT_ERR_HIP, "launching the regrow's link kernel failed"));
      }
    }
    if (k + 1 < old_layers) {  // (else no ray of layer k + 1 has an old index)
      RayTreeRegrowCopyArgs A{};
      A.from = t->layer[k + 1];
      A.to = NL[k + 1];
      A.src = t->d_src[to];
      A.n_from = (uint32_t)I.n_rays[k + 1];
      A.n_to = (uint32_t)n1;
      A.n_lights = I.n_lights;
      A.n_materials = n_mtl;
      A.mtls = s->dev.mtls;
      A.texs = s->dev.texs;
      A.albedo_changed = D.albedo ? t->d_albedo_changed : nullptr;
      A.tri_mtl = tri_mtl_now;
      A.attr = attr;
      if (launch_flat(raytree_regrow_copy_kernel, n1, stream, A) != hipSuccess) {
        return release(fail(MT_ERR_HIP, "launching the regrow's copy kernel failed"));
      }
    }
    // the traced rays of layer k + 1: the link kernel left 1 in their spawn bytes, so the layer's own compaction gives
    // their places in the dense list (child_refl) and their number
    hipLaunchKernelGGL(raytree_compact_kernel, dim3(1), dim3(kRayTreeCompactThreads), 0, stream, NL[k + 1], (uint32_t)n1,
                       t->d_count);
    unsigned long long listed = 0;
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(&listed, t->d_count, sizeof listed, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) {
      return release(fail(MT_ERR_HIP, "listing the traced rays of layer %d failed", k + 1));
    }
    const size_t m = (size_t)listed;  // (<= n1 < 2^31)
    n_traced[k + 1] = m;
    if (m == 0) continue;
    RayTreeRegrowListArgs A{};
    const size_t tmp_bytes = raytree_carve_layer(nullptr, n_l, k + 1, m, t->keep_uvw, t->keep_tri, &A.tmp);
    if (const int rc = raytree_scratch(&t->d_tmp, &t->tmp_cap, tmp_bytes, "the ray tree's list of traced rays")) {
      return release(rc);
    }
    (void)raytree_carve_layer(t->d_tmp, n_l, k + 1, m, t->keep_uvw, t->keep_tri, &A.tmp);
    A.L = NL[k + 1];
    A.n_rays = (uint32_t)n1;
    A.n_list = (uint32_t)m;
    A.n_lights = I.n_lights;
    if (launch_flat(raytree_regrow_gather_kernel, n1, stream, A) != hipSuccess) {
      return release(fail(MT_ERR_HIP, "launching the regrow's gather kernel failed"));
    }
    if (const int rc = launch_raytree_trace(t, A.tmp, m, k + 1, stream)) return release(rc);
    if (launch_flat(raytree_regrow_scatter_kernel, n1, stream, A) != hipSuccess) {
      return release(fail(MT_ERR_HIP, "launching the regrow's scatter kernel failed"));
    }
  }
  // the last tracing launch's status; nothing of the old tree has been written so far, and nothing below fails for size
  if (const int rc = raytree_read_counters(s, stream)) return release(rc);
  // ---- the commit: layer 0 in place, the layers below swapped
  if (hipMemcpyAsync(t->layer[0].child_refl, NL[0].child_refl, n0 * 4, hipMemcpyDeviceToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(t->layer[0].child_refr, NL[0].child_refr, n0 * 4, hipMemcpyDeviceToDevice, stream) != hipSuccess) {
    return release(fail(MT_ERR_HIP, "writing layer 0's child indices failed"));
  }
  if (D.albedo || tri_mtl_now != nullptr) {
    if (launch_flat(raytree_recommit_kernel, n0, stream, raytree_recommit_args(t, D, t->layer[0], n0, 0)) != hipSuccess) {
      return release(fail(MT_ERR_HIP, "launching layer 0's commit failed"));
    }
  }
  if ((D.normals || D.uvws) && launch_raytree_reattr(t, D, t->layer[0], n0, 0, false, stream) != hipSuccess) {
    return release(fail(MT_ERR_HIP, "launching layer 0's attribute commit failed"));
  }
  if (hipStreamSynchronize(stream) != hipSuccess) return release(fail(MT_ERR_HIP, "the regrow's commit failed"));
  if (info) {
    info->regrown = 1;
    info->n_layers_before = old_layers;
    info->n_layers_after = new_layers;
    for (int k = 0; k <= MT_MAX_RECURSION; k++) {
      info->traced[k] = (int64_t)n_traced[k];
      info->kept[k] = (int64_t)(n_new[k] - n_traced[k]);
      info->dropped[k] = I.n_rays[k] - info->kept[k];  // (0 from the old tree's last layer on)
    }
  }
  RayTreeLayer none{};
  for (int k = 1; k <= MT_MAX_RECURSION; k++) {
    if (t->alloc[k]) {
      I.bytes -= raytree_carve_layer(nullptr, n_l, k, (size_t)I.n_rays[k], t->keep_uvw, t->keep_tri, &none);
      (void)hipFree(t->alloc[k]);
    }
    t->alloc[k] = alloc[k];
    t->layer[k] = NL[k];
    I.n_rays[k] = (int64_t)n_new[k];
    if (alloc[k]) I.bytes += raytree_carve_layer(nullptr, n_l, k, n_new[k], t->keep_uvw, t->keep_tri, &none);
  }
  I.n_layers = new_layers;
  for (int k = 0; k <= MT_MAX_RECURSION; k++) {
    float ms = 0;
    if (n_traced[k] != 0) HIP_TRY(hipEventElapsedTime(&ms, t->ev_layer[k][0], t->ev_layer[k][1]));
    I.trace_ms[k] = ms;
  }
  return MT_OK;
}

// What the scene's edits since the tree's snapshot ask of the tree (*out), or why the tree cannot take them
int raytree_diff(const mt_raytree *t, MaterialDiff *out) {
  const mt_scene *s = t->scene;
  MaterialDiff &D = *out;
  diff_materials(t->mtls, s->mtls_host, &D);
  if (D.textured >= 0 && !t->keep_uvw) {
    return fail(MT_ERR_UNSUPPORTED, "material %d has a texture and its ambient or tex changed: the ray tree keeps neither "
                                    "the texel nor the primitive, a new tree is needed", D.textured);
  }
  // a texture set since the snapshot: the materials that use it NOW are retextured (one that used it and left it has a
  // changed `tex`: diff_materials has it; one that no material uses is nothing to do)
  for (size_t i = 0; i < s->mtls_host.size(); i++) {
    const int tex = s->mtls_host[i].tex;
    if (tex < 0 || t->tex_generation[(size_t)tex] == s->tex_generation[(size_t)tex]) continue;
    if (!t->keep_uvw) {
      return fail(MT_ERR_UNSUPPORTED, "texture %d was set after the ray tree was made and material %d uses it: the ray "
                                      "tree keeps no uvw (mt_scene_set_raytree_uvw), a new tree is needed", tex, (int)i);
    }
    D.albedo = true;
    D.albedo_changed[i] = 1;
  }
  // a reassignment since the snapshot (A -> B -> A is none)
  if (t->asg_generation != s->asg_generation && t->tri_mtl != s->tri_mtl_host) {
    diff_assignment(*t->tri_mtl, *s->tri_mtl_host, t->mtls, s->mtls_host, &D);
  }
  if (D.reassigned != 0 && !t->keep_tri) {
    return fail(MT_ERR_UNSUPPORTED, "%lld triangles were given another material after the ray tree was made, the first is "
                                    "triangle %d: the ray tree keeps no tri (mt_scene_set_raytree_tri), a new tree is needed",
                D.reassigned, D.first_reassigned);
  }
  if (D.textured_tri >= 0 && !t->keep_uvw) {
    return fail(MT_ERR_UNSUPPORTED, "triangle %d was given material %d, which has a texture: the ray tree keeps no uvw "
                                    "(mt_scene_set_raytree_uvw), a new tree is needed", D.textured_tri, D.textured_tri_mtl);
  }
  // an attribute set since the snapshot: the generation moves only with a changed triangle, so some stamp is newer
  for (int w = 0; w < 2; w++) {
    if (t->attr_generation[w] == s->attr_generation[w]) continue;
    if (!t->keep_tri) {
      long long stamped = 0, first = -1;
      const std::vector<uint32_t> &stamp = s->attr_stamp_host[w];
      for (size_t i = 0; i < stamp.size(); i++) {
        if (stamp[i] > t->attr_generation[w] && stamped++ == 0) first = (long long)i;
      }
      return fail(MT_ERR_UNSUPPORTED, "the %s of %lld triangles was set after the ray tree was made, the first is triangle "
                                      "%lld: the ray tree keeps no tri (mt_scene_set_raytree_tri), a new tree is needed",
                  kAttrName[w], stamped, first);
    }
    (w == 0 ? D.normals : D.uvws) = true;
  }
  return MT_OK;
}

// The attribute part of the check pass: raytree_attr_check_kernel over every layer counts the normal-dirty rays that
// have a reflected child: found[0] of them, the first at layer found[1] >> 32, ray found[1] & 0xffffffff.  Synchronises.
int raytree_attr_check_pass(mt_raytree *t, const MaterialDiff &D, hipStream_t stream, unsigned long long found[2]) {
  const mt_raytree_desc &I = t->info;
  for (int k = 0; k < I.n_layers; k++) {
    HIP_TRY(launch_raytree_reattr(t, D, t->layer[k], (size_t)I.n_rays[k], k, true, stream));
  }
  found[0] = found[1] = 0;
  HIP_TRY(hipMemcpyAsync(found, t->d_attr_count + kRayTreeAttrBlocked, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return MT_OK;
}

// The check pass: raytree_recoef_kernel over every layer restates the rays' coefficients under the scene's current
// materials (aside, in the next layer's colour plane) and counts the rays that would spawn other children: found[0]
// of them, the first at layer found[1] >> 32, ray found[1] & 0xffffffff.  Synchronises.
int raytree_check_pass(mt_raytree *t, const MaterialDiff &D, hipStream_t stream, unsigned long long found[2]) {
  const mt_scene *s = t->scene;
  const mt_raytree_desc &I = t->info;
  if (!t->d_mismatch) {
    MT_TRY(device_malloc((void **)&t->d_mismatch, 2 * sizeof(unsigned long long), "the ray tree's mismatch count"));
  }
  HIP_TRY(hipMemsetAsync(t->d_mismatch, 0, sizeof(unsigned long long), stream));
  HIP_TRY(hipMemsetAsync(t->d_mismatch + 1, 0xff, sizeof(unsigned long long), stream));
  for (int k = 0; k < I.n_layers; k++) {
    const size_t n = (size_t)I.n_rays[k];
    RayTreeRecoefArgs A{};
    A.L = t->layer[k];
    A.child_scratch = k + 1 < I.n_layers ? t->layer[k + 1].color : nullptr;
    A.mtls = s->dev.mtls;
    A.tri_mtl = D.reassigned != 0 ? s->dev.tri_mtl : nullptr;
    A.n_rays = (uint32_t)n;
    A.n_materials = s->n_materials;
    A.layer = k;
    A.may_spawn = k < I.max_depth ? 1 : 0;
    A.mismatch = t->d_mismatch;
    HIP_TRY(launch_flat(raytree_recoef_kernel, n, stream, A));
  }
  found[0] = found[1] = 0;
  HIP_TRY(hipMemcpyAsync(found, t->d_mismatch, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return MT_OK;
}

// The commit of a tree that keeps its shape: raytree_recommit_kernel over the layers the edit touches
int raytree_commit(mt_raytree *t, const MaterialDiff &D, hipStream_t stream) {
  const mt_raytree_desc &I = t->info;
  if (D.albedo) MT_TRY(raytree_upload_albedo_changed(t, D, stream));
  for (int k = 0; k < I.n_layers; k++) {
    const size_t n = (size_t)I.n_rays[k];
    const RayTreeRecommitArgs A = raytree_recommit_args(t, D, t->layer[k], n, D.shape && k > 0 ? 1 : 0);
    if (!A.copy_coef && !A.albedo_changed && !A.tri_mtl) continue;
    HIP_TRY(launch_flat(raytree_recommit_kernel, n, stream, A));
  }
  // the dirty rays' normal, uvw and albedo, behind the materials' commit: the material plane is the effective one
  if (D.normals || D.uvws) {
    for (int k = 0; k < I.n_layers; k++) {
      HIP_TRY(launch_raytree_reattr(t, D, t->layer[k], (size_t)I.n_rays[k], k, false, stream));
    }
  }
  return MT_OK;
}

// mt_raytree_update_materials, and mt_raytree_regrow_materials when `regrow` is set: the two calls differ in the light
// count check and in what a check pass with mismatches leads to.
int raytree_take_materials(mt_raytree *t, mt_stats *stats, bool regrow, mt_raytree_regrow_info *info) {
  if (!t) return fail(MT_ERR_ARG, "the ray tree is NULL");
  mt_scene *s = t->scene;
  HostCall call(s, stats, t->ev0, t->ev1);
  const mt_raytree_desc &I = t->info;
  if (stats) memset(stats, 0, sizeof *stats);
  if (info) {
    memset(info, 0, sizeof *info);
    info->n_layers_before = info->n_layers_after = I.n_layers;
  }
  MT_TRY(check_raytree_geometry(t));
  t->attr_last = mt_raytree_attr_info{};
  if (t->mtl_generation == s->mtl_generation) return MT_OK;
  // ---- 1. the edit, and the edits this tree cannot take
  MaterialDiff D;
  MT_TRY(raytree_diff(t, &D));
  const bool attrs = D.normals || D.uvws;
  // ---- 2. the lights the tracing launches would read
  const bool retrace = D.shadow && I.n_lights > 0;
  // (a regrow may trace new rays, whose light planes come from the scene's current lights)
  const bool lights_read = regrow ? (D.shape || D.shadow || D.normals) && I.n_lights > 0 : retrace;
  if (lights_read && s->dev.n_lights != I.n_lights) {
    return fail(MT_ERR_ARG, "the scene has %d lights, the ray tree was made with %d", s->dev.n_lights, I.n_lights);
  }
  bool regrown = false;
  unsigned long long attr_count[kRayTreeAttrWords] = {};
  if (D.shape || D.albedo || retrace || attrs) {
    HIP_TRY(hipSetDevice(s->device));
    const hipStream_t stream = call.stream;
    if (attrs) {
      if (!t->d_attr_count) {
        MT_TRY(device_malloc((void **)&t->d_attr_count, sizeof attr_count, "the ray tree's attribute counts"));
      }
      HIP_TRY(hipMemsetAsync(t->d_attr_count, 0, sizeof attr_count, stream));
      HIP_TRY(hipMemsetAsync(t->d_attr_count + kRayTreeAttrFirst, 0xff, sizeof(unsigned long long), stream));
    }
    MT_TRY(call.begin(false));  // (the counters are cleared where a tracing launch follows)
    // ---- 3. the check pass
    if (D.shape || D.normals) {
      unsigned long long found[2] = {0, 0}, blocked[2] = {0, 0};
      if (D.shape) MT_TRY(raytree_check_pass(t, D, stream, found));
      if (D.normals) MT_TRY(raytree_attr_check_pass(t, D, stream, blocked));
      if (found[0] != 0 && !regrow) {
        return fail(MT_ERR_UNSUPPORTED, "the new materials change the shape of the ray tree: %llu rays spawn other "
                                        "children, the first in layer %d at ray %llu; a new tree is needed",
                    found[0], (int)(found[1] >> 32), found[1] & 0xffffffffull);
      }
      if (blocked[0] != 0 && !regrow) {
        return fail(MT_ERR_UNSUPPORTED, "the new normals move reflected rays of the ray tree: %llu rays on edited triangles "
                                        "have a reflected child, the first in layer %d at ray %llu; "
                                        "mt_raytree_regrow_materials or a new tree is needed",
                    blocked[0], (int)(blocked[1] >> 32), blocked[1] & 0xffffffffull);
      }
      if (found[0] != 0 || blocked[0] != 0) {
        // (only a tree of zero lights gets here with another count: the tracing kernel runs the SCENE's lights' loops,
        // and the new layers have planes for the tree's)
        if (s->dev.n_lights != I.n_lights) {
          return fail(MT_ERR_ARG, "the scene has %d lights, the ray tree was made with %d", s->dev.n_lights, I.n_lights);
        }
        // ---- 4a. the regrow, whose tracing launches count from zero
        MT_TRY(call.clear_counters());
        MT_TRY(raytree_regrow(t, D, info, stream));
        regrown = true;
      }
    }
    // ---- 4b. or the commit of a tree that keeps its shape (a regrown tree has taken everything already)
    if (!regrown) MT_TRY(raytree_commit(t, D, stream));
    // ---- 5. the light planes again, and the way back
    if (retrace) {
      if (!regrown) MT_TRY(call.clear_counters());  // (a regrown tree's tracing launches have counted already)
      std::vector<int32_t> all((size_t)I.n_lights);
      for (int i = 0; i < I.n_lights; i++) all[(size_t)i] = i;
      MT_TRY(launch_raytree_update(t, all.data(), I.n_lights, stream));
    }
    MT_TRY(call.mark_end());
    if (call.counters) MT_TRY(call.counters_home());
    if (attrs) {
      HIP_TRY(hipMemcpyAsync(attr_count, t->d_attr_count, sizeof attr_count, hipMemcpyDeviceToHost, stream));
    }
  }
  if (!regrown && info) {
    for (int k = 0; k < I.n_layers; k++) info->kept[k] = I.n_rays[k];
  }
  MT_TRY(call.close());
  t->attr_last.renormaled = (int64_t)attr_count[kRayTreeAttrNormal];
  t->attr_last.reuvwed = (int64_t)attr_count[kRayTreeAttrUVW];
  t->attr_last.respawned = (int64_t)attr_count[kRayTreeAttrRespawned];
  raytree_snapshot(t);
  return MT_OK;
}

}  // namespace

int mt_raytree_update_materials(mt_raytree *t, mt_stats *stats) { return raytree_take_materials(t, stats, false, nullptr); }

int mt_raytree_regrow_materials(mt_raytree *t, mt_raytree_regrow_info *info, mt_stats *stats) {
  return raytree_take_materials(t, stats, true, info);
}

int mt_raytree_attr_info_last(const mt_raytree *t, mt_raytree_attr_info *out) {
  if (!t) return fail(MT_ERR_ARG, "the ray tree is NULL");
  if (!out) return fail(MT_ERR_ARG, "the mt_raytree_attr_info is NULL");
  *out = t->attr_last;
  return MT_OK;
}

// ---- one frame on several GPUs of this process (main_net_master.cc:195-236) --------------------------
// Replica r renders ITS tiles -- dealt out by cost, see mt_order_tiles_device; by tile number while no frame of this
// geometry has been measured -- into its own tile buffer on its own device and stream (the launches are made from one
// host thread per replica, so that no device waits for another's launch calls); the first replica's stream then waits
// for each replica's event, pulls its buffer over xGMI (hipMemcpyPeerAsync; the buffers of replicas on the SAME device
// are read in place) and blits it into the frame; one D2H copy ends the call.
int mt_render_frame_multi(mt_scene *const *scenes, int n, const mt_sensor *sensor, int image_w, int image_h,
                          int tile_w, int tile_h, int max_depth, uint8_t *out_rgb, mt_stats *stats) {
  if (!scenes || n < 1 || n > 1024) return fail(MT_ERR_ARG, "bad scene list");
  for (int r = 0; r < n; r++) {
    if (!scenes[r]) return fail(MT_ERR_ARG, "scenes[%d] is NULL", r);
    for (int q = 0; q < r; q++) {
      if (scenes[q] == scenes[r]) return fail(MT_ERR_ARG, "scenes[%d] and scenes[%d] are the same replica", q, r);
    }
  }
  if (!out_rgb) return fail(MT_ERR_ARG, "out_rgb is NULL");
  int rc = check_image_args(scenes[0], sensor, image_w, image_h);
  if (rc != MT_OK) return rc;
  if (tile_w <= 0 || tile_h <= 0) return fail(MT_ERR_ARG, "bad tile size");
  const auto w0 = std::chrono::steady_clock::now();
  const long long tiles_total_ll = tile_count(image_w, image_h, tile_w, tile_h);
  if (tiles_total_ll > (1ll << 20)) return fail(MT_ERR_ARG, "too many tiles (%lld)", tiles_total_ll);
  const int tiles_total = (int)tiles_total_ll;
  const size_t slot = (size_t)tile_w * tile_h * 3;
  const int n_max = (tiles_total + n - 1) / n;
  auto tiles_of = [&](int r) -> int { return dealt_tile_count(tiles_total, n, r); };
  mt_scene *root = scenes[0];
  // the replicas' block costs are exchanged after every frame (mt_scene_export_costs_device: a moving camera's next
  // frame is ordered by the costs of ALL tiles of this one, and the tiles are dealt out by them)
  const bool share_costs = n > 1 && (tile_w & 7) == 0 && (tile_h & 7) == 0;
  const int map_w = (image_w + 7) / 8, map_h = (image_h + 7) / 8;
  const size_t map_bytes = (size_t)map_w * map_h * sizeof(unsigned);

  // ---- who renders what.  State of the previous call (kept on every replica, decided on the first one's): the same
  // geometry and replica list?  Then the tiles are dealt out anew by the combined costs of the previous frame -- every
  // replica holds that map and orders it by itself -- unless the camera has been at rest for two frames: from then on
  // the assignment is kept, and with it the per-slot cost history (running means, the blocks' two measured forms).
  const unsigned long long geom = fnv1a({image_w, image_h, tile_w, tile_h, max_depth, n});
  bool same_geom = true;
  for (int r = 0; r < n; r++) {
    same_geom = same_geom && scenes[r]->multi_geom == geom && scenes[r]->multi_rank == r &&
                scenes[r]->multi_list_id == root->multi_list_id;
  }
  const bool balance = share_costs && root->tune.v[MT_TUNE_MULTI_BALANCE] != 0.0;
  const bool at_rest = same_geom && memcmp(&root->multi_sensor, sensor, sizeof(mt_sensor)) == 0;
  const int frames_at_rest = at_rest ? root->multi_frames_at_rest + 1 : 0;
  const bool by_map = same_geom && balance && root->multi_have_map && (!at_rest || frames_at_rest < 2);
  const bool redeal = !same_geom || by_map;
  static std::atomic<unsigned long long> next_list_id{1};
  const unsigned long long list_id = redeal ? next_list_id.fetch_add(1) : root->multi_list_id;
  // the one exit of a failure: let whatever was launched finish before the caller touches its buffers or the scenes
  // again, forget the state of the previous call, report
  auto failed = [&](int code, const std::string &text) -> int {
    for (int q = 0; q < n; q++) {
      if (scenes[q]->multi_stream) {
        (void)hipSetDevice(scenes[q]->device);
        (void)hipStreamSynchronize(scenes[q]->multi_stream);
      }
      scenes[q]->multi_geom = 0;
    }
    (void)hipSetDevice(root->device);
    return fail(code, "%s", text.c_str());
  };
  // copy between replicas: over xGMI where the devices differ (or MULTI_FORCE_PEER_COPY), else on the device
  const bool force_peer = root->tune.v[MT_TUNE_MULTI_FORCE_PEER_COPY] != 0.0;
  auto copy = [&](void *dst, int dst_device, const void *src, int src_device, size_t bytes, hipStream_t stream) -> int {
    if (dst_device != src_device || force_peer) HIP_TRY(hipMemcpyPeerAsync(dst, dst_device, src, src_device, bytes, stream));
    else HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream));
    return MT_OK;
  };

  // ---- phase 1: every replica renders its tiles
  std::vector<int> rcs((size_t)n, MT_OK);
  std::vector<std::string> errs((size_t)n);
  auto launch_one = [&](int r) {
    mt_scene *s = scenes[r];
    auto body = [&]() -> int {
      HIP_TRY(hipSetDevice(s->device));
      if (!s->multi_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&s->multi_stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&s->multi_done, hipEventDisableTiming));
      }
      MT_TRY(s->d_multi_tiles.ensure((size_t)n_max * slot));
      MT_TRY(s->d_multi_list.ensure((size_t)n_max * 4));
      int rc2;
      if (redeal) {
        const int32_t *order = nullptr;
        if (by_map) {
          MT_TRY(s->d_multi_order.ensure((size_t)tiles_total * 4));
          MT_TRY(mt_order_tiles_device(s, s->d_multi_map, map_w, map_h, image_w, image_h, tile_w, tile_h, s->d_multi_order,
                                       s->multi_stream));
          order = s->d_multi_order;
        }
        if ((rc2 = mt_deal_tiles_device(s, order, image_w, image_h, tile_w, tile_h, n, r, s->d_multi_list, s->multi_stream)) < 0) return rc2;
      }
      if (stats) HIP_TRY(hipMemsetAsync(s->d_counters, 0, ST_COUNT * sizeof(unsigned long long), s->multi_stream));
      const bool counters_were = s->stats_enabled;
      if (stats) s->stats_enabled = true;
      rc2 = launch_render(s, sensor, image_w, image_h, 0, 0, image_w, image_h, tile_w, tile_h, 0, 1, tiles_of(r),
                          max_depth, s->d_multi_tiles, nullptr, s->multi_stream, tiles_of(r) > 0 ? s->d_multi_list.p : nullptr,
                          list_id);
      s->stats_enabled = counters_were;
      if (rc2 != MT_OK) return rc2;
      if (share_costs) {
        MT_TRY(s->d_multi_map.ensure(map_bytes));
        HIP_TRY(hipMemsetAsync(s->d_multi_map, 0, map_bytes, s->multi_stream));
        if (tiles_of(r) > 0) MT_TRY(mt_scene_export_costs_device(s, s->d_multi_map, map_w, map_h, s->multi_stream));
      }
      HIP_TRY(hipEventRecord(s->multi_done, s->multi_stream));
      return MT_OK;
    };
    rcs[(size_t)r] = body();
    if (rcs[(size_t)r] != MT_OK) errs[(size_t)r] = g_err;  // (thread-local text: hand it to the caller's thread)
  };
  if (n == 1) {
    launch_one(0);
  } else {
    std::vector<std::thread> th;
    th.reserve((size_t)n);
    for (int r = 0; r < n; r++) th.emplace_back(launch_one, r);
    for (auto &t : th) t.join();
  }
  for (int r = 0; r < n; r++) {
    if (rcs[(size_t)r] != MT_OK) return failed(rcs[(size_t)r], "replica " + std::to_string(r) + ": " + errs[(size_t)r]);
  }

  // ---- phase 2: gather on the first replica's device, blit, one copy to the host.  (One exit: a failure half way
  // must not return while copies into out_rgb or kernels on the replicas' buffers are still queued.)
  auto phase2 = [&]() -> int {
    HIP_TRY(hipSetDevice(root->device));
    MT_TRY(root->d_multi_frame.ensure((size_t)image_w * image_h * 3));
    MT_TRY(root->d_multi_gather.ensure((size_t)n * (size_t)n_max * slot));
    MT_TRY(root->d_multi_lists.ensure((size_t)n * (size_t)n_max * 4));
    int rc2;
    if (redeal) {  // every replica's list, for the blit: the same order, dealt out for every rank
      for (int r = 0; r < n; r++) {
        if ((rc2 = mt_deal_tiles_device(root, by_map ? root->d_multi_order.p : nullptr, image_w, image_h, tile_w, tile_h, n, r,
                                        root->d_multi_lists + (size_t)r * n_max, root->multi_stream)) < 0) return rc2;
      }
    }
    for (int r = 1; r < n; r++) HIP_TRY(hipStreamWaitEvent(root->multi_stream, scenes[r]->multi_done, 0));  // (every replica: also one without tiles has a map on its way)
    for (int r = 0; r < n; r++) {
      mt_scene *s = scenes[r];
      const int n_r = tiles_of(r);
      if (n_r == 0) continue;
      const uint8_t *src = s->d_multi_tiles;
      if (s->device != root->device || force_peer) {
        if (s->device != root->device) {  // direct xGMI reads where the platform offers them (once per pair; the copy works without, staged)
          static std::mutex mu;
          static std::map<std::pair<int, int>, bool> tried;
          std::lock_guard<std::mutex> lock(mu);
          bool &done = tried[std::make_pair(root->device, s->device)];
          if (!done) {
            done = true;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, root->device, s->device) == hipSuccess && can) {
              if (hipDeviceEnablePeerAccess(s->device, 0) != hipSuccess) (void)hipGetLastError();  // (already enabled)
            } else {
              (void)hipGetLastError();
            }
          }
        }
        uint8_t *dst = root->d_multi_gather + (size_t)r * (size_t)n_max * slot;
        MT_TRY(copy(dst, root->device, s->d_multi_tiles, s->device, (size_t)n_r * slot, root->multi_stream));
        src = dst;
      }
      MT_TRY(mt_blit_tile_list_device(root, image_w, image_h, tile_w, tile_h, root->d_multi_lists + (size_t)r * n_max, n_r,
                                      src, root->d_multi_frame, root->multi_stream));
    }
    HIP_TRY(hipMemcpyAsync(out_rgb, root->d_multi_frame, (size_t)image_w * image_h * 3, hipMemcpyDeviceToHost, root->multi_stream));
    if (share_costs) {
      // all maps to the first replica's device, element-wise maximum, and back to every replica -- behind the frame's
      // copy on the same streams
      MT_TRY(root->d_multi_maps.ensure((size_t)n * map_bytes));
      if (!root->multi_comb_done) HIP_TRY(hipEventCreateWithFlags(&root->multi_comb_done, hipEventDisableTiming));
      for (int r = 0; r < n; r++) {
        MT_TRY(copy(root->d_multi_maps + (size_t)r * map_w * map_h, root->device, scenes[r]->d_multi_map, scenes[r]->device,
                    map_bytes, root->multi_stream));
      }
      hipLaunchKernelGGL(max_maps_kernel, dim3(256), dim3(256), 0, root->multi_stream, root->d_multi_maps, n, (size_t)map_w * map_h);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(root->multi_comb_done, root->multi_stream));
      for (int r = 0; r < n; r++) {
        mt_scene *s = scenes[r];
        HIP_TRY(hipSetDevice(s->device));
        HIP_TRY(hipStreamWaitEvent(s->multi_stream, root->multi_comb_done, 0));
        MT_TRY(copy(s->d_multi_map, s->device, root->d_multi_maps, root->device, map_bytes, s->multi_stream));
        MT_TRY(mt_scene_import_costs_device(s, s->d_multi_map, map_w, map_h, s->multi_stream));
      }
      HIP_TRY(hipSetDevice(root->device));
    }
    HIP_TRY(hipStreamSynchronize(root->multi_stream));
    return MT_OK;
  };
  if ((rc = phase2()) != MT_OK) return failed(rc, g_err);
  const double total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
  // every replica's launch has completed (the root's stream waited for their events); its device status and counters
  auto phase3 = [&]() -> int {
    int worst = MT_OK;
    std::string text;
    for (int r = 0; r < n; r++) {
      mt_scene *s = scenes[r];
      HIP_TRY(hipSetDevice(s->device));
      HIP_TRY(hipStreamSynchronize(s->multi_stream));
      unsigned long long c[ST_COUNT];
      HIP_TRY(hipMemcpy(c, s->d_counters, sizeof c, hipMemcpyDeviceToHost));
      const int st_rc = check_status(c);
      if (st_rc != MT_OK && worst == MT_OK) {  // (keep going: every replica is synchronised and read)
        worst = st_rc;
        text = g_err;
      }
      if (stats) {
        HIP_TRY(hipMemset(s->d_counters, 0, sizeof c));
        memset(&stats[r], 0, sizeof(mt_stats));
        fill_stats(c, &stats[r]);
        double a = 0.0, b = 0.0;
        if (tiles_of(r) > 0 && mt_scene_kernel_times(s, 1, &a, &b) == 1) stats[r].kernel_ms = a + b;
        stats[r].total_ms = total_ms;
      }
    }
    if (worst != MT_OK) return fail(worst, "%s", text.c_str());
    return MT_OK;
  };
  if ((rc = phase3()) != MT_OK) return failed(rc, g_err);
  for (int r = 0; r < n; r++) {
    scenes[r]->multi_geom = geom;
    scenes[r]->multi_rank = r;
    scenes[r]->multi_list_id = list_id;
  }
  root->multi_have_map = share_costs;
  root->multi_sensor = *sensor;
  root->multi_frames_at_rest = frames_at_rest;
  (void)hipSetDevice(root->device);  // (the calling thread's current device: the first replica's, as on entry to phase 2)
  return MT_OK;
}

int mt_intersect_rays(mt_scene *s, int n, const double *rays, int32_t *tri, int32_t *line_no,
                      double *t, double *point, mt_stats *stats) {
  if (!s || n < 0 || (n > 0 && !rays)) return fail(MT_ERR_ARG, "bad ray batch");
  if (stats) memset(stats, 0, sizeof *stats);
  if (n == 0) return MT_OK;
  HIP_TRY(hipSetDevice(s->device));
  Buf<double> d_rays, d_t, d_point;
  Buf<int> d_tri, d_line;
  MT_TRY(d_rays.ensure((size_t)n * 48));
  MT_TRY(d_t.ensure((size_t)n * 8));
  MT_TRY(d_point.ensure((size_t)n * 24));
  MT_TRY(d_tri.ensure((size_t)n * 4));
  MT_TRY(d_line.ensure((size_t)n * 4));
  HIP_TRY(hipMemcpy(d_rays, rays, (size_t)n * 48, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(s->d_counters, 0, ST_COUNT * sizeof(unsigned long long)));
  const int block = s->waves_per_block * 64;
  // (DEEP layout: every wave of a launch has an area of global memory -- batches of at most 128 K rays per launch)
  const int per_launch = s->deep ? (n < (1 << 17) ? n : (1 << 17)) : n;
  MT_TRY(ensure_deep(s, (size_t)((per_launch + block - 1) / block) * s->waves_per_block));
  HIP_TRY(hipMemcpyAsync(s->d_dev, &s->dev, sizeof(DevScene), hipMemcpyHostToDevice, nullptr));
  HIP_TRY(hipEventRecord(s->ev0, nullptr));
  for (int at = 0; at < n; at += per_launch) {
    const int m = n - at < per_launch ? n - at : per_launch;
    hipLaunchKernelGGL(kernels_of(s->deep).intersect, dim3((m + block - 1) / block), dim3(block), s->lds_bytes, nullptr, s->dev,
                       m, d_rays + (size_t)at * 6, d_tri + at, d_line + at, d_t + at, d_point + (size_t)at * 3, s->d_counters.p);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev1, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  if (tri) HIP_TRY(hipMemcpy(tri, d_tri, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (line_no) HIP_TRY(hipMemcpy(line_no, d_line, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (t) HIP_TRY(hipMemcpy(t, d_t, (size_t)n * 8, hipMemcpyDeviceToHost));
  if (point) HIP_TRY(hipMemcpy(point, d_point, (size_t)n * 24, hipMemcpyDeviceToHost));
  mt_stats local;
  MT_TRY(mt_scene_read_stats(s, &local));
  if (stats) {
    *stats = local;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    stats->kernel_ms = ms;
  }
  return MT_OK;
}

// ---- the octree built on the GPU (mt_build.h) ---------------------------------------------------------------------
struct mt_octree {
  int device = 0;
  int32_t n_tris = 0, n_nodes = 0, depth = 0;
  mt_build_info info{};
  Buf<double> d_aabb, d_center, d_tri_aabb;
  Buf<int32_t> d_first_child, d_prim_begin, d_prim_count, d_tri_id;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

namespace {

extern "C++" {

// b grown to `want` elements with its first `keep` kept; what does not fit is MT_ERR_NOMEM with b as it was
template <typename T>
int build_grow(Buf<T> &b, size_t keep, size_t want, const char *what, hipStream_t stream) {
  Buf<T> grown;
  MT_TRY(attr_nomem(grown.ensure(want * sizeof(T)), want * sizeof(T), what));
  if (keep) HIP_TRY(hipMemcpyAsync(grown.p, b.p, keep * sizeof(T), hipMemcpyDeviceToDevice, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  b.swap(grown);
  return MT_OK;
}

template <typename T>
int build_room(Buf<T> &b, size_t count, const char *what) {
  return attr_nomem(b.ensure(count * sizeof(T)), count * sizeof(T), what);
}

// rocPRIM's exclusive scan of n values of `in` into out, on `stream`, through the scratch buffer `temp`
template <typename In>
int build_scan(Buf<char> &temp, In in, int32_t *out, size_t n, hipStream_t stream) {
  size_t bytes = 0;
  HIP_TRY(rocprim::exclusive_scan(nullptr, bytes, in, out, (int32_t)0, n, rocprim::plus<int32_t>(), stream));
  MT_TRY(build_room(temp, bytes, "the scan's scratch memory"));
  HIP_TRY(rocprim::exclusive_scan((void *)temp.p, bytes, in, out, (int32_t)0, n, rocprim::plus<int32_t>(), stream));
  return MT_OK;
}

}  // extern "C++"

// The build of t->n_tris triangles on t->device: mt_build.h's kernels level by level, one round trip per level.  The
// vertices are d_vertex_in, a device array in add order (mt_scene_set_triangle_vertices' staging array), or, where
// that is NULL, the host array tri_vertex, copied to the device first (mt_octree_build).
int octree_build(mt_octree *t, const double *tri_vertex, const double *d_vertex_in = nullptr) {
  const auto w0 = std::chrono::steady_clock::now();
  const int32_t n = t->n_tris;
  const size_t nt = (size_t)n;
  HIP_TRY(hipSetDevice(t->device));
  HIP_TRY(hipEventCreate(&t->ev0));
  HIP_TRY(hipEventCreate(&t->ev1));
  HostCall call(nullptr, nullptr, t->ev0, t->ev1);
  const hipStream_t stream = call.stream;
  // ---- everything whose size is known: the triangles' arrays, the first nodes
  Buf<double> d_vertex_own;
  Buf<int32_t> d_cur, d_reached, d_split_before, d_value;
  Buf<uint32_t> d_key, d_key_sorted;
  Buf<unsigned long long> d_root_key;
  Buf<char> d_temp;
  size_t cap = nt / 2 + 1024;  // nodes the arrays hold; doubled when a level does not fit
  if (!d_vertex_in) MT_TRY(build_room(d_vertex_own, nt * 9, "the triangles' vertices"));
  const double *const d_vertex = d_vertex_in ? d_vertex_in : d_vertex_own.p;
  MT_TRY(build_room(t->d_tri_aabb, nt * 6, "the triangles' boxes"));
  MT_TRY(build_room(d_cur, nt, "the triangles' nodes"));
  MT_TRY(build_room(d_key, nt, "the sort's keys"));
  MT_TRY(build_room(d_key_sorted, nt, "the sort's keys"));
  MT_TRY(build_room(d_value, nt, "the sort's values"));
  MT_TRY(build_room(t->d_tri_id, nt, "the tree's tri_id"));
  MT_TRY(build_room(d_root_key, 6, "the root box"));
  MT_TRY(build_room(t->d_aabb, cap * 6, "the nodes' boxes"));
  MT_TRY(build_room(t->d_center, cap * 3, "the nodes' centres"));
  MT_TRY(build_room(t->d_first_child, cap, "the nodes' children"));
  MT_TRY(build_room(d_reached, cap, "the nodes' counters"));
  MT_TRY(build_room(t->d_prim_count, cap, "the nodes' counts"));
  const unsigned long long zero_keys[6] = {kBuildKeyZero, kBuildKeyZero, kBuildKeyZero, kBuildKeyZero, kBuildKeyZero, kBuildKeyZero};
  HIP_TRY(hipMemcpy(d_root_key, zero_keys, sizeof zero_keys, hipMemcpyHostToDevice));
  if (n > 0) {
    if (!d_vertex_in) HIP_TRY(hipMemcpy(d_vertex_own, tri_vertex, nt * 72, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(d_cur, 0, nt * sizeof(int32_t), stream));  // every triangle starts at the root
  }
  auto tree = [&]() {
    BuildTree T{};
    T.aabb = t->d_aabb;
    T.center = t->d_center;
    T.first_child = t->d_first_child;
    T.reached = d_reached;
    T.prim_count = t->d_prim_count;
    return T;
  };
  MT_TRY(call.begin(false));
  if (n > 0) HIP_TRY(launch_flat(build_tri_box_kernel, nt, stream, d_vertex, (uint32_t)n, t->d_tri_aabb.p, d_root_key.p));
  hipLaunchKernelGGL(build_root_kernel, dim3(1), dim3(64), 0, stream, tree(), d_root_key.p, n);
  HIP_TRY(hipGetLastError());
  // ---- level by level: a level is the contiguous range [level_begin, level_begin + level_n) of node indices
  int32_t level_begin = 0, level_n = 1, n_nodes = 1;
  int depth = 1, levels = 0;
  for (int level = 1; level <= MT_MAX_TREE_DEPTH; level++) {
    levels++;
    MT_TRY(build_room(d_split_before, (size_t)level_n, "the level's split counts"));
    MT_TRY(build_scan(d_temp, rocprim::make_transform_iterator((const int32_t *)d_reached.p + level_begin, BuildSplits()),
                      d_split_before.p, (size_t)level_n, stream));
    int32_t last[2] = {0, 0};  // the splitting nodes before the level's last node; what reached that node
    HIP_TRY(hipMemcpyAsync(&last[0], d_split_before.p + (level_n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&last[1], d_reached.p + level_begin + (level_n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const long long splits = (long long)last[0] + (last[1] >= kBuildSplit ? 1 : 0);
    if (splits == 0) break;
    if (level == MT_MAX_TREE_DEPTH) {
      return fail(MT_ERR_UNSUPPORTED, "octree depth %d exceeds MT_MAX_TREE_DEPTH %d", level + 1, MT_MAX_TREE_DEPTH);
    }
    const long long grown = (long long)n_nodes + 8 * splits;
    if (grown > 0x7fffffffll) {
      return fail(MT_ERR_UNSUPPORTED, "the octree needs %lld nodes, more than an int32 indexes", grown);
    }
    if ((size_t)grown > cap) {
      size_t want = cap;
      while (want < (size_t)grown) want *= 2;
      MT_TRY(build_grow(t->d_aabb, (size_t)n_nodes * 6, want * 6, "the nodes' boxes", stream));
      MT_TRY(build_grow(t->d_center, (size_t)n_nodes * 3, want * 3, "the nodes' centres", stream));
      MT_TRY(build_grow(t->d_first_child, (size_t)n_nodes, want, "the nodes' children", stream));
      MT_TRY(build_grow(d_reached, (size_t)n_nodes, want, "the nodes' counters", stream));
      MT_TRY(build_grow(t->d_prim_count, (size_t)n_nodes, want, "the nodes' counts", stream));
      cap = want;
    }
    HIP_TRY(launch_flat(build_split_kernel, (size_t)level_n, stream, tree(), level_begin, level_n, (const int32_t *)d_split_before.p, n_nodes));
    HIP_TRY(launch_flat(build_descend_kernel, nt, stream, tree(), (const double *)t->d_tri_aabb.p, d_cur.p, (uint32_t)n));
    level_begin = n_nodes;
    level_n = (int32_t)(8 * splits);
    n_nodes = (int32_t)grown;
    depth = level + 1;
  }
  // ---- the stream: prim_count, prim_begin, and the stable sort of (node, add index)
  MT_TRY(build_room(t->d_prim_begin, (size_t)n_nodes, "the nodes' prim_begin"));
  if (n > 0) {
    HIP_TRY(launch_flat(build_finish_kernel, nt, stream, tree(), (const int32_t *)d_cur.p, (uint32_t)n, d_key.p, d_value.p));
  }
  MT_TRY(build_scan(d_temp, (const int32_t *)t->d_prim_count.p, t->d_prim_begin.p, (size_t)n_nodes, stream));
  if (n > 0) {
    unsigned end_bit = 1;
    while (end_bit < 32 && ((unsigned)(n_nodes - 1) >> end_bit) != 0) end_bit++;
    size_t bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, bytes, d_key.p, d_key_sorted.p, d_value.p, t->d_tri_id.p, nt, 0u, end_bit, stream));
    MT_TRY(build_room(d_temp, bytes, "the sort's scratch memory"));
    HIP_TRY(rocprim::radix_sort_pairs((void *)d_temp.p, bytes, d_key.p, d_key_sorted.p, d_value.p, t->d_tri_id.p, nt, 0u, end_bit, stream));
  }
  MT_TRY(call.mark_end());
  MT_TRY(call.close());  // (waits for the stream)
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, t->ev0, t->ev1));
  t->n_nodes = n_nodes;
  t->depth = depth;
  t->info.n_nodes = n_nodes;
  t->info.depth = depth;
  t->info.levels = levels;
  t->info.kernel_ms = ms;
  t->info.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
  return MT_OK;
}

// checked before any device call, in the order of the header
int check_octree_build_args(int device, int n_tris, const double *tri_vertex) {
  if (n_tris < 0) return fail(MT_ERR_ARG, "%d triangles", n_tris);
  if (n_tris > 0 && !tri_vertex) return fail(MT_ERR_ARG, "the triangle vertex array is NULL");
  const int n_dev = mt_device_count();
  if (n_dev < 0) return n_dev;
  if (device < 0 || device >= n_dev) return fail(MT_ERR_ARG, "device %d outside 0..%d", device, n_dev - 1);
  return MT_OK;
}

// out's counts, and the arrays it asks for, from device arrays of one tree
int octree_read_arrays(int32_t n_nodes, int32_t n_tris, int32_t depth, const double *d_aabb, const double *d_center,
                       const int32_t *d_first_child, const int32_t *d_prim_begin, const int32_t *d_prim_count,
                       const int32_t *d_tri_id, const double *d_tri_aabb, mt_octree_arrays *out) {
  out->n_nodes = n_nodes;
  out->n_tris = n_tris;
  out->depth = depth;
  const size_t nn = (size_t)n_nodes, nt = (size_t)n_tris;
  if (out->node_aabb) HIP_TRY(hipMemcpy(out->node_aabb, d_aabb, nn * 48, hipMemcpyDeviceToHost));
  if (out->node_center) HIP_TRY(hipMemcpy(out->node_center, d_center, nn * 24, hipMemcpyDeviceToHost));
  if (out->first_child) HIP_TRY(hipMemcpy(out->first_child, d_first_child, nn * 4, hipMemcpyDeviceToHost));
  if (out->prim_begin) HIP_TRY(hipMemcpy(out->prim_begin, d_prim_begin, nn * 4, hipMemcpyDeviceToHost));
  if (out->prim_count) HIP_TRY(hipMemcpy(out->prim_count, d_prim_count, nn * 4, hipMemcpyDeviceToHost));
  if (nt && out->tri_id) HIP_TRY(hipMemcpy(out->tri_id, d_tri_id, nt * 4, hipMemcpyDeviceToHost));
  if (nt && out->tri_aabb) HIP_TRY(hipMemcpy(out->tri_aabb, d_tri_aabb, nt * 48, hipMemcpyDeviceToHost));
  return MT_OK;
}

// *out = the tree of t (mt_host_tree.h); *box_add, where wanted, the build's boxes of the triangles in add order
int read_host_tree(const mt_octree *t, HostTree *out, std::vector<double> *box_add) {
  mt_octree_arrays a = out->room_for(t->n_nodes, t->n_tris, box_add);
  HIP_TRY(hipSetDevice(t->device));
  MT_TRY(octree_read_arrays(t->n_nodes, t->n_tris, t->depth, t->d_aabb, t->d_center, t->d_first_child, t->d_prim_begin,
                            t->d_prim_count, t->d_tri_id, t->d_tri_aabb, &a));
  out->n_nodes = a.n_nodes;
  out->n_tris = a.n_tris;
  out->depth = a.depth;
  return MT_OK;
}

}  // namespace

void mt_octree_destroy(mt_octree *t) {
  if (!t) return;
  (void)hipSetDevice(t->device);  // (the buffers are freed with the tree)
  if (t->ev0) (void)hipEventDestroy(t->ev0);
  if (t->ev1) (void)hipEventDestroy(t->ev1);
  delete t;
}

mt_octree *mt_octree_build(int device, int n_tris, const double *tri_vertex, mt_build_info *info) {
  if (check_octree_build_args(device, n_tris, tri_vertex) != MT_OK) return nullptr;
  mt_octree *t = new mt_octree();
  t->device = device;
  t->n_tris = n_tris;
  const int rc = octree_build(t, tri_vertex);
  if (rc != MT_OK) {
    const KeptError why;
    (void)hipGetLastError();
    mt_octree_destroy(t);
    (void)why.fail_again(rc);
    return nullptr;
  }
  if (info) *info = t->info;
  return t;
}

int mt_octree_info(const mt_octree *t, mt_build_info *out) {
  if (!t) return fail(MT_ERR_ARG, "the octree is NULL");
  if (!out) return fail(MT_ERR_ARG, "the mt_build_info is NULL");
  *out = t->info;
  return MT_OK;
}

int mt_octree_read(const mt_octree *t, mt_octree_arrays *out) {
  if (!t) return fail(MT_ERR_ARG, "the octree is NULL");
  if (!out) return fail(MT_ERR_ARG, "the mt_octree_arrays is NULL");
  HIP_TRY(hipSetDevice(t->device));
  return octree_read_arrays(t->n_nodes, t->n_tris, t->depth, t->d_aabb, t->d_center, t->d_first_child, t->d_prim_begin,
                            t->d_prim_count, t->d_tri_id, t->d_tri_aabb, out);
}

mt_scene *mt_scene_create_triangles(const mt_triangle_desc *d, mt_build_info *info) {
  if (!d) {
    fail(MT_ERR_ARG, "desc is NULL");
    return nullptr;
  }
  if (d->struct_size != sizeof(mt_triangle_desc) || d->abi_version != MT_ABI_VERSION) {
    fail(MT_ERR_ARG, "mt_triangle_desc size/version mismatch (%u/%u, want %zu/%d)", d->struct_size, d->abi_version,
         sizeof(mt_triangle_desc), MT_ABI_VERSION);
    return nullptr;
  }
  if (d->n_tris < 0 || d->n_materials < 0 || d->n_textures < 0) {
    fail(MT_ERR_ARG, "negative or empty counts");
    return nullptr;
  }
  if (d->n_tris > 0 && (!d->tri_vertex || !d->tri_normal || !d->tri_uvw || !d->tri_material || !d->tri_line_no)) {
    fail(MT_ERR_ARG, "triangle arrays missing");
    return nullptr;
  }
  if ((d->n_materials > 0 && !d->materials) || (d->n_textures > 0 && !d->textures)) {
    fail(MT_ERR_ARG, "material/texture arrays missing");
    return nullptr;
  }
  mt_build_info built{};
  mt_octree *t = mt_octree_build(d->device, d->n_tris, d->tri_vertex, &built);
  if (!t) return nullptr;
  // the tree on the host, and the triangles gathered into its stream order
  const size_t nt = (size_t)d->n_tris;
  HostTree tree;
  std::vector<double> box_add;
  const int rc = read_host_tree(t, &tree, &box_add);
  mt_octree_destroy(t);
  if (rc != MT_OK) return nullptr;
  std::vector<double> vertex(nt * 9), normal(nt * 9), uvw(nt * 9), box(nt * 6);
  std::vector<int32_t> material(nt), line_no(nt);
  for (size_t s = 0; s < nt; s++) {
    const size_t i = (size_t)tree.tri_id[s];
    memcpy(&vertex[s * 9], d->tri_vertex + i * 9, 72);
    memcpy(&normal[s * 9], d->tri_normal + i * 9, 72);
    memcpy(&uvw[s * 9], d->tri_uvw + i * 9, 72);
    memcpy(&box[s * 6], &box_add[i * 6], 48);
    material[s] = d->tri_material[i];
    line_no[s] = d->tri_line_no[i];
  }
  mt_scene_desc sd = new_scene_desc(d->device, d->n_tris, d->n_materials, d->n_textures);
  describe_tree(tree, &sd);
  sd.tri_vertex = vertex.data();
  sd.tri_normal = normal.data();
  sd.tri_uvw = uvw.data();
  sd.tri_aabb = box.data();
  sd.tri_material = material.data();
  sd.tri_line_no = line_no.data();
  sd.materials = d->materials;
  sd.textures = d->textures;
  mt_scene *s = mt_scene_create(&sd);
  if (s && info) *info = built;
  return s;
}

int mt_scene_read_tree(const mt_scene *s, mt_octree_arrays *out) {
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  if (!out) return fail(MT_ERR_ARG, "the mt_octree_arrays is NULL");
  if (!s->have_tri_id) return fail(MT_ERR_ARG, "the scene was made without tri_id");
  const size_t nn = (size_t)s->dev.n_nodes, nt = (size_t)s->dev.n_tris;
  out->n_nodes = s->dev.n_nodes;
  out->n_tris = s->dev.n_tris;
  out->depth = s->dev.tree_depth;
  HIP_TRY(hipSetDevice(s->device));
  std::vector<NodeRec> recs(nn);
  HIP_TRY(hipMemcpy(recs.data(), s->dev.nodes, nn * sizeof(NodeRec), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < nn; i++) {
    const NodeRec &r = recs[i];
    for (int k = 0; k < 3; k++) {
      if (out->node_aabb) {
        out->node_aabb[i * 6 + k] = r.lo[k];
        out->node_aabb[i * 6 + 3 + k] = r.hi[k];
      }
      if (out->node_center) out->node_center[i * 3 + k] = r.c[k];
    }
    if (out->first_child) out->first_child[i] = r.first_child;
    if (out->prim_begin) out->prim_begin[i] = r.prim_begin;
    if (out->prim_count) out->prim_count[i] = r.prim_count;
  }
  if (nt && out->tri_id) memcpy(out->tri_id, s->tri_id_host.data(), nt * sizeof(int32_t));
  if (nt && out->tri_aabb) {  // (the scene holds the boxes in stream order)
    std::vector<double> box(nt * 6);
    HIP_TRY(hipMemcpy(box.data(), s->dev.tri_aabb, nt * 48, hipMemcpyDeviceToHost));
    for (size_t p = 0; p < nt; p++) memcpy(out->tri_aabb + (size_t)s->tri_id_host[p] * 6, &box[p * 6], 48);
  }
  return MT_OK;
}

// ---- triangles moved in place (mt_build.h's move_* kernels, mt_move.h's bookkeeping), and triangles added and removed
// in place (its edit_* kernels, mt_edit.h's bookkeeping): one set of steps, a move being the edit that keeps the count --
namespace {

double ms_since(const std::chrono::steady_clock::time_point &t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// What mt_scene_edit_triangles was given, for the steps that differ from a move's
struct EditList {
  const int32_t *remove_idx = nullptr;
  int n_remove = 0, n_add = 0;
  const double *add_vertex = nullptr, *add_normal = nullptr, *add_uvw = nullptr;
  const int32_t *add_material = nullptr, *add_line_no = nullptr;
};

// What the steps of a move or an edit hand on to one another.  Everything in it is built aside and frees itself: until
// move_swap nothing of the scene is written, and a return leaves the scene exactly as it was.
struct Move {
  int32_t n = 0;      // the triangles of the scene that is being built (a move: the scene's own count)
  int32_t n_old = 0;  // the scene's triangles
  const EditList *edit = nullptr;  // an edit's lists; NULL: a move
  // 1. + 2. the vertices in (the new) add order; a move: add index -> old stream position, an edit: new add index -> old
  // stream position or ~(added triangle) (d_old_pos for both); and the step's own inputs
  Buf<double> d_stage, d_listed;
  Buf<int32_t> d_old_pos, d_old_id, d_idx;
  Buf<unsigned int> d_changed;
  // an edit's: the keep plane and its scan, the added triangles' attributes
  Buf<int32_t> d_keep, d_new_add, d_add_mtl, d_add_line;
  Buf<double> d_add_normal, d_add_uvw;
  Buf<char> d_scan_temp;
  // 3.
  std::unique_ptr<mt_octree, void (*)(mt_octree *)> tree{nullptr, mt_octree_destroy};
  // 4. the scene's next `geo` and `tri`, the boxes in stream order, the scene's next stamp planes and tri_id
  DeviceAllocs geo;
  TriArrays tri;
  Buf<double> d_box_stream;
  Buf<uint32_t> d_stamp[2];
  Buf<int32_t> d_tri_id;
  // 5. the tree, the stream-order boxes and vertices on the host; the next mirrors, layout and DevScene
  HostTree host;
  std::vector<double> box, vertex;
  MovedMirrors mirrors;
  std::shared_ptr<const std::vector<int32_t>> tri_mtl;
  SceneLayout L;
  DevScene dev{};
};

// 1. + 2.: the live vertices in add order, the listed triangles written over them.  *changed: the triangles of the list
// whose vertices are not the live ones, bit for bit.
int move_stage(const mt_scene *s, const int32_t *add_idx, int n_idx, const double *vertices, Move &M, unsigned int *changed) {
  const size_t nt = (size_t)M.n, ni = (size_t)n_idx;
  const hipStream_t stream = nullptr;
  MT_TRY(build_room(M.d_stage, nt * 9, "the staged vertices"));
  MT_TRY(build_room(M.d_listed, ni * 9, "the listed vertices"));
  MT_TRY(build_room(M.d_old_id, nt, "the old tri_id"));
  MT_TRY(build_room(M.d_old_pos, nt, "the old stream positions"));
  MT_TRY(build_room(M.d_idx, ni, "the index list"));
  MT_TRY(build_room(M.d_changed, 1, "the changed count"));
  HIP_TRY(hipMemcpyAsync(M.d_old_id, s->tri_id_host.data(), nt * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(M.d_idx, add_idx, ni * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(M.d_listed, vertices, ni * 72, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetAsync(M.d_old_pos, 0xff, nt * sizeof(int32_t), stream));
  HIP_TRY(hipMemsetAsync(M.d_changed, 0, sizeof(unsigned int), stream));
  HIP_TRY(launch_flat(move_unscatter_kernel, nt, stream, s->dev.tri_vertex, (const int32_t *)M.d_old_id.p, (uint32_t)M.n,
                      M.d_stage.p, M.d_old_pos.p));
  HIP_TRY(launch_flat(move_overwrite_kernel, ni, stream, (const int32_t *)M.d_idx.p, (const double *)M.d_listed.p, (uint32_t)n_idx,
                      (uint32_t)M.n, M.d_stage.p, M.d_changed.p));
  HIP_TRY(hipMemcpyAsync(changed, M.d_changed, sizeof *changed, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return MT_OK;
}

// 1. + 2. of an edit: the survivors' live vertices in the new add order, the added triangles behind them, and every new
// add index's source (mt_build.h).  The scan's total is held to the host's own count.
int edit_stage(const mt_scene *s, Move &M) {
  const EditList &E = *M.edit;
  const size_t n_old = (size_t)M.n_old, nt = (size_t)M.n, nr = (size_t)E.n_remove, na = (size_t)E.n_add;
  const int32_t n_keep = M.n_old - E.n_remove;
  const hipStream_t stream = nullptr;
  MT_TRY(build_room(M.d_stage, nt * 9, "the staged vertices"));
  MT_TRY(build_room(M.d_old_pos, nt, "the triangles' sources"));
  MT_TRY(build_room(M.d_old_id, n_old, "the old tri_id"));
  MT_TRY(build_room(M.d_keep, n_old, "the keep plane"));
  MT_TRY(build_room(M.d_new_add, n_old, "the new add indices"));
  HIP_TRY(hipMemcpyAsync(M.d_old_id, s->tri_id_host.data(), n_old * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)M.d_keep.p, 1, n_old, stream));
  HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)M.d_old_pos.p, kEditNoSource, nt, stream));
  if (nr > 0) {
    MT_TRY(build_room(M.d_idx, nr, "the remove list"));
    HIP_TRY(hipMemcpyAsync(M.d_idx, E.remove_idx, nr * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(launch_flat(edit_mark_kernel, nr, stream, (const int32_t *)M.d_idx.p, (uint32_t)nr, (uint32_t)n_old, M.d_keep.p));
  }
  if (na > 0) {
    MT_TRY(build_room(M.d_listed, na * 9, "the added vertices"));
    MT_TRY(build_room(M.d_add_normal, na * 9, "the added normals"));
    MT_TRY(build_room(M.d_add_uvw, na * 9, "the added uvw"));
    MT_TRY(build_room(M.d_add_mtl, na, "the added materials"));
    MT_TRY(build_room(M.d_add_line, na, "the added line numbers"));
    HIP_TRY(hipMemcpyAsync(M.d_listed, E.add_vertex, na * 72, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(M.d_add_normal, E.add_normal, na * 72, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(M.d_add_uvw, E.add_uvw, na * 72, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(M.d_add_mtl, E.add_material, na * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(M.d_add_line, E.add_line_no, na * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  }
  MT_TRY(build_scan(M.d_scan_temp, (const int32_t *)M.d_keep.p, M.d_new_add.p, n_old, stream));
  int32_t last[2] = {0, 0};  // the survivors before the last old add index; whether that one is kept
  HIP_TRY(hipMemcpyAsync(&last[0], M.d_new_add.p + (n_old - 1), sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(&last[1], M.d_keep.p + (n_old - 1), sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if ((long long)last[0] + last[1] != (long long)n_keep) {
    return fail(MT_ERR_INTERNAL, "the keep plane sums to %lld survivors, the lists to %d", (long long)last[0] + last[1], n_keep);
  }
  HIP_TRY(launch_flat(edit_stage_kernel, n_old + na, stream, s->dev.tri_vertex, (const int32_t *)M.d_old_id.p,
                      (const int32_t *)M.d_keep.p, (const int32_t *)M.d_new_add.p, (uint32_t)n_old, (uint32_t)n_keep,
                      (const double *)M.d_listed.p, (uint32_t)na, M.d_stage.p, M.d_old_pos.p));
  HIP_TRY(hipStreamSynchronize(stream));
  return MT_OK;
}

// 3.: the tree, from the staging array
int move_build(const mt_scene *s, Move &M) {
  M.tree.reset(new mt_octree());
  M.tree->device = s->device;
  M.tree->n_tris = M.n;
  const int rc = octree_build(M.tree.get(), nullptr, M.d_stage.p);
  if (rc != MT_OK) (void)hipGetLastError();  // (the refusal's text stands: nothing here writes g_err)
  return rc;
}

// 4.: the per-triangle arrays in the new order, in new allocations
int move_regather(const mt_scene *s, Move &M) {
  const size_t nt = (size_t)M.n;
  const hipStream_t stream = nullptr;
  const mt_octree *tree = M.tree.get();
  MoveArrays was{}, now{};
  was.vertex = s->tri.vertex;
  was.normal = s->tri.normal;
  was.uvw = s->tri.uvw;
  was.mtl = s->tri.mtl;
  was.line = s->tri.line;  // (was.aabb stays NULL: the boxes come from the build, not from the old scene)
  MT_TRY(M.geo.alloc<double>(nt * 9, "the triangles' vertices", &now.vertex));
  MT_TRY(M.geo.alloc<double>(nt * 9, "the triangles' normals", &now.normal));
  MT_TRY(M.geo.alloc<double>(nt * 9, "the triangles' uvw", &now.uvw));
  MT_TRY(M.geo.alloc<int32_t>(nt, "the triangles' materials", &now.mtl));
  MT_TRY(M.geo.alloc<int32_t>(nt, "the triangles' line numbers", &now.line));
  M.tri = TriArrays{now.vertex, now.normal, now.uvw, now.mtl, now.line};
  MT_TRY(build_room(M.d_box_stream, nt * 6, "the triangles' boxes"));
  now.aabb = M.d_box_stream;
  for (int w = 0; w < 2; w++) {
    if (s->d_attr_stamp[w].p == nullptr) continue;
    MT_TRY(build_room(M.d_stamp[w], nt, "the triangles' stamp plane"));
    was.stamp[w] = s->d_attr_stamp[w];
    now.stamp[w] = M.d_stamp[w];
  }
  if (s->d_tri_id.p != nullptr) {  // (the G-buffer's `prim` plane reads it)
    MT_TRY(build_room(M.d_tri_id, nt, "the scene's tri_id"));
    HIP_TRY(hipMemcpyAsync(M.d_tri_id, tree->d_tri_id, nt * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
  }
  if (M.edit != nullptr) {
    const EditAdds add{M.d_add_normal, M.d_add_uvw, M.d_add_mtl, M.d_add_line};
    HIP_TRY(launch_flat(edit_regather_kernel, nt, stream, was, add, now, (const double *)M.d_stage.p,
                        (const double *)tree->d_tri_aabb.p, (const int32_t *)tree->d_tri_id.p, (const int32_t *)M.d_old_pos.p,
                        (uint32_t)M.n, (uint32_t)M.n_old, (uint32_t)M.edit->n_add));
  } else {
    HIP_TRY(launch_flat(move_regather_kernel, nt, stream, was, now, (const double *)M.d_stage.p, (const double *)tree->d_tri_aabb.p,
                        (const int32_t *)tree->d_tri_id.p, (const int32_t *)M.d_old_pos.p, (uint32_t)M.n));
  }
  HIP_TRY(hipStreamSynchronize(stream));
  return MT_OK;
}

// 5., the device's half: the tree, the stream-order boxes and vertices on the host
int move_readback(Move &M) {
  const size_t nt = (size_t)M.n;
  M.box.resize(nt * 6);
  M.vertex.resize(nt * 9);
  MT_TRY(read_host_tree(M.tree.get(), &M.host, nullptr));
  HIP_TRY(hipMemcpy(M.box.data(), M.d_box_stream, nt * 48, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(M.vertex.data(), M.tri.vertex, nt * 72, hipMemcpyDeviceToHost));
  return MT_OK;
}

// 5., the host's half: the mirrors in the new order, then the checks and the derived arrays of a new scene
int move_derive(const mt_scene *s, Move &M) {
  std::vector<int32_t> from;
  MoveError merr;
  const bool made =
      M.edit != nullptr
          ? edit_mirrors(s->tri_id_host, M.edit->remove_idx, (size_t)M.edit->n_remove, (size_t)M.edit->n_add, M.edit->add_material,
                         M.host.tri_id.data(), (size_t)M.n, *s->tri_mtl_host, s->attr_stamp_host, &M.mirrors, &from, &merr)
          : move_mirrors(s->tri_id_host, M.host.tri_id.data(), *s->tri_mtl_host, s->attr_stamp_host, &M.mirrors, &from, &merr);
  if (!made) return fail(merr);
  M.tri_mtl = std::make_shared<const std::vector<int32_t>>(std::move(M.mirrors.tri_mtl));  // (trees hold the old one)
  // The description of the new scene as mt_scene_create would get it.  check_scene_desc and derive_layout read the node
  // arrays, tri_vertex, tri_aabb, tri_material and the material / texture tables; of tri_normal, tri_uvw, tri_line_no
  // and the textures' texels they only ask that they are there (the scene keeps no host copy of them: stand-ins).
  std::vector<mt_texture> texs((size_t)s->n_textures);
  for (size_t i = 0; i < texs.size(); i++) {
    const DevTexture &t = s->texs_host[i];
    texs[i] = mt_texture{t.width, t.height, t.format, 0, t.texels};
  }
  mt_scene_desc sd = new_scene_desc(s->device, M.n, s->n_materials, s->n_textures);
  describe_tree(M.host, &sd);
  sd.tri_vertex = M.vertex.data();
  sd.tri_normal = M.vertex.data();  // (stand-in)
  sd.tri_uvw = M.vertex.data();     // (stand-in)
  sd.tri_aabb = M.box.data();
  sd.tri_material = M.tri_mtl->data();
  sd.tri_line_no = M.host.tri_id.data();  // (stand-in)
  sd.materials = s->mtls_host.data();
  sd.textures = texs.data();
  std::vector<int> depth_of;
  int max_depth = 0;
  LayoutError lerr;
  if (!check_scene_desc(sd, &depth_of, &max_depth, &lerr)) return fail(lerr);
  derive_layout(sd, depth_of, &M.L);
  return MT_OK;
}

// 6.: the swap.  M.dev, the live DevScene with the derived arrays of M.geo, gets the rest of the moved scene: its
// per-triangle arrays, and the counts with what is computed from them (the packed stack's shift here; the engine gate
// reads dev.n_tris at every launch; the G-buffer's d_tri_id, where allocated, was made for the new count).  The
// launch configuration depends on the tree (deep layout, LDS bytes, packed stack): if it cannot be made, the old scene
// and its configuration come back.  After it nothing fails, and the scene takes what was built aside: M keeps what the
// scene gives up.
int move_swap(mt_scene *s, Move &M) {
  show_tri_arrays(M.tri, &M.dev);
  M.dev.n_tris = M.n;
  M.dev.n_nodes = M.host.n_nodes;
  M.dev.pack_shift = s->tune.v[MT_TUNE_PACKED_STACK] != 0.0 ? pack_shift_for(M.n, M.host.n_nodes) : 0;
  const DevScene dev_was = s->dev;
  s->dev = M.dev;
  const int rc = configure_launch(s);
  if (rc != MT_OK) {
    const KeptError why;
    (void)hipGetLastError();
    s->dev = dev_was;
    (void)configure_launch(s);
    return why.fail_again(rc);
  }
  s->dev_uploaded_valid = false;
  s->geo.swap(M.geo);
  M.geo.free_all();  // (the old arrays, within the call's total_ms)
  s->tri = M.tri;
  s->tri_id_host.swap(M.mirrors.tri_id);
  s->tri_mtl_host = M.tri_mtl;
  for (int w = 0; w < 2; w++) {
    s->attr_stamp_host[w].swap(M.mirrors.stamp[w]);
    if (M.d_stamp[w].p != nullptr) s->d_attr_stamp[w].swap(M.d_stamp[w]);
  }
  if (M.d_tri_id.p != nullptr) s->d_tri_id.swap(M.d_tri_id);
  s->geo_generation++;
  return MT_OK;
}

// Steps 1 .. 6 of mt_scene_set_triangle_vertices for a checked list of n_idx >= 1 triangles, and of
// mt_scene_edit_triangles for checked lists that are not both empty (edit != NULL)
int move_triangles(mt_scene *s, const int32_t *add_idx, int n_idx, const double *vertices, const EditList *edit, mt_build_info *info) {
  const auto w0 = std::chrono::steady_clock::now();
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipDeviceSynchronize());  // no kernel of an earlier call reads the scene while it is taken apart
  Move M;
  M.n_old = s->dev.n_tris;
  M.n = edit != nullptr ? M.n_old - edit->n_remove + edit->n_add : M.n_old;
  M.edit = edit;
  if (edit != nullptr) {
    MT_TRY(edit_stage(s, M));
  } else {
    unsigned int changed = 0;
    MT_TRY(move_stage(s, add_idx, n_idx, vertices, M, &changed));
    if (changed == 0) return MT_OK;  // the listed vertices are the live ones, bit for bit
  }
  double part_ms[MT_MOVE_TIMES] = {};
  auto t0 = std::chrono::steady_clock::now();
  const auto lap = [&](int part) {
    part_ms[part] = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
  };
  MT_TRY(move_build(s, M));
  lap(MT_MOVE_MS_BUILD);
  MT_TRY(move_regather(s, M));
  lap(MT_MOVE_MS_REGATHER);
  MT_TRY(move_readback(M));
  lap(MT_MOVE_MS_READBACK);
  MT_TRY(move_derive(s, M));
  lap(MT_MOVE_MS_LAYOUT);
  M.dev = s->dev;
  MT_TRY(upload_derived(M.L, M.geo, &M.dev));
  lap(MT_MOVE_MS_UPLOAD);
  MT_TRY(move_swap(s, M));
  for (int k = 0; k < MT_MOVE_TIMES; k++) s->move_ms[k] = part_ms[k];
  if (info) {
    *info = M.tree->info;
    info->total_ms = ms_since(w0);
  }
  return MT_OK;
}

}  // namespace

int mt_scene_set_triangle_vertices(mt_scene *s, const int32_t *add_idx, int n_idx, const double *vertices, mt_build_info *info) {
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  MoveError err;
  if (!check_move_list(s->have_tri_id, s->dev.n_tris, add_idx, n_idx, vertices, &err)) return fail(err);
  if (info) memset(info, 0, sizeof *info);
  if (n_idx == 0) return MT_OK;
  if (!s->tri_id_checked) {  // (a tri_id is the caller's at mt_scene_create: the kernels scatter through it; checked once)
    std::vector<int32_t> from;
    if (!compose_move(s->tri_id_host.data(), s->tri_id_host.data(), s->tri_id_host.size(), &from, &err)) {
      return fail(MT_ERR_ARG, "the scene's tri_id is no permutation of its triangles: %s", err.msg.c_str());
    }
    s->tri_id_checked = true;
  }
  try {
    return move_triangles(s, add_idx, n_idx, vertices, nullptr, info);
  } catch (const std::bad_alloc &) {
    return fail(MT_ERR_NOMEM, "no host memory for the moved scene's arrays");
  }
}

int mt_scene_edit_triangles(mt_scene *s, const int32_t *remove_idx, int n_remove, int n_add, const double *add_vertex,
                            const double *add_normal, const double *add_uvw, const int32_t *add_material,
                            const int32_t *add_line_no, mt_build_info *info) {
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  MoveError err;
  EditAdd add;
  add.n = n_add;
  add.vertex = add_vertex;
  add.normal = add_normal;
  add.uvw = add_uvw;
  add.material = add_material;
  add.line_no = add_line_no;
  try {
    if (!check_edit_args(s->have_tri_id, s->dev.n_tris, remove_idx, n_remove, add, s->n_materials, &err)) return fail(err);
    if (info) memset(info, 0, sizeof *info);
    if (n_remove == 0 && n_add == 0) return MT_OK;
    if (!s->tri_id_checked) {  // (as for a move: the kernels scatter through a tri_id that was the caller's)
      std::vector<int32_t> from;
      if (!compose_move(s->tri_id_host.data(), s->tri_id_host.data(), s->tri_id_host.size(), &from, &err)) {
        return fail(MT_ERR_ARG, "the scene's tri_id is no permutation of its triangles: %s", err.msg.c_str());
      }
      s->tri_id_checked = true;
    }
    const EditList edit{remove_idx, n_remove, n_add, add_vertex, add_normal, add_uvw, add_material, add_line_no};
    return move_triangles(s, nullptr, 0, nullptr, &edit, info);
  } catch (const std::bad_alloc &) {
    return fail(MT_ERR_NOMEM, "no host memory for the edited scene's arrays");
  }
}

int mt_scene_get_triangle_vertices(mt_scene *s, double *out, int n_tris) {
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  MoveError err;
  if (!check_move_get(s->have_tri_id, s->dev.n_tris, out, n_tris, &err)) return fail(err);
  if (n_tris == 0) return MT_OK;
  const size_t nt = (size_t)n_tris;
  try {
    std::vector<double> stream_order(nt * 9);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpy(stream_order.data(), s->dev.tri_vertex, nt * 72, hipMemcpyDeviceToHost));  // (waits for the device)
    for (size_t p = 0; p < nt; p++) {
      const int32_t a = s->tri_id_host[p];
      if (a < 0 || a >= n_tris) return fail(MT_ERR_ARG, "the scene's tri_id is no permutation of its triangles");
      memcpy(out + (size_t)a * 9, &stream_order[p * 9], 72);
    }
  } catch (const std::bad_alloc &) {
    return fail(MT_ERR_NOMEM, "no host memory for %d triangles' vertices", n_tris);
  }
  return MT_OK;
}

int mt_scene_move_times_last(const mt_scene *s, double *out_ms) {
  if (!s) return fail(MT_ERR_ARG, "scene is NULL");
  if (!out_ms) return fail(MT_ERR_ARG, "the output array is NULL");
  for (int k = 0; k < MT_MOVE_TIMES; k++) out_ms[k] = s->move_ms[k];
  return MT_OK;
}

}  // extern "C"
