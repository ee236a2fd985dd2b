/* mythtracer_hip.h — C ABI of libmythtracer_hip.so (MI355X / gfx950).
 *
 * The reference (gynvael/MythTracer, /root/reference/VerStarting) has no FFI or
 * plugin layer: its seam is the C++ class raytracer::MythTracer
 * (mythtracer.h:55-66).  This C ABI sits directly UNDER that seam.  Each entry
 * point below names the reference code it replaces; the host-side C++ facade
 * (mythtracer_amd/host, same class/field names as the reference) and any other
 * language binding call these and nothing else.  See INTEGRATION.md.
 *
 * Conventions: plain C, POD only, no exceptions.  Functions returning int
 * return MT_OK (0) or a negative MT_ERR_*; mt_last_error() gives the text for
 * the calling thread.  All pointers in mt_scene_desc / mt_render_* arguments
 * are HOST pointers unless the name starts with d_ (device pointer on the
 * scene's GPU).  One render may be in flight per mt_scene at a time.  The
 * library never falls back to a CPU path: without a usable HIP device every
 * call fails with MT_ERR_HIP.
 */
#ifndef MYTHTRACER_HIP_H_
#define MYTHTRACER_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MT_ABI_VERSION 5

enum {
  MT_OK = 0,
  MT_ERR_ARG = -1,         /* bad argument / inconsistent description */
  MT_ERR_HIP = -2,         /* HIP runtime error (text in mt_last_error) */
  MT_ERR_UNSUPPORTED = -3, /* e.g. octree deeper than MT_MAX_TREE_DEPTH */
  MT_ERR_NOMEM = -4,
  MT_ERR_INTERNAL = -5     /* a device-side loop bound tripped: kernel logic error */
};

/* Deepest octree (root = depth 1) the traversal stack can hold.  The
 * reference has no limit (octtree.cc:52-135 recurses while a node holds >= 16
 * primitives); we refuse deeper trees instead of overflowing. */
#define MT_MAX_TREE_DEPTH 64
/* Deepest reflection/refraction recursion (reference: compile-time
 * MAX_RECURSION_LEVEL = 5, mythtracer.h:11). */
#define MT_MAX_RECURSION 16

/* raytracer::Material (material.h:12-48), tex = index into textures or -1. */
typedef struct mt_material {
  double ambient[3], diffuse[3], specular[3];
  double specular_exp, reflectance, transparency;
  double transmission_filter[3];
  double refraction_index;
  int32_t tex;
  int32_t reserved;
} mt_material;

/* raytracer::Light (light.h:8-14). */
typedef struct mt_light {
  double position[3], ambient[3], diffuse[3], specular[3];
} mt_light;

enum { MT_TEX_RGB8 = 0, MT_TEX_F64 = 1 };

/* raytracer::Texture (texture.h:13-23).  RGB8: 3 bytes per texel, colour =
 * byte / 255.0 (exactly what texture.cc:100-104 stores); F64: 3 doubles. */
typedef struct mt_texture {
  int32_t width, height;
  int32_t format;
  int32_t reserved;
  const void *texels;
} mt_texture;

/* Camera::Sensor after Sensor::Reset (camera.cc:27-63) plus the camera
 * origin: what Sensor::GetRay (camera.cc:65-69) needs.  Computed on the host
 * (sin/cos stay glibc's). */
typedef struct mt_sensor {
  double origin[3];
  double start_point[3];
  double delta_scanline[3];
  double delta_pixel[3];
} mt_sensor;

/* PerPixelDebugInfo (mythtracer.h:13-16). */
typedef struct mt_debug_px {
  int32_t line_no; /* -1 = no hit */
  int32_t reserved;
  double point[3];
} mt_debug_px;

/* Work counters of one call (sums over all pixels / rays). */
typedef struct mt_stats {
  uint64_t rays_primary;   /* OctTree::IntersectRay from level-0 TraceRayWorker */
  uint64_t rays_secondary; /* ... from level>0 (reflection / refraction) */
  uint64_t rays_shadow;    /* ... from the shadow loop (mythtracer.cc:94-156) */
  uint64_t box_tests;      /* Node::NodeIntersectRay evaluations (root included) */
  uint64_t node_visits;    /* Node::PrimitiveIntersectRay evaluations */
  uint64_t tri_tests;      /* Triangle::IntersectRay evaluations */
  uint64_t mt_tests;       /* ... that passed the AABB pre-filter */
  uint64_t shaded_hits;    /* TraceRayWorker calls that hit a primitive */
  uint64_t wave_node_steps;/* wave-level node scans executed (GPU only) */
  uint64_t wave_tri_steps; /* wave-level triangle slab evaluations (GPU only) */
  double kernel_ms;        /* device time of the kernel(s), HIP events */
  double total_ms;         /* wall time of the call incl. copies */
  /* Bytes the kernels REQUESTED (counted at the load/store instructions of the
   * path, whatever cache served them): by wave-uniform scalar loads -- one box
   * or node record fetched once for all rays of a wave -- and by per-lane
   * vector accesses (boxes, vertices, node records, shading inputs, per-ray
   * state), summed over lanes.  bench.py's roofline numerator. */
  uint64_t bytes_scalar;
  uint64_t bytes_vector;
} mt_stats;

/* Flattened scene: what Scene{tree, materials, textures} (scene.h:9-15) holds
 * after OctTree::Finalize (octtree.cc:16-24).
 *
 * Nodes are in breadth-first order, root = node 0; the 8 children of a split
 * node are the consecutive nodes first_child .. first_child+7 in the
 * reference's child order (octtree.cc:61-100: bit0 = x high, bit1 = z high,
 * bit2 = y high); first_child = 0 means "no children".
 *
 * Triangles are in NODE-STREAM order: node after node (same order as the node
 * array), inside a node in the order of Node::primitives.  prim_begin/count
 * index into that stream.  tri_id gives the AddPrimitive order index. */
typedef struct mt_scene_desc {
  uint32_t struct_size; /* sizeof(mt_scene_desc) */
  uint32_t abi_version; /* MT_ABI_VERSION */
  int32_t device;       /* HIP device ordinal */
  int32_t n_nodes, n_tris, n_materials, n_textures;
  int32_t tree_depth;   /* root = 1 */
  const double *node_aabb;        /* n_nodes x 6: min xyz, max xyz */
  const double *node_center;      /* n_nodes x 3 (Node::CalcCenter) */
  const int32_t *node_first_child;
  const int32_t *node_prim_begin;
  const int32_t *node_prim_count;
  const double *tri_vertex;       /* n_tris x 9 */
  const double *tri_normal;       /* n_tris x 9 */
  const double *tri_uvw;          /* n_tris x 9 */
  const double *tri_aabb;         /* n_tris x 6 (Triangle::cached_aabb) */
  const int32_t *tri_material;    /* -1 = mtl == nullptr */
  const int32_t *tri_line_no;     /* Primitive::debug_line_no */
  const int32_t *tri_id;
  const mt_material *materials;
  const mt_texture *textures;
} mt_scene_desc;

typedef struct mt_scene mt_scene;

const char *mt_last_error(void);
int mt_abi_version(void);
/* Number of visible HIP devices (<0 on error). */
int mt_device_count(void);

/* Uploads the flattened scene to HBM.  Replaces: the in-memory Scene the
 * reference keeps after LoadObj + Finalize (mythtracer.cc:247-256,281-285).
 * NULL on failure, with mt_last_error: an upload that does not fit on the device
 * is MT_ERR_NOMEM, as for every other call here that allocates. */
mt_scene *mt_scene_create(const mt_scene_desc *desc);
void mt_scene_destroy(mt_scene *scene);

/* scene.lights (scene.h:14) — read at render time (mythtracer.cc:78), mutated
 * by the caller between frames (main_local.cc:79-110). */
int mt_scene_set_lights(mt_scene *scene, const mt_light *lights, int n);

/* scene.materials edited in place: the constants of ALL materials replaced -- the same count, the textures untouched;
 * `tex` may point at another existing texture.  (No reference counterpart: its drivers load a scene once.)  For a
 * look-dev session that changes a wall's colour or a mirror's reflectance between frames without flattening and
 * uploading the triangles again.  Every kernel reads the material table at run time and nothing derived from it is
 * baked into the uploaded scene, so the call is one copy.
 * mt_scene_set_materials is synchronous: it waits until the scene's device is idle, then copies.  "One call in flight
 * per scene" holds for it like for every other call.  The scene keeps a host copy of its current materials and a
 * generation number: mt_scene_create fills both, the generation starts at 0 and is bumped by every successful set that
 * changes at least one byte.  A set that changes nothing changes no state and makes no device call.
 * mt_scene_get_materials returns the host copy.  Zero materials and n = 0 is MT_OK and does nothing, in both.
 * CONTRACT: after mt_scene_set_materials(B), every call that renders or shades -- mt_render_chunk[_device], _ss,
 * _adaptive, the tile and tile-list forms, mt_render_gbuffer, mt_render_lightbuffer, mt_shade_direct,
 * mt_update_lightbuffer, mt_raytree_create[_rays], mt_trace_rays, mt_intersect_rays -- gives, byte for byte and plane
 * for plane, what the same call gives on a scene newly created from the same description with materials B.
 * Cost history, forecasts and engine choice are left as they are: they are forecasts, not results, and a frame under
 * edited materials is scheduled by the costs of the frames before it.  G-buffer and light-buffer planes are the
 * caller's: planes rendered before the edit describe the old materials.  Ray trees of the scene become STALE, see
 * mt_raytree_update_materials.
 * Argument checks come before any device call, in this order: the scene (NULL); n unequal to the scene's material
 * count; a NULL array with n > 0; set only: a `tex` outside -1 .. n_textures - 1 (mt_scene_create's message).  All
 * MT_ERR_ARG. */
int mt_scene_set_materials(mt_scene *scene, const mt_material *materials, int n);
int mt_scene_get_materials(const mt_scene *scene, mt_material *out, int n);

/* MythTracer::RayTrace(WorkChunk*) (mythtracer.cc:280-312): renders the chunk
 * [chunk_x, chunk_x+chunk_w) x [chunk_y, chunk_y+chunk_h) of an image_w x
 * image_h image.  out_rgb: chunk_w*chunk_h*3 bytes, chunk-local row-major
 * RGB8 (WorkChunk::output_bitmap).  out_debug (nullable): chunk_w*chunk_h
 * entries (WorkChunk::output_debug).  max_depth = MAX_RECURSION_LEVEL (5). */
int mt_render_chunk(mt_scene *scene, const mt_sensor *sensor, int image_w,
                    int image_h, int chunk_x, int chunk_y, int chunk_w,
                    int chunk_h, int max_depth, uint8_t *out_rgb,
                    mt_debug_px *out_debug, mt_stats *stats);

/* Same, asynchronous, output left in HBM: d_rgb / d_debug are device pointers
 * on the scene's GPU, stream is a hipStream_t (NULL = default stream).  Work
 * counters accumulate in the scene and are fetched with mt_scene_read_stats
 * after the stream has been synchronised. */
int mt_render_chunk_device(mt_scene *scene, const mt_sensor *sensor,
                           int image_w, int image_h, int chunk_x, int chunk_y,
                           int chunk_w, int chunk_h, int max_depth,
                           void *d_rgb, void *d_debug, void *stream);

/* The master's work split (main_net_master.cc:195-221 GenerateWork, 128x128
 * WorkChunks) for a multi-GPU frame: the image is cut into tile_w x tile_h
 * tiles in row-major order; this call renders tiles first_tile,
 * first_tile+tile_stride, ... (n_tiles of them) in ONE launch.  Tile number j
 * of the call is written to d_rgb + j*tile_w*tile_h*3 as a chunk-local
 * row-major bitmap of its actual (edge-clipped) width x height, i.e. the PXLS
 * payload of that WorkChunk.  mt_blit_tiles_device is BlitWorkChunk
 * (main_net_master.cc:223-236) for such a buffer. */
int mt_render_tiles_device(mt_scene *scene, const mt_sensor *sensor,
                           int image_w, int image_h, int tile_w, int tile_h,
                           int first_tile, int tile_stride, int n_tiles,
                           int max_depth, void *d_rgb, void *stream);
int mt_blit_tiles_device(mt_scene *scene, int image_w, int image_h,
                         int tile_w, int tile_h, int first_tile,
                         int tile_stride, int n_tiles, const void *d_tiles,
                         void *d_image, void *stream);

/* Cost-balanced ownership of a multi-GPU frame's tiles.  The reference's master hands its WorkChunks out dynamically:
 * a worker asks for the next chunk when it is done with one (main_net_master.cc:62-80 the queue, :82-169
 * WorkerHandler), so no worker idles while chunks wait.  Ranks that render at the same time cannot pull from one
 * queue without a collective per tile; instead every rank computes THE SAME balanced assignment by itself from the
 * frame-wide cost map all ranks hold after their exchange (mt_scene_export_costs_device, all-reduce MAX): the tiles
 * sorted by the summed cost of their blocks, most expensive first (ties: lower tile number first), are dealt out in
 * rounds of alternating direction -- 0 1 .. N-1, N-1 .. 1 0, ... -- so that every rank holds one tile of every round:
 * the tile counts stay what the modular assignment gave (buffer sizes and the gather do not change) and the cost sums
 * differ by less than one tile of a round.
 *   mt_order_tiles_device: d_order[p] (int32, tiles_x * tiles_y entries) = tile at position p of that order, computed
 *     from d_cost_map (uint32 [map_h][map_w], one word per 8x8 block of the image) on the scene's GPU.  An all-zero map
 *     orders the tiles by number.
 *   mt_dealt_tile_count: how many tiles rank `rank` of `world` holds (host arithmetic, no device access).
 *   mt_deal_tiles_device: d_list[q] (int32) = the rank's tile of round q (d_order == NULL: the order by tile number);
 *     returns the count.
 *   mt_render_tile_list_device / mt_blit_tile_list_device: as the modular forms above with tile d_list[j] in slot j.
 *     list_id: launches with the same non-zero list_id promise the same list -- the scene then keeps its per-block
 *     cost history, running means included, as for any repeated launch; a launch with another list_id (or 0) takes its
 *     forecast from the cost map imported since the previous launch (mt_scene_import_costs_device; all ranks' costs by
 *     image position) and is a first frame without one.  The list is copied: the caller may reuse d_list at once.
 * Nothing computed for a pixel depends on the assignment: the gathered frame is byte-identical. */
int mt_order_tiles_device(mt_scene *scene, const void *d_cost_map, int map_w, int map_h,
                          int image_w, int image_h, int tile_w, int tile_h, void *d_order,
                          void *stream);
int mt_dealt_tile_count(int image_w, int image_h, int tile_w, int tile_h, int world, int rank);
int mt_deal_tiles_device(mt_scene *scene, const void *d_order, int image_w, int image_h,
                         int tile_w, int tile_h, int world, int rank, void *d_list, void *stream);
int mt_render_tile_list_device(mt_scene *scene, const mt_sensor *sensor, int image_w,
                               int image_h, int tile_w, int tile_h, const void *d_list,
                               int n_tiles, uint64_t list_id, int max_depth, void *d_rgb,
                               void *stream);
int mt_blit_tile_list_device(mt_scene *scene, int image_w, int image_h, int tile_w, int tile_h,
                             const void *d_list, int n_tiles, const void *d_tiles, void *d_image,
                             void *stream);

/* Supersampled frames: ss x ss samples per pixel, ss in 1 .. 4, resolved on the GPU.  (No reference counterpart: the
 * reference's pixel loop traces one ray per pixel, mythtracer.cc:292-305.)  The SAMPLE FRAME of an image_w x image_h
 * image is the frame of the plain calls at ss image_w x ss image_h for the same camera: Camera::GetSensor
 * (camera.cc:27-69) for that size puts its rays on an ss x ss grid inside every pixel of the image_w x image_h image.
 * Output pixel (x, y), channel c = (sum + n / 2) / n in unsigned integer arithmetic, n = ss ss, sum = the n sample
 * bytes at (ss x + i, ss y + j), 0 <= i, j < ss: the mean of the reference's bytes, rounded to nearest, ties up.
 * In these calls image_*, chunk_* and tile_* are the OUTPUT geometry, and `sensor` is the sensor OF THE SAMPLE GRID
 * (ss image_w x ss image_h).  Both sizes of the sample grid must stay within the 100000 the plain calls allow.
 *   mt_render_chunk_ss: as mt_render_chunk (no debug buffer).  The chunk (ss chunk_x, ss chunk_y, ss chunk_w,
 *     ss chunk_h) of the sample frame is rendered into a buffer the scene owns (ss ss chunk_w chunk_h 3 bytes, grown on
 *     demand; MT_ERR_NOMEM when it does not fit: never a lower ss instead) by ONE ordinary launch -- cost history,
 *     engine choice and forecasts work as for any repeated launch of that geometry -- and resolved; chunk_w chunk_h 3
 *     bytes come back.  stats counts the sample frame's work (rays_primary = ss ss chunk_w chunk_h); kernel_ms
 *     includes the resolve.
 *   mt_render_chunk_ss_device: the same, asynchronous, output left in HBM at d_rgb; stream ordering as for
 *     mt_render_chunk_device.
 *   mt_resolve_tiles_device: the building block of a multi-GPU supersampled frame.  A rank renders its tiles of the
 *     sample frame with mt_render_tiles_device or mt_render_tile_list_device at (ss image_w, ss image_h, ss tile_w,
 *     ss tile_h) -- the tile numbers are the same, the grid is the same -- into d_samples; this call resolves slot j
 *     of d_samples (ss ss tile_w tile_h 3 bytes each) into slot j of d_tiles (tile_w tile_h 3 bytes each: what the plain
 *     tile calls write at the output geometry), and the unchanged gather and blit at (image_w, image_h, tile_w, tile_h)
 *     finish the frame: the gather carries 1 / (ss ss) of the bytes.  d_list (nullable): the tile of slot j, as
 *     for mt_blit_tile_list_device; NULL: first_tile + j tile_stride.
 * ss = 1 is the plain call, through the plain call's path.  Argument checks come before any device call, ss and the
 * sample grid's size before everything else. */
int mt_render_chunk_ss(mt_scene *scene, const mt_sensor *sensor, int image_w, int image_h, int chunk_x,
                       int chunk_y, int chunk_w, int chunk_h, int ss, int max_depth, uint8_t *out_rgb,
                       mt_stats *stats);
int mt_render_chunk_ss_device(mt_scene *scene, const mt_sensor *sensor, int image_w, int image_h,
                              int chunk_x, int chunk_y, int chunk_w, int chunk_h, int ss, int max_depth,
                              void *d_rgb, void *stream);
int mt_resolve_tiles_device(mt_scene *scene, int image_w, int image_h, int tile_w, int tile_h,
                            int first_tile, int tile_stride, const void *d_list, int n_tiles, int ss,
                            const void *d_samples, void *d_tiles, void *stream);

/* Adaptive supersampling (Whitted's): one ray per pixel first, ss x ss samples only where neighbouring pixels differ.
 * (No reference counterpart.)  Everything is integer arithmetic on bytes the calls above already make:
 *   BLOCKS are the 8 x 8 grid of the IMAGE (not of the chunk): block (bx, by) covers [8 bx, 8 bx + 8) x [8 by, 8 by + 8)
 *     clipped to the image; its tile number is by ceil(image_w / 8) + bx -- the number the tile calls use at (image_w,
 *     image_h, 8, 8) and at (ss image_w, ss image_h, 8 ss, 8 ss).  The blocks OF A CHUNK are those with a chunk pixel:
 *     mask_x0 = chunk_x / 8, mask_w = (chunk_x + chunk_w - 1) / 8 - mask_x0 + 1, likewise in y; n_blocks = mask_w mask_h,
 *     row-major.
 *   CONTRAST: F = the chunk's plain frame (mt_render_chunk's bytes).  Two horizontal or vertical neighbours that BOTH
 *     lie in the chunk are a pair; a pair is contrasty when max over the channels of |F[p][c] - F[q][c]| > threshold
 *     (0 .. 255).  A block is REFINED iff a pixel of a contrasty pair lies in it: a pair across a block border refines
 *     both blocks.  Threshold 255 refines nothing.
 *   OUTPUT: the chunk's pixels in refined blocks are mt_render_chunk_ss's bytes (same ss, sensor_ss = the sensor of the
 *     sample grid), all others mt_render_chunk's (sensor = the sensor of the output grid).
 * Pairs across the chunk's border do not exist, so an adaptive chunk is THE ONE RESULT OF THIS LIBRARY THAT DEPENDS ON
 * HOW THE IMAGE WAS CUT INTO CHUNKS: chunks blitted together are not the adaptive frame of the whole image.
 *   mt_refine_mask_device: the building block, for a chunk bitmap already in HBM at d_rgb: d_mask (nullable) gets the
 *     n_blocks flags (0 / 1), d_list (int32, capacity n_blocks) the refined blocks' tile numbers IN ASCENDING ORDER -- an
 *     order-preserving compaction: the same bitmap gives the same list --, d_count (uint32) their number.  Asynchronous.
 *   mt_render_chunk_adaptive: (1) the plain launch into the output bitmap, exactly mt_render_chunk's; (2) mask and
 *     list; (3) the count and a hash of the list come back to the host: ONE STREAM SYNCHRONISATION in the middle of
 *     the call, because a launch sizes its buffers from a host-known number of tiles; (4) the scene's sample buffer is
 *     grown to n_refined 64 ss ss 3 bytes (MT_ERR_NOMEM when it does not fit: never a lower ss); (5) the refined blocks
 *     are rendered whole -- pixels outside the chunk included -- by one tile-list launch at (ss image_w, ss image_h,
 *     8 ss, 8 ss) with sensor_ss; (6) and resolved over the output bitmap.  Without refined blocks (4) - (6) do not run.
 *     The two launches keep SEPARATE cost histories: after the call the scene's history is what mt_render_chunk with
 *     the same arguments would have left (a following plain frame, mt_scene_export_costs_device and the next adaptive
 *     call's plain launch see that); the refinement launch runs on measured costs when the previous refinement of the
 *     same geometry had the same list (list_id = hash | 1), else it is a launch without history.
 *     mt_scene_set_scheduling, mt_scene_set_engine and mt_scene_set_tuning forget both histories.
 *     out_mask (nullable): n_blocks bytes.  stats: the work counters are the sums of both launches -- rays_primary =
 *     chunk_w chunk_h + ss ss (sum of area(refined block within the image)) --, kernel_ms all kernels of the call by
 *     events (the synchronisation's idle time excluded), total_ms the wall time.  mt_scene_kernel_times reports the
 *     plain launch and then the refinement launch, TWO entries (one without refined blocks).
 *   mt_render_chunk_adaptive_device: the same with d_rgb / d_mask in HBM and no stats.  NOT fully asynchronous: it
 *     synchronises `stream` once (step 3) and returns with steps (5) - (6) queued.
 * ss = 1 is the plain call through the plain call's path: an all-zero mask, n_refined 0.  Argument checks come before
 * any device call, in this order: ss and the sample grid, threshold, the output pointer, image and chunk, the scene,
 * the sensors (sensor_ss may be NULL with ss = 1 only). */
typedef struct mt_adaptive_info {
  int32_t n_blocks;        /* blocks of the chunk (mask_w * mask_h) */
  int32_t n_refined;       /* of them refined */
  int32_t plain_history;   /* 1: the plain launch took its work order from measured costs */
  int32_t refine_history;  /* the same for the refinement launch; 0 also when n_refined == 0 */
} mt_adaptive_info;
int mt_refine_mask_device(mt_scene *scene, int image_w, int image_h, int chunk_x, int chunk_y, int chunk_w,
                          int chunk_h, int threshold, const void *d_rgb, void *d_mask, void *d_list,
                          void *d_count, void *stream);
int mt_render_chunk_adaptive(mt_scene *scene, const mt_sensor *sensor, const mt_sensor *sensor_ss, int image_w,
                             int image_h, int chunk_x, int chunk_y, int chunk_w, int chunk_h, int ss, int threshold,
                             int max_depth, uint8_t *out_rgb, uint8_t *out_mask, mt_adaptive_info *info,
                             mt_stats *stats);
int mt_render_chunk_adaptive_device(mt_scene *scene, const mt_sensor *sensor, const mt_sensor *sensor_ss,
                                    int image_w, int image_h, int chunk_x, int chunk_y, int chunk_w, int chunk_h,
                                    int ss, int threshold, int max_depth, void *d_rgb, void *d_mask,
                                    mt_adaptive_info *info, void *stream);

/* The primary-hit G-buffer of a chunk: what the first call of TraceRayWorker (mythtracer.cc:18-64) knows about a pixel
 * before it looks at a light, as separate planes.  (No reference counterpart: the reference returns a colour and
 * PerPixelDebugInfo only.)  Per pixel, with the frame kernels' arithmetic: Sensor::GetRay (camera.cc:65-69),
 * OctTree::IntersectRay from the camera origin, and on a hit
 *   depth     the hit distance t along the normalised ray
 *   point     origin + direction t (primitive_triangle.cc:141; mt_debug_px::point)
 *   normal    Triangle::GetNormal(point) (primitive_triangle.cc) -- as returned, NOT flipped towards the camera
 *             (mythtracer.cc:42-45 flips its own copy afterwards)
 *   uvw       Triangle::GetUVW(point) (primitive_triangle.cc)
 *   albedo    material.ambient, times Texture::GetColorAt(uvw.x, uvw.y) where the material has a texture
 *             (mythtracer.cc:58-64): the unlit surface colour
 *   prim      the AddPrimitive index (mt_scene_desc::tri_id; scenes created without tri_id cannot give this plane)
 *   line_no   Primitive::debug_line_no (mt_debug_px::line_no)
 *   material  index into mt_scene_desc::materials, -1 = no material (albedo is then NaN)
 * depth is 1 double per pixel, point / normal / uvw / albedo 3 interleaved doubles, the others 1 int32; every plane is
 * chunk-local row-major.  A miss: NaN in the double planes, -1 in the int32 planes.  Every pointer is nullable -- a
 * plane nobody asked for is neither computed nor written -- but at least one must be set.
 *   mt_render_gbuffer: `out` holds HOST pointers; stats (nullable): rays_primary = chunk pixels, shaded_hits = hits,
 *     the traversal's counters, kernel_ms = the kernel by HIP events, total_ms = wall time of the call.
 *   mt_render_gbuffer_device: `d_out` (a host struct) holds DEVICE pointers on the scene's GPU; asynchronous on
 *     `stream`; counters as for mt_render_chunk_device.
 * One kernel next to the frame kernels (mt::gbuffer_kernel).  The calls leave everything a frame launch decides by --
 * cost history, engine choice, forecasts, mt_scene_kernel_times -- alone: a frame after a G-buffer call is the
 * repeated launch it would have been without it.  Argument checks come before any device call, in this order: `out`,
 * image size and chunk (mt_render_chunk's limits and messages), scene, sensor. */
typedef struct mt_gbuffer {
  double *depth, *point, *normal, *uvw, *albedo;
  int32_t *prim, *line_no, *material;
} mt_gbuffer;
int mt_render_gbuffer(mt_scene *scene, const mt_sensor *sensor, int image_w, int image_h,
                      int chunk_x, int chunk_y, int chunk_w, int chunk_h,
                      const mt_gbuffer *out, mt_stats *stats);
int mt_render_gbuffer_device(mt_scene *scene, const mt_sensor *sensor, int image_w, int image_h,
                             int chunk_x, int chunk_y, int chunk_w, int chunk_h,
                             const mt_gbuffer *d_out, void *stream);

/* The direct-light buffer of a chunk and the deferred relight pass: the direct term of TraceRayWorker
 * (mythtracer.cc:38-177) cut where geometry ends and light colours begin.  (No reference counterpart.)
 *
 * mt_render_lightbuffer runs, for every pixel of the chunk and every light of the scene (mt_scene_set_lights, in light
 * order), the shadow loop of mythtracer.cc:90-156 -- from the primary hit towards the light, through every transparent
 * occluder -- with the frame kernels' arithmetic, and stores what the loop leaves behind:
 *   power      [n_lights][chunk_h][chunk_w][3] doubles: light_power when the loop of that light ends, BEFORE
 *              mythtracer.cc:159-161 raise it to light.ambient
 *   in_shadow  [n_lights][chunk_h][chunk_w] bytes: 0 = lit, 1 = in_shadow, 255 = no light loop ran for this pixel
 * Pixels for which the reference never enters the light loop -- a miss (:23-31) or a hit on a triangle without a
 * material (:49-52) -- get NaN in power and 255 in in_shadow.  An OCCLUDER without a material counts as opaque, as in
 * the frame kernels (the reference dereferences its NULL mtl, :121).  Both planes depend on geometry, materials and the
 * lights' POSITIONS only: not on any light's ambient, diffuse or specular.  Each pointer of `lb` is nullable -- a plane
 * nobody asked for is not written -- but at least one must be set.  `gb` (nullable, and each of its pointers too): the
 * G-buffer planes requested through it are written by the same launch from the same primary trace, with the bits
 * mt_render_gbuffer gives: one call delivers everything a relight needs.  With zero lights set the light-buffer planes
 * are empty (nothing is written through `lb`) and the call is valid only if a plane of `gb` is requested: MT_ERR_ARG
 * otherwise.
 *   mt_render_lightbuffer: host pointers; stats (nullable): rays_primary = chunk pixels, rays_shadow = iterations of
 *     the shadow loops, shaded_hits = primary hits, the traversal's counters, kernel_ms = the kernel by HIP events,
 *     total_ms = wall time of the call.
 *   mt_render_lightbuffer_device: `d_gb` / `d_lb` (host structs) hold DEVICE pointers on the scene's GPU; asynchronous
 *     on `stream`; counters as for mt_render_chunk_device.
 * One kernel next to the frame kernels (mt::lightbuffer_kernel).  Like the G-buffer calls these leave everything a frame
 * launch decides by -- cost history, engine choice, forecasts, mt_scene_kernel_times -- alone.
 *
 * mt_shade_direct evaluates mythtracer.cc:38-177 per pixel from stored planes, without any traversal, in the
 * reference's order of operations: the pixel's ray from `sensor` (Sensor::GetRay); towards_camera and the normal flip of
 * :40-45 applied to the stored (unflipped) normal; the grey of :49-52 where material == -1 on a hit; black for a miss
 * (a miss <=> point[0] is NaN); reflected_direction (:68-69); then per light, in the order of `lights`:
 * light_direction = Norm(position - point); colour += ambient * albedo; lp = max(power, ambient) per channel;
 * colour += material.diffuse * albedo * dot(light_direction, normal) * diffuse * lp; and, where in_shadow == 0 and
 * dot(reflected_direction, towards_camera) > 0, the specular term of :169-177; finally V3DtoRGB (:235-241).  Material
 * constants come from the scene.  It needs the point, normal, albedo and material planes of the G-buffer and both planes
 * of the light buffer, all of the same chunk of the same image for the same sensor.
 * `lights` (a HOST array in both forms; the scene's own lights are neither read nor changed) may differ from the lights
 * the light buffer was made with in ambient, diffuse and specular ONLY: the count and every position must be the same.
 * Neither is checked -- the calls are stateless, the planes carry no record of their lights.  A MOVED light needs new
 * planes: mt_update_lightbuffer (below) traces those of the moved lights again from the stored G-buffer and leaves the
 * others alone.  A value of the material plane outside the scene's materials (planes of another scene) is shaded as
 * "no material".
 * CONTRACT: for unchanged positions the bitmap is byte-identical to mt_render_chunk(..., max_depth = 0, ...) after
 * mt_scene_set_lights(lights, n_lights).
 *   mt_shade_direct_device: device pointers in `d_gb`, `d_lb` and `d_rgb` (chunk_w * chunk_h * 3 bytes); asynchronous
 *     on `stream`.  Up to 8 lights travel with the launch; a longer `lights` array is copied by the stream, into a buffer
 *     the scene owns, and must stay unchanged until the stream has reached the call.
 * As for every call on an mt_scene, one call may be in flight per scene at a time: the *_device forms of one scene go to
 * ONE stream (or are ordered by the caller) -- they share the scene's work counter, statistics and that light buffer.
 *   mt_shade_direct: host pointers; stats (nullable): kernel_ms = mt::shade_direct_kernel by HIP events, total_ms =
 *     wall time of the call with its copies; the work counters are zero (no ray is traced).
 *
 * Argument checks come before any device call, in this order: the `lb` and `gb` pointers (and, for mt_shade_direct, the
 * bitmap), image size and chunk (mt_render_chunk's limits and messages), scene, sensor, lights. */
typedef struct mt_lightbuffer {
  double *power;
  uint8_t *in_shadow;
} mt_lightbuffer;
int mt_render_lightbuffer(mt_scene *scene, const mt_sensor *sensor, int image_w, int image_h,
                          int chunk_x, int chunk_y, int chunk_w, int chunk_h,
                          const mt_gbuffer *gb, const mt_lightbuffer *lb, mt_stats *stats);
int mt_render_lightbuffer_device(mt_scene *scene, const mt_sensor *sensor, int image_w, int image_h,
                                 int chunk_x, int chunk_y, int chunk_w, int chunk_h,
                                 const mt_gbuffer *d_gb, const mt_lightbuffer *d_lb, void *stream);
int mt_shade_direct(mt_scene *scene, const mt_sensor *sensor, int image_w, int image_h,
                    int chunk_x, int chunk_y, int chunk_w, int chunk_h,
                    const mt_gbuffer *gb, const mt_lightbuffer *lb, const mt_light *lights, int n_lights,
                    uint8_t *out_rgb, mt_stats *stats);
int mt_shade_direct_device(mt_scene *scene, const mt_sensor *sensor, int image_w, int image_h,
                           int chunk_x, int chunk_y, int chunk_w, int chunk_h,
                           const mt_gbuffer *d_gb, const mt_lightbuffer *d_lb, const mt_light *lights,
                           int n_lights, void *d_rgb, void *stream);

/* The light-buffer planes of the LISTED lights again, after those lights have MOVED: the shadow loop depends on the
 * primary hit point, on whether the hit has a material and on the light's position only, and the first two are stored
 * bit for bit in the G-buffer's `point` and `material` planes.  No sensor, no image geometry: nothing here depends on
 * the camera once the point is stored, and no primary ray is traced.
 *   gb   read, not written: `point` (3 doubles per pixel) and `material` (int32) of the chunk; other planes ignored.
 *   lb   mt_render_lightbuffer's layout for the scene's CURRENT lights (mt_scene_set_lights):
 *        [n_lights][chunk_h][chunk_w]; each pointer nullable, at least one set.
 *   light_idx, n_idx   the lights to trace again (indices into the scene's lights, each at most once, any order): a
 *        HOST array in both forms.
 * For every listed light l and every pixel with point[0] not NaN and 0 <= material < the scene's material count, the
 * shadow loop runs exactly as for mt_render_lightbuffer (the same operations in the same order) under the scene's light l, and
 * power / in_shadow are stored in plane l.  Every other pixel gets NaN and 255 in plane l -- a material index outside
 * the scene's materials included, as for mt_shade_direct.  Planes of unlisted lights are not written, not one byte; in
 * the host form their host memory is not written (or read) either.
 * CONTRACT: after mt_scene_set_lights(B), planes made under lights A -- same count, positions different at the listed
 * indices only -- updated from the same chunk's point and material are bit-identical to mt_render_lightbuffer under B
 * (power with NaN = NaN, in_shadow byte for byte).
 *   mt_update_lightbuffer: host pointers; stats (nullable): rays_primary = shaded_hits = rays_secondary = 0,
 *     rays_shadow = loop iterations of the listed lights, the traversal's counters, kernel_ms = the kernel by HIP
 *     events, total_ms = wall time of the call.
 *   mt_update_lightbuffer_device: device pointers in `d_gb` / `d_lb`; asynchronous on `stream`; counters as for
 *     mt_render_chunk_device.  Up to 8 indices travel with the launch; a longer list is copied by the stream into a
 *     buffer the scene owns and must stay unchanged until the stream has reached the call.  One call in flight per
 *     scene, as for its siblings (they share the work counter and the statistics).
 * One kernel next to the frame kernels (mt::lightbuffer_update_kernel; a work item is an 8x8 block of the chunk x one
 * listed light); cost history, engine choice, forecasts and mt_scene_kernel_times are left alone.
 * Argument checks come before any device call, in this order: `lb` (NULL, no plane), `gb` (NULL, point or material
 * missing), chunk_w and chunk_h in 1 .. 100000, scene, the list (n_idx <= 0 or NULL), an index outside
 * 0 .. n_lights - 1, an index listed twice. */
int mt_update_lightbuffer(mt_scene *scene, int chunk_w, int chunk_h,
                          const mt_gbuffer *gb, const int32_t *light_idx, int n_idx,
                          const mt_lightbuffer *lb, mt_stats *stats);
int mt_update_lightbuffer_device(mt_scene *scene, int chunk_w, int chunk_h,
                                 const mt_gbuffer *d_gb, const int32_t *light_idx, int n_idx,
                                 const mt_lightbuffer *d_lb, void *stream);

/* The ray-tree buffer of a chunk: the whole call tree of TraceRayWorker (mythtracer.cc:13-228) for every pixel, traced
 * once and kept in HBM, and the relight pass over it -- the FULL-DEPTH frame under edited light colours without tracing
 * a ray.  Nothing in the shape of the recursion depends on a light's colour: whether a call spawns a reflected child
 * (:181-184) or a refracted one (:192) depends on level, the material's reflectance and transparency,
 * current_reflection_coef and in_object; the rays, their hits and every shadow loop depend on geometry, materials and
 * the lights' POSITIONS.  (No reference counterpart.)
 *
 * Layers, for a given max_depth (which stands where the reference has MAX_RECURSION_LEVEL):
 *   layer 0      one ray per pixel of the chunk: Sensor::GetRay, level 0, in_object = false, coef = 1.0
 *   layer k + 1  the child rays of layer k's rays: the reflected ray of :68-74 (origin = point + direction * 0.0001, the
 *                direction NOT normalised) where :181-184 holds, the refracted ray of :208-218 where :192 holds; ordered
 *                by parent index, a parent's reflected ray before its refracted one; in_object and coef as the recursive
 *                call receives them (:186-187, :222-223)
 * A miss and a hit on a triangle without a material have no children.  Layers end before the first empty one: there are
 * at most max_depth + 1, and a layer's rays are the calls of TraceRayWorker at that level.
 * Order of layer 0: the 8x8-pixel blocks of the CHUNK (block (0, 0) at the chunk's corner) in row-major order; within a
 * block its pixels in row-major order; a block cut by the chunk's right or bottom edge holds only its pixels, so the list
 * has chunk_w * chunk_h entries and no holes.  Chunk pixel (x, y), with bw = min(8, chunk_w - 8 (x / 8)) and
 * bh = min(8, chunk_h - 8 (y / 8)), has index  8 (y / 8) chunk_w + 8 (x / 8) bh + (y % 8) bw + x % 8.  A fixed function
 * of (chunk_w, chunk_h); mythtracer_amd/tiling.py restates it (raytree_layer0_order).
 *
 * Per ray of a layer of n rays (mt_raytree_layer: the planes mt_raytree_read_layer copies out, each pointer nullable):
 *   ray        [n][6] doubles: origin and direction exactly as handed to OctTree::IntersectRay
 *   in_object  [n] bytes 0 / 1;   coef  [n] doubles
 *   point, normal, albedo  [n][3] doubles, material [n] int32: mt_render_gbuffer's planes for that ray, with its bits
 *              (normal unflipped; a miss: NaN / -1; no material: albedo NaN, material -1)
 *   power      [n_lights][n][3] doubles, in_shadow [n_lights][n] bytes: mt_render_lightbuffer's meaning and its
 *              NaN / 255 rule for rays that never enter the light loop
 *   child_refl, child_refr  [n] int32: index into layer k + 1, -1 = none
 *   pixel      [n] int32, LAYER 0 ONLY (MT_ERR_ARG for another layer): the ray's chunk-local row-major pixel index
 *
 * mt_raytree_create traces the tree under the scene's CURRENT lights (mt_scene_set_lights; zero lights is valid: the
 * light planes are empty) and returns it, or NULL with mt_last_error set.  The tree is opaque and lives on the scene's
 * GPU.  The call is synchronous and makes one host round trip per layer: a layer's child count sizes the next one.
 * stats (nullable): the sums over all layers -- rays_primary, rays_secondary, rays_shadow and shaded_hits equal what
 * mt_render_chunk reports for the same frame --, kernel_ms = device time from the first to the last kernel (the round
 * trips between the layers included), total_ms = wall time.  A layer of 2^31 rays or more is MT_ERR_UNSUPPORTED; an
 * allocation that does not fit is MT_ERR_NOMEM (never a shallower tree); a tripped loop bound is MT_ERR_INTERNAL.
 * mt_raytree_destroy (NULL is fine) must be called BEFORE the scene's mt_scene_destroy; trees of one scene may be
 * destroyed in any order.  mt_raytree_info fills an mt_raytree_desc: layers, lights, chunk, depth, rays per layer, bytes.
 *
 * mt_raytree_shade shades the layers bottom-up, one thread per ray and one launch per layer.  Per ray: colour = the
 * direct term of :38-177 from the stored planes, the stored ray direction and the CALLER's lights -- mt_shade_direct's
 * arithmetic, grey for material == -1 and black for a miss included --; where child_refl >= 0
 * colour += colour[child_refl] * reflectance (:185-188); where child_refr >= 0
 * colour += colour[child_refr] * transmission_filter * transparency, associated as :220-224 writes it; layer 0 ends in
 * V3DtoRGB (:235-241), written to the pixel's place of the chunk-local row-major bitmap.  Material constants come from
 * the scene.  `lights` is a HOST array in both forms; the scene's own lights are neither read nor changed.  They may
 * differ from the lights the tree was made with in ambient, diffuse and specular ONLY; of that, the count is checked
 * (MT_ERR_ARG), the positions cannot be.
 * CONTRACT: for lights whose count and positions are those the tree was made with, the bitmap is byte-identical to
 * mt_render_chunk(..., max_depth, ...) after mt_scene_set_lights(lights, n_lights), for the same scene, sensor and chunk.
 *   mt_raytree_shade: out_rgb = chunk_w * chunk_h * 3 host bytes; stats (nullable): kernel_ms = the layers' launches
 *     by HIP events, total_ms = wall time of the call; the work counters are zero (no ray is traced).
 *   mt_raytree_shade_device: d_rgb on the scene's GPU; asynchronous on `stream`.  Up to 8 lights travel with the
 *     launches; a longer array is copied by the stream into a buffer the scene owns and must stay unchanged until the
 *     stream has reached the call.
 * The per-ray colours are scratch of the TREE: one shade may be in flight per tree.  All calls share the scene's work
 * counter, statistics and light buffer with their siblings: one call in flight per scene.  Like the G-buffer and
 * light-buffer calls they leave everything a frame launch decides by -- cost history, engine choice, forecasts,
 * mt_scene_kernel_times -- alone.
 *
 * Argument checks come before any device call, in this order.  mt_raytree_create: image size and chunk
 * (mt_render_chunk's limits and messages), scene, sensor, max_depth in 0 .. MT_MAX_RECURSION.  mt_raytree_info: tree,
 * out.  mt_raytree_read_layer: tree, layer in 0 .. n_layers - 1, out, `pixel` for a layer other than 0.
 * mt_raytree_shade[_device]: the bitmap, tree, then the lights (n_lights < 0 or a NULL array of n_lights > 0; n_lights
 * unequal to the tree's), and last a tree that is stale after mt_scene_set_materials (mt_raytree_update_materials). */
typedef struct mt_raytree mt_raytree;
typedef struct mt_raytree_desc {
  int32_t n_layers, n_lights;
  int32_t image_w, image_h, chunk_x, chunk_y, chunk_w, chunk_h;
  int32_t max_depth, from_rays;           /* 0: made from a sensor (mt_raytree_create), 1: from a ray list */
  int64_t n_rays[MT_MAX_RECURSION + 1];   /* per layer; 0 from n_layers on */
  double trace_ms[MT_MAX_RECURSION + 1];  /* per layer: its tracing kernel at creation, by HIP events */
  uint64_t bytes;                          /* HBM held by the tree */
} mt_raytree_desc;
typedef struct mt_raytree_layer {
  double *ray;
  uint8_t *in_object;
  double *coef;
  double *point, *normal, *albedo;
  int32_t *material;
  double *power;
  uint8_t *in_shadow;
  int32_t *child_refl, *child_refr;
  int32_t *pixel;
} mt_raytree_layer;
mt_raytree *mt_raytree_create(mt_scene *scene, const mt_sensor *sensor, int image_w, int image_h,
                              int chunk_x, int chunk_y, int chunk_w, int chunk_h, int max_depth, mt_stats *stats);
void mt_raytree_destroy(mt_raytree *tree);
int mt_raytree_info(const mt_raytree *tree, mt_raytree_desc *out);
int mt_raytree_read_layer(mt_raytree *tree, int layer, const mt_raytree_layer *out);
int mt_raytree_shade(mt_raytree *tree, const mt_light *lights, int n_lights, uint8_t *out_rgb, mt_stats *stats);
int mt_raytree_shade_device(mt_raytree *tree, const mt_light *lights, int n_lights, void *d_rgb, void *stream);

/* A moved light: the planes of the listed lights again in EVERY layer of a ray tree, from the tree's own stored hits.
 * The shape of the tree does not depend on the lights -- rays, hits, G-buffer planes and child indices of all layers
 * stay as they are --, so a light that moved since the tree was made costs its shadow loops and nothing else: no
 * sensor is used, no primary or secondary ray is traced.  (No reference counterpart; mt_update_lightbuffer's
 * counterpart at depth.)
 * For every listed light l, every layer k and every ray i of that layer with point[i][0] not NaN and
 * 0 <= material[i] < the scene's material count, the shadow loop of mythtracer.cc:90-156 runs from the stored point
 * under the scene's CURRENT light l (mt_scene_set_lights), exactly as mt_raytree_create runs it (the same operations
 * in the same order), and power / in_shadow are stored at [l][i] of that layer.  Every other ray of the layer gets NaN
 * and 255 there.  Planes of unlisted lights are not written, not one byte, and nothing else in the tree is: not rays,
 * G-buffer planes, child indices or `pixel`.
 * CONTRACT: a tree made under lights A, after mt_scene_set_lights(B) -- same count, positions different at the listed
 * indices only -- and an update at those indices, is bit-identical in every plane of every layer to mt_raytree_create
 * under B for the same scene, sensor, chunk and max_depth (power with NaN = NaN, bytes and indices exactly); so
 * mt_raytree_shade(tree, B) is mt_render_chunk(..., max_depth, ...) under B byte for byte.
 * `light_idx` is a HOST array in both forms; each index at most once, in any order.
 *   mt_raytree_update_lights: synchronous.  stats (nullable): rays_primary = rays_secondary = shaded_hits = 0,
 *     rays_shadow = the loop iterations of the listed lights over all layers, the traversal's counters, kernel_ms =
 *     the kernel by HIP events, total_ms = wall time of the call; with stats set the counters are switched on for the
 *     call.  A tripped loop bound is MT_ERR_INTERNAL.
 *   mt_raytree_update_lights_device: fully asynchronous on `stream` -- no synchronisation, no read-back; counters as
 *     for mt_render_chunk_device.  Up to 8 indices travel with the launch; a longer list is copied by the stream into a
 *     buffer the scene owns and must stay unchanged until the stream has reached the call.
 * One kernel next to the frame kernels, ONE launch for all layers and all listed lights (mt::raytree_update_kernel; a
 * work item is 64 consecutive rays of one layer x one listed light); more than 0xfffffff0 items are MT_ERR_ARG.  One
 * call in flight per scene and per tree, as for the siblings (they share the work counter and the statistics); cost
 * history, engine choice, forecasts and mt_scene_kernel_times are left alone.
 * Argument checks come before any device call, in this order: the tree (NULL), the list (n_idx <= 0 or NULL), the
 * scene's current light count unequal to the tree's, an index outside 0 .. n_lights - 1, an index listed twice, and
 * last a tree that is stale after mt_scene_set_materials (mt_raytree_update_materials).  All are MT_ERR_ARG; a tree of
 * zero lights refuses every list. */
int mt_raytree_update_lights(mt_raytree *tree, const int32_t *light_idx, int n_idx, mt_stats *stats);
int mt_raytree_update_lights_device(mt_raytree *tree, const int32_t *light_idx, int n_idx, void *stream);

/* Edited materials: a ray tree brought to the scene's CURRENT materials (mt_scene_set_materials) without tracing a
 * primary or secondary ray -- or refused, and then left exactly as it was.  (No reference counterpart.)
 * What a stored tree holds that depends on a material: albedo (the material's ambient, times the texel where it has a
 * texture), coef (products of reflectance along the path), the child conditions (reflectance > 0, coef > 0.01,
 * transparency > 0) and the light planes (transparency and transmission_filter of whatever a shadow ray crosses).
 * Rays, hits, point, normal, material, in_object and pixel depend on no material.
 * A tree remembers the materials it is valid for -- a host snapshot and the scene's generation, taken at creation and
 * after each successful update.  After a mt_scene_set_materials that changed something, every tree of the scene is
 * STALE: mt_raytree_shade[_device], mt_raytree_shade_colors[_device] and mt_raytree_update_lights[_device] refuse it with
 * MT_ERR_ARG -- the LAST of each call's checks, after those listed above --; mt_raytree_info, _read_layer and _destroy
 * keep working, and its planes are still the old materials' planes, untouched.
 * The call: (1) tree NULL is MT_ERR_ARG; (2) equal generations: MT_OK, no device call, stats all zero; (3) the
 * snapshot is compared with the scene's host copy, per material, doubles by their bits.
 *   diffuse, specular, specular_exp, refraction_index, and transmission_filter of a material whose transparency is 0
 *     before and after: nothing to do, the shade reads them from the scene.  No kernel is launched.
 *   ambient or tex: where the material has a texture before or after the edit, MT_ERR_UNSUPPORTED before any device
 *     call (the tree keeps neither the texel nor the primitive) -- unless the tree keeps uvw, see
 *     mt_scene_set_raytree_uvw below, which lifts this refusal.  Otherwise every ray whose material it is gets
 *     albedo = ambient, which is what the tracing kernel stores for an untextured material.
 *   reflectance or transparency, of any material: the tree's shape may or may not survive.  A CHECK pass
 *     (mt::raytree_recoef_kernel, one launch per layer, top-down) carries every ray's coefficient under the new
 *     materials down the tree in the tree's scratch colours and evaluates the two child conditions exactly as the
 *     tracing kernel does; a ray whose conditions differ from the children it has, in either direction, is counted.
 *     The host reads the count: non-zero is MT_ERR_UNSUPPORTED with the count, and the layer and index of the first
 *     such ray (the lowest layer, in it the lowest index), in the message; nothing but scratch has been written.
 *   then the COMMIT (mt::raytree_recommit_kernel, one launch per layer that has something to take): the new
 *     coefficients into coef of layers >= 1, the new ambient into albedo.
 *   transparency of any material, or transmission_filter of one whose transparency is not 0 before or after: a shadow
 *     ray may cross it whether or not a ray of the tree hits it, so after the commit the planes of ALL lights are
 *     traced again in all layers under the scene's current lights, by mt_raytree_update_lights's kernel over the
 *     indices 0 .. n_lights - 1 (the scene's light count must be the tree's: MT_ERR_ARG before any device call).  A
 *     tree of zero lights skips this.  Composed with a moved light: if a light moved since the tree's planes were
 *     made (mt_scene_set_lights without mt_raytree_update_lights), this re-trace brings the planes of EVERY light to
 *     the scene's current positions, so a following mt_raytree_update_lights over the moved index changes no bit;
 *     an update that runs no re-trace leaves the old positions' planes, and the tree is then the fresh tree under the
 *     new materials and the OLD positions until mt_raytree_update_lights is called.
 * CONTRACT: the update succeeds exactly when mt_raytree_create[_rays] under the new materials has the same rays per
 * layer and the same child indices, and no textured material changed ambient or tex.  After a successful update the
 * tree is bit-identical in every plane of every layer to that fresh tree (doubles with NaN = NaN, bytes and indices
 * exactly), so mt_raytree_shade on it is mt_render_chunk(..., max_depth, ...) under the new materials byte for byte.
 * After a refused update the tree's planes are bit-identical to what they were and the tree is still stale; setting
 * the old materials back and updating again succeeds, with no launch beyond what that second comparison asks for.
 * Synchronous; there is no _device form (the check pass needs its read-back, as mt_raytree_create does).  The scratch
 * colours are the shade's: one shade OR one update in flight per tree, one call in flight per scene.  stats (nullable):
 * rays_shadow and the traversal's counters from the light re-trace, if one ran (the counters are switched on for
 * it); rays_primary = rays_secondary = shaded_hits = 0; kernel_ms = from the first to the last kernel by the tree's
 * events (the check's read-back included), 0 when none ran; total_ms = wall time.  A tripped loop bound in the
 * re-trace is MT_ERR_INTERNAL (a kernel logic error: the tree stays stale).  Cost history, engine choice and
 * forecasts are left alone. */
int mt_raytree_update_materials(mt_raytree *tree, mt_stats *stats);

/* Edited materials that change the tree's SHAPE: a stale ray tree brought to the scene's CURRENT materials whatever the
 * edit does to the child conditions -- a matte surface made reflective, a mirror switched off, a pane made opaque, a
 * reflectance lowered until a deep bounce falls under coef > 0.01.  Where mt_raytree_update_materials refuses, this call
 * keeps the rays that survive, drops the dead subtrees, traces only the new ones and knits the layers back into the
 * order mt_raytree_create produces (by parent index, the reflected child before the refracted one).  (No reference
 * counterpart.)  mt_raytree_update_materials itself is unchanged and keeps refusing such an edit.
 * A ray of the new tree is KEPT when its path exists in the old tree: every ray of layer 0; a child whose parent is kept
 * and whose OLD parent had a child in the same slot (reflected / refracted).  Every other ray of the new tree is TRACED.
 * A kept ray takes ray, in_object, point, normal, material and its light planes from the old tree, its coef and child
 * conditions from the new materials, its albedo from the old tree or -- where its material's ambient changed -- the new
 * ambient.  A traced ray is spawned from its parent's stored hit and traced by the kernel mt_raytree_create uses, in a
 * dense list of the layer's traced rays (a work item is 64 consecutive ones).
 * Steps and checks, in this order; the first four come before any device call.
 *   (1) tree NULL: MT_ERR_ARG.
 *   (2) equal generations: MT_OK, no device call; info and stats all zero except n_layers_before = n_layers_after.
 *   (3) ambient or tex of a material that has a texture before or after the edit: MT_ERR_UNSUPPORTED with
 *       mt_raytree_update_materials's message (kept rays hold neither the texel nor the primitive); not for a tree that
 *       keeps uvw (mt_scene_set_raytree_uvw below).
 *   (4) a reflectance or transparency changed, or the edit is one a shadow ray may see (mt_raytree_update_materials's
 *       rule), the tree has lights, and the scene's light count is not the tree's: MT_ERR_ARG with
 *       mt_raytree_update_materials's message.  Stricter than that call: traced rays get their light planes from the
 *       scene's current lights.
 *   (5) mt_raytree_update_materials's check pass, where a reflectance or transparency changed.  With no mismatch the
 *       call continues exactly as mt_raytree_update_materials does (commit, light re-trace where a shadow ray may see
 *       the edit): regrown = 0, kept = the rays per layer, traced = dropped = 0.
 *   (6) otherwise the tree is regrown (a tree of ZERO lights under a scene that now has lights is MT_ERR_ARG here, with
 *       (4)'s message and the tree untouched: the tracing kernel would run the scene's lights): regrown = 1; and where a shadow ray may see the edit, the planes of ALL lights
 *       are then traced again over the whole new tree (mt_raytree_update_lights's kernel, one launch), the traced
 *       rays' a second time.
 * CONTRACT: after MT_OK the tree is bit-identical to mt_raytree_create[_rays] under the new materials and the scene's
 * current lights, for the same sensor / ray list, chunk and max_depth: every plane of every layer (doubles with
 * NaN = NaN, bytes and indices exactly, `pixel` in layer 0), and n_layers, n_rays and bytes of mt_raytree_info.  The
 * tree is fresh: mt_raytree_shade on it is mt_render_chunk(..., max_depth, ...) under the new materials byte for byte,
 * and mt_raytree_update_lights works on it.  trace_ms[k] becomes the device time of this call's tracing launch for
 * layer k, 0 where no ray of that layer was traced.
 * Light POSITIONS cannot be checked, as everywhere in this family.  If lights moved between the tree's last valid state
 * and the call, kept rays hold the old positions' planes and traced rays the new ones; mt_raytree_update_lights over
 * the moved indices after the regrow makes the tree the fresh tree under the new lights.
 * Failure: the new layers >= 1 are built ASIDE, and so are layer 0's child indices; its albedo waits.  The old tree's
 * planes are written only after the last step that can fail for size -- an allocation that does not fit is
 * MT_ERR_NOMEM, a layer of 2^31 rays or more MT_ERR_UNSUPPORTED with mt_raytree_create's message --, and after such a
 * failure the tree is bit-identical to what it was and still stale.  A tripped loop bound in a tracing launch is
 * MT_ERR_INTERNAL with the tree as it was; in the light re-trace it is MT_ERR_INTERNAL and the tree stays stale, as for
 * mt_raytree_update_materials.
 * info (nullable): kept and traced per layer of the NEW tree (kept + traced = the new n_rays), dropped per layer of the
 * OLD tree (its rays with no place in the new one).  stats (nullable; the counters are switched on for the call):
 * rays_primary = 0, rays_secondary = the sum of traced, shaded_hits = the hits among the traced rays, rays_shadow = the
 * shadow-loop iterations of the traced rays plus, where it ran, those of the all-lights re-trace; kernel_ms = from the
 * first to the last kernel by the tree's events, read-backs included; total_ms = wall time.
 * Synchronous; there is no _device form (the layer sizes need a read-back, as in mt_raytree_create).  The tree keeps
 * the scratch it needed (an index per ray of the two largest new layers, layer 0's child indices, the dense list) for
 * the next call; mt_raytree_info's bytes does not count it.  One call in flight per tree and per scene; cost history,
 * engine choice, forecasts and mt_scene_kernel_times are left alone.  (mt::raytree_regrow_*_kernel in mt_raytree.h.) */
typedef struct mt_raytree_regrow_info {
  int32_t regrown;                       /* 0: the shape survived, the call did what mt_raytree_update_materials does */
  int32_t n_layers_before, n_layers_after;
  int64_t kept[MT_MAX_RECURSION + 1];    /* per layer of the NEW tree: rays taken over from the old tree */
  int64_t traced[MT_MAX_RECURSION + 1];  /* ... rays newly spawned and traced; kept + traced = new n_rays */
  int64_t dropped[MT_MAX_RECURSION + 1]; /* per layer of the OLD tree: rays with no place in the new one */
} mt_raytree_regrow_info;
int mt_raytree_regrow_materials(mt_raytree *tree, mt_raytree_regrow_info *info, mt_stats *stats);

/* Edited TEXTURES: texture `index` of the uploaded scene replaced in place -- size and format may change, the count may
 * not -- for a look-dev session that swaps a floor's planks for tiles without flattening and uploading the triangles
 * again.  (No reference counterpart.)  A texture touches exactly one quantity anywhere in this library, albedo =
 * ambient * Texture::GetColorAt(u, v) (mythtracer.cc:58-64): no ray, hit, child condition or shadow loop reads one.
 * mt_scene_set_texture is synchronous, like mt_scene_set_materials: it allocates room for the new texels, waits until
 * the scene's device is idle, uploads them, patches the scene's one table entry and only then frees the old texels.  An
 * allocation that does not fit is MT_ERR_NOMEM and the scene stays exactly as it was.  The kernels read size, format
 * and texels through that table at run time; nothing derived from a texture is baked into the uploaded scene or cached
 * on the host, so there is nothing else to refresh.
 * Generations: the scene keeps one per texture, 0 at creation, bumped by EVERY successful set -- the scene keeps no host
 * copy of the texels, so no comparison is made and setting the same bytes again counts as an edit.  Each successful set
 * also bumps the scene's material generation: every ray tree of the scene becomes stale exactly as after a material
 * edit (mt_raytree_update_materials).
 * mt_scene_get_texture_info fills width, height and format of the texture as it now is; texels is set to NULL.
 * CONTRACT: after the set, every call that renders or shades -- mt_scene_set_materials's list -- gives, byte for byte
 * and plane for plane, what it gives on a scene newly created from the same description with that texture.  Cost
 * history, forecasts and engine choice are left alone; G-buffer planes are the caller's (mt_retexture_gbuffer below).
 * Argument checks come before any device call, in this order: the scene (NULL); index outside 0 .. n_textures - 1; a
 * NULL mt_texture; set only: mt_scene_create's size and format check with its message ("texture %d: bad
 * size/format").  All MT_ERR_ARG. */
int mt_scene_set_texture(mt_scene *scene, int index, const mt_texture *tex);
int mt_scene_get_texture_info(const mt_scene *scene, int index, mt_texture *out);

/* Ray trees that keep uvw.  mt_scene_set_raytree_uvw(scene, 1): every tree made from now on -- mt_raytree_create,
 * _create_rays, _create_rays_device, and the one inside mt_trace_rays -- stores one more plane per layer on the scene's
 * GPU, uvw[n][3] doubles: Triangle::GetUVW(point), bit for bit mt_render_gbuffer's uvw for that ray, NaN for a miss.
 * The tracing kernel computes it exactly as it does for a textured albedo, so no bit of any other plane moves.  0 is
 * the default: bytes, planes and launches of a tree are then what they always were.  (MT_ERR_ARG: scene NULL, keep
 * other than 0 or 1.)  A tree remembers how it was made (mt_raytree_keeps_uvw: 0 / 1, MT_ERR_ARG < 0 for NULL), and
 * mt_raytree_info's bytes counts the plane: exactly 24 bytes per ray of the tree more than without it.  mt_raytree_layer stays as it is; mt_raytree_read_uvw copies one layer's plane to out_uvw[n_rays][3].  Its
 * checks, in this order, all MT_ERR_ARG, before any device call: tree NULL; layer outside the tree's; out_uvw NULL; a
 * tree that keeps no uvw.
 * What uvw buys: mt_raytree_update_materials and mt_raytree_regrow_materials also compare the per-texture generations
 * with the tree's snapshot of them (taken at creation and after each successful update or regrow).  A material is
 * RETEXTURED when (a) its ambient or tex changed and it has a texture before or after the edit -- those calls' refusal
 * (3) --, or (b) its current tex >= 0 and that texture was set since the snapshot.  A texture no material uses is
 * nothing to do.
 *   A tree WITHOUT uvw: (a) is refused as ever, with the same message; (b) is MT_ERR_UNSUPPORTED too, checked right
 *     after (a) and before any device call, the message naming the texture and the first material that uses it; the
 *     tree is untouched and still stale.  (Without this refusal a texture-only edit would compare equal materials and
 *     declare a wrong tree fresh.)
 *   A tree WITH uvw: the rays of a retextured material get albedo = ambient, times GetColorAt(texture, uvw.x, uvw.y)
 *     where tex >= 0 -- the tracing kernel's expressions in its order, from the stored plane -- in the commit
 *     (mt::raytree_recommit_kernel; in a regrow mt::raytree_regrow_copy_kernel for kept rays, reading the old layer's
 *     uvw, which kept rays carry over and traced rays get from their trace).  No light plane is traced again for a
 *     retexture alone: stats->rays_shadow stays 0.
 * Everything else in the two calls is as documented above.  CONTRACT, unchanged in form: after MT_OK the tree is
 * bit-identical, in every plane of every layer, uvw included, to mt_raytree_create[_rays] on a scene with the new
 * materials and textures and the same switch; after a refusal it is bit-identical to what it was. */
int mt_scene_set_raytree_uvw(mt_scene *scene, int keep);
int mt_raytree_read_uvw(mt_raytree *tree, int layer, double *out_uvw);
int mt_raytree_keeps_uvw(const mt_raytree *tree);

/* The deferred path's counterpart: the albedo plane of a stored G-buffer again under the scene's CURRENT materials and
 * textures.  Stateless, like mt_update_lightbuffer: reads gb->material and gb->uvw (chunk_w x chunk_h pixels, row-major)
 * and writes gb->albedo for EVERY pixel: NaN where material is outside 0 .. n_materials - 1 (what mt_render_gbuffer
 * stores for a miss or "no material"), else ambient, times GetColorAt(texture, uvw.x, uvw.y) where tex >= 0.  uvw may
 * be NULL only while no current material has a texture.  No sensor, no traversal (mt::gbuffer_retexture_kernel, one
 * thread per pixel): stats (nullable) has zero work counters, kernel_ms by events, total_ms = wall time.  No other
 * plane is read or written.  Infinite u or v is left undefined, as in the tracing kernels.
 * Checks, before any device call, in this order, all MT_ERR_ARG: gb NULL; material or albedo missing; uvw missing while
 * a current material has a texture; chunk_w, chunk_h outside 1 .. 100000; the scene (NULL).  _device: the planes are
 * device pointers on the scene's GPU, the launch is asynchronous on `stream`.
 * CONTRACT: the albedo plane is bit-identical to mt_render_gbuffer's under the new materials and textures, so
 * mt_shade_direct over it is mt_render_chunk(..., max_depth = 0) byte for byte. */
int mt_retexture_gbuffer(mt_scene *scene, int chunk_w, int chunk_h, const mt_gbuffer *gb, mt_stats *stats);
int mt_retexture_gbuffer_device(mt_scene *scene, int chunk_w, int chunk_h, const mt_gbuffer *d_gb, void *stream);

/* Triangles given another MATERIAL in place: the whole tri_material array replaced, in node-stream order, exactly as
 * mt_scene_desc::tri_material has it -- the same count, every entry one of the scene's materials or -1.  (No reference
 * counterpart.)  For a look-dev session that paints the box with the mirror's material or makes the pane opaque by
 * giving it the wall's: mt_scene_set_materials cannot express that, since a material's constants belong to every
 * object that shares it.  Every kernel reads a triangle's material index at run time and nothing derived from the
 * assignment is baked into the uploaded scene, so the call is one copy into the existing array, no kernel.
 * mt_scene_set_triangle_materials is synchronous, like mt_scene_set_materials: it waits until the scene's device is
 * idle, then copies.  The scene keeps a host copy of the assignment and an ASSIGNMENT generation, 0 at creation; a set
 * that changes at least one entry bumps it and bumps the material generation too, so every ray tree of the scene
 * becomes stale exactly as after a material edit (mt_raytree_update_materials).  A set that changes nothing changes no
 * state and makes no device call.  mt_scene_get_triangle_materials returns the host copy.  Zero triangles and
 * n_tris = 0 is MT_OK and does nothing, in both.  After mt_scene_set_triangle_vertices the node-stream order is the new
 * tree's: both calls speak that order from then on (mt_scene_read_tree gives its tri_id).
 * CONTRACT: after the set, every call that renders or shades -- mt_scene_set_materials's list, both frame engines, the
 * hybrid, the lean kernel and its redo launch, supersampled and adaptive frames, tile lists and mt_render_frame_multi
 * replicas that share a device -- gives, byte for byte and plane for plane, what the same call gives on a scene newly
 * created from the same description with that tri_material.  Cost history, forecasts and engine choice are left alone.
 * G-buffer and light-buffer planes are the caller's and describe the old assignment; there is no G-buffer counterpart
 * of this edit: render the G-buffer again, one primary pass.  There is no _device form.
 * Argument checks come before any device call, in this order: the scene (NULL); n_tris unequal to the scene's; a NULL
 * array with n_tris > 0; set only: an entry outside -1 .. n_materials - 1 (mt_scene_create's message, "triangle %d:
 * material index %d outside -1..%d").  All MT_ERR_ARG. */
int mt_scene_set_triangle_materials(mt_scene *scene, const int32_t *tri_material, int n_tris);
int mt_scene_get_triangle_materials(const mt_scene *scene, int32_t *out, int n_tris);

/* Ray trees that keep the triangle.  mt_scene_set_raytree_tri(scene, 1): every tree made from now on --
 * mt_raytree_create, _create_rays, _create_rays_device, and the one inside mt_trace_rays -- stores one more plane per
 * layer on the scene's GPU, tri[n] int32: the node-stream index of the triangle the ray hit (the index of
 * mt_scene_desc::tri_material and of mt_intersect_rays's `tri`), -1 for a miss.  The tracing kernel has it in hand, so
 * no bit of any other plane moves.  0 is the default: bytes, planes and launches of a tree are then what they always
 * were.  (MT_ERR_ARG: scene NULL, keep other than 0 or 1.)  The switch is independent of mt_scene_set_raytree_uvw.  A
 * tree remembers how it was made (mt_raytree_keeps_tri: 0 / 1, MT_ERR_ARG < 0 for NULL), and mt_raytree_info's bytes
 * counts the plane: exactly 4 bytes per ray of the tree more than without it.  mt_raytree_layer stays as it is;
 * mt_raytree_read_tri copies one layer's plane to out_tri[n_rays].  Its checks, in this order, all MT_ERR_ARG, before any
 * device call: tree NULL; layer outside the tree's; out_tri NULL; a tree that keeps no tri.
 * What tri buys: mt_raytree_update_materials and mt_raytree_regrow_materials take a REASSIGNMENT.  A tree's snapshot
 * holds the scene's assignment generation and the assignment itself, taken at creation and after each successful update
 * or regrow.  When the generations differ, CHANGED = the stream indices where the snapshot and the scene's current
 * assignment differ.  An empty CHANGED (A -> B -> A) is nothing to do for the assignment; if no constant or texture
 * changed either, the call is MT_OK without a device call and the tree is fresh.  Otherwise, before any device call and
 * after the two texture refusals, MT_ERR_UNSUPPORTED with the tree untouched and still stale:
 *   a tree WITHOUT tri: the message gives the count of changed triangles and the first.  (Without this refusal a
 *     reassignment would compare equal material tables and declare a wrong tree fresh.)
 *   a tree with tri but WITHOUT uvw, and a changed triangle whose NEW material has tex >= 0: the message names the
 *     triangle and the material.
 * mt_raytree_regrow_materials's light count check (4) also fires for a non-empty CHANGED.
 * While a reassignment is pending, every kernel of the two calls that reads a stored or kept ray's material reads the
 * EFFECTIVE material m'(i) = tri[i] < 0 ? -1 : tri_material_now[tri[i]] instead: for the child conditions, the
 * coefficient product and the albedo (mt::raytree_recoef_kernel, _recommit_kernel, _regrow_flags_kernel,
 * _regrow_copy_kernel, and _regrow_link_kernel).  The check pass always runs.  Commit and copy write m'(i) into the
 * material plane and restate the albedo where m'(i) differs from the stored material or m'(i)'s ambient, tex or
 * texture changed: ambient, times the texel at the stored uvw where textured; NaN for m' = -1, what the tracing kernel
 * stores.  The check pass still writes nothing but scratch.
 * Light planes: ALL are traced again in all layers (mt_raytree_update_lights's kernel over 0 .. n_lights - 1) when
 * mt_raytree_update_materials's rule says so OR some changed triangle qualifies.  With a = its old material under the
 * tree's snapshot of the constants and b = its new one under the scene's current table, it qualifies when a or b is -1
 * (a ray on it enters or leaves the light loop), when the transparencies differ by their bits, or when either
 * transparency is not 0 and the transmission filters differ.  The rule is conservative on purpose.
 * CONTRACT, unchanged in form: after MT_OK the tree is bit-identical in every plane of every layer, tri and uvw
 * included where kept, and in n_layers, n_rays and bytes, to mt_raytree_create[_rays] on a scene newly created with the
 * current assignment, materials, textures and lights and the same switches; after a refusal it is bit-identical to
 * what it was.  regrown, kept, traced, dropped and the stats keep their documented meaning. */
int mt_scene_set_raytree_tri(mt_scene *scene, int keep);
int mt_raytree_read_tri(mt_raytree *tree, int layer, int32_t *out_tri);
int mt_raytree_keeps_tri(const mt_raytree *tree);

/* Per-vertex ATTRIBUTES replaced in place: shading normals and texture coordinates.  (No reference counterpart.)  For a
 * look-dev session that smooths or flattens an object's shading, or tiles, offsets or rotates a texture on a surface.
 * The arrays are n_tris x 9 doubles in node-stream order, exactly as mt_scene_desc::tri_normal / tri_uvw have them.
 * Every kernel reads them at run time and nothing mt_scene_create derives from the description reads them (node
 * records, lists and boxes come from vertices alone), so the edit is one copy.  Vertex POSITIONS change the octree and
 * every derived record: mt_scene_set_triangle_vertices.  After such a set the node-stream order is the NEW tree's, and
 * these four calls speak that order (mt_scene_read_tree gives its tri_id).
 * The set is synchronous, like mt_scene_set_triangle_materials: it waits until the scene's device is idle.  The scene
 * keeps NO host copy of the attributes (144 bytes per triangle): the new array goes to a staging buffer on the GPU and
 * mt::tri_attr_stamp_kernel, one thread per triangle, compares each triangle's 9 doubles BY THEIR BITS with the live
 * array, copies the triangles that differ, writes the new generation into a per-triangle uint32 STAMP plane (one plane
 * per attribute, mirrored on the host, 4 bytes per triangle each), counts the changed triangles and keeps the lowest
 * changed index.  A staging buffer or stamp plane that does not fit is MT_ERR_NOMEM with the scene exactly as it was.
 * The scene keeps a NORMAL generation and a UVW generation, both 0 at creation; a set with at least one changed triangle
 * bumps its own and the material generation too, so every ray tree of the scene becomes stale exactly as after a
 * material edit.  A set that changes nothing bumps nothing and copies nothing into the live array.  (The generations are
 * 32 bits wide, like the stamps: after 2^32 - 1 sets that changed a triangle the next is MT_ERR_UNSUPPORTED.)  The getters read
 * the live array back from the device.  Zero triangles and n_tris = 0 is MT_OK and does nothing.  No _device form.
 * CONTRACT: after the set, every call that renders or shades -- mt_scene_set_materials's list, both frame engines, the
 * hybrid, the lean kernel and its redo launch, supersampled and adaptive frames, tile lists, mt_render_gbuffer, the
 * light-buffer calls, mt_raytree_create[_rays], mt_trace_rays and mt_render_frame_multi replicas that share a device --
 * gives, byte for byte and plane for plane, what the same call gives on a scene newly created from the same description
 * with that array.  Cost history, forecasts and engine choice are left alone.  G-buffer planes are the caller's and
 * describe the old attributes; they hold no stream index, so there is no G-buffer counterpart: render it again.
 * Argument checks come before any device call, in this order, all MT_ERR_ARG: the scene (NULL); n_tris unequal to the
 * scene's; a NULL array with n_tris > 0.  Values are not checked: NaN, zero and unnormalised normals are legal input, as
 * they are in a description. */
int mt_scene_set_triangle_normals(mt_scene *scene, const double *tri_normal, int n_tris);
int mt_scene_set_triangle_uvw(mt_scene *scene, const double *tri_uvw, int n_tris);
int mt_scene_get_triangle_normals(mt_scene *scene, double *out, int n_tris);
int mt_scene_get_triangle_uvw(mt_scene *scene, double *out, int n_tris);

/* Ray trees that keep tri take the attribute edit in mt_raytree_update_materials / mt_raytree_regrow_materials.  A
 * tree's snapshot also holds the two attribute generations, taken at creation and after each successful update or
 * regrow.  Ray i is UVW-DIRTY when tri[i] >= 0 and uvw_stamp[tri[i]] is greater than the snapshot's uvw generation;
 * NORMAL-DIRTY likewise with the normal stamps.  (A -> B -> A counts as dirty: the recomputation gives the old bits
 * back, so the contract below still holds.)
 * Refusal, after the texture and reassignment refusals and before any device call, MT_ERR_UNSUPPORTED with the tree
 * untouched and still stale: a tree WITHOUT tri while any triangle carries a stamp newer than the snapshot, in either
 * attribute; the message gives the attribute, the count and the first triangle.  (Without it an attribute-only edit
 * would compare equal tables and declare a wrong tree fresh.)
 * A uvw-dirty ray: uvw' = interpolate(tri_uvw[tri], barycentric(tri_vertex[tri], point)), the tracing kernel's
 * expressions from the stored point, goes to the uvw plane where the tree keeps one (the stored uvw is not required);
 * albedo = ambient, times the texel at uvw' where the ray's effective material has tex >= 0.  The retexture and
 * reassignment paths read uvw' for such a ray.  No light plane is traced for a uvw edit alone; the tree's shape never
 * changes.
 * A normal-dirty ray: normal' = interpolate(tri_normal[tri], ...) goes to the normal plane, unflipped.  Its reflected
 * child, if any, is no longer KEPT: it is spawned again from normal' and TRACED, with everything below it.  The
 * refracted child and its subtree stay kept; the ray's own light planes stay (their loop starts from point).
 * mt_raytree_update_materials: the check pass also counts normal-dirty rays with a reflected child; a non-zero count is
 * MT_ERR_UNSUPPORTED with the count and the first (layer, ray), as for a shape mismatch.  Otherwise
 * mt::raytree_reattr_kernel, one thread per ray, rewrites the dirty rays' planes in the commit.
 * mt_raytree_regrow_materials: a child is kept when its path exists in the old tree AND (it is the refracted child OR
 * its parent is not normal-dirty); a respawned reflected child's ray comes from the parent's EFFECTIVE normal.  The
 * copy kernel rewrites normal, uvw and albedo of kept dirty rays; layer 0 is rewritten in place at the commit.  The
 * light count check (4) also fires when any triangle is normal-stamped since the snapshot.
 * CONTRACT, unchanged in form: after MT_OK the tree is bit-identical in every plane of every layer, tri and uvw included
 * where kept, and in n_layers, n_rays and bytes, to mt_raytree_create[_rays] on a scene newly created with the current
 * attributes, assignment, materials, textures and lights and the same switches; after a refusal it is bit-identical to
 * what it was.
 * mt_raytree_attr_info_last: counts of the tree's last update or regrow (zero before the first): the rays whose normal /
 * uvw-dependent planes were rewritten, and the reflected children traced because of a dirty parent normal.
 * MT_ERR_ARG: tree or out NULL. */
typedef struct mt_raytree_attr_info {
  int64_t renormaled, reuvwed, respawned;
} mt_raytree_attr_info;
int mt_raytree_attr_info_last(const mt_raytree *tree, mt_raytree_attr_info *out);

/* A ray tree over the CALLER's rays, and the shade's colours before V3DtoRGB: TraceRay(ray) (mythtracer.h:77) for a ray
 * list at full depth -- a panorama or fisheye camera, an orthographic view, a probe, any ray a caller wants the colour
 * of.  Everything after layer 0 of a ray tree already runs over a ray list and never looks at a sensor or an image, so
 * a tree whose layer 0 comes from the caller is traced by the same kernels, launch for launch, and carries the relight
 * family with it.
 *
 * Layer 0 of a ray-list tree: the list counts as a list_w x list_h chunk at (0, 0) of an image of that size.  Caller's
 * ray p (row-major: x = p % list_w, y = p / list_w) goes to the place the order of layer 0 above gives chunk pixel
 * (x, y), with in_object[p] and coef[p] (0 and 1.0 where the arrays are NULL), and pixel = p.  A list_w x 1 list keeps
 * the caller's order: the place of p is p.  An image-shaped ray set therefore gets an 8x8 block per wave, like a
 * sensor tree; a bare list gets waves of 64 consecutive rays of the caller's.  The directions need NOT be normalised
 * (a reflected child ray is not either); exact zeros in one or two components are valid.
 * From there the tree is an ordinary mt_raytree: the same planes and layer rules; mt_raytree_info, _read_layer,
 * _shade[_device], _update_lights[_device] and _destroy work unchanged; mt_raytree_shade's bitmap is [n][3] bytes in the
 * caller's order.  mt_raytree_desc reports image_w = chunk_w = list_w, image_h = chunk_h = list_h,
 * chunk_x = chunk_y = 0 and from_rays = 1.
 * CONTRACT: the sensor's rays of a chunk, handed in as a chunk_w x chunk_h list, give mt_raytree_create's tree in every
 * plane of every layer; layer k of a tree, handed in as an n x 1 list with its in_object and coef and
 * max_depth - k, gives that tree's layers k onwards.
 *   mt_raytree_create_rays: the arrays of `rays` are HOST memory.  Synchronous.  stats (nullable): rays_primary = n,
 *     everything else as mt_raytree_create fills it (the copy of the list and its import are inside kernel_ms).
 *   mt_raytree_create_rays_device: the arrays of `d_rays` are on the scene's GPU (the struct itself is host memory).
 *     They are read on the scene's DEFAULT stream: the caller must have finished producing them (synchronise the
 *     producing stream first).  Synchronous, like the host form.
 * A ray is REFUSED when one of its six numbers is not finite, its direction is (0, 0, 0), its in_object byte is above
 * 1, or its coef is not finite: the walk has never been handed such a ray and is not by these calls.  The host form
 * scans the list on the host before any device call.  The device form cannot: the import kernel
 * (mt::raytree_rays_kernel) counts the refused rays and keeps the lowest index, and the host reads both BEFORE the
 * first tracing launch.  In both forms any refused ray is MT_ERR_ARG with the count and the first index in the
 * message; no tree is returned, no tracing kernel has run and no work counter has moved.
 * Argument checks come before any device call, in this order: `rays` or rays->ray NULL; list_w < 1, list_h < 1
 * (MT_ERR_ARG), list_w * list_h of 2^31 or more (MT_ERR_ARG, the layer limit's message; there is no limit of 100000
 * per side); the scene; max_depth in 0 .. MT_MAX_RECURSION; host form only: the content of the list.
 *
 * mt_raytree_shade_colors[_device]: mt_raytree_shade[_device] with layer 0's colours written as they are, before
 * V3DtoRGB clamps and quantises them: [n][3] doubles at the rays' `pixel` places -- chunk-local row-major for a sensor
 * tree, the caller's order for a ray-list tree (mt::raytree_color_kernel: out[pixel[i]] = colour[i]).  For a caller
 * who filters, tone-maps or composites.  Both kinds of tree; lights, stats, asynchrony and the one-shade-in-flight rule
 * as for mt_raytree_shade[_device]; the checks in its order (the output, tree, lights).
 * CONTRACT: V3DtoRGB of the colours equals mt_raytree_shade's bytes, byte for byte, for the same tree and lights.
 *
 * mt_trace_rays: mt_raytree_create_rays, the shade under the scene's CURRENT lights (mt_scene_set_lights), destroy.
 * out_color ([n][3] doubles) and out_rgb ([n][3] bytes) in the caller's order; either may be NULL, both NULL is
 * MT_ERR_ARG and checked first, then mt_raytree_create_rays's checks.  Synchronous.  stats (nullable): the create's
 * counters, kernel_ms = the create's plus the shade's, total_ms = wall time of the call. */
typedef struct mt_ray_list {
  const double *ray;        /* [n][6] origin, direction as handed to OctTree::IntersectRay;
                               the direction need NOT be normalised (child rays are not either) */
  const uint8_t *in_object; /* [n] 0 / 1, nullable = all 0 */
  const double *coef;       /* [n] current_reflection_coef, nullable = all 1.0 */
  int32_t list_w, list_h;   /* n = list_w * list_h, caller's order row-major;
                               a plain list is n x 1 */
} mt_ray_list;
mt_raytree *mt_raytree_create_rays(mt_scene *scene, const mt_ray_list *rays, int max_depth, mt_stats *stats);
mt_raytree *mt_raytree_create_rays_device(mt_scene *scene, const mt_ray_list *d_rays, int max_depth, mt_stats *stats);
int mt_raytree_shade_colors(mt_raytree *tree, const mt_light *lights, int n_lights, double *out_color, mt_stats *stats);
int mt_raytree_shade_colors_device(mt_raytree *tree, const mt_light *lights, int n_lights, void *d_color, void *stream);
int mt_trace_rays(mt_scene *scene, const mt_ray_list *rays, int max_depth, double *out_color, uint8_t *out_rgb,
                  mt_stats *stats);

/* One frame on SEVERAL GPUs of this process -- the master/worker farm of the
 * reference (main_net_master.cc:195-236: GenerateWork cuts the frame into
 * WorkChunks, every worker renders chunks with the full-image sensor from its
 * own copy of the scene, main_net_worker.cc:29-32,148-150, BlitWorkChunk puts
 * them into the frame) inside one host process: scenes[r] is a replica of the
 * scene on its own HIP device (mt_scene_desc.device; several replicas may share
 * a device), the tiles of the tile_w x tile_h grid are dealt out by cost as
 * described above (first frame of a geometry: by tile number; a camera at rest
 * keeps its assignment from the second frame on), all
 * replicas render at the same time, the tile buffers travel to scenes[0]'s
 * device (peer copies over xGMI, 3 bytes per pixel in total), are blitted there
 * and the frame is copied to out_rgb (image_w*image_h*3 bytes, row-major, top
 * row first -- what RayTrace(int,int,Camera*,vector*) returns).  Lights must
 * have been set on every replica.  stats (nullable): n_scenes entries, the work
 * counters, kernel_ms = that replica's frame kernels, total_ms = wall time of
 * the whole call; stats[0].total_ms - max kernel_ms ~ exchange + blit + D2H.
 * The result is byte-identical to mt_render_chunk of the whole frame.
 * STATE OF TESTING: on one-GPU boxes only.  Replicas that share a device are
 * covered by the GPU tests, including the gather-buffer offsets and the blit of
 * the cross-device branch (forced through hipMemcpyPeerAsync on one device by
 * MT_TUNE_MULTI_FORCE_PEER_COPY); peer access BETWEEN devices
 * (hipDeviceCanAccessPeer / EnablePeerAccess, cross-device events) has not run
 * on hardware yet, and no multi-GPU scaling figure has been measured. */
int mt_render_frame_multi(mt_scene *const *scenes, int n_scenes,
                          const mt_sensor *sensor, int image_w, int image_h,
                          int tile_w, int tile_h, int max_depth,
                          uint8_t *out_rgb, mt_stats *stats);

/* Multi-GPU frames with a MOVING camera (the reference's loop turns it every
 * frame, main_local.cc:51-76).  A launch orders its work by the block costs of
 * the previous frame, re-projected through the camera change -- but a rank
 * measured only its own tiles, and the old-image position of a block mostly
 * lies in another rank's tile.  So the ranks exchange their costs, 4 bytes per
 * 8x8 block of the frame (the path's second, tiny exchange step; the reference's
 * master hands chunks out dynamically instead, main_net_master.cc:62-80):
 * export writes the costs of this scene's LAST launch, on a common scale, into a
 * frame-wide map d_map[map_h][map_w] of uint32 (map_w >= ceil(image_w / 8),
 * map_h >= ceil(image_h / 8); only the blocks of that launch's tiles are
 * written: zero the map first); the ranks combine their maps with an
 * element-wise MAX (torch.distributed.all_reduce / RCCL); import hands the
 * result to the scene, whose NEXT launch reads it wherever a re-projected
 * forecast needs a cost (later launches fall back to the scene's own costs
 * unless a new map is imported).  Any uint32 value is acceptable input: 0 =
 * nobody reported that block, and whatever else a word holds (export never
 * sets bit 31) only orders the work.  Nothing computed for a pixel depends on
 * it.
 * mt_render_frame_multi does the same between its replicas by itself. */
int mt_scene_export_costs_device(mt_scene *scene, void *d_map, int map_w,
                                 int map_h, void *stream);
int mt_scene_import_costs_device(mt_scene *scene, const void *d_map, int map_w,
                                 int map_h, void *stream);

/* Fetches and clears the accumulated counters (kernel_ms/total_ms = 0). */
int mt_scene_read_stats(mt_scene *scene, mt_stats *stats);

/* Work counters of the *_device calls: 1 (default) = the kernels count rays,
 * node visits, box tests, requested bytes ... as they go (about 7 % of a
 * frame's time: one LDS atomic per counter and node visit); 0 = kernels built
 * without the counters (mt_scene_read_stats then returns zeros).  The image is
 * the same either way.  mt_render_chunk with a stats pointer always counts. */
int mt_scene_set_stats(mt_scene *scene, int enabled);

/* Work scheduling.  use_cost_history = 1 (default): a launch with the same
 * geometry as the previous one (image, region, tiling, recursion depth, light
 * count) hands out its 8x8-pixel blocks in the order of the costs measured in
 * that previous launch, longest first, the few longest as four quarters with
 * four lanes per pixel; everything then runs in ONE kernel.  0: every launch
 * classifies its blocks by material first (two kernels).  Either way each
 * pixel is computed by the same arithmetic: the output does not depend on it.
 * The call also forgets the recorded costs.  (No reference counterpart: the
 * reference hands rows to a thread pool, mythtracer.cc:244-290.) */
int mt_scene_set_scheduling(mt_scene *scene, int use_cost_history);

/* Frame engine.  Two implementations of TraceRayWorker's control flow exist;
 * every pixel goes through the same operations in the same order in both, so
 * the output does not depend on the choice.  1 = throughput engine: one lane
 * per pixel runs the recursion as a state machine (lowest cost per ray).  2 =
 * latency engine: the recursion of every pixel is unrolled into a per-wave pool
 * of rays, so that a call's shadow loops and child calls are traced side by
 * side (shortest chain of dependent passes per pixel; wins when a launch has
 * few blocks per wave, e.g. one rank's share of a multi-GPU frame).  3 =
 * hybrid: ONE kernel in which every wave first works through the launch's
 * longest blocks, cut into pieces, as a ray-pool wave and then through
 * everything else as a state-machine wave (needs measured block costs and has no
 * debug-buffer path: a launch without the one or with the other is rendered by
 * engine 2).  0 = automatic (default): 2 for launches without measured block
 * costs; with them, 3 for launches with fewer than 9 blocks per resident wave,
 * else 1.  Also forgets the recorded costs.  Limits of engine 2: at most 254 lights (a pool entry holds the
 * light in 8 bits), and its scratch -- per resident wave `capacity` records of
 * 160 + 80 n_lights bytes, capacity <= 1024 -- must fit a budget (4 GiB; the
 * capacity shrinks to fit, down to the ~280 records its depth-first throttle
 * needs).  The automatic mode never fails on either limit: launches the pool
 * cannot hold comfortably are rendered by engine 1, which has no such limits;
 * only an EXPLICIT engine 2 beyond them returns MT_ERR_UNSUPPORTED.
 * (No reference counterpart.) */
int mt_scene_set_engine(mt_scene *scene, int engine);
/* Process-wide default of mt_scene_set_engine for scenes created afterwards
 * (also those the C++ facade creates); 0 initially. */
int mt_set_default_engine(int engine);

/* Tuning constants of the work order and of the engine choice (defaults = what
 * the sweeps in DESIGN.md settled on).  None of them changes a pixel; tests and
 * experiment scripts use them instead of environment variables.  The call also
 * forgets the recorded costs. */
enum {
  MT_TUNE_POOL_BELOW = 0,     /* automatic engine: ray pool below this many blocks per resident wave (9) */
  MT_TUNE_POOL_CAP,           /* records per wave of the ray pool, 0 = default (tests: force the throttle) */
  MT_TUNE_PACKED_STACK,       /* 1 (default): 16-byte traversal stack frames when indices fit; 0: 20-byte */
  MT_TUNE_BLOCKS_PER_CU,      /* 0 = as many workgroups per CU as fit */
  MT_TUNE_FORECAST_RADIUS,    /* blocks; < 0 = 1, or 2 when the camera origin moved */
  MT_TUNE_BLEND,              /* damping of a repeated frame's cost forecast (0.9) */
  MT_TUNE_FORMS,              /* 1 (default): per-block ratio of the two measured cost forms */
  MT_TUNE_POOL_CUT_SHARE,     /* < 0 = 1.0 with history, 0.3 without */
  MT_TUNE_POOL_PIECE_TIME1, MT_TUNE_POOL_PIECE_TIME2,
  MT_TUNE_POOL_PIECE_WORK1, MT_TUNE_POOL_PIECE_WORK2,
  MT_TUNE_POOL_CELL_FACTOR,
  MT_TUNE_QUAD_SHARE, MT_TUNE_QUAD_SHARE_MOVING, MT_TUNE_QUAD_KEEP,
  MT_TUNE_QUAD_WORK, MT_TUNE_QUAD_WORK_MOVING,
  MT_TUNE_POOL_SCRATCH_MB,    /* scratch budget of the ray pool (4096) */
  MT_TUNE_HYBRID_POOL_SHARE,  /* engine 3: blocks above this share of an even split go to the ray pool in pieces (1.3) */
  MT_TUNE_HYBRID_QUAD_SHARE,  /* ... above this one to the state machine as quarters, four lanes per pixel (1.0 = none) */
  MT_TUNE_HYBRID_WORK1, MT_TUNE_HYBRID_WORK2, /* pool quarters / cells: summed cost over the whole block's (1.3, 3.3) */
  MT_TUNE_FORECAST_STEP,      /* pixels between the positions a re-projected forecast takes its maximum over (8) */
  MT_TUNE_HYBRID_STARTER_SHARE, /* engine 3: state-machine units above this share of an even split start with the launch,
                                   on waves that skip the pool's part (0.33; a value above every unit = none) */
  MT_TUNE_DEEP_LAYOUT,        /* 1 (default): octrees of 12 .. 16 levels keep only the first ten levels' traversal frames in LDS
                                 (the rest in global memory: 8 waves per CU instead of 7 .. 5); 0: everything in LDS */
  MT_TUNE_MULTI_FORCE_PEER_COPY, /* tests: mt_render_frame_multi copies every replica's tiles into the gather buffer with
                                    hipMemcpyPeerAsync even when it shares the first replica's device (0) */
  MT_TUNE_MULTI_BALANCE,      /* mt_render_frame_multi: 1 (default) = tiles dealt out by cost, 0 = by tile number */
  MT_TUNE_XCD_QUEUES,         /* state-machine launches ordered by cost history: 0 = one work order for the chip; 1 = eight
                                 orders, one per XCD, each over a stripe of the picture with an eighth of the forecast cost
                                 (an XCD's L2 then holds its stripe's part of the tree; an XCD that runs dry takes units
                                 from the fullest other queue); 2 = a 4 x 2 grid of regions instead of stripes */
  MT_TUNE_ORDER_GROUPS,       /* workgroups of the three kernels that make a launch's work order (forecast per block,
                                 counting sort, units longest first): 64; 1 .. 256 */
  MT_TUNE_SM_CELL_SHARE,      /* state machine: a block goes out as sixteen 2x2 cells (four lanes per pixel) when a QUARTER
                                 of it is expected above this multiple of the quarters' cutting threshold */
  MT_TUNE_SM_CELL_TIME, MT_TUNE_SM_CELL_WORK, /* a cell's expected time / the cells' summed cost, over the block as one unit */
  MT_TUNE_HYBRID_CELL_FACTOR, /* engine 3: the pool's pieces of a block are 2x2 cells when a quarter is expected above this
                                 multiple of the pool's threshold (0.85; the ray pool by itself: MT_TUNE_POOL_CELL_FACTOR) */
  MT_TUNE_LEAN_KERNEL,        /* state-machine launches with a cost history, traversal mode 0, a scene the hit-set walk takes:
                                 the LEAN frame kernel (the walk alone; a unit that meets a ray the walk cannot take is
                                 abandoned and rendered by the full kernel in a launch behind it).  0 = never; 1 (default)
                                 = unless a primary ray of the frame has a zero direction component; 2 = even then (tests) */
  MT_TUNE_COUNT
};
/* One more knob, outside the dense range above: those are constants of a launch's scheduling, this one is a property of
 * the traversal.  Frame kernels (the state machine of engines 1 and 3, lean and full; the ray pool's own shadow records
 * are never bounded): an iteration of the shadow loop does not walk into subtrees that its ray enters beyond the light
 * (mt_shadow_bound.h; a scene that is not eligible traces as before).  The picture is the same; the WORK COUNTERS are
 * not -- the far wall's triangle is no longer tested.  0 = never; 1 (default) = launches with the counters off
 * (mt_scene_set_stats(scene, 0)), so that the counters always describe the unbounded traversal, whose work is never
 * below the reference's; 2 = counting launches too (tests, measurements). */
#define MT_TUNE_SHADOW_BOUND 1000
int mt_scene_set_tuning(mt_scene *scene, int knob, double value);

/* Device durations of the launches made since the previous call (at most the
 * last 64, oldest first; at most max_n): primary_ms[i] = the kernels that
 * prepare the work order (mt::order_forecast_kernel, mt::order_count_kernel
 * and mt::order_scatter_kernel with cost history, else mt::primary_kernel;
 * for the latency engine's first frame mt::probe_kernel + those three),
 * render_ms[i] = the frame kernel
 * (mt::render_kernel or mt::pool_kernel) of launch i, from HIP events recorded on
 * the launch's own stream.  Waits for those launches.  Returns the number of
 * entries written, or a negative MT_ERR_*.  (No reference counterpart: the
 * reference times a frame with wall clocks, main_local.cc:86-101.) */
int mt_scene_kernel_times(mt_scene *scene, int max_n, double *primary_ms,
                          double *render_ms);

/* What the scene's last launch was (MT_TUNE_LEAN_KERNEL).  lean = 1: its frame kernel was the lean one, and then:
 * units = work units of its order; redo_units = those the full kernel rendered in the redo launch (abandoned by the
 * lean kernel, or all of them: handed_over = 1, the lean kernel opened none because earlier lean launches of the scene
 * abandoned too many); lean_ms / redo_ms = device durations of the two launches (render_ms of mt_scene_kernel_times
 * is their sum).  Waits for the device.  (No reference counterpart.) */
typedef struct mt_lean_info {
  int32_t lean, handed_over;
  uint32_t units, redo_units;
  double lean_ms, redo_ms;
} mt_lean_info;
int mt_scene_lean_info(mt_scene *scene, mt_lean_info *out);

/* OctTree::IntersectRay (octtree.cc:26-40) for a batch: rays = n x 6 doubles
 * (origin, direction).  Outputs (each nullable): tri = stream-order triangle
 * index or -1, line_no, t, point (3 per ray; untouched = NaN on miss). */
int mt_intersect_rays(mt_scene *scene, int n, const double *rays,
                      int32_t *tri, int32_t *line_no, double *t,
                      double *point, mt_stats *stats);

/* Test hook: 0 = automatic (default: regular rays take the hit-set walk --
 * every node once per wave, children in any order, the reference's choice among
 * them by its (entry distance, index) rule; DESIGN.md section 3.1 -- and the
 * ordered descent of the modes below serves the rest), 1 = always use the exact
 * std::min/std::max comparison path, 2 = allow min/max instructions but not
 * the octant-uniform path, 3 = automatic but never the triangle-parallel
 * (transposed) node scan, 4 = automatic but without the fp32 conservative
 * pre-filter, 5 = automatic but every node through a wave step (no
 * lane-parallel scan of small nodes), 6 = automatic but without the block
 * boxes that skip runs of triangles, 7 = automatic but without the subtree
 * boxes that skip children.  Results are identical in every mode; the
 * counters box_tests / node_visits / tri_tests / mt_tests equal the
 * reference's traversal in modes 1, 2, 4 and 7 (no subtree is skipped there);
 * in the others the first three count only the nodes actually visited, and in
 * mode 0 all four are the walk's own work (it may look at a node that lies
 * behind the reference's early exit: mt_tests is then not smaller than the
 * reference's, never the other way round). */
int mt_scene_set_traversal_mode(mt_scene *scene, int mode);

/* The octree built ON THE GPU from triangles in ADD order (AddPrimitive order): node for node and bit for bit the tree
 * OctTree::Finalize builds on the host (the reference's AttemptSplit, octtree.cc:52-135).  (No reference counterpart:
 * the reference builds on one host thread.)  tri_vertex is a HOST array of n_tris x 9 doubles.  The result is opaque
 * and lives on `device`; NULL with mt_last_error set on failure, and nothing is left allocated then.
 * The rules, each the host builder's with the same fp64 operations in the same order:
 *   triangle box (Triangle::CacheAABB): {v0, v0} extended by v1, then v2, with std::min(box, p) / std::max(box, p): a
 *     NaN in v0 stays, a NaN in v1 or v2 is ignored;
 *   root box (OctTree::AddPrimitive): {0,0,0}-{0,0,0} extended by every triangle box: a NaN bound never enters, a bound
 *     that comes out as zero is +0.0;
 *   a node splits iff at least 16 triangles reached it, at c = lo + (hi - lo) / 2.0 per axis, into the eight octants
 *     of mt_scene_desc's child order; a triangle goes to the FIRST child whose box contains its box (closed intervals:
 *     any NaN means not contained), else it stays; the children of one level's nodes are numbered in the order of their
 *     parents, so a level is a contiguous range of node indices; centre is zero for a node that does not split;
 *   the stream: nodes in index order, a node's triangles in ascending add index.
 * How: mt_build.h -- a level-by-level descent with integer counters (one host round trip per level reads how many
 * nodes split), then one stable sort of (node, add index).  Nothing depends on the order in which atomics arrive: two
 * builds of the same input give the same bytes.
 * Limits: a node that would have to split at depth MT_MAX_TREE_DEPTH (root = 1) ends the build with
 * MT_ERR_UNSUPPORTED and mt_scene_create's message ("octree depth %d exceeds MT_MAX_TREE_DEPTH %d"), the verdict
 * mt_scene_create gives for such a tree built on the host; more nodes than an int32 indexes are MT_ERR_UNSUPPORTED; an
 * allocation that does not fit is MT_ERR_NOMEM.  n_tris = 0 is a tree of one node, the box {0,0,0}-{0,0,0}.
 * Argument checks come before any device call, in this order, all MT_ERR_ARG: n_tris negative; tri_vertex NULL with
 * n_tris > 0; then the device ordinal (mt_device_count: "device %d outside 0..%d").  Values are not checked.
 * info (nullable): n_nodes; depth (root = 1); levels = the host round trips made (= depth); kernel_ms by HIP events from
 * the first to the last kernel, the per-level round trips included; total_ms = wall time of the call. */
typedef struct mt_octree mt_octree;
typedef struct mt_build_info {
  int32_t n_nodes, depth, levels;
  double kernel_ms, total_ms;
} mt_build_info;
/* The arrays of a tree, the FlatTree of the facade.  n_nodes, n_tris and depth are always written by a read; every
 * pointer is the caller's buffer of the size given, or NULL for an array that is not wanted. */
typedef struct mt_octree_arrays {
  int32_t n_nodes, n_tris, depth;
  double *node_aabb;     /* n_nodes x 6 */
  double *node_center;   /* n_nodes x 3 */
  int32_t *first_child;  /* n_nodes */
  int32_t *prim_begin;   /* n_nodes */
  int32_t *prim_count;   /* n_nodes */
  int32_t *tri_id;       /* n_tris: stream position -> add index */
  double *tri_aabb;      /* n_tris x 6, in ADD order */
} mt_octree_arrays;
mt_octree *mt_octree_build(int device, int n_tris, const double *tri_vertex, mt_build_info *info);
/* MT_ERR_ARG: tree or out NULL. */
int mt_octree_info(const mt_octree *tree, mt_build_info *out);
int mt_octree_read(const mt_octree *tree, mt_octree_arrays *out);
void mt_octree_destroy(mt_octree *tree);

/* A scene from triangles in ADD order: the tree is built on the GPU (mt_octree_build on d->device), the triangle arrays
 * are gathered into node-stream order with its tri_id, and the description goes through mt_scene_create's own
 * path: validation, derived records and every message are mt_scene_create's.
 * CONTRACT: the scene is indistinguishable from mt_scene_create on the host-built description of the same triangles --
 * every frame, plane, statistic and getter, and tri_id (the G-buffer's `prim` plane).
 * Checks before any device call, in this order, all MT_ERR_ARG: d NULL; struct_size / abi_version; a negative count;
 * a triangle array missing with n_tris > 0 (tri_vertex, tri_normal, tri_uvw, tri_material, tri_line_no); the material
 * or texture array missing with a count > 0; then mt_octree_build's device check.  What mt_scene_create checks in the
 * description (material and texture indices, texture sizes) it checks here too, after the build.
 * info (nullable): the build's, as mt_octree_build reports it. */
typedef struct mt_triangle_desc {
  uint32_t struct_size; /* sizeof(mt_triangle_desc) */
  uint32_t abi_version; /* MT_ABI_VERSION */
  int32_t device;
  int32_t n_tris, n_materials, n_textures;
  const double *tri_vertex;     /* n_tris x 9, ADD order like the four below */
  const double *tri_normal;
  const double *tri_uvw;
  const int32_t *tri_material;
  const int32_t *tri_line_no;
  const mt_material *materials;
  const mt_texture *textures;
} mt_triangle_desc;
mt_scene *mt_scene_create_triangles(const mt_triangle_desc *d, mt_build_info *info);

/* The same arrays from ANY scene: its node records and triangle boxes read back from the device, its tri_id mirror
 * (after mt_scene_set_triangle_vertices: the new tree and the new order's tri_id).
 * Checks, in this order, all MT_ERR_ARG: scene NULL; out NULL; a scene made without tri_id. */
int mt_scene_read_tree(const mt_scene *scene, mt_octree_arrays *out);

/* Triangles MOVED in place: the vertex positions of the listed triangles replaced on the uploaded scene.  (No reference
 * counterpart.)  For a session that moves an object between frames without giving up the scene: materials, textures (no
 * texel is uploaded again), lights, tuning, engine, traversal mode, the stats switch, the material / texture /
 * assignment / attribute generations, cost history and forecasts all stay.
 * add_idx holds ADD-order indices (mt_scene_desc::tri_id values), each at most once, in any order; vertices holds
 * n_idx x 9 doubles, triangle add_idx[i] at vertices + 9 i.  mt_scene_get_triangle_vertices returns ALL vertices in add
 * order.  Both calls are synchronous, like mt_scene_set_triangle_normals: they wait until the scene's device is idle.
 * There is no _device form.  The scene keeps no host copy of vertices, normals or uvw, before or after.
 * CONTRACT: after a successful set, every call that renders, shades or reads the scene -- both frame engines, the
 * hybrid, the lean kernel and its redo launch, supersampled and adaptive frames, tiles and tile lists, the G-buffer and
 * light-buffer calls, mt_raytree_create[_rays], mt_trace_rays, mt_intersect_rays, mt_render_frame_multi replicas,
 * mt_scene_read_tree and every getter -- gives, byte for byte and plane for plane, what the same call gives on a scene
 * newly made by mt_scene_create_triangles from the same triangles in add order with the new vertices, the live normals,
 * uvw, assignment, line numbers, materials, textures and lights, and the same switches; the counters of mt_stats match
 * too (not the times) wherever the two frames are SCHEDULED alike -- a first frame, a frame with
 * mt_scene_set_scheduling(scene, 0), the G-buffer, light-buffer, ray-tree and ray-list calls: the wave-level counters
 * of a frame depend on its work order, and a moved scene orders its next frame by the costs of the frames before the
 * move (forecasts, not results: the frame's bytes do not depend on them), which a new scene does not have.
 * STREAM ORDER: the tree is built anew, so the scene's node-stream order is the NEW tree's from then on.
 * mt_scene_set_triangle_materials, mt_scene_set_triangle_normals, mt_scene_set_triangle_uvw and their getters speak the
 * new order, and mt_scene_read_tree gives the new order's tri_id: read it after every set that may have changed a
 * triangle.
 * How, all on the scene's GPU (mt_build.h): mt::move_unscatter_kernel brings the live vertices into add order through
 * the old tri_id and writes the inverse permutation; mt::move_overwrite_kernel writes the listed triangles over them,
 * comparing each triangle's 9 doubles BY THEIR BITS and counting the changed triangles; the tree is built from that
 * device array (mt_octree_build's path); mt::move_regather_kernel writes vertices, normals, uvw, material indices,
 * line numbers, boxes and the attribute stamp planes in the new order into new allocations.  The host reads back the
 * tree, the stream-order boxes and vertices, runs mt_scene_create's own checks and derivation (mt_layout.h) and uploads
 * the derived arrays into new allocations.  Only then the scene's pointers and counts are swapped, the launch
 * configuration is made again (deep layout, LDS bytes, packed stack), the host mirrors are permuted (mt_move.h) and the
 * old allocations freed.
 * NO-OP: a set whose listed vertices equal the live ones by their bits changes no state and bumps nothing.  n_idx = 0
 * is MT_OK and does nothing.
 * FAILURE before the swap leaves the scene EXACTLY as it was -- the next frame, mt_scene_read_tree and the getters are
 * what they were: MT_ERR_NOMEM; MT_ERR_UNSUPPORTED with the build's message for a tree deeper than MT_MAX_TREE_DEPTH or
 * of more nodes than an int32 indexes; MT_ERR_HIP.
 * RAY TREES: the scene has a GEOMETRY generation, 0 at creation, bumped by every set that changed a triangle.  A tree
 * snapshots it at creation.  A tree's tri plane and hit points belong to the geometry it was traced in, so a tree of an
 * older geometry generation is refused for good with MT_ERR_ARG by mt_raytree_shade[_colors][_device],
 * mt_raytree_update_lights[_device], mt_raytree_update_materials and mt_raytree_regrow_materials; the message says to
 * destroy the tree.  The check stands directly before the stale-materials check and leaves the tree untouched.
 * mt_raytree_destroy, mt_raytree_info and the mt_raytree_read_* calls keep working.  G-buffer and light-buffer planes
 * are the caller's and describe the old geometry; the `prim` plane holds add indices, which a move does not change.
 * Argument checks come before any device call, in this order, all MT_ERR_ARG: scene NULL; a scene made without tri_id;
 * n_idx negative or greater than n_tris; add_idx or vertices NULL with n_idx > 0; an index outside 0 .. n_tris - 1; an
 * index listed twice.  (Then, for a scene from mt_scene_create: a tri_id that is no permutation of 0 .. n_tris - 1.)
 * Values are not checked: NaN and +-inf are legal, as for the build.  The getter: scene NULL; no tri_id; n_tris unequal
 * to the scene's; out NULL with n_tris > 0.
 * info (nullable): the build's, as mt_octree_build reports it, with total_ms = the wall time of the whole set; all zero
 * after a no-op.  mt_scene_move_times_last, a diagnostic in the manner of mt_scene_kernel_times: the wall times in ms of
 * the parts of the scene's last set that changed a triangle -- or of its last mt_scene_edit_triangles (below) that was
 * not the no-op, whichever came later --, out_ms[MT_MOVE_TIMES], all zero before the first such call
 * (MT_ERR_ARG: scene or out_ms NULL).  mt_build_info cannot carry them without a change of the ABI's structs. */
enum {
  MT_MOVE_MS_BUILD = 0,  /* the tree */
  MT_MOVE_MS_REGATHER,   /* the per-triangle arrays in the new order */
  MT_MOVE_MS_READBACK,   /* tree, boxes and vertices to the host */
  MT_MOVE_MS_LAYOUT,     /* mirrors, checks, derived arrays (host) */
  MT_MOVE_MS_UPLOAD,     /* the derived arrays to the device */
  MT_MOVE_TIMES
};
int mt_scene_set_triangle_vertices(mt_scene *scene, const int32_t *add_idx, int n_idx,
                                   const double *vertices /* n_idx x 9 */, mt_build_info *info /* nullable */);
int mt_scene_get_triangle_vertices(mt_scene *scene, double *out /* n_tris x 9 */, int n_tris);
int mt_scene_move_times_last(const mt_scene *scene, double *out_ms /* MT_MOVE_TIMES */);

/* Triangles ADDED and REMOVED in place: the triangle set of the uploaded scene changed, n_tris with it.  (No reference
 * counterpart.)  For a session in which an object appears or leaves without giving up the scene: everything a move keeps
 * is kept -- materials, textures (no texel moves), lights, tuning, engine, traversal mode, the stats switch, the
 * material / texture / assignment / attribute generations, and the forecast banks with their cost history (they are per
 * image block and do not know n_tris).
 * remove_idx holds ADD-order indices of the scene as it is, each at most once, in any order.  The add_* arrays are HOST
 * arrays in mt_triangle_desc's layout: 9 / 9 / 9 doubles and 1 / 1 int32 per added triangle.  add_material indexes the
 * scene's existing material table, or is -1: the call adds no material and no texture.
 * NEW ADD ORDER: the surviving triangles come first, in their old relative order, numbered densely -- new index = old
 * index - the number of removed indices below it --; the n_add new triangles follow in the order given.  (numpy.delete
 * followed by concatenate: the caller can compute it, so no call reports it.)
 * CONTRACT: mt_scene_set_triangle_vertices's, word for word.  After a successful edit every call that renders, shades or
 * reads the scene -- all frame engines, the hybrid, the lean kernel and its redo launch, supersampled and adaptive
 * frames, tiles and tile lists, the G-buffer and light-buffer calls, mt_raytree_create[_rays], mt_trace_rays,
 * mt_intersect_rays, mt_render_frame_multi replicas, mt_scene_read_tree and every getter -- gives, byte for byte and
 * plane for plane, what it gives on a scene newly made by mt_scene_create_triangles from the resulting add-order arrays:
 * the survivors with their live vertices, normals, uvw, assignment and line numbers, the added triangles with theirs,
 * and the live materials, textures, lights and switches.  The counters of mt_stats match wherever the two frames are
 * scheduled alike (see above).
 * COUNT AND ORDER: n_tris is the new count and the node-stream order the new tree's from then on.
 * mt_scene_set_triangle_materials / _normals / _uvw, their getters, mt_scene_get_triangle_vertices and
 * mt_scene_set_triangle_vertices speak the new count and the new order; a call with the old count gets their
 * "%d triangles for a scene made with %d".
 * STAMPS: an added triangle's attribute stamp is 0, as for a triangle no set has touched; a stamp plane that does not
 * exist yet stays non-existent.
 * How (mt_build.h): mt::edit_mark_kernel writes keep[a] = 0 for every listed index over a plane of ones; an exclusive
 * integer prefix sum of it (rocPRIM) is every survivor's new add index, its total the survivor count, which is held to
 * n_tris - n_remove (MT_ERR_INTERNAL if they differ); mt::edit_stage_kernel brings the survivors' live vertices and the
 * added vertices into the new add order and notes every triangle's source; the tree is built from that array with the new
 * count; mt::edit_regather_kernel writes all per-triangle arrays and the stamp planes in the new stream order into new
 * allocations, the attributes from the old arrays or from the uploaded add arrays.  From there on the steps are a
 * move's, with another count: read-back, mt_scene_create's checks and derivation, upload, swap -- which also sets
 * n_tris and what is computed from it --, the mirrors in the new count (mt_edit.h), the old allocations freed.
 * NO-OP: n_remove = 0 and n_add = 0 is MT_OK, changes no state and makes no device call.  Every other accepted edit
 * changes the scene: removing a triangle and adding an identical one renumbers the add order.
 * FAILURE before the swap leaves the scene EXACTLY as it was, as for a move: MT_ERR_NOMEM; MT_ERR_UNSUPPORTED with the
 * build's message for a tree deeper than MT_MAX_TREE_DEPTH or of more nodes than an int32 indexes; MT_ERR_HIP.
 * RAY TREES: every edit that is not the no-op bumps the geometry generation, so a tree of the old geometry is refused for
 * good by the calls that refuse it after a move (above); no other check exists or is needed.  The `prim` plane of an
 * older G-buffer holds add indices of the OLD numbering.
 * Argument checks come before any device call, in this order, all MT_ERR_ARG: scene NULL; a scene made without tri_id;
 * a scene of zero triangles; n_remove negative or greater than n_tris; n_add negative; remove_idx NULL with
 * n_remove > 0; a missing add array with n_add > 0, named in the order vertex, normal, uvw, material, line_no; a remove
 * index outside 0 .. n_tris - 1; a remove index listed twice; a resulting count (computed in 64 bits) below 1 or above
 * what an int32 holds; an add_material outside -1 .. n_materials - 1 (mt_scene_create's message).  (Then, for a scene
 * from mt_scene_create, once: a tri_id that is no permutation.)  An edit never empties a scene and never starts from an
 * empty one, which keeps zero-sized launches and allocations out of the path.  Vertex values are not checked: NaN and
 * +-inf are legal, as for the build.
 * info (nullable): the build's, with total_ms = the wall time of the whole edit; all zero after the no-op.
 * mt_scene_move_times_last reports the parts of the scene's last move OR edit, through the same five entries
 * (MT_MOVE_MS_BUILD does not include the staging, as for a move). */
int mt_scene_edit_triangles(mt_scene *scene, const int32_t *remove_idx, int n_remove, int n_add, const double *add_vertex,
                            const double *add_normal, const double *add_uvw, const int32_t *add_material,
                            const int32_t *add_line_no, mt_build_info *info /* nullable */);

#ifdef __cplusplus
}
#endif
#endif /* MYTHTRACER_HIP_H_ */
