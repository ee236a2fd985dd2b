// mythtracer.h — the renderer class: the drop-in seam (reference:
// VerStarting/mythtracer.h:11-79).  Same names, fields and call contract as the
// reference so that main_local.cc / main_net_worker.cc build unchanged; the
// pixel loop behind RayTrace runs on an MI355X through libmythtracer_hip.so.
#pragma once
#include <stdint.h>
#include <cstddef>
#include <string>
#include <vector>
#include "camera.h"
#include "objreader.h"
#include "octtree.h"

struct mt_scene;
struct mt_stats;
struct mt_raytree;

namespace raytracer {
using math3d::V3D;

const int MAX_RECURSION_LEVEL = 5;

struct PerPixelDebugInfo {
  int line_no;
  V3D point;
};

class WorkChunk {
 public:
  // input
  int image_width, image_height;
  int chunk_x, chunk_y;
  int chunk_width, chunk_height;
  Camera camera;  // not part of the serialized input

  static const size_t kSerializedInputSize = 6 * sizeof(uint32_t);
  void SerializeInput(std::vector<uint8_t>* bytes);
  bool DeserializeInput(const std::vector<uint8_t>& bytes);

  // output: chunk-local row-major RGB8; optional per-pixel first-hit info
  std::vector<uint8_t> output_bitmap;
  std::vector<PerPixelDebugInfo> output_debug;

  static const size_t kSerializedOutputMinimumSize = sizeof(uint32_t);
  bool SerializeOutput(std::vector<uint8_t>* bytes);
  bool DeserializeOutput(const std::vector<uint8_t>& bytes);
};

// Work counters of the last RayTrace call (extension; see mt_stats).
struct RenderStats {
  uint64_t rays_primary = 0, rays_secondary = 0, rays_shadow = 0;
  uint64_t box_tests = 0, node_visits = 0, tri_tests = 0, mt_tests = 0, shaded_hits = 0;
  double kernel_ms = 0, total_ms = 0;
};

// The primary-hit G-buffer of a frame or chunk (extension; mt_render_gbuffer in mythtracer_hip.h): per pixel the first
// hit's distance, point, Triangle::GetNormal (as returned: not flipped towards the camera), Triangle::GetUVW, unlit
// surface colour (material ambient x texture), AddPrimitive index, .obj line and material.  `channels` says which planes
// RayTraceGBuffer fills (the others are left empty and cost nothing); every plane is chunk-local row-major, the V3D
// planes three doubles per pixel.  A miss: NaN / -1.  material = the triangle's material in order of first use by the
// octree's triangle stream (FlatScene::materials), -1 = none (albedo is then NaN).
struct GBuffer {
  enum : unsigned {
    kDepth = 1u, kPoint = 2u, kNormal = 4u, kUvw = 8u, kAlbedo = 16u, kPrim = 32u, kLineNo = 64u, kMaterial = 128u,
    kAll = 255u
  };
  unsigned channels = kAll;
  int width = 0, height = 0;  // of the chunk the planes describe
  std::vector<double> depth, point, normal, uvw, albedo;
  std::vector<int32_t> prim, line_no, material;
};

// The direct-light buffer of a frame or chunk (extension; mt_render_lightbuffer in mythtracer_hip.h): per light (in the
// order of Scene::lights) and pixel, what the shadow loop of TraceRayWorker leaves behind -- light_power before it is
// raised to the light's ambient, three doubles, and in_shadow, one byte: 0 lit, 1 in shadow, 255 = no light loop ran for
// the pixel (a miss or a hit without a material; power is NaN there).  The plane of light l starts l * width * height
// pixels into the vector.  With the point, normal, albedo and material planes of a GBuffer it holds everything
// ShadeDirect needs.  It depends on the lights' positions, not on their colours.
struct LightBuffer {
  enum : unsigned { kPower = 1u, kInShadow = 2u, kAll = 3u };
  unsigned channels = kAll;
  int width = 0, height = 0, n_lights = 0;
  std::vector<double> power;
  std::vector<uint8_t> in_shadow;
};

// The ray-tree buffer of a frame or chunk (extension; mt_raytree_create in mythtracer_hip.h): the whole call tree of
// TraceRayWorker for every pixel, traced once by BuildRayTree and kept on the GPU, from which ShadeRayTree makes the
// full-depth frame under edited light colours without tracing a ray.  Move-only; destroys its mt_raytree.  It belongs
// to the MythTracer that built it and must be destroyed (or Reset) before that MythTracer, and before anything that
// uploads the scene again (LoadObj, SetDevices, UpdateGeometry).
class RayTree {
 public:
  RayTree() = default;
  ~RayTree() { Reset(); }
  RayTree(const RayTree&) = delete;
  RayTree& operator=(const RayTree&) = delete;
  RayTree(RayTree&& o) noexcept : tree_(o.tree_) { o.tree_ = nullptr; }
  RayTree& operator=(RayTree&& o) noexcept {
    if (this != &o) {
      Reset();
      tree_ = o.tree_;
      o.tree_ = nullptr;
    }
    return *this;
  }
  void Reset();
  bool Empty() const { return tree_ == nullptr; }
  mt_raytree* Get() const { return tree_; }
  // layers, rays of layer k (0 beyond the last layer), lights, bytes of HBM held; zeros for an empty handle
  int Layers() const;
  long long Rays(int layer) const;
  int Lights() const;
  unsigned long long Bytes() const;

 private:
  friend class MythTracer;
  mt_raytree* tree_ = nullptr;
};

class MythTracer {
 public:
  MythTracer();
  ~MythTracer();
  MythTracer(const MythTracer&) = delete;
  MythTracer& operator=(const MythTracer&) = delete;

  Scene* GetScene();
  bool LoadObj(const char* fname);
  bool RayTrace(int image_width, int image_height, Camera* camera,
                std::vector<uint8_t>* output_bitmap);
  bool RayTrace(WorkChunk* chunk);

  // --- extensions (not in the reference)
  void SetDevice(int hip_device) {
    device_ = hip_device;
    scene.tree.SetDevice(hip_device);
  }
  // Several GPUs of this process for the W x H overload of RayTrace: a scene replica per listed HIP device
  // (a device may be listed more than once), tiles k = r (mod N) of the frame rendered side by side, gathered
  // and blitted on the first device -- mt_render_frame_multi; the master/worker farm of main_net_master.cc:195-236
  // in one process.  RayTrace(WorkChunk*) -- the unit a worker renders -- stays on the first device.
  void SetDevices(const std::vector<int>& hip_devices);
  void SetMaxRecursionLevel(int level) { max_level_ = level; }  // default MAX_RECURSION_LEVEL
  // Supersampling: s x s samples per pixel (default 1 = the reference's one ray per pixel), resolved on the GPU:
  // both RayTrace overloads return the reference's frame at s W x s H, box-filtered s x s (mt_render_chunk_ss).
  // A factor outside 1 .. 4 makes the next RayTrace fail; so do s > 1 with a non-empty WorkChunk::output_debug (a
  // debug record belongs to a ray, not to a mean) and, for the W x H overload, s > 1 with more than one device
  // (SetDevices): a supersampled frame is rendered on one device, never silently so when several were asked for.
  void SetSupersampling(int s) { supersampling_ = s; }
  // Adaptive supersampling (mt_render_chunk_adaptive): one ray per pixel, then s x s samples in the 8 x 8 blocks of
  // the image where neighbouring pixels differ by more than `threshold` (0 .. 255) in a channel.  s <= 1 switches it
  // off.  Independent of SetSupersampling; with both set, adaptive wins.  Refused like SetSupersampling's frames:
  // with output_debug, and by the W x H overload after SetDevices with several devices.  A chunk's result depends on
  // the chunk's borders (pairs of pixels across them are not looked at).
  void SetAdaptiveSupersampling(int s, int threshold) {
    adaptive_ss_ = s > 1 ? s : 1;
    adaptive_threshold_ = threshold;
  }
  // The primary-hit G-buffer of a W x H frame, or of chunk->chunk_* (its camera and image size; output_bitmap and
  // output_debug are not touched).  No reference counterpart: the reference returns a colour and PerPixelDebugInfo.
  // One kernel launch next to the frame's (mt_render_gbuffer); the frames' cost history is left alone.
  // SetSupersampling does NOT apply: a G-buffer value belongs to one ray, the pixel's, never to a mean -- the call
  // ignores the factor.  With more than one device (SetDevices) the call is refused with a message: there is no
  // multi-GPU G-buffer, and it is never silently rendered on the first device.  LastStats() describes the call.
  bool RayTraceGBuffer(int image_width, int image_height, Camera* camera, GBuffer* out);
  bool RayTraceGBuffer(WorkChunk* chunk, GBuffer* out);
  // The direct-light buffer under GetScene()->lights, and in the same launch, from the same primary rays, the planes
  // `gbuffer->channels` selects (gbuffer may be NULL: none).  Everything said about RayTraceGBuffer applies.
  bool RayTraceLightBuffer(int image_width, int image_height, Camera* camera, GBuffer* gbuffer, LightBuffer* out);
  bool RayTraceLightBuffer(WorkChunk* chunk, GBuffer* gbuffer, LightBuffer* out);
  // The frame of the direct term -- what RayTrace gives with SetMaxRecursionLevel(0) -- from stored planes and
  // GetScene()->lights, without tracing a ray (mt_shade_direct): for lights whose ambient, diffuse or specular were
  // edited since the light buffer was made.  Their count and positions must be the light buffer's: a moved light needs
  // UpdateLightBuffer first.  `gbuffer` must hold point, normal, albedo and material, `lightbuffer` both planes, all
  // of this frame (or chunk->chunk_*) and camera.  output_bitmap is resized to width x height x 3.
  bool ShadeDirect(int image_width, int image_height, Camera* camera, const GBuffer& gbuffer,
                   const LightBuffer& lightbuffer, std::vector<uint8_t>* output_bitmap);
  bool ShadeDirect(WorkChunk* chunk, const GBuffer& gbuffer, const LightBuffer& lightbuffer);
  // After lights have MOVED: the planes of the lights listed in `lights` (indices into GetScene()->lights, each at most
  // once) of `lightbuffer` traced again under GetScene()->lights from the point and material planes of `gbuffer`, without
  // a primary ray (mt_update_lightbuffer); the planes of the other lights are not touched.  Both structs must describe
  // the same chunk, `lightbuffer` as many lights as the scene has now; the planes `lightbuffer->channels` selects are
  // updated.  The result is what a new RayTraceLightBuffer gives if only the listed lights moved since the planes were
  // made.  Refused with several devices, like its siblings; LastStats() describes the call.
  bool UpdateLightBuffer(const GBuffer& gbuffer, const std::vector<int>& lights, LightBuffer* lightbuffer);
  // The ray tree of a W x H frame, or of chunk->chunk_* (its camera and image size), to the recursion level of
  // SetMaxRecursionLevel under GetScene()->lights (mt_raytree_create); what `tree` held before is destroyed.
  // SetSupersampling does not apply.  Refused with a message after SetDevices with several devices, like
  // RayTraceGBuffer.  LastStats() describes the call: its ray counts are those of RayTrace for the same frame.
  bool BuildRayTree(int image_width, int image_height, Camera* camera, RayTree* tree);
  bool BuildRayTree(WorkChunk* chunk, RayTree* tree);
  // The frame RayTrace would give -- at the level the tree was built with -- under the CURRENT GetScene()->lights,
  // from the stored tree without tracing a ray (mt_raytree_shade): for lights whose ambient, diffuse or specular were
  // edited since BuildRayTree.  Their count must be the tree's (checked) and so must their positions (not checked).
  // The chunk form writes chunk->output_bitmap; the chunk must have the tree's size.
  bool ShadeRayTree(const RayTree& tree, std::vector<uint8_t>* output_bitmap);
  bool ShadeRayTree(const RayTree& tree, WorkChunk* chunk);
  // After lights have MOVED: the planes of the lights listed in `lights` (indices into GetScene()->lights, each at most
  // once) in every layer of `tree` traced again under GetScene()->lights from the tree's own stored hits, without a
  // primary or secondary ray (mt_raytree_update_lights); nothing else in the tree is touched.  The tree is then what a new
  // BuildRayTree gives if only the listed lights moved since it was built, and ShadeRayTree gives RayTrace's frame.
  // The facade itself refuses, with a message and before any device call: several devices (SetDevices), an empty
  // list, a NULL or empty RayTree, and another number of lights than the tree's.  An index out of range or listed twice
  // is refused by mt_raytree_update_lights, after the facade has uploaded GetScene()->lights; the tree is untouched in
  // every case.  LastStats() describes the call.
  bool UpdateRayTree(const std::vector<int>& lights, RayTree* tree);
  // After materials were EDITED in GetScene()->materials (a wall's colour, a mirror's reflectance): flattens them into
  // the dense table in its uploaded order (order of first use) and replaces the constants on every device replica
  // (mt_scene_set_materials), without uploading a triangle again; every later RayTrace, G-buffer, light buffer and
  // BuildRayTree sees them.  Refused with a message when the set of material NAMES differs from the uploaded one (the
  // call edits, it neither adds nor removes) or a material points at a texture that was not uploaded.  Before the
  // first upload it is Prepare.  RayTrees built before the edit are stale until UpdateRayTreeMaterials.
  bool UpdateMaterials();
  // After a texture was EDITED in place in GetScene()->textures[key] (its colors, width and height; the Texture object
  // itself stays, materials point at it): replaces the uploaded texture on every device replica by the entry as it now
  // is (mt_scene_set_texture), size and format free to change, without uploading a triangle again.  `key` is the
  // texture table's key.  Refused with a message when the table has no such key, when that texture was not uploaded (no
  // material of a triangle used it at the upload: the call edits, it neither adds nor removes) or when its size and
  // colours disagree.  Before the first upload it is Prepare.  RayTrees built before the edit are stale until
  // UpdateRayTreeMaterials, which needs a tree that keeps uvw for it (SetRayTreeKeepUVW).
  bool UpdateTexture(const std::string& key);
  // RayTrees built from now on also keep each ray's texture coordinates (mt_scene_set_raytree_uvw): 24 bytes more per
  // ray, and UpdateRayTreeMaterials / RegrowRayTree then take texture edits and ambient or texture changes of textured
  // materials, which they refuse for a tree without.  Off by default.
  void SetRayTreeKeepUVW(bool keep);
  // After triangles were given another MATERIAL (GetScene()->tree.MutableTriangle(i)->mtl pointing at another of
  // GetScene()->materials, or at none): derives the per-triangle material indices again, in the uploaded order and
  // through the uploaded dense table, and replaces them on every device replica (mt_scene_set_triangle_materials),
  // without uploading a triangle again; every later RayTrace, G-buffer, light buffer and BuildRayTree sees them.
  // Refused with a message when a triangle points at a material that was not uploaded (no triangle used it at the
  // upload: the call edits, it does not add).  Before the first upload it is Prepare.  RayTrees built before the edit
  // are stale until UpdateRayTreeMaterials / RegrowRayTree, which need a tree that keeps triangles for it.
  bool UpdateTriangleMaterials();
  // After triangles' per-vertex NORMALS or texture coordinates were edited (GetScene()->tree.MutableTriangle(i)->normal
  // / ->uvw): flattens them again in the uploaded order and replaces them on every device replica
  // (mt_scene_set_triangle_normals, mt_scene_set_triangle_uvw), without uploading a triangle again.  Vertex positions
  // are not covered: a moved vertex needs UpdateGeometryInPlace or a new upload.  Before the first upload it is Prepare.  RayTrees built before
  // the edit are stale until UpdateRayTreeMaterials / RegrowRayTree, which need a tree that keeps triangles for it.
  bool UpdateTriangleAttributes();
  // The octree of the next Prepare is built on the GPU (OctTree::SetDeviceBuild, mt_octree_build on the facade's first
  // device) instead of by OctTree::Finalize on the host: the same tree, bit for bit, so everything downstream -- the
  // upload, the edit calls' stream order, IntersectRays -- runs as it does with the host builder.  Off by default.  With
  // the switch on, no GPU or a failed build makes Prepare return false with the reason in LastError(): the host builder
  // is never used instead.
  void SetDeviceTreeBuild(bool on) { scene.tree.SetDeviceBuild(on); }
  // MOVING geometry: the three vertices of each of the triangles `add_indices` (LoadObj / AddPrimitive order) replaced
  // by vertices[3 k .. 3 k + 2], and the triangle's box cached again (Triangle::CacheAABB).  Only the host scene
  // changes; refused with a message, and no triangle changed, for an index outside the scene's triangles or another
  // number of vertices than three per index.  UpdateGeometry() must follow before the scene is used again.
  bool SetTriangleVertices(const std::vector<int>& add_indices, const std::vector<V3D>& vertices);
  // After SetTriangleVertices (or any edit of MutableTriangle(i)->vertex followed by its CacheAABB): the root box is
  // recomputed from {0,0,0}-{0,0,0} over all triangles -- it can shrink --, the tree is marked unfinalized and the device
  // scenes are dropped, so the next Prepare (every rendering call makes one) builds the tree again, with either
  // builder, and uploads.  RayTree objects follow SetDevices's rule: a RayTree built before the call belongs to a device
  // scene that no longer exists and must have been destroyed or Reset BEFORE the call (see RayTree); there is no way
  // to bring such a tree to the moved geometry, and none to ask it whether it is fresh: build a new one.
  void UpdateGeometry();
  // The same IN PLACE (mt_scene_set_triangle_vertices): the device scenes stay alive and keep their materials, textures
  // (nothing of them is uploaded again), lights, tuning, engine and cost history.  The root box is recomputed on the
  // host, the triangles moved by SetTriangleVertices since the last upload or update (all triangles when none were
  // moved through it) go to every device replica, which builds the tree again on its GPU and re-orders its arrays, and
  // the host tree adopts the new flat tree from the first replica.  UpdateTriangleMaterials, UpdateTriangleAttributes
  // and flatten() speak the new order afterwards; the scene stays finalized and uploaded.  With nothing uploaded yet it
  // is UpdateGeometry() followed by Prepare().  Refused with a message while a batch of AddTriangle / RemoveTriangles
  // is pending (UpdateTrianglesInPlace() first).  False with LastError() set when a device refuses (no memory, a tree
  // deeper than MT_MAX_TREE_DEPTH): that device's scene is as it was, and neither the host builder nor a new upload
  // is used instead.  With one device the facade is then exactly as before the call.  With several, the first device
  // moves first and the host tree adopts its tree at once, so the host's stream order is always the first device's; a
  // LATER replica that refuses stays on the old geometry, and the only legal calls then are a repeated
  // UpdateGeometryInPlace() (the moved triangles are remembered; the set is a no-op where it already happened) or
  // UpdateGeometry().  RayTree objects follow
  // UpdateGeometry's rule: destroy or Reset them BEFORE the call (a tree of the old geometry is refused by every call
  // that shades or updates it).
  bool UpdateGeometryInPlace();
  // ADDING and REMOVING triangles of an uploaded scene, in place (mt_scene_edit_triangles): an object that appears in
  // a session or leaves it.  AddTriangle takes ownership and appends the triangle (Triangle::CacheAABB is the
  // caller's, as for AddPrimitive): it gets the last add index.  RemoveTriangles deletes the listed triangles (LoadObj /
  // AddPrimitive indices, each at most once); the survivors keep their relative order and are numbered densely.  Only
  // the host scene changes: UpdateTrianglesInPlace() must follow before the scene is used again.  ONE pending batch at a
  // time: since the last upload or update RemoveTriangles may be called at most once and only before any AddTriangle,
  // so that its indices are the uploaded scene's; anything else is refused with a message that says to update first.
  // SetTriangleVertices is refused while a batch is pending, and so are UpdateGeometryInPlace, UpdateTriangleMaterials
  // and UpdateTriangleAttributes, whose numbering and stream order the batch has left behind; AddTriangle (the triangle
  // is deleted then) and RemoveTriangles are refused while triangles moved by SetTriangleVertices await
  // UpdateGeometryInPlace(), whose indices a batch would renumber.  So moves and a batch are never pending together.
  // While a batch is pending on an uploaded scene the flat tree describes the old triangles: flatten() and the tree's
  // dump refuse too.
  bool AddTriangle(Triangle* triangle);
  bool RemoveTriangles(const std::vector<int>& add_indices);
  // The pending batch to every device replica: the root box is recomputed on the host, the first replica removes and
  // adds the triangles in place -- it keeps its materials, textures (nothing of them is uploaded again), lights, tuning,
  // engine and cost history --, the host tree adopts that replica's new flat tree, and the other replicas follow.
  // UpdateTriangleMaterials, UpdateTriangleAttributes, SetTriangleVertices and flatten() speak the new count and order
  // afterwards.  With nothing uploaded yet it is UpdateGeometry() followed by Prepare(), whatever is pending, moved
  // vertices included; with nothing pending it does nothing.  Refused with a message, before any device call and with the batch still pending, when triangles moved by
  // SetTriangleVertices await UpdateGeometryInPlace(), or when an added triangle points at a material that was not
  // uploaded (the call adds no material: UpdateGeometry() uploads such a batch).  An edit is not idempotent and the host
  // scene cannot go back, so a device that refuses (no memory, a tree deeper than MT_MAX_TREE_DEPTH, an edit that
  // leaves no triangle) must not leave host and replicas in a mixed state: ALL device scenes are dropped and the
  // scene is marked unfinalized, as by UpdateGeometry(); false with LastError() set, and the next Prepare() uploads the
  // host's state anew.  RayTree objects follow UpdateGeometry's rule: destroy or Reset them BEFORE the call.
  bool UpdateTrianglesInPlace();
  // RayTrees built from now on also keep the triangle each ray hit (mt_scene_set_raytree_tri): 4 bytes more per ray,
  // and UpdateRayTreeMaterials / RegrowRayTree then take an UpdateTriangleMaterials, which they refuse for a tree
  // without.  Off by default; independent of SetRayTreeKeepUVW (a reassignment TO a textured material needs both).
  void SetRayTreeKeepTriangles(bool keep);
  // Brings `tree` to the materials of the last UpdateMaterials without tracing a primary or secondary ray
  // (mt_raytree_update_materials): new albedo and coefficients, and the light planes again where a shadow ray can see
  // the edit (under GetScene()->lights).  Fails, with the tree exactly as it was, when the edit changes which rays
  // spawn children, or -- for a tree built without SetRayTreeKeepUVW -- touches the ambient of a textured material or a
  // texture in use: a new BuildRayTree is needed then.  Refused with
  // several devices, like BuildRayTree, and for a NULL or empty RayTree.  LastStats() describes the call.
  bool UpdateRayTreeMaterials(RayTree* tree);
  // The same after an edit that changes which rays spawn children -- a matte surface made reflective, a mirror switched
  // off, a pane made opaque (mt_raytree_regrow_materials): the rays whose path survives are kept, the dead subtrees
  // dropped and only the new rays traced, under GetScene()->lights; Layers() and Rays() follow.  The tree is then what a
  // new BuildRayTree gives, and ShadeRayTree gives RayTrace's frame.  Where the shape survives the call is
  // UpdateRayTreeMaterials.  Still fails for the ambient of a textured material or an edited texture when the tree
  // was built without SetRayTreeKeepUVW.  Refused with several devices and for a
  // NULL or empty RayTree.  LastStats() describes the call (rays_secondary = the rays traced).
  bool RegrowRayTree(RayTree* tree);
  // The caller's rays instead of a camera's (mt_raytree_create_rays): TraceRay for a ray list, to the recursion level of
  // SetMaxRecursionLevel under GetScene()->lights.  list_width 0 means an n x 1 list, whose waves are 64 consecutive
  // rays of the caller's; otherwise it must divide n and the list is treated as a list_width x (n / list_width) image,
  // row-major, whose waves are 8x8 blocks.  The directions need not be normalised; a ray with a number that is not
  // finite or with the direction (0, 0, 0) is refused with a message naming the count and the first index.  The tree
  // is an ordinary RayTree: ShadeRayTree (bitmap and colours in the caller's order) and UpdateRayTree accept it.
  // Refused, before anything touches a device: a NULL tree, several devices (SetDevices), an empty list, a list_width
  // that is negative or does not divide n.  LastStats() describes the call (rays_primary = n).
  bool BuildRayTree(const std::vector<Ray>& rays, int list_width, RayTree* tree);
  // ShadeRayTree's colours before V3DtoRGB (mt_raytree_shade_colors), one V3D per layer-0 ray: chunk-local row-major
  // for a camera's tree, the caller's order for a ray list's.  V3DtoRGB of them is ShadeRayTree's bitmap byte for byte.
  bool ShadeRayTree(const RayTree& tree, std::vector<V3D>* colours);
  // BuildRayTree(rays, list_width), the shade under GetScene()->lights, and the tree is gone (mt_trace_rays): the
  // colours, the RGB8 bitmap (n x 3 bytes) or both, in the caller's order.  Either output may be NULL, not both.
  bool TraceRays(const std::vector<Ray>& rays, int list_width, std::vector<V3D>* colours, std::vector<uint8_t>* bitmap);
  void SetQuiet(bool quiet) {                                   // no progress text on stdout
    quiet_ = quiet;
    scene.tree.SetQuiet(quiet);
  }
  // Work counters of a render (LastStats).  On by default (the tests read them); a driver that only wants the frame
  // switches them off: the kernels built without the counting are about a tenth faster (mt_scene_set_stats).
  void SetCollectStats(bool on) { collect_stats_ = on; }
  const RenderStats& LastStats() const { return stats_; }
  const char* LastError() const { return error_.c_str(); }
  // Finalizes the tree if needed and uploads the scene; RayTrace does this
  // lazily on its first call exactly like the reference finalizes lazily.
  bool Prepare();
  mt_scene* DeviceScene() { return dev_; }

 private:
  Scene scene;
  bool was_scene_finalized = false;
  mt_scene* dev_ = nullptr;            // replica on devices_[0] (= device_)
  std::vector<mt_scene*> replicas_;    // replicas on devices_[1..]
  std::vector<int> devices_;           // empty = {device_}
  int device_ = 0;
  void DropDeviceScenes();
  std::vector<std::string> uploaded_names_, dense_names_;  // UpdateMaterials: all names at the upload; the dense table's
  std::vector<const Texture*> uploaded_textures_;          // ... and the texture table's sources
  std::vector<const Material*> uploaded_materials_;        // UpdateTriangleMaterials: the dense table's sources
  bool keep_uvw_ = false;                                  // SetRayTreeKeepUVW
  bool keep_tri_ = false;                                  // SetRayTreeKeepTriangles
  std::vector<int> moved_;                                 // SetTriangleVertices' indices since the last upload or update
  // the pending batch of AddTriangle / RemoveTriangles: the removed indices (of the uploaded scene), whether
  // RemoveTriangles was called, the number of triangles appended since (they are the host tree's last ones)
  std::vector<int32_t> removed_;
  bool removal_pending_ = false;
  size_t added_ = 0;
  bool EditPending() const { return removal_pending_ || added_ > 0; }
  void ForgetEdit();
  void HostOnlyEdit();
  int max_level_ = MAX_RECURSION_LEVEL;
  int supersampling_ = 1;
  int adaptive_ss_ = 1, adaptive_threshold_ = 16;
  bool CheckSupersampling(int image_width, int image_height, bool on_all_devices);
  bool quiet_ = false;
  bool collect_stats_ = true;
  RenderStats stats_;
  std::string error_;
};

}  // namespace raytracer
