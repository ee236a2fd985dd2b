// octtree.h — the loose octree of the facade (reference:
// VerStarting/octtree.h:14-69, octtree.cc).
//
// Same public interface; different inside.  Finalize() builds the tree straight
// into flat, breadth-first arrays (the layout libmythtracer_hip.so consumes,
// include/mythtracer_hip.h mt_scene_desc) instead of a pointer tree, and
// IntersectRay() runs on the GPU.  The split rule, child boxes, first-fit
// child order and in-node primitive order reproduce octtree.cc:52-135 exactly:
// traversal results depend on them.
#pragma once
#include <cstdint>
#include <functional>
#include <memory>
#include <vector>
#include "math3d.h"
#include "primitive.h"

struct mt_scene;
struct mt_octree_arrays;

namespace raytracer {
using math3d::V3D;

class Triangle;

// Flattened tree + triangle streams (host copy of what lives in HBM).
struct FlatTree {
  int depth = 0;  // root = 1
  std::vector<double> node_aabb;      // 6 per node
  std::vector<double> node_center;    // 3 per node
  std::vector<int32_t> first_child;   // 0 = leaf
  std::vector<int32_t> prim_begin, prim_count;
  std::vector<int32_t> tri_id;        // stream position -> AddPrimitive index
  size_t NodeCount() const { return first_child.size(); }
};

class OctTree {
 public:
  OctTree();
  ~OctTree();
  OctTree(const OctTree&) = delete;
  OctTree& operator=(const OctTree&) = delete;

  // Takes ownership.  Only Triangle primitives are supported; anything else
  // is rejected (deleted, message on stderr).  Not allowed after Finalize().
  void AddPrimitive(Primitive* p);

  // Builds the tree.  Prints "Triangles: N" like the reference.
  void Finalize();
  bool IsFinalized() const { return finalized_; }
  // extension: AppendPrimitive / RemovePrimitives changed the triangle set of a finalized tree, and Flat() still
  // describes the old one (its tri_id may name triangles that are gone): nothing may read it until Adopt() or Refit()
  bool FlatIsStale() const { return flat_is_stale_; }
  // extension: Finalize() builds the tree on the GPU (mt_octree_build on the device of SetDevice) instead of on the
  // host: the same FlatTree, bit for bit.  Off by default.  When it is on and the build fails -- no GPU, no memory, a
  // tree deeper than MT_MAX_TREE_DEPTH -- Finalize() leaves the tree unfinalized with the reason in LastError(): it
  // never falls back to the host builder.
  void SetDeviceBuild(bool on) { device_build_ = on; }
  bool DeviceBuild() const { return device_build_; }
  // extension, after triangles were MOVED (MutableTriangle(i)->vertex, then its CacheAABB): the root box again from
  // {0,0,0}-{0,0,0} over all triangles in add order -- it can shrink --, and the tree is unfinalized: the next
  // Finalize() builds it again.  The standalone IntersectRay's upload is dropped.
  void Refit();
  // extension, for a tree that was rebuilt elsewhere after triangles were moved (mt_scene_set_triangle_vertices on the
  // uploaded scene): RefitRoot recomputes the root box like Refit and drops the standalone IntersectRay's upload, but
  // leaves the tree as it is; Adopt takes `flat` as the finalized tree, as Finalize does under SetDeviceBuild.
  void RefitRoot();
  void Adopt(FlatTree flat);
  // extension, for a triangle SET that changes after Finalize() while the tree is rebuilt elsewhere
  // (mt_scene_edit_triangles on the uploaded scene).  AppendPrimitive is AddPrimitive -- it takes ownership, Triangle
  // only, the root box extended -- but allowed after Finalize(); the triangle gets the last add index.
  // RemovePrimitives deletes the listed triangles (add indices, each at most once; false with LastError() and nothing
  // removed otherwise); the survivors keep their relative order and are numbered densely, and the root box is
  // recomputed.  Both leave the flat tree as it is, in the manner of RefitRoot: on a finalized tree it then describes
  // the OLD triangle set, and IntersectRay(s) refuses, until Adopt() or Refit() + Finalize().
  void AppendPrimitive(Primitive* p);
  bool RemovePrimitives(const std::vector<int>& add_indices);
  // A flat tree through `read` (mt_octree_read of a tree, mt_scene_read_tree of a scene: MT_OK or an error code): a
  // first read with no array wanted gives the counts, a second fills the arrays.  The code of a failed read, else 0.
  static int ReadFlat(const std::function<int(mt_octree_arrays*)>& read, FlatTree* out);
  // extension: no "Triangles: N" line on stdout
  void SetQuiet(bool quiet) { quiet_ = quiet; }
  // extension: HIP device of the standalone IntersectRay(s) (MythTracer::SetDevice forwards to it)
  void SetDevice(int hip_device) { device_ = hip_device; }

  // Closest hit of one ray, on the GPU (a batch of one; see IntersectRays for
  // the efficient form).  nullptr when nothing is hit or no GPU is usable (the
  // reason is then available from LastError()).
  const Primitive* IntersectRay(const Ray& ray, V3D* point, V3D::basetype* distance) const;

  // Batch form: rays = n x {origin xyz, direction xyz}.  Outputs may be null.
  // Returns false on a device error.
  bool IntersectRays(int n, const double* rays, const Primitive** prims, double* distances,
                     double* points) const;

  AABB GetAABB() const;

  // --- used by MythTracer / tests
  const FlatTree& Flat() const { return flat_; }
  size_t PrimitiveCount() const { return prims_.size(); }
  const Triangle* GetTriangle(size_t add_index) const;
  // the same triangle, for a caller that gives it another material (Triangle::mtl; MythTracer::UpdateTriangleMaterials).
  // Vertices and boxes are the finalized tree's: a caller that changes them calls Refit() before the tree is used again
  // (MythTracer::SetTriangleVertices / UpdateGeometry do).
  Triangle* MutableTriangle(size_t add_index);
  const char* LastError() const { return error_.c_str(); }
  static const int SPLIT_BOUNDARY = 16;  // octtree.h:43

 private:
  AABB root_aabb_;  // starts as {0,0,0}-{0,0,0} and only grows (octtree.cc:8-14)
  std::vector<std::unique_ptr<Primitive>> prims_;
  FlatTree flat_;
  bool finalized_ = false;
  bool flat_is_stale_ = false;  // AppendPrimitive / RemovePrimitives after Finalize(): flat_ awaits Adopt() or Refit()
  bool quiet_ = false;
  bool device_build_ = false;
  bool FinalizeOnDevice();
  void DropGeometryOnly();
  int device_ = 0;
  mutable mt_scene* geometry_only_ = nullptr;  // for standalone IntersectRay
  mutable std::string error_;
};

}  // namespace raytracer
