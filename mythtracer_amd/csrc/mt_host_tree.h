// mt_host_tree.h — a built octree on the host, and the mt_scene_desc that is made of one.  mt_scene_create_triangles and
// mt_scene_set_triangle_vertices both turn a tree of mt_build.h into the description that mt_layout.h checks and
// derives from; what differs between them, where the per-triangle arrays come from, stays with them.  Host only and
// free of HIP calls: mt_capi.hip does the copies.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "mythtracer_hip.h"

namespace mt {

// The node arrays of an mt_scene_desc and the stream's tri_id
struct HostTree {
  int32_t n_nodes = 0, n_tris = 0, depth = 0;
  std::vector<double> node_aabb, node_center;
  std::vector<int32_t> first_child, prim_begin, prim_count, tri_id;

  // Room for a tree of nn nodes over nt triangles, and the mt_octree_arrays that reads one into it.  tri_id is never
  // empty: a scene made of this tree has a tri_id.  *box_add, where wanted: the triangles' boxes in add order.
  mt_octree_arrays room_for(int32_t nn, int32_t nt, std::vector<double> *box_add) {
    node_aabb.resize((size_t)nn * 6);
    node_center.resize((size_t)nn * 3);
    first_child.resize((size_t)nn);
    prim_begin.resize((size_t)nn);
    prim_count.resize((size_t)nn);
    tri_id.resize(nt ? (size_t)nt : 1);
    if (box_add) box_add->resize((size_t)nt * 6);
    mt_octree_arrays a;
    memset(&a, 0, sizeof a);
    a.node_aabb = node_aabb.data();
    a.node_center = node_center.data();
    a.first_child = first_child.data();
    a.prim_begin = prim_begin.data();
    a.prim_count = prim_count.data();
    a.tri_id = tri_id.data();
    a.tri_aabb = box_add ? box_add->data() : nullptr;
    return a;
  }
};

// a zeroed mt_scene_desc with its size, ABI version, device and the counts that no tree decides
inline mt_scene_desc new_scene_desc(int device, int n_tris, int n_materials, int n_textures) {
  mt_scene_desc sd;
  memset(&sd, 0, sizeof sd);
  sd.struct_size = sizeof sd;
  sd.abi_version = MT_ABI_VERSION;
  sd.device = device;
  sd.n_tris = n_tris;
  sd.n_materials = n_materials;
  sd.n_textures = n_textures;
  return sd;
}

// the node half of *sd, and its tri_id, from T (which must outlive the use of *sd)
inline void describe_tree(const HostTree &T, mt_scene_desc *sd) {
  sd->n_nodes = T.n_nodes;
  sd->tree_depth = T.depth;
  sd->node_aabb = T.node_aabb.data();
  sd->node_center = T.node_center.data();
  sd->node_first_child = T.first_child.data();
  sd->node_prim_begin = T.prim_begin.data();
  sd->node_prim_count = T.prim_count.data();
  sd->tri_id = T.tri_id.data();
}

}  // namespace mt
