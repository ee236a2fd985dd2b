// mythtracer.cc — MythTracer / WorkChunk of the facade (reference:
// VerStarting/mythtracer.cc:243-429).  Everything under the reference's pixel
// loop (mythtracer.cc:292-305) is one kernel launch behind mt_render_chunk.
#include "mythtracer.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <limits>
#include <unordered_map>

#include "flatten.h"
#include "mythtracer_hip.h"
#include "primitive_triangle.h"

namespace raytracer {

MythTracer::MythTracer() {}

MythTracer::~MythTracer() { DropDeviceScenes(); }

void MythTracer::DropDeviceScenes() {
  if (dev_) mt_scene_destroy(dev_);
  dev_ = nullptr;
  for (mt_scene* r : replicas_) mt_scene_destroy(r);
  replicas_.clear();
}

void MythTracer::SetDevices(const std::vector<int>& hip_devices) {
  DropDeviceScenes();  // uploaded again, where they are wanted, by the next Prepare
  devices_ = hip_devices;
  if (!devices_.empty()) SetDevice(devices_[0]);
}

Scene* MythTracer::GetScene() { return &scene; }

bool MythTracer::LoadObj(const char* fname) {
  if (!quiet_) puts("Reading .OBJ file.");
  ObjFileReader reader;
  if (!reader.ReadObjFile(&scene, fname)) return false;
  was_scene_finalized = false;
  return true;
}

namespace {

// Textures whose texels all came from 8-bit data (colour == k / 255.0, which
// is what both the reference's loader and ours produce) travel as RGB8; the
// kernel re-creates the identical double with byte / 255.0.
bool PackRgb8(const Texture& t, std::vector<uint8_t>* out) {
  out->resize(t.colors.size() * 3);
  for (size_t i = 0; i < t.colors.size(); i++) {
    for (int c = 0; c < 3; c++) {
      const double v = t.colors[i].v[c];
      const int k = (int)(v * 255.0 + 0.5);
      if (!(v >= 0.0 && v <= 1.0) || k < 0 || k > 255 || (double)k / 255.0 != v) {
        out->clear();
        return false;
      }
      (*out)[i * 3 + c] = (uint8_t)k;
    }
  }
  return true;
}

}  // namespace

bool FlatScene::Build(const Scene& scene) {
  const OctTree& tree = scene.tree;
  if (!tree.IsFinalized()) {
    error = "scene tree is not finalized";
    return false;
  }
  if (tree.FlatIsStale()) {
    error = "triangles were added or removed and the tree still describes the old ones: UpdateTrianglesInPlace() first";
    return false;
  }
  const FlatTree& f = tree.Flat();
  const size_t nt = f.tri_id.size();

  // materials / textures -> dense tables, in order of first use
  std::unordered_map<const Material*, int32_t> mtl_index;
  std::unordered_map<const Texture*, int32_t> tex_index;
  std::vector<const Material*> mtls;
  std::vector<const Texture*> texs;
  auto intern_material = [&](const Material* m) -> int32_t {
    if (m == nullptr) return -1;
    auto it = mtl_index.find(m);
    if (it != mtl_index.end()) return it->second;
    const int32_t id = (int32_t)mtls.size();
    mtl_index[m] = id;
    mtls.push_back(m);
    if (m->tex != nullptr && tex_index.find(m->tex) == tex_index.end()) {
      tex_index[m->tex] = (int32_t)texs.size();
      texs.push_back(m->tex);
    }
    return id;
  };

  vertex.resize(nt * 9);
  normal.resize(nt * 9);
  uvw.resize(nt * 9);
  aabb.resize(nt * 6);
  material.resize(nt);
  line_no.resize(nt);
  for (size_t s = 0; s < nt; s++) {
    const Triangle* t = tree.GetTriangle((size_t)f.tri_id[s]);
    memcpy(&vertex[s * 9], t->vertex, 72);
    memcpy(&normal[s * 9], t->normal, 72);
    memcpy(&uvw[s * 9], t->uvw, 72);
    memcpy(&aabb[s * 6], t->cached_aabb.min.v, 24);
    memcpy(&aabb[s * 6 + 3], t->cached_aabb.max.v, 24);
    material[s] = intern_material(t->mtl);
    line_no[s] = t->debug_line_no;
  }
  materials.assign(mtls.size(), mt_material{});
  for (size_t i = 0; i < mtls.size(); i++) materials[i] = FlatMaterial(*mtls[i], mtls[i]->tex ? tex_index[mtls[i]->tex] : -1);
  material_of = mtls;
  texture_of = texs;
  textures.assign(texs.size(), mt_texture{});
  rgb8.assign(texs.size(), {});
  for (size_t i = 0; i < texs.size(); i++) {
    const Texture& t = *texs[i];
    if (t.colors.size() != t.width * t.height || t.width == 0 || t.height == 0) {
      error = "texture with inconsistent size";
      return false;
    }
    mt_texture& o = textures[i];
    o.width = (int32_t)t.width;
    o.height = (int32_t)t.height;
    if (PackRgb8(t, &rgb8[i])) {
      o.format = MT_TEX_RGB8;
      o.texels = rgb8[i].data();
    } else {
      o.format = MT_TEX_F64;
      o.texels = t.colors.data();  // V3D is three packed doubles
    }
  }
  return true;
}

mt_material FlatScene::FlatMaterial(const Material& m, int32_t tex) {
  mt_material o{};
  memcpy(o.ambient, m.ambient.v, 24);
  memcpy(o.diffuse, m.diffuse.v, 24);
  memcpy(o.specular, m.specular.v, 24);
  memcpy(o.transmission_filter, m.transmission_filter.v, 24);
  o.specular_exp = m.specular_exp;
  o.reflectance = m.reflectance;
  o.transparency = m.transparency;
  o.refraction_index = m.refraction_index;
  o.tex = tex;
  return o;
}

mt_scene_desc FlatScene::Describe(const Scene& scene, int device) const {
  const FlatTree& f = scene.tree.Flat();
  mt_scene_desc d;
  memset(&d, 0, sizeof d);
  d.struct_size = sizeof d;
  d.abi_version = MT_ABI_VERSION;
  d.device = device;
  d.n_nodes = (int32_t)f.NodeCount();
  d.n_tris = (int32_t)f.tri_id.size();
  d.n_materials = (int32_t)materials.size();
  d.n_textures = (int32_t)textures.size();
  d.tree_depth = f.depth;
  d.node_aabb = f.node_aabb.data();
  d.node_center = f.node_center.data();
  d.node_first_child = f.first_child.data();
  d.node_prim_begin = f.prim_begin.data();
  d.node_prim_count = f.prim_count.data();
  d.tri_vertex = vertex.data();
  d.tri_normal = normal.data();
  d.tri_uvw = uvw.data();
  d.tri_aabb = aabb.data();
  d.tri_material = material.data();
  d.tri_line_no = line_no.data();
  d.tri_id = f.tri_id.data();
  d.materials = materials.data();
  d.textures = textures.data();
  return d;
}

bool MythTracer::Prepare() {
  if (!was_scene_finalized) {
    if (!quiet_) puts("Finalizing tree.");
    scene.tree.Finalize();
    DropDeviceScenes();  // geometry changed (LoadObj after a render, UpdateGeometry): upload again
    if (!scene.tree.IsFinalized()) {  // (SetDeviceTreeBuild: the build on the GPU failed, and the host builder is not asked instead)
      error_ = scene.tree.LastError();
      return false;
    }
    was_scene_finalized = true;
  }
  if (dev_) return true;
  FlatScene flat;
  if (!flat.Build(scene)) {
    error_ = flat.error;
    return false;
  }
  // one replica per listed device: every worker of the reference loads its own copy of the scene
  // (main_net_worker.cc:29-32)
  const size_t n = devices_.empty() ? 1 : devices_.size();
  for (size_t r = 0; r < n; r++) {
    const mt_scene_desc d = flat.Describe(scene, devices_.empty() ? device_ : devices_[r]);
    mt_scene* s = mt_scene_create(&d);
    if (s == nullptr) {
      error_ = mt_last_error();
      fprintf(stderr, "error: cannot create the device scene: %s\n", error_.c_str());
      DropDeviceScenes();
      return false;
    }
    (void)mt_scene_set_raytree_uvw(s, keep_uvw_ ? 1 : 0);
    (void)mt_scene_set_raytree_tri(s, keep_tri_ ? 1 : 0);
    if (r == 0) dev_ = s;
    else replicas_.push_back(s);
  }
  // what UpdateMaterials needs of this upload: every material's name, the dense table's names in its order, the
  // uploaded textures
  uploaded_names_.clear();
  for (const auto& kv : scene.materials) uploaded_names_.push_back(kv.first);
  std::sort(uploaded_names_.begin(), uploaded_names_.end());
  dense_names_.assign(flat.material_of.size(), std::string());
  for (const auto& kv : scene.materials) {
    for (size_t i = 0; i < flat.material_of.size(); i++) {
      if (flat.material_of[i] == kv.second.get()) dense_names_[i] = kv.first;
    }
  }
  uploaded_textures_ = flat.texture_of;
  uploaded_materials_ = flat.material_of;
  moved_.clear();  // (the upload took every vertex as it is)
  ForgetEdit();    // (... and every triangle)
  return true;
}

void MythTracer::ForgetEdit() {
  removed_.clear();
  removal_pending_ = false;
  added_ = 0;
}

bool MythTracer::SetTriangleVertices(const std::vector<int>& add_indices, const std::vector<V3D>& vertices) {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  if (EditPending()) {
    return refuse("triangles were added or removed and the edit is pending: UpdateTrianglesInPlace() first");
  }
  if (vertices.size() != add_indices.size() * 3) {
    return refuse(std::to_string(add_indices.size()) + " triangles need " + std::to_string(add_indices.size() * 3) +
                  " vertices, not " + std::to_string(vertices.size()));
  }
  for (int i : add_indices) {
    if (i < 0 || (size_t)i >= scene.tree.PrimitiveCount()) {
      return refuse("triangle index " + std::to_string(i) + " outside the scene's " +
                    std::to_string(scene.tree.PrimitiveCount()) + " triangles");
    }
  }
  for (size_t k = 0; k < add_indices.size(); k++) {
    Triangle* t = scene.tree.MutableTriangle((size_t)add_indices[k]);
    for (int v = 0; v < 3; v++) t->vertex[v] = vertices[k * 3 + (size_t)v];
    t->CacheAABB();
  }
  moved_.insert(moved_.end(), add_indices.begin(), add_indices.end());
  return true;
}

void MythTracer::UpdateGeometry() {
  scene.tree.Refit();
  was_scene_finalized = false;
  moved_.clear();
  ForgetEdit();
  DropDeviceScenes();
}

bool MythTracer::AddTriangle(Triangle* triangle) {
  if (triangle == nullptr) {
    error_ = "AddTriangle: the triangle is NULL";
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  }
  if (!moved_.empty()) {  // (their indices are the uploaded scene's, like a removal's)
    error_ = "triangles moved by SetTriangleVertices are pending: UpdateGeometryInPlace() first";
    fprintf(stderr, "error: %s\n", error_.c_str());
    delete triangle;
    return false;
  }
  scene.tree.AppendPrimitive(triangle);
  added_++;
  HostOnlyEdit();
  return true;
}

// With nothing uploaded there is no scene to edit in place: the tree is built again by the next Prepare.
void MythTracer::HostOnlyEdit() {
  if (dev_ != nullptr) return;
  if (scene.tree.IsFinalized()) scene.tree.Refit();
  was_scene_finalized = false;
}

bool MythTracer::RemoveTriangles(const std::vector<int>& add_indices) {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  if (!moved_.empty()) {  // (a removal renumbers the triangles that the moved indices name)
    return refuse("triangles moved by SetTriangleVertices are pending: UpdateGeometryInPlace() first");
  }
  if (removal_pending_) {
    return refuse("RemoveTriangles was called already since the last upload or update: UpdateTrianglesInPlace() first");
  }
  if (added_ > 0) {
    return refuse("triangles were added since the last upload or update, so the indices would not be the uploaded "
                  "scene's: UpdateTrianglesInPlace() first");
  }
  if (!scene.tree.RemovePrimitives(add_indices)) return refuse(scene.tree.LastError());
  removed_.assign(add_indices.begin(), add_indices.end());
  removal_pending_ = true;
  HostOnlyEdit();
  return true;
}

bool MythTracer::UpdateTrianglesInPlace() {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  if (!was_scene_finalized || dev_ == nullptr) {  // nothing uploaded yet: the upload takes the triangles as they are
    UpdateGeometry();
    return Prepare();
  }
  if (!moved_.empty()) {
    return refuse("triangles moved by SetTriangleVertices are pending: UpdateGeometryInPlace() first");
  }
  if (!EditPending()) return true;
  // the added triangles: the host tree's last ones, their materials through the uploaded dense table
  const size_t nt = scene.tree.PrimitiveCount(), na = added_;
  std::unordered_map<const Material*, int32_t> index;
  for (size_t i = 0; i < uploaded_materials_.size(); i++) index[uploaded_materials_[i]] = (int32_t)i;
  std::vector<double> vertex(na * 9), normal(na * 9), uvw(na * 9);
  std::vector<int32_t> material(na), line_no(na);
  for (size_t j = 0; j < na; j++) {
    const Triangle* t = scene.tree.GetTriangle(nt - na + j);
    memcpy(&vertex[j * 9], t->vertex, 72);
    memcpy(&normal[j * 9], t->normal, 72);
    memcpy(&uvw[j * 9], t->uvw, 72);
    line_no[j] = t->debug_line_no;
    material[j] = -1;
    if (t->mtl != nullptr) {
      const auto it = index.find(t->mtl);
      if (it == index.end()) {
        return refuse("added triangle " + std::to_string(nt - na + j) + " points at a material that was not uploaded: "
                      "UpdateTrianglesInPlace adds no material (UpdateGeometry() uploads the scene anew)");
      }
      material[j] = it->second;
    }
  }
  // From here on a refusal leaves no replica behind the host: everything is dropped and uploaded anew by the next Prepare.
  auto give_up = [&](const std::string& why) {
    const std::string text = why + mt_last_error();
    UpdateGeometry();
    return refuse(text);
  };
  scene.tree.RefitRoot();
  std::vector<mt_scene*> all(1, dev_);
  all.insert(all.end(), replicas_.begin(), replicas_.end());
  for (size_t r = 0; r < all.size(); r++) {
    if (mt_scene_edit_triangles(all[r], removed_.data(), (int)removed_.size(), (int)na, vertex.data(), normal.data(), uvw.data(),
                                material.data(), line_no.data(), nullptr) != MT_OK) {
      return give_up(r == 0 ? "editing the triangles in place failed: " : "editing the triangles in place failed on a replica: ");
    }
    if (r == 0) {  // at once its new tree: the host tree speaks the order dev_ speaks
      FlatTree f;
      mt_scene* const first = dev_;
      if (OctTree::ReadFlat([first](mt_octree_arrays* a) { return mt_scene_read_tree(first, a); }, &f) != MT_OK) {
        return give_up("reading the edited tree failed: ");
      }
      scene.tree.Adopt(std::move(f));
    }
  }
  ForgetEdit();
  return true;
}

bool MythTracer::UpdateGeometryInPlace() {
  if (!was_scene_finalized || dev_ == nullptr) {  // nothing uploaded yet: the upload takes the vertices as they are
    UpdateGeometry();
    return Prepare();
  }
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  if (EditPending()) {  // (the host's triangles are numbered anew already; the devices' are not)
    return refuse("triangles were added or removed and the edit is pending: UpdateTrianglesInPlace() first");
  }
  scene.tree.RefitRoot();
  // the moved triangles, each once (all of them when the caller edited MutableTriangle(i)->vertex itself)
  const size_t nt = scene.tree.PrimitiveCount();
  std::vector<int32_t> idx;
  if (moved_.empty()) {
    idx.resize(nt);
    for (size_t i = 0; i < nt; i++) idx[i] = (int32_t)i;
  } else {
    std::vector<bool> seen(nt, false);
    for (int i : moved_) {
      if (!seen[(size_t)i]) idx.push_back((int32_t)i);
      seen[(size_t)i] = true;
    }
  }
  std::vector<double> vtx(idx.size() * 9);
  for (size_t k = 0; k < idx.size(); k++) memcpy(&vtx[k * 9], scene.tree.GetTriangle((size_t)idx[k])->vertex, 72);
  // The first replica, and at once its new tree: from here on the host tree speaks the order dev_ speaks, whatever a
  // later replica answers.
  if (mt_scene_set_triangle_vertices(dev_, idx.data(), (int)idx.size(), vtx.data(), nullptr) != MT_OK) {
    return refuse(std::string("moving the triangles in place failed: ") + mt_last_error());
  }
  FlatTree f;
  mt_scene* const first = dev_;
  if (OctTree::ReadFlat([first](mt_octree_arrays* a) { return mt_scene_read_tree(first, a); }, &f) != MT_OK) {
    return refuse(std::string("reading the moved tree failed: ") + mt_last_error());
  }
  scene.tree.Adopt(std::move(f));
  // The other replicas.  One that refuses keeps its old geometry while dev_ has moved: moved_ is kept, so a repeated
  // call moves the replicas that are behind (the set is a no-op on those that are not); UpdateGeometry() uploads anew.
  for (mt_scene* s : replicas_) {
    if (mt_scene_set_triangle_vertices(s, idx.data(), (int)idx.size(), vtx.data(), nullptr) != MT_OK) {
      return refuse(std::string("moving the triangles in place failed on a replica: ") + mt_last_error());
    }
  }
  moved_.clear();
  return true;
}

bool MythTracer::UpdateTriangleMaterials() {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  if (!was_scene_finalized || dev_ == nullptr) return Prepare();  // nothing uploaded yet: the upload takes them as they are
  if (EditPending()) return refuse("triangles were added or removed and the edit is pending: UpdateTrianglesInPlace() first");
  // FlatScene::Build's stream order, through the uploaded dense table
  const FlatTree& f = scene.tree.Flat();
  std::unordered_map<const Material*, int32_t> index;
  for (size_t i = 0; i < uploaded_materials_.size(); i++) index[uploaded_materials_[i]] = (int32_t)i;
  std::vector<int32_t> material(f.tri_id.size());
  for (size_t s = 0; s < material.size(); s++) {
    const Triangle* t = scene.tree.GetTriangle((size_t)f.tri_id[s]);
    if (t->mtl == nullptr) {
      material[s] = -1;
      continue;
    }
    const auto it = index.find(t->mtl);
    if (it == index.end()) {
      return refuse("triangle " + std::to_string(f.tri_id[s]) + " points at a material that was not uploaded: "
                    "UpdateTriangleMaterials edits, it does not add");
    }
    material[s] = it->second;
  }
  std::vector<mt_scene*> all(1, dev_);
  all.insert(all.end(), replicas_.begin(), replicas_.end());
  for (mt_scene* s : all) {
    if (mt_scene_set_triangle_materials(s, material.data(), (int)material.size()) != MT_OK) {
      return refuse(std::string("triangle material update failed: ") + mt_last_error());
    }
  }
  return true;
}

bool MythTracer::UpdateTriangleAttributes() {
  if (!was_scene_finalized || dev_ == nullptr) return Prepare();  // nothing uploaded yet: the upload takes them as they are
  if (EditPending()) {
    error_ = "triangles were added or removed and the edit is pending: UpdateTrianglesInPlace() first";
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  }
  // FlatScene::Build's stream order
  const FlatTree& f = scene.tree.Flat();
  const size_t nt = f.tri_id.size();
  std::vector<double> normal(nt * 9), uvw(nt * 9);
  for (size_t s = 0; s < nt; s++) {
    const Triangle* t = scene.tree.GetTriangle((size_t)f.tri_id[s]);
    memcpy(&normal[s * 9], t->normal, 72);
    memcpy(&uvw[s * 9], t->uvw, 72);
  }
  std::vector<mt_scene*> all(1, dev_);
  all.insert(all.end(), replicas_.begin(), replicas_.end());
  for (mt_scene* s : all) {
    if (mt_scene_set_triangle_normals(s, normal.data(), (int)nt) != MT_OK ||
        mt_scene_set_triangle_uvw(s, uvw.data(), (int)nt) != MT_OK) {
      error_ = std::string("triangle attribute update failed: ") + mt_last_error();
      fprintf(stderr, "error: %s\n", error_.c_str());
      return false;
    }
  }
  return true;
}

void MythTracer::SetRayTreeKeepTriangles(bool keep) {
  keep_tri_ = keep;
  if (dev_ != nullptr) (void)mt_scene_set_raytree_tri(dev_, keep ? 1 : 0);
  for (mt_scene* s : replicas_) (void)mt_scene_set_raytree_tri(s, keep ? 1 : 0);
}

bool MythTracer::UpdateMaterials() {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  if (!was_scene_finalized || dev_ == nullptr) return Prepare();  // nothing uploaded yet: the upload takes them as they are
  std::vector<std::string> names;
  for (const auto& kv : scene.materials) names.push_back(kv.first);
  std::sort(names.begin(), names.end());
  if (names != uploaded_names_) {
    return refuse("the scene's materials are not the uploaded ones by name: UpdateMaterials edits, it neither adds nor removes");
  }
  std::vector<mt_material> table(dense_names_.size());
  for (size_t i = 0; i < dense_names_.size(); i++) {
    const Material& m = *scene.materials.at(dense_names_[i]);
    int32_t tex = -1;
    if (m.tex != nullptr) {
      for (size_t k = 0; k < uploaded_textures_.size(); k++) {
        if (uploaded_textures_[k] == m.tex) tex = (int32_t)k;
      }
      if (tex < 0) return refuse("material " + dense_names_[i] + " points at a texture that was not uploaded");
    }
    table[i] = FlatScene::FlatMaterial(m, tex);
  }
  std::vector<mt_scene*> all(1, dev_);
  all.insert(all.end(), replicas_.begin(), replicas_.end());
  for (mt_scene* s : all) {
    if (mt_scene_set_materials(s, table.data(), (int)table.size()) != MT_OK) {
      return refuse(std::string("material update failed: ") + mt_last_error());
    }
  }
  return true;
}

bool MythTracer::UpdateTexture(const std::string& key) {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  if (!was_scene_finalized || dev_ == nullptr) return Prepare();  // nothing uploaded yet: the upload takes it as it is
  const auto it = scene.textures.find(key);
  if (it == scene.textures.end()) return refuse("the scene has no texture " + key);
  const Texture& t = *it->second;
  int index = -1;
  for (size_t k = 0; k < uploaded_textures_.size(); k++) {
    if (uploaded_textures_[k] == &t) index = (int)k;
  }
  if (index < 0) return refuse("texture " + key + " was not uploaded: UpdateTexture edits, it neither adds nor removes");
  if (t.colors.size() != t.width * t.height || t.width == 0 || t.height == 0) {
    return refuse("texture with inconsistent size");
  }
  // FlatScene::Build's choice of format
  mt_texture o{};
  o.width = (int32_t)t.width;
  o.height = (int32_t)t.height;
  std::vector<uint8_t> rgb8;
  if (PackRgb8(t, &rgb8)) {
    o.format = MT_TEX_RGB8;
    o.texels = rgb8.data();
  } else {
    o.format = MT_TEX_F64;
    o.texels = t.colors.data();  // V3D is three packed doubles
  }
  std::vector<mt_scene*> all(1, dev_);
  all.insert(all.end(), replicas_.begin(), replicas_.end());
  for (mt_scene* s : all) {
    if (mt_scene_set_texture(s, index, &o) != MT_OK) {
      return refuse(std::string("texture update failed: ") + mt_last_error());
    }
  }
  return true;
}

void MythTracer::SetRayTreeKeepUVW(bool keep) {
  keep_uvw_ = keep;
  if (dev_ != nullptr) (void)mt_scene_set_raytree_uvw(dev_, keep ? 1 : 0);
  for (mt_scene* s : replicas_) (void)mt_scene_set_raytree_uvw(s, keep ? 1 : 0);
}

bool MythTracer::UpdateRayTreeMaterials(RayTree* tree) {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  // (the facade's own refusals, before anything touches a device)
  if (devices_.size() > 1) return refuse("the ray tree is not supported with several devices (SetDevices)");
  if (tree == nullptr) return refuse("RayTree is NULL");
  if (tree->Empty()) return refuse("the RayTree is empty: BuildRayTree first");
  if (dev_ != nullptr &&
      mt_scene_set_lights(dev_, reinterpret_cast<const mt_light*>(scene.lights.data()), (int)scene.lights.size()) != MT_OK) {
    return refuse(std::string("ray-tree material update failed: ") + mt_last_error());
  }
  mt_stats st;
  memset(&st, 0, sizeof st);
  if (dev_ != nullptr) (void)mt_scene_set_stats(dev_, collect_stats_ ? 1 : 0);
  if (mt_raytree_update_materials(tree->Get(), &st) != MT_OK) {
    return refuse(std::string("ray-tree material update failed: ") + mt_last_error());
  }
  stats_ = RenderStats{};
  stats_.rays_shadow = st.rays_shadow;
  stats_.box_tests = st.box_tests;
  stats_.node_visits = st.node_visits;
  stats_.tri_tests = st.tri_tests;
  stats_.mt_tests = st.mt_tests;
  stats_.kernel_ms = st.kernel_ms;
  stats_.total_ms = st.total_ms;
  return true;
}

bool MythTracer::RegrowRayTree(RayTree* tree) {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  // (the facade's own refusals, before anything touches a device)
  if (devices_.size() > 1) return refuse("the ray tree is not supported with several devices (SetDevices)");
  if (tree == nullptr) return refuse("RayTree is NULL");
  if (tree->Empty()) return refuse("the RayTree is empty: BuildRayTree first");
  if (dev_ != nullptr &&
      mt_scene_set_lights(dev_, reinterpret_cast<const mt_light*>(scene.lights.data()), (int)scene.lights.size()) != MT_OK) {
    return refuse(std::string("ray-tree regrow failed: ") + mt_last_error());
  }
  mt_stats st;
  memset(&st, 0, sizeof st);
  mt_raytree_regrow_info info;
  if (dev_ != nullptr) (void)mt_scene_set_stats(dev_, collect_stats_ ? 1 : 0);
  if (mt_raytree_regrow_materials(tree->Get(), &info, &st) != MT_OK) {
    return refuse(std::string("ray-tree regrow failed: ") + mt_last_error());
  }
  stats_ = RenderStats{};
  stats_.rays_secondary = st.rays_secondary;
  stats_.rays_shadow = st.rays_shadow;
  stats_.box_tests = st.box_tests;
  stats_.node_visits = st.node_visits;
  stats_.tri_tests = st.tri_tests;
  stats_.mt_tests = st.mt_tests;
  stats_.shaded_hits = st.shaded_hits;
  stats_.kernel_ms = st.kernel_ms;
  stats_.total_ms = st.total_ms;
  return true;
}

// The supersampling factor is checked before anything touches a device: a caller without one sees this message too.
bool MythTracer::CheckSupersampling(int image_width, int image_height, bool on_all_devices) {
  // (SetAdaptiveSupersampling wins over SetSupersampling)
  const bool adaptive = adaptive_ss_ > 1;
  const int s = adaptive ? adaptive_ss_ : supersampling_;
  const std::string what = adaptive ? "adaptive supersampling" : "supersampling";
  if (s < 1 || s > 4) {
    error_ = what + " factor " + std::to_string(s) + " outside 1 .. 4";
  } else if (adaptive && (adaptive_threshold_ < 0 || adaptive_threshold_ > 255)) {
    error_ = "adaptive supersampling threshold " + std::to_string(adaptive_threshold_) + " outside 0 .. 255";
  } else if (s > 1 && on_all_devices && devices_.size() > 1) {
    error_ = what + " is not supported with several devices (SetDevices)";
  } else if (s > 1 && (image_width <= 0 || image_height <= 0 || image_width > 100000 / s || image_height > 100000 / s)) {
    error_ = "image size " + std::to_string(image_width) + "x" + std::to_string(image_height) + " out of range for supersampling factor " + std::to_string(s);
  } else {
    return true;
  }
  fprintf(stderr, "error: %s\n", error_.c_str());
  return false;
}

bool MythTracer::RayTrace(int image_width, int image_height, Camera* camera,
                          std::vector<uint8_t>* output_bitmap) {
  if (!CheckSupersampling(image_width, image_height, true)) return false;
  if (devices_.size() > 1) {
    // the whole frame on all listed GPUs (mt_render_frame_multi); 64x64 tiles, finer than the master's 128x128
    // chunks (main_net_master.cc:24-25): a pixel's cost varies 60-fold across the frame
    if (!Prepare()) return false;
    if (!quiet_) puts("Rendering.");
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<mt_scene*> all{dev_};
    all.insert(all.end(), replicas_.begin(), replicas_.end());
    for (mt_scene* s : all) {
      if (mt_scene_set_lights(s, reinterpret_cast<const mt_light*>(scene.lights.data()), (int)scene.lights.size()) != MT_OK) {
        error_ = mt_last_error();
        return false;
      }
    }
    const Camera::Sensor sensor = camera->GetSensor(image_width, image_height);
    mt_sensor ms;
    memcpy(ms.origin, camera->origin.v, 24);
    memcpy(ms.start_point, sensor.StartPoint().v, 24);
    memcpy(ms.delta_scanline, sensor.DeltaScanline().v, 24);
    memcpy(ms.delta_pixel, sensor.DeltaPixel().v, 24);
    output_bitmap->resize((size_t)image_width * image_height * 3);
    std::vector<mt_stats> st(all.size());
    if (mt_render_frame_multi(all.data(), (int)all.size(), &ms, image_width, image_height, 64, 64, max_level_,
                              output_bitmap->data(), st.data()) != MT_OK) {
      error_ = mt_last_error();
      fprintf(stderr, "error: render failed: %s\n", error_.c_str());
      return false;
    }
    stats_ = RenderStats{};
    for (const mt_stats& q : st) {
      stats_.rays_primary += q.rays_primary;
      stats_.rays_secondary += q.rays_secondary;
      stats_.rays_shadow += q.rays_shadow;
      stats_.box_tests += q.box_tests;
      stats_.node_visits += q.node_visits;
      stats_.tri_tests += q.tri_tests;
      stats_.mt_tests += q.mt_tests;
      stats_.shaded_hits += q.shaded_hits;
      if (q.kernel_ms > stats_.kernel_ms) stats_.kernel_ms = q.kernel_ms;  // the slowest replica
      stats_.total_ms = q.total_ms;
    }
    if (!quiet_) printf("%.3fs\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return true;
  }
  // (mythtracer.cc:258-278 wraps a full-frame WorkChunk and resizes the caller's vector.)  The chunk borrows the caller's
  // vector: a frame loop that hands the same vector in again (main_local.cc:51-132) keeps its storage -- no 6 MB
  // allocation with its page faults per frame.
  WorkChunk chunk{image_width, image_height, 0, 0, image_width, image_height, *camera, {}, {}};
  chunk.output_bitmap.swap(*output_bitmap);
  chunk.output_bitmap.resize((size_t)image_width * image_height * 3);
  const bool ok = RayTrace(&chunk);
  output_bitmap->swap(chunk.output_bitmap);
  return ok;
}

bool MythTracer::RayTrace(WorkChunk* chunk) {
  if (!CheckSupersampling(chunk->image_width, chunk->image_height, false)) return false;
  const bool adaptive = adaptive_ss_ > 1;
  const int ss = adaptive ? adaptive_ss_ : supersampling_;
  if (ss > 1 && !chunk->output_debug.empty()) {
    error_ = adaptive ? "WorkChunk::output_debug is not available with adaptive supersampling"
                      : "WorkChunk::output_debug is not available with supersampling";
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  }
  if (!Prepare()) return false;
  if (!quiet_) puts("Rendering.");
  const auto t0 = std::chrono::steady_clock::now();

  // Lights are re-read on every call: callers rewrite scene.lights between
  // frames (main_local.cc:79-110).
  static_assert(sizeof(Light) == sizeof(mt_light), "Light must match mt_light");
  if (mt_scene_set_lights(dev_, reinterpret_cast<const mt_light*>(scene.lights.data()),
                          (int)scene.lights.size()) != MT_OK) {
    error_ = mt_last_error();
    return false;
  }
  // (the sensor of the sample grid: ss x ss rays inside every pixel; ss = 1: the reference's)
  const Camera::Sensor sensor = chunk->camera.GetSensor(ss * chunk->image_width, ss * chunk->image_height);
  mt_sensor ms;
  memcpy(ms.origin, chunk->camera.origin.v, 24);
  memcpy(ms.start_point, sensor.StartPoint().v, 24);
  memcpy(ms.delta_scanline, sensor.DeltaScanline().v, 24);
  memcpy(ms.delta_pixel, sensor.DeltaPixel().v, 24);
  mt_sensor ms1 = ms;  // adaptive: the sensor of the output grid for the plain pass, `ms` for the refined blocks
  if (adaptive) {
    const Camera::Sensor plain = chunk->camera.GetSensor(chunk->image_width, chunk->image_height);
    memcpy(ms1.start_point, plain.StartPoint().v, 24);
    memcpy(ms1.delta_scanline, plain.DeltaScanline().v, 24);
    memcpy(ms1.delta_pixel, plain.DeltaPixel().v, 24);
  }

  const size_t npx = (size_t)chunk->chunk_width * (size_t)chunk->chunk_height;
  if (chunk->output_bitmap.size() < npx * 3) {
    error_ = "WorkChunk::output_bitmap is smaller than chunk_width*chunk_height*3";
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  }
  std::vector<mt_debug_px> dbg;
  const bool want_debug = !chunk->output_debug.empty();
  if (want_debug) {
    if (chunk->output_debug.size() < npx) {
      error_ = "WorkChunk::output_debug is smaller than chunk_width*chunk_height";
      return false;
    }
    dbg.resize(npx);
  }
  mt_stats st;
  memset(&st, 0, sizeof st);
  (void)mt_scene_set_stats(dev_, collect_stats_ ? 1 : 0);
  const int rc = adaptive ? mt_render_chunk_adaptive(dev_, &ms1, &ms, chunk->image_width, chunk->image_height,
                                                     chunk->chunk_x, chunk->chunk_y, chunk->chunk_width,
                                                     chunk->chunk_height, ss, adaptive_threshold_, max_level_,
                                                     chunk->output_bitmap.data(), nullptr, nullptr,
                                                     collect_stats_ ? &st : nullptr)
           : ss > 1 ? mt_render_chunk_ss(dev_, &ms, chunk->image_width, chunk->image_height, chunk->chunk_x,
                                             chunk->chunk_y, chunk->chunk_width, chunk->chunk_height, ss, max_level_,
                                             chunk->output_bitmap.data(), collect_stats_ ? &st : nullptr)
                        : mt_render_chunk(dev_, &ms, chunk->image_width, chunk->image_height, chunk->chunk_x,
                                          chunk->chunk_y, chunk->chunk_width, chunk->chunk_height, max_level_,
                                          chunk->output_bitmap.data(), want_debug ? dbg.data() : nullptr,
                                          collect_stats_ ? &st : nullptr);
  if (rc != MT_OK) {
    error_ = mt_last_error();
    fprintf(stderr, "error: render failed: %s\n", error_.c_str());
    return false;
  }
  for (size_t i = 0; want_debug && i < npx; i++) {
    chunk->output_debug[i].line_no = dbg[i].line_no;
    chunk->output_debug[i].point = {dbg[i].point[0], dbg[i].point[1], dbg[i].point[2]};
  }
  stats_.rays_primary = st.rays_primary;
  stats_.rays_secondary = st.rays_secondary;
  stats_.rays_shadow = st.rays_shadow;
  stats_.box_tests = st.box_tests;
  stats_.node_visits = st.node_visits;
  stats_.tri_tests = st.tri_tests;
  stats_.mt_tests = st.mt_tests;
  stats_.shaded_hits = st.shaded_hits;
  stats_.kernel_ms = st.kernel_ms;
  stats_.total_ms = st.total_ms;
  if (!quiet_) {
    // wall-clock, unlike the reference's clock() (process CPU time)
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%.3fs\n", sec);
  }
  return true;
}

bool MythTracer::RayTraceGBuffer(int image_width, int image_height, Camera* camera, GBuffer* out) {
  WorkChunk chunk{image_width, image_height, 0, 0, image_width, image_height, *camera, {}, {}};
  return RayTraceGBuffer(&chunk, out);
}

bool MythTracer::RayTraceGBuffer(WorkChunk* chunk, GBuffer* out) {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  // (checked before anything touches a device: a caller without one sees these messages too)
  if (out == nullptr) return refuse("GBuffer is NULL");
  if (devices_.size() > 1) return refuse("the G-buffer is not supported with several devices (SetDevices)");
  if ((out->channels & GBuffer::kAll) == 0) return refuse("GBuffer::channels selects no plane");
  if (chunk->chunk_width <= 0 || chunk->chunk_height <= 0) return refuse("empty chunk");
  if (!Prepare()) return false;
  // (the reference's sensor of the image: one ray per pixel, whatever SetSupersampling says)
  const Camera::Sensor sensor = chunk->camera.GetSensor(chunk->image_width, chunk->image_height);
  mt_sensor ms;
  memcpy(ms.origin, chunk->camera.origin.v, 24);
  memcpy(ms.start_point, sensor.StartPoint().v, 24);
  memcpy(ms.delta_scanline, sensor.DeltaScanline().v, 24);
  memcpy(ms.delta_pixel, sensor.DeltaPixel().v, 24);
  const size_t npx = (size_t)chunk->chunk_width * (size_t)chunk->chunk_height;
  const unsigned c = out->channels;
  auto sized = [&](auto& v, unsigned bit, size_t per_px) -> decltype(v.data()) {
    v.clear();
    if (!(c & bit)) return nullptr;
    v.resize(npx * per_px);
    return v.data();
  };
  mt_gbuffer g;
  g.depth = sized(out->depth, GBuffer::kDepth, 1);
  g.point = sized(out->point, GBuffer::kPoint, 3);
  g.normal = sized(out->normal, GBuffer::kNormal, 3);
  g.uvw = sized(out->uvw, GBuffer::kUvw, 3);
  g.albedo = sized(out->albedo, GBuffer::kAlbedo, 3);
  g.prim = sized(out->prim, GBuffer::kPrim, 1);
  g.line_no = sized(out->line_no, GBuffer::kLineNo, 1);
  g.material = sized(out->material, GBuffer::kMaterial, 1);
  out->width = chunk->chunk_width;
  out->height = chunk->chunk_height;
  mt_stats st;
  memset(&st, 0, sizeof st);
  (void)mt_scene_set_stats(dev_, collect_stats_ ? 1 : 0);
  if (mt_render_gbuffer(dev_, &ms, chunk->image_width, chunk->image_height, chunk->chunk_x, chunk->chunk_y,
                        chunk->chunk_width, chunk->chunk_height, &g, &st) != MT_OK) {
    return refuse(std::string("G-buffer failed: ") + mt_last_error());
  }
  stats_ = RenderStats{};
  stats_.rays_primary = st.rays_primary;
  stats_.box_tests = st.box_tests;
  stats_.node_visits = st.node_visits;
  stats_.tri_tests = st.tri_tests;
  stats_.mt_tests = st.mt_tests;
  stats_.shaded_hits = st.shaded_hits;
  stats_.kernel_ms = st.kernel_ms;
  stats_.total_ms = st.total_ms;
  return true;
}

namespace {

mt_sensor SensorOf(const WorkChunk& chunk) {
  const Camera::Sensor sensor = chunk.camera.GetSensor(chunk.image_width, chunk.image_height);
  mt_sensor ms;
  memcpy(ms.origin, chunk.camera.origin.v, 24);
  memcpy(ms.start_point, sensor.StartPoint().v, 24);
  memcpy(ms.delta_scanline, sensor.DeltaScanline().v, 24);
  memcpy(ms.delta_pixel, sensor.DeltaPixel().v, 24);
  return ms;
}

}  // namespace

bool MythTracer::RayTraceLightBuffer(int image_width, int image_height, Camera* camera, GBuffer* gbuffer,
                                     LightBuffer* out) {
  WorkChunk chunk{image_width, image_height, 0, 0, image_width, image_height, *camera, {}, {}};
  return RayTraceLightBuffer(&chunk, gbuffer, out);
}

bool MythTracer::RayTraceLightBuffer(WorkChunk* chunk, GBuffer* gbuffer, LightBuffer* out) {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  // (checked before anything touches a device, as in RayTraceGBuffer)
  if (out == nullptr) return refuse("LightBuffer is NULL");
  if (devices_.size() > 1) return refuse("the light buffer is not supported with several devices (SetDevices)");
  if ((out->channels & LightBuffer::kAll) == 0) return refuse("LightBuffer::channels selects no plane");
  if (chunk->chunk_width <= 0 || chunk->chunk_height <= 0) return refuse("empty chunk");
  if (!Prepare()) return false;
  if (mt_scene_set_lights(dev_, reinterpret_cast<const mt_light*>(scene.lights.data()), (int)scene.lights.size()) != MT_OK) {
    return refuse(std::string("light buffer failed: ") + mt_last_error());
  }
  const mt_sensor ms = SensorOf(*chunk);
  const size_t npx = (size_t)chunk->chunk_width * (size_t)chunk->chunk_height;
  const size_t n_l = scene.lights.size();
  const unsigned c = gbuffer ? gbuffer->channels : 0u;
  auto sized = [&](auto& v, unsigned bit, size_t per_px) -> decltype(v.data()) {
    v.clear();
    if (!(c & bit)) return nullptr;
    v.resize(npx * per_px);
    return v.data();
  };
  mt_gbuffer g{};
  if (gbuffer) {
    g.depth = sized(gbuffer->depth, GBuffer::kDepth, 1);
    g.point = sized(gbuffer->point, GBuffer::kPoint, 3);
    g.normal = sized(gbuffer->normal, GBuffer::kNormal, 3);
    g.uvw = sized(gbuffer->uvw, GBuffer::kUvw, 3);
    g.albedo = sized(gbuffer->albedo, GBuffer::kAlbedo, 3);
    g.prim = sized(gbuffer->prim, GBuffer::kPrim, 1);
    g.line_no = sized(gbuffer->line_no, GBuffer::kLineNo, 1);
    g.material = sized(gbuffer->material, GBuffer::kMaterial, 1);
    gbuffer->width = chunk->chunk_width;
    gbuffer->height = chunk->chunk_height;
  }
  // (zero lights: the planes are empty and nothing is written, but a pointer must still say "wanted")
  double no_power = 0;
  uint8_t no_shadow = 0;
  out->power.clear();
  out->in_shadow.clear();
  mt_lightbuffer lb{};
  if (out->channels & LightBuffer::kPower) {
    out->power.resize(n_l * npx * 3);
    lb.power = n_l ? out->power.data() : &no_power;
  }
  if (out->channels & LightBuffer::kInShadow) {
    out->in_shadow.resize(n_l * npx);
    lb.in_shadow = n_l ? out->in_shadow.data() : &no_shadow;
  }
  out->width = chunk->chunk_width;
  out->height = chunk->chunk_height;
  out->n_lights = (int)n_l;
  mt_stats st;
  memset(&st, 0, sizeof st);
  (void)mt_scene_set_stats(dev_, collect_stats_ ? 1 : 0);
  if (mt_render_lightbuffer(dev_, &ms, chunk->image_width, chunk->image_height, chunk->chunk_x, chunk->chunk_y,
                            chunk->chunk_width, chunk->chunk_height, gbuffer ? &g : nullptr, &lb, &st) != MT_OK) {
    return refuse(std::string("light buffer failed: ") + mt_last_error());
  }
  stats_ = RenderStats{};
  stats_.rays_primary = st.rays_primary;
  stats_.rays_shadow = st.rays_shadow;
  stats_.box_tests = st.box_tests;
  stats_.node_visits = st.node_visits;
  stats_.tri_tests = st.tri_tests;
  stats_.mt_tests = st.mt_tests;
  stats_.shaded_hits = st.shaded_hits;
  stats_.kernel_ms = st.kernel_ms;
  stats_.total_ms = st.total_ms;
  return true;
}

bool MythTracer::ShadeDirect(int image_width, int image_height, Camera* camera, const GBuffer& gbuffer,
                             const LightBuffer& lightbuffer, std::vector<uint8_t>* output_bitmap) {
  WorkChunk chunk{image_width, image_height, 0, 0, image_width, image_height, *camera, {}, {}};
  chunk.output_bitmap.swap(*output_bitmap);  // (reuses the caller's allocation)
  const bool ok = ShadeDirect(&chunk, gbuffer, lightbuffer);
  chunk.output_bitmap.swap(*output_bitmap);
  return ok;
}

bool MythTracer::ShadeDirect(WorkChunk* chunk, const GBuffer& gbuffer, const LightBuffer& lightbuffer) {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  if (devices_.size() > 1) return refuse("the relight pass is not supported with several devices (SetDevices)");
  if (chunk->chunk_width <= 0 || chunk->chunk_height <= 0) return refuse("empty chunk");
  const size_t npx = (size_t)chunk->chunk_width * (size_t)chunk->chunk_height;
  const size_t n_l = scene.lights.size();
  if (gbuffer.width != chunk->chunk_width || gbuffer.height != chunk->chunk_height ||
      lightbuffer.width != chunk->chunk_width || lightbuffer.height != chunk->chunk_height) {
    return refuse("the GBuffer and the LightBuffer must describe the chunk");
  }
  if (gbuffer.point.size() != npx * 3 || gbuffer.normal.size() != npx * 3 || gbuffer.albedo.size() != npx * 3 ||
      gbuffer.material.size() != npx) {
    return refuse("ShadeDirect needs the point, normal, albedo and material planes of the GBuffer");
  }
  if ((size_t)lightbuffer.n_lights != n_l) {
    return refuse("the LightBuffer was made with another number of lights: a new RayTraceLightBuffer is needed");
  }
  if (lightbuffer.power.size() != n_l * npx * 3 || lightbuffer.in_shadow.size() != n_l * npx) {
    return refuse("ShadeDirect needs both planes of the LightBuffer");
  }
  if (!Prepare()) return false;
  const mt_sensor ms = SensorOf(*chunk);
  chunk->output_bitmap.resize(npx * 3);
  mt_gbuffer g{};
  g.point = const_cast<double*>(gbuffer.point.data());
  g.normal = const_cast<double*>(gbuffer.normal.data());
  g.albedo = const_cast<double*>(gbuffer.albedo.data());
  g.material = const_cast<int32_t*>(gbuffer.material.data());
  // (zero lights: empty planes, but the pointers must be set)
  double no_power = 0;
  uint8_t no_shadow = 0;
  mt_lightbuffer lb{n_l ? const_cast<double*>(lightbuffer.power.data()) : &no_power,
                    n_l ? const_cast<uint8_t*>(lightbuffer.in_shadow.data()) : &no_shadow};
  mt_stats st;
  memset(&st, 0, sizeof st);
  if (mt_shade_direct(dev_, &ms, chunk->image_width, chunk->image_height, chunk->chunk_x, chunk->chunk_y,
                      chunk->chunk_width, chunk->chunk_height, &g, &lb,
                      reinterpret_cast<const mt_light*>(scene.lights.data()), (int)n_l, chunk->output_bitmap.data(),
                      &st) != MT_OK) {
    return refuse(std::string("relight failed: ") + mt_last_error());
  }
  stats_ = RenderStats{};
  stats_.kernel_ms = st.kernel_ms;
  stats_.total_ms = st.total_ms;
  return true;
}

void RayTree::Reset() {
  if (tree_) mt_raytree_destroy(tree_);
  tree_ = nullptr;
}

namespace {
mt_raytree_desc DescOf(const mt_raytree* t) {
  mt_raytree_desc d;
  memset(&d, 0, sizeof d);
  if (t) (void)mt_raytree_info(t, &d);
  return d;
}
}  // namespace

int RayTree::Layers() const { return DescOf(tree_).n_layers; }
long long RayTree::Rays(int layer) const {
  return layer >= 0 && layer <= MT_MAX_RECURSION ? (long long)DescOf(tree_).n_rays[layer] : 0;
}
int RayTree::Lights() const { return DescOf(tree_).n_lights; }
unsigned long long RayTree::Bytes() const { return DescOf(tree_).bytes; }

bool MythTracer::BuildRayTree(int image_width, int image_height, Camera* camera, RayTree* tree) {
  WorkChunk chunk{image_width, image_height, 0, 0, image_width, image_height, *camera, {}, {}};
  return BuildRayTree(&chunk, tree);
}

bool MythTracer::BuildRayTree(WorkChunk* chunk, RayTree* tree) {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  // (checked before anything touches a device, as in RayTraceGBuffer)
  if (tree == nullptr) return refuse("RayTree is NULL");
  if (devices_.size() > 1) return refuse("the ray tree is not supported with several devices (SetDevices)");
  if (chunk->chunk_width <= 0 || chunk->chunk_height <= 0) return refuse("empty chunk");
  if (max_level_ < 0 || max_level_ > MT_MAX_RECURSION) {
    return refuse("recursion level " + std::to_string(max_level_) + " outside 0 .. " + std::to_string(MT_MAX_RECURSION));
  }
  tree->Reset();
  if (!Prepare()) return false;
  if (mt_scene_set_lights(dev_, reinterpret_cast<const mt_light*>(scene.lights.data()), (int)scene.lights.size()) != MT_OK) {
    return refuse(std::string("ray tree failed: ") + mt_last_error());
  }
  const mt_sensor ms = SensorOf(*chunk);
  mt_stats st;
  memset(&st, 0, sizeof st);
  (void)mt_scene_set_stats(dev_, collect_stats_ ? 1 : 0);
  tree->tree_ = mt_raytree_create(dev_, &ms, chunk->image_width, chunk->image_height, chunk->chunk_x, chunk->chunk_y,
                                  chunk->chunk_width, chunk->chunk_height, max_level_, &st);
  if (tree->tree_ == nullptr) return refuse(std::string("ray tree failed: ") + mt_last_error());
  stats_ = RenderStats{};
  stats_.rays_primary = st.rays_primary;
  stats_.rays_secondary = st.rays_secondary;
  stats_.rays_shadow = st.rays_shadow;
  stats_.box_tests = st.box_tests;
  stats_.node_visits = st.node_visits;
  stats_.tri_tests = st.tri_tests;
  stats_.mt_tests = st.mt_tests;
  stats_.shaded_hits = st.shaded_hits;
  stats_.kernel_ms = st.kernel_ms;
  stats_.total_ms = st.total_ms;
  return true;
}

bool MythTracer::ShadeRayTree(const RayTree& tree, std::vector<uint8_t>* output_bitmap) {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  if (output_bitmap == nullptr) return refuse("the output bitmap is NULL");
  if (devices_.size() > 1) return refuse("the ray tree is not supported with several devices (SetDevices)");
  if (tree.Empty()) return refuse("the RayTree is empty: BuildRayTree first");
  const mt_raytree_desc d = DescOf(tree.Get());
  if ((size_t)d.n_lights != scene.lights.size()) {
    return refuse("the RayTree was made with another number of lights: a new BuildRayTree is needed");
  }
  output_bitmap->resize((size_t)d.chunk_w * (size_t)d.chunk_h * 3);
  mt_stats st;
  memset(&st, 0, sizeof st);
  if (mt_raytree_shade(tree.Get(), reinterpret_cast<const mt_light*>(scene.lights.data()), (int)scene.lights.size(),
                       output_bitmap->data(), &st) != MT_OK) {
    return refuse(std::string("ray-tree shade failed: ") + mt_last_error());
  }
  stats_ = RenderStats{};
  stats_.kernel_ms = st.kernel_ms;
  stats_.total_ms = st.total_ms;
  return true;
}

bool MythTracer::ShadeRayTree(const RayTree& tree, WorkChunk* chunk) {
  if (!tree.Empty()) {
    const mt_raytree_desc d = DescOf(tree.Get());
    if (d.chunk_w != chunk->chunk_width || d.chunk_h != chunk->chunk_height) {
      error_ = "the RayTree must describe the chunk";
      fprintf(stderr, "error: %s\n", error_.c_str());
      return false;
    }
  }
  return ShadeRayTree(tree, &chunk->output_bitmap);
}

bool MythTracer::UpdateRayTree(const std::vector<int>& lights, RayTree* tree) {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  // (the facade's own refusals, before anything touches a device; the indices are checked by the C ABI, below)
  if (devices_.size() > 1) return refuse("the ray tree is not supported with several devices (SetDevices)");
  if (lights.empty()) return refuse("no light is listed");
  if (tree == nullptr) return refuse("RayTree is NULL");
  if (tree->Empty()) return refuse("the RayTree is empty: BuildRayTree first");
  const size_t n_l = scene.lights.size();
  if ((size_t)DescOf(tree->Get()).n_lights != n_l) {
    return refuse("the RayTree was made with another number of lights: a new BuildRayTree is needed");
  }
  if (!Prepare()) return false;
  if (mt_scene_set_lights(dev_, reinterpret_cast<const mt_light*>(scene.lights.data()), (int)n_l) != MT_OK) {
    return refuse(std::string("ray-tree update failed: ") + mt_last_error());
  }
  const std::vector<int32_t> idx(lights.begin(), lights.end());
  mt_stats st;
  memset(&st, 0, sizeof st);
  (void)mt_scene_set_stats(dev_, collect_stats_ ? 1 : 0);
  if (mt_raytree_update_lights(tree->Get(), idx.data(), (int)idx.size(), &st) != MT_OK) {
    return refuse(std::string("ray-tree update failed: ") + mt_last_error());
  }
  stats_ = RenderStats{};
  stats_.rays_shadow = st.rays_shadow;
  stats_.box_tests = st.box_tests;
  stats_.node_visits = st.node_visits;
  stats_.tri_tests = st.tri_tests;
  stats_.mt_tests = st.mt_tests;
  stats_.kernel_ms = st.kernel_ms;
  stats_.total_ms = st.total_ms;
  return true;
}

namespace {
static_assert(sizeof(Ray) == 6 * sizeof(double) && sizeof(V3D) == 3 * sizeof(double),
              "a vector of Ray is the C ABI's [n][6] doubles, a vector of V3D its [n][3]");

// the list's shape, or the reason it has none
bool RayListOf(const std::vector<Ray>& rays, int list_width, mt_ray_list* out, std::string* why) {
  const size_t n = rays.size();
  if (n == 0) {
    *why = "the ray list is empty";
    return false;
  }
  if (list_width < 0 || (list_width > 0 && n % (size_t)list_width != 0)) {
    *why = "list_width " + std::to_string(list_width) + " does not divide the " + std::to_string(n) + " rays";
    return false;
  }
  const size_t w = list_width > 0 ? (size_t)list_width : n;
  if (n >= 0x80000000ull) {
    *why = "a list of " + std::to_string(n) + " rays (2^31 or more)";
    return false;
  }
  memset(out, 0, sizeof *out);
  out->ray = reinterpret_cast<const double*>(rays.data());
  out->list_w = (int32_t)w;
  out->list_h = (int32_t)(n / w);
  return true;
}

void CopyStats(const mt_stats& st, RenderStats* out) {
  *out = RenderStats{};
  out->rays_primary = st.rays_primary;
  out->rays_secondary = st.rays_secondary;
  out->rays_shadow = st.rays_shadow;
  out->box_tests = st.box_tests;
  out->node_visits = st.node_visits;
  out->tri_tests = st.tri_tests;
  out->mt_tests = st.mt_tests;
  out->shaded_hits = st.shaded_hits;
  out->kernel_ms = st.kernel_ms;
  out->total_ms = st.total_ms;
}
}  // namespace

bool MythTracer::BuildRayTree(const std::vector<Ray>& rays, int list_width, RayTree* tree) {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  // (checked before anything touches a device, as in BuildRayTree(WorkChunk*, ...))
  if (tree == nullptr) return refuse("RayTree is NULL");
  if (devices_.size() > 1) return refuse("the ray tree is not supported with several devices (SetDevices)");
  mt_ray_list list;
  std::string why;
  if (!RayListOf(rays, list_width, &list, &why)) return refuse(why);
  if (max_level_ < 0 || max_level_ > MT_MAX_RECURSION) {
    return refuse("recursion level " + std::to_string(max_level_) + " outside 0 .. " + std::to_string(MT_MAX_RECURSION));
  }
  tree->Reset();
  if (!Prepare()) return false;
  if (mt_scene_set_lights(dev_, reinterpret_cast<const mt_light*>(scene.lights.data()), (int)scene.lights.size()) != MT_OK) {
    return refuse(std::string("ray tree failed: ") + mt_last_error());
  }
  mt_stats st;
  memset(&st, 0, sizeof st);
  (void)mt_scene_set_stats(dev_, collect_stats_ ? 1 : 0);
  tree->tree_ = mt_raytree_create_rays(dev_, &list, max_level_, &st);
  if (tree->tree_ == nullptr) return refuse(std::string("ray tree failed: ") + mt_last_error());
  CopyStats(st, &stats_);
  return true;
}

bool MythTracer::ShadeRayTree(const RayTree& tree, std::vector<V3D>* colours) {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  if (colours == nullptr) return refuse("the output colours are NULL");
  if (devices_.size() > 1) return refuse("the ray tree is not supported with several devices (SetDevices)");
  if (tree.Empty()) return refuse("the RayTree is empty: BuildRayTree first");
  const mt_raytree_desc d = DescOf(tree.Get());
  if ((size_t)d.n_lights != scene.lights.size()) {
    return refuse("the RayTree was made with another number of lights: a new BuildRayTree is needed");
  }
  colours->resize((size_t)d.chunk_w * (size_t)d.chunk_h);
  mt_stats st;
  memset(&st, 0, sizeof st);
  if (mt_raytree_shade_colors(tree.Get(), reinterpret_cast<const mt_light*>(scene.lights.data()), (int)scene.lights.size(),
                              reinterpret_cast<double*>(colours->data()), &st) != MT_OK) {
    return refuse(std::string("ray-tree shade failed: ") + mt_last_error());
  }
  stats_ = RenderStats{};
  stats_.kernel_ms = st.kernel_ms;
  stats_.total_ms = st.total_ms;
  return true;
}

bool MythTracer::TraceRays(const std::vector<Ray>& rays, int list_width, std::vector<V3D>* colours,
                           std::vector<uint8_t>* bitmap) {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  // (checked before anything touches a device)
  if (colours == nullptr && bitmap == nullptr) return refuse("the output colours and the output bitmap are both NULL");
  if (devices_.size() > 1) return refuse("the ray tree is not supported with several devices (SetDevices)");
  mt_ray_list list;
  std::string why;
  if (!RayListOf(rays, list_width, &list, &why)) return refuse(why);
  if (max_level_ < 0 || max_level_ > MT_MAX_RECURSION) {
    return refuse("recursion level " + std::to_string(max_level_) + " outside 0 .. " + std::to_string(MT_MAX_RECURSION));
  }
  if (!Prepare()) return false;
  if (mt_scene_set_lights(dev_, reinterpret_cast<const mt_light*>(scene.lights.data()), (int)scene.lights.size()) != MT_OK) {
    return refuse(std::string("tracing the rays failed: ") + mt_last_error());
  }
  if (colours) colours->resize(rays.size());
  if (bitmap) bitmap->resize(rays.size() * 3);
  mt_stats st;
  memset(&st, 0, sizeof st);
  (void)mt_scene_set_stats(dev_, collect_stats_ ? 1 : 0);
  if (mt_trace_rays(dev_, &list, max_level_, colours ? reinterpret_cast<double*>(colours->data()) : nullptr,
                    bitmap ? bitmap->data() : nullptr, &st) != MT_OK) {
    return refuse(std::string("tracing the rays failed: ") + mt_last_error());
  }
  CopyStats(st, &stats_);
  return true;
}

bool MythTracer::UpdateLightBuffer(const GBuffer& gbuffer, const std::vector<int>& lights, LightBuffer* lightbuffer) {
  auto refuse = [&](const std::string& why) {
    error_ = why;
    fprintf(stderr, "error: %s\n", error_.c_str());
    return false;
  };
  // (checked before anything touches a device, as in RayTraceLightBuffer)
  if (lightbuffer == nullptr) return refuse("LightBuffer is NULL");
  if (devices_.size() > 1) return refuse("the light-buffer update is not supported with several devices (SetDevices)");
  if ((lightbuffer->channels & LightBuffer::kAll) == 0) return refuse("LightBuffer::channels selects no plane");
  if (lightbuffer->width <= 0 || lightbuffer->height <= 0) return refuse("empty chunk");
  const size_t npx = (size_t)lightbuffer->width * (size_t)lightbuffer->height;
  const size_t n_l = scene.lights.size();
  if (gbuffer.width != lightbuffer->width || gbuffer.height != lightbuffer->height) {
    return refuse("the GBuffer and the LightBuffer must describe the same chunk");
  }
  if (gbuffer.point.size() != npx * 3 || gbuffer.material.size() != npx) {
    return refuse("UpdateLightBuffer needs the point and material planes of the GBuffer");
  }
  if ((size_t)lightbuffer->n_lights != n_l) {
    return refuse("the LightBuffer was made with another number of lights: a new RayTraceLightBuffer is needed");
  }
  const bool power = (lightbuffer->channels & LightBuffer::kPower) != 0;
  const bool shadow = (lightbuffer->channels & LightBuffer::kInShadow) != 0;
  if ((power && lightbuffer->power.size() != n_l * npx * 3) || (shadow && lightbuffer->in_shadow.size() != n_l * npx)) {
    return refuse("the planes LightBuffer::channels selects do not have the size of n_lights x the chunk");
  }
  if (lights.empty()) return refuse("no light is listed");
  if (!Prepare()) return false;
  if (mt_scene_set_lights(dev_, reinterpret_cast<const mt_light*>(scene.lights.data()), (int)n_l) != MT_OK) {
    return refuse(std::string("light-buffer update failed: ") + mt_last_error());
  }
  mt_gbuffer g{};
  g.point = const_cast<double*>(gbuffer.point.data());
  g.material = const_cast<int32_t*>(gbuffer.material.data());
  mt_lightbuffer lb{power ? lightbuffer->power.data() : nullptr, shadow ? lightbuffer->in_shadow.data() : nullptr};
  std::vector<int32_t> idx(lights.begin(), lights.end());
  mt_stats st;
  memset(&st, 0, sizeof st);
  (void)mt_scene_set_stats(dev_, collect_stats_ ? 1 : 0);
  if (mt_update_lightbuffer(dev_, lightbuffer->width, lightbuffer->height, &g, idx.data(), (int)idx.size(), &lb, &st) !=
      MT_OK) {
    return refuse(std::string("light-buffer update failed: ") + mt_last_error());
  }
  stats_ = RenderStats{};
  stats_.rays_shadow = st.rays_shadow;
  stats_.box_tests = st.box_tests;
  stats_.node_visits = st.node_visits;
  stats_.tri_tests = st.tri_tests;
  stats_.mt_tests = st.mt_tests;
  stats_.kernel_ms = st.kernel_ms;
  stats_.total_ms = st.total_ms;
  return true;
}

// ---- wire format of a chunk (mythtracer.cc:314-429): six little-endian u32
// in, u32 byte count + RGB bytes out.

void WorkChunk::SerializeInput(std::vector<uint8_t>* bytes) {
  const uint32_t f[6] = {(uint32_t)image_width, (uint32_t)image_height, (uint32_t)chunk_x,
                         (uint32_t)chunk_y,     (uint32_t)chunk_width,  (uint32_t)chunk_height};
  bytes->resize(kSerializedInputSize);
  memcpy(bytes->data(), f, sizeof f);
}

bool WorkChunk::DeserializeInput(const std::vector<uint8_t>& bytes) {
  if (bytes.size() != kSerializedInputSize) return false;
  uint32_t f[6];
  memcpy(f, bytes.data(), sizeof f);
  const uint32_t iw = f[0], ih = f[1], cx = f[2], cy = f[3], cw = f[4], ch = f[5];
  const bool sane = iw >= 1 && ih >= 1 && cw >= 1 && ch >= 1 && iw <= 100000 && ih <= 100000 &&
                    cx <= iw && cy <= ih && cw <= iw && ch <= ih && cx + cw <= iw && cy + ch <= ih;
  if (!sane) return false;
  image_width = (int)iw;
  image_height = (int)ih;
  chunk_x = (int)cx;
  chunk_y = (int)cy;
  chunk_width = (int)cw;
  chunk_height = (int)ch;
  return true;
}

bool WorkChunk::SerializeOutput(std::vector<uint8_t>* bytes) {
  if (output_bitmap.size() > std::numeric_limits<uint32_t>::max()) {
    fprintf(stderr, "error: too large WorkerChunk, cannot serialize\n");
    return false;
  }
  const uint32_t n = (uint32_t)output_bitmap.size();
  bytes->resize(sizeof n + n);
  memcpy(bytes->data(), &n, sizeof n);
  if (n) memcpy(bytes->data() + sizeof n, output_bitmap.data(), n);
  return true;
}

bool WorkChunk::DeserializeOutput(const std::vector<uint8_t>& bytes) {
  if (bytes.size() < kSerializedOutputMinimumSize) return false;
  uint32_t n;
  memcpy(&n, bytes.data(), sizeof n);
  const uint64_t want = (uint64_t)chunk_width * (uint64_t)chunk_height * 3;
  if ((uint64_t)n != want) return false;
  // The reference trusts the count and reads n bytes whatever the packet
  // holds (mythtracer.cc:425-426); a short packet is rejected here.
  if (bytes.size() - sizeof n < n) return false;
  output_bitmap.assign(bytes.begin() + sizeof n, bytes.begin() + sizeof n + n);
  return true;
}

}  // namespace raytracer
