// host_capi.cc — a thin extern "C" shim over the C++ facade so that Python
// (ctypes) can drive it: tests, bench.py and __graft_entry__.py.  It adds no
// behaviour of its own; every call forwards to the raytracer:: classes.
#include <cstdint>
#include <cstdio>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "flatten.h"
#include "mythtracer.h"
#include "mythtracer_hip.h"
#include "primitive_triangle.h"

using raytracer::Camera;
using raytracer::Light;
using raytracer::Material;
using raytracer::MythTracer;
using raytracer::PerPixelDebugInfo;
using raytracer::Texture;
using raytracer::Triangle;
using raytracer::WorkChunk;
using math3d::V3D;

namespace {

struct Handle {
  MythTracer mt;
  std::vector<Material*> mtl_by_index;   // programmatic materials
  std::vector<Texture*> tex_by_index;
  std::string error;
  std::string shim_error;  // a refusal of a shim function itself (the facade was not asked, or succeeded)
};

Camera MakeCamera(const double* c) { return Camera{{c[0], c[1], c[2]}, c[3], c[4], c[5], c[6]}; }

}  // namespace

extern "C" {

void* mth_new(int device, int quiet) {
  Handle* h = new Handle;
  h->mt.SetDevice(device);
  h->mt.SetQuiet(quiet != 0);
  return h;
}

void mth_free(void* p) { delete static_cast<Handle*>(p); }

void mth_set_devices(void* p, const int* devices, int n) {
  static_cast<Handle*>(p)->mt.SetDevices(std::vector<int>(devices, devices + n));
}

const char* mth_last_error(void* p) {
  Handle* h = static_cast<Handle*>(p);
  h->error = h->shim_error.empty() ? h->mt.LastError() : h->shim_error;
  h->shim_error.clear();
  return h->error.c_str();
}

int mth_load_obj(void* p, const char* path) { return static_cast<Handle*>(p)->mt.LoadObj(path) ? 1 : 0; }

int mth_add_material(void* p, const char* name, const double* ka, const double* kd, const double* ks,
                     double ns, double refl, double tr, const double* tf, double ni) {
  Handle* h = static_cast<Handle*>(p);
  std::unique_ptr<Material> m(new Material);
  m->ambient = {ka[0], ka[1], ka[2]};
  m->diffuse = {kd[0], kd[1], kd[2]};
  m->specular = {ks[0], ks[1], ks[2]};
  m->transmission_filter = {tf[0], tf[1], tf[2]};
  m->specular_exp = ns;
  m->reflectance = refl;
  m->transparency = tr;
  m->refraction_index = ni;
  h->mtl_by_index.push_back(m.get());
  h->mt.GetScene()->materials[name] = std::move(m);
  return (int)h->mtl_by_index.size() - 1;
}

int mth_add_texture(void* p, const char* name, int w, int hgt, const double* rgb) {
  Handle* h = static_cast<Handle*>(p);
  std::unique_ptr<Texture> t(new Texture);
  t->width = (size_t)w;
  t->height = (size_t)hgt;
  t->colors.resize((size_t)w * hgt);
  for (size_t i = 0; i < t->colors.size(); i++) t->colors[i] = {rgb[i * 3], rgb[i * 3 + 1], rgb[i * 3 + 2]};
  h->tex_by_index.push_back(t.get());
  h->mt.GetScene()->textures[name] = std::move(t);
  return (int)h->tex_by_index.size() - 1;
}

int mth_material_set_texture(void* p, int mtl, int tex) {
  Handle* h = static_cast<Handle*>(p);
  if (mtl < 0 || (size_t)mtl >= h->mtl_by_index.size() || tex < -1 || tex >= (int)h->tex_by_index.size()) return 0;
  h->mtl_by_index[(size_t)mtl]->tex = tex < 0 ? nullptr : h->tex_by_index[(size_t)tex];
  return 1;
}

int mth_add_triangle(void* p, const double* v, const double* n, const double* uvw, int mtl, int line_no) {
  Handle* h = static_cast<Handle*>(p);
  Triangle* t = new Triangle();
  for (int k = 0; k < 3; k++) {
    t->vertex[k] = {v[k * 3], v[k * 3 + 1], v[k * 3 + 2]};
    if (n) t->normal[k] = {n[k * 3], n[k * 3 + 1], n[k * 3 + 2]};
    if (uvw) t->uvw[k] = {uvw[k * 3], uvw[k * 3 + 1], uvw[k * 3 + 2]};
  }
  t->mtl = (mtl >= 0 && (size_t)mtl < h->mtl_by_index.size()) ? h->mtl_by_index[(size_t)mtl] : nullptr;
  t->debug_line_no = line_no;
  t->CacheAABB();
  h->mt.GetScene()->tree.AddPrimitive(t);
  return (int)h->mt.GetScene()->tree.PrimitiveCount() - 1;
}

void mth_set_lights(void* p, const double* l, int n) {
  auto& lights = static_cast<Handle*>(p)->mt.GetScene()->lights;
  lights.clear();
  for (int i = 0; i < n; i++) {
    const double* q = l + 12 * i;
    lights.push_back(Light{{q[0], q[1], q[2]}, {q[3], q[4], q[5]}, {q[6], q[7], q[8]}, {q[9], q[10], q[11]}});
  }
}

void mth_set_max_level(void* p, int level) { static_cast<Handle*>(p)->mt.SetMaxRecursionLevel(level); }
void mth_set_supersampling(void* p, int s) { static_cast<Handle*>(p)->mt.SetSupersampling(s); }
void mth_set_adaptive_supersampling(void* p, int s, int threshold) {
  static_cast<Handle*>(p)->mt.SetAdaptiveSupersampling(s, threshold);
}

// host-only: builds the octree (no GPU needed)
void mth_finalize(void* p) { static_cast<Handle*>(p)->mt.GetScene()->tree.Finalize(); }

// finalize + upload to the GPU
int mth_prepare(void* p) { return static_cast<Handle*>(p)->mt.Prepare() ? 1 : 0; }

void* mth_device_scene(void* p) { return static_cast<Handle*>(p)->mt.DeviceScene(); }

void mth_root_aabb(void* p, double* out6) {
  const raytracer::AABB b = static_cast<Handle*>(p)->mt.GetScene()->tree.GetAABB();
  memcpy(out6, b.min.v, 24);
  memcpy(out6 + 3, b.max.v, 24);
}

void mth_tree_info(void* p, int* n_nodes, int* n_tris, int* depth) {
  const auto& tree = static_cast<Handle*>(p)->mt.GetScene()->tree;
  *n_nodes = (int)tree.Flat().NodeCount();
  *n_tris = (int)tree.PrimitiveCount();
  *depth = tree.Flat().depth;
}

// 0, with a message and nothing written, while the flat tree describes another triangle set than the scene holds
// (MythTracer::AddTriangle / RemoveTriangles before UpdateTrianglesInPlace): the arrays were sized by mth_tree_info
int mth_tree_dump(void* p, double* aabb, double* center, int32_t* first_child, int32_t* prim_begin,
                  int32_t* prim_count, int32_t* prim_ids) {
  Handle* h = static_cast<Handle*>(p);
  if (h->mt.GetScene()->tree.FlatIsStale()) {
    h->shim_error = "triangles were added or removed and the tree still describes the old ones: "
                    "UpdateTrianglesInPlace() first";
    return 0;
  }
  const raytracer::FlatTree& f = h->mt.GetScene()->tree.Flat();
  memcpy(aabb, f.node_aabb.data(), f.node_aabb.size() * 8);
  memcpy(center, f.node_center.data(), f.node_center.size() * 8);
  memcpy(first_child, f.first_child.data(), f.first_child.size() * 4);
  memcpy(prim_begin, f.prim_begin.data(), f.prim_begin.size() * 4);
  memcpy(prim_count, f.prim_count.data(), f.prim_count.size() * 4);
  memcpy(prim_ids, f.tri_id.data(), f.tri_id.size() * 4);
  return 1;
}

// vertex(9) normal(9) uvw(9) aabb(6) per triangle in AddPrimitive order;
// mtl_name_hash is not exported: material identity is checked through renders.
void mth_triangles(void* p, double* out33, int32_t* line_no, int32_t* has_mtl) {
  const auto& tree = static_cast<Handle*>(p)->mt.GetScene()->tree;
  for (size_t i = 0; i < tree.PrimitiveCount(); i++) {
    const Triangle* t = tree.GetTriangle(i);
    double* o = out33 + i * 33;
    memcpy(o, t->vertex, 72);
    memcpy(o + 9, t->normal, 72);
    memcpy(o + 18, t->uvw, 72);
    memcpy(o + 27, t->cached_aabb.min.v, 24);
    memcpy(o + 30, t->cached_aabb.max.v, 24);
    line_no[i] = t->debug_line_no;
    has_mtl[i] = t->mtl != nullptr;
  }
}

// The flattened scene exactly as MythTracer::Prepare hands it to
// mt_scene_create, for tests that call the C ABI directly.  Two-step protocol:
// call with NULL outputs to get the counts, then with buffers.
int mth_flatten(void* p, int* n_tris, int* n_materials, int* n_textures, double* vertex,
                double* normal, double* uvw, double* aabb, int32_t* material, int32_t* line_no,
                double* mats17 /* 16 values + tex index per material */,
                int32_t* tex_whf /* width,height,format per texture */) {
  Handle* h = static_cast<Handle*>(p);
  auto* scene = h->mt.GetScene();
  if (!scene->tree.IsFinalized()) scene->tree.Finalize();
  raytracer::FlatScene f;
  if (!f.Build(*scene)) {
    h->error = f.error;
    h->shim_error = f.error;  // (mth_last_error reports the shim's own refusals through it)
    return 0;
  }
  *n_tris = (int)f.material.size();
  *n_materials = (int)f.materials.size();
  *n_textures = (int)f.textures.size();
  if (vertex == nullptr) return 1;
  memcpy(vertex, f.vertex.data(), f.vertex.size() * 8);
  memcpy(normal, f.normal.data(), f.normal.size() * 8);
  memcpy(uvw, f.uvw.data(), f.uvw.size() * 8);
  memcpy(aabb, f.aabb.data(), f.aabb.size() * 8);
  memcpy(material, f.material.data(), f.material.size() * 4);
  memcpy(line_no, f.line_no.data(), f.line_no.size() * 4);
  for (size_t i = 0; i < f.materials.size(); i++) {
    const mt_material& m = f.materials[i];
    double* o = mats17 + i * 17;
    memcpy(o, m.ambient, 24);
    memcpy(o + 3, m.diffuse, 24);
    memcpy(o + 6, m.specular, 24);
    o[9] = m.specular_exp;
    o[10] = m.reflectance;
    o[11] = m.transparency;
    memcpy(o + 12, m.transmission_filter, 24);
    o[15] = m.refraction_index;
    o[16] = (double)m.tex;
  }
  for (size_t i = 0; i < f.textures.size(); i++) {
    tex_whf[i * 3] = f.textures[i].width;
    tex_whf[i * 3 + 1] = f.textures[i].height;
    tex_whf[i * 3 + 2] = f.textures[i].format;
  }
  return 1;
}

// texels of texture i of the flattened scene: RGB8 bytes or doubles
int mth_flatten_texels(void* p, int i, void* out) {
  Handle* h = static_cast<Handle*>(p);
  raytracer::FlatScene f;
  if (!f.Build(*h->mt.GetScene()) || i < 0 || (size_t)i >= f.textures.size()) return 0;
  const mt_texture& t = f.textures[(size_t)i];
  memcpy(out, t.texels, (size_t)t.width * t.height * (t.format == MT_TEX_RGB8 ? 3 : 24));
  return 1;
}

int mth_num_materials(void* p) { return (int)static_cast<Handle*>(p)->mt.GetScene()->materials.size(); }

// ka kd ks ns refl tr tf ni (16 doubles) of the named material; 0 if absent
int mth_get_material(void* p, const char* name, double* out16, int* has_tex) {
  auto& mats = static_cast<Handle*>(p)->mt.GetScene()->materials;
  auto it = mats.find(name);
  if (it == mats.end()) return 0;
  const Material& m = *it->second;
  memcpy(out16, m.ambient.v, 24);
  memcpy(out16 + 3, m.diffuse.v, 24);
  memcpy(out16 + 6, m.specular.v, 24);
  out16[9] = m.specular_exp;
  out16[10] = m.reflectance;
  out16[11] = m.transparency;
  memcpy(out16 + 12, m.transmission_filter.v, 24);
  out16[15] = m.refraction_index;
  *has_tex = m.tex != nullptr;
  return 1;
}

void mth_sensor(const double* cam7, int w, int hgt, double* out12) {
  const Camera cam = MakeCamera(cam7);
  const Camera::Sensor s = cam.GetSensor(w, hgt);
  memcpy(out12, cam.origin.v, 24);
  memcpy(out12 + 3, s.StartPoint().v, 24);
  memcpy(out12 + 6, s.DeltaScanline().v, 24);
  memcpy(out12 + 9, s.DeltaPixel().v, 24);
}

void mth_sensor_ray(const double* cam7, int w, int hgt, int x, int y, double* dir3) {
  const Camera cam = MakeCamera(cam7);
  const raytracer::Ray r = cam.GetSensor(w, hgt).GetRay(x, y);
  memcpy(dir3, r.direction.v, 24);
}

// MythTracer::RayTrace(WorkChunk*).  stats10: rays p/s/sh, box, node, tri, mt,
// shaded, then kernel_ms and total_ms as doubles in ms2.
int mth_render_chunk(void* p, const double* cam7, int iw, int ih, int cx, int cy, int cw, int ch,
                     uint8_t* rgb, int32_t* dbg_line, double* dbg_point, uint64_t* stats8, double* ms2) {
  Handle* h = static_cast<Handle*>(p);
  WorkChunk chunk{iw, ih, cx, cy, cw, ch, MakeCamera(cam7), {}, {}};
  const size_t npx = (size_t)(cw > 0 ? cw : 0) * (size_t)(ch > 0 ? ch : 0);
  chunk.output_bitmap.resize(npx * 3);
  if (dbg_line) chunk.output_debug.resize(npx);
  if (!h->mt.RayTrace(&chunk)) return 0;
  memcpy(rgb, chunk.output_bitmap.data(), npx * 3);
  for (size_t i = 0; dbg_line && i < npx; i++) {
    dbg_line[i] = chunk.output_debug[i].line_no;
    if (dbg_point) memcpy(dbg_point + i * 3, chunk.output_debug[i].point.v, 24);
  }
  const raytracer::RenderStats& s = h->mt.LastStats();
  if (stats8) {
    const uint64_t v[8] = {s.rays_primary, s.rays_secondary, s.rays_shadow, s.box_tests,
                           s.node_visits,  s.tri_tests,      s.mt_tests,    s.shaded_hits};
    memcpy(stats8, v, sizeof v);
  }
  if (ms2) {
    ms2[0] = s.kernel_ms;
    ms2[1] = s.total_ms;
  }
  return 1;
}

// MythTracer::RayTraceGBuffer(WorkChunk*, GBuffer*).  channels = GBuffer::k* bits; planes[8] = depth, point, normal,
// uvw, albedo (doubles), prim, line_no, material (int32), each NULL or sized for the chunk.
int mth_render_gbuffer(void* p, const double* cam7, int iw, int ih, int cx, int cy, int cw, int ch, unsigned channels,
                       void* const* planes, uint64_t* stats8, double* ms2) {
  Handle* h = static_cast<Handle*>(p);
  WorkChunk chunk{iw, ih, cx, cy, cw, ch, MakeCamera(cam7), {}, {}};
  raytracer::GBuffer g;
  g.channels = channels;
  if (!h->mt.RayTraceGBuffer(&chunk, &g)) return 0;
  const std::vector<double>* f[5] = {&g.depth, &g.point, &g.normal, &g.uvw, &g.albedo};
  const std::vector<int32_t>* i32[3] = {&g.prim, &g.line_no, &g.material};
  for (int k = 0; k < 5; k++) {
    if (planes[k] && !f[k]->empty()) memcpy(planes[k], f[k]->data(), f[k]->size() * 8);
  }
  for (int k = 0; k < 3; k++) {
    if (planes[5 + k] && !i32[k]->empty()) memcpy(planes[5 + k], i32[k]->data(), i32[k]->size() * 4);
  }
  const raytracer::RenderStats& s = h->mt.LastStats();
  if (stats8) {
    const uint64_t v[8] = {s.rays_primary, s.rays_secondary, s.rays_shadow, s.box_tests,
                           s.node_visits,  s.tri_tests,      s.mt_tests,    s.shaded_hits};
    memcpy(stats8, v, sizeof v);
  }
  if (ms2) {
    ms2[0] = s.kernel_ms;
    ms2[1] = s.total_ms;
  }
  return 1;
}

int mth_num_lights(void* p) { return (int)static_cast<Handle*>(p)->mt.GetScene()->lights.size(); }

// MythTracer::RayTraceLightBuffer(WorkChunk*, GBuffer*, LightBuffer*).  gb_channels / gb_planes[8] as in
// mth_render_gbuffer (0 = no GBuffer); lb_channels = LightBuffer::k* bits, lb_planes[2] = power (doubles), in_shadow
// (bytes), each NULL or sized for n_lights x the chunk; n_lights = what the caller sized them for.
int mth_render_lightbuffer(void* p, const double* cam7, int iw, int ih, int cx, int cy, int cw, int ch,
                           unsigned gb_channels, void* const* gb_planes, unsigned lb_channels, void* const* lb_planes,
                           int n_lights, uint64_t* stats8, double* ms2) {
  Handle* h = static_cast<Handle*>(p);
  WorkChunk chunk{iw, ih, cx, cy, cw, ch, MakeCamera(cam7), {}, {}};
  raytracer::GBuffer g;
  g.channels = gb_channels;
  raytracer::LightBuffer lb;
  lb.channels = lb_channels;
  if ((int)h->mt.GetScene()->lights.size() != n_lights) {  // (checked first: nothing may be copied into planes of another size)
    h->shim_error = "the planes were sized for " + std::to_string(n_lights) + " lights, the scene has " +
                    std::to_string(h->mt.GetScene()->lights.size());
    return 0;
  }
  if (!h->mt.RayTraceLightBuffer(&chunk, gb_channels ? &g : nullptr, &lb)) return 0;
  const std::vector<double>* f[5] = {&g.depth, &g.point, &g.normal, &g.uvw, &g.albedo};
  const std::vector<int32_t>* i32[3] = {&g.prim, &g.line_no, &g.material};
  for (int k = 0; k < 5; k++) {
    if (gb_planes[k] && !f[k]->empty()) memcpy(gb_planes[k], f[k]->data(), f[k]->size() * 8);
  }
  for (int k = 0; k < 3; k++) {
    if (gb_planes[5 + k] && !i32[k]->empty()) memcpy(gb_planes[5 + k], i32[k]->data(), i32[k]->size() * 4);
  }
  if (lb_planes[0] && !lb.power.empty()) memcpy(lb_planes[0], lb.power.data(), lb.power.size() * 8);
  if (lb_planes[1] && !lb.in_shadow.empty()) memcpy(lb_planes[1], lb.in_shadow.data(), lb.in_shadow.size());
  const raytracer::RenderStats& s = h->mt.LastStats();
  if (stats8) {
    const uint64_t v[8] = {s.rays_primary, s.rays_secondary, s.rays_shadow, s.box_tests,
                           s.node_visits,  s.tri_tests,      s.mt_tests,    s.shaded_hits};
    memcpy(stats8, v, sizeof v);
  }
  if (ms2) {
    ms2[0] = s.kernel_ms;
    ms2[1] = s.total_ms;
  }
  return 1;
}

// MythTracer::ShadeDirect(WorkChunk*, GBuffer, LightBuffer) under the facade's lights.  gb_planes[4] = point, normal,
// albedo (doubles), material (int32) of the chunk; lb_planes[2] = power, in_shadow for n_lights lights.
int mth_shade_direct(void* p, const double* cam7, int iw, int ih, int cx, int cy, int cw, int ch,
                     void* const* gb_planes, int n_lights, void* const* lb_planes, uint8_t* rgb, double* ms2) {
  Handle* h = static_cast<Handle*>(p);
  WorkChunk chunk{iw, ih, cx, cy, cw, ch, MakeCamera(cam7), {}, {}};
  const size_t npx = (size_t)(cw > 0 ? cw : 0) * (size_t)(ch > 0 ? ch : 0);
  const size_t n_l = (size_t)(n_lights > 0 ? n_lights : 0);
  raytracer::GBuffer g;
  g.width = cw;
  g.height = ch;
  const double* f[3] = {(const double*)gb_planes[0], (const double*)gb_planes[1], (const double*)gb_planes[2]};
  g.point.assign(f[0], f[0] + npx * 3);
  g.normal.assign(f[1], f[1] + npx * 3);
  g.albedo.assign(f[2], f[2] + npx * 3);
  g.material.assign((const int32_t*)gb_planes[3], (const int32_t*)gb_planes[3] + npx);
  raytracer::LightBuffer lb;
  lb.width = cw;
  lb.height = ch;
  lb.n_lights = n_lights;
  lb.power.assign((const double*)lb_planes[0], (const double*)lb_planes[0] + n_l * npx * 3);
  lb.in_shadow.assign((const uint8_t*)lb_planes[1], (const uint8_t*)lb_planes[1] + n_l * npx);
  if (!h->mt.ShadeDirect(&chunk, g, lb)) return 0;
  memcpy(rgb, chunk.output_bitmap.data(), npx * 3);
  if (ms2) {
    ms2[0] = h->mt.LastStats().kernel_ms;
    ms2[1] = h->mt.LastStats().total_ms;
  }
  return 1;
}

// MythTracer::BuildRayTree(WorkChunk*, RayTree*) at the facade's recursion level and lights: a new RayTree on the heap
// (mth_raytree_free), NULL on failure.
void* mth_raytree_build(void* p, const double* cam7, int iw, int ih, int cx, int cy, int cw, int ch, uint64_t* stats8,
                        double* ms2) {
  Handle* h = static_cast<Handle*>(p);
  WorkChunk chunk{iw, ih, cx, cy, cw, ch, MakeCamera(cam7), {}, {}};
  raytracer::RayTree* t = new raytracer::RayTree();
  if (!h->mt.BuildRayTree(&chunk, t)) {
    delete t;
    return nullptr;
  }
  const raytracer::RenderStats& s = h->mt.LastStats();
  if (stats8) {
    const uint64_t v[8] = {s.rays_primary, s.rays_secondary, s.rays_shadow, s.box_tests,
                           s.node_visits,  s.tri_tests,      s.mt_tests,    s.shaded_hits};
    memcpy(stats8, v, sizeof v);
  }
  if (ms2) {
    ms2[0] = s.kernel_ms;
    ms2[1] = s.total_ms;
  }
  return t;
}

void mth_raytree_free(void* t) { delete static_cast<raytracer::RayTree*>(t); }

// the mt_raytree behind a RayTree (for mt_raytree_info / mt_raytree_read_layer)
void* mth_raytree_handle(void* t) { return t ? static_cast<raytracer::RayTree*>(t)->Get() : nullptr; }

// MythTracer::ShadeRayTree(tree, &bitmap) under the facade's current lights; rgb holds rgb_bytes bytes.
int mth_raytree_shade(void* p, void* t, uint8_t* rgb, size_t rgb_bytes, double* ms2) {
  Handle* h = static_cast<Handle*>(p);
  if (t == nullptr) {
    h->shim_error = "the RayTree is NULL";
    return 0;
  }
  std::vector<uint8_t> bitmap;
  if (!h->mt.ShadeRayTree(*static_cast<raytracer::RayTree*>(t), &bitmap)) return 0;
  if (bitmap.size() != rgb_bytes) {
    h->shim_error = "the bitmap was sized for " + std::to_string(rgb_bytes) + " bytes, the tree's chunk has " +
                    std::to_string(bitmap.size());
    return 0;
  }
  memcpy(rgb, bitmap.data(), bitmap.size());
  if (ms2) {
    ms2[0] = h->mt.LastStats().kernel_ms;
    ms2[1] = h->mt.LastStats().total_ms;
  }
  return 1;
}

namespace {
// n rays of 6 doubles as the facade's vector (empty for NULL or n <= 0)
std::vector<raytracer::Ray> RaysOf(const double* rays6, long long n) {
  std::vector<raytracer::Ray> rays;
  for (long long i = 0; rays6 != nullptr && i < n; i++) {
    const double* r = rays6 + i * 6;
    rays.emplace_back(V3D{r[0], r[1], r[2]}, V3D{r[3], r[4], r[5]});
  }
  return rays;
}

void StatsOut(const raytracer::RenderStats& s, uint64_t* stats8, double* ms2) {
  if (stats8) {
    const uint64_t v[8] = {s.rays_primary, s.rays_secondary, s.rays_shadow, s.box_tests,
                           s.node_visits,  s.tri_tests,      s.mt_tests,    s.shaded_hits};
    memcpy(stats8, v, sizeof v);
  }
  if (ms2) {
    ms2[0] = s.kernel_ms;
    ms2[1] = s.total_ms;
  }
}
}  // namespace

// MythTracer::BuildRayTree(rays, list_width, RayTree*) at the facade's recursion level and lights; rays6 = n x 6
// doubles.  A new RayTree on the heap (mth_raytree_free), NULL on failure.
void* mth_raytree_build_rays(void* p, const double* rays6, long long n, int list_width, uint64_t* stats8, double* ms2) {
  Handle* h = static_cast<Handle*>(p);
  raytracer::RayTree* t = new raytracer::RayTree();
  if (!h->mt.BuildRayTree(RaysOf(rays6, n), list_width, t)) {
    delete t;
    return nullptr;
  }
  StatsOut(h->mt.LastStats(), stats8, ms2);
  return t;
}

// MythTracer::ShadeRayTree(tree, &colours) under the facade's current lights; colors holds n_colors x 3 doubles.
int mth_raytree_shade_colors(void* p, void* t, double* colors, size_t n_colors, double* ms2) {
  Handle* h = static_cast<Handle*>(p);
  if (t == nullptr) {
    h->shim_error = "the RayTree is NULL";
    return 0;
  }
  std::vector<V3D> colours;
  if (!h->mt.ShadeRayTree(*static_cast<raytracer::RayTree*>(t), &colours)) return 0;
  if (colours.size() != n_colors) {
    h->shim_error = "the colours were sized for " + std::to_string(n_colors) + " rays, the tree's layer 0 has " +
                    std::to_string(colours.size());
    return 0;
  }
  memcpy(colors, colours.data(), colours.size() * sizeof(V3D));
  StatsOut(h->mt.LastStats(), nullptr, ms2);
  return 1;
}

// MythTracer::TraceRays(rays, list_width, colours, bitmap): colors (n x 3 doubles) and rgb (n x 3 bytes), either may
// be NULL.
int mth_trace_rays(void* p, const double* rays6, long long n, int list_width, double* colors, uint8_t* rgb,
                   uint64_t* stats8, double* ms2) {
  Handle* h = static_cast<Handle*>(p);
  std::vector<V3D> colours;
  std::vector<uint8_t> bitmap;
  if (!h->mt.TraceRays(RaysOf(rays6, n), list_width, colors ? &colours : nullptr, rgb ? &bitmap : nullptr)) return 0;
  if (colors) memcpy(colors, colours.data(), colours.size() * sizeof(V3D));
  if (rgb) memcpy(rgb, bitmap.data(), bitmap.size());
  StatsOut(h->mt.LastStats(), stats8, ms2);
  return 1;
}

// MythTracer::UpdateRayTree(lights, tree) under the facade's lights; `t` as mth_raytree_build returned it (NULL is
// refused by the facade, after the checks that need no tree).
int mth_raytree_update(void* p, void* t, const int* light_idx, int n_idx, uint64_t* stats8, double* ms2) {
  Handle* h = static_cast<Handle*>(p);
  const std::vector<int> lights(light_idx, light_idx + (light_idx && n_idx > 0 ? n_idx : 0));
  if (!h->mt.UpdateRayTree(lights, static_cast<raytracer::RayTree*>(t))) return 0;
  const raytracer::RenderStats& s = h->mt.LastStats();
  if (stats8) {
    const uint64_t v[8] = {s.rays_primary, s.rays_secondary, s.rays_shadow, s.box_tests,
                           s.node_visits,  s.tri_tests,      s.mt_tests,    s.shaded_hits};
    memcpy(stats8, v, sizeof v);
  }
  if (ms2) {
    ms2[0] = s.kernel_ms;
    ms2[1] = s.total_ms;
  }
  return 1;
}

// MythTracer::UpdateMaterials after an edit of one material by name: values16 = ka kd ks ns refl tr tf ni (mth_get_material's
// order), NULL = no edit, only the update.  0 with the facade's message when it refuses; an unknown name is the shim's.
int mth_update_materials(void* p, const char* name, const double* values16) {
  Handle* h = static_cast<Handle*>(p);
  if (name != nullptr && values16 != nullptr) {
    auto& mats = h->mt.GetScene()->materials;
    auto it = mats.find(name);
    if (it == mats.end()) {
      h->shim_error = std::string("no material named ") + name;
      return 0;
    }
    Material& m = *it->second;
    const double* v = values16;
    m.ambient = {v[0], v[1], v[2]};
    m.diffuse = {v[3], v[4], v[5]};
    m.specular = {v[6], v[7], v[8]};
    m.specular_exp = v[9];
    m.reflectance = v[10];
    m.transparency = v[11];
    m.transmission_filter = {v[12], v[13], v[14]};
    m.refraction_index = v[15];
  }
  return h->mt.UpdateMaterials() ? 1 : 0;
}

// MythTracer::UpdateTexture after an edit of one texture by its key: w x hgt colours in rgb (NULL = no edit, only the
// update).  The Texture object is edited in place, so the materials that point at it keep doing so.  0 with the facade's
// message when it refuses; an unknown key is the shim's.
int mth_update_texture(void* p, const char* name, int w, int hgt, const double* rgb) {
  Handle* h = static_cast<Handle*>(p);
  if (name == nullptr) {
    h->shim_error = "the texture key is NULL";
    return 0;
  }
  if (rgb != nullptr) {
    auto& texs = h->mt.GetScene()->textures;
    auto it = texs.find(name);
    if (it == texs.end()) {
      h->shim_error = std::string("no texture named ") + name;
      return 0;
    }
    if (w < 1 || hgt < 1) {
      h->shim_error = "texture size out of range";
      return 0;
    }
    Texture& t = *it->second;
    t.width = (size_t)w;
    t.height = (size_t)hgt;
    t.colors.resize((size_t)w * hgt);
    for (size_t i = 0; i < t.colors.size(); i++) t.colors[i] = {rgb[i * 3], rgb[i * 3 + 1], rgb[i * 3 + 2]};
  }
  return h->mt.UpdateTexture(name) ? 1 : 0;
}

// MythTracer::SetRayTreeKeepUVW
void mth_set_raytree_keep_uvw(void* p, int keep) { static_cast<Handle*>(p)->mt.SetRayTreeKeepUVW(keep != 0); }

// Triangle::mtl of the listed triangles (AddPrimitive indices) pointed at the material `name` (NULL = none), through
// OctTree::MutableTriangle; nothing is uploaded (mth_update_triangle_materials does that).  0 with the shim's message for
// an unknown name or an index outside the scene's triangles: no triangle is changed then.
int mth_assign_material(void* p, const int32_t* add_indices, int n, const char* name) {
  Handle* h = static_cast<Handle*>(p);
  auto* scene = h->mt.GetScene();
  Material* m = nullptr;
  if (name != nullptr) {
    auto it = scene->materials.find(name);
    if (it == scene->materials.end()) {
      h->shim_error = std::string("no material named ") + name;
      return 0;
    }
    m = it->second.get();
  }
  if (n < 0 || (n > 0 && add_indices == nullptr)) {
    h->shim_error = "bad triangle index list";
    return 0;
  }
  for (int i = 0; i < n; i++) {
    if (add_indices[i] < 0 || (size_t)add_indices[i] >= scene->tree.PrimitiveCount()) {
      h->shim_error = "triangle index " + std::to_string(add_indices[i]) + " outside the scene's " +
                      std::to_string(scene->tree.PrimitiveCount()) + " triangles";
      return 0;
    }
  }
  for (int i = 0; i < n; i++) scene->tree.MutableTriangle((size_t)add_indices[i])->mtl = m;
  return 1;
}

// MythTracer::UpdateTriangleMaterials; 0 with the facade's message when it refuses
int mth_update_triangle_materials(void* p) { return static_cast<Handle*>(p)->mt.UpdateTriangleMaterials() ? 1 : 0; }

// Triangle::normal (which = 0) or Triangle::uvw (1) of the listed triangles (AddPrimitive indices) replaced by
// attr[n][9], through OctTree::MutableTriangle; nothing is uploaded (mth_update_triangle_attributes does that).  0 with
// the shim's message for a bad list or an index outside the scene's triangles: no triangle is changed then.
int mth_set_triangle_attr(void* p, int which, const int32_t* add_indices, int n, const double* attr) {
  Handle* h = static_cast<Handle*>(p);
  auto* scene = h->mt.GetScene();
  if ((which != 0 && which != 1) || n < 0 || (n > 0 && (add_indices == nullptr || attr == nullptr))) {
    h->shim_error = "bad triangle attribute list";
    return 0;
  }
  for (int i = 0; i < n; i++) {
    if (add_indices[i] < 0 || (size_t)add_indices[i] >= scene->tree.PrimitiveCount()) {
      h->shim_error = "triangle index " + std::to_string(add_indices[i]) + " outside the scene's " +
                      std::to_string(scene->tree.PrimitiveCount()) + " triangles";
      return 0;
    }
  }
  for (int i = 0; i < n; i++) {
    auto* t = scene->tree.MutableTriangle((size_t)add_indices[i]);
    memcpy(which == 0 ? (void*)t->normal : (void*)t->uvw, attr + (size_t)i * 9, 72);
  }
  return 1;
}

// MythTracer::UpdateTriangleAttributes; 0 with the facade's message when it refuses
int mth_update_triangle_attributes(void* p) { return static_cast<Handle*>(p)->mt.UpdateTriangleAttributes() ? 1 : 0; }

// MythTracer::SetDeviceTreeBuild
void mth_set_device_tree_build(void* p, int on) { static_cast<Handle*>(p)->mt.SetDeviceTreeBuild(on != 0); }

// MythTracer::SetTriangleVertices: vertices[n][9] for the triangles add_indices[n]; 0 with the facade's message (or the
// shim's for a bad list) when it refuses: no triangle is changed then
int mth_set_triangle_vertices(void* p, const int32_t* add_indices, int n, const double* vertices) {
  Handle* h = static_cast<Handle*>(p);
  if (n < 0 || (n > 0 && (add_indices == nullptr || vertices == nullptr))) {
    h->shim_error = "bad triangle vertex list";
    return 0;
  }
  std::vector<int> idx(add_indices, add_indices + n);
  std::vector<raytracer::V3D> v((size_t)n * 3);
  for (size_t k = 0; k < v.size(); k++) v[k] = {vertices[k * 3], vertices[k * 3 + 1], vertices[k * 3 + 2]};
  h->shim_error.clear();
  return h->mt.SetTriangleVertices(idx, v) ? 1 : 0;
}

// MythTracer::UpdateGeometry
void mth_update_geometry(void* p) { static_cast<Handle*>(p)->mt.UpdateGeometry(); }

// MythTracer::UpdateGeometryInPlace; 0 with the facade's message when a device refuses
int mth_update_geometry_in_place(void* p) { return static_cast<Handle*>(p)->mt.UpdateGeometryInPlace() ? 1 : 0; }

// MythTracer::AddTriangle for n triangles: vertices (n x 9), normals and uvw (n x 9, or NULL for the Triangle's defaults),
// all with the scene's material `material` (NULL: none), line numbers (n, or NULL for 0).  0 with a message, and no
// triangle added, for an unknown material name or a bad list.
int mth_add_triangles(void* p, int n, const double* v, const double* nrm, const double* uvw, const char* material,
                      const int32_t* line_no) {
  Handle* h = static_cast<Handle*>(p);
  auto* scene = h->mt.GetScene();
  Material* m = nullptr;
  if (material != nullptr) {
    auto it = scene->materials.find(material);
    if (it == scene->materials.end()) {
      h->shim_error = std::string("no material named ") + material;
      return 0;
    }
    m = it->second.get();
  }
  if (n < 0 || (n > 0 && v == nullptr)) {
    h->shim_error = "bad triangle list";
    return 0;
  }
  h->shim_error.clear();
  for (int i = 0; i < n; i++) {
    Triangle* t = new Triangle();
    for (int k = 0; k < 3; k++) {
      const size_t at = (size_t)i * 9 + (size_t)k * 3;
      t->vertex[k] = {v[at], v[at + 1], v[at + 2]};
      if (nrm) t->normal[k] = {nrm[at], nrm[at + 1], nrm[at + 2]};
      if (uvw) t->uvw[k] = {uvw[at], uvw[at + 1], uvw[at + 2]};
    }
    t->mtl = m;
    t->debug_line_no = line_no ? line_no[i] : 0;
    t->CacheAABB();
    if (!h->mt.AddTriangle(t)) return 0;
  }
  return 1;
}

// MythTracer::RemoveTriangles
int mth_remove_triangles(void* p, const int32_t* add_indices, int n) {
  Handle* h = static_cast<Handle*>(p);
  if (n < 0 || (n > 0 && add_indices == nullptr)) {
    h->shim_error = "bad triangle index list";
    return 0;
  }
  h->shim_error.clear();
  return h->mt.RemoveTriangles(std::vector<int>(add_indices, add_indices + n)) ? 1 : 0;
}

// MythTracer::UpdateTrianglesInPlace; 0 with the facade's message when it or a device refuses
int mth_update_triangles_in_place(void* p) { return static_cast<Handle*>(p)->mt.UpdateTrianglesInPlace() ? 1 : 0; }

// MythTracer::SetRayTreeKeepTriangles
void mth_set_raytree_keep_triangles(void* p, int keep) { static_cast<Handle*>(p)->mt.SetRayTreeKeepTriangles(keep != 0); }

// MythTracer::UpdateRayTreeMaterials; stats8 / ms2 as mth_raytree_update fills them
int mth_raytree_update_materials(void* p, void* t, uint64_t* stats8, double* ms2) {
  Handle* h = static_cast<Handle*>(p);
  if (!h->mt.UpdateRayTreeMaterials(static_cast<raytracer::RayTree*>(t))) return 0;
  const raytracer::RenderStats& s = h->mt.LastStats();
  if (stats8) {
    const uint64_t v[8] = {s.rays_primary, s.rays_secondary, s.rays_shadow, s.box_tests,
                           s.node_visits,  s.tri_tests,      s.mt_tests,    s.shaded_hits};
    memcpy(stats8, v, sizeof v);
  }
  if (ms2) {
    ms2[0] = s.kernel_ms;
    ms2[1] = s.total_ms;
  }
  return 1;
}

// MythTracer::RegrowRayTree; stats8 / ms2 as mth_raytree_update fills them
int mth_raytree_regrow(void* p, void* t, uint64_t* stats8, double* ms2) {
  Handle* h = static_cast<Handle*>(p);
  if (!h->mt.RegrowRayTree(static_cast<raytracer::RayTree*>(t))) return 0;
  const raytracer::RenderStats& s = h->mt.LastStats();
  if (stats8) {
    const uint64_t v[8] = {s.rays_primary, s.rays_secondary, s.rays_shadow, s.box_tests,
                           s.node_visits,  s.tri_tests,      s.mt_tests,    s.shaded_hits};
    memcpy(stats8, v, sizeof v);
  }
  if (ms2) {
    ms2[0] = s.kernel_ms;
    ms2[1] = s.total_ms;
  }
  return 1;
}

// MythTracer::UpdateLightBuffer(GBuffer, lights, LightBuffer*) under the facade's lights.  gb_planes[2] = point
// (doubles), material (int32) of the cw x ch chunk; lb_channels = LightBuffer::k* bits, lb_planes[2] = power, in_shadow
// for n_lights lights (each NULL or sized for them), updated in place: the planes of the listed lights only.
int mth_update_lightbuffer(void* p, int cw, int ch, void* const* gb_planes, const int* light_idx, int n_idx,
                           unsigned lb_channels, void* const* lb_planes, int n_lights, uint64_t* stats8, double* ms2) {
  Handle* h = static_cast<Handle*>(p);
  const size_t npx = (size_t)(cw > 0 ? cw : 0) * (size_t)(ch > 0 ? ch : 0);
  const size_t n_l = (size_t)(n_lights > 0 ? n_lights : 0);
  raytracer::GBuffer g;
  g.width = cw;
  g.height = ch;
  if (gb_planes && gb_planes[0] && gb_planes[1]) {  // (else the facade refuses: the planes are missing)
    g.point.assign((const double*)gb_planes[0], (const double*)gb_planes[0] + npx * 3);
    g.material.assign((const int32_t*)gb_planes[1], (const int32_t*)gb_planes[1] + npx);
  }
  raytracer::LightBuffer lb;
  lb.channels = lb_channels;
  lb.width = cw;
  lb.height = ch;
  lb.n_lights = n_lights;
  const bool power = (lb_channels & raytracer::LightBuffer::kPower) && lb_planes && lb_planes[0];
  const bool shadow = (lb_channels & raytracer::LightBuffer::kInShadow) && lb_planes && lb_planes[1];
  // The update reads nothing of the old planes and writes the listed ones only: the caller's planes are not copied
  // in, and only the listed planes are copied back (the list is valid once the call has succeeded).
  if (power) lb.power.resize(n_l * npx * 3);
  if (shadow) lb.in_shadow.resize(n_l * npx);
  const std::vector<int> lights(light_idx, light_idx + (light_idx && n_idx > 0 ? n_idx : 0));
  if (!h->mt.UpdateLightBuffer(g, lights, &lb)) return 0;
  for (int l : lights) {
    const size_t at = (size_t)l * npx;
    if (power) memcpy((double*)lb_planes[0] + at * 3, lb.power.data() + at * 3, npx * 3 * sizeof(double));
    if (shadow) memcpy((uint8_t*)lb_planes[1] + at, lb.in_shadow.data() + at, npx);
  }
  const raytracer::RenderStats& s = h->mt.LastStats();
  if (stats8) {
    const uint64_t v[8] = {s.rays_primary, s.rays_secondary, s.rays_shadow, s.box_tests,
                           s.node_visits,  s.tri_tests,      s.mt_tests,    s.shaded_hits};
    memcpy(stats8, v, sizeof v);
  }
  if (ms2) {
    ms2[0] = s.kernel_ms;
    ms2[1] = s.total_ms;
  }
  return 1;
}

// MythTracer::RayTrace(int, int, Camera*, vector*)
int mth_render_image(void* p, const double* cam7, int iw, int ih, uint8_t* rgb) {
  Handle* h = static_cast<Handle*>(p);
  Camera cam = MakeCamera(cam7);
  std::vector<uint8_t> bmp;
  if (!h->mt.RayTrace(iw, ih, &cam, &bmp)) return 0;
  memcpy(rgb, bmp.data(), bmp.size());
  return 1;
}

// The frame loop of main_local.cc:51-132 as a driver written against the facade runs it: per frame the lights are
// cleared and pushed again (:79-110), a Camera is aggregate-initialised with the frame's yaw (:72-76, `dyaw` degrees
// per frame, a triangular pan of +-4 steps around cam7's yaw that ends on it) and RayTrace(W, H, &cam, &bitmap)
// fills ONE vector that lives outside the loop (:122).  ms[i] = wall time of frame i's RayTrace call including the
// light upload and the copy of the frame into `bitmap` -- what the drop-in caller waits for; rgb = the last frame.
int mth_frame_loop(void* p, const double* cam7, int iw, int ih, int n_frames, double dyaw, int collect_stats,
                   double* ms, uint8_t* rgb) {
  Handle* h = static_cast<Handle*>(p);
  h->mt.SetCollectStats(collect_stats != 0);
  const std::vector<raytracer::Light> lights = h->mt.GetScene()->lights;
  std::vector<uint8_t> bitmap;
  for (int i = 0; i < n_frames; i++) {
    auto& L = h->mt.GetScene()->lights;
    L.clear();
    for (const raytracer::Light& l : lights) L.push_back(l);
    const int j = ((n_frames - 1 - i) % 16 + 16) % 16;
    const int tri = j <= 4 ? j : (j <= 12 ? 8 - j : j - 16);
    double c[7];
    memcpy(c, cam7, sizeof c);
    c[4] += dyaw * tri;
    Camera cam = MakeCamera(c);
    const auto t0 = std::chrono::steady_clock::now();
    if (!h->mt.RayTrace(iw, ih, &cam, &bitmap)) {
      h->mt.SetCollectStats(true);
      return 0;
    }
    ms[i] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  h->mt.SetCollectStats(true);
  if (rgb && !bitmap.empty()) memcpy(rgb, bitmap.data(), bitmap.size());
  return 1;
}

// OctTree::IntersectRays; prim = AddPrimitive index or -1
int mth_intersect(void* p, int n, const double* rays, int32_t* prim, int32_t* line, double* t, double* point) {
  Handle* h = static_cast<Handle*>(p);
  auto& tree = h->mt.GetScene()->tree;
  if (!tree.IsFinalized()) tree.Finalize();
  std::vector<const raytracer::Primitive*> hits((size_t)n);
  if (!tree.IntersectRays(n, rays, hits.data(), t, point)) {
    h->error = tree.LastError();
    return 0;
  }
  for (int i = 0; i < n; i++) {
    int idx = -1;
    if (hits[(size_t)i]) {
      for (size_t k = 0; k < tree.PrimitiveCount(); k++) {
        if (tree.GetTriangle(k) == hits[(size_t)i]) { idx = (int)k; break; }
      }
    }
    if (prim) prim[i] = idx;
    if (line) line[i] = hits[(size_t)i] ? hits[(size_t)i]->debug_line_no : -1;
  }
  return 1;
}

// --- wire formats (WorkChunk / Camera), for the serialisation tests
int mth_chunk_serialize_input(const int32_t* f6, uint8_t* out24) {
  WorkChunk c{f6[0], f6[1], f6[2], f6[3], f6[4], f6[5], Camera{}, {}, {}};
  std::vector<uint8_t> b;
  c.SerializeInput(&b);
  memcpy(out24, b.data(), b.size());
  return (int)b.size();
}

int mth_chunk_deserialize_input(const uint8_t* bytes, int n, int32_t* f6) {
  WorkChunk c{};
  if (!c.DeserializeInput(std::vector<uint8_t>(bytes, bytes + n))) return 0;
  const int32_t v[6] = {c.image_width, c.image_height, c.chunk_x, c.chunk_y, c.chunk_width, c.chunk_height};
  memcpy(f6, v, sizeof v);
  return 1;
}

int mth_chunk_output_roundtrip(int cw, int ch, const uint8_t* rgb, int n_rgb, uint8_t* packet,
                               int packet_cap, uint8_t* back) {
  WorkChunk c{};
  c.chunk_width = cw;
  c.chunk_height = ch;
  c.output_bitmap.assign(rgb, rgb + n_rgb);
  std::vector<uint8_t> b;
  if (!c.SerializeOutput(&b) || (int)b.size() > packet_cap) return -1;
  memcpy(packet, b.data(), b.size());
  WorkChunk d{};
  d.chunk_width = cw;
  d.chunk_height = ch;
  if (!d.DeserializeOutput(b)) return -2;
  memcpy(back, d.output_bitmap.data(), d.output_bitmap.size());
  return (int)b.size();
}

int mth_chunk_deserialize_output(int cw, int ch, const uint8_t* packet, int n) {
  WorkChunk d{};
  d.chunk_width = cw;
  d.chunk_height = ch;
  return d.DeserializeOutput(std::vector<uint8_t>(packet, packet + n)) ? 1 : 0;
}

int mth_camera_roundtrip(const double* cam7, uint8_t* out56, double* back7) {
  Camera cam = MakeCamera(cam7);
  std::vector<uint8_t> b;
  cam.Serialize(&b);
  memcpy(out56, b.data(), b.size());
  Camera c2{};
  if (!c2.Deserialize(b)) return 0;
  const double v[7] = {c2.origin.v[0], c2.origin.v[1], c2.origin.v[2], c2.pitch, c2.yaw, c2.roll, c2.aov};
  memcpy(back7, v, sizeof v);
  return (int)b.size();
}

}  // extern "C"
