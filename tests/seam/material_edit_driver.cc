// material_edit_driver — a C++ program against the facade's headers (mythtracer_amd/host/include) and
// libmythtracer_host.so, like raytree_update_driver.cc, for the edited-material round trip the reference does not have:
//   LoadObj -> lights -> SetMaxRecursionLevel(depth) -> BuildRayTree(W, H, &cam, &tree) -> ShadeRayTree -> frame 0;
//   material <name> gets a new reflectance and a new ambient in GetScene()->materials -> UpdateMaterials ->
//   ShadeRayTree must REFUSE the stale tree -> UpdateRayTreeMaterials(&tree) -> ShadeRayTree -> frame 1;
//   RayTrace under the edited materials -> frame 2 (must equal frame 1).
// A second MythTracer on the devices {0, 0} shows the refusals with several devices and with a changed set of names,
// and that UpdateMaterials reaches every replica: its W x H RayTrace after the same edit -> frame 3 (= frame 2).
//
// usage: material_edit_driver <obj> <W> <H> <depth> <ox oy oz pitch yaw roll aov> <material> <refl> <ka r g b>
//                             <n_lights> <12 doubles per light> ... <out.bin>
// stdout: "layers <n> shadow <s>" -- the tree's layers and UpdateRayTreeMaterials's LastStats().rays_shadow
// out.bin: the four frames (W x H x 3 bytes each)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>

#include "mythtracer.h"

using raytracer::Camera;
using raytracer::Light;
using raytracer::Material;
using raytracer::MythTracer;
using raytracer::RayTree;

static int fail(const char *what, MythTracer &mt) {
  fprintf(stderr, "material_edit_driver: %s: %s\n", what, mt.LastError());
  return 1;
}

int main(int argc, char **argv) {
  if (argc < 18) {
    fprintf(stderr, "usage: see the header comment\n");
    return 2;
  }
  int a = 1;
  const char *obj = argv[a++];
  const int W = atoi(argv[a++]), H = atoi(argv[a++]), depth = atoi(argv[a++]);
  double c[7];
  for (double &x : c) x = atof(argv[a++]);
  const std::string name = argv[a++];
  const double refl = atof(argv[a++]);
  double ka[3];
  for (double &x : ka) x = atof(argv[a++]);
  const int n_lights = atoi(argv[a++]);
  if (argc != 18 + 12 * n_lights + 1) return 2;
  std::vector<Light> lights;
  for (int i = 0; i < n_lights; i++) {
    double q[12];
    for (double &x : q) x = atof(argv[a++]);
    lights.push_back(Light{{q[0], q[1], q[2]}, {q[3], q[4], q[5]}, {q[6], q[7], q[8]}, {q[9], q[10], q[11]}});
  }
  const char *out = argv[a++];
  Camera cam{{c[0], c[1], c[2]}, c[3], c[4], c[5], c[6]};
  auto edit = [&](MythTracer &mt) {
    Material &m = *mt.GetScene()->materials.at(name);
    m.reflectance = refl;
    m.ambient = {ka[0], ka[1], ka[2]};
  };

  MythTracer mt;
  mt.SetQuiet(true);
  if (!mt.LoadObj(obj)) return 1;
  mt.GetScene()->lights = lights;
  mt.SetMaxRecursionLevel(depth);
  std::vector<uint8_t> before, updated, fresh, multi;
  int layers = 0;
  unsigned long long shadow = 0;
  {
    RayTree tree;
    // refused before anything is built
    if (mt.UpdateRayTreeMaterials(nullptr) || mt.UpdateRayTreeMaterials(&tree)) return 1;
    if (!mt.BuildRayTree(W, H, &cam, &tree)) return fail("BuildRayTree", mt);
    if (!mt.ShadeRayTree(tree, &before)) return fail("ShadeRayTree", mt);
    if (!mt.UpdateRayTreeMaterials(&tree)) return fail("an update with nothing edited", mt);
    edit(mt);
    if (!mt.UpdateMaterials()) return fail("UpdateMaterials", mt);
    std::vector<uint8_t> stale;
    if (mt.ShadeRayTree(tree, &stale)) {
      fprintf(stderr, "material_edit_driver: a stale tree was shaded\n");
      return 1;
    }
    if (!mt.UpdateRayTreeMaterials(&tree)) return fail("UpdateRayTreeMaterials", mt);
    shadow = mt.LastStats().rays_shadow;
    layers = tree.Layers();
    if (!mt.ShadeRayTree(tree, &updated)) return fail("ShadeRayTree after the update", mt);
  }
  if (!mt.RayTrace(W, H, &cam, &fresh)) return fail("RayTrace", mt);

  MythTracer two;
  two.SetQuiet(true);
  two.SetDevices({0, 0});
  if (!two.LoadObj(obj)) return 1;
  two.GetScene()->lights = lights;
  two.SetMaxRecursionLevel(depth);
  {
    RayTree none;
    if (two.UpdateRayTreeMaterials(&none) || strstr(two.LastError(), "several devices") == nullptr) return 1;
  }
  if (!two.Prepare()) return fail("Prepare on two replicas", two);
  two.GetScene()->materials["one_more"] = std::unique_ptr<Material>(new Material);
  if (two.UpdateMaterials() || strstr(two.LastError(), "by name") == nullptr) return 1;
  two.GetScene()->materials.erase("one_more");
  edit(two);
  if (!two.UpdateMaterials()) return fail("UpdateMaterials on two replicas", two);
  if (!two.RayTrace(W, H, &cam, &multi)) return fail("RayTrace on two replicas", two);

  printf("layers %d shadow %llu\n", layers, shadow);
  FILE *f = fopen(out, "wb");
  if (!f) return 1;
  for (const std::vector<uint8_t> *v : {&before, &updated, &fresh, &multi}) {
    if (v->size() != (size_t)W * H * 3 || fwrite(v->data(), 1, v->size(), f) != v->size()) return 1;
  }
  fclose(f);
  return 0;
}
