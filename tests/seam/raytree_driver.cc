// raytree_driver — a C++ program against the facade's headers (mythtracer_amd/host/include) and libmythtracer_host.so,
// like lightbuffer_driver.cc, for the full-depth relight round trip the reference does not have:
//   LoadObj -> lights -> SetMaxRecursionLevel(depth) -> RayTrace -> frame 1; BuildRayTree(W, H, &cam, &tree) ->
//   ShadeRayTree with the same lights -> frame 2 (must equal frame 1); the lights' colours edited -> ShadeRayTree from
//   the OLD tree -> frame 3; RayTrace under the edited lights -> frame 4 (must equal frame 3).  The tree is moved once on
//   the way (RayTree is move-only).
//
// usage: raytree_driver <obj> <W> <H> <depth> <ox oy oz pitch yaw roll aov> <n_lights> <12 doubles per light> ... <out.bin>
// stdout: "layers <n> rays <n_0> ... secondary <s> shadow <s>" -- the tree's layers and BuildRayTree's LastStats
// out.bin: the four frames (W x H x 3 bytes each)
#include <stdio.h>
#include <stdlib.h>
#include <utility>
#include <vector>

#include "mythtracer.h"

using raytracer::Camera;
using raytracer::Light;
using raytracer::MythTracer;
using raytracer::RayTree;

int main(int argc, char **argv) {
  if (argc < 13) {
    fprintf(stderr, "usage: see the header comment\n");
    return 2;
  }
  int a = 1;
  const char *obj = argv[a++];
  const int W = atoi(argv[a++]), H = atoi(argv[a++]), depth = atoi(argv[a++]);
  double c[7];
  for (double &x : c) x = atof(argv[a++]);
  const int n_lights = atoi(argv[a++]);
  if (argc != 13 + 12 * n_lights + 1) return 2;
  MythTracer mt;
  mt.SetQuiet(true);
  if (!mt.LoadObj(obj)) return 1;
  for (int i = 0; i < n_lights; i++) {
    double q[12];
    for (double &x : q) x = atof(argv[a++]);
    mt.GetScene()->lights.push_back(Light{{q[0], q[1], q[2]}, {q[3], q[4], q[5]}, {q[6], q[7], q[8]}, {q[9], q[10], q[11]}});
  }
  Camera cam{{c[0], c[1], c[2]}, c[3], c[4], c[5], c[6]};
  mt.SetMaxRecursionLevel(depth);

  std::vector<uint8_t> frame, same, relit, fresh;
  if (!mt.RayTrace(W, H, &cam, &frame)) return 1;
  {
    RayTree built;
    if (!mt.BuildRayTree(W, H, &cam, &built)) {
      fprintf(stderr, "raytree_driver: %s\n", mt.LastError());
      return 1;
    }
    RayTree tree = std::move(built);
    if (!built.Empty() || tree.Empty() || tree.Lights() != n_lights || tree.Bytes() == 0) return 1;
    printf("layers %d rays", tree.Layers());
    for (int k = 0; k < tree.Layers(); k++) printf(" %lld", tree.Rays(k));
    printf(" secondary %llu shadow %llu\n", (unsigned long long)mt.LastStats().rays_secondary,
           (unsigned long long)mt.LastStats().rays_shadow);
    if (!mt.ShadeRayTree(tree, &same)) return 1;
    for (Light &l : mt.GetScene()->lights) {  // colours only
      l.ambient = {0.05, 0.1, 0.02};
      l.diffuse = {0.9, 0.6, 0.7};
      l.specular = {0.2, 1.0, 0.6};
    }
    if (!mt.ShadeRayTree(tree, &relit)) return 1;
    RayTree empty;
    if (mt.ShadeRayTree(empty, &fresh)) return 1;  // refused: nothing was built
  }  // (the tree goes before the MythTracer)
  if (!mt.RayTrace(W, H, &cam, &fresh)) return 1;

  FILE *f = fopen(argv[a++], "wb");
  if (!f) return 1;
  const size_t n = (size_t)W * H * 3;
  bool ok = true;
  for (const std::vector<uint8_t> *v : {&frame, &same, &relit, &fresh}) {
    ok = ok && v->size() == n && fwrite(v->data(), 1, n, f) == n;
  }
  fclose(f);
  return ok ? 0 : 1;
}
