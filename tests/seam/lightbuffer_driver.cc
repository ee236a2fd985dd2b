// lightbuffer_driver — a C++ program against the facade's headers (mythtracer_amd/host/include) and
// libmythtracer_host.so, like gbuffer_driver.cc, for the relight round trip the reference does not have:
//   LoadObj -> lights -> RayTraceLightBuffer(W, H, &cam, &gbuffer, &lightbuffer) -> fwrite of the planes,
//   ShadeDirect with the same lights -> frame 1; the lights' colours edited -> ShadeDirect with the OLD buffers ->
//   frame 2; SetMaxRecursionLevel(0) + RayTrace under the edited lights -> frame 3 (must equal frame 2).
//
// usage: lightbuffer_driver <obj> <W> <H> <ox oy oz pitch yaw roll aov> <n_lights> <12 doubles per light> ... <out.bin>
// out.bin: power (f64, n_lights x W x H x 3), in_shadow (u8, n_lights x W x H), then the three frames (W x H x 3 bytes)
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "mythtracer.h"

using raytracer::Camera;
using raytracer::GBuffer;
using raytracer::Light;
using raytracer::LightBuffer;
using raytracer::MythTracer;

template <typename T>
static bool dump(FILE *f, const std::vector<T> &v, size_t want) {
  return v.size() == want && fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char **argv) {
  if (argc < 12) {
    fprintf(stderr, "usage: see the header comment\n");
    return 2;
  }
  int a = 1;
  const char *obj = argv[a++];
  const int W = atoi(argv[a++]), H = atoi(argv[a++]);
  double c[7];
  for (double &x : c) x = atof(argv[a++]);
  const int n_lights = atoi(argv[a++]);
  if (argc != 12 + 12 * n_lights + 1) return 2;
  MythTracer mt;
  mt.SetQuiet(true);
  if (!mt.LoadObj(obj)) return 1;
  for (int i = 0; i < n_lights; i++) {
    double q[12];
    for (double &x : q) x = atof(argv[a++]);
    mt.GetScene()->lights.push_back(Light{{q[0], q[1], q[2]}, {q[3], q[4], q[5]}, {q[6], q[7], q[8]}, {q[9], q[10], q[11]}});
  }
  Camera cam{{c[0], c[1], c[2]}, c[3], c[4], c[5], c[6]};

  GBuffer g;
  g.channels = GBuffer::kPoint | GBuffer::kNormal | GBuffer::kAlbedo | GBuffer::kMaterial;
  LightBuffer lb;
  if (!mt.RayTraceLightBuffer(W, H, &cam, &g, &lb)) {
    fprintf(stderr, "lightbuffer_driver: %s\n", mt.LastError());
    return 1;
  }
  const size_t n = (size_t)W * H, nl = (size_t)n_lights;
  if (lb.width != W || lb.height != H || lb.n_lights != n_lights || !g.depth.empty()) return 1;
  printf("primary %llu shadow %llu\n", (unsigned long long)mt.LastStats().rays_primary,
         (unsigned long long)mt.LastStats().rays_shadow);

  std::vector<uint8_t> same, relit, fresh;
  if (!mt.ShadeDirect(W, H, &cam, g, lb, &same)) return 1;
  for (Light &l : mt.GetScene()->lights) {  // colours only
    l.ambient = {0.05, 0.1, 0.02};
    l.diffuse = {0.9, 0.6, 0.7};
    l.specular = {0.2, 1.0, 0.6};
  }
  if (!mt.ShadeDirect(W, H, &cam, g, lb, &relit)) return 1;
  mt.SetMaxRecursionLevel(0);
  if (!mt.RayTrace(W, H, &cam, &fresh)) return 1;

  FILE *f = fopen(argv[a++], "wb");
  if (!f) return 1;
  const bool ok = dump(f, lb.power, nl * n * 3) && dump(f, lb.in_shadow, nl * n) && dump(f, same, n * 3) &&
                  dump(f, relit, n * 3) && dump(f, fresh, n * 3);
  fclose(f);
  return ok ? 0 : 1;
}
