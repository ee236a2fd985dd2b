// lightupdate_driver — a C++ program against the facade's headers (mythtracer_amd/host/include) and
// libmythtracer_host.so, like lightbuffer_driver.cc, for the round trip of a MOVED light:
//   LoadObj -> lights -> RayTraceLightBuffer(W, H, &cam, &gbuffer, &lightbuffer); one light's position changed ->
//   UpdateLightBuffer(gbuffer, {moved}, &lightbuffer) -> the planes; a fresh RayTraceLightBuffer under the new lights ->
//   its planes (must equal the updated ones); ShadeDirect over the updated planes -> frame 1; SetMaxRecursionLevel(0) +
//   RayTrace -> frame 2 (must equal frame 1).
//
// usage: lightupdate_driver <obj> <W> <H> <ox oy oz pitch yaw roll aov> <n_lights> <12 doubles per light> ...
//                           <moved index> <x y z> <out.bin>
// out.bin: power (f64, n_lights x W x H x 3) and in_shadow (u8, n_lights x W x H) of the updated buffer, the same of the
// fresh one, then the two frames (W x H x 3 bytes)
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
  if (argc < 16) {
    fprintf(stderr, "usage: see the header comment\n");
    return 2;
  }
  int a = 1;
  const char *obj = argv[a++];
  const int W = atoi(argv[a++]), H = atoi(argv[a++]);
  double c[7];
  for (double &x : c) x = atof(argv[a++]);
  const int n_lights = atoi(argv[a++]);
  if (argc != 12 + 12 * n_lights + 4 + 1) return 2;
  MythTracer mt;
  mt.SetQuiet(true);
  if (!mt.LoadObj(obj)) return 1;
  for (int i = 0; i < n_lights; i++) {
    double q[12];
    for (double &x : q) x = atof(argv[a++]);
    mt.GetScene()->lights.push_back(Light{{q[0], q[1], q[2]}, {q[3], q[4], q[5]}, {q[6], q[7], q[8]}, {q[9], q[10], q[11]}});
  }
  const int moved = atoi(argv[a++]);
  double to[3];
  for (double &x : to) x = atof(argv[a++]);
  if (moved < 0 || moved >= n_lights) return 2;
  Camera cam{{c[0], c[1], c[2]}, c[3], c[4], c[5], c[6]};

  GBuffer g;
  g.channels = GBuffer::kPoint | GBuffer::kNormal | GBuffer::kAlbedo | GBuffer::kMaterial;
  LightBuffer lb, fresh;
  if (!mt.RayTraceLightBuffer(W, H, &cam, &g, &lb)) {
    fprintf(stderr, "lightupdate_driver: %s\n", mt.LastError());
    return 1;
  }
  mt.GetScene()->lights[moved].position = {to[0], to[1], to[2]};
  if (!mt.UpdateLightBuffer(g, {moved}, &lb)) {
    fprintf(stderr, "lightupdate_driver: %s\n", mt.LastError());
    return 1;
  }
  printf("primary %llu shadow %llu\n", (unsigned long long)mt.LastStats().rays_primary,
         (unsigned long long)mt.LastStats().rays_shadow);
  if (!mt.RayTraceLightBuffer(W, H, &cam, nullptr, &fresh)) return 1;

  std::vector<uint8_t> relit, traced;
  if (!mt.ShadeDirect(W, H, &cam, g, lb, &relit)) return 1;
  mt.SetMaxRecursionLevel(0);
  if (!mt.RayTrace(W, H, &cam, &traced)) return 1;

  const size_t n = (size_t)W * H, nl = (size_t)n_lights;
  FILE *f = fopen(argv[a++], "wb");
  if (!f) return 1;
  const bool ok = dump(f, lb.power, nl * n * 3) && dump(f, lb.in_shadow, nl * n) && dump(f, fresh.power, nl * n * 3) &&
                  dump(f, fresh.in_shadow, nl * n) && dump(f, relit, n * 3) && dump(f, traced, n * 3);
  fclose(f);
  return ok ? 0 : 1;
}
