// gbuffer_driver — a C++ program against the facade's headers (mythtracer_amd/host/include) and
// libmythtracer_host.so, like seam_driver.cc, for the one call the reference does not have:
//   LoadObj -> Camera{...} -> RayTraceGBuffer(W, H, &cam, &gbuffer) -> fwrite of every plane,
// then the WorkChunk form for a region with a subset of the planes.
//
// usage: gbuffer_driver <obj> <W> <H> <ox oy oz pitch yaw roll aov> <out.bin> <cx> <cy> <cw> <ch> <chunk.bin>
// out.bin:   depth, point, normal, uvw, albedo (f64), prim, line_no, material (i32), each plane whole, in this order
// chunk.bin: depth (f64), line_no (i32) of the chunk
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "mythtracer.h"

using raytracer::Camera;
using raytracer::GBuffer;
using raytracer::MythTracer;
using raytracer::WorkChunk;

template <typename T>
static bool dump(FILE *f, const std::vector<T> &v, size_t want) {
  return v.size() == want && fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char **argv) {
  if (argc != 17) {
    fprintf(stderr, "usage: see the header comment\n");
    return 2;
  }
  int a = 1;
  const char *obj = argv[a++];
  const int W = atoi(argv[a++]), H = atoi(argv[a++]);
  double c[7];
  for (double &x : c) x = atof(argv[a++]);
  MythTracer mt;
  mt.SetQuiet(true);
  if (!mt.LoadObj(obj)) return 1;
  Camera cam{{c[0], c[1], c[2]}, c[3], c[4], c[5], c[6]};
  mt.SetSupersampling(3);  // ignored by the G-buffer

  GBuffer g;  // channels = kAll
  if (!mt.RayTraceGBuffer(W, H, &cam, &g)) {
    fprintf(stderr, "gbuffer_driver: %s\n", mt.LastError());
    return 1;
  }
  if (g.width != W || g.height != H) return 1;
  const size_t n = (size_t)W * H;
  FILE *f = fopen(argv[a++], "wb");
  if (!f) return 1;
  const bool ok = dump(f, g.depth, n) && dump(f, g.point, 3 * n) && dump(f, g.normal, 3 * n) && dump(f, g.uvw, 3 * n) &&
                  dump(f, g.albedo, 3 * n) && dump(f, g.prim, n) && dump(f, g.line_no, n) && dump(f, g.material, n);
  fclose(f);
  if (!ok) return 1;
  printf("primary %llu hits %llu\n", (unsigned long long)mt.LastStats().rays_primary,
         (unsigned long long)mt.LastStats().shaded_hits);

  WorkChunk work{};
  work.image_width = W;
  work.image_height = H;
  work.chunk_x = atoi(argv[a++]);
  work.chunk_y = atoi(argv[a++]);
  work.chunk_width = atoi(argv[a++]);
  work.chunk_height = atoi(argv[a++]);
  work.camera = cam;
  GBuffer part;
  part.channels = GBuffer::kDepth | GBuffer::kLineNo;
  if (!mt.RayTraceGBuffer(&work, &part)) return 1;
  const size_t m = (size_t)work.chunk_width * work.chunk_height;
  if (!part.point.empty() || !part.normal.empty() || !part.prim.empty()) return 1;  // not asked for
  f = fopen(argv[a++], "wb");
  if (!f) return 1;
  const bool ok2 = dump(f, part.depth, m) && dump(f, part.line_no, m);
  fclose(f);
  return ok2 ? 0 : 1;
}
