#!/usr/bin/env python3
"""Ray-list trees and linear colours: the numbers of DESIGN.md section 3.12, from one GPU session.

  python scripts/raylist_numbers.py [--width 1920 --height 1080] [--scene room] [--depth 5] [--out FILE.json]

Room, the bench's camera and lights, max_depth = 5, HIP events (kernel_ms of the calls' stats) and wall time (total_ms),
median of 11 after 3 warm-ups, with min .. max:
  1. mt_raytree_create from the sensor: the path that was there before, the yardstick
  2. mt_raytree_create_rays_device from the same width x height rays already in HBM (a torch tensor): the difference
     to 1 is the import kernel and the read-back of its count of refused rays
  3. mt_raytree_create_rays from host memory: 48 bytes per ray over PCIe on top
  4. mt_raytree_shade_colors against mt_raytree_shade: 24 bytes written per ray of layer 0 instead of 3
  5. a 2048x1024 equirectangular panorama from the camera's position: create and both shades
The rays of 2 and 3 are the sensor tree's own layer 0 un-permuted by `pixel`, so the three trees are the same tree; the
script checks that (layer sizes and shaded bytes).  Nothing here is a pass/fail threshold.  Prints a markdown table and,
with --out, writes the numbers as JSON.  Everything printed is measured in this run.
"""
import argparse
import json
import math
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM = 11, 3


def med(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def panorama_rays(w, h, eye):
    """pixel (x, y) looks along (sin t sin p, cos t, sin t cos p), t = pi (y + 0.5) / h, p = 2 pi (x + 0.5) / w"""
    t = math.pi * (np.arange(h) + 0.5) / h
    p = 2.0 * math.pi * (np.arange(w) + 0.5) / w
    rays = np.zeros((h, w, 6))
    rays[:, :, :3] = eye
    rays[:, :, 3] = np.sin(t)[:, None] * np.sin(p)[None, :]
    rays[:, :, 4] = np.cos(t)[:, None]
    rays[:, :, 5] = np.sin(t)[:, None] * np.cos(p)[None, :]
    return rays.reshape(w * h, 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default="room")
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--pano", type=int, nargs=2, default=(2048, 1024))
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()  # (torch's copy of the HIP runtime first, as tests/conftest.py does)
    from mythtracer_amd import binding, scenegen
    W, H, D = args.width, args.height, args.depth
    abi = binding.hip_abi()
    assert abi.device_count() >= 1, "no GPU: these are measurements, there is nothing to report without one"
    with tempfile.TemporaryDirectory() as td:
        obj = scenegen.write_scene(args.scene, td)["obj"]
        flat = binding.MythTracer(obj).flatten()
    h = abi.scene_create(flat)
    lights = scenegen.ROOM_LIGHTS
    abi.set_lights(h, lights)
    sens = binding.sensor(scenegen.ROOM_CAMERA, W, H)
    res = dict(scene=args.scene, width=W, height=H, max_depth=D, n_lights=len(lights), reps=REPS, warmups=WARM)

    def measure(create):
        """(tree of the last repetition, wall and kernel medians)"""
        wall, kern, tree = [], [], None
        for _ in range(REPS + WARM):
            if tree is not None:
                abi.raytree_destroy(tree)
            tree, st = create()
            wall.append(st["total_ms"])
            kern.append(st["kernel_ms"])
        return tree, dict(wall_ms=med(wall[WARM:]), kernel_ms=med(kern[WARM:]))

    def shades(tree):
        out = {}
        for name, fn in (("shade", abi.raytree_shade), ("shade_colors", abi.raytree_shade_colors)):
            wall, kern = [], []
            for _ in range(REPS + WARM):
                r = fn(tree, lights)
                wall.append(r["stats"]["total_ms"])
                kern.append(r["stats"]["kernel_ms"])
            out[name] = dict(wall_ms=med(wall[WARM:]), kernel_ms=med(kern[WARM:]))
        return out

    # 1. the sensor tree
    tree, res["create_sensor"] = measure(lambda: abi.raytree_create(h, sens, W, H, max_depth=D))
    info = abi.raytree_info(tree)
    res["n_rays"] = info["n_rays"]
    lay = abi.raytree_read_layer(tree, 0, ("ray", "pixel"))
    rays = np.zeros((W * H, 6))
    rays[lay["pixel"]] = lay["ray"]
    rgb = abi.raytree_shade(tree, lights)["rgb"]
    # 4. on the sensor tree
    res["shades_sensor"] = shades(tree)
    abi.raytree_destroy(tree)
    # 2. the same rays from HBM
    d_rays = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    tree, res["create_rays_device"] = measure(lambda: abi.raytree_create_rays(h, d_rays, W, max_depth=D, device=True))
    same = abi.raytree_info(tree)["n_rays"] == info["n_rays"] and np.array_equal(abi.raytree_shade(tree, lights)["rgb"], rgb)
    abi.raytree_destroy(tree)
    del d_rays
    # 3. from host memory
    tree, res["create_rays_host"] = measure(lambda: abi.raytree_create_rays(h, rays, W, max_depth=D))
    same = same and abi.raytree_info(tree)["n_rays"] == info["n_rays"] and \
        np.array_equal(abi.raytree_shade(tree, lights)["rgb"], rgb)
    res["same_tree"] = bool(same)
    abi.raytree_destroy(tree)
    # 5. a panorama
    pw, ph = args.pano
    pano = panorama_rays(pw, ph, scenegen.ROOM_CAMERA[:3])
    tree, res["create_panorama"] = measure(lambda: abi.raytree_create_rays(h, pano, pw, max_depth=D))
    pinfo = abi.raytree_info(tree)
    res["panorama"] = dict(width=pw, height=ph, n_rays=pinfo["n_rays"], bytes=pinfo["bytes"])
    res["shades_panorama"] = shades(tree)
    abi.raytree_destroy(tree)
    abi.scene_destroy(h)

    f = lambda m: "%.3f (%.3f .. %.3f)" % (m["median"], m["min"], m["max"])  # noqa: E731
    print("| | figure | kernels, ms | wall, ms |")
    print("|---|---|---|---|")
    rows = [("1", "mt_raytree_create from the sensor, %dx%d" % (W, H), res["create_sensor"]),
            ("2", "mt_raytree_create_rays_device, the same %d rays in HBM" % (W * H), res["create_rays_device"]),
            ("3", "mt_raytree_create_rays, the same rays in host memory (%.1f MB)" % (W * H * 48 / 1e6), res["create_rays_host"]),
            ("4", "mt_raytree_shade, sensor tree (%.1f MB written)" % (W * H * 3 / 1e6), res["shades_sensor"]["shade"]),
            ("4", "mt_raytree_shade_colors, sensor tree (%.1f MB written)" % (W * H * 24 / 1e6), res["shades_sensor"]["shade_colors"]),
            ("5", "mt_raytree_create_rays, %dx%d panorama, layers %s" % (pw, ph, pinfo["n_rays"]), res["create_panorama"]),
            ("5", "mt_raytree_shade, panorama", res["shades_panorama"]["shade"]),
            ("5", "mt_raytree_shade_colors, panorama", res["shades_panorama"]["shade_colors"])]
    for no, what, m in rows:
        print("| %s | %s | %s | %s |" % (no, what, f(m["kernel_ms"]), f(m["wall_ms"])))
    print("layers of the sensor tree: %s; the trees of 2 and 3 are the sensor tree (layer sizes, shaded bytes): %s"
          % (info["n_rays"], res["same_tree"]))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    assert res["same_tree"]


if __name__ == "__main__":
    main()
