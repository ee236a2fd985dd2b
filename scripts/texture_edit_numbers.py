#!/usr/bin/env python3
"""Texture edits on a stored ray tree: the numbers of DESIGN.md section 3.15, from one GPU session.

  python scripts/texture_edit_numbers.py [--width 1920 --height 1080] [--scene room_tex] [--depth 5] [--out FILE.json]
  python scripts/texture_edit_numbers.py --create-only     (uses nothing this feature added: runs on an older checkout)

room_tex, the bench's camera and lights, max_depth = 5.  Kernel times are HIP events (the stats of the host calls).
  create, switch 0   mt_raytree_create's kernel_ms and bytes as they always were, REPS times after WARM warm-ups: every
                     figure, the median and the spread.  With --create-only nothing else is measured, so that the same
                     lines come from the parent commit's checkout for the comparison.
  create, switch 1   the same with mt_scene_set_raytree_uvw(1): what the uvw plane costs in time and bytes.
  update             mt_scene_set_texture of the first texture, alternating a 2 x 2 texture and the original, then
                     mt_raytree_update_materials on the tree with uvw: its kernel_ms and wall time, rays_shadow (0: no
                     light plane is traced again), and the updated tree shaded against mt_render_chunk's frame.
Everything printed is measured in this run.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM = 9, 2


def med(v):
    v = sorted(float(x) for x in v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], all=[round(x, 4) for x in v])


def creates(abi, h, sens, W, H, D):
    ms, info = [], None
    for _ in range(REPS + WARM):
        t, st = abi.raytree_create(h, sens, W, H, max_depth=D)
        ms.append(st["kernel_ms"])
        info = abi.raytree_info(t)
        abi.raytree_destroy(t)
    return dict(kernel_ms=med(ms[WARM:]), bytes=info["bytes"], n_rays=info["n_rays"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default="room_tex")
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--create-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    from mythtracer_amd import binding, scenegen
    W, H, D = args.width, args.height, args.depth
    abi = binding.hip_abi()
    assert abi.device_count() >= 1, "no GPU: these are measurements, there is nothing to report without one"
    with tempfile.TemporaryDirectory() as td:
        flat = binding.MythTracer(scenegen.write_scene(args.scene, td)["obj"]).flatten()
    h = abi.scene_create(flat)
    lights = [tuple(float(v) for v in l) for l in scenegen.ROOM_LIGHTS]
    abi.set_lights(h, lights)
    sens = binding.sensor(scenegen.ROOM_CAMERA, W, H)
    res = dict(scene=args.scene, width=W, height=H, max_depth=D, reps=REPS, warmups=WARM)
    f = lambda m: "%.3f (%.3f .. %.3f)" % (m["median"], m["min"], m["max"])  # noqa: E731
    res["create_switch_0"] = creates(abi, h, sens, W, H, D)
    r = res["create_switch_0"]
    print("create, switch 0: kernel_ms %s, every run %s; bytes %d; rays per layer %s"
          % (f(r["kernel_ms"]), r["kernel_ms"]["all"], r["bytes"], r["n_rays"]))
    if not args.create_only:
        abi.set_raytree_uvw(h, True)
        res["create_switch_1"] = creates(abi, h, sens, W, H, D)
        r1 = res["create_switch_1"]
        print("create, switch 1: kernel_ms %s, every run %s; bytes %d (+ %d = 24 x %d rays)"
              % (f(r1["kernel_ms"]), r1["kernel_ms"]["all"], r1["bytes"], r1["bytes"] - r["bytes"], sum(r1["n_rays"])))
        assert r1["bytes"] - r["bytes"] == 24 * sum(r1["n_rays"])
        tree, _ = abi.raytree_create(h, sens, W, H, max_depth=D)
        original = np.array(flat["textures"][0]["texels"], copy=True)
        small = np.array([[[255, 0, 0], [0, 255, 0]], [[0, 0, 255], [255, 255, 64]]], dtype=np.uint8)
        k, w, shadow, same = [], [], 0, True
        for rep in range(REPS + WARM):
            for texels in (small, original):
                abi.set_texture(h, 0, texels)
                st = abi.raytree_update_materials(tree)
                k.append(st["kernel_ms"])
                w.append(st["total_ms"])
                shadow += st["rays_shadow"]
                if rep == REPS + WARM - 1:
                    rgb = abi.raytree_shade(tree, lights)["rgb"]
                    same = same and bool(np.array_equal(rgb, abi.render_chunk(h, sens, W, H, max_depth=D)["rgb"]))
        res["update_after_set_texture"] = dict(kernel_ms=med(k[2 * WARM:]), wall_ms=med(w[2 * WARM:]), rays_shadow=shadow,
                                               updated_tree_shades_to_the_frame=same)
        u = res["update_after_set_texture"]
        print("mt_raytree_update_materials after mt_scene_set_texture: kernel_ms %s, wall %s, rays_shadow %d; the "
              "updated trees shade to the frame: %s" % (f(u["kernel_ms"]), f(u["wall_ms"]), shadow, same))
        abi.raytree_destroy(tree)
        assert same and shadow == 0
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    abi.scene_destroy(h)


if __name__ == "__main__":
    main()
