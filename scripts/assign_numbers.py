#!/usr/bin/env python3
"""Triangles given another material on a stored ray tree: the numbers of DESIGN.md section 3.16, from one GPU session.

  python scripts/assign_numbers.py [--width 1920 --height 1080] [--scene room] [--group blue --target mirror]
                                   [--depth 5] [--out FILE.json]

The bench's room, camera and lights, max_depth = 5, trees that keep tri (mt_scene_set_raytree_tri).  One object -- the
triangles of the .obj's `usemtl GROUP` -- is given the material of `usemtl TARGET` and then its own again, REPS times
after WARM warm-ups; every figure is printed with its median and spread.
  set      mt_scene_set_triangle_materials: wall time of the call (it waits for the device and copies; no kernel).
  regrow   mt_raytree_regrow_materials after each set: mt_stats.kernel_ms and total_ms, kept and traced rays.
  create   a fresh mt_raytree_create under the same assignment: mt_stats.kernel_ms and total_ms.
The last regrown tree is shaded against mt_render_chunk's frame.  Everything printed is measured in this run.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM = 3, 1


def med(v):
    v = sorted(float(x) for x in v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], all=[round(x, 4) for x in v])


def group_of_lines(obj):
    """{line of an f line (0-based, a triangle's line_no): the usemtl in force}"""
    out, group = {}, None
    for no, text in enumerate(open(obj)):
        words = text.split()
        if words and words[0] == "usemtl":
            group = words[1]
        elif words and words[0] == "f":
            out[no] = group
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default="room")
    ap.add_argument("--group", default="blue")
    ap.add_argument("--target", default="mirror")
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    from mythtracer_amd import binding, scenegen
    W, H, D = args.width, args.height, args.depth
    abi = binding.hip_abi()
    assert abi.device_count() >= 1, "no GPU: these are measurements, there is nothing to report without one"
    with tempfile.TemporaryDirectory() as td:
        obj = scenegen.write_scene(args.scene, td)["obj"]
        flat = binding.MythTracer(obj).flatten()
        groups = group_of_lines(obj)
    of = np.array([groups[int(l)] for l in flat["tri_line_no"]])
    A = np.array(flat["tri_material"], dtype=np.int32)
    target = int(A[np.nonzero(of == args.target)[0][0]])
    B = A.copy()
    B[of == args.group] = target
    n_changed = int((A != B).sum())
    assert n_changed > 0
    h = abi.scene_create(flat)
    lights = [tuple(float(v) for v in l) for l in scenegen.ROOM_LIGHTS]
    abi.set_lights(h, lights)
    abi.set_raytree_tri(h, True)
    sens = binding.sensor(scenegen.ROOM_CAMERA, W, H)
    tree, _ = abi.raytree_create(h, sens, W, H, max_depth=D)
    set_ms, regrow_k, regrow_w, create_k, create_w, moves = [], [], [], [], [], []
    for rep in range(REPS + WARM):
        for now in (B, A):
            t0 = time.perf_counter()
            abi.set_triangle_materials(h, now)
            set_ms.append((time.perf_counter() - t0) * 1e3)
            out = abi.raytree_regrow(tree)
            regrow_k.append(out["kernel_ms"])
            regrow_w.append(out["total_ms"])
            moves.append(dict(regrown=out["regrown"], kept=sum(out["kept"]), traced=sum(out["traced"]), rays_shadow=out["rays_shadow"]))
            t, st = abi.raytree_create(h, sens, W, H, max_depth=D)
            create_k.append(st["kernel_ms"])
            create_w.append(st["total_ms"])
            info = abi.raytree_info(t)
            assert info["n_rays"] == abi.raytree_info(tree)["n_rays"] and info["bytes"] == abi.raytree_info(tree)["bytes"]
            abi.raytree_destroy(t)
    same = bool(np.array_equal(abi.raytree_shade(tree, lights)["rgb"], abi.render_chunk(h, sens, W, H, max_depth=D)["rgb"]))
    skip = 2 * WARM
    res = dict(scene=args.scene, width=W, height=H, max_depth=D, reps=REPS, warmups=WARM, group=args.group, target=args.target,
               triangles_reassigned=n_changed, n_tris=len(A), n_rays=abi.raytree_info(tree)["n_rays"],
               set_wall_ms=med(set_ms[skip:]), regrown_tree_shades_to_the_frame=same)
    f = lambda m: "%.3f (%.3f .. %.3f) %s" % (m["median"], m["min"], m["max"], m["all"])  # noqa: E731
    print("%s %dx%d depth %d, %s -> %s and back: %d of %d triangles, %d rays in the tree as it is" %
          (args.scene, W, H, D, args.group, args.target, n_changed, len(A), sum(res["n_rays"])))
    print("mt_scene_set_triangle_materials, wall ms: %s" % f(res["set_wall_ms"]))
    # the two directions are two different amounts of work: reported apart
    for k, way in enumerate(("%s -> %s" % (args.group, args.target), "and back")):
        r = dict(regrow_kernel_ms=med(regrow_k[skip + k::2]), regrow_total_ms=med(regrow_w[skip + k::2]),
                 create_kernel_ms=med(create_k[skip + k::2]), create_total_ms=med(create_w[skip + k::2]), regrows=moves[skip + k::2])
        res["there" if k == 0 else "back"] = r
        print("%s:" % way)
        print("  mt_raytree_regrow_materials: kernel_ms %s, total_ms %s" % (f(r["regrow_kernel_ms"]), f(r["regrow_total_ms"])))
        print("    per call:", r["regrows"])
        print("  mt_raytree_create (fresh): kernel_ms %s, total_ms %s" % (f(r["create_kernel_ms"]), f(r["create_total_ms"])))
    print("the last regrown tree shades to mt_render_chunk's frame: %s" % same)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    abi.raytree_destroy(tree)
    abi.scene_destroy(h)
    assert same


if __name__ == "__main__":
    main()
