#!/usr/bin/env python3
"""Vertex normals and texture coordinates edited on a stored ray tree: the numbers of DESIGN.md section 3.17, from one
GPU session.

  python scripts/vertex_attr_numbers.py [--width 1920 --height 1080] [--scene room] [--depth 5] [--out FILE.json]

The bench's room, camera and lights, max_depth = 5, trees that keep tri and uvw.  Three edits, each applied and taken
back REPS times after WARM warm-ups (the two directions touch the same triangles; the figures are of the way there):
  floor uvw      the floor's texture coordinates doubled              -> mt_raytree_update_materials
  red normal     the red wall's (matte) normals tilted                -> mt_raytree_update_materials
  mirror normal  the mirror's normals tilted                          -> mt_raytree_regrow_materials
Per edit, in the same session:
  new        mt_scene_set_triangle_normals / _uvw (wall) + the tree call (mt_stats.kernel_ms, total_ms)
  yardstick  the only route there was: mt_scene_create from the edited description (wall) + mt_raytree_create
             (mt_stats.kernel_ms, total_ms)
The last tree of every edit is shaded against mt_render_chunk's frame.  Everything printed is measured in this run.
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

REPS, WARM = 11, 3


def med(v):
    v = sorted(float(x) for x in v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


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


def tilted(normal, sel):
    out = np.array(normal, dtype=np.float64).reshape(-1, 3, 3).copy()
    out[sel] = out[sel] + np.array([0.03, 0.02, 0.01])
    out[sel] /= np.sqrt((out[sel] ** 2).sum(axis=-1, keepdims=True))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default="room")
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
    normal_a = np.array(flat["tri_normal"], dtype=np.float64).reshape(-1, 3, 3)
    uvw_a = np.array(flat["tri_uvw"], dtype=np.float64).reshape(-1, 3, 3)
    uvw_b = uvw_a.copy()
    uvw_b[of == "floor"] = uvw_b[of == "floor"] * 2.0 + 0.25
    cases = [
        ("floor uvw", "tri_uvw", uvw_a, uvw_b, "update"),
        ("red normal", "tri_normal", normal_a, tilted(normal_a, of == "red"), "update"),
        ("mirror normal", "tri_normal", normal_a, tilted(normal_a, of == "mirror"), "regrow"),
    ]
    lights = [tuple(float(v) for v in l) for l in scenegen.ROOM_LIGHTS]
    sens = binding.sensor(scenegen.ROOM_CAMERA, W, H)
    h = abi.scene_create(flat)
    abi.set_lights(h, lights)
    abi.set_raytree_tri(h, True)
    abi.set_raytree_uvw(h, True)
    res = dict(scene=args.scene, width=W, height=H, max_depth=D, reps=REPS, warmups=WARM, n_tris=len(of), cases={})
    f = lambda m: "%.3f (%.3f .. %.3f)" % (m["median"], m["min"], m["max"])  # noqa: E731
    for name, key, A, B, call in cases:
        setter = abi.set_triangle_normals if key == "tri_normal" else abi.set_triangle_uvw
        take = abi.raytree_update_materials if call == "update" else abi.raytree_regrow
        changed = int((A.reshape(len(A), -1) != B.reshape(len(B), -1)).any(axis=1).sum())
        assert changed > 0, name
        tree, _ = abi.raytree_create(h, sens, W, H, max_depth=D)
        set_ms, take_k, take_w, scene_ms, create_k, create_w, notes = [], [], [], [], [], [], []
        for rep in range(REPS + WARM):
            for way, now in enumerate((B, A)):
                t0 = time.perf_counter()
                setter(h, now)
                dt = (time.perf_counter() - t0) * 1e3
                out = take(tree)
                attr = abi.raytree_attr_info(tree)
                # the yardstick: a scene created from the edited description, and a fresh tree on it
                built = dict(flat)
                built[key] = np.ascontiguousarray(now).reshape(np.shape(flat[key]))
                t0 = time.perf_counter()
                h2 = abi.scene_create(built)
                ds = (time.perf_counter() - t0) * 1e3
                abi.set_lights(h2, lights)
                abi.set_raytree_tri(h2, True)
                abi.set_raytree_uvw(h2, True)
                t2, st = abi.raytree_create(h2, sens, W, H, max_depth=D)
                assert abi.raytree_info(t2)["n_rays"] == abi.raytree_info(tree)["n_rays"]
                abi.raytree_destroy(t2)
                abi.scene_destroy(h2)
                if way == 0 and rep >= WARM:
                    set_ms.append(dt)
                    take_k.append(out["kernel_ms"])
                    take_w.append(out["total_ms"])
                    scene_ms.append(ds)
                    create_k.append(st["kernel_ms"])
                    create_w.append(st["total_ms"])
                    notes.append(dict(attr, traced=sum(out.get("traced", [])), rays_secondary=out["rays_secondary"]))
        same = bool(np.array_equal(abi.raytree_shade(tree, lights)["rgb"], abi.render_chunk(h, sens, W, H, max_depth=D)["rgb"]))
        r = dict(call=call, triangles_changed=changed, rays=sum(abi.raytree_info(tree)["n_rays"]), last=notes[-1],
                 set_wall_ms=med(set_ms), take_kernel_ms=med(take_k), take_total_ms=med(take_w),
                 new_wall_ms=med([a + b for a, b in zip(set_ms, take_w)]),
                 scene_create_wall_ms=med(scene_ms), create_kernel_ms=med(create_k), create_total_ms=med(create_w),
                 yardstick_wall_ms=med([a + b for a, b in zip(scene_ms, create_w)]), tree_shades_to_the_frame=same)
        res["cases"][name] = r
        print("%s: %d of %d triangles, %s, %d rays in the tree; last call %s" % (name, changed, len(of), call, r["rays"], r["last"]))
        print("  new:       set wall %s ms; %s kernel %s ms, total %s ms; together %s ms" %
              (f(r["set_wall_ms"]), call, f(r["take_kernel_ms"]), f(r["take_total_ms"]), f(r["new_wall_ms"])))
        print("  yardstick: mt_scene_create wall %s ms; mt_raytree_create kernel %s ms, total %s ms; together %s ms" %
              (f(r["scene_create_wall_ms"]), f(r["create_kernel_ms"]), f(r["create_total_ms"]), f(r["yardstick_wall_ms"])))
        print("  the tree shades to mt_render_chunk's frame: %s" % same)
        abi.raytree_destroy(tree)
        assert same
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    abi.scene_destroy(h)


if __name__ == "__main__":
    main()
