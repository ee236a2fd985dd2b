#!/usr/bin/env python3
"""Triangles moved in place against UpdateGeometry(): the numbers of DESIGN.md section 3.19, from one GPU session and
one process.

  python scripts/move_vertices_numbers.py [--scenes room,loft] [--width 1920 --height 1080] [--out FILE.json]

Per scene (the bench's room, 101 152 triangles; the loft, 770 720), medians of REPS after WARM warm-ups with min .. max,
every route timed in the same loop, the same 100 triangles moved to and fro:
  moved -> frame   set_triangle_vertices + the update + the first frame (wall), by three routes: update_geometry() with
                   the facade's device-build switch off and on (a new tree, FlatScene::Build, mt_scene_create, every
                   texture uploaded again) and update_geometry_in_place() (mt_scene_set_triangle_vertices)
  the set          mt_scene_set_triangle_vertices on a scene of its own: total_ms, the build's kernel_ms, and the wall
                   times of its parts (mt_scene_move_times_last): build, regather, read-back, layout (mirrors, checks,
                   derive_layout), upload
  the frame after  the frame that follows the in-place move (cost history kept) and a frame at rest after it, against
                   the first frame of the re-uploaded scene
The in-place route's frame is compared with the other routes' by bytes in every repetition.  Everything printed is
measured in this run.
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
ROUTES = ("update_geometry, host build", "update_geometry, device build", "update_geometry_in_place")
PARTS = ("build", "regather", "readback", "layout", "upload")


def med(v):
    v = sorted(float(x) for x in v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="room,loft")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out")
    args = ap.parse_args()
    from mythtracer_amd import binding, scenegen
    abi = binding.hip_abi()
    assert abi.device_count() >= 1, "no GPU: these are measurements, there is nothing to report without one"
    W, H = args.width, args.height
    f = lambda m: "%.3f (%.3f .. %.3f)" % (m["median"], m["min"], m["max"])  # noqa: E731
    res = dict(width=W, height=H, reps=REPS, warmups=WARM, scenes={})
    for scene in args.scenes.split(","):
        with tempfile.TemporaryDirectory() as td:
            obj = scenegen.write_scene(scene, td)["obj"]
            facades = {r: binding.MythTracer(obj) for r in ROUTES}
        for r, m in facades.items():
            m.set_device_tree_build(r != ROUTES[0])
            m.set_lights(scenegen.ROOM_LIGHTS)
            m.set_max_level(5)
            m.render(scenegen.ROOM_CAMERA, W, H)  # uploaded, with a frame's history
        data, _, _ = facades[ROUTES[0]].triangles()
        v = np.ascontiguousarray(data[:, :9])
        idx = np.arange(0, min(len(v), 4000), 40, dtype=np.int32)  # the triangles that move, to and fro
        there, back = v[idx].reshape(-1, 3, 3) + np.array([0.5, 0.25, -0.5]), v[idx].reshape(-1, 3, 3)
        # the set alone, on a scene made from the same triangles in add order
        flat = facades[ROUTES[0]].flatten()
        tris = {}
        for k in ("tri_vertex", "tri_normal", "tri_uvw", "tri_material", "tri_line_no"):
            a = np.zeros_like(flat[k])
            a[flat["tri_id"]] = flat[k]
            tris[k] = a
        tris["materials"], tris["textures"] = flat["materials"], flat["textures"]
        h, built = abi.scene_create_triangles(tris)
        route = {r: [] for r in ROUTES}
        set_total, set_kernel, parts = [], [], {p: [] for p in PARTS}
        after, rest, first = [], [], []
        for rep in range(REPS + WARM):
            target = there if rep % 2 == 0 else back
            frames = {}
            for r, m in facades.items():
                t0 = time.perf_counter()
                m.set_triangle_vertices(idx, target)
                if r == ROUTES[2]:
                    m.update_geometry_in_place()
                else:
                    m.update_geometry()
                frame = m.render(scenegen.ROOM_CAMERA, W, H)
                wall = (time.perf_counter() - t0) * 1e3
                frames[r] = (wall, frame)
            assert np.array_equal(frames[ROUTES[0]][1]["rgb"], frames[ROUTES[2]][1]["rgb"]), "the in-place frame differs"
            assert np.array_equal(frames[ROUTES[1]][1]["rgb"], frames[ROUTES[2]][1]["rgb"]), "the in-place frame differs"
            again = facades[ROUTES[2]].render(scenegen.ROOM_CAMERA, W, H)
            info = abi.scene_set_triangle_vertices(h, idx, target)
            times = abi.scene_move_times(h)
            if rep >= WARM:
                for r in ROUTES:
                    route[r].append(frames[r][0])
                set_total.append(info["total_ms"])
                set_kernel.append(info["kernel_ms"])
                for p in PARTS:
                    parts[p].append(times[p])
                after.append(frames[ROUTES[2]][1]["kernel_ms"])
                rest.append(again["kernel_ms"])
                first.append(frames[ROUTES[1]][1]["kernel_ms"])
        abi.scene_destroy(h)
        r = dict(n_tris=len(v), n_nodes=built["n_nodes"], depth=built["depth"], moved=len(idx),
                 moved_to_frame_ms={k: med(x) for k, x in route.items()}, set_total_ms=med(set_total),
                 set_build_kernel_ms=med(set_kernel), set_parts_ms={p: med(x) for p, x in parts.items()},
                 frame_after_move_kernel_ms=med(after), frame_at_rest_kernel_ms=med(rest), first_frame_kernel_ms=med(first))
        res["scenes"][scene] = r
        print("%s: %d triangles, %d nodes, depth %d, %d triangles moved" % (scene, r["n_tris"], r["n_nodes"], r["depth"], len(idx)))
        for k in ROUTES:
            print("  moved -> frame, %-30s %s ms" % (k, f(r["moved_to_frame_ms"][k])))
        print("  the set: total %s ms, the build's kernels %s ms" % (f(r["set_total_ms"]), f(r["set_build_kernel_ms"])))
        for p in PARTS:
            print("    %-9s %s ms" % (p, f(r["set_parts_ms"][p])))
        print("  frame kernels: after the move (history kept) %s ms, at rest %s ms, first frame of a new upload %s ms"
              % (f(r["frame_after_move_kernel_ms"]), f(r["frame_at_rest_kernel_ms"]), f(r["first_frame_kernel_ms"])))
        for m in facades.values():
            m.close()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
