#!/usr/bin/env python3
"""Triangles added and removed in place against UpdateGeometry(): the numbers of DESIGN.md section 3.20, from one GPU
session and one process.

  python scripts/edit_triangles_numbers.py [--scenes room,loft] [--width 1920 --height 1080] [--out FILE.json]

Per scene (the bench's room, 101 152 triangles; the loft, 770 720), medians of REPS after WARM warm-ups with min .. max,
every route timed in the same loop.  100 triangles of one material are taken out and appended again at another place,
to and fro: the first repetition removes them where the .obj has them, every later one removes the last 100 add indices.
  edit -> frame    remove_triangles + add_triangles + the update + the first frame (wall), by three routes:
                   update_geometry() with the facade's device-build switch off and on (a new tree, FlatScene::Build,
                   mt_scene_create, every texture uploaded again: the route there was before) and
                   update_triangles_in_place() (mt_scene_edit_triangles)
  the edit         mt_scene_edit_triangles on a scene of its own: total_ms, the build's kernel_ms, and the wall times of
                   its parts (mt_scene_move_times_last): build, regather, read-back, layout (mirrors, checks,
                   derive_layout), upload
  the frame after  the frame that follows the in-place edit (cost history kept) and a frame at rest after it, against
                   the first frame of the re-uploaded scene
The in-place route's frame is compared with the other routes' by bytes in every repetition.  Everything printed is
measured in this run.
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM = 11, 3
ROUTES = ("update_geometry, host build", "update_geometry, device build", "update_triangles_in_place")
PARTS = ("build", "regather", "readback", "layout", "upload")
PER_TRIANGLE = ("tri_vertex", "tri_normal", "tri_uvw", "tri_material", "tri_line_no")
K = 100


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
            names = []
            for fn in os.listdir(td):
                if fn.endswith(".mtl"):
                    names += re.findall(r"^newmtl\s+(\S+)", open(os.path.join(td, fn)).read(), flags=re.M)
            facades = {r: binding.MythTracer(obj) for r in ROUTES}
        for r, m in facades.items():
            m.set_device_tree_build(r != ROUTES[0])
            m.set_lights(scenegen.ROOM_LIGHTS)
            m.set_max_level(5)
            m.render(scenegen.ROOM_CAMERA, W, H)  # uploaded, with a frame's history
        # the scene in add order, and the dense material that most of its first 4000 triangles have, by name
        flat = facades[ROUTES[0]].flatten()
        tris = {}
        for k in PER_TRIANGLE:
            a = np.zeros_like(flat[k])
            a[flat["tri_id"]] = flat[k]
            tris[k] = a
        tris["materials"], tris["textures"] = flat["materials"], flat["textures"]
        n = len(tris["tri_material"])
        head = tris["tri_material"][:min(n, 4000)]
        dense = int(np.bincount(head[head >= 0]).argmax())
        name = [x for x in names if np.array_equal(facades[ROUTES[0]].get_material(x)[0], flat["materials"][dense]["values"])]
        assert name, "the dense material %d has no name in the .mtl" % dense
        idx = np.nonzero(head == dense)[0][::max(1, int((head == dense).sum()) // K)][:K].astype(np.int32)
        assert len(idx) == K
        block = {k: tris[k][idx].copy() for k in PER_TRIANGLE}
        places = [block["tri_vertex"].reshape(-1, 3, 3) + np.array([0.5, 0.25, -0.5]), block["tri_vertex"].reshape(-1, 3, 3)]
        last = np.arange(n - K, n, dtype=np.int32)
        h, built = abi.scene_create_triangles(tris)
        route = {r: [] for r in ROUTES}
        edit_total, edit_kernel, parts = [], [], {p: [] for p in PARTS}
        after, rest, first = [], [], []
        for rep in range(REPS + WARM):
            remove = idx if rep == 0 else last
            target = places[rep % 2]
            frames = {}
            for r, m in facades.items():
                t0 = time.perf_counter()
                m.remove_triangles(remove)
                m.add_triangles(target, block["tri_normal"], block["tri_uvw"], material=name[0], line_no=block["tri_line_no"])
                if r == ROUTES[2]:
                    m.update_triangles_in_place()
                else:
                    m.update_geometry()
                frame = m.render(scenegen.ROOM_CAMERA, W, H)
                wall = (time.perf_counter() - t0) * 1e3
                frames[r] = (wall, frame)
            assert np.array_equal(frames[ROUTES[0]][1]["rgb"], frames[ROUTES[2]][1]["rgb"]), "the in-place frame differs"
            assert np.array_equal(frames[ROUTES[1]][1]["rgb"], frames[ROUTES[2]][1]["rgb"]), "the in-place frame differs"
            again = facades[ROUTES[2]].render(scenegen.ROOM_CAMERA, W, H)
            info = abi.scene_edit_triangles(h, remove, dict(block, tri_vertex=target.reshape(-1, 9)))
            times = abi.scene_move_times(h)
            if rep >= WARM:
                for r in ROUTES:
                    route[r].append(frames[r][0])
                edit_total.append(info["total_ms"])
                edit_kernel.append(info["kernel_ms"])
                for p in PARTS:
                    parts[p].append(times[p])
                after.append(frames[ROUTES[2]][1]["kernel_ms"])
                rest.append(again["kernel_ms"])
                first.append(frames[ROUTES[1]][1]["kernel_ms"])
        abi.scene_destroy(h)
        r = dict(n_tris=n, n_nodes=built["n_nodes"], depth=built["depth"], edited=K,
                 edit_to_frame_ms={k: med(x) for k, x in route.items()}, edit_total_ms=med(edit_total),
                 edit_build_kernel_ms=med(edit_kernel), edit_parts_ms={p: med(x) for p, x in parts.items()},
                 frame_after_edit_kernel_ms=med(after), frame_at_rest_kernel_ms=med(rest), first_frame_kernel_ms=med(first))
        res["scenes"][scene] = r
        print("%s: %d triangles, %d nodes, depth %d, %d triangles out and in" % (scene, n, r["n_nodes"], r["depth"], K))
        for k in ROUTES:
            print("  edit -> frame, %-30s %s ms" % (k, f(r["edit_to_frame_ms"][k])))
        print("  the edit: total %s ms, the build's kernels %s ms" % (f(r["edit_total_ms"]), f(r["edit_build_kernel_ms"])))
        for p in PARTS:
            print("    %-9s %s ms" % (p, f(r["edit_parts_ms"][p])))
        print("  frame kernels: after the edit (history kept) %s ms, at rest %s ms, first frame of a new upload %s ms"
              % (f(r["frame_after_edit_kernel_ms"]), f(r["frame_at_rest_kernel_ms"]), f(r["first_frame_kernel_ms"])))
        sys.stdout.flush()
        for m in facades.values():
            m.close()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
