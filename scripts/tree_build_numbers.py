#!/usr/bin/env python3
"""The octree built on the GPU against OctTree::Finalize on the host: the numbers of DESIGN.md section 3.18, from one
GPU session and one process.

  python scripts/tree_build_numbers.py [--scenes room,loft] [--width 1920 --height 1080] [--out FILE.json]

Per scene (the bench's room, 101 152 triangles; the loft, 770 720), medians of REPS after WARM warm-ups with min .. max,
every route timed in the same loop:
  device build   mt_octree_build on the triangles in add order: kernel_ms (HIP events, first to last kernel, the
                 per-level round trips included) and total_ms (the call: allocations, the vertices' upload, the kernels)
  host build     OctTree::Finalize through mth_finalize (wall), on a tree marked unfinalized by UpdateGeometry -- the
                 code every scene went through before there was a device builder
  moved -> frame set_triangle_vertices + update_geometry + the first frame (wall), with the facade's switch off and on:
                 the tree, FlatScene::Build, mt_scene_create and one frame at --width x --height, depth 5
The device tree is compared with the host's by bits once per scene.  Everything printed is measured in this run.
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
            facades = {on: binding.MythTracer(obj) for on in (False, True)}
        for on, m in facades.items():
            m.set_device_tree_build(on)
            m.set_lights(scenegen.ROOM_LIGHTS)
            m.set_max_level(5)
        host = facades[False]
        data, _, _ = host.triangles()
        v = np.ascontiguousarray(data[:, :9])
        # the same tree, once
        t, info = abi.octree_build(v)
        dev = abi.octree_read(t)
        abi.octree_destroy(t)
        want = host.tree()
        for a, b in (("node_aabb", "aabb"), ("node_center", "center"), ("first_child", "first_child"),
                     ("prim_begin", "prim_begin"), ("prim_count", "prim_count"), ("tri_id", "prim_ids")):
            assert np.array_equal(np.ascontiguousarray(dev[a]).view(np.uint8), np.ascontiguousarray(want[b]).view(np.uint8)), a
        assert dev["depth"] == want["depth"]
        idx = np.arange(0, min(len(v), 4000), 40, dtype=np.int32)  # the triangles that move, to and fro
        there, back = v[idx].reshape(-1, 3, 3) + np.array([0.5, 0.25, -0.5]), v[idx].reshape(-1, 3, 3)
        dev_k, dev_t, host_w, route = [], [], [], {False: [], True: []}
        for rep in range(REPS + WARM):
            t, i = abi.octree_build(v)
            abi.octree_destroy(t)
            host.update_geometry()  # (marks the tree unfinalized; not timed)
            t0 = time.perf_counter()
            host.finalize()
            hw = (time.perf_counter() - t0) * 1e3
            rw = {}
            for on, m in facades.items():
                t0 = time.perf_counter()
                m.set_triangle_vertices(idx, there if rep % 2 == 0 else back)
                m.update_geometry()
                frame = m.render(scenegen.ROOM_CAMERA, W, H)
                rw[on] = ((time.perf_counter() - t0) * 1e3, frame["rgb"])
            assert np.array_equal(rw[False][1], rw[True][1]), "the two builders' frames differ"
            if rep >= WARM:
                dev_k.append(i["kernel_ms"])
                dev_t.append(i["total_ms"])
                host_w.append(hw)
                for on in route:
                    route[on].append(rw[on][0])
        r = dict(n_tris=len(v), n_nodes=info["n_nodes"], depth=info["depth"], device_kernel_ms=med(dev_k),
                 device_total_ms=med(dev_t), host_finalize_ms=med(host_w), moved_to_frame_host_ms=med(route[False]),
                 moved_to_frame_device_ms=med(route[True]))
        res["scenes"][scene] = r
        print("%s: %d triangles, %d nodes, depth %d" % (scene, r["n_tris"], r["n_nodes"], r["depth"]))
        print("  mt_octree_build   kernel %s ms, total %s ms" % (f(r["device_kernel_ms"]), f(r["device_total_ms"])))
        print("  host Finalize     wall %s ms" % f(r["host_finalize_ms"]))
        print("  moved -> frame    switch off %s ms, switch on %s ms (%d x %d, depth 5)"
              % (f(r["moved_to_frame_host_ms"]), f(r["moved_to_frame_device_ms"]), W, H))
        for m in facades.values():
            m.close()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
