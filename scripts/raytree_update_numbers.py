#!/usr/bin/env python3
"""The ray-tree update: the numbers of DESIGN.md section 3.11, from one GPU session.

  python scripts/raytree_update_numbers.py [--width 1920 --height 1080] [--scene room] [--depth 5] [--out FILE.json]
                                           [--other DIR]

Room, the bench's camera and lights, max_depth = 5, light 1 moved to (150, 120, 250); kernel time from HIP events (the
stats of the host calls), median of 11 after 3 warm-ups, with the spread:
  (i)   frame_ms     the frame at max_depth (mt_render_chunk) under the moved lights -- the plain re-trace.  With
                     --other DIR it is also measured with the built checkout of another commit in DIR (the parent's: the
                     yardstick), in a process of its own, BETWEEN two measurements of this tree in the same session.
  (ii)  create       mt_raytree_create under the moved lights -- the only remedy without the update: wall time, kernel
                     time (first to last kernel, the per-layer round trips included), per layer its rays and its tracing
                     kernel's time
  (iii) update       mt_raytree_update_lights of light 1 alone and of all three lights, under the moved lights: kernel
                     time and wall time.  An update reads nothing of the old planes, so repeating it under the same
                     lights repeats the work of the move.
  (iv)  shade_ms     mt_raytree_shade
and the two comparisons: "move a light, see the full-depth frame" = (iii, one light) + (iv) against (i), and (iii)
against the sum of the deeper layers' tracing kernels of (ii) -- whether the single launch hides their tails.
The update of all lights must leave the tree that a fresh create gives: checked on the shaded frame.  Prints a markdown
table and, with --out, writes the numbers as JSON.  Everything printed is measured in this run; nothing is taken from an
earlier one.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM = 11, 3
MOVED, MOVED_TO = 1, (150.0, 120.0, 250.0)


def med(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def moved_lights(lights, indices):
    """`lights` with light MOVED at MOVED_TO and, of `indices`, every other light shifted by (-30, 10, 40)."""
    out = [tuple(float(v) for v in l) for l in lights]
    for i in indices:
        p = MOVED_TO if i == MOVED else (out[i][0] - 30.0, out[i][1] + 10.0, out[i][2] + 40.0)
        out[i] = tuple(p) + out[i][3:]
    return out


def frame_only(args):
    """(i) alone, with the package and libraries of the checkout in --other: the child process of a comparison."""
    sys.path.insert(0, os.path.abspath(args.other))
    from mythtracer_amd import binding, scenegen
    assert os.path.abspath(binding.__file__).startswith(os.path.abspath(args.other)), binding.__file__
    abi = binding.hip_abi()
    with tempfile.TemporaryDirectory() as td:
        obj = scenegen.write_scene(args.scene, td)["obj"]
        flat = binding.MythTracer(obj).flatten()
    h = abi.scene_create(flat)
    abi.set_lights(h, moved_lights(scenegen.ROOM_LIGHTS, [MOVED]))
    sens = binding.sensor(scenegen.ROOM_CAMERA, args.width, args.height)
    t = [abi.render_chunk(h, sens, args.width, args.height, max_depth=args.depth)["stats"]["kernel_ms"]
         for _ in range(REPS + WARM)]
    print(json.dumps(med(t[WARM:])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default="room")
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--other", help="a built checkout of another commit (the parent's) to measure (i) with as well")
    ap.add_argument("--frame-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.frame_only:
        return frame_only(args)
    from mythtracer_amd import binding, scenegen
    W, H, D = args.width, args.height, args.depth
    abi = binding.hip_abi()
    assert abi.device_count() >= 1, "no GPU: these are measurements, there is nothing to report without one"
    with tempfile.TemporaryDirectory() as td:
        obj = scenegen.write_scene(args.scene, td)["obj"]
        flat = binding.MythTracer(obj).flatten()
    h = abi.scene_create(flat)
    A = [tuple(float(v) for v in l) for l in scenegen.ROOM_LIGHTS]
    n_l = len(A)
    B1 = moved_lights(A, [MOVED])
    B3 = moved_lights(A, list(range(n_l)))
    sens = binding.sensor(scenegen.ROOM_CAMERA, W, H)
    res = dict(scene=args.scene, width=W, height=H, max_depth=D, n_lights=n_l, reps=REPS, warmups=WARM, moved=MOVED,
               moved_to=MOVED_TO)

    def frames():
        return [abi.render_chunk(h, sens, W, H, max_depth=D)["stats"]["kernel_ms"] for _ in range(REPS + WARM)][WARM:]

    abi.set_lights(h, B1)
    res["frame_ms"] = med(frames())
    if args.other:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--frame-only", "--other", args.other, "--scene",
                              args.scene, "--width", str(W), "--height", str(H), "--depth", str(D)],
                             stdout=subprocess.PIPE, timeout=600, check=True).stdout.decode()
        res["frame_other_ms"] = json.loads(out.strip().splitlines()[-1])
        res["other"] = args.other
        res["frame_again_ms"] = med(frames())
    frame_b1 = abi.render_chunk(h, sens, W, H, max_depth=D)["rgb"]

    # (ii) the only remedy without the update
    wall, kern, layers = [], [], []
    tree = None
    for _ in range(REPS + WARM):
        if tree is not None:
            abi.raytree_destroy(tree)
        tree, st = abi.raytree_create(h, sens, W, H, max_depth=D)
        wall.append(st["total_ms"])
        kern.append(st["kernel_ms"])
        layers.append(abi.raytree_info(tree)["trace_ms"])
    info = abi.raytree_info(tree)
    res["create_wall_ms"] = med(wall[WARM:])
    res["create_kernel_ms"] = med(kern[WARM:])
    res["n_rays"] = info["n_rays"]
    res["bytes"] = info["bytes"]
    res["layer_trace_ms"] = [med([l[k] for l in layers[WARM:]]) for k in range(info["n_layers"])]
    res["deeper_layers_trace_ms"] = float(sum(m["median"] for m in res["layer_trace_ms"][1:]))
    res["all_layers_trace_ms"] = float(sum(m["median"] for m in res["layer_trace_ms"]))

    # (iii) an update reads nothing of the old planes: the same call again is the same work
    def updates(idx, lights):
        abi.set_lights(h, lights)
        k, w, shadow = [], [], 0
        for _ in range(REPS + WARM):
            st = abi.raytree_update_lights(tree, idx)
            k.append(st["kernel_ms"])
            w.append(st["total_ms"])
            shadow = st["rays_shadow"]
        return med(k[WARM:]), med(w[WARM:]), shadow

    abi.set_lights(h, A)
    abi.raytree_update_lights(tree, list(range(n_l)))  # the tree under A: what a move starts from
    res["update_one_ms"], res["update_one_wall_ms"], res["update_one_rays_shadow"] = updates([MOVED], B1)
    res["update_all_ms"], res["update_all_wall_ms"], res["update_all_rays_shadow"] = updates(list(range(n_l)), B3)
    abi.set_lights(h, B1)
    abi.raytree_update_lights(tree, list(range(n_l)))  # back under B1, through the update
    t = []
    for _ in range(REPS + WARM):
        r = abi.raytree_shade(tree, B1)
        t.append(r["stats"]["kernel_ms"])
    res["shade_ms"] = med(t[WARM:])
    res["updated_tree_shades_to_the_frame"] = bool(np.array_equal(r["rgb"], frame_b1))
    res["move_and_see_ms"] = res["update_one_ms"]["median"] + res["shade_ms"]["median"]
    res["move_and_see_over_frame"] = res["move_and_see_ms"] / res["frame_ms"]["median"]
    res["update_all_over_deeper_layers"] = res["update_all_ms"]["median"] / res["deeper_layers_trace_ms"]

    f = lambda m: "%.3f (%.3f .. %.3f)" % (m["median"], m["min"], m["max"])  # noqa: E731
    print("| figure | ms, median (min .. max) of %d |" % REPS)
    print("|---|---|")
    print("| (i) frame at max_depth = %d under the moved lights, this build, kernels | %s |" % (D, f(res["frame_ms"])))
    if args.other:
        print("| (i) the same frame, the checkout in %s, kernels | %s |" % (args.other, f(res["frame_other_ms"])))
        print("| (i) this build again, after it | %s |" % f(res["frame_again_ms"]))
    print("| (ii) mt_raytree_create, wall | %s |" % f(res["create_wall_ms"]))
    print("| (ii) mt_raytree_create, first to last kernel | %s |" % f(res["create_kernel_ms"]))
    for k, m in enumerate(res["layer_trace_ms"]):
        print("| (ii) layer %d: %d rays, raytree_trace_kernel | %s |" % (k, info["n_rays"][k], f(m)))
    print("| (iii) mt_raytree_update_lights, light %d, kernel | %s |" % (MOVED, f(res["update_one_ms"])))
    print("| (iii) mt_raytree_update_lights, light %d, wall | %s |" % (MOVED, f(res["update_one_wall_ms"])))
    print("| (iii) mt_raytree_update_lights, all %d lights, kernel | %s |" % (n_l, f(res["update_all_ms"])))
    print("| (iii) mt_raytree_update_lights, all %d lights, wall | %s |" % (n_l, f(res["update_all_wall_ms"])))
    print("| (iv) mt_raytree_shade, kernels | %s |" % f(res["shade_ms"]))
    print("(iii): %d shadow-loop iterations for light %d, %d for all lights; the tree holds %d bytes (%.1f MB)"
          % (res["update_one_rays_shadow"], MOVED, res["update_all_rays_shadow"], info["bytes"], info["bytes"] / 1e6))
    print("move a light, see the full-depth frame: update (one light) + shade = %.3f ms against %.3f ms of re-tracing the "
          "frame (%.2f x) and %.3f ms wall of a new tree"
          % (res["move_and_see_ms"], res["frame_ms"]["median"], res["move_and_see_over_frame"],
             res["create_wall_ms"]["median"]))
    print("the single launch: update of all lights %.3f ms against %.3f ms for the tracing kernels of layers >= 1 "
          "(%.2f x; of all layers %.3f ms) -- those kernels trace the rays too, so this bounds the tails from above"
          % (res["update_all_ms"]["median"], res["deeper_layers_trace_ms"], res["update_all_over_deeper_layers"],
             res["all_layers_trace_ms"]))
    print("the updated tree shades to the frame under the moved lights: %s" % res["updated_tree_shades_to_the_frame"])
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    abi.raytree_destroy(tree)
    abi.scene_destroy(h)
    assert res["updated_tree_shades_to_the_frame"]


if __name__ == "__main__":
    main()
