#!/usr/bin/env python3
"""The ray-tree buffer: the numbers of DESIGN.md section 3.10, from one GPU session.

  python scripts/raytree_numbers.py [--width 1920 --height 1080] [--scene room] [--depth 5] [--out FILE.json] [--other DIR]

Room, the bench's camera and lights, max_depth = 5, kernel time from HIP events (the stats of the host calls), median of
11 after 3 warm-ups, with the spread:
  (i)   frame_ms     the frame at max_depth (mt_render_chunk) -- what a colour edit costs without the feature.  With
                     --other DIR it is also measured with the built checkout of another commit in DIR (the parent's: the
                     yardstick), in a process of its own, in the same session.
  (ii)  create       mt_raytree_create: wall time, kernel time (first to last kernel, the per-layer round trips
                     included), and per layer its rays and its tracing kernel's time; the share of layers >= 1
  (iii) shade_ms     mt_raytree_shade: the layers' launches; with it the bytes a shade moves -- per ray it reads the
                     direction (24), point, normal, albedo (72), material and two child indices (12), per light power and
                     in_shadow (25), up to two child colours (24 each, counted by the child indices), and writes a colour
                     (24) or, in layer 0, reads a pixel index (4) and writes 3 bytes -- over the time, and that rate over
                     the HBM peak (8 TB/s spec, ~6.3 TB/s achievable)
  (iv)  bytes        the HBM the tree holds
and the number of colour edits from which the tree pays: the smallest N with create + N shade < N frame.
The required ordering is (iii) < (i).  Prints a markdown table and, with --out, writes the numbers as JSON.  Everything
printed is measured in this run; nothing is taken from an earlier one.
"""
import argparse
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC, HBM_ACHIEVABLE = 8.0e12, 6.3e12
REPS, WARM = 11, 3


def med(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


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
    abi.set_lights(h, scenegen.ROOM_LIGHTS)
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
    lights = scenegen.ROOM_LIGHTS
    n_l = len(lights)
    abi.set_lights(h, lights)
    sens = binding.sensor(scenegen.ROOM_CAMERA, W, H)
    res = dict(scene=args.scene, width=W, height=H, max_depth=D, n_lights=n_l, reps=REPS, warmups=WARM)

    t = [abi.render_chunk(h, sens, W, H, max_depth=D)["stats"]["kernel_ms"] for _ in range(REPS + WARM)]
    res["frame_ms"] = med(t[WARM:])
    frame = abi.render_chunk(h, sens, W, H, max_depth=D)["rgb"]
    if args.other:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--frame-only", "--other", args.other, "--scene",
                              args.scene, "--width", str(W), "--height", str(H), "--depth", str(D)],
                             stdout=subprocess.PIPE, timeout=600, check=True).stdout.decode()
        res["frame_other_ms"] = json.loads(out.strip().splitlines()[-1])
        res["other"] = args.other
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
    res["layer_trace_ms"] = [med([l[k] for l in layers[WARM:]]) for k in range(info["n_layers"])]
    traced = sum(m["median"] for m in res["layer_trace_ms"])
    res["share_of_layers_ge_1"] = (traced - res["layer_trace_ms"][0]["median"]) / traced
    res["bytes"] = info["bytes"]
    t = []
    for _ in range(REPS + WARM):
        r = abi.raytree_shade(tree, lights)
        t.append(r["stats"]["kernel_ms"])
    res["shade_ms"] = med(t[WARM:])
    res["shaded_equals_frame"] = bool(np.array_equal(r["rgb"], frame))
    moved = 0
    for k, n in enumerate(info["n_rays"]):
        kids = abi.raytree_read_layer(tree, k, ("child_refl", "child_refr"))
        n_kids = int((kids["child_refl"] >= 0).sum() + (kids["child_refr"] >= 0).sum())
        moved += n * (24 + 72 + 12 + 25 * n_l + (7 if k == 0 else 24)) + 24 * n_kids
    res["shade_bytes"] = moved
    res["shade_bytes_per_ray"] = moved / float(sum(info["n_rays"]))
    rate = moved / (res["shade_ms"]["median"] * 1e-3)
    res["shade_bytes_per_s"] = rate
    res["shade_share_of_hbm_spec"] = rate / HBM_SPEC
    res["shade_share_of_hbm_achievable"] = rate / HBM_ACHIEVABLE
    res["ordering_iii_below_i"] = bool(res["shade_ms"]["median"] < res["frame_ms"]["median"])
    gain = res["frame_ms"]["median"] - res["shade_ms"]["median"]
    res["pays_from_edits"] = int(math.floor(res["create_wall_ms"]["median"] / gain)) + 1 if gain > 0 else None

    f = lambda m: "%.3f (%.3f .. %.3f)" % (m["median"], m["min"], m["max"])  # noqa: E731
    print("| figure | ms, median (min .. max) of %d |" % REPS)
    print("|---|---|")
    print("| (i) frame at max_depth = %d, this build, kernels | %s |" % (D, f(res["frame_ms"])))
    if args.other:
        print("| (i) frame at max_depth = %d, the checkout in %s, kernels | %s |" % (D, args.other, f(res["frame_other_ms"])))
    print("| (ii) mt_raytree_create, wall | %s |" % f(res["create_wall_ms"]))
    print("| (ii) mt_raytree_create, first to last kernel | %s |" % f(res["create_kernel_ms"]))
    for k, m in enumerate(res["layer_trace_ms"]):
        print("| (ii) layer %d: %d rays, raytree_trace_kernel | %s |" % (k, info["n_rays"][k], f(m)))
    print("| (iii) mt_raytree_shade, kernels | %s |" % f(res["shade_ms"]))
    print("(ii): layers >= 1 take %.1f %% of the tracing kernels' time with %.1f %% of the rays"
          % (100 * res["share_of_layers_ge_1"], 100.0 * sum(info["n_rays"][1:]) / sum(info["n_rays"])))
    print("(iii): %d bytes per shade = %.1f per ray, %.3g B/s = %.1f %% of the HBM spec peak, %.1f %% of the achievable rate"
          % (moved, res["shade_bytes_per_ray"], rate, 100 * res["shade_share_of_hbm_spec"],
             100 * res["shade_share_of_hbm_achievable"]))
    print("(iv): the tree holds %d bytes (%.1f MB)" % (info["bytes"], info["bytes"] / 1e6))
    print("the tree pays from %s colour edits on (create wall + N shade < N frame); shaded frame equals the frame: %s; "
          "(iii) < (i): %s" % (res["pays_from_edits"], res["shaded_equals_frame"], res["ordering_iii_below_i"]))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    abi.raytree_destroy(tree)
    abi.scene_destroy(h)
    assert res["shaded_equals_frame"] and res["ordering_iii_below_i"]


if __name__ == "__main__":
    main()
