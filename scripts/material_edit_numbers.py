#!/usr/bin/env python3
"""Material edits in place: the numbers of DESIGN.md section 3.13, from one GPU session.

  python scripts/material_edit_numbers.py [--width 1920 --height 1080] [--scene room] [--depth 5] [--out FILE.json]
                                          [--other DIR]

Room, the bench's camera and lights, max_depth = 5; median of 11 after 3 warm-ups, with the spread.  Kernel times are HIP
events (the stats of the host calls), wall times the calls' own total_ms or, where a call reports none, a clock around
the call.  Three edits of the room's .mtl, each a scene BUILT with the edited text whose flat material table is handed
to mt_scene_set_materials:
  colour      blue Ka 0.9 0.5 0.25; red Kd 0.2 0.3 0.9, Ks 0.5 0.5 0.5, Ns 12    (albedo: the commit alone)
  mirror 0.5  mirror Refl 0.6 -> 0.5                                              (the check pass + the commit of coef)
  glass Tr    glass Tr 0.8 -> 0.5                                                 (check, commit, all lights re-traced)
  (0)   the only route without these calls: mt_scene_create with the edited materials + the first frame, and + a new
        mt_raytree_create.  With --other DIR it is measured with the built checkout of another commit in DIR (the
        parent's: the yardstick) in a process of its own, otherwise with this tree (the same code path).
  (i)   mt_scene_set_materials, wall
  (ii)  mt_raytree_update_materials per edit: kernel and wall.  The check pass and the commit are not timed apart: the
        colour edit runs the commit alone, mirror 0.5 the check and the commit.
  (iii) mt_raytree_shade after each edit
  (iv)  the frame under B (mt_render_chunk at max_depth), per edit
Each updated tree must shade to the frame under B: checked.  Prints a markdown table and, with --out, writes the numbers
as JSON.  Everything printed is measured in this run; nothing is taken from an earlier one.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM = 11, 3
EDITS = {
    "colour": [("blue", "Ka", "0.9 0.5 0.25"), ("red", "Kd", "0.2 0.3 0.9"), ("red", "Ks", "0.5 0.5 0.5"), ("red", "Ns", "12")],
    "mirror 0.5": [("mirror", "Refl", "0.5")],
    "glass Tr": [("glass", "Tr", "0.5")],
}


def med(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def edited_mtl(text, edits):
    """The .mtl text with the keyword's line of the named material's block replaced."""
    for name, key, value in edits:
        pat = re.compile(r"(newmtl %s\n(?:(?!newmtl ).*\n)*?)%s .*\n" % (re.escape(name), re.escape(key)))
        text, n = pat.subn(lambda m: "%s%s %s\n" % (m.group(1), key, value), text, count=1)
        assert n == 1, (name, key)
    return text


def tables(binding, scenegen, scene):
    """The flat scene, and per edit the flat material table of the scene built with the edited .mtl."""
    out = {}
    with tempfile.TemporaryDirectory() as td:
        obj = scenegen.write_scene(scene, td)["obj"]
        flat = binding.MythTracer(obj).flatten()
        mtl = open(os.path.join(td, scene + ".mtl")).read()
        for name, edits in EDITS.items():
            with open(os.path.join(td, scene + ".mtl"), "w", newline="\n") as f:
                f.write(edited_mtl(mtl, edits))
            out[name] = binding.MythTracer(obj).flatten()["materials"]
    return flat, out


def route(binding, scenegen, args):
    """(0): per repetition a new scene with the edited materials, its first frame, a new tree."""
    abi = binding.hip_abi()
    flat, tabs = tables(binding, scenegen, args.scene)
    flat = dict(flat, materials=tabs["mirror 0.5"])
    sens = binding.sensor(scenegen.ROOM_CAMERA, args.width, args.height)
    create, frame_k, frame_w, tree_k, tree_w, all_w = [], [], [], [], [], []
    for _ in range(REPS + WARM):
        t0 = time.perf_counter()
        h = abi.scene_create(flat)
        t1 = time.perf_counter()
        abi.set_lights(h, scenegen.ROOM_LIGHTS)
        st = abi.render_chunk(h, sens, args.width, args.height, max_depth=args.depth)["stats"]
        t2 = time.perf_counter()
        tree, ts = abi.raytree_create(h, sens, args.width, args.height, max_depth=args.depth)
        t3 = time.perf_counter()
        abi.raytree_destroy(tree)
        abi.scene_destroy(h)
        create.append((t1 - t0) * 1e3)
        frame_k.append(st["kernel_ms"])
        frame_w.append((t2 - t1) * 1e3)
        tree_k.append(ts["kernel_ms"])
        tree_w.append((t3 - t2) * 1e3)
        all_w.append((t3 - t0) * 1e3)
    return dict(scene_create_wall_ms=med(create[WARM:]), first_frame_kernel_ms=med(frame_k[WARM:]),
                first_frame_wall_ms=med(frame_w[WARM:]), tree_kernel_ms=med(tree_k[WARM:]), tree_wall_ms=med(tree_w[WARM:]),
                create_frame_wall_ms=med(np.array(create[WARM:]) + np.array(frame_w[WARM:])), route_wall_ms=med(all_w[WARM:]))


def route_only(args):
    sys.path.insert(0, os.path.abspath(args.other))
    from mythtracer_amd import binding, scenegen
    assert os.path.abspath(binding.__file__).startswith(os.path.abspath(args.other)), binding.__file__
    print(json.dumps(route(binding, scenegen, args)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default="room")
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--other", help="a built checkout of another commit (the parent's) to measure (0) with")
    ap.add_argument("--route-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.route_only:
        return route_only(args)
    from mythtracer_amd import binding, scenegen
    W, H, D = args.width, args.height, args.depth
    abi = binding.hip_abi()
    assert abi.device_count() >= 1, "no GPU: these are measurements, there is nothing to report without one"
    res = dict(scene=args.scene, width=W, height=H, max_depth=D, reps=REPS, warmups=WARM)
    if args.other:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--route-only", "--other", args.other, "--scene",
                              args.scene, "--width", str(W), "--height", str(H), "--depth", str(D)],
                             stdout=subprocess.PIPE, timeout=900, check=True).stdout.decode()
        res["route"] = json.loads(out.strip().splitlines()[-1])
        res["route_by"] = args.other
    else:
        res["route"] = route(binding, scenegen, args)
        res["route_by"] = "this tree"
    flat, tabs = tables(binding, scenegen, args.scene)
    A = flat["materials"]
    h = abi.scene_create(flat)
    lights = [tuple(float(v) for v in l) for l in scenegen.ROOM_LIGHTS]
    abi.set_lights(h, lights)
    sens = binding.sensor(scenegen.ROOM_CAMERA, W, H)
    tree, _ = abi.raytree_create(h, sens, W, H, max_depth=D)
    res["n_rays"] = abi.raytree_info(tree)["n_rays"]
    set_wall = []
    res["edits"] = {}
    for name, B in tabs.items():
        up_k, up_w, sh, fr = [], [], [], []
        shadow = 0
        for _ in range(REPS + WARM):
            abi.set_materials(h, A)
            abi.raytree_update_materials(tree)
            t0 = time.perf_counter()
            abi.set_materials(h, B)
            set_wall.append((time.perf_counter() - t0) * 1e3)
            st = abi.raytree_update_materials(tree)
            up_k.append(st["kernel_ms"])
            up_w.append(st["total_ms"])
            shadow = st["rays_shadow"]
            r = abi.raytree_shade(tree, lights)
            sh.append(r["stats"]["kernel_ms"])
            f = abi.render_chunk(h, sens, W, H, max_depth=D)
            fr.append(f["stats"]["kernel_ms"])
        same = bool(np.array_equal(r["rgb"], f["rgb"]))
        res["edits"][name] = dict(update_kernel_ms=med(up_k[WARM:]), update_wall_ms=med(up_w[WARM:]), shade_ms=med(sh[WARM:]),
                                  frame_ms=med(fr[WARM:]), rays_shadow=shadow, updated_tree_shades_to_the_frame=same)
    res["set_materials_wall_ms"] = med(set_wall[WARM:])

    f = lambda m: "%.3f (%.3f .. %.3f)" % (m["median"], m["min"], m["max"])  # noqa: E731
    R = res["route"]
    print("| figure | ms, median (min .. max) of %d |" % REPS)
    print("|---|---|")
    print("| (0) mt_scene_create with the edited materials, wall (%s) | %s |" % (res["route_by"], f(R["scene_create_wall_ms"])))
    print("| (0) its first frame, kernels / wall | %s / %s |" % (f(R["first_frame_kernel_ms"]), f(R["first_frame_wall_ms"])))
    print("| (0) mt_scene_create + first frame, wall | %s |" % f(R["create_frame_wall_ms"]))
    print("| (0) + mt_raytree_create, kernels / wall | %s / %s |" % (f(R["tree_kernel_ms"]), f(R["tree_wall_ms"])))
    print("| (0) the whole route, wall | %s |" % f(R["route_wall_ms"]))
    print("| (i) mt_scene_set_materials, wall | %s |" % f(res["set_materials_wall_ms"]))
    for name, e in res["edits"].items():
        print("| (ii) mt_raytree_update_materials, %s, kernels / wall | %s / %s |" % (name, f(e["update_kernel_ms"]), f(e["update_wall_ms"])))
        print("| (iii) mt_raytree_shade after it | %s |" % f(e["shade_ms"]))
        print("| (iv) the frame under B, kernels | %s |" % f(e["frame_ms"]))
    for name, e in res["edits"].items():
        print("%s: %d shadow-loop iterations; the updated tree shades to the frame under B: %s"
              % (name, e["rays_shadow"], e["updated_tree_shades_to_the_frame"]))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    abi.raytree_destroy(tree)
    abi.scene_destroy(h)
    assert all(e["updated_tree_shades_to_the_frame"] for e in res["edits"].values())


if __name__ == "__main__":
    main()
