#!/usr/bin/env python3
"""Regrowing a stored ray tree after a shape-changing material edit: the numbers of DESIGN.md section 3.14, from one GPU
session.

  python scripts/regrow_numbers.py [--width 1920 --height 1080] [--scene room] [--depth 5] [--out FILE.json]

Room, the bench's camera and lights, max_depth = 5; median of 11 after 3 warm-ups, with the spread.  Kernel times are HIP
events (the stats of the host calls), wall times the calls' own total_ms plus, for the yardstick, a clock around
mt_scene_set_materials.  Three edits of the room's .mtl, each a scene BUILT with the edited text whose flat material
table is handed to mt_scene_set_materials:
  grow         red Refl 0 -> 0.3      (a matte wall made reflective: new subtrees are traced)
  drop         mirror Refl 0.6 -> 0   (the mirror switched off: subtrees are dropped, no ray is traced)
  drop+shadow  glass Tr 0.8 -> 0      (the pane made opaque: subtrees dropped, all lights re-traced over the new tree)
Per edit, A -> B and the way back B -> A (the reverse swaps traced and dropped), each against the only route without the
call: mt_scene_set_materials + a new mt_raytree_create on the same scene, timed in the same session -- never against the
call itself.  The share of a regrow's device time that is not a tracing launch (flags, the one-workgroup compactions,
link, copy, gather, scatter and the read-backs between them) is kernel_ms minus the sum of mt_raytree_info's trace_ms;
the compaction is not timed apart.  Each regrown tree must shade to the frame under the new materials: checked.  Prints a
markdown table and, with --out, writes the numbers as JSON.  Everything printed is measured in this run.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from material_edit_numbers import edited_mtl, med  # noqa: E402

REPS, WARM = 11, 3
EDITS = {
    "grow (red Refl 0.3)": [("red", "Kd", None, "Refl 0.3")],
    "drop (mirror Refl 0)": [("mirror", "Refl", "0", None)],
    "drop + shadow (glass Tr 0)": [("glass", "Tr", "0", None)],
}


def tables(binding, scenegen, scene):
    """The flat scene, and per edit the flat material table of the scene built with the edited .mtl."""
    out = {}
    with tempfile.TemporaryDirectory() as td:
        obj = scenegen.write_scene(scene, td)["obj"]
        flat = binding.MythTracer(obj).flatten()
        path = os.path.join(td, scene + ".mtl")
        mtl = open(path).read()
        for name, edits in EDITS.items():
            text = mtl
            for material, key, value, new_line in edits:
                if new_line is None:
                    text = edited_mtl(text, [(material, key, value)])
                else:  # the material has no such line: one more after its `key` line
                    head = "newmtl %s\n" % material
                    at = text.index(head)
                    end = text.index("\n", text.index("\n" + key + " ", at) + 1) + 1
                    text = text[:end] + new_line + "\n" + text[end:]
            with open(path, "w", newline="\n") as f:
                f.write(text)
            out[name] = binding.MythTracer(obj).flatten()["materials"]
    return flat, out


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
    res = dict(scene=args.scene, width=W, height=H, max_depth=D, reps=REPS, warmups=WARM)
    flat, tabs = tables(binding, scenegen, args.scene)
    A = flat["materials"]
    h = abi.scene_create(flat)
    lights = [tuple(float(v) for v in l) for l in scenegen.ROOM_LIGHTS]
    abi.set_lights(h, lights)
    sens = binding.sensor(scenegen.ROOM_CAMERA, W, H)
    tree, _ = abi.raytree_create(h, sens, W, H, max_depth=D)
    res["n_rays"] = abi.raytree_info(tree)["n_rays"]
    res["edits"] = {}
    for name, B in tabs.items():
        rows = {}
        for direction, mats in (("A -> B", B), ("B -> A", A)):
            rows[direction] = dict(k=[], w=[], rest=[], create_k=[], create_w=[])
        same = True
        for rep in range(REPS + WARM):
            for direction, mats in (("A -> B", B), ("B -> A", A)):
                r = rows[direction]
                abi.set_materials(h, mats)
                out = abi.raytree_regrow(tree)
                info = abi.raytree_info(tree)
                r["k"].append(out["kernel_ms"])
                r["w"].append(out["total_ms"])
                r["rest"].append(out["kernel_ms"] - sum(info["trace_ms"]))
                r["out"] = out
                r["n_rays"] = info["n_rays"]
                r["trace_ms"] = info["trace_ms"]
                # the yardstick: the same materials set again from the other table, and a new tree
                abi.set_materials(h, A if mats is B else B)
                t0 = time.perf_counter()
                abi.set_materials(h, mats)
                t1 = time.perf_counter()
                fresh, st = abi.raytree_create(h, sens, W, H, max_depth=D)
                r["create_k"].append(st["kernel_ms"])
                r["create_w"].append(st["total_ms"] + (t1 - t0) * 1e3)
                # (the generation moved twice with nothing changed in between: the tree is stale, and has nothing to take)
                assert abi.raytree_regrow(tree)["regrown"] == 0
                if rep == REPS + WARM - 1:
                    rgb = abi.raytree_shade(tree, lights)["rgb"]
                    frame = abi.render_chunk(h, sens, W, H, max_depth=D)["rgb"]
                    same = same and bool(np.array_equal(rgb, frame))
                    same = same and abi.raytree_info(fresh)["n_rays"] == info["n_rays"]
                abi.raytree_destroy(fresh)
        res["edits"][name] = {
            d: dict(regrow_kernel_ms=med(r["k"][WARM:]), regrow_wall_ms=med(r["w"][WARM:]),
                    not_tracing_ms=med(r["rest"][WARM:]), create_kernel_ms=med(r["create_k"][WARM:]),
                    set_and_create_wall_ms=med(r["create_w"][WARM:]), regrown=r["out"]["regrown"],
                    kept=sum(r["out"]["kept"]), traced=sum(r["out"]["traced"]), dropped=sum(r["out"]["dropped"]),
                    rays_shadow=r["out"]["rays_shadow"], n_rays=r["n_rays"], traced_per_layer=r["out"]["traced"],
                    trace_ms_last_run=r["trace_ms"])
            for d, r in rows.items()}
        res["edits"][name]["regrown_tree_shades_to_the_frame"] = same

    f = lambda m: "%.3f (%.3f .. %.3f)" % (m["median"], m["min"], m["max"])  # noqa: E731
    print("tree under A: rays per layer", res["n_rays"])
    print("| edit | kept / traced / dropped | regrow, kernels | regrow, wall | of the kernels: not a tracing launch "
          "| set_materials + mt_raytree_create, kernels | ... wall |")
    print("|---|---|---|---|---|---|---|")
    for name, e in res["edits"].items():
        for d in ("A -> B", "B -> A"):
            r = e[d]
            print("| %s, %s | %d / %d / %d | %s | %s | %s | %s | %s |"
                  % (name, d, r["kept"], r["traced"], r["dropped"], f(r["regrow_kernel_ms"]), f(r["regrow_wall_ms"]),
                     f(r["not_tracing_ms"]), f(r["create_kernel_ms"]), f(r["set_and_create_wall_ms"])))
    for name, e in res["edits"].items():
        print("%s: rays per layer under B %s, %d shadow-loop iterations; the regrown trees shade to the frame: %s"
              % (name, e["A -> B"]["n_rays"], e["A -> B"]["rays_shadow"], e["regrown_tree_shades_to_the_frame"]))
    for name, e in res["edits"].items():
        for d in ("A -> B", "B -> A"):
            print("%s, %s: traced per layer %s, their tracing launches (last run) %s ms"
                  % (name, d, e[d]["traced_per_layer"], ["%.3f" % v for v in e[d]["trace_ms_last_run"]]))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    abi.raytree_destroy(tree)
    abi.scene_destroy(h)
    assert all(e["regrown_tree_shades_to_the_frame"] for e in res["edits"].values())
    assert all(e[d]["regrown"] == 1 for e in res["edits"].values() for d in ("A -> B", "B -> A"))


if __name__ == "__main__":
    main()
