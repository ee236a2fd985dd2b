#!/usr/bin/env python3
"""The direct-light buffer and the relight pass: the numbers of DESIGN.md section 3.7, from one GPU session.

  python scripts/lightbuffer_numbers.py [--width 1920 --height 1080] [--scene room] [--out FILE.json] [--other DIR]

Room, the bench's camera and lights, kernel time from HIP events (the stats of the host calls), median of 11 after 3
warm-ups, with the spread:
  (i)   frame0_ms       the frame at max_depth = 0 (mt_render_chunk: primary / order kernels + frame kernel) -- what a
                        light edit costs without the feature.  With --other DIR it is also measured with the built checkout
                        of another commit in DIR (the parent's), in a process of its own, in the same session.
  (ii)  lightbuffer_ms  lightbuffer_kernel, both light-buffer planes, no G-buffer plane
  (iii) combined_ms     lightbuffer_kernel with the four G-buffer planes a relight reads
  (iv)  shade_ms        shade_direct_kernel over those planes; with it the bytes it moves (read 24 x 3 + 4 + 25 n_lights
                        per pixel, written 3) over the time, and that rate over the HBM peak (8 TB/s spec, ~6.3 TB/s
                        achievable).
The required ordering is (iv) < (i).  Prints a markdown table and, with --out, writes the numbers as JSON.  Everything
printed is measured in this run; nothing is taken from an earlier one.
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

HBM_SPEC, HBM_ACHIEVABLE = 8.0e12, 6.3e12
REPS, WARM = 11, 3


def med(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def frame0_only(args):
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
    t = [abi.render_chunk(h, sens, args.width, args.height, max_depth=0)["stats"]["kernel_ms"] for _ in range(REPS + WARM)]
    print(json.dumps(med(t[WARM:])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default="room")
    ap.add_argument("--out")
    ap.add_argument("--other", help="a built checkout of another commit (the parent's) to measure (i) with as well")
    ap.add_argument("--frame0-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.frame0_only:
        return frame0_only(args)
    from mythtracer_amd import binding, scenegen
    W, H = args.width, args.height
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
    res = dict(scene=args.scene, width=W, height=H, n_lights=n_l, reps=REPS, warmups=WARM)

    t = [abi.render_chunk(h, sens, W, H, max_depth=0)["stats"]["kernel_ms"] for _ in range(REPS + WARM)]
    res["frame0_ms"] = med(t[WARM:])
    frame = abi.render_chunk(h, sens, W, H, max_depth=0)["rgb"]
    if args.other:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--frame0-only", "--other", args.other, "--scene",
                              args.scene, "--width", str(W), "--height", str(H)], stdout=subprocess.PIPE, timeout=600,
                             check=True).stdout.decode()
        res["frame0_other_ms"] = json.loads(out.strip().splitlines()[-1])
        res["other"] = args.other
    t = [abi.render_lightbuffer(h, sens, W, H, n_l)["stats"]["kernel_ms"] for _ in range(REPS + WARM)]
    res["lightbuffer_ms"] = med(t[WARM:])
    t = []
    for _ in range(REPS + WARM):
        b = abi.render_lightbuffer(h, sens, W, H, n_l, gbuffer_channels=binding.RELIGHT_GBUFFER_PLANES)
        t.append(b["stats"]["kernel_ms"])
    res["combined_ms"] = med(t[WARM:])
    res["rays_shadow"] = int(b["stats"]["rays_shadow"])
    t = []
    for _ in range(REPS + WARM):
        r = abi.shade_direct(h, sens, W, H, b, b, lights)
        t.append(r["stats"]["kernel_ms"])
    res["shade_ms"] = med(t[WARM:])
    res["relit_equals_frame0"] = bool(np.array_equal(r["rgb"], frame))
    per_px = 24 * 3 + 4 + 25 * n_l + 3
    res["shade_bytes"] = per_px * W * H
    rate = res["shade_bytes"] / (res["shade_ms"]["median"] * 1e-3)
    res["shade_bytes_per_s"] = rate
    res["shade_share_of_hbm_spec"] = rate / HBM_SPEC
    res["shade_share_of_hbm_achievable"] = rate / HBM_ACHIEVABLE
    res["ordering_iv_below_i"] = bool(res["shade_ms"]["median"] < res["frame0_ms"]["median"])

    f = lambda m: "%.3f (%.3f .. %.3f)" % (m["median"], m["min"], m["max"])  # noqa: E731
    print("| figure | kernel ms, median (min .. max) of %d |" % REPS)
    print("|---|---|")
    print("| (i) frame at max_depth = 0, this build | %s |" % f(res["frame0_ms"]))
    if args.other:
        print("| (i) frame at max_depth = 0, the checkout in %s | %s |" % (args.other, f(res["frame0_other_ms"])))
    print("| (ii) lightbuffer_kernel | %s |" % f(res["lightbuffer_ms"]))
    print("| (iii) lightbuffer_kernel + 4 G-buffer planes | %s |" % f(res["combined_ms"]))
    print("| (iv) shade_direct_kernel | %s |" % f(res["shade_ms"]))
    print("(iv): %d bytes per frame, %.3g B/s = %.1f %% of the HBM spec peak, %.1f %% of the achievable rate"
          % (res["shade_bytes"], rate, 100 * res["shade_share_of_hbm_spec"], 100 * res["shade_share_of_hbm_achievable"]))
    print("shadow-loop iterations per frame: %d; relit frame equals the max_depth = 0 frame: %s; (iv) < (i): %s"
          % (res["rays_shadow"], res["relit_equals_frame0"], res["ordering_iv_below_i"]))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    abi.scene_destroy(h)
    assert res["relit_equals_frame0"] and res["ordering_iv_below_i"]


if __name__ == "__main__":
    main()
