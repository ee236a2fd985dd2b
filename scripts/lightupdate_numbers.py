#!/usr/bin/env python3
"""The light-buffer update: the numbers of DESIGN.md section 3.8, from one GPU session.

  python scripts/lightupdate_numbers.py [--width 1920 --height 1080] [--scene room] [--out FILE.json] [--other DIR]

Room, the bench's camera and lights, kernel time from HIP events (the stats of the host calls), median of 21 after 3
warm-ups, with the spread:
  (i)   frame0_ms        the frame at max_depth = 0 (mt_render_chunk) -- what a moved light costs without the deferred path
  (ii)  lightbuffer_ms   lightbuffer_kernel, both planes -- what it cost with the deferred path before this call existed.
                         With --other DIR it is also measured with the built checkout of another commit in DIR (the
                         parent's), in a process of its own, in the same session: the kernel's text is unchanged (the
                         update kernel restates its loop), so the two figures must agree within the spread.
  (iii) update_one_ms    lightbuffer_update_kernel, light 1 moved
  (iv)  update_all_ms    lightbuffer_update_kernel, all three listed
  (v)   shade_ms         shade_direct_kernel
"Move one light, see the frame" is (iii) + (v), against (i).  Prints a markdown table and, with --out, writes the numbers
as JSON.  Everything printed is measured in this run; nothing is taken from an earlier one.
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

REPS, WARM = 21, 3


def med(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def setup(args, root=None):
    if root:
        sys.path.insert(0, os.path.abspath(root))
    from mythtracer_amd import binding, scenegen
    if root:
        assert os.path.abspath(binding.__file__).startswith(os.path.abspath(root)), binding.__file__
    abi = binding.hip_abi()
    assert abi.device_count() >= 1, "no GPU: these are measurements, there is nothing to report without one"
    with tempfile.TemporaryDirectory() as td:
        obj = scenegen.write_scene(args.scene, td)["obj"]
        flat = binding.MythTracer(obj).flatten()
    h = abi.scene_create(flat)
    lights = [tuple(float(v) for v in l) for l in scenegen.ROOM_LIGHTS]
    abi.set_lights(h, lights)
    sens = binding.sensor(scenegen.ROOM_CAMERA, args.width, args.height)
    return binding, abi, h, lights, sens


def baseline(abi, h, sens, W, H, n_l):
    """(i) and (ii): the two figures a checkout without the update can give too."""
    res = {}
    t = [abi.render_chunk(h, sens, W, H, max_depth=0)["stats"]["kernel_ms"] for _ in range(REPS + WARM)]
    res["frame0_ms"] = med(t[WARM:])
    t = [abi.render_lightbuffer(h, sens, W, H, n_l)["stats"]["kernel_ms"] for _ in range(REPS + WARM)]
    res["lightbuffer_ms"] = med(t[WARM:])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default="room")
    ap.add_argument("--out")
    ap.add_argument("--other", help="a built checkout of another commit (the parent's) to measure (i) and (ii) with as well")
    ap.add_argument("--baseline-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    W, H = args.width, args.height
    if args.baseline_only:
        _, abi, h, lights, sens = setup(args, args.other)
        print(json.dumps(baseline(abi, h, sens, W, H, len(lights))))
        return
    binding, abi, h, lights, sens = setup(args)
    n_l = len(lights)
    res = dict(scene=args.scene, width=W, height=H, n_lights=n_l, reps=REPS, warmups=WARM)
    res.update(baseline(abi, h, sens, W, H, n_l))
    if args.other:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-only", "--other", args.other, "--scene",
                              args.scene, "--width", str(W), "--height", str(H)], stdout=subprocess.PIPE, timeout=900,
                             check=True).stdout.decode()
        res["other"] = dict(json.loads(out.strip().splitlines()[-1]), path=args.other)
        res["lightbuffer_again_ms"] = baseline(abi, h, sens, W, H, n_l)["lightbuffer_ms"]  # (after the other: drift?)
    old = abi.render_lightbuffer(h, sens, W, H, n_l, gbuffer_channels=binding.RELIGHT_GBUFFER_PLANES)
    moved = list(lights)
    moved[1] = (150.0, 120.0, 250.0) + lights[1][3:]
    abi.set_lights(h, moved)
    fresh = abi.render_lightbuffer(h, sens, W, H, n_l)
    frame = abi.render_chunk(h, sens, W, H, max_depth=0)["rgb"]
    lb = dict(power=old["power"].copy(), in_shadow=old["in_shadow"].copy())
    t = [abi.update_lightbuffer(h, old, lb, [1])["stats"]["kernel_ms"] for _ in range(REPS + WARM)]
    res["update_one_ms"] = med(t[WARM:])
    res["update_equals_fresh"] = bool(np.array_equal(lb["in_shadow"], fresh["in_shadow"]) and
                                      np.array_equal(lb["power"].view(np.uint64), fresh["power"].view(np.uint64)))
    t = []
    for _ in range(REPS + WARM):
        r = abi.update_lightbuffer(h, old, lb, [0, 1, 2])
        t.append(r["stats"]["kernel_ms"])
    res["update_all_ms"] = med(t[WARM:])
    res["rays_shadow_all"] = int(r["stats"]["rays_shadow"])
    t = []
    for _ in range(REPS + WARM):
        r = abi.shade_direct(h, sens, W, H, old, lb, moved)
        t.append(r["stats"]["kernel_ms"])
    res["shade_ms"] = med(t[WARM:])
    res["relit_equals_frame0"] = bool(np.array_equal(r["rgb"], frame))
    res["move_one_light_ms"] = res["update_one_ms"]["median"] + res["shade_ms"]["median"]

    f = lambda m: "%.3f (%.3f .. %.3f)" % (m["median"], m["min"], m["max"])  # noqa: E731
    print("| figure | kernel ms, median (min .. max) of %d |" % REPS)
    print("|---|---|")
    print("| (i) frame at max_depth = 0 | %s |" % f(res["frame0_ms"]))
    print("| (ii) lightbuffer_kernel, this build | %s |" % f(res["lightbuffer_ms"]))
    if args.other:
        print("| (i) frame at max_depth = 0, the checkout in %s | %s |" % (args.other, f(res["other"]["frame0_ms"])))
        print("| (ii) lightbuffer_kernel, the checkout in %s | %s |" % (args.other, f(res["other"]["lightbuffer_ms"])))
        print("| (ii) lightbuffer_kernel, this build, measured again afterwards | %s |" % f(res["lightbuffer_again_ms"]))
    print("| (iii) lightbuffer_update_kernel, one light | %s |" % f(res["update_one_ms"]))
    print("| (iv) lightbuffer_update_kernel, all %d lights | %s |" % (n_l, f(res["update_all_ms"])))
    print("| (v) shade_direct_kernel | %s |" % f(res["shade_ms"]))
    print("move one light, see the frame: (iii) + (v) = %.3f ms against (i) %.3f ms; updated planes equal fresh ones: %s; "
          "relit frame equals the max_depth = 0 frame: %s"
          % (res["move_one_light_ms"], res["frame0_ms"]["median"], res["update_equals_fresh"], res["relit_equals_frame0"]))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    abi.scene_destroy(h)
    assert res["update_equals_fresh"] and res["relit_equals_frame0"]


if __name__ == "__main__":
    main()
