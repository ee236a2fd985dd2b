#!/usr/bin/env python3
"""Supersampled frames: the numbers of DESIGN.md's section on them, from one GPU session.

  python scripts/ss_numbers.py [--width 1920 --height 1080] [--out FILE.json]

Room scene, recursion depth 5, work counters of the device calls off, for s = 1 .. 4:
  render_ms   the sample frame's kernel (mt_scene_kernel_times), camera at rest and turning 2 degrees per frame
              (the bench's pan within +-8 degrees), median over the timed frames, next to s*s x the s = 1 figure;
  resolve     resolve_kernel alone, HIP events around mt_resolve_tiles_device for the frame as one tile, median of 30
              after 5 warm-ups: once over the same sample buffer (it fits the Infinity Cache for small s) and once
              rotating through >= 1 GB of sample buffers (HBM); bandwidth = (3 s*s + 3) W H bytes over that time;
  wall        mt_render_chunk_ss (frame to a numpy array) against the path it replaces: mt_render_chunk at s W x s H
              plus tiling.resolve_ss in numpy on the host; camera at rest, median of 7 after 3 warm-ups.
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import mythtracer_amd as M
    from mythtracer_amd import binding, scenegen, tiling
    abi = M.hip_abi()
    W, H = a.width, a.height
    obj = scenegen.write_scene("room", tempfile.mkdtemp())["obj"]
    h = abi.scene_create(M.MythTracer(obj).flatten())
    abi.set_lights(h, scenegen.ROOM_LIGHTS)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    pan = [0, 2, 4, 6, 8, 6, 4, 2, 0, -2, -4, -6, -8, -6, -4, -2]
    res = {"image": [W, H], "s": {}}
    for s in (1, 2, 3, 4):
        r = {}
        out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        abi.set_stats(h, False)

        def frames(cams):
            abi.kernel_times(h)
            for cam in cams:
                abi.render_chunk_ss_device(h, binding.sensor(cam, s * W, s * H), W, H, (0, 0, W, H), s, 5, vp(out))
            torch.cuda.synchronize()
            return abi.kernel_times(h)[1]

        rest = [scenegen.ROOM_CAMERA] * 13
        turning = []
        for k in range(3 + 16):
            cam = list(scenegen.ROOM_CAMERA)
            cam[4] += pan[k % len(pan)]
            turning.append(cam)
        r["render_ms_rest"] = float(np.median(frames(rest)[3:]))
        r["render_ms_turning"] = float(np.median(frames(turning)[3:]))
        abi.set_stats(h, True)
        if s > 1:
            n_bytes = 3 * s * s * W * H
            n_buf = max(2, -(-(1 << 30) // n_bytes))
            bufs = [torch.randint(0, 256, (n_bytes,), dtype=torch.uint8, device="cuda") for _ in range(n_buf)]
            for name, pick in (("resolve_ms_same_buffer", lambda i: bufs[0]), ("resolve_ms_rotating", lambda i: bufs[i % n_buf])):
                ts = []
                for i in range(35):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    abi.resolve_tiles_device(h, W, H, W, H, 0, 1, None, 1, s, vp(pick(i)), vp(out),
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1))
                r[name] = float(np.median(ts[5:]))
                r[name.replace("_ms_", "_gbs_")] = (3 * s * s + 3) * W * H / (r[name] * 1e-3) / 1e9
            want = tiling.resolve_ss(bufs[0].cpu().numpy().reshape(s * H, s * W, 3), s)
            abi.resolve_tiles_device(h, W, H, W, H, 0, 1, None, 1, s, vp(bufs[0]), vp(out))
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want), "resolve differs from tiling.resolve_ss"
            del bufs
            sens = binding.sensor(scenegen.ROOM_CAMERA, s * W, s * H)
            t_ss, t_diy = [], []
            for i in range(10):
                t0 = time.perf_counter()
                got = abi.render_chunk_ss(h, sens, W, H, s)["rgb"]
                t1 = time.perf_counter()
                diy = tiling.resolve_ss(abi.render_chunk(h, sens, s * W, s * H)["rgb"], s)
                t2 = time.perf_counter()
                assert np.array_equal(got, diy)
                t_ss.append((t1 - t0) * 1e3)
                t_diy.append((t2 - t1) * 1e3)
            r["wall_ms_render_chunk_ss"] = float(np.median(t_ss[3:]))
            r["wall_ms_render_chunk_plus_numpy"] = float(np.median(t_diy[3:]))
            r["wall_ratio"] = r["wall_ms_render_chunk_plus_numpy"] / r["wall_ms_render_chunk_ss"]
        res["s"][str(s)] = r
        print(s, json.dumps(r), flush=True)
    one = res["s"]["1"]
    for s in (2, 3, 4):
        r = res["s"][str(s)]
        for regime in ("rest", "turning"):
            r["render_over_s2_x_one_sample_" + regime] = r["render_ms_" + regime] / (s * s * one["render_ms_" + regime])
    abi.scene_destroy(h)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
