#!/usr/bin/env python3
"""Adaptive supersampling: the numbers of DESIGN.md section 3.9, from one GPU session.

  python scripts/adaptive_numbers.py [--width 1920 --height 1080] [--threshold 16] [--frames 12] [--out FILE.json]

Room scene, recursion depth 5, work counters of the device calls off.  For ss = 2, 3, 4, camera at rest and turning
2 degrees per frame (the bench's pan within +-8 degrees), medians over the timed frames after 3 warm-ups:
  share        refined blocks over the chunk's blocks
  kernel_ms    mt_render_chunk_adaptive's stats (all kernels by events, the synchronisation's idle time excluded)
  wall_ms      the same call, frame to a numpy array
  plain_ms / refine_ms   the two launches of the call (mt_scene_kernel_times: work order + frame kernel each)
  other_ms     kernel_ms - plain_ms - refine_ms: mask, compaction, resolve and the gaps between the kernels
  mask_ms      refine_mask_kernel + refine_compact_kernel alone on the plain frame, HIP events, median of 30 after 5;
               bandwidth = 3 W H bytes over that time
  refine_history   share of the timed frames whose refinement launch ran on measured costs
Yardsticks of the same session, interleaved with the adaptive frames of the same camera: mt_render_chunk_ss at the
same ss and mt_render_chunk (kernel_ms and wall_ms of the host calls), and the plain launch of a repeated
mt_render_chunk next to plain_ms (the first forecast bank survives the refinement launch when the two agree).
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
    ap.add_argument("--threshold", type=int, default=16)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import mythtracer_amd as M
    from mythtracer_amd import binding, scenegen, tiling
    abi = M.hip_abi()
    W, H, T = a.width, a.height, a.threshold
    obj = scenegen.write_scene("room", tempfile.mkdtemp())["obj"]
    flat = M.MythTracer(obj).flatten()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    pan = [0, 2, 4, 6, 8, 6, 4, 2, 0, -2, -4, -6, -8, -6, -4, -2]
    warm = 3

    def cams(turning):
        out = []
        for k in range(warm + a.frames):
            cam = list(scenegen.ROOM_CAMERA)
            if turning:
                cam[4] += pan[k % len(pan)]
            out.append(cam)
        return out

    med = lambda v: float(np.median(v[warm:]))
    res = {"image": [W, H], "threshold": T, "ss": {}}
    for s in (2, 3, 4):
        res["ss"][str(s)] = {}
        for regime in ("rest", "turning"):
            # three scenes, one per call under measurement, fed the same cameras in turn: each keeps its own history
            hs = {k: abi.scene_create(flat) for k in ("adaptive", "ss", "plain")}
            for h in hs.values():
                abi.set_lights(h, scenegen.ROOM_LIGHTS)
                abi.set_stats(h, False)
            rows = {k: [] for k in ("share", "kernel", "wall", "plain", "refine", "hist", "ss_kernel", "ss_wall",
                                     "pl_kernel", "pl_wall", "pl_launch")}
            for cam in cams(regime == "turning"):
                s1, ss = binding.sensor(cam, W, H), binding.sensor(cam, s * W, s * H)
                abi.kernel_times(hs["adaptive"])
                t0 = time.perf_counter()
                r = abi.render_chunk_adaptive(hs["adaptive"], s1, ss, W, H, s, T)
                rows["wall"].append((time.perf_counter() - t0) * 1e3)
                kt = abi.kernel_times(hs["adaptive"])
                launches = kt[0] + kt[1]
                rows["plain"].append(launches[0])
                rows["refine"].append(launches[1] if len(launches) > 1 else 0.0)
                rows["kernel"].append(r["stats"]["kernel_ms"])
                rows["share"].append(r["info"]["n_refined"] / r["info"]["n_blocks"])
                rows["hist"].append(r["info"]["refine_history"])
                t0 = time.perf_counter()
                q = abi.render_chunk_ss(hs["ss"], ss, W, H, s)
                rows["ss_wall"].append((time.perf_counter() - t0) * 1e3)
                rows["ss_kernel"].append(q["stats"]["kernel_ms"])
                abi.kernel_times(hs["plain"])
                t0 = time.perf_counter()
                p = abi.render_chunk(hs["plain"], s1, W, H)
                rows["pl_wall"].append((time.perf_counter() - t0) * 1e3)
                rows["pl_kernel"].append(p["stats"]["kernel_ms"])
                kt = abi.kernel_times(hs["plain"])
                rows["pl_launch"].append((kt[0] + kt[1])[0])
            # the contract once per configuration, on the last frame's bytes
            mask, _ = tiling.refine_mask(p["rgb"], W, H, None, T)
            assert np.array_equal(r["mask"], mask)
            assert np.array_equal(r["rgb"], tiling.compose_adaptive(p["rgb"], q["rgb"], mask, (0, 0, W, H)))
            out = {"share": med(rows["share"]), "kernel_ms": med(rows["kernel"]), "wall_ms": med(rows["wall"]),
                   "plain_ms": med(rows["plain"]), "refine_ms": med(rows["refine"]),
                   "refine_history": float(np.mean(rows["hist"][warm:])),
                   "ss_kernel_ms": med(rows["ss_kernel"]), "ss_wall_ms": med(rows["ss_wall"]),
                   "plain_call_kernel_ms": med(rows["pl_kernel"]), "plain_call_wall_ms": med(rows["pl_wall"]),
                   "plain_call_launch_ms": med(rows["pl_launch"])}
            out["other_ms"] = out["kernel_ms"] - out["plain_ms"] - out["refine_ms"]
            out["kernel_speedup_over_ss"] = out["ss_kernel_ms"] / out["kernel_ms"]
            out["wall_speedup_over_ss"] = out["ss_wall_ms"] / out["wall_ms"]
            res["ss"][str(s)][regime] = out
            print(s, regime, json.dumps(out), flush=True)
            for h in hs.values():
                abi.scene_destroy(h)
    # mask + compaction alone, on the plain frame
    h = abi.scene_create(flat)
    abi.set_lights(h, scenegen.ROOM_LIGHTS)
    frame = abi.render_chunk(h, binding.sensor(scenegen.ROOM_CAMERA, W, H), W, H)["rgb"]
    d_rgb = torch.from_numpy(frame).cuda()
    _, _, mw, mh = tiling.chunk_blocks((0, 0, W, H))
    d_mask = torch.zeros(mw * mh, dtype=torch.uint8, device="cuda")
    d_list = torch.zeros(mw * mh, dtype=torch.int32, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    ts = []
    for i in range(35):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        abi.refine_mask_device(h, W, H, (0, 0, W, H), T, vp(d_rgb), vp(d_mask), vp(d_list), vp(d_count),
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    res["mask_ms"] = float(np.median(ts[5:]))
    res["mask_gbs"] = 3 * W * H / (res["mask_ms"] * 1e-3) / 1e9
    want_mask, want_list = tiling.refine_mask(frame, W, H, None, T)
    assert np.array_equal(d_mask.cpu().numpy().reshape(mh, mw), want_mask.astype(np.uint8))
    assert np.array_equal(d_list.cpu().numpy()[:int(d_count.cpu()[0])], want_list)
    abi.scene_destroy(h)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
