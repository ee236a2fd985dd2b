#!/usr/bin/env python3
"""The primary-hit G-buffer: the numbers of DESIGN.md section 3.6, from one GPU session.

  python scripts/gbuffer_numbers.py [--width 1920 --height 1080] [--scenes room,room_tex] [--out FILE.json]

Per scene (the bench's camera), for ALL planes and for depth only:
  kernel_ms   gbuffer_kernel alone: HIP events around mt_render_gbuffer_device into planes in HBM, work counters off,
              median of 15 after 3 warm-ups;
  call_ms     wall time of mt_render_gbuffer (host planes, allocated and touched beforehand), median of 7 after 2;
  bytes       what the kernel stores per frame (116 B per pixel for all planes, 8 for depth).
For comparison:
  primary_ms  primary_kernel for the same geometry: mt_scene_set_scheduling(0), engine 1, mt_scene_kernel_times'
              primary_ms, median of 15 after 3;
  old_ms      the route without the feature, wall time, median of 3: W x H rays built on the host, mt_intersect_rays
              (48 B per ray up; tri, line, t, point down), then normal / uvw / albedo in numpy (vectorised: the
              Heron-area weights of Triangle::GetNormal, and the bilinear fetch of Texture::GetColorAt).
Prints a markdown table and, with --out, writes the numbers as JSON.
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


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return [float(v.min()), float(v.max())]


def old_route(abi, h, flat, sens, W, H):
    """Host-built rays -> mt_intersect_rays -> numpy.  Returns the planes (depth, point, normal, uvw, albedo, prim,
    line_no, material)."""
    s = np.asarray(sens).reshape(4, 3)
    ys, xs = np.mgrid[0:H, 0:W]
    d = s[1] + s[2] * ys[..., None].astype(np.float64) + s[3] * xs[..., None].astype(np.float64)
    d = d / np.sqrt((d * d).sum(axis=-1))[..., None]
    rays = np.empty((H * W, 6))
    rays[:, :3] = s[0]
    rays[:, 3:] = d.reshape(-1, 3)
    r = abi.intersect_rays(h, rays)
    tri, P = r["tri"], r["point"]
    hit = tri >= 0
    t = np.maximum(tri, 0)
    vtx = flat["tri_vertex"][t].reshape(-1, 3, 3)
    dist = lambda a, b: np.sqrt(((b - a) ** 2).sum(axis=-1))

    def heron(a, b, c):
        p = (a + b + c) / 2.0
        q = p * (p - a) * (p - b) * (p - c)
        return np.sqrt(np.maximum(q, 0.0))
    a, b, c = dist(vtx[:, 0], vtx[:, 1]), dist(vtx[:, 1], vtx[:, 2]), dist(vtx[:, 2], vtx[:, 0])
    p0, p1, p2 = dist(P, vtx[:, 0]), dist(P, vtx[:, 1]), dist(P, vtx[:, 2])
    n0, n1, n2 = heron(b, p2, p1), heron(c, p0, p2), heron(a, p1, p0)
    n = n0 + n1 + n2

    def interp(attr):
        q = attr[t].reshape(-1, 3, 3)
        return (q[:, 0] * n0[:, None] + q[:, 1] * n1[:, None] + q[:, 2] * n2[:, None]) / n[:, None]
    normal, uvw = interp(flat["tri_normal"]), interp(flat["tri_uvw"])
    mtl = np.where(hit, flat["tri_material"][t], -1)
    amb = np.array([m["values"][0:3] for m in flat["materials"]] + [[np.nan] * 3])
    albedo = amb[mtl]
    mtex = np.array([m["tex"] for m in flat["materials"]] + [-1])[mtl]
    for ti, tex in enumerate(flat["textures"]):
        sel = np.nonzero(mtex == ti)[0]
        if not len(sel):
            continue
        tx = tex["texels"].astype(np.float64) / (255.0 if tex["texels"].dtype == np.uint8 else 1.0)
        th, tw = tx.shape[:2]
        u, v = np.fmod(uvw[sel, 0], 1.0), np.fmod(uvw[sel, 1], 1.0)
        u, v = np.where(u < 0, u + 1.0, u), 1.0 - np.where(v < 0, v + 1.0, v)
        x, y = np.nan_to_num(u * (tw - 1)), np.nan_to_num(v * (th - 1))
        bx, by = np.clip(x.astype(np.int64), 0, tw - 1), np.clip(y.astype(np.int64), 0, th - 1)
        x1, y1 = np.minimum(bx + 1, tw - 1), np.minimum(by + 1, th - 1)
        fx, fy = (x - bx)[:, None], (y - by)[:, None]
        albedo[sel] = albedo[sel] * (tx[by, bx] * (1 - fx) * (1 - fy) + tx[by, x1] * fx * (1 - fy) +
                                     tx[y1, bx] * (1 - fx) * fy + tx[y1, x1] * fx * fy)
    for plane in (normal, uvw, albedo):
        plane[~hit] = np.nan
    return dict(depth=r["t"], point=P, normal=normal, uvw=uvw, albedo=albedo,
                prim=np.where(hit, flat["tri_id"][t], -1), line_no=r["line"], material=mtl)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scenes", default="room,room_tex")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import mythtracer_amd as M
    from mythtracer_amd import binding, scenegen
    abi = M.hip_abi()
    W, H = a.width, a.height
    cam = scenegen.ROOM_CAMERA
    sens = binding.sensor(cam, W, H)
    msens = abi.make_sensor(sens)
    res = {"image": [W, H], "scenes": {}}
    sets = {"all": list(binding.GBUFFER_PLANES), "depth": ["depth"]}
    for scene in a.scenes.split(","):
        obj = scenegen.write_scene(scene, tempfile.mkdtemp())["obj"]
        flat = M.MythTracer(obj).flatten()
        h = abi.scene_create(flat)
        abi.set_lights(h, scenegen.ROOM_LIGHTS)
        r = {}
        for key, names in sets.items():
            # kernel: device planes, HIP events
            abi.set_stats(h, False)
            dev = {}
            for n in names:
                dt, k = binding.GBUFFER_PLANES[n]
                dev[n] = torch.zeros((H, W) + ((k,) if k > 1 else ()),
                                     dtype=torch.float64 if dt is np.float64 else torch.int32, device="cuda")
            ptrs = {n: t.data_ptr() for n, t in dev.items()}
            torch.cuda.synchronize()
            ms = []
            for i in range(18):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                abi.render_gbuffer_device(h, sens, W, H, (0, 0, W, H), ptrs)
                e1.record()
                torch.cuda.synchronize()
                if i >= 3:
                    ms.append(e0.elapsed_time(e1))
            del dev
            # call: host planes that exist and have been touched
            host = {}
            for n in names:
                dt, k = binding.GBUFFER_PLANES[n]
                host[n] = np.ones((H, W) + ((k,) if k > 1 else ()), dtype=dt)
            g = binding.mt_gbuffer(**{n: arr.ctypes.data for n, arr in host.items()})
            wall = []
            for i in range(9):
                t0 = time.perf_counter()
                abi.check(abi.lib.mt_render_gbuffer(h, ctypes.byref(msens), W, H, 0, 0, W, H, ctypes.byref(g), None))
                if i >= 2:
                    wall.append((time.perf_counter() - t0) * 1e3)
            px_bytes = sum(np.dtype(binding.GBUFFER_PLANES[n][0]).itemsize * binding.GBUFFER_PLANES[n][1] for n in names)
            r[key] = {"kernel_ms": median(ms), "kernel_ms_range": spread(ms), "call_ms": median(wall),
                      "call_ms_range": spread(wall), "bytes_stored": px_bytes * W * H,
                      "hits": int((host["depth"] == host["depth"]).sum())}
            del host
        # primary_kernel on the same geometry
        abi.set_stats(h, False)
        abi.set_scheduling(h, False)
        abi.set_engine(h, 1)
        out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        abi.kernel_times(h)
        for i in range(18):
            abi.render_chunk_device(h, sens, W, H, (0, 0, W, H), 5, ctypes.c_void_p(out.data_ptr()))
        torch.cuda.synchronize()
        pm, rm = abi.kernel_times(h)
        r["primary_ms"], r["primary_ms_range"] = median(pm[3:]), spread(pm[3:])
        r["frame_render_ms"] = median(rm[3:])
        abi.set_scheduling(h, True)
        abi.set_engine(h, 0)
        # the old route
        old = []
        for i in range(3):
            t0 = time.perf_counter()
            planes = old_route(abi, h, flat, sens, W, H)
            old.append((time.perf_counter() - t0) * 1e3)
        r["old_ms"], r["old_ms_range"] = median(old), spread(old)
        new = abi.render_gbuffer(h, sens, W, H)
        r["old_route_depth_equal"] = bool(np.array_equal(np.nan_to_num(planes["depth"], nan=-1.0),
                                                         np.nan_to_num(new["depth"].reshape(-1), nan=-1.0)))
        r["speedup_wall"] = r["old_ms"] / r["all"]["call_ms"]
        res["scenes"][scene] = r
        abi.scene_destroy(h)
    print("| scene | planes | kernel ms (min..max) | call ms (min..max) | stored MB | primary_kernel ms | old route ms | old / call |")
    print("|---|---|---|---|---|---|---|---|")
    for scene, r in res["scenes"].items():
        for key in ("all", "depth"):
            q = r[key]
            print("| %s | %s | %.3f (%.3f..%.3f) | %.1f (%.1f..%.1f) | %.1f | %.3f (%.3f..%.3f) | %s | %s |" % (
                scene, key, q["kernel_ms"], *q["kernel_ms_range"], q["call_ms"], *q["call_ms_range"],
                q["bytes_stored"] / 1e6, r["primary_ms"], *r["primary_ms_range"],
                "%.0f (%.0f..%.0f)" % (r["old_ms"], *r["old_ms_range"]) if key == "all" else "",
                "%.1f" % r["speedup_wall"] if key == "all" else ""))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
