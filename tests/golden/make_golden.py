#!/usr/bin/env python3
"""Generates the golden vectors under tests/golden/ by running the REFERENCE
ITSELF (oracle/_ref/ref_driver, compiled from /root/reference/VerStarting by
oracle/Makefile).  Run in the build container only:

    make -C oracle ref && python tests/golden/make_golden.py [--big | --big4k]

Outputs are data only (inputs + what the reference returned): .npz archives
(numpy, no pickle) and frames.json.  --big also renders the BASELINE-sized
frames (about two minutes of CPU).
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orclib  # noqa: E402
from mythtracer_amd import scenegen  # noqa: E402
import quirk_files  # noqa: E402

CORNELL = os.path.join(ROOT, "tests", "scenes", "cornell_n.obj")
CORNELL_CAM = (50, 50, -120, 0, 0, 0, 60)
CORNELL_LIGHTS = [(50, 90, 50, .3, .3, .3, 1, 1, 1, 1, 1, 1)]
# second camera: inside the box, rolled and pitched, two lights
CORNELL_CAM2 = (20, 70, 10, 25, 35, 10, 95)
# a pane of glass with an opaque decal 5e-6 above it (tests/scenes/f2_decal.obj): the shadow loop crosses the
# pane and restarts 1.01e-5 further on (mythtracer.cc:137, :95-99) -- BEYOND the decal, which it never sees
F2_DECAL = os.path.join(ROOT, "tests", "scenes", "f2_decal.obj")
F2_CAM = (50.0, 6.0, -30.0, 12.0, 0.0, 0.0, 70.0)
F2_LIGHTS = [(50.0, 60.0, 50.0, .1, .1, .1, 1, 1, 1, 0, 0, 0)]
CORNELL_LIGHTS2 = [(50, 90, 50, .2, .2, .2, .8, .8, .8, 1, 1, 1), (10, 20, 90, 0, 0, .1, .3, .3, .6, .2, .2, .2)]


ROOM_VIEWS = [
    ("room_view_back", (330.0, 60.0, 380.0, -5.0, 200.0, 0.0, 90.0), scenegen.ROOM_LIGHTS),
    ("room_view_floor", (40.0, 15.0, 200.0, 8.0, 90.0, 12.0, 100.0), scenegen.ROOM_LIGHTS),
    ("room_view_down", (200.0, 240.0, 200.0, 88.0, 30.0, 0.0, 80.0), scenegen.ROOM_LIGHTS[:2]),
    ("room_view_axis", (200.0, 125.0, 5.0, 0.0, 0.0, 0.0, 70.0), scenegen.ROOM_LIGHTS),
]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def render_case(td, name, obj, W, H, cam, lights, chunk=None):
    r = orclib.run_ref(os.path.join(td, name), obj, (W, H), chunk=chunk, cam=cam, lights=lights,
                       want_debug=True)
    assert r["returncode"] == 0, r["stderr"]
    np.savez_compressed(os.path.join(HERE, name + ".npz"), rgb=r["rgb"], line=r["line"],
                        point=r["point"], cam=np.array(cam, dtype=np.float64),
                        lights=np.array(lights, dtype=np.float64),
                        image=np.array([W, H], dtype=np.int32),
                        chunk=np.array(chunk if chunk else (0, 0, W, H), dtype=np.int32))
    print(name, r["rgb"].shape, sha(r["rgb"]))
    return r


def random_rays(seed, n, lo, hi):
    rnd = scenegen.SplitMix64(seed)
    rays = np.zeros((n, 6))
    for i in range(n):
        o = [rnd.rng(lo[k] - 30, hi[k] + 30) for k in range(3)]
        t = [rnd.rng(lo[k], hi[k]) for k in range(3)]
        d = np.array(t) - np.array(o)
        d /= np.sqrt((d * d).sum())
        rays[i, :3], rays[i, 3:] = o, d
    return rays


def special_rays():
    """Axis-parallel directions (1/0 = inf), origins on box planes (0*inf = NaN),
    negative zero components, rays starting inside, rays pointing away."""
    rays = []
    for o in [(50, 50, -120), (50, 50, 50), (0, 50, 50), (100, 100, 100), (50, 0, 50), (30, 1, 30),
              (50, 50, 200), (-10, -10, -10), (50, 1, 50), (70, 1, 70)]:
        for d in [(0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0),
                  (0.0, 0.6, 0.8), (-0.0, 0.6, 0.8), (0.6, -0.0, 0.8), (0.6, 0.8, 0.0),
                  (0.6, 0.8, -0.0), (-0.6, 0.0, -0.8)]:
            rays.append(o + d)
    return np.array(rays, dtype=np.float64)


def ray_case(td, name, obj, rays):
    r = orclib.run_ref(os.path.join(td, name), obj, rays=rays)
    assert r["returncode"] == 0, r["stderr"]
    out = r["rays"]
    np.savez_compressed(os.path.join(HERE, name + ".npz"), rays=rays, line=out["line"], t=out["t"],
                        point=out["point"], normal=out["normal"], uvw=out["uvw"])
    print(name, len(rays), "rays,", int((out["line"] >= 0).sum()), "hits")


def sensor_case(td):
    cams = [CORNELL_CAM, CORNELL_CAM2, scenegen.ROOM_CAMERA, (300.0, 107.0, 40.0, 30.0, 214.0, 0.0, 110.0),
            (1.5, -2.25, 3.0, -90.0, 180.0, 45.0, 60.0)]
    sizes = [(256, 256), (320, 180), (1920, 1080), (480, 270), (7, 5)]
    out = {}
    for i, (cam, (W, H)) in enumerate(zip(cams, sizes)):
        # corners + centre + a few interior pixels, as 1x1 chunks
        pix = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2), (W // 3, (2 * H) // 3)]
        dirs = []
        for (x, y) in pix:
            r = orclib.run_ref(os.path.join(td, "sensor"), CORNELL, (W, H), chunk=(x, y, 1, 1), cam=cam,
                               want_rgb=False, want_sensor=True)
            assert r["returncode"] == 0, r["stderr"]
            dirs.append(r["sensor"][0, 0])
        out["cam%d" % i] = np.array(cam, dtype=np.float64)
        out["size%d" % i] = np.array([W, H], dtype=np.int32)
        out["pix%d" % i] = np.array(pix, dtype=np.int32)
        out["dir%d" % i] = np.array(dirs)
    np.savez_compressed(os.path.join(HERE, "sensor_rays.npz"), **out)
    print("sensor_rays", len(cams), "cameras")


def quirk_cases(td):
    """OBJ/MTL parser behaviours: for each small file, does LoadObj succeed and
    what does a 24x24 render (with first-hit line numbers) look like."""
    qdir = os.path.join(ROOT, "tests", "scenes", "quirks")
    quirk_files.write_all(qdir)
    res = {}
    for name in quirk_files.NAMES:
        obj = os.path.join(qdir, name + ".obj")
        r = orclib.run_ref(os.path.join(td, "q_" + name), obj, (24, 24), cam=quirk_files.CAM,
                           lights=quirk_files.LIGHTS, want_debug=True)
        ok = r["returncode"] == 0
        res["ok_" + name] = np.array([1 if ok else 0], dtype=np.int32)
        if ok:
            res["rgb_" + name] = r["rgb"]
            res["line_" + name] = r["line"]
        print("quirk", name, "loads" if ok else "FAILS to load",
              "" if not ok else "lines hit: %s" % sorted(set(r["line"].reshape(-1).tolist())))
    np.savez_compressed(os.path.join(HERE, "obj_quirks.npz"), **res)


def big_frames(td):
    scenes = os.path.join(td, "scenes")
    frames = {}
    fpath = os.path.join(HERE, "frames.json")
    if os.path.exists(fpath):
        frames = json.load(open(fpath))
    for name, (W, H) in [("room_nomtl", (1280, 720)), ("room", (1920, 1080))]:
        info = scenegen.write_scene(name, scenes)
        r = orclib.run_ref(os.path.join(td, name + "_big"), info["obj"], (W, H), cam=scenegen.ROOM_CAMERA,
                           lights=scenegen.ROOM_LIGHTS, want_debug=True)
        assert r["returncode"] == 0, r["stderr"]
        key = "%s_%dx%d_d5" % (name, W, H)
        frames[key] = {"sha256": sha(r["rgb"]), "line_sha256": sha(r["line"].astype("<i4")),
                       "seconds_reference_here": r["time"]["seconds"], "threads": r["time"]["threads"],
                       "scene_sha256": info["sha256"]}
        np.savez_compressed(os.path.join(HERE, key + "_sub16.npz"), rgb=r["rgb"][::16, ::16],
                            line=r["line"][::16, ::16], point=r["point"][::16, ::16])
        print(key, frames[key])
    # two more full-size frames from other views (camera and lights recorded with the hash)
    for name, cam, lights in ROOM_VIEWS[:2]:
        info = scenegen.write_scene("room", scenes)
        W, H = 1920, 1080
        r = orclib.run_ref(os.path.join(td, name + "_big"), info["obj"], (W, H), cam=cam, lights=lights,
                           want_debug=True)
        assert r["returncode"] == 0, r["stderr"]
        key = "%s_%dx%d_d5" % (name, W, H)
        frames[key] = {"sha256": sha(r["rgb"]), "line_sha256": sha(r["line"].astype("<i4")),
                       "seconds_reference_here": r["time"]["seconds"], "threads": r["time"]["threads"],
                       "scene_sha256": info["sha256"], "cam": list(cam), "lights": [list(l) for l in lights]}
        print(key, frames[key]["sha256"], frames[key]["seconds_reference_here"])
    json.dump(frames, open(fpath, "w"), indent=1, sort_keys=True)


def big4k_frame(td):
    """BASELINE configs[4]'s frame (3840x2160, room, 3 lights, depth 5) rendered ONCE by the compiled reference
    (about four minutes on 8 threads): SHA-256 of frame and first-hit buffer + every 16th pixel."""
    scenes = os.path.join(td, "scenes")
    fpath = os.path.join(HERE, "frames.json")
    frames = json.load(open(fpath))
    info = scenegen.write_scene("room", scenes)
    W, H = 3840, 2160
    r = orclib.run_ref(os.path.join(td, "room_4k"), info["obj"], (W, H), cam=scenegen.ROOM_CAMERA,
                       lights=scenegen.ROOM_LIGHTS, want_debug=True)
    assert r["returncode"] == 0, r["stderr"]
    key = "room_%dx%d_d5" % (W, H)
    frames[key] = {"sha256": sha(r["rgb"]), "line_sha256": sha(r["line"].astype("<i4")),
                   "seconds_reference_here": r["time"]["seconds"], "threads": r["time"]["threads"],
                   "scene_sha256": info["sha256"]}
    np.savez_compressed(os.path.join(HERE, key + "_sub16.npz"), rgb=r["rgb"][::16, ::16],
                        line=r["line"][::16, ::16], point=r["point"][::16, ::16])
    # odd pixels only (the even ones are the 1080p frame's): a second sub-sample, offset (5, 11), every 16th
    np.savez_compressed(os.path.join(HERE, key + "_sub16_odd.npz"), rgb=r["rgb"][11::16, 5::16],
                        line=r["line"][11::16, 5::16], point=r["point"][11::16, 5::16])
    json.dump(frames, open(fpath, "w"), indent=1, sort_keys=True)
    print(key, frames[key])


def parse_tree_dump(raw: bytes):
    """ref_driver's `tree` dump -> arrays (see oracle/ref_driver.cc)."""
    n = int(np.frombuffer(raw, dtype="<i4", count=1)[0])
    off = 4
    aabb, center = np.zeros((n, 6)), np.zeros((n, 3))
    has_children, n_prims = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    lines = []
    for i in range(n):
        aabb[i] = np.frombuffer(raw, dtype="<f8", count=6, offset=off)
        center[i] = np.frombuffer(raw, dtype="<f8", count=3, offset=off + 48)
        has_children[i], n_prims[i] = np.frombuffer(raw, dtype="<i4", count=2, offset=off + 72)
        off += 80
        lines.append(np.frombuffer(raw, dtype="<i4", count=int(n_prims[i]), offset=off))
        off += 4 * int(n_prims[i])
    assert off == len(raw)
    return dict(aabb=aabb, center=center, has_children=has_children, n_prims=n_prims,
                lines=np.concatenate(lines) if lines else np.zeros(0, dtype=np.int32))


WIRE_CANDIDATES = [
    [1920, 1080, 128, 256, 128, 128], [0, 10, 0, 0, 1, 1], [10, 10, 0, 0, 0, 1], [10, 10, 5, 5, 6, 1],
    [100001, 10, 0, 0, 1, 1], [100000, 100000, 0, 0, 1, 1], [10, 10, 11, 0, 1, 1], [10, 10, 10, 0, 1, 1],
    [10, 10, 0, 0, 11, 1], [10, 10, 0, 0, 10, 10], [10, 10, 9, 9, 1, 1], [10, 10, 9, 9, 2, 1],
    [7, 5, 0, 4, 7, 1], [7, 5, 0, 5, 7, 1], [0xffffffff, 5, 0, 0, 1, 1], [10, 10, 0xfffffff0, 0, 32, 1],
]


def tree_and_wire_cases(td):
    """Octree topology (per node: box, centre, ordered debug_line_no list) and the
    wire bytes of WorkChunk / Camera, dumped from the compiled reference."""
    scenes = os.path.join(td, "scenes")
    trees = {}
    for name in ("cornell", "mini", "room"):
        obj = CORNELL if name == "cornell" else scenegen.write_scene(name, scenes)["obj"]
        wd = os.path.join(td, "tree_" + name)
        os.makedirs(wd, exist_ok=True)
        job = os.path.join(wd, "job.txt")
        out = os.path.join(wd, "tree.bin")
        open(job, "w").write("obj %s\nimage 0 0\ntree %s\n" % (obj, out))
        import subprocess
        subprocess.check_call([orclib.REF_DRIVER, job])
        raw = open(out, "rb").read()
        t = parse_tree_dump(raw)
        trees[name] = {"sha256": hashlib.sha256(raw).hexdigest(), "n_nodes": int(len(t["n_prims"])),
                       "n_prims": int(t["n_prims"].sum())}
        if name != "room":  # the room's dump is 1.9 MB: its hash is kept, the small trees in full
            np.savez_compressed(os.path.join(HERE, "tree_%s.npz" % name), **t)
        print("tree", name, trees[name])
    json.dump(trees, open(os.path.join(HERE, "trees.json"), "w"), indent=1, sort_keys=True)
    # wire bytes: one rendered chunk of the Cornell scene
    wd = os.path.join(td, "wire")
    os.makedirs(wd, exist_ok=True)
    cand = np.array(WIRE_CANDIDATES, dtype="<u4")
    cand.tofile(os.path.join(wd, "cand.bin"))
    cam = CORNELL_CAM2
    job = ["obj %s" % CORNELL, "image 96 64", "chunk 13 7 20 9",
           "camera " + " ".join(repr(float(c)) for c in cam)]
    for l in CORNELL_LIGHTS2:
        job.append("light " + " ".join(repr(float(c)) for c in l))
    job += ["out_rgb %s" % os.path.join(wd, "out.raw"), "wire %s" % os.path.join(wd, "wire.bin"),
            "wire_in %s" % os.path.join(wd, "cand.bin")]
    open(os.path.join(wd, "job.txt"), "w").write("\n".join(job) + "\n")
    import subprocess
    subprocess.check_call([orclib.REF_DRIVER, os.path.join(wd, "job.txt")])
    raw = np.fromfile(os.path.join(wd, "wire.bin"), dtype=np.uint8)
    n_out = 4 + 20 * 9 * 3
    assert raw.size == 24 + 56 + n_out + len(WIRE_CANDIDATES)
    np.savez_compressed(os.path.join(HERE, "wire.npz"), image=np.array([96, 64], dtype=np.int32),
                        chunk=np.array([13, 7, 20, 9], dtype=np.int32), cam=np.array(cam, dtype=np.float64),
                        lights=np.array(CORNELL_LIGHTS2, dtype=np.float64),
                        input_bytes=raw[:24], camera_bytes=raw[24:80], output_bytes=raw[80:80 + n_out],
                        candidates=cand.astype(np.uint32), verdicts=raw[80 + n_out:])
    print("wire", raw[:24].tobytes().hex(), "verdicts", list(raw[80 + n_out:]))


def main():
    assert orclib.have_ref(), "build the reference first: make -C oracle ref"
    if "--r4scenes" in sys.argv:
        # round 4's two more scenes (profiles/README.md): "loft" by the compiled reference (small frame in full + the SHA-256
        # of the 1920x1080 frame), "room_tex" by the ORACLE -- the reference build here has no texture.cc (SDL2), so a
        # textured frame cannot come from it: Texture::GetColorAt stays "parity unpinned", as everywhere
        with tempfile.TemporaryDirectory() as td:
            scenes = os.path.join(td, "scenes")
            loft = scenegen.write_scene("loft", scenes)
            render_case(td, "loft_240x135", loft["obj"], 240, 135, scenegen.ROOM_CAMERA, scenegen.ROOM_LIGHTS)
            tex = scenegen.write_scene("room_tex", scenes)
            o = orclib.OracleScene(tex["obj"])
            o.set_lights(scenegen.ROOM_LIGHTS)
            r = o.render(scenegen.ROOM_CAMERA, 240, 135, debug=True)
            np.savez_compressed(os.path.join(HERE, "room_tex_240x135.npz"), rgb=r["rgb"], line=r["line"], point=r["point"],
                                cam=np.array(scenegen.ROOM_CAMERA), lights=np.array(scenegen.ROOM_LIGHTS),
                                image=np.array([240, 135], dtype=np.int32), chunk=np.array([0, 0, 240, 135], dtype=np.int32))
            print("room_tex_240x135 (oracle-made)", sha(r["rgb"]))
            meta = json.load(open(os.path.join(HERE, "scene_hashes.json")))
            meta["loft"], meta["room_tex"] = loft["sha256"], tex["sha256"]
            json.dump(meta, open(os.path.join(HERE, "scene_hashes.json"), "w"), indent=1, sort_keys=True)
            fpath = os.path.join(HERE, "frames.json")
            frames = json.load(open(fpath))
            if "--big" in sys.argv:
                W, H = 1920, 1080
                rr = orclib.run_ref(os.path.join(td, "loft_big"), loft["obj"], (W, H), cam=scenegen.ROOM_CAMERA,
                                    lights=scenegen.ROOM_LIGHTS, want_debug=True)
                assert rr["returncode"] == 0, rr["stderr"]
                frames["loft_1920x1080_d5"] = {"sha256": sha(rr["rgb"]), "line_sha256": sha(rr["line"].astype("<i4")),
                                               "seconds_reference_here": rr["time"]["seconds"], "threads": rr["time"]["threads"],
                                               "scene_sha256": loft["sha256"]}
                print("loft_1920x1080_d5", frames["loft_1920x1080_d5"])
                ro = o.render(scenegen.ROOM_CAMERA, W, H, debug=True)
                frames["room_tex_1920x1080_d5"] = {"sha256": sha(ro["rgb"]), "line_sha256": sha(ro["line"].astype("<i4")),
                                                   "scene_sha256": tex["sha256"],
                                                   "made_by": "oracle (Texture::GetColorAt has no buildable reference here: parity unpinned)"}
                print("room_tex_1920x1080_d5", frames["room_tex_1920x1080_d5"])
            json.dump(frames, open(fpath, "w"), indent=1, sort_keys=True)
        return
    if "--deep20" in sys.argv:
        # "loft_fine": an octree of 20 levels, by the compiled reference (small frame in full + the SHA-256 of 1920x1080)
        with tempfile.TemporaryDirectory() as td:
            fine = scenegen.write_scene("loft_fine", os.path.join(td, "scenes"))
            render_case(td, "loft_fine_240x135", fine["obj"], 240, 135, scenegen.ROOM_CAMERA, scenegen.ROOM_LIGHTS)
            meta = json.load(open(os.path.join(HERE, "scene_hashes.json")))
            meta["loft_fine"] = fine["sha256"]
            json.dump(meta, open(os.path.join(HERE, "scene_hashes.json"), "w"), indent=1, sort_keys=True)
            W, H = 1920, 1080
            rr = orclib.run_ref(os.path.join(td, "fine_big"), fine["obj"], (W, H), cam=scenegen.ROOM_CAMERA,
                                lights=scenegen.ROOM_LIGHTS, want_debug=True)
            assert rr["returncode"] == 0, rr["stderr"]
            fpath = os.path.join(HERE, "frames.json")
            frames = json.load(open(fpath))
            frames["loft_fine_1920x1080_d5"] = {"sha256": sha(rr["rgb"]), "line_sha256": sha(rr["line"].astype("<i4")),
                                                "seconds_reference_here": rr["time"]["seconds"], "threads": rr["time"]["threads"],
                                                "scene_sha256": fine["sha256"]}
            print("loft_fine_1920x1080_d5", frames["loft_fine_1920x1080_d5"])
            json.dump(frames, open(fpath, "w"), indent=1, sort_keys=True)
        return
    if "--f2" in sys.argv:
        with tempfile.TemporaryDirectory() as td:
            render_case(td, "f2_decal_96x64", F2_DECAL, 96, 64, F2_CAM, F2_LIGHTS)
        return
    if "--big4k" in sys.argv:
        with tempfile.TemporaryDirectory() as td:
            big4k_frame(td)
        return
    if "--tree-wire-only" in sys.argv:
        with tempfile.TemporaryDirectory() as td:
            tree_and_wire_cases(td)
        return
    with tempfile.TemporaryDirectory() as td:
        scenes = os.path.join(td, "scenes")
        mini = scenegen.write_scene("mini", scenes)
        mini_n = scenegen.write_scene("mini_nomtl", scenes)
        render_case(td, "cornell_256", CORNELL, 256, 256, CORNELL_CAM, CORNELL_LIGHTS)
        render_case(td, "cornell_cam2_96x64", CORNELL, 96, 64, CORNELL_CAM2, CORNELL_LIGHTS2)
        render_case(td, "cornell_nolights_64", CORNELL, 64, 64, CORNELL_CAM, [])
        render_case(td, "f2_decal_96x64", F2_DECAL, 96, 64, F2_CAM, F2_LIGHTS)
        render_case(td, "mini_320x180", mini["obj"], 320, 180, scenegen.ROOM_CAMERA, scenegen.ROOM_LIGHTS)
        render_case(td, "mini_nomtl_320x180", mini_n["obj"], 320, 180, scenegen.ROOM_CAMERA, scenegen.ROOM_LIGHTS)
        render_case(td, "mini_chunk_101x67", mini["obj"], 320, 180, scenegen.ROOM_CAMERA, scenegen.ROOM_LIGHTS,
                    chunk=(37, 21, 101, 67))
        render_case(td, "mini_1x1", mini["obj"], 320, 180, scenegen.ROOM_CAMERA, scenegen.ROOM_LIGHTS,
                    chunk=(160, 90, 1, 1))
        ray_case(td, "rays_cornell", CORNELL,
                 np.concatenate([random_rays(11, 600, (0, 0, 0), (100, 100, 100)), special_rays()]))
        ray_case(td, "rays_mini", mini["obj"], random_rays(12, 800, (0, 0, 0), (400, 250, 400)))
        sensor_case(td)
        quirk_cases(td)
        room = scenegen.write_scene("room", scenes)
        render_case(td, "room_240x135", room["obj"], 240, 135, scenegen.ROOM_CAMERA, scenegen.ROOM_LIGHTS)
        # more views of the room: other octants, grazing floor reflections, a close-up of
        # the glass, an axis-aligned camera on the root's split plane (x = 200), two lights
        for name, cam, lights in ROOM_VIEWS:
            render_case(td, name, room["obj"], 200, 112, cam, lights)
        ray_case(td, "rays_room", room["obj"], random_rays(13, 400, (0, 0, 0), (400, 250, 400)))
        meta = {"mini": mini["sha256"], "mini_nomtl": mini_n["sha256"], "room": room["sha256"]}
        json.dump(meta, open(os.path.join(HERE, "scene_hashes.json"), "w"), indent=1, sort_keys=True)
        tree_and_wire_cases(td)
        if "--big" in sys.argv:
            big_frames(td)


if __name__ == "__main__" and "--depth4" not in sys.argv and "--live" not in sys.argv:
    main()


def depth4_frames():
    """BASELINE configs[3] (recursion depth 4): the reference's depth is a
    compile-time 5 (mythtracer.h:11), so these vectors come from the ORACLE
    (oracle/mt_oracle.c, max_level = 4), which is pinned bit-for-bit to the
    reference at depth 5 by everything else in this directory:
        python tests/golden/make_golden.py --depth4"""
    with tempfile.TemporaryDirectory() as td:
        info = scenegen.write_scene("room", os.path.join(td, "scenes"))
        o = orclib.OracleScene(info["obj"])
        o.set_lights(scenegen.ROOM_LIGHTS)
        W, H = 1920, 1080
        r = o.render(scenegen.ROOM_CAMERA, W, H, max_level=4, debug=True)
        fpath = os.path.join(HERE, "frames.json")
        frames = json.load(open(fpath))
        key = "room_%dx%d_d4" % (W, H)
        frames[key] = {"sha256": sha(r["rgb"]), "line_sha256": sha(r["line"].astype("<i4")),
                       "scene_sha256": info["sha256"], "made_by": "oracle (max_level 4), not the reference",
                       "rays": {k: r["counters"][k] for k in ("rays_primary", "rays_secondary", "rays_shadow")}}
        np.savez_compressed(os.path.join(HERE, key + "_sub16.npz"), rgb=r["rgb"][::16, ::16],
                            line=r["line"][::16, ::16], point=r["point"][::16, ::16])
        json.dump(frames, open(fpath, "w"), indent=1, sort_keys=True)
        print(key, frames[key])


if "--depth4" in sys.argv and __name__ == "__main__":
    depth4_frames()


LIVE_CAM = (120.0, 90.0, 60.0, 5.0, 20.0, -3.0, 100.0)


def live_case():
    """The case of tests/test_oracle_golden.py::test_live_reference_agrees (mini scene, a camera and two lights no
    other fixture uses), stored so that the test runs without the compiled reference:
        python tests/golden/make_golden.py --live"""
    assert orclib.have_ref(), "build the reference first: make -C oracle ref"
    with tempfile.TemporaryDirectory() as td:
        mini = scenegen.write_scene("mini", os.path.join(td, "scenes"))
        render_case(td, "mini_live_200x120", mini["obj"], 200, 120, LIVE_CAM, scenegen.ROOM_LIGHTS[:2])


if "--live" in sys.argv and __name__ == "__main__":
    live_case()
