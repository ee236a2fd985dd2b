#!/usr/bin/env python3
"""Generates tests/golden/gbuffer_<scene>_<W>x<H>.npz by running the REFERENCE ITSELF (oracle/_ref/ref_driver, built
by `python __graft_entry__.py` or `make -C oracle ref` where the reference's sources exist):

    python tests/golden/make_gbuffer_golden.py

For each camera two jobs of orclib.run_ref: `want_sensor=True` gives the reference's ray direction of every pixel
(Sensor::GetRay), and `rays=` over (camera origin, that direction) gives what the reference's OctTree::IntersectRay,
Triangle::GetNormal and Triangle::GetUVW return for it: line, t, point, normal, uvw.  The files hold data only: the
inputs (camera, image size) and what the reference wrote; `made_by` records that.  On a miss the reference's driver
writes line = -1 and leaves the doubles unspecified: they are stored as NaN.
"""
from __future__ import annotations

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

W, H = 96, 54
CORNELL = os.path.join(ROOT, "tests", "scenes", "cornell_n.obj")
# cornell: from outside the box with a wide lens -- the background is in view (misses) -- and yaw 0: the pixel column
#          with a zero direction component is the NaN column of Node::NodeIntersectRay;
# mini:    a rolled and pitched camera no axis is special for;
# room:    the bench's camera, yaw 0 again, inside the room.
CASES = [("cornell", (50.0, 50.0, -120.0, 0.0, 0.0, 0.0, 100.0)),
         ("mini", (120.0, 90.0, 60.0, 5.0, 20.0, -3.0, 100.0)),
         ("room", scenegen.ROOM_CAMERA)]
MADE_BY = "reference (oracle/_ref/ref_driver: sensor dump, then its ray job over those rays)"


def make_case(td, name, obj, cam):
    r = orclib.run_ref(os.path.join(td, name + "_sensor"), obj, (W, H), cam=cam, want_rgb=False, want_sensor=True)
    assert r["returncode"] == 0, r["stderr"]
    dirs = r["sensor"]  # (H, W, 3)
    rays = np.concatenate([np.broadcast_to(np.array(cam[:3], dtype=np.float64), (H, W, 3)), dirs], axis=-1)
    q = orclib.run_ref(os.path.join(td, name + "_rays"), obj, rays=rays.reshape(-1, 6))
    assert q["returncode"] == 0, q["stderr"]
    out = q["rays"]
    line = out["line"].reshape(H, W).astype(np.int32)
    miss = line < 0
    planes = {}
    for k, shape in (("t", (H, W)), ("point", (H, W, 3)), ("normal", (H, W, 3)), ("uvw", (H, W, 3))):
        a = np.array(out[k], dtype=np.float64).reshape(shape)
        a[miss] = np.nan
        planes[k] = a
    path = os.path.join(HERE, "gbuffer_%s_%dx%d.npz" % (name, W, H))
    np.savez_compressed(path, cam=np.array(cam, dtype=np.float64), image=np.array([W, H], dtype=np.int32), dirs=dirs,
                        line=line, made_by=np.array(MADE_BY), **planes)
    print(name, "%dx%d" % (W, H), int((~miss).sum()), "hits,", int(miss.sum()), "misses,", os.path.getsize(path), "bytes")


def main():
    assert orclib.have_ref(), "build the reference first: python __graft_entry__.py (or make -C oracle ref)"
    with tempfile.TemporaryDirectory() as td:
        scenes = os.path.join(td, "scenes")
        for name, cam in CASES:
            obj = CORNELL if name == "cornell" else scenegen.write_scene(name, scenes)["obj"]
            make_case(td, name, obj, cam)


if __name__ == "__main__":
    main()
