#!/usr/bin/env python3
"""Generates tests/golden/hostile_<case>.npz and tests/golden/hostile.json by running the REFERENCE ITSELF
(oracle/_ref/ref_driver, built by `python __graft_entry__.py` or `make -C oracle ref` where the reference's sources
exist) on every case of tests/hostile_scenes.py:

    python tests/golden/make_hostile_golden.py

Per case one job of orclib.run_ref (64 x 48, the reference's compile-time depth of 5) gives the reference's frame and
its debug plane.  The files hold data only: the inputs (cam, lights, depth) and what the reference wrote (rgb, line,
point); `made_by` records that.  On a miss the reference writes line = -1 and NaN into the point.  A point plane that
is bit-identical to an earlier case's (the primary hits depend on camera and triangles alone) is stored once: the
later file names the earlier case in `point_of` instead.

A reference run that crashes or does not end within 60 s drops the case from the reference pin (hostile.json:
"dropped" with the reason; two at the most); so does reference=False (a depth the reference cannot be asked for).

Each case must bite: hostile_scenes.bite counts, with the oracle and the numpy restatements, the rays at which the
case's own comparison is decided by the hostile value; the count goes into hostile.json and a case with fewer than 20
fails here.  The oracle's disagreements with the reference are printed, not judged: tests/test_hostile_cpu.py judges.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostile_scenes as hs  # noqa: E402
import orclib  # noqa: E402
import raytree_ref as rr  # noqa: E402

MADE_BY = "reference (oracle/_ref/ref_driver: out_rgb and out_debug of one frame job)"
MIN_BITE = 20


def main():
    assert orclib.have_ref(), "build the reference first: python __graft_entry__.py (or make -C oracle ref)"
    pin = dict(image=[hs.W, hs.H], obj_sha256={v: hs.sha(hs.obj_text(v)) for v in hs.NORMAL_VARIANTS}, cases={},
               dropped={})
    points = {}
    toothless = []
    total = 0
    with tempfile.TemporaryDirectory() as td:
        for name, c in hs.CASES.items():
            obj = hs.write(name, td, check=False)
            orc = orclib.OracleScene(obj)
            orc.set_lights(c["lights"])
            tree = rr.build(orc, c["camera"], hs.W, hs.H, c["lights"], c["depth"])
            count = hs.bite(orc, tree, c["lights"])[c["counter"]]
            if count < MIN_BITE:
                toothless.append("%s: %s = %d" % (name, c["counter"], count))
            entry = dict(group=c["group"], counter=c["counter"], count=int(count), mtl_sha256=hs.sha(hs.mtl_text(c["edit"])),
                         normals=c["normals"], rays_per_layer=tree["n_rays"])
            pin["cases"][name] = entry
            if not c["reference"]:
                pin["dropped"][name] = "max_depth %d: the reference's limit is a compile-time 5; oracle only" % c["depth"]
                print(name, "oracle only;", c["counter"], count)
                continue
            r = orclib.run_ref(os.path.join(td, name + "_job"), obj, (hs.W, hs.H), cam=c["camera"], lights=c["lights"],
                               want_debug=True, timeout=60)
            if r["returncode"] != 0:
                pin["dropped"][name] = ("the reference did not end within 60 s" if r["returncode"] is None else
                                        "the reference crashed (exit status %d)" % r["returncode"])
                print(name, "DROPPED:", pin["dropped"][name], r["stderr"][-200:])
                continue
            line = r["line"].astype(np.int32)
            point = np.array(r["point"], dtype=np.float64)
            point[line < 0] = np.nan
            planes = dict(point=point)
            for other, p in points.items():
                if p.tobytes() == point.tobytes():
                    planes = dict(point_of=np.array(other))
                    break
            else:
                points[name] = point
            path = hs.golden_path(name)
            np.savez_compressed(path, cam=np.array(c["camera"], dtype=np.float64),
                                lights=np.array(c["lights"], dtype=np.float64), depth=np.array(c["depth"], dtype=np.int32),
                                image=np.array([hs.W, hs.H], dtype=np.int32), rgb=r["rgb"], line=line,
                                made_by=np.array(MADE_BY), **planes)
            size = os.path.getsize(path)
            assert size < 100 * 1024, (name, size)
            total += size
            want = orc.render(c["camera"], hs.W, hs.H, max_level=c["depth"], debug=True)
            print("%-28s %-28s %6d  %6d bytes  oracle differs in %d bytes, %d lines" % (
                name, c["counter"], count, size, int((want["rgb"] != r["rgb"]).sum()), int((want["line"] != line).sum())))
    assert not toothless, "cases that do not bite: " + "; ".join(toothless)
    assert total < 1024 * 1024, total
    unplanned = [n for n in pin["dropped"] if hs.CASES[n]["reference"]]
    assert len(unplanned) <= 2, unplanned
    with open(hs.JSON, "w", newline="\n") as f:
        json.dump(pin, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(pin["cases"]), "cases,", total, "bytes of goldens, dropped:", pin["dropped"])


if __name__ == "__main__":
    main()
