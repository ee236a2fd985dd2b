#!/usr/bin/env python3
"""Generates tests/golden/lightbuffer_<scene>_<W>x<H>.npz with the REFERENCE ITSELF as the intersector of every shadow
ray (oracle/_ref/ref_driver, built by `python __graft_entry__.py` or `make -C oracle ref` where the reference's sources
exist):

    python tests/golden/make_lightbuffer_golden.py

The primary hits are those of tests/golden/gbuffer_<scene>_*.npz, which the reference wrote.  From them the shadow loop
of mythtracer.cc:90-156 runs in tests/lightbuffer_ref.shadow_loops -- the same Python loop the tests use with the oracle
-- but every iteration's rays go through orclib.run_ref(..., rays=...), one job per iteration: the reference's
OctTree::IntersectRay answers with line, distance and point.  An occluder's material is the one of its .obj line (every
face of these scenes has one material; checked).  The reference cannot load textures here, so the scenes are the
untextured ones.  The files hold data only: inputs (camera, image size, lights), power, in_shadow, iteration counts,
and `made_by`.

Two conditions are asserted and their counts recorded in the files: some scene has pixels whose shadow loop runs two or
more iterations (light crossing a transparent occluder), and some scene has all three outcomes (lit, in shadow, 255).
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
import gbuffer_ref  # noqa: E402
import lightbuffer_ref  # noqa: E402
import orclib  # noqa: E402
from mythtracer_amd import scenegen  # noqa: E402

W, H = 96, 54
CORNELL = os.path.join(ROOT, "tests", "scenes", "cornell_n.obj")
SCENES = ("cornell", "mini", "room")
MADE_BY = "reference (oracle/_ref/ref_driver: its ray job answers every iteration of the shadow loops)"


def reference_intersector(td, obj, orc):
    _, tri_mtl, line = orc.triangles()
    mats = orc.materials()
    of_line = {}
    for m, l in zip(tri_mtl, line):
        assert of_line.setdefault(int(l), int(m)) == int(m), "two materials on .obj line %d" % l
    tr = np.array([m[1][11] for m in mats] + [0.0])
    tf = np.array([m[1][12:15] for m in mats] + [np.zeros(3)])
    jobs = [0]

    def intersect(rays):
        jobs[0] += 1
        q = orclib.run_ref(os.path.join(td, "job%d" % jobs[0]), obj, rays=rays)
        assert q["returncode"] == 0, q["stderr"]
        out = q["rays"]
        hit = out["line"] >= 0
        m = np.array([of_line[int(l)] if l >= 0 else -1 for l in out["line"]], dtype=np.int64)
        return dict(hit=hit, t=np.array(out["t"]), point=np.array(out["point"]),
                    transparency=np.where(hit, tr[m], 0.0), filter=tf[m])
    return intersect, of_line


def make_case(td, name, obj):
    g = gbuffer_ref.load_golden(name, W, H)
    orc = orclib.OracleScene(obj)
    intersect, of_line = reference_intersector(os.path.join(td, name), obj, orc)
    hit = g["line"] >= 0
    lit = hit & np.array([[of_line.get(int(l), -1) >= 0 for l in row] for row in g["line"]])
    data = {}
    glass = mix = 0
    for key, lights in lightbuffer_ref.light_sets(name).items():
        lb = lightbuffer_ref.shadow_loops(intersect, g["point"], lit, lights)
        data["lights_" + key] = np.array(lights, dtype=np.float64)
        data["power_" + key] = lb["power"]
        data["in_shadow_" + key] = lb["in_shadow"]
        data["iterations_" + key] = lb["iterations"]
        glass += int((lb["iterations"] >= 2).sum())
        outcomes = [int((lb["in_shadow"] == v).sum()) for v in (0, 1, 255)]
        mix += int(all(outcomes))
        print(name, key, "lit / shadowed / no loop:", outcomes, " loops of >= 2 iterations:",
              int((lb["iterations"] >= 2).sum()), " shadow rays:", int(lb["iterations"].sum()))
    path = os.path.join(HERE, "lightbuffer_%s_%dx%d.npz" % (name, W, H))
    np.savez_compressed(path, cam=g["cam"], image=np.array([W, H], dtype=np.int32), made_by=np.array(MADE_BY),
                        glass_loops=np.array(glass), outcome_mixes=np.array(mix), **data)
    print(name, os.path.getsize(path), "bytes")
    return glass, mix


def main():
    assert orclib.have_ref(), "build the reference first: python __graft_entry__.py (or make -C oracle ref)"
    glass = mix = 0
    with tempfile.TemporaryDirectory() as td:
        scenes = os.path.join(td, "scenes")
        for name in SCENES:
            obj = CORNELL if name == "cornell" else scenegen.write_scene(name, scenes)["obj"]
            a, b = make_case(td, name, obj)
            glass += a
            mix += b
    assert glass > 0, "no golden scene has a shadow loop of two or more iterations"
    assert mix > 0, "no golden scene has all three outcomes (lit, in shadow, no loop)"


if __name__ == "__main__":
    main()
