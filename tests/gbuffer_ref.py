"""What the CPU oracle (tests/orclib.py) says a primary-hit G-buffer is -- shared by tests/test_gbuffer_cpu.py, which pins
it to the reference-made goldens, and tests/test_gpu_gbuffer.py, which holds the kernel to it.  Test infrastructure."""
from __future__ import annotations

import os

import numpy as np

import orclib

F64_PLANES = ("depth", "point", "normal", "uvw", "albedo")
I32_PLANES = ("prim", "line_no", "material")
ALL_PLANES = F64_PLANES + I32_PLANES
TRAVERSAL_COUNTERS = ("box_tests", "node_visits", "tri_tests", "mt_tests")


def pixel_rays(cam, W, H, chunk=None):
    """(ch, cw, 6): camera origin and orclib.sensor_ray of every pixel of the chunk (Sensor::GetRay)."""
    cx, cy, cw, ch = chunk if chunk else (0, 0, W, H)
    sens = orclib.sensor(cam, W, H)
    rays = np.zeros((ch, cw, 6))
    rays[..., :3] = sens[:3]
    for y in range(ch):
        for x in range(cw):
            rays[y, x, 3:] = orclib.sensor_ray(sens, cx + x, cy + y)
    return rays


def oracle_gbuffer(orc, cam, W, H, chunk=None):
    """The eight planes by the oracle, plus "counters" (the traversal's work for these rays) and "rays".
      depth, point, normal, uvw, line_no   Scene.intersect's t, point, normal, uvw, line; NaN / -1 on a miss
      prim       the oracle's `tri`: it indexes its triangles in AddPrimitive order
      material   OracleScene.triangles()'s material index of that triangle, -1 = none (the ORACLE's numbering:
                 the order of the .mtl file; compare materials by value, see material_values)
      albedo     ambient * tex_color_at(u, v), elementwise in fp64, where the material has a texture, else ambient;
                 NaN without a material; NaN where u or v is NaN (what the kernels define for such coordinates)."""
    rays = pixel_rays(cam, W, H, chunk)
    ch, cw = rays.shape[:2]
    r = orc.intersect(rays.reshape(-1, 6))
    hit = r["tri"] >= 0
    out = {"rays": rays, "counters": r["counters"]}
    out["prim"] = r["tri"].astype(np.int32).reshape(ch, cw)
    out["line_no"] = np.where(hit, r["line"], -1).astype(np.int32).reshape(ch, cw)
    out["depth"] = np.where(hit, r["t"], np.nan).reshape(ch, cw)
    for src, dst in (("point", "point"), ("normal", "normal"), ("uvw", "uvw")):
        a = r[src].copy()
        a[~hit] = np.nan
        out[dst] = a.reshape(ch, cw, 3)
    _, tri_mtl, _ = orc.triangles()
    mats = orc.materials()
    material = np.full(len(hit), -1, dtype=np.int32)
    albedo = np.full((len(hit), 3), np.nan)
    for i in np.nonzero(hit)[0]:
        m = int(tri_mtl[r["tri"][i]])
        material[i] = m
        if m < 0:
            continue
        _, values, tex = mats[m]
        surf = values[0:3].copy()
        if tex >= 0:
            u, v = r["uvw"][i, 0], r["uvw"][i, 1]
            surf = surf * (orc.tex_color_at(tex, u, v) if (u == u and v == v) else np.full(3, np.nan))
        albedo[i] = surf
    out["material"] = material.reshape(ch, cw)
    out["albedo"] = albedo.reshape(ch, cw, 3)
    return out


def material_values(orc):
    """The oracle's materials by index: (16 values, has a texture)."""
    return [(values, tex >= 0) for _, values, tex in orc.materials()]


def same_bits(got, want, what=""):
    """Bit identity of two f64 arrays: the uint64 views are equal, except that a NaN equals a NaN (a miss is `some
    NaN`, whatever its payload).  Returns the number of differing elements; prints it."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    differ = (got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want))
    n = int(differ.sum())
    print("%s: %d of %d elements differ" % (what, n, got.size))
    return n


def load_golden(name, W=96, H=54):
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, "gbuffer_%s_%dx%d.npz" % (name, W, H)), allow_pickle=False)
    assert tuple(int(v) for v in g["image"]) == (W, H)
    assert str(g["made_by"]).startswith("reference"), g["made_by"]
    return g
