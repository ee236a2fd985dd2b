"""What the CPU oracle (tests/orclib.py) says a direct-light buffer is, and the relight pass over it -- shared by
tests/test_lightbuffer_cpu.py, which pins both (to the oracle's own max_level = 0 frames, byte for byte, and to goldens
made with the reference's IntersectRay), and tests/test_gpu_lightbuffer.py, which holds the kernels to them.  Test
infrastructure.

The shadow loop of mythtracer.cc:90-156 runs here in numpy fp64, vectorised over the pixels, ONE ITERATION AT A TIME:
every iteration hands the shadow rays of the pixels still in the loop to an `intersector` and consumes the answers in the
reference's order of operations -- Norm, Distance and SqrDistance as math3d.h writes them, sums left to right, every
product and sum rounded on its own (numpy never fuses).  The intersector is OracleScene.intersect (oracle_intersector)
or the compiled reference's own IntersectRay (tests/golden/make_lightbuffer_golden.py).
"""
from __future__ import annotations

import math
import os

import numpy as np

import orclib
from mythtracer_amd import scenegen

# light sets of the tests: the bench's three lights, and one light with three different colours per term
BENCH_LIGHTS = [tuple(float(v) for v in l) for l in scenegen.ROOM_LIGHTS]
ONE_LIGHT = {
    "cornell": [(50.0, 90.0, 50.0, 0.3, 0.3, 0.3, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)],
    "f2_decal": [(50.0, 60.0, 50.0, 0.1, 0.1, 0.1, 1.0, 1.0, 1.0, 0.5, 0.5, 0.5)],
    None: [(150.0, 180.0, 120.0, 0.1, 0.2, 0.05, 0.9, 0.8, 1.0, 0.7, 1.0, 0.5)],
}
# the camera of every scene of these tests (the G-buffer goldens' for cornell, mini and room)
CAMERAS = {"cornell": (50.0, 50.0, -120.0, 0.0, 0.0, 0.0, 100.0),
           "mini": (120.0, 90.0, 60.0, 5.0, 20.0, -3.0, 100.0),
           "room": scenegen.ROOM_CAMERA,
           "f2_decal": (50.0, 6.0, -30.0, 12.0, 0.0, 0.0, 70.0)}  # (looks across the pane of glass and its decal)


def light_sets(scene):
    return {"bench": BENCH_LIGHTS, "one": ONE_LIGHT.get(scene, ONE_LIGHT[None])}


def edited(lights, k):
    """Colour edits of a light set, positions untouched.  k = 0: other colours; 1: an ambient ABOVE every stored power
    (mythtracer.cc:159-161 then takes the ambient); 2: zero specular; 3: everything zero but the ambient."""
    out = []
    for i, l in enumerate(lights):
        p = list(l[:3])
        if k == 0:
            out.append(tuple(p + [0.05 * (i + 1), 0.1, 0.02, 0.9, 0.5 + 0.1 * i, 0.7, 0.2, 1.0, 0.6]))
        elif k == 1:
            out.append(tuple(p + [1.5, 1.25, 2.0] + list(l[6:12])))
        elif k == 2:
            out.append(tuple(p + list(l[3:9]) + [0.0, 0.0, 0.0]))
        else:
            out.append(tuple(p + [0.2, 0.3, 0.4] + [0.0] * 6))
    return out


def _norm(v):
    """V3D::Norm, math3d.h:128-131."""
    l = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    return v / l[:, None]


def _sqr_distance(self, a):
    """self.SqrDistance(a), math3d.h:105-110."""
    d = a - self
    return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]


def _dot(self, a):
    """self.Dot(a), math3d.h:116-118."""
    return a[:, 0] * self[:, 0] + a[:, 1] * self[:, 1] + a[:, 2] * self[:, 2]


def oracle_intersector(orc):
    """rays (n, 6) -> hit, t, point and the occluder's transparency and transmission filter (an occluder without a
    material: transparency 0, i.e. opaque -- what the kernels define where the reference dereferences NULL)."""
    _, tri_mtl, _ = orc.triangles()
    mats = orc.materials()
    tr = np.array([m[1][11] for m in mats] + [0.0])
    tf = np.array([m[1][12:15] for m in mats] + [np.zeros(3)])

    def intersect(rays):
        r = orc.intersect(rays)
        hit = r["tri"] >= 0
        m = np.where(hit, tri_mtl[np.maximum(r["tri"], 0)], -1)
        return dict(hit=hit, t=r["t"], point=r["point"], transparency=np.where(hit, tr[m], 0.0), filter=tf[m])
    return intersect


def shadow_loops(intersect, point, lit, lights, info=None):
    """point (ch, cw, 3), lit (ch, cw) = the pixels for which the reference enters the light loop.  Returns
    power (n_lights, ch, cw, 3), in_shadow (n_lights, ch, cw) uint8 with 255 where not lit, iterations (n_lights, ch, cw).
    info: a dict that receives how often each way out of the loop was taken and what kind of occluder was met (for
    tests/hostile_scenes.py, which counts the iterations an unusual value decides)."""
    ch, cw = lit.shape
    n = ch * cw
    P = np.ascontiguousarray(point, dtype=np.float64).reshape(n, 3)
    lit = lit.reshape(n)
    L = np.asarray(lights, dtype=np.float64).reshape(-1, 12)
    power = np.full((len(L), n, 3), np.nan)
    shadow = np.full((len(L), n), 255, dtype=np.uint8)
    iterations = np.zeros((len(L), n), dtype=np.int32)
    idx0 = np.nonzero(lit)[0]
    ends = dict.fromkeys(("ended_behind_the_light", "ended_past_the_light", "ended_opaque", "light_within_1e-5_of_start",
                          "occluders_negative_tr", "occluders_negative_zero_tr", "occluders_hostile_tr",
                          "dim_at_exactly_0.001", "one_channel_above_0.001", "t_equals_light_distance"), 0)
    for li, light in enumerate(L):
        lpos = np.broadcast_to(light[0:3], (len(idx0), 3))
        Pt = P[idx0]
        ld = _norm(lpos - Pt)                       # :79-80
        lp = np.ones((len(idx0), 3))                # :90
        in_shadow = np.zeros(len(idx0), dtype=bool)
        traversing = np.zeros(len(idx0), dtype=bool)
        start = Pt.copy()                           # :94
        running = np.ones(len(idx0), dtype=bool)
        while running.any():
            k = np.nonzero(running)[0]
            origin = start[k] + (ld[k] * 0.00001)   # :95-99
            light_distance = np.sqrt(_sqr_distance(start[k], lpos[k]))  # :101-102
            r = intersect(np.concatenate([origin, ld[k]], axis=1))
            iterations[li, idx0[k]] += 1
            hit = r["hit"]
            behind = hit & (r["t"] > light_distance)             # :115-118
            opaque = hit & ~behind & (r["transparency"] == 0.0)  # :121-125
            through = hit & ~behind & ~opaque
            lp[k[opaque]] = 0.0
            in_shadow[k[opaque]] = True
            running[k[~hit | behind | opaque]] = False
            t = k[through]
            first = ~traversing[t]                               # :129-132
            f = r["filter"][through] * r["transparency"][through][:, None]
            lp[t[first]] = lp[t[first]] * f[first]
            traversing[t] = ~traversing[t]
            start[t] = r["point"][through] + (ld[t] * 0.0000001)  # :137
            past = _sqr_distance(Pt[t], start[t]) > _sqr_distance(Pt[t], lpos[t])  # :141-145
            dim = ~past & (lp[t] <= 0.001).all(axis=1)            # :149-155
            dim_exact = int((dim & (lp[t] == 0.001).any(axis=1)).sum())
            lp[t[dim]] = 0.0
            in_shadow[t[dim]] = True
            running[t[past | dim]] = False
            tr_ = r["transparency"]
            ends["ended_behind_the_light"] += int(behind.sum())
            ends["ended_past_the_light"] += int(past.sum())
            ends["ended_opaque"] += int(opaque.sum())
            ends["light_within_1e-5_of_start"] += int((light_distance < 0.00001).sum())
            ends["occluders_negative_tr"] += int((through & (tr_ < 0.0)).sum())
            ends["occluders_negative_zero_tr"] += int((opaque & np.signbit(tr_)).sum())
            ends["occluders_hostile_tr"] += int((through & ((tr_ >= 1.0) | (tr_ < 1e-3) | (r["filter"] == 0.0).any(axis=1))).sum())
            ends["dim_at_exactly_0.001"] += dim_exact
            ends["t_equals_light_distance"] += int((hit & (r["t"] == light_distance)).sum())
            ends["one_channel_above_0.001"] += int((~past & ~dim & ((lp[t] <= 0.001).sum(axis=1) == 2)).sum())
        power[li, idx0] = lp
        shadow[li, idx0] = in_shadow
    if info is not None:
        info.update(ends)
    return dict(power=power.reshape(len(L), ch, cw, 3), in_shadow=shadow.reshape(len(L), ch, cw),
                iterations=iterations.reshape(len(L), ch, cw))


def ref_lightbuffer(orc, gb, lights):
    """The light buffer by the oracle for the primary hits of gbuffer_ref.oracle_gbuffer: power, in_shadow, iterations
    (see shadow_loops) and rays_shadow = their sum."""
    lit = (gb["prim"] >= 0) & (gb["material"] >= 0)
    out = shadow_loops(oracle_intersector(orc), gb["point"], lit, lights)
    out["rays_shadow"] = int(out["iterations"].sum())
    return out


def shade(orc, gb, lb, lights, materials=None, hit=None, info=None):
    """mythtracer.cc:38-177 and V3DtoRGB per pixel from the planes: the frame of the direct term, (ch, cw, 3) uint8.
    gb: oracle_gbuffer's dict (rays, point, normal -- unflipped --, albedo, material in the oracle's numbering, prim);
    lb: power and in_shadow.  pow is math.pow: glibc's, what the oracle and the reference call.
    For planes no scene made (tests/synthetic_inputs.py): `materials` = a table (n_materials, 16) of material values in
    place of the oracle scene's (orc may be None), its numbering the material plane's -- an index outside the table is
    "no material", as shade_direct_kernel defines it --, and `hit` (ch, cw) bool in place of prim >= 0.  info: a dict
    that receives "specular" (ch, cw) bool, the pixels that take the specular branch (:169-177) for some light."""
    ch, cw = gb["material"].shape
    n = ch * cw
    L = np.asarray(lights, dtype=np.float64).reshape(-1, 12)
    assert lb["power"].shape == (len(L), ch, cw, 3) and lb["in_shadow"].shape == (len(L), ch, cw)
    table = np.array([m[1] for m in orc.materials()] if materials is None else materials, dtype=np.float64).reshape(-1, 16)
    direction = gb["rays"][..., 3:].reshape(n, 3)
    hit = (gb["prim"] >= 0 if hit is None else np.asarray(hit, dtype=bool)).reshape(n)
    material = gb["material"].reshape(n)
    color = np.zeros((n, 3))                                    # :23-31 for the misses
    h = np.nonzero(hit)[0]
    d = direction[h]
    normal = gb["normal"].reshape(n, 3)[h].copy()
    towards_camera = -d                                         # :40
    nrd = _dot(normal, towards_camera)
    flip = nrd < 0.0                                            # :42-45
    normal[flip] = -normal[flip]
    nrd[flip] = _dot(normal[flip], towards_camera[flip])
    bare = (material[h] < 0) | (material[h] >= len(table))      # :49-52
    g = (nrd[bare] + 1.0) * 0.5
    color[h[bare]] = np.stack([g, g, g], axis=1)
    s = ~bare
    hs = h[s]
    d, normal, towards_camera = d[s], normal[s], towards_camera[s]
    Pt = gb["point"].reshape(n, 3)[hs]
    surf = gb["albedo"].reshape(n, 3)[hs]
    values = table[material[hs]].reshape(len(hs), 16)
    kd, ks, ns = values[:, 3:6], values[:, 6:9], values[:, 9]
    reflected = d - normal * (2 * _dot(d, normal))[:, None]     # :68-69 (ray.direction.Dot(normal))
    refl_dot = _dot(reflected, towards_camera)                  # :170
    c = np.zeros((len(hs), 3))
    specular = np.zeros(n, dtype=bool)
    for li, light in enumerate(L):
        lpos, amb, ldiff, lspec = light[0:3], light[3:6], light[6:9], light[9:12]
        ld = _norm(lpos[None, :] - Pt)                          # :79-80
        c = c + amb[None, :] * surf                             # :83-84
        lp = lb["power"][li].reshape(n, 3)[hs]
        lp = np.where(lp < amb[None, :], amb[None, :], lp)      # std::max(lp, amb), :159-161
        c = c + kd * surf * _dot(ld, normal)[:, None] * ldiff[None, :] * lp  # :163-167 (light_direction.Dot(normal))
        spec = (lb["in_shadow"][li].reshape(n)[hs] == 0) & (refl_dot > 0)      # :169-177
        k = np.nonzero(spec)[0]
        specular[hs[k]] = True
        p = np.array([math.pow(a, b) for a, b in zip(refl_dot[k], ns[k])]).reshape(len(k))
        c[k] = c[k] + ks[k] * surf[k] * p[:, None] * lspec[None, :]
    color[hs] = c
    if info is not None:
        info["specular"] = specular.reshape(ch, cw)
    rgb = np.zeros((n, 3), dtype=np.uint8)
    for i in range(n):
        rgb[i] = orclib.v3d_to_rgb(color[i])
    return rgb.reshape(ch, cw, 3)


def load_golden(name, W=96, H=54):
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, "lightbuffer_%s_%dx%d.npz" % (name, W, H)), allow_pickle=False)
    assert tuple(int(v) for v in g["image"]) == (W, H)
    assert str(g["made_by"]).startswith("reference"), g["made_by"]
    return g

