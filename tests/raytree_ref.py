"""What the CPU oracle (tests/orclib.py) says a ray-tree buffer is (include/mythtracer_hip.h, mt_raytree_create ff.), and the
shade over it -- shared by tests/test_raytree_cpu.py, which pins the composite frame to OracleScene.render byte for byte,
and tests/test_gpu_raytree.py, which holds the kernels to it.  Test infrastructure.

The definition in numpy fp64, one layer at a time.  A layer's rays go through a pluggable intersector (`trace`, by
default OracleScene.intersect); the planes follow gbuffer_ref's rules (plane_rules restates oracle_gbuffer's for a ray
LIST; the CPU test holds layer 0 to oracle_gbuffer itself); the shadow loops are lightbuffer_ref.shadow_loops; the
direct term is lightbuffer_ref.shade's before V3DtoRGB (direct_term; the CPU test holds its quantised layer 0 at depth 0
to lightbuffer_ref.shade itself).  Layer 0's order comes from mythtracer_amd.tiling.raytree_layer0_order.  Every product
and sum is rounded on its own, in the reference's order of operations (numpy never fuses).
"""
from __future__ import annotations

import math
import os

import numpy as np

import gbuffer_ref
import lightbuffer_ref as lr
from conftest import ROOT
from mythtracer_amd import tiling

TWO_WAY = os.path.join(ROOT, "tests", "scenes", "two_way.obj")
# the cameras of lightbuffer_ref plus the one of tests/scenes/two_way.obj: in the open side of the room, turned a little past the pane
CAMERAS = dict(lr.CAMERAS, two_way=(200.0, 110.0, 10.0, 0.0, 20.0, 0.0, 100.0))
F64_PLANES = ("ray", "coef", "point", "normal", "albedo", "power")
INT_PLANES = ("in_object", "material", "in_shadow", "child_refl", "child_refr")


def plane_rules(orc, r):
    """point, normal, albedo, material (the ORACLE's numbering) and prim of a ray list from OracleScene.intersect's
    answer `r`, by gbuffer_ref.oracle_gbuffer's rules: NaN / -1 on a miss; albedo = ambient, times tex_color_at(u, v)
    where the material has a texture; NaN without a material and where u or v is NaN."""
    hit = r["tri"] >= 0
    n = len(hit)
    out = {"prim": r["tri"].astype(np.int32)}
    for name in ("point", "normal"):
        a = r[name].copy()
        a[~hit] = np.nan
        out[name] = a
    _, tri_mtl, _ = orc.triangles()
    mats = orc.materials()
    material = np.full(n, -1, dtype=np.int32)
    albedo = np.full((n, 3), np.nan)
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
    out["material"] = material
    out["albedo"] = albedo
    return out


def _flipped(normal, d):
    """mythtracer.cc:40-45: the normal turned towards the ray's origin, and normal_ray_dot."""
    normal = normal.copy()
    towards_camera = -d
    nrd = lr._dot(normal, towards_camera)
    flip = nrd < 0.0
    normal[flip] = -normal[flip]
    nrd[flip] = lr._dot(normal[flip], towards_camera[flip])
    return normal, nrd


def layer0_rays(cam, W, H, chunk=None):
    """Layer 0: the chunk's pixel rays (Sensor::GetRay) in tiling.raytree_layer0_order, and that order."""
    cx, cy, cw, ch = chunk if chunk else (0, 0, W, H)
    order = tiling.raytree_layer0_order(cw, ch)
    rays = gbuffer_ref.pixel_rays(cam, W, H, chunk).reshape(cw * ch, 6)
    return rays[order], order


def build(orc, cam, W, H, lights, max_depth, chunk=None, trace=None, shadow=None):
    """The ray tree of a chunk under `lights` (n x 12; the positions matter): dict with
      layers      one dict per layer: ray (n, 6), in_object (n,) uint8, coef (n,), point / normal / albedo (n, 3), material
                  (n,) int32 in the ORACLE's numbering, prim, power (n_lights, n, 3), in_shadow (n_lights, n) uint8,
                  iterations (n_lights, n), child_refl / child_refr (n,) int32, and `pixel` in layer 0
      n_rays      per layer
      rays_primary, rays_secondary, rays_shadow, shaded_hits   what a frame of this depth counts
    trace: rays (n, 6) -> OracleScene.intersect's dict; shadow: lightbuffer_ref.oracle_intersector's kind."""
    trace = trace or orc.intersect
    shadow = shadow or lr.oracle_intersector(orc)
    mats = orc.materials()
    L = np.asarray(lights, dtype=np.float64).reshape(-1, 12)
    rays, order = layer0_rays(cam, W, H, chunk)
    in_object = np.zeros(len(rays), dtype=np.uint8)
    coef = np.ones(len(rays))
    layers = []
    for level in range(max_depth + 1):
        n = len(rays)
        lay = dict(ray=rays, in_object=in_object, coef=coef)
        lay.update(plane_rules(orc, trace(rays)))
        lit = (lay["prim"] >= 0) & (lay["material"] >= 0)
        sl = lr.shadow_loops(shadow, lay["point"].reshape(1, n, 3), lit.reshape(1, n), L)
        lay["power"] = sl["power"].reshape(len(L), n, 3)
        lay["in_shadow"] = sl["in_shadow"].reshape(len(L), n)
        lay["iterations"] = sl["iterations"].reshape(len(L), n)
        if level == 0:
            lay["pixel"] = order.copy()
        # the child conditions, mythtracer.cc:181-184 and :192, with max_depth for MAX_RECURSION_LEVEL
        values = np.array([mats[m][1] if m >= 0 else np.zeros(16) for m in lay["material"]]).reshape(n, 16)
        reflectance, transparency = values[:, 10], values[:, 11]
        deeper = level < max_depth
        refl = lit & deeper & (reflectance > 0.0) & (coef > 0.01) & (in_object == 0)
        refr = lit & deeper & (transparency > 0.0)
        # children in parent order, a parent's reflected ray before its refracted one
        slot = np.cumsum(refl.astype(np.int64) + refr.astype(np.int64)) - (refl.astype(np.int64) + refr.astype(np.int64))
        lay["child_refl"] = np.where(refl, slot, -1).astype(np.int32)
        lay["child_refr"] = np.where(refr, slot + refl, -1).astype(np.int32)
        lay["refused"] = dict(  # (for the tests' own input checks) a reflection refused by one condition alone
            by_coef=lit & deeper & (reflectance > 0.0) & ~(coef > 0.01) & (in_object == 0),
            by_in_object=lit & deeper & (reflectance > 0.0) & (coef > 0.01) & (in_object != 0))
        layers.append(lay)
        n_next = int(refl.sum() + refr.sum())
        if n_next == 0:
            break
        d = rays[:, 3:]
        normal, _ = _flipped(lay["normal"], d)
        nrays = np.zeros((n_next, 6))
        nin = np.zeros(n_next, dtype=np.uint8)
        ncoef = np.zeros(n_next)
        k = np.nonzero(refl)[0]
        reflected = d[k] - normal[k] * (2 * lr._dot(d[k], normal[k]))[:, None]   # :68-69
        at = lay["child_refl"][k]
        nrays[at, :3] = lay["point"][k] + (reflected * 0.0001)                    # :70-74
        nrays[at, 3:] = reflected
        nin[at] = in_object[k]                                                    # :186-187
        ncoef[at] = coef[k] * reflectance[k]
        k = np.nonzero(refr)[0]
        refracted = lr._norm(d[k])                                                # :208-212
        at = lay["child_refr"][k]
        nrays[at, :3] = lay["point"][k] + refracted * 0.00001                     # :214-218
        nrays[at, 3:] = refracted
        nin[at] = 1 - in_object[k]                                                # :222-223
        ncoef[at] = coef[k]
        rays, in_object, coef = nrays, nin, ncoef
    return finish(dict(layers=layers, max_depth=max_depth, n_lights=len(L)))


def finish(tree):
    layers = tree["layers"]
    tree["n_rays"] = [len(l["ray"]) for l in layers]
    tree["rays_primary"] = tree["n_rays"][0]
    tree["rays_secondary"] = int(sum(tree["n_rays"][1:]))
    tree["rays_shadow"] = int(sum(int(l["iterations"].sum()) for l in layers))
    tree["shaded_hits"] = int(sum(int((l["prim"] >= 0).sum()) for l in layers))
    return tree


def truncated(tree, max_depth):
    """The tree of a SHALLOWER max_depth from a deeper one of the same frame and lights: nothing above a layer depends on
    max_depth but `level < max_depth` in the child conditions, so the layers 0 .. max_depth are the same and the rays
    of layer max_depth have no children."""
    assert 0 <= max_depth <= tree["max_depth"]
    layers = [dict(l) for l in tree["layers"][:max_depth + 1]]
    if len(layers) == max_depth + 1:
        last = layers[-1]
        last["child_refl"] = np.full_like(last["child_refl"], -1)
        last["child_refr"] = np.full_like(last["child_refr"], -1)
    return finish(dict(layers=layers, max_depth=max_depth, n_lights=tree["n_lights"]))


def direct_term(orc, lay, lights, info=None):
    """mythtracer.cc:38-177 per ray of a layer from its planes and the stored direction: lightbuffer_ref.shade before
    V3DtoRGB -- black for a miss, the grey of :49-52 without a material -- as (n, 3) float64.  info: a dict that
    receives "specular" (n,) bool, the rays that take the specular branch (:169-177) for some light."""
    n = len(lay["ray"])
    L = np.asarray(lights, dtype=np.float64).reshape(-1, 12)
    assert lay["power"].shape == (len(L), n, 3), (lay["power"].shape, len(L), n)
    mats = orc.materials()
    color = np.zeros((n, 3))                                    # :23-31 for the misses
    h = np.nonzero(lay["prim"] >= 0)[0]
    d = lay["ray"][h, 3:]
    normal, nrd = _flipped(lay["normal"][h], d)
    towards_camera = -d
    bare = lay["material"][h] < 0                               # :49-52
    g = (nrd[bare] + 1.0) * 0.5
    color[h[bare]] = np.stack([g, g, g], axis=1)
    s = ~bare
    hs = h[s]
    d, normal, towards_camera = d[s], normal[s], towards_camera[s]
    Pt = lay["point"][hs]
    surf = lay["albedo"][hs]
    values = np.array([mats[m][1] for m in lay["material"][hs]]).reshape(len(hs), 16)
    kd, ks, ns = values[:, 3:6], values[:, 6:9], values[:, 9]
    reflected = d - normal * (2 * lr._dot(d, normal))[:, None]  # :68-69
    refl_dot = lr._dot(reflected, towards_camera)               # :170
    c = np.zeros((len(hs), 3))
    specular = np.zeros(n, dtype=bool)
    for li, light in enumerate(L):
        lpos, amb, ldiff, lspec = light[0:3], light[3:6], light[6:9], light[9:12]
        ld = lr._norm(lpos[None, :] - Pt)                       # :79-80
        c = c + amb[None, :] * surf                             # :83-84
        lp = lay["power"][li][hs]
        lp = np.where(lp < amb[None, :], amb[None, :], lp)      # std::max(lp, amb), :159-161
        c = c + kd * surf * lr._dot(ld, normal)[:, None] * ldiff[None, :] * lp  # :163-167
        spec = (lay["in_shadow"][li][hs] == 0) & (refl_dot > 0)                # :169-177
        k = np.nonzero(spec)[0]
        specular[hs[k]] = True
        p = np.array([math.pow(a, b) for a, b in zip(refl_dot[k], ns[k])]).reshape(len(k))
        c[k] = c[k] + ks[k] * surf[k] * p[:, None] * lspec[None, :]
    color[hs] = c
    if info is not None:
        info["specular"] = specular
    return color


def v3d_to_rgb(color):
    """MythTracer::V3DtoRGB (mythtracer.cc:235-241) over (n, 3): > 1 -> 255, < 0 -> 0, else the truncated v * 255; a
    NaN -- light colours no scene file holds -- gives 0, as orclib.v3d_to_rgb and channel_to_u8 define it."""
    inside = np.clip(np.where(np.isnan(color), 0.0, color), 0.0, 1.0)
    return np.where(color > 1.0, 255, np.where(color < 0.0, 0, (inside * 255).astype(np.uint8))).astype(np.uint8)


def shade(orc, tree, lights, cw, ch, info=None):
    """The frame of a tree under `lights` (count and positions the tree's): layers bottom-up, per ray the direct term,
    + colour[child_refl] * reflectance (:185-188), + colour[child_refr] * transmission_filter * transparency as
    :220-224 associates it; layer 0 through V3DtoRGB to the ray's pixel.  (ch, cw, 3) uint8.  info: a dict that
    receives "specular" (ch, cw) bool, the pixels with a ray in their tree that takes the specular branch."""
    mats = orc.materials()
    below = spec_below = None
    for lay in reversed(tree["layers"]):
        term = {}
        color = direct_term(orc, lay, lights, term)
        spec = term["specular"]
        for name in ("child_refl", "child_refr"):
            k = np.nonzero(lay[name] >= 0)[0]
            if len(k):
                spec[k] |= spec_below[lay[name][k]]
        spec_below = spec
        values = np.array([mats[m][1] if m >= 0 else np.zeros(16) for m in lay["material"]]).reshape(len(color), 16)
        k = np.nonzero(lay["child_refl"] >= 0)[0]
        if len(k):
            color[k] = color[k] + below[lay["child_refl"][k]] * values[k, 10][:, None]
        k = np.nonzero(lay["child_refr"] >= 0)[0]
        if len(k):
            color[k] = color[k] + below[lay["child_refr"][k]] * values[k, 12:15] * values[k, 11][:, None]
        below = color
    rgb = np.zeros((cw * ch, 3), dtype=np.uint8)
    rgb[tree["layers"][0]["pixel"]] = v3d_to_rgb(below)
    if info is not None:
        px = np.zeros(cw * ch, dtype=bool)
        px[tree["layers"][0]["pixel"]] = spec_below
        info["specular"] = px.reshape(ch, cw)
    return rgb.reshape(ch, cw, 3)
