"""The hostile scene family: ONE small geometry (a floor, a back wall, two mirrors facing each other, a stack of six
horizontal panes under the main light, a cluster of small triangles and a dome fan with per-vertex normals) under
material tables, normals and lights at which TraceRayWorker's comparisons (mythtracer.cc:13-228) are decided by the
unusual value and not by a near miss -- shared by tests/golden/make_hostile_golden.py, tests/test_hostile_cpu.py and
tests/test_gpu_hostile.py.  Test infrastructure.

A case is (material edit, normal variant, lights, camera, depth), one thing changed at a time from a tame base, plus
a few combined ones; every frame is 64 x 48.  All inputs are finite and every triangle has a material (the reference
reads NULL otherwise, and V3DtoRGB of a NaN is undefined).  Every material of the base table has Ns 0, so pow() is
exactly 1 in every libm: the cases that leave it so are the EXACT group (the bar is identity everywhere), the ones
that edit Ns are the POW group.

The generated text is pinned by sha256 in tests/golden/hostile.json (write checks it), which also holds, per case,
the group, the name of the case's own counter -- the rays at which its comparison is decided by the hostile value --
and the count the maker measured.  `bite` measures the counters from the numpy restatements.
"""
from __future__ import annotations

import hashlib
import json
import math
import os

import numpy as np

import lightbuffer_ref as lr
from mythtracer_amd import scenegen

HERE = os.path.dirname(os.path.abspath(__file__))
JSON = os.path.join(HERE, "golden", "hostile.json")
W, H = 64, 48
SEED = 0x4057113
DEPTH = 5
PANE_Y = (20.0, 24.0, 28.0, 32.0, 36.0, 40.0)

# ka kd ks ns refl tr tf ni -- the tame table; Ns 0 everywhere (the exact group)
BASE = {
    "floor": dict(Ka=(0.6, 0.6, 0.55), Kd=(0.6, 0.6, 0.55), Ks=(0.2, 0.2, 0.2), Ns=0, Refl=0.2),
    "wall": dict(Ka=(0.7, 0.7, 0.75), Kd=(0.7, 0.7, 0.75), Ks=(0.1, 0.1, 0.1), Ns=0),
    "mirror": dict(Ka=(0.1, 0.1, 0.1), Kd=(0.1, 0.1, 0.1), Ks=(0.5, 0.5, 0.5), Ns=0, Refl=0.6),
    "glass": dict(Ka=(0.05, 0.05, 0.05), Kd=(0.05, 0.05, 0.05), Ks=(0.4, 0.4, 0.4), Ns=0, Tr=0.7,
                  Tf=(0.9, 0.95, 1.0), Ni=1.5),
    "red": dict(Ka=(0.75, 0.15, 0.15), Kd=(0.75, 0.15, 0.15), Ks=(0.0, 0.0, 0.0), Ns=0),
    "blue": dict(Ka=(0.2, 0.3, 0.8), Kd=(0.2, 0.3, 0.8), Ks=(0.3, 0.3, 0.3), Ns=0),
    "ball": dict(Ka=(0.5, 0.4, 0.2), Kd=(0.5, 0.4, 0.2), Ks=(0.3, 0.3, 0.3), Ns=0, Refl=0.3),
}
ORDER = ("Ka", "Kd", "Ks", "Ns", "Refl", "Tr", "Tf", "Ni")
SHINY = ("floor", "wall", "mirror", "glass", "blue", "ball")   # the materials with Ks > 0

CAMERA = (45.0, 38.0, -62.0, 8.0, 0.0, 0.0, 80.0)
MAIN = (45.0, 80.0, 45.0)
SIDE = (12.0, 55.0, 8.0)


def _light(pos, amb=(0.1, 0.1, 0.1), dif=(0.8, 0.8, 0.8), spec=(0.5, 0.5, 0.5)):
    return tuple(float(v) for v in tuple(pos) + tuple(amb) + tuple(dif) + tuple(spec))


LIGHTS = [_light(MAIN), _light(SIDE, (0.05, 0.1, 0.02), (0.5, 0.4, 0.6), (0.3, 0.5, 0.2))]
# the coefficient cases: a contribution of Refl^2 or Refl^3 has to reach a byte, so the lights are bright
BRIGHT = [_light(MAIN, (0.0, 0.0, 0.0), (400.0, 300.0, 500.0), (100.0, 100.0, 100.0)),
          _light(SIDE, (0.0, 0.0, 0.0), (300.0, 500.0, 400.0), (100.0, 100.0, 100.0))]
NINE = LIGHTS + [_light((10.0 + 9.0 * i, 60.0 + 3.0 * i, 5.0 + 10.0 * i), (0.01, 0.01, 0.01),
                        (0.1 + 0.02 * i, 0.15, 0.2 - 0.02 * i), (0.1, 0.05 * i, 0.1)) for i in range(7)]


def _case(edit=None, normals="unit", lights=None, camera=CAMERA, depth=DEPTH, group="exact", counter=None,
          reference=True):
    return dict(edit=edit or {}, normals=normals, lights=LIGHTS if lights is None else lights, camera=camera,
                depth=depth, group=group, counter=counter, reference=reference)


def _refl(v):
    """Every opaque material a mirror: the coefficient reaches the last level undecayed along every path."""
    return {m: {"Refl": v} for m in ("mirror", "floor", "wall", "ball")}


def _ns(v):
    return {m: {"Ns": v} for m in SHINY}


CASES = {
    "base": _case(counter="lit_hits"),
    # ---- reflectance (on the two mirrors)
    "refl_0.01": _case({"mirror": {"Refl": 0.01}}, lights=BRIGHT, counter="coef_is_0.01"),
    "refl_0.1": _case({"mirror": {"Refl": 0.1}, "floor": {"Refl": 0.1}, "ball": {"Refl": 0.1}}, lights=BRIGHT,
                      counter="coef_just_above_0.01"),
    "refl_1": _case(_refl(1.0), counter="coef_undecayed_at_depth"),
    "refl_1.5": _case(_refl(1.5), counter="coef_undecayed_at_depth"),
    "refl_neg": _case({"mirror": {"Refl": -0.5}}, counter="refl_negative_hits"),
    "refl_denormal": _case({"mirror": {"Refl": 5e-324}}, counter="refl_denormal_children"),
    # ---- transparency (on the panes)
    "tr_1": _case({"glass": {"Tr": 1.0}}, counter="occluders_hostile_tr"),
    "tr_2": _case({"glass": {"Tr": 2.0}}, counter="occluders_hostile_tr"),
    "tr_neg": _case({"glass": {"Tr": -0.25}}, counter="occluders_negative_tr"),
    "tr_negzero": _case({"glass": {"Tr": -0.0}}, counter="occluders_negative_zero_tr"),
    "tr_1e-300": _case({"glass": {"Tr": 1e-300}}, counter="occluders_hostile_tr"),
    "tf_0.002": _case({"glass": {"Tr": 0.5, "Tf": (0.002, 0.002, 0.002)}}, counter="dim_at_exactly_0.001"),
    "tf_0.0021": _case({"glass": {"Tr": 0.5, "Tf": (0.002, 0.002, 0.0021)}}, counter="one_channel_above_0.001"),
    "tf_0": _case({"glass": {"Tf": (0.0, 0.0, 0.0)}}, counter="occluders_hostile_tr"),
    "tf_3": _case({"glass": {"Tf": (3.0, 3.0, 3.0)}}, counter="power_above_1"),
    "tf_neg": _case({"glass": {"Tf": (-1.0, 1.0, 1.0)}}, counter="power_negative"),
    "refl_1_tr_1": _case({"glass": {"Refl": 1.0, "Tr": 1.0}}, counter="rays_with_both_children"),
    # ---- the specular exponent: the pow group
    "ns_0.5": _case(_ns(0.5), group="pow", counter="specular_terms"),
    "ns_1e4": _case(_ns(1e4), group="pow", counter="specular_terms"),
    "ns_neg2": _case(_ns(-2.0), group="pow", counter="specular_terms"),
    # ---- colours
    "ka_3": _case({"wall": {"Ka": (3.0, 3.0, 3.0)}, "floor": {"Ka": (3.0, 3.0, 3.0)}}, counter="ka_above_1_hits"),
    "kd_neg": _case({"floor": {"Kd": (-1.0, -1.0, -1.0)}}, counter="kd_negative_hits"),
    "ks_0": _case({m: {"Ks": (0.0, 0.0, 0.0)} for m in SHINY}, counter="lit_hits"),
    # ---- the refraction index: partial_res is computed and never used, the frame is the base's
    "ni_0": _case({"glass": {"Ni": 0.0}}, counter="glass_hits"),
    "ni_1": _case({"glass": {"Ni": 1.0}}, counter="glass_hits"),
    "ni_1e300": _case({"glass": {"Ni": 1e300}}, counter="glass_hits"),
    # ---- normals
    "vn_x0.01": _case(normals="x0.01", counter="normals_not_unit"),
    "vn_x100": _case(normals="x100", counter="refl_dot_above_1"),
    "vn_negated": _case(normals="negated", counter="flips"),
    "vn_fan_inconsistent": _case(normals="fan", counter="normals_nearly_zero"),
    "vn_mirror_zero": _case(normals="mirror0", counter="normals_zero"),
    # the back wall's vn lies IN the wall, along x: the pixel column whose rays have an x component of exactly zero
    # (yaw and roll are 0) meets it with normal_ray_dot = 0, where `< 0.0` and `<= 0.0` part
    "vn_wall_sideways": _case(normals="sideways", counter="normal_ray_dot_is_zero"),
    # ---- lights
    "light_in_stack": _case(lights=[_light((45.0, 30.0, 45.0)), LIGHTS[1]], counter="ended_behind_the_light"),
    "light_1e-6_above_pane": _case(lights=[_light((45.0, 40.000001, 45.0)), LIGHTS[1]],
                                   counter="light_within_1e-5_of_start"),
    # (1e-6 is further than the 1e-7 the loop steps past an occluder, so there the NEXT ray starts beyond the light;
    # at 5e-8 the step itself passes the light and the SqrDistance comparison of :141-145 ends the loop)
    "light_5e-8_above_pane": _case(lights=[_light((45.0, 40.00000005, 45.0)), LIGHTS[1]], counter="ended_past_the_light"),
    "light_at_camera": _case(lights=[_light(CAMERA[:3]), LIGHTS[1]], counter="lit_hits"),
    "light_behind_wall": _case(lights=[_light((45.0, 40.0, 96.0)), LIGHTS[1]], counter="ended_opaque"),
    "light_ambient_above_power": _case(lights=[_light(MAIN, (1.5, 1.25, 2.0)), LIGHTS[1]], counter="ambient_above_power"),
    "nine_lights": _case(lights=NINE, counter="lit_hits"),
    # ---- combined
    "combined_mirrors": _case(dict(_refl(1.0), glass={"Tr": -0.25}), normals="x100", counter="refl_dot_above_1"),
    "combined_panes": _case({"glass": {"Refl": 1.0, "Tr": 2.0, "Tf": (-1.0, 1.0, 3.0)}, "floor": {"Kd": (-1.0, -1.0, -1.0)}},
                            normals="negated", lights=[_light((45.0, 30.0, 45.0), (1.5, 1.25, 2.0)), LIGHTS[1]],
                            counter="ended_behind_the_light"),
    # Tr -0.25 alone leaves `lp` negative after one pane, and the loop then ends as if the pane were opaque (:149-155);
    # with a negative filter as well `lp` stays positive and the negative Tr is seen to be transparent
    "combined_tr_neg_tf_neg": _case({"glass": {"Tr": -0.25, "Tf": (-1.0, -1.0, -1.0)}}, counter="occluders_negative_tr"),
    "combined_dim": _case({"glass": {"Tr": 0.5, "Tf": (0.002, 0.002, 0.002)}, "mirror": {"Refl": 0.01}}, normals="fan",
                          lights=BRIGHT, counter="dim_at_exactly_0.001"),
    "combined_pow": _case(dict(_ns(0.5), mirror={"Ns": 0.5, "Refl": 1.5}, glass={"Ns": 0.5, "Tr": -0.25}), normals="negated",
                          lights=NINE, group="pow", counter="specular_terms"),
    # ---- deeper than the reference can go (its limit is a compile-time 5): the oracle alone
    "depth_16": _case(depth=16, counter="rays_below_layer_5", reference=False),
}
NI_CASES = ("ni_0", "ni_1", "ni_1e300")
NORMAL_VARIANTS = ("unit", "x0.01", "x100", "negated", "fan", "mirror0", "sideways")


# ---------------------------------------------------------------------------------------------------------- the text

def _num(v):
    return repr(float(v))


def mtl_text(edit):
    out = ["# hostile scene family: materials"]
    for name, base in BASE.items():
        values = dict(base)
        values.update(edit.get(name, {}))
        out.append("newmtl %s" % name)
        for key in ORDER:
            if key in values:
                out.append("%s %s" % (key, " ".join(_num(v) for v in np.atleast_1d(values[key]))))
    assert set(edit) <= set(BASE), edit
    return "\n".join(out) + "\n"


def table(edit):
    """The 16 values per material (ka kd ks ns refl tr tf ni) of a case's table, in BASE's order: what the .mtl says."""
    out = np.zeros((len(BASE), 16))
    at = {"Ka": 0, "Kd": 3, "Ks": 6, "Ns": 9, "Refl": 10, "Tr": 11, "Tf": 12, "Ni": 15}
    for i, (name, base) in enumerate(BASE.items()):
        values = dict(base)
        values.update(edit.get(name, {}))
        for key, v in values.items():
            v = np.atleast_1d(np.asarray(v, dtype=np.float64))
            out[i, at[key]:at[key] + len(v)] = v
    return out


def obj_text(normals="unit"):
    """The geometry with one of NORMAL_VARIANTS.  Triangles only; 160 of them."""
    assert normals in NORMAL_VARIANTS, normals
    scale = {"x0.01": 0.01, "x100": 100.0, "negated": -1.0}.get(normals, 1.0)
    w = scenegen.ObjWriter("hostile.mtl")
    rng = scenegen.SplitMix64(SEED)

    def vn(n, part=None, k=0):
        n = [c * scale for c in n]
        if normals == "mirror0" and part == "mirror":
            n = [0.0, 0.0, 0.0]
        if normals == "sideways" and part == "wall":
            n = [1.0, 0.0, 0.0]
        if normals == "fan" and part == "fan" and k % 2:
            n = [-c for c in n]
        w.lines.append("vn " + " ".join(_num(c + 0.0) for c in n))
        w.nn += 1
        return w.nn

    def grid(origin, du, dv, nu, nv, normal, part=None):
        n = vn(normal, part)
        idx = [[w.v(*(origin[a] + du[a] * i / nu + dv[a] * j / nv for a in range(3))) for i in range(nu + 1)]
               for j in range(nv + 1)]
        for j in range(nv):
            for i in range(nu):
                a, b, c, d = idx[j][i], idx[j][i + 1], idx[j + 1][i + 1], idx[j + 1][i]
                w.face([(a, None, n), (b, None, n), (c, None, n)])
                w.face([(a, None, n), (c, None, n), (d, None, n)])

    w.usemtl("floor")
    grid((0.0, 0.0, 0.0), (90.0, 0.0, 0.0), (0.0, 0.0, 90.0), 3, 3, (0.0, 1.0, 0.0))
    w.usemtl("wall")
    grid((0.0, 0.0, 90.0), (90.0, 0.0, 0.0), (0.0, 90.0, 0.0), 3, 3, (0.0, 0.0, -1.0), "wall")
    w.usemtl("mirror")  # two mirrors facing each other, turned a little towards the camera
    grid((4.0, 4.0, 15.0), (4.0, 0.0, 70.0), (0.0, 66.0, 0.0), 2, 2, (0.998, 0.0, -0.057), "mirror")
    grid((86.0, 4.0, 15.0), (-4.0, 0.0, 70.0), (0.0, 66.0, 0.0), 2, 2, (-0.998, 0.0, -0.057), "mirror")
    w.usemtl("glass")
    for y in PANE_Y:
        grid((30.0, y, 30.0), (30.0, 0.0, 0.0), (0.0, 0.0, 30.0), 1, 1, (0.0, 1.0, 0.0))
    for k in range(60):  # the cluster: small triangles without normals
        w.usemtl(("red", "blue")[k % 2])
        c = (rng.rng(62.0, 80.0), rng.rng(2.0, 22.0), rng.rng(20.0, 50.0))
        w.face([(w.v(*(c[a] + rng.rng(-2.5, 2.5) for a in range(3))), None, None) for _ in range(3)])
    # the dome: an apex and two rings of 12 on a sphere of radius 17 about (20, 2, 40), normals radial
    w.usemtl("ball")
    centre, radius = (20.0, 2.0, 40.0), 17.0
    ring = []
    count = 0
    for elevation in (90.0, 50.0, 12.0):
        row = []
        for i in range(1 if elevation == 90.0 else 12):
            a = 2.0 * math.pi * i / 12
            e = math.radians(elevation)
            n = (math.cos(e) * math.cos(a), math.sin(e), math.cos(e) * math.sin(a))
            n = tuple(round(c, 6) for c in n)
            row.append((w.v(*(centre[a_] + radius * n[a_] for a_ in range(3))), None, vn(n, "fan", count)))
            count += 1
        ring.append(row)
    for i in range(12):
        j = (i + 1) % 12
        w.face([ring[0][0], ring[1][i], ring[1][j]])
        w.face([ring[1][i], ring[2][i], ring[2][j]])
        w.face([ring[1][i], ring[2][j], ring[1][j]])
    return w.text()


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def pinned():
    return json.load(open(JSON))


def write(name, out_dir, check=True):
    """Writes <out_dir>/<name>/hostile.obj and hostile.mtl of a case and returns the .obj's path.  check: the text is
    what tests/golden/hostile.json pins."""
    c = CASES[name]
    d = os.path.join(out_dir, name)
    os.makedirs(d, exist_ok=True)
    obj, mtl = obj_text(c["normals"]), mtl_text(c["edit"])
    if check:
        pin = pinned()
        assert pin["obj_sha256"][c["normals"]] == sha(obj), "hostile geometry drifted (%s)" % c["normals"]
        assert pin["cases"][name]["mtl_sha256"] == sha(mtl), "hostile materials drifted (%s)" % name
    for fn, text in (("hostile.obj", obj), ("hostile.mtl", mtl)):
        with open(os.path.join(d, fn), "w", newline="\n") as f:
            f.write(text)
    return os.path.join(d, "hostile.obj")


def golden_path(name):
    return os.path.join(HERE, "golden", "hostile_%s.npz" % name)


def load_golden(name):
    """The reference's answer for a case: cam, lights, depth, rgb, line, point.  A file whose `point_of` names another
    case holds no point plane of its own: the maker found the reference's plane bit-identical to that case's (the
    primary hits depend on the camera and the triangles alone)."""
    g = dict(np.load(golden_path(name), allow_pickle=False))
    assert str(g["made_by"]).startswith("reference"), g["made_by"]
    if "point" not in g:
        g["point"] = np.load(golden_path(str(g["point_of"])), allow_pickle=False)["point"]
    return g


# ------------------------------------------------------------------------------------------------- does the case bite

def bite(orc, tree, lights):
    """Counts, over a restated tree (raytree_ref.build) of a case, the rays at which each comparison is decided by an
    unusual value: {counter name: count}.  A case's own counter is CASES[name]["counter"]."""
    mats = orc.materials()
    names = [m[0] for m in mats]
    L = np.asarray(lights, dtype=np.float64).reshape(-1, 12)
    out = dict.fromkeys(set(c["counter"] for c in CASES.values()), 0)
    shadow = lr.oracle_intersector(orc)
    for level, lay in enumerate(tree["layers"]):
        n = len(lay["ray"])
        lit = (lay["prim"] >= 0) & (lay["material"] >= 0)
        values = np.array([mats[m][1] if m >= 0 else np.zeros(16) for m in lay["material"]]).reshape(n, 16)
        mname = np.array([names[m] if m >= 0 else "" for m in lay["material"]])
        refl, tr = values[:, 10], values[:, 11]
        deeper = level < tree["max_depth"]
        could = lit & deeper & (refl > 0.0) & (lay["in_object"] == 0)
        out["lit_hits"] += int(lit.sum())
        out["coef_is_0.01"] += int((could & (lay["coef"] == 0.01)).sum())
        out["coef_just_above_0.01"] += int((could & (lay["coef"] > 0.01) & (lay["coef"] <= 0.0100000001)).sum())
        if level == tree["max_depth"]:
            out["coef_undecayed_at_depth"] += int((lit & (lay["coef"] >= 1.0)).sum())
        out["refl_negative_hits"] += int((lit & deeper & (refl < 0.0) & (lay["in_object"] == 0) & (lay["coef"] > 0.01)).sum())
        out["refl_denormal_children"] += int(((lay["child_refl"] >= 0) & (refl > 0.0) & (refl < 2.3e-308)).sum())
        out["rays_with_both_children"] += int(((lay["child_refl"] >= 0) & (lay["child_refr"] >= 0)).sum())
        out["glass_hits"] += int((lit & (mname == "glass")).sum())
        out["ka_above_1_hits"] += int((lit & (values[:, 0] > 1.0)).sum())
        out["kd_negative_hits"] += int((lit & (values[:, 3] < 0.0)).sum())
        if level > 5:
            out["rays_below_layer_5"] += n
        # the normals as the planes hold them, before the flip
        d = lay["ray"][:, 3:]
        nrm = lay["normal"]
        length = np.sqrt(lr._dot(nrm, nrm))
        with np.errstate(invalid="ignore"):
            out["normals_not_unit"] += int((lit & (length > 0.0) & (np.abs(length - 1.0) > 0.5)).sum())
            out["normals_nearly_zero"] += int((lit & (mname == "ball") & (length < 0.25)).sum())
            out["normals_zero"] += int((lit & (mname == "mirror") & (length == 0.0)).sum())
            nrd = lr._dot(nrm, -d)
            out["flips"] += int((lit & (nrd < 0.0)).sum())
            out["normal_ray_dot_is_zero"] += int((lit & (nrd == 0.0) & (length > 0.0)).sum())
            flipped = np.where((nrd < 0.0)[:, None], -nrm, nrm)
            reflected = d - flipped * (2 * lr._dot(d, flipped))[:, None]
            refl_dot = lr._dot(reflected, -d)
            out["refl_dot_above_1"] += int((lit & (refl_dot > 1.0)).sum())
            out["refl_dot_is_zero"] = out.get("refl_dot_is_zero", 0) + int((lit & (refl_dot == 0.0)).sum())
            spec = lit & (refl_dot > 0) & (values[:, 6:9] != 0.0).any(axis=1)
        out["specular_terms"] += int((spec[None, :] & (lay["in_shadow"] == 0)).sum())
        with np.errstate(invalid="ignore"):
            out["power_above_1"] += int((lay["power"] > 1.0).any(axis=2).sum())
            out["power_negative"] += int((lay["power"] < 0.0).any(axis=2).sum())
            out["ambient_above_power"] += int((lay["power"] < L[:, None, 3:6]).any(axis=2).sum())
        ends = {}
        sl = lr.shadow_loops(shadow, lay["point"].reshape(1, n, 3), lit.reshape(1, n), L, info=ends)
        assert np.array_equal(sl["in_shadow"].reshape(len(L), n), lay["in_shadow"])
        for key in ("ended_behind_the_light", "ended_past_the_light", "ended_opaque", "light_within_1e-5_of_start",
                    "occluders_negative_tr", "occluders_negative_zero_tr", "occluders_hostile_tr",
                    "dim_at_exactly_0.001", "one_channel_above_0.001", "t_equals_light_distance"):
            out[key] = out.get(key, 0) + ends[key]
    return out


# --------------------------------------------------------------------------------- the truths, made once per session

class Family:
    """name -> the case's files, its oracle scene, the oracle's frame (rgb, line, point, counters at the case's depth)
    and the restated tree; made on first use and then left unchanged."""

    def __init__(self, out_dir):
        self.out_dir = out_dir
        self.made = {}

    def __call__(self, name):
        if name not in self.made:
            import orclib
            import raytree_ref as rr
            c = CASES[name]
            obj = write(name, self.out_dir)
            orc = orclib.OracleScene(obj)
            orc.set_lights(c["lights"])
            want = orc.render(c["camera"], W, H, max_level=c["depth"], debug=True)
            tree = rr.build(orc, c["camera"], W, H, c["lights"], c["depth"])
            self.made[name] = dict(c, name=name, obj=obj, orc=orc, want=want, tree=tree)
        return self.made[name]


def first_difference(tree_a, tree_b):
    """The lowest (layer, ray) at which two restated trees of the same frame give a ray different children, or None:
    down to that layer the two hold the same rays."""
    for k, (a, b) in enumerate(zip(tree_a["layers"], tree_b["layers"])):
        assert len(a["ray"]) == len(b["ray"])
        bad = np.nonzero(((a["child_refl"] >= 0) != (b["child_refl"] >= 0)) |
                         ((a["child_refr"] >= 0) != (b["child_refr"] >= 0)))[0]
        if len(bad):
            return (k, int(bad[0]))
    assert len(tree_a["layers"]) == len(tree_b["layers"])
    return None
