"""The model of an EDIT SESSION: one uploaded scene and its stored ray trees kept alive through chains of material,
texture and light edits (mt_scene_set_materials, mt_scene_set_texture, mt_scene_set_lights, mt_raytree_update_materials,
mt_raytree_regrow_materials, mt_raytree_update_lights; include/mythtracer_hip.h) -- shared by
tests/test_edit_sessions_cpu.py, which pins the model and its inputs with the oracle alone, and
tests/test_gpu_edit_sessions.py, which holds the live scene to it after every call.  Test infrastructure: numpy and the
oracle only.

The scene is the tiny scene of tests/texture_edit_ref.py at 48 x 32, depth 5, under TINY_LIGHTS, with its third texture
(the spare one no material uses) in the table.

  STATE      what the scene holds: the materials table (5 x 16 values), tex_of, three texel arrays, the two lights, and
             the two generations the header describes (`gen` moves with every material edit that changes a bit and with
             every texture set; `tex_gen[i]` with every set of texture i).  Ops are pure functions on it (`apply`).
  TREE       per stored tree: the state it was last synced to, whether it keeps uvw, the position every light's planes
             hold (None where the documented MIXED case left kept rays at the old position and traced rays at the new
             one), and the tree as the documented rules ASSEMBLE it from the tree of the step before (`tree`).
  predict    what the header says a call must return, in the header's order of checks.
  truth      raytree_ref.build / raylist_ref.build_from_rays on an OracleScene BUILT from the synced state, under the
             positions the tree's planes hold, plus the uvw plane from the oracle's intersection answer.
  chained    regrow_ref.regrow for regrows and the commit rule for same-shape updates, both extended to retextured
             materials by texture_edit_ref.albedo on the carried uvw.  tests/test_edit_sessions_cpu.py holds it to `truth`
             in every plane of every layer at every sync of every session and seed, so the two are interchangeable
             wherever both exist; `predict` reads the assembled tree, which also exists in the mixed case.

The three newer edit kinds -- mt_scene_set_triangle_materials, mt_scene_set_triangle_normals, mt_scene_set_triangle_uvw --
are ops too ("assign", "normals", "uvws"), and NEW_TREES are the trees that keep tri, uvw, both or neither.  The state
holds the assignment, the two attribute arrays (AddPrimitive numbering, 12 triangles), the assignment generation, the
two attribute generations and the per-triangle stamps; `build_scene` builds all of them into the scene, so the truth is
still a BUILT scene.  `chained` is NOT extended to the new kinds: a tree that keeps tri, and every tree once a new-kind op
has happened, is taken from `truth` after a successful sync (the generator keeps the rule that no light moves while a
tracing regrow may be pending, so the truth under the positions the planes hold is defined); kept / traced / dropped and
renormaled / reuvwed / respawned come from vertex_attr_ref.match between the tree before and the truth after.
"""
import numpy as np

import assign_ref as ar
import material_edit_ref as me
import orclib
import raylist_ref as rl
import raytree_ref as rr
import raytree_update_ref as ru
import regrow_ref as rg
import texture_edit_ref as te
import vertex_attr_ref as va

W, H = te.TINY_IMAGE
CAM = te.TINY_CAMERA
DEPTH = 5
OFF_GRID = (7, 5, 33, 22)
LIST_W = 64
FLOOR, WALL, MIRROR, PANE, MATTE = te.FLOOR, te.WALL, te.MIRROR, te.PANE, te.MATTE
NAMES = [m[0] for m in te.TINY_MATERIALS]
# the scene DESCRIPTION numbers the materials by their first use in a triangle (MythTracer.flatten()): material g of the
# description is DENSE[g] of the table.  The model speaks the table's numbering, the oracle's, everywhere; only the
# order in which the library meets the materials -- the "first" material a refusal names -- follows DENSE.
DENSE = list(dict.fromkeys(t[3] for t in te.tiny_triangles()))
# the four trees of a session: name -> (chunk or None for the frame or "list" for the 64 x 1 ray list, keeps uvw)
TREES = {"full": (None, True), "chunk": (OFF_GRID, True), "list": ("list", True), "plain": (None, False)}
PLANES = me.PLANES + ("uvw",)
OUTCOMES = ("ok", "ok_nothing_to_do", "unsupported_shape", "unsupported_textured", "unsupported_texture_set", "stale")
SHADE_ONLY = ("Kd", "Ks", "Ns", "Ni")
# the trees of the sessions with the newer edit kinds: name -> (chunk / None / "list", keeps uvw, keeps tri)
NEW_TREES = {"full_tu": (None, True, True), "chunk_tu": (OFF_GRID, True, True), "list_tu": ("list", True, True),
             "full_t": (None, False, True), "full_u": (None, True, False), "full_0": (None, False, False)}
NEW_OUTCOMES = ("unsupported_no_tri", "unsupported_textured_target", "unsupported_attr_no_tri", "unsupported_normals")
N_TRIS = len(te.tiny_triangles())
ATTR_NAMES = ("normal", "uvw")  # as the library's messages name them
ATTR_COUNTS = ("renormaled", "reuvwed", "respawned")


def tree_def(name):
    """(spec, keeps uvw, keeps tri) of a tree of TREES or NEW_TREES."""
    return TREES[name] + (False,) if name in TREES else NEW_TREES[name]


# the node-stream index of every triangle, by AddPrimitive index: pinned here so that the predicted refusals do not take
# their numbers from the product (on this scene the stream keeps the order in which the triangles were added).  The CPU test holds the
# facade's flatten() to it, the GPU test the description's tri_id.
STREAM_ORDER = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)


def stream_of():
    """{AddPrimitive index: node-stream index} of the tiny scene's triangles: the numbering of the library's messages
    and of the tri plane."""
    return dict(enumerate(STREAM_ORDER))


# ---- the state and its ops

def start_state():
    mats = []
    for _, ka, kd, ks, ns, refl, tr, tf in te.TINY_MATERIALS:
        mats.append(np.array(list(ka) + list(kd) + list(ks) + [ns, refl, tr] + list(tf) + [1.0], dtype=np.float64))
    tris = te.tiny_triangles()
    return dict(mats=mats, tex_of=[0, 1, -1, -1, -1], texs=te.tiny_textures(), lights=[tuple(l) for l in te.TINY_LIGHTS],
                gen=0, tex_gen=[0, 0, 0],
                tri_mtl=[int(t[3]) for t in tris], normals=np.array([t[1] for t in tris], dtype=np.float64),
                uvws=np.array([t[2] for t in tris], dtype=np.float64), asg_gen=0, attr_gen=[0, 0],
                stamp=[np.zeros(len(tris), dtype=np.int64), np.zeros(len(tris), dtype=np.int64)])


ORIGINAL_TEXELS = te.tiny_textures()


def texels_of(index, key):
    """The texel array an op ("tex", index, key) sets: texture_edit_ref.replacements of texture `index`'s original."""
    return te.replacements(ORIGINAL_TEXELS[index])[key]


def same_look(a, b):
    """Two states hold the same materials, tex_of and texels, bit for bit."""
    return (all(x.tobytes() == y.tobytes() for x, y in zip(a["mats"], b["mats"])) and a["tex_of"] == b["tex_of"] and
            all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a["texs"], b["texs"])) and
            a["tri_mtl"] == b["tri_mtl"] and a["normals"].tobytes() == b["normals"].tobytes() and
            a["uvws"].tobytes() == b["uvws"].tobytes())


def apply(state, op):
    """The state after `op`, a new dict; the ops:
      ("mat", i, {MTL keyword: value})   fields of material i (material_edit_ref.FIELDS' keywords)
      ("tex", i, key)                    texture i set to texels_of(i, key): size and format may change
      ("tex_move", material, index)      the material's tex, -1 for none
      ("move_light", i, (x, y, z))
      ("colour_light", i, (nine numbers: ambient, diffuse, specular))
      ("set_lights", [lights])           the whole list, another count allowed
      ("assign", {triangle: material or -1})    the triangles' materials (AddPrimitive and table numbering)
      ("normals", {triangle: (3, 3)})           the triangles' three normals
      ("uvws", {triangle: (3, 3)})              the triangles' three texture coordinates
    The generations move as the scene's do: a material edit that changes no bit moves none, a texture set always does;
    a reassignment that changes an entry bumps asg_gen and gen; an attribute set bumps its generation and gen only if
    some triangle's 9 doubles differ by their bits, and stamps those triangles alone with the new generation."""
    s = dict(state, mats=[m.copy() for m in state["mats"]], tex_of=list(state["tex_of"]), texs=list(state["texs"]),
             lights=list(state["lights"]), tex_gen=list(state["tex_gen"]), attr_gen=list(state["attr_gen"]),
             stamp=list(state["stamp"]))
    kind = op[0]
    if kind == "assign":
        now = list(s["tri_mtl"])
        for t, m in op[1].items():
            assert -1 <= int(m) < len(s["mats"])
            now[t] = int(m)
        if now != s["tri_mtl"]:
            s["tri_mtl"] = now
            s["asg_gen"] += 1
            s["gen"] += 1
    elif kind in ("normals", "uvws"):
        w = 0 if kind == "normals" else 1
        now = s[kind].copy()
        for t, v in op[1].items():
            now[t] = np.asarray(v, dtype=np.float64).reshape(3, 3)
        changed = va.changed_triangles(s[kind], now)
        if len(changed):
            s[kind] = now
            s["attr_gen"][w] += 1
            s["gen"] += 1
            stamp = s["stamp"][w].copy()
            stamp[changed] = s["attr_gen"][w]
            s["stamp"][w] = stamp
    elif kind == "mat":
        s["mats"][op[1]] = me.expected_values(s["mats"][op[1]], op[2])
    elif kind == "tex":
        s["texs"][op[1]] = np.array(texels_of(op[1], op[2]), copy=True)
        s["tex_gen"][op[1]] += 1
        s["gen"] += 1
    elif kind == "tex_move":
        s["tex_of"][op[1]] = int(op[2])
    elif kind == "move_light":
        s["lights"][op[1]] = tuple(float(v) for v in op[2]) + tuple(s["lights"][op[1]][3:])
    elif kind == "colour_light":
        assert len(op[2]) == 9
        s["lights"][op[1]] = tuple(s["lights"][op[1]][:3]) + tuple(float(v) for v in op[2])
    elif kind == "set_lights":   # the whole list: the COUNT may change (scripted sessions only)
        s["lights"] = [tuple(float(v) for v in l) for l in op[1]]
    else:
        raise ValueError(op)
    if kind in ("mat", "tex_move"):
        same = all(x.tobytes() == y.tobytes() for x, y in zip(s["mats"], state["mats"])) and s["tex_of"] == state["tex_of"]
        if not same:
            s["gen"] += 1
    return s


def net_noop(before, after):
    return same_look(before, after) and before["lights"] == after["lights"]


def positions(state):
    return [tuple(l[:3]) for l in state["lights"]]


def flat_materials(state):
    """The tables as mt_scene_set_materials takes them (flat["materials"] of MythTracer.flatten())."""
    return [dict(values=v.copy(), tex=int(t)) for v, t in zip(state["mats"], state["tex_of"])]


def oracle_materials(state):
    """The tables as OracleScene.materials() gives them."""
    return [(n, v.copy(), int(t)) for n, v, t in zip(NAMES, state["mats"], state["tex_of"])]


def table(state):
    """The materials in TINY_MATERIALS' form with the refraction index, for texture_edit_ref.build_tiny."""
    return [(n, v[0:3], v[3:6], v[6:9], float(v[9]), float(v[10]), float(v[11]), v[12:15], float(v[15]))
            for n, v in zip(NAMES, state["mats"])]


def build_scene(scene, state):
    """The tiny scene BUILT from a state, on an OracleScene or a MythTracer: every triangle is added with the state's
    normals, texture coordinates and material (vertex_attr_ref.build_tiny's wrapping, with a material override)."""
    real = scene.add_triangle
    count = [0]

    def add_triangle(v, n, t, mtl=-1, line_no=0):
        i = count[0]
        count[0] += 1
        return real(v, state["normals"][i].tolist(), state["uvws"][i].tolist(), mtl=state["tri_mtl"][i], line_no=line_no)
    scene.add_triangle = add_triangle
    try:
        te.build_tiny(scene, textures=state["texs"], tex_of=dict(enumerate(state["tex_of"])), materials=table(state))
    finally:
        del scene.add_triangle
    assert count[0] == N_TRIS
    return scene


_oracles = {}


def look_key(state):
    return (b"".join(m.tobytes() for m in state["mats"]), tuple(state["tex_of"]),
            tuple((t.dtype.str, t.shape, t.tobytes()) for t in state["texs"]),
            tuple(state["tri_mtl"]), state["normals"].tobytes(), state["uvws"].tobytes())


def oracle(state):
    """An OracleScene built from the state's description (cached by the description), under the state's lights."""
    key = look_key(state)
    if key not in _oracles:
        _oracles[key] = build_scene(orclib.OracleScene(), state)
    _oracles[key].set_lights(state["lights"])
    return _oracles[key]


def oracle_frame(state, depth=DEPTH, chunk=None, held=None):
    """The oracle's frame of a state; held: light positions that replace the state's (a tree's)."""
    orc = oracle(state)
    if held is not None:
        orc.set_lights(lights_at(state, held))
    return orc.render(CAM, W, H, chunk=chunk, max_level=depth)["rgb"]


# ---- truth

_truths = {}


def lights_at(state, held):
    """The state's lights with the positions `held` (None: the state's own)."""
    return [tuple(p if p is not None else l[:3]) + tuple(l[3:]) for l, p in zip(state["lights"], held)]


def truth_tree(state, spec, held, rays=None):
    """The restated tree of a tree definition under a state's materials and textures and the light positions `held`:
    spec = a chunk, None for the frame, or "list" with rays = (rays (64, 6), in_object, coef).  With the uvw plane:
    Triangle::GetUVW from the oracle's intersection answer, NaN for a miss."""
    lights = lights_at(state, held)
    key = (look_key(state), tuple(l[:3] for l in lights), spec if spec != "list" else ("list", rays[0].tobytes()))
    if key in _truths:
        return _truths[key]
    orc = oracle(state)
    if spec == "list":
        tree = rl.build_from_rays(orc, rays[0], LIST_W, 1, lights, DEPTH, in_object=rays[1], coef=rays[2])
    else:
        tree = rr.build(orc, CAM, W, H, lights, DEPTH, chunk=spec)
    for lay in tree["layers"]:
        r = orc.intersect(lay["ray"])
        assert np.array_equal(r["tri"], lay["prim"])
        uvw = r["uvw"].copy()
        uvw[r["tri"] < 0] = np.nan
        lay["uvw"] = uvw
        lay["tri"] = np.asarray(r["tri"], dtype=np.int64).copy()  # (AddPrimitive numbering; stream_of() gives the kernel's)
    _truths[key] = tree
    return tree


def copy_tree(tree):
    out = dict(layers=[{k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in lay.items() if k != "refused"}
                       for lay in tree["layers"]], max_depth=tree["max_depth"])
    out["n_rays"] = [len(l["ray"]) for l in out["layers"]]
    return out


def planes_of(tree, keep_uvw=True, keep_tri=False):
    """The planes a read-back holds, per layer, of a restated or assembled tree."""
    out = []
    for k, lay in enumerate(tree["layers"]):
        names = [p for p in PLANES if keep_uvw or p != "uvw"] + (["tri"] if keep_tri else []) + (["pixel"] if k == 0 else [])
        out.append({p: lay[p] for p in names})
    return out


def differing_planes(a, b, keep_uvw=True, keep_tri=False):
    """[(layer, plane)] that differ in a bit between two trees (raytree_update_ref.same_plane: doubles by bits with
    NaN = NaN); every plane of a layer the other tree does not have counts."""
    pa, pb = planes_of(a, keep_uvw, keep_tri), planes_of(b, keep_uvw, keep_tri)
    bad = [(k, "missing") for k in range(min(len(pa), len(pb)), max(len(pa), len(pb)))]
    for k, (x, y) in enumerate(zip(pa, pb)):
        for name in x:
            same = ru.same_plane(x[name], y[name]) if x[name].dtype == y[name].dtype else \
                ru.same_plane(np.asarray(x[name], dtype=np.int64), np.asarray(y[name], dtype=np.int64))
            if not same:
                bad.append((k, name))
    return bad


def changed_rays(a, b):
    """{plane: most rays of one layer whose value differs} between two trees of one shape; where the shapes differ,
    {"shape": the difference in rays}."""
    if a["n_rays"] != b["n_rays"]:
        return {"shape": sum(abs(x - y) for x, y in zip(a["n_rays"] + [0] * 6, b["n_rays"] + [0] * 6))}
    out = {}
    for x, y in zip(a["layers"], b["layers"]):
        for name in PLANES:
            p, q = np.asarray(x[name]), np.asarray(y[name])
            if p.dtype == np.float64:
                d = (p.view(np.uint64) != q.view(np.uint64)) & ~(np.isnan(p) & np.isnan(q))
            else:
                d = p != q
            if name in ("power", "in_shadow"):
                d = np.moveaxis(d, 0, -1) if d.ndim > 1 else d
            n = int(d.reshape(len(x["ray"]), -1).any(axis=1).sum())
            if n:
                out[name] = max(out.get(name, 0), n)
    return out


# ---- what an edit asks of a tree (diff_materials and the texture generations of mt_capi.hip, from the header's words)

def diff(was, now):
    """dict(shape, shadow, albedo_changed per material, textured = the first material of rule (a) or None, texture_set =
    (texture, first material that uses it) of rule (b) or None)."""
    n = len(now["mats"])
    out = dict(shape=False, shadow=False, albedo_changed=np.zeros(n, dtype=bool), textured=None, texture_set=None)
    for i in DENSE:
        a, b = was["mats"][i], now["mats"][i]
        ta, tb = was["tex_of"][i], now["tex_of"][i]
        if a[0:3].tobytes() != b[0:3].tobytes() or ta != tb:
            out["albedo_changed"][i] = True
            if (ta >= 0 or tb >= 0) and out["textured"] is None:
                out["textured"] = i
        if a[10:12].tobytes() != b[10:12].tobytes():
            out["shape"] = True
    out["shadow"] = rg.shadow_relevant(oracle_materials(was), oracle_materials(now))
    for i in DENSE:
        tb = now["tex_of"][i]
        if tb >= 0 and was["tex_gen"][tb] != now["tex_gen"][tb]:
            out["albedo_changed"][i] = True
            if out["texture_set"] is None:
                out["texture_set"] = (tb, i)
    return out


# ---- the assembled tree

def retextured(lay, mask, state):
    """albedo of the rays in `mask` of a layer under the state's tables, from the carried uvw."""
    i = np.nonzero(mask)[0]
    if len(i):
        uvw = lay["uvw"][i] if "uvw" in lay else None
        lay["albedo"][i] = te.albedo(flat_materials(state), state["texs"], lay["material"][i], uvw)


def chained(prev, fresh, was, now, d, regrown):
    """The tree the documented rules assemble from `prev` (the assembled tree of the step before) for the edit
    was -> now; `fresh` = truth_tree under `now` and the scene's current light positions, read only where the rules
    read the scene: the shape, traced rays, the all-lights re-trace.  d = diff(was, now).
    regrown: regrow_ref.match + regrow_ref.regrow, uvw carried by kept rays and B's for traced ones, then the retexture
    of kept rays; else the commit rule: coef from material_edit_ref.check_pass, albedo of changed materials, the light
    planes from `fresh` where a shadow ray may see the edit."""
    mats_a, mats_b = oracle_materials(was), oracle_materials(now)
    keep_uvw = "uvw" in prev["layers"][0]
    if regrown:
        m = rg.match(prev, fresh, d["shadow"])
        layers = rg.regrow(prev, fresh, m["src"], mats_a, mats_b, d["shadow"])
        for k, (lay, s) in enumerate(zip(layers, m["src"])):
            keep = s >= 0
            if keep_uvw:
                lay["uvw"] = np.array(fresh["layers"][k]["uvw"])
                if keep.any():
                    lay["uvw"][keep] = prev["layers"][k]["uvw"][s[keep]]
            mat = lay["material"]
            retextured(lay, keep & (mat >= 0) & d["albedo_changed"][np.maximum(mat, 0)], now)
    else:
        assert prev["n_rays"] == fresh["n_rays"]
        layers = copy_tree(prev)["layers"]
        coefs = me.check_pass(prev, mats_b)["coef"] if d["shape"] else None
        for k, lay in enumerate(layers):
            if coefs is not None and k > 0:
                lay["coef"] = coefs[k].copy()
            mat = lay["material"]
            retextured(lay, (mat >= 0) & d["albedo_changed"][np.maximum(mat, 0)], now)
            if d["shadow"]:
                lay["power"] = np.array(fresh["layers"][k]["power"])
                lay["in_shadow"] = np.array(fresh["layers"][k]["in_shadow"])
    out = dict(layers=layers, max_depth=DEPTH, n_rays=[len(l["ray"]) for l in layers])
    return out


class Tree:
    """The bookkeeping of one stored tree."""

    def __init__(self, name, state, rays=None):
        self.name = name
        self.spec, self.keep_uvw, self.keep_tri = tree_def(name)
        self.rays = rays
        self.synced = state
        self.held = positions(state)
        self.tree = self._plain(copy_tree(truth_tree(state, self.spec, self.held, rays)))

    def _plain(self, tree):
        for lay in tree["layers"]:
            if not self.keep_uvw:
                lay.pop("uvw", None)
            if not self.keep_tri:
                lay.pop("tri", None)
        return tree

    def stale(self, state):
        return self.synced["gen"] != state["gen"]

    def doomed(self, state):
        """A tree that an edit has put beyond every update.  Without uvw: a texture one of its snapshot's materials
        uses was set; while the material stays with the texture rule (b) refuses the tree, once it leaves rule (a).
        Without tri: a triangle carries an attribute stamp newer than the snapshot."""
        was = self.synced
        if not self.keep_tri and any((state["stamp"][w] > was["attr_gen"][w]).any() for w in (0, 1)):
            return True
        return not self.keep_uvw and any(t >= 0 and was["tex_gen"][t] != state["tex_gen"][t] for t in was["tex_of"])

    def pending(self, state):
        """(CHANGED, [normal-dirty triangles, uvw-dirty triangles]) of the scene state against the tree's snapshot, in
        AddPrimitive numbering: CHANGED compares the assignments themselves (A -> B -> A is empty), the dirty sets are
        the stamps newer than the snapshot's generation (A -> B -> A is dirty)."""
        was = self.synced
        changed = []
        if was["asg_gen"] != state["asg_gen"]:
            changed = [i for i, (a, b) in enumerate(zip(was["tri_mtl"], state["tri_mtl"])) if a != b]
        dirty = [np.nonzero(state["stamp"][w] > was["attr_gen"][w])[0] for w in (0, 1)]
        for w in (0, 1):
            assert bool(len(dirty[w])) == (was["attr_gen"][w] != state["attr_gen"][w])
        return changed, dirty

    def effective(self, state):
        """The stored tree with every ray's material replaced by its triangle's CURRENT one (the header's m')."""
        now = np.array(state["tri_mtl"] + [-1], dtype=np.int64)
        out = dict(self.tree, layers=[dict(lay, material=now[lay["tri"]]) for lay in self.tree["layers"]])
        return out

    def pending_lights(self, state):
        return [i for i, (h, p) in enumerate(zip(self.held, positions(state))) if h != p]

    def settled(self, state):
        """The tree's planes hold the scene's light positions: the shaded tree is the scene's frame."""
        return not self.pending_lights(state)

    def truth(self):
        """The fresh tree of the synced state under the positions the planes hold (not defined in the mixed case)."""
        assert None not in self.held, "mixed light positions: update_lights first"
        return truth_tree(self.synced, self.spec, self.held, self.rays)

    def predict(self, state, call):
        """What `call` -- "update_materials", "regrow", "shade" or ("update_lights", [indices]) -- must return on this
        tree under the scene state `state`: dict(outcome = one of OUTCOMES, ...).  For a sync call that succeeds also
        regrown, kept, traced, dropped, rays_secondary, shaded_hits, rays_shadow, n_rays, and `plan` for commit()."""
        if call == "shade" or call[0] == "update_lights":
            return dict(outcome="stale" if self.stale(state) else "ok")
        assert call in ("update_materials", "regrow")
        n = self.tree["n_rays"]
        nothing = dict(outcome="ok_nothing_to_do", regrown=0, kept=list(n), traced=[0] * len(n), dropped=[0] * len(n),
                       rays_secondary=0, shaded_hits=0, rays_shadow=0, n_rays=list(n), plan=None,
                       renormaled=0, reuvwed=0, respawned=0)
        if not self.stale(state):  # (equal generations: the header's step (2), info all zero but the layer counts)
            return dict(nothing, kept=[0] * len(n))
        d = diff(self.synced, state)
        if d["textured"] is not None and not self.keep_uvw:
            return dict(outcome="unsupported_textured", material=d["textured"])
        if d["texture_set"] is not None and not self.keep_uvw:
            return dict(outcome="unsupported_texture_set", texture=d["texture_set"][0], material=d["texture_set"][1])
        # the reassignment and the attribute edits: the header's refusals, in its order
        changed, dirty = self.pending(state)
        if changed and not self.keep_tri:
            return dict(outcome="unsupported_no_tri", count=len(changed), first=min(stream_of()[i] for i in changed))
        to_textured = [i for i in changed if state["tri_mtl"][i] >= 0 and state["tex_of"][state["tri_mtl"][i]] >= 0]
        if to_textured and not self.keep_uvw:
            i = min(to_textured, key=lambda i: stream_of()[i])
            return dict(outcome="unsupported_textured_target", triangle=stream_of()[i], material=state["tri_mtl"][i])
        for w in (0, 1):
            if len(dirty[w]) and not self.keep_tri:
                return dict(outcome="unsupported_attr_no_tri", attr=ATTR_NAMES[w], count=len(dirty[w]),
                            first=min(stream_of()[int(i)] for i in dirty[w]))
        if changed:
            pairs = [(self.synced["tri_mtl"][i], state["tri_mtl"][i]) for i in changed]
            d["shape"] = True  # (the check pass decides)
            d["shadow"] = d["shadow"] or ar.shadow_visible(self.synced["mats"], state["mats"], pairs)
        normals, uvws = len(dirty[0]) > 0, len(dirty[1]) > 0
        d.update(changed=changed, dirty=dirty, aba=self.synced["asg_gen"] != state["asg_gen"] and not changed)
        # the regrow's check (4), the update's light count check: the lights a tracing launch would read
        lights_read = (d["shape"] or d["shadow"] or normals) if call == "regrow" else d["shadow"]
        if lights_read and len(self.held) > 0 and len(state["lights"]) != len(self.held):
            return dict(outcome="light_count", scene=len(state["lights"]), tree=len(self.held))
        regrown = False
        blocked = 0
        if d["shape"]:
            cp = me.check_pass(self.effective(state) if changed else self.tree, oracle_materials(state))
            if cp["count"] and call == "update_materials":
                return dict(outcome="unsupported_shape", count=cp["count"], first=cp["first"])
            regrown = cp["count"] > 0
        if normals:
            at = [np.nonzero(va.dirty(lay["tri"], dirty[0]) & (lay["child_refl"] >= 0))[0] for lay in self.tree["layers"]]
            blocked = int(sum(len(a) for a in at))
            if blocked and call == "update_materials":
                first = [(k, int(a[0])) for k, a in enumerate(at) if len(a)][0]
                return dict(outcome="unsupported_normals", count=blocked, first=first)
            regrown = regrown or blocked > 0
        if not (d["shape"] or d["albedo_changed"].any() or d["shadow"] or normals or uvws):
            return dict(nothing, plan=(d, False, None))
        fresh = truth_tree(state, self.spec, positions(state), self.rays)
        out = dict(outcome="ok", regrown=int(regrown), plan=(d, regrown, fresh), renormaled=0, reuvwed=0, respawned=0)
        if regrown and self.keep_tri:
            m = va.match(self.tree["layers"], fresh["layers"], dirty[0], dirty[1])
            assert m["blocked"] == blocked
            new = [np.nonzero(s < 0)[0] for s in m["src"]]
            out.update(kept=m["kept"], traced=m["traced"], n_rays=list(fresh["n_rays"]),
                       dropped=[r - (m["kept"][k] if k < len(m["kept"]) else 0) for k, r in enumerate(n)],
                       rays_secondary=int(sum(m["traced"])),
                       shaded_hits=int(sum(int((l["prim"][i] >= 0).sum()) for l, i in zip(fresh["layers"], new))),
                       rays_shadow=int(sum(int(l["iterations"][:, i].sum()) for l, i in zip(fresh["layers"], new))) +
                       (fresh["rays_shadow"] if d["shadow"] else 0))
            out.update({k: m[k] for k in ATTR_COUNTS})
        elif regrown:
            m = rg.match(self.tree, fresh, d["shadow"])
            out.update({k: m[k] for k in ("kept", "traced", "dropped", "rays_secondary", "shaded_hits", "rays_shadow")})
            out["n_rays"] = list(fresh["n_rays"])
        else:
            out.update(kept=list(n), traced=[0] * len(n), dropped=[0] * len(n), rays_secondary=0, shaded_hits=0,
                       rays_shadow=fresh["rays_shadow"] if d["shadow"] else 0, n_rays=list(n))
            if self.keep_tri:
                out["renormaled"] = int(sum(int(va.dirty(lay["tri"], dirty[0]).sum()) for lay in self.tree["layers"]))
                out["reuvwed"] = int(sum(int(va.dirty(lay["tri"], dirty[1]).sum()) for lay in self.tree["layers"]))
        return out

    def commit(self, state, prediction):
        """The bookkeeping after a sync call that returned MT_OK."""
        assert prediction["outcome"] in ("ok", "ok_nothing_to_do")
        plan = prediction["plan"]
        if plan is not None and plan[2] is not None:
            d, regrown, fresh = plan
            now = positions(state)
            if self.keep_tri or state["asg_gen"] or any(state["attr_gen"]):
                # the newer edit kinds: the tree is the truth under the positions its planes then hold (the module's
                # docstring); the mixed case is not modelled here
                assert d["shadow"] or not (regrown and sum(prediction["traced"]) > 0 and self.pending_lights(state))
                held = now if d["shadow"] else self.held
                assert None not in held
                self.tree = self._plain(copy_tree(truth_tree(state, self.spec, held, self.rays)))
            else:
                self.tree = self._plain(chained(self.tree, fresh, self.synced, state, d, regrown))
            if d["shadow"]:
                self.held = now
            elif regrown and sum(prediction["traced"]) > 0:
                self.held = [h if h == p else None for h, p in zip(self.held, now)]  # the documented mixed case
        if plan is not None:
            self.synced = state

    def update_lights(self, state, indices):
        """The bookkeeping after mt_raytree_update_lights over `indices` returned MT_OK."""
        assert not self.stale(state)
        now = positions(state)
        for i in indices:
            self.held[i] = now[i]
        fresh = truth_tree(self.synced, self.spec, [h if h is not None else p for h, p in zip(self.held, now)], self.rays)
        for lay, f in zip(self.tree["layers"], fresh["layers"]):
            for i in indices:
                lay["power"][i] = f["power"][i]
                lay["in_shadow"][i] = f["in_shadow"][i]


def list_rays(state):
    """The 64 x 1 ray list of a session: the first 64 rays of layer 1 of the frame's tree under `state`."""
    lay = truth_tree(state, None, positions(state))["layers"][1]
    assert len(lay["ray"]) >= LIST_W
    return lay["ray"][:LIST_W].copy(), lay["in_object"][:LIST_W].copy(), lay["coef"][:LIST_W].copy()


def make_trees(state, names):
    return {n: Tree(n, state, list_rays(state) if tree_def(n)[0] == "list" else None) for n in names}


# ---- the scripted sessions.  A step: dict(ops = the edits, in order; calls = {tree: [calls, in order]}; claim = what
# tests/test_edit_sessions_cpu.py holds the step's ops to; check = False where checkpoint A waits for a later step)

def step(ops, calls, claim=None, check=True):
    return dict(ops=list(ops), calls=calls, claim=claim, check=check)


def mat(i, **fields):
    return ("mat", i, fields)


def back_to(state, target):
    """The mat / tex_move ops that bring `state`'s materials to `target`'s."""
    ops = []
    for i, (a, b) in enumerate(zip(state["mats"], target["mats"])):
        fields = {k: (b[at:at + n].tolist() if n > 1 else float(b[at])) for k, (at, n) in me.FIELDS.items()
                  if a[at:at + n].tobytes() != b[at:at + n].tobytes()}
        if fields:
            ops.append(("mat", i, fields))
        if state["tex_of"][i] != target["tex_of"][i]:
            ops.append(("tex_move", i, target["tex_of"][i]))
    return ops


def after(state, steps):
    for st in steps:
        for op in st["ops"]:
            state = apply(state, op)
    return state


# session 1, "shape walk": rays per layer, kept, traced, dropped of the frame's tree, as literal numbers
SHAPE_WALK = [
    # (name, op, n_rays, kept, traced, dropped, pattern)
    ("matte Refl 0.5", mat(MATTE, Refl=0.5), [1536, 1100, 668, 248, 33, 5], [1536, 715, 170, 0, 0, 0], [0, 385, 498, 248, 33, 5], None, "grow"),
    ("mirror Refl 0", mat(MIRROR, Refl=0.0), [1536, 918, 362, 66], None, None, [0, 182, 306, 182, 33, 5], "drop"),
    ("pane Tr 0", mat(PANE, Tr=0.0), [1536, 792, 248, 34], None, None, None, "drop"),
    ("floor Refl 0", mat(FLOOR, Refl=0.0), [1536, 385], None, None, None, "drop"),
    ("wall Refl 0.6, Tr 0.3, Tf", mat(WALL, Refl=0.6, Tr=0.3, Tf=(0.5, 0.6, 0.7)), [1536, 1103], None, [0, 718], None, "grow"),
    ("mirror Refl 0.9", mat(MIRROR, Refl=0.9), [1536, 1285, 537, 219], None, None, None, "grow"),
    ("back to A", None, [1536, 715, 170], [1536, 182, 0], [0, 533, 170], [0, 1103, 537, 219], "both"),
]
SHAPE_WALK_A = [1536, 715, 170]
WALK_TREES = ("full", "chunk", "list")


def session_shape_walk():
    steps, state = [], start_state()
    for name, op, _, _, _, _, pattern in SHAPE_WALK:
        ops = [op] if op is not None else back_to(state, start_state())
        steps.append(step(ops, {t: ["regrow"] for t in WALK_TREES}, claim=("regrow", pattern)))
        state = after(state, steps[-1:])
    return steps


# session 2, "pending edits"
PILE = [
    (mat(WALL, Kd=(0.2, 0.3, 0.9)), "shade-only"),
    (("tex", 0, "2x2"), "planes"),
    (mat(MATTE, Refl=0.5), "planes"),
    (("tex", 0, "3x5_f64"), "planes"),          # the same texture set twice
    (mat(FLOOR, Ka=(0.9, 0.5, 0.25)), "planes"),  # the ambient of the textured floor
    (("tex_move", WALL, -1), "planes"),
]


def session_pile():
    """2a: the pile, then one regrow."""
    return [step([op for op, _ in PILE], {t: ["regrow"] for t in WALK_TREES}, claim=("regrow", "grow"))]


def session_refused_then_reverted():
    """2b: the pile, update_materials refused for the shape; the matte edit alone reverted; update_materials ok with a
    retexture and no shadow ray."""
    return [step([op for op, _ in PILE], {t: ["update_materials"] for t in ("full", "chunk")}, claim=("refused", "unsupported_shape")),
            step([mat(MATTE, Refl=0.0)], {t: ["update_materials"] for t in ("full", "chunk")}, claim=("retexture", None))]


def session_net_zero():
    """2c: edits that are all undone before the sync, except one set of the spare texture, which no material uses."""
    ops = [mat(MATTE, Refl=0.5), mat(FLOOR, Ka=(0.9, 0.5, 0.25)), ("tex_move", WALL, -1), ("tex", 2, "1x1"),
           mat(MATTE, Refl=0.0), mat(FLOOR, Ka=te.TINY_MATERIALS[FLOOR][1]), ("tex_move", WALL, 1)]
    return [step(ops, {t: ["update_materials"] if t != "chunk" else ["regrow"] for t in ("full", "chunk", "list", "plain")},
                 claim=("nothing", None))]


def session_three_rhythms():
    """2d: the frame's tree syncs after every op, the chunk's only once at the end, the tree without uvw is asked at
    every op: ok while only untextured materials changed, refused from the first textured change on -- and still refused
    after the original texels are back, because the generation moved."""
    ops = [mat(MIRROR, Ka=(0.3, 0.2, 0.1)),            # untextured: the plain tree takes it
           mat(MATTE, Refl=0.5),                       # and this, regrown
           mat(FLOOR, Ka=(0.9, 0.5, 0.25)),            # rule (a): a textured material's ambient
           mat(FLOOR, Ka=te.TINY_MATERIALS[FLOOR][1]),  # ... undone: the plain tree is in step again
           ("tex", 0, "2x2"),                          # rule (b)
           ("tex", 0, "original"),                     # the original texels: the generation moved, still refused
           mat(PANE, Tr=0.0),
           ("tex_move", MATTE, 1)]
    steps = []
    for i, op in enumerate(ops):
        calls = {"full": ["regrow"], "plain": ["regrow" if i % 2 else "update_materials"]}
        if i + 1 == len(ops):
            calls["chunk"] = ["regrow"]
        steps.append(step([op], calls))
    return steps


# session 3, "lights interleaved": the moves, with the rays of layers 0, 1, 2 whose in_shadow changes
LIGHT_MOVES = [(1, (8.0, 3.0, 4.0), [85, 14, 2]), (0, (5.0, 2.0, 7.0), [92, 23, 2]), (1, (9.5, 7.0, 9.0), [53, 11, 2])]
LIGHT_TREES = ("full", "chunk", "list")


def session_lights():
    (i1, p1, _), (i2, p2, _), (i3, p3, _) = LIGHT_MOVES
    every = lambda calls: {t: list(calls) for t in LIGHT_TREES}  # noqa: E731
    return [
        step([("move_light", i1, p1)], every([("update_lights", [i1])]), claim=("light", i1)),
        # shadow-relevant, with a moved light pending: ALL lights are traced again at the scene's positions ...
        step([mat(PANE, Tf=(0.5, 0.25, 1.0)), ("move_light", i2, p2)], every(["update_materials"]), claim=("all lights", i2)),
        # ... so the update of the moved light changes no bit
        step([], every([("update_lights", [i2])]), claim=("no bit", i2)),
        # not shadow-relevant: the tree keeps the old position's planes of light 1
        step([("move_light", i3, p3), ("colour_light", 0, (0.2, 0.1, 0.1, 0.7, 0.8, 0.9, 0.4, 0.5, 0.6)), mat(MIRROR, Ka=(0.3, 0.2, 0.1))],
             every(["update_materials"]), claim=("old position", i3)),
        step([], every([("update_lights", [i3])]), claim=("new position", i3)),
        # the documented mixed case, once: a move, a regrow with traced rays, update_lights, and only then the checkpoint
        step([("move_light", i1, p1), mat(MATTE, Refl=0.5)], every(["regrow"]), claim=("mixed", i1), check=False),
        step([], every([("update_lights", [i1])]), claim=("new position", i1)),
    ]


# session 4, "deferred planes": session 1's states plus two texture steps, for the stored G-buffer and light buffer
def session_deferred():
    walk = session_shape_walk()
    extra = [step([("tex", 0, "3x5_f64"), ("tex_move", MATTE, 1)], {}), step([("move_light", 1, LIGHT_MOVES[0][1])], {}),
             step([("tex", 1, "2x2"), mat(FLOOR, Ka=(0.9, 0.5, 0.25))], {})]
    return walk[:3] + extra[:2] + walk[3:] + extra[2:]


SCRIPTED = {
    "shape walk": (session_shape_walk, WALK_TREES),
    "pile": (session_pile, WALK_TREES),
    "refused then reverted": (session_refused_then_reverted, ("full", "chunk")),
    "net zero": (session_net_zero, ("full", "chunk", "list", "plain")),
    "three rhythms": (session_three_rhythms, ("full", "chunk", "plain")),
    "lights": (session_lights, LIGHT_TREES),
}


# ---- the seeded generator

SEEDS = (0x5e5506, 0x5e5509, 0x5e550a)  # chosen so that tests/test_edit_sessions_cpu.py's generator conditions hold
N_OPS = 24
ALL_TREES = ("full", "chunk", "list", "plain")
LIGHT_SPOTS = [p for _, p, _ in LIGHT_MOVES] + [tuple(l[:3]) for l in te.TINY_LIGHTS] + [(2.0, 7.0, 1.0), (7.0, 4.0, 6.0)]


def generate(seed, n_ops=N_OPS):
    """A session of n_ops steps of one op each on all four trees, a sync call per tree after every op (and
    update_lights over a moved light first), drawn from texture_edit_ref.splitmix(seed).  The generator runs the model
    as it goes, for two rules: a light moves only while every tree is fresh or beyond every update (no regrow then
    traces rays with a moved light pending: the mixed case stays with the scripted session), and an op that would leave
    the state as it is is drawn again a few times."""
    r = te.splitmix(seed)
    pick = lambda seq: seq[int(r() * len(seq))]  # noqa: E731
    short = lambda: round(0.05 + 0.9 * r(), 2)  # noqa: E731  (short decimals)
    state = start_state()
    trees = make_trees(state, ALL_TREES)
    steps = []

    def draw(state):
        u = r()
        if u < 0.58:   # a material flipped between reflective and transparent: subtrees die and others grow at once
            i = pick((FLOOR, WALL, MIRROR, PANE, MATTE))
            v = state["mats"][i]
            if v[10] > 0.0 or (v[11] == 0.0 and r() < 0.5):
                return mat(i, Refl=0.0, Tr=pick((0.3, 0.5, 0.6)), Tf=(short(), short(), short()))
            return mat(i, Refl=pick((0.25, 0.5, 0.75)), Tr=0.0)
        if u < 0.64:
            return mat(pick((MIRROR, PANE, MATTE, FLOOR, WALL)), **{pick(("Kd", "Ks")): (short(), short(), short()), "Ns": pick((2.0, 8.0, 20.0))})
        if u < 0.71:
            return mat(pick((FLOOR, WALL, MIRROR, PANE, MATTE)), Ka=(short(), short(), short()))
        if u < 0.81:
            return ("tex", pick((0, 0, 1, 1, 2)), pick(("1x1", "2x2", "3x5_f64", "original")))
        if u < 0.89:
            return ("tex_move", pick((FLOOR, WALL, MATTE, MIRROR)), pick((-1, 0, 1, 2)))
        if u < 0.95:
            return ("move_light", pick((0, 1)), pick(LIGHT_SPOTS))
        return ("colour_light", pick((0, 1)), tuple(short() for _ in range(9)))

    for _ in range(n_ops):
        for attempt in range(8):
            op = draw(state)
            if op[0] == "move_light" and not all(not t.stale(state) or t.doomed(state) for t in trees.values()):
                continue
            if not net_noop(state, apply(state, op)) or attempt == 7:
                break
        state = apply(state, op)
        calls = {}
        for name, t in trees.items():
            mine = []
            if op[0] == "move_light":
                mine.append(("update_lights", [op[1]]))
            mine.append("update_materials" if r() < 0.2 else "regrow")
            calls[name] = mine
        steps.append(step([op], calls))
        run_step(trees, state, steps[-1])
    return steps


def run_step(trees, state, st, log=None):
    """The model's side of a step's calls; `state` already holds the step's ops.  log: a list that receives
    (tree, call, prediction)."""
    for name, calls in st["calls"].items():
        t = trees[name]
        for call in calls:
            p = t.predict(state, call)
            if log is not None:
                log.append((name, call, p))
            if call in ("update_materials", "regrow"):
                if p["outcome"] in ("ok", "ok_nothing_to_do"):
                    t.commit(state, p)
            elif call != "shade" and p["outcome"] == "ok":
                t.update_lights(state, call[1])


# ---- the newer edit kinds: the menus (AddPrimitive numbering: floor 0 1, wall 2 3, mirror 4 5, matte 6 7, pane 8 9,
# the NaN-uvw triangle 10, the zero-area one 11)

ORIGINAL = start_state()
ASSIGNS = {
    "matte->mirror": {6: MIRROR, 7: MIRROR},   # the tree grows
    "mirror->wall": {4: WALL, 5: WALL},        # the tree shrinks (the wall is textured)
    "pane->wall": {8: WALL, 9: WALL},          # shadow-visible by assign_ref.shadow_visible, as is ...
    "wall->pane": {2: PANE, 3: PANE},
    "matte->floor": {6: FLOOR, 7: FLOOR},      # the target is TEXTURED
    "matte#1->mirror": {6: MIRROR},            # one triangle of a quad only
    "matte#2->floor": {7: FLOOR},
    "floor->none": {0: -1, 1: -1},
}


def _tilt(tris, by):
    out = {}
    for i in tris:
        n = ORIGINAL["normals"][i] + np.asarray(by, dtype=np.float64)
        out[i] = n / np.sqrt((n * n).sum(axis=1))[:, None]
    return out


def _minus_zero(i, component):
    n = ORIGINAL["normals"][i].copy()
    assert (n[:, component] == 0.0).all() and not np.signbit(n[:, component]).any()
    n[:, component] = -0.0
    return {i: n}


NORMALS = {
    "matte tilt": _tilt((6, 7), (0.0, 0.05, 0.0)),    # no reflected child: an update takes it
    "mirror tilt": _tilt((4, 5), (0.05, 0.0, 0.0)),   # reflected children: the update refuses, the regrow respawns
    "floor tilt": _tilt((0, 1), (0.03, 0.0, 0.0)),
    "floor#2 zero": {1: np.zeros((3, 3))},
    "matte#1 -0.0": _minus_zero(6, 1),                # bit-different and value-equal
}
UVWS = {name: make() for name, make in va.UVW_EDITS.items()}
MENUS = {"assign": ASSIGNS, "normals": NORMALS, "uvws": UVWS}
STATE_KEY = {"assign": "tri_mtl", "normals": "normals", "uvws": "uvws"}


def edit(kind, name):
    return (kind, MENUS[kind][name])


def original(kind, tris):
    """The inverse: the triangles `tris` back to the original."""
    src = ORIGINAL[STATE_KEY[kind]]
    return (kind, {int(i): (src[i] if kind == "assign" else src[i].copy()) for i in tris})


def holds(state, op):
    """The state already holds what the op sets."""
    return same_look(state, apply(state, op))


# ---- the scripted sessions of the newer kinds

def _calls(with_tri, without_tri, names=tuple(NEW_TREES)):
    return {n: list(with_tri if NEW_TREES[n][2] else without_tri) for n in names}


# session a, "stamp walk": per step what the frame's tree with tri and uvw ("full_tu") must report, as literal numbers:
# (the refused update's blocked count and first (layer, ray) or None, regrown, kept, traced, renormaled, reuvwed,
# respawned) -- found once with the oracle, held by tests/test_edit_sessions_cpu.py
STAMP_WALK = [
    (None, 0, [1536, 715, 170], [0, 0, 0], 531, 0, 0),
    (None, 0, [1536, 715, 170], [0, 0, 0], 0, 441, 0),
    ((232, (0, 79)), 1, [1536, 533, 114], [0, 182, 56], 383, 0, 232),   # 383: mirror rays alone, not the matte's 531
    (None, 0, [0, 0, 0], [0, 0, 0], 0, 0, 0),                           # equal generations: nothing to do
    ((232, (0, 79)), 1, [1536, 533, 114], [0, 182, 56], 383, 0, 232),
]


def session_stamp_walk():
    return [
        step([edit("normals", "matte tilt")], _calls(["update_materials"], ["update_materials"]), claim=("attr", "renormaled")),
        step([edit("uvws", "floor x2")], _calls(["update_materials"], ["regrow"]), claim=("attr", "reuvwed")),
        # refused (reflected children), untouched and still stale; the regrow respawns, and renormals ONLY mirror rays
        step([edit("normals", "mirror tilt")], _calls(["update_materials", "regrow"], ["regrow"]), claim=("respawn", None)),
        step([edit("normals", "mirror tilt")], _calls(["update_materials"], ["update_materials"]), claim=("nothing", None)),
        # A -> B -> A is dirty: refused again, and the regrow gives the planes of step 1 back
        step([original("normals", (4, 5))], _calls(["update_materials", "regrow"], ["regrow"]), claim=("respawn", None)),
    ]


# session b, "assignment walk": (regrown, rays per layer, kept, traced, dropped, rays_shadow) of "full_tu" per step, and
# what the tree with tri but without uvw ("full_t") answers: the wall and the floor are both TEXTURED, so it refuses
# from step 1 on, naming (triangle, material), and its snapshot stays step 0's
ASSIGN_WALK = [
    (1, [1536, 1100, 668, 248, 33, 5], [1536, 715, 170, 0, 0, 0], [0, 385, 498, 248, 33, 5], [0, 0, 0], 1882),
    (1, [1536, 974, 554, 185, 5, 3], [1536, 974, 554, 185, 5, 3], [0, 0, 0, 0, 0, 0], [0, 126, 114, 63, 28, 2], 5436),
    (0, [1536, 974, 554, 185, 5, 3], [1536, 974, 554, 185, 5, 3], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], 0),
    (1, [1536, 715, 170], [1536, 589, 89], [0, 126, 81], [0, 385, 465, 185, 5, 3], 4970),
]
ASSIGN_WALK_TRI_ONLY = ["ok", (8, WALL), (6, FLOOR), "ok"]


def session_assignment_walk():
    every = lambda calls: {n: list(calls) for n in NEW_TREES}  # noqa: E731
    return [
        step([edit("assign", "matte->mirror")], every(["regrow"]), claim=("regrow", "grow")),
        # shadow-visible (rays_shadow > 0 though no ray is traced), subtrees drop
        step([edit("assign", "pane->wall")], every(["regrow"]), claim=("regrow", "drop")),
        # the mirror-painted box given the floor's material: a TEXTURED target; the children stay (Refl 0.75 -> 0.25)
        step([edit("assign", "matte->floor")], every(["regrow"]), claim=("retexture", None)),
        # everything back: CHANGED against the LAST SUCCESSFUL sync decides -- empty for the trees without tri (nothing
        # to do), the matte box alone for full_t, whose snapshot is step 0's
        step([original("assign", (6, 7, 8, 9))], every(["regrow"]), claim=("regrow", "both")),
    ]


# session c, "the pile": six edits, one sync
NEW_PILE = [mat(FLOOR, Refl=0.0), edit("assign", "matte#1->mirror"), edit("normals", "matte tilt"), edit("uvws", "floor x2"),
            ("tex", 0, "2x2"), edit("assign", "matte#2->floor")]
PILE_TREES = ("full_tu", "chunk_tu", "list_tu")
# "full_tu": the refused update's (count, first), then the regrow's rays, kept, traced, dropped, renormaled, reuvwed
NEW_PILE_FULL = ((640, (0, 78)), [1536, 427, 90, 27], [1536, 308, 0, 0], [0, 119, 90, 27], [0, 407, 170], 427, 423)


def session_new_pile(reverse=False):
    """The update is refused for the shape, one regrow takes all six; reverse: the same pile in the other order."""
    ops = NEW_PILE[::-1] if reverse else NEW_PILE
    return [step(ops, {n: ["update_materials", "regrow"] if n == "full_tu" else ["regrow"] for n in PILE_TREES},
                 claim=("regrow", "both"))]


# session d, "rhythms": the full tree syncs after every op, the chunk after every third, the list once at the end; the
# trees without tri are asked at every op
RHYTHM_OPS = [
    mat(MIRROR, Ka=(0.3, 0.2, 0.1)),
    edit("normals", "matte tilt"),
    edit("assign", "pane->wall"),
    edit("uvws", "floor x2"),
    ("tex", 0, "2x2"),
    edit("normals", "mirror tilt"),        # other triangles than the first set's
    original("assign", (8, 9)),
    original("normals", (4, 5, 6, 7)),     # the original arrays: the stamps are newer, the trees without tri stay refused
    original("uvws", (0, 1)),
]
RHYTHM_TREES = ("full_tu", "chunk_tu", "list_tu", "full_u", "full_0")
# "full_tu" per op: (regrown, rays per layer, kept, traced, dropped, rays_shadow, (renormaled, reuvwed, respawned)) -- op 7
# renormals the rays of all four triangles (856) though only the mirror's have reflected children (232 respawned)
_A, _B = [1536, 715, 170], [1536, 589, 89]
RHYTHMS_FULL = [
    (0, _A, _A, [0, 0, 0], [0, 0, 0], 0, (0, 0, 0)),
    (0, _A, _A, [0, 0, 0], [0, 0, 0], 0, (531, 0, 0)),
    (1, _B, _B, [0, 0, 0], [0, 126, 81], 3906, (0, 0, 0)),
    (0, _B, _B, [0, 0, 0], [0, 0, 0], 0, (0, 403, 0)),
    (0, _B, _B, [0, 0, 0], [0, 0, 0], 0, (0, 0, 0)),
    (1, _B, [1536, 407, 33], [0, 182, 56], [0, 182, 56], 248, (232, 0, 232)),
    (1, _A, _B, [0, 126, 81], [0, 0, 0], 4950, (0, 0, 0)),
    (1, _A, [1536, 533, 114], [0, 182, 56], [0, 182, 56], 274, (856, 0, 232)),
    (0, _A, _A, [0, 0, 0], [0, 0, 0], 0, (0, 441, 0)),
]


def session_new_rhythms():
    steps = []
    for i, op in enumerate(RHYTHM_OPS):
        calls = {"full_tu": ["regrow"], "full_u": ["regrow" if i % 2 else "update_materials"],
                 "full_0": ["update_materials" if i % 2 else "regrow"]}
        if i % 3 == 2:
            calls["chunk_tu"] = ["regrow"]
        if i + 1 == len(RHYTHM_OPS):
            calls["list_tu"] = ["regrow"]
        steps.append(step([op], calls))
    return steps


# session e, "lights interleaved"
NEW_LIGHT_TREES = ("full_tu", "chunk_tu", "list_tu")


def _lights_after_the_moves():
    (i1, p1, _), (i2, p2, _), _ = LIGHT_MOVES
    return apply(apply(start_state(), ("move_light", i1, p1)), ("move_light", i2, p2))["lights"]


TWO_LIGHTS = _lights_after_the_moves()
ONE_LIGHT = TWO_LIGHTS[:1]
# "full_tu" per step, in RHYTHMS_FULL's form: None where the step syncs no tree (update_lights) or the sync is refused
NEW_LIGHTS_FULL = [
    (1, _B, _B, [0, 0, 0], [0, 126, 81], 3906, (0, 0, 0)),
    None,
    (0, _B, _B, [0, 0, 0], [0, 0, 0], 0, (0, 403, 0)),
    None,
    None,   # (the light count refusal: 1 light in the scene, 2 in the tree)
    (1, _B, [1536, 407, 33], [0, 182, 56], [0, 182, 56], 248, (232, 0, 232)),
]


def session_new_lights():
    (i1, p1, _), (i2, p2, _), _ = LIGHT_MOVES
    every = lambda calls: {t: list(calls) for t in NEW_LIGHT_TREES}  # noqa: E731
    return [
        # a moved light pending across a shadow-visible reassignment: ALL lights are traced again at the current positions
        step([("move_light", i1, p1), edit("assign", "pane->wall")], every(["regrow"]), claim=("all lights", i1)),
        step([], every([("update_lights", [i1])]), claim=("no bit", i1)),
        # across a uvw-only edit: the old planes are kept, then update_lights catches up
        step([("move_light", i2, p2), edit("uvws", "floor x2")], every(["update_materials"]), claim=("old position", i2)),
        step([], every([("update_lights", [i2])]), claim=("new position", i2)),
        # a normal edit's regrow under another light COUNT: check (4) refuses with MT_ERR_ARG, the tree untouched and
        # still stale; taken once the count is restored
        step([("set_lights", ONE_LIGHT), edit("normals", "mirror tilt")], {"full_tu": ["regrow"], "chunk_tu": ["regrow"]},
             claim=("light count", None)),
        step([("set_lights", TWO_LIGHTS)], {"full_tu": ["regrow"], "chunk_tu": ["regrow"]}, claim=("respawn", None)),
    ]


# session f, "frames between edits": eight ops of the newer kinds, a frame after each; the G-buffer, light buffer,
# supersampled and adaptive frames after the ops FRAME_EXTRAS
FRAME_OPS = [edit("assign", "matte->mirror"), edit("normals", "matte tilt"), edit("uvws", "floor x2"),
             edit("assign", "pane->wall"), edit("normals", "floor tilt"), edit("uvws", "nan swap"),
             edit("assign", "floor->none"), original("normals", (0, 1, 6, 7))]
FRAME_EXTRAS = (1, 4, 7)


CLAIM_TREES = ("full_tu", "chunk_tu")  # (the 64 rays of the list hit the matte box or nothing)


def hold_claim(claim, mine, before, tree, state):
    """Holds a step's claim on one tree that keeps tri and uvw: mine = [(call, prediction)] of the step's calls on it, in
    order; before = a copy_tree of the model's tree before the step; tree = the Tree after it; state = the scene's.
    Where the step asks update_materials before the regrow, the update is refused for what the claim names.  Returns
    the claim's kind."""
    kind, arg = claim
    what = (claim, [(c, p["outcome"]) for c, p in mine])
    for call, q in mine[:-1]:
        assert call == "update_materials" and q["outcome"] == dict(respawn="unsupported_normals", regrow="unsupported_shape")[kind], what
        assert q["count"] > 0
    call, p = mine[-1]
    moved = {name for _, name in differing_planes(before, tree.tree, True, True)} if before["n_rays"] == tree.tree["n_rays"] else None
    if kind == "light count":   # the regrow's check (4): refused, the tree untouched and still stale
        assert p["outcome"] == "light_count" and (p["scene"], p["tree"]) == (len(state["lights"]), len(tree.held)), what
        assert p["scene"] != p["tree"] and moved == set() and tree.stale(state), what
        return kind
    assert p["outcome"] == ("ok_nothing_to_do" if kind == "nothing" else "ok"), what
    assert not tree.stale(state), what
    if kind == "regrow":
        t, d = sum(p["traced"]), sum(p["dropped"])
        assert p["regrown"] == 1 and (t > 0, d > 0) == dict(grow=(True, False), drop=(False, True), both=(True, True))[arg], (what, t, d)
    elif kind == "retexture":
        assert p["regrown"] == 0 and p["rays_shadow"] == 0 and "albedo" in moved and not moved & {"power", "in_shadow"}, (what, moved)
    elif kind == "nothing":
        assert moved == set() and all(p[k] == 0 for k in ATTR_COUNTS), what
    elif kind == "attr":      # a same-shape update that rewrites the edited triangles' rays, and nothing else
        assert p["regrown"] == 0 and p[arg] > 0 and all(p[k] == 0 for k in ATTR_COUNTS if k != arg), what
        assert p["rays_shadow"] == 0 and dict(renormaled="normal", reuvwed="uvw")[arg] in moved, (what, moved)
        assert moved <= dict(renormaled={"normal"}, reuvwed={"uvw", "albedo"})[arg], (what, moved)
    elif kind == "respawn":   # reflected children of edited triangles start again from the new normal
        assert p["regrown"] == 1 and p["respawned"] > 0 and p["renormaled"] >= p["respawned"] and sum(p["traced"]) > 0, what
    elif kind == "all lights":  # shadow-visible with a moved light pending: every light again, at the scene's positions
        assert p["rays_shadow"] > 0 and tree.settled(state), what
        a, b = before["layers"][0], tree.tree["layers"][0]
        assert p["kept"][0] == len(a["ray"]) == len(b["ray"]) and (a["in_shadow"][arg] != b["in_shadow"][arg]).any(), what
    elif kind == "old position":  # not shadow-visible: the moved light's planes stay at the old position
        assert p["rays_shadow"] == 0 and tree.pending_lights(state) == [arg], what
        assert moved is not None and not moved & {"power", "in_shadow"}, (what, moved)
    elif kind == "no bit":
        assert tree.settled(state) and moved == set(), (what, moved)
    elif kind == "new position":
        assert tree.settled(state) and moved and moved <= {"power", "in_shadow"}, (what, moved)
    else:
        raise ValueError(claim)
    return kind


NEW_SCRIPTED = {
    "stamp walk": (session_stamp_walk, tuple(NEW_TREES)),
    "assignment walk": (session_assignment_walk, tuple(NEW_TREES)),
    "new pile": (session_new_pile, PILE_TREES),
    "new rhythms": (session_new_rhythms, RHYTHM_TREES),
    "new lights": (session_new_lights, NEW_LIGHT_TREES),
}


# ---- the seeded generator of the newer kinds: its own draw path, so that SEEDS' streams do not move

NEW_SEEDS = (0xa5e5e2, 0xa5e60f, 0xa5e645)  # chosen so that tests/test_edit_sessions_cpu.py's FLOORS hold for each, with the model alone
NEW_N_OPS = 24


def generate_new(seed, n_ops=NEW_N_OPS):
    """A session of n_ops steps of one op each on all six NEW_TREES, a sync call per tree after every op (and
    update_lights over a moved light first).  About half of the draws are ops of the newer kinds or their inverses (an
    edit the state already holds is drawn as "back to the original"); the others are `generate`'s.  The same two rules:
    a light moves only while every tree is fresh or beyond every update, and an op that would leave the state as it is
    is drawn again a few times."""
    r = te.splitmix(seed)
    pick = lambda seq: seq[int(r() * len(seq))]  # noqa: E731
    short = lambda: round(0.05 + 0.9 * r(), 2)  # noqa: E731
    state = start_state()
    trees = make_trees(state, tuple(NEW_TREES))
    steps = []

    def draw_new(state):
        if steps and steps[-1]["ops"][0][0] in MENUS and r() < 0.4:  # the last edit reverted at once: A -> B -> A
            last = steps[-1]["ops"][0]
            return original(last[0], sorted(last[1]))
        kind = pick(("assign", "normals", "uvws"))
        name = pick(sorted(MENUS[kind]))
        op = edit(kind, name)
        return original(kind, sorted(op[1])) if holds(state, op) else op

    def draw_old(state):
        u = r()
        if u < 0.40:
            i = pick((FLOOR, WALL, MIRROR, PANE, MATTE))
            v = state["mats"][i]
            if v[10] > 0.0 or (v[11] == 0.0 and r() < 0.5):
                return mat(i, Refl=0.0, Tr=pick((0.3, 0.5, 0.6)), Tf=(short(), short(), short()))
            return mat(i, Refl=pick((0.25, 0.5, 0.75)), Tr=0.0)
        if u < 0.52:
            return mat(pick((FLOOR, WALL, MIRROR, PANE, MATTE)), Ka=(short(), short(), short()))
        if u < 0.76:
            return ("tex", pick((0, 0, 1, 1, 2)), pick(("1x1", "2x2", "3x5_f64", "original")))
        if u < 0.86:
            return ("tex_move", pick((FLOOR, WALL, MATTE, MIRROR)), pick((-1, 0, 1, 2)))
        if u < 0.95:
            return ("move_light", pick((0, 1)), pick(LIGHT_SPOTS))
        return ("colour_light", pick((0, 1)), tuple(short() for _ in range(9)))

    for _ in range(n_ops):
        for attempt in range(8):
            op = draw_new(state) if r() < 0.55 else draw_old(state)
            if op[0] == "move_light" and not all(not t.stale(state) or t.doomed(state) for t in trees.values()):
                continue
            if not net_noop(state, apply(state, op)) or attempt == 7:
                break
        if op[0] == "move_light" and not all(not t.stale(state) or t.doomed(state) for t in trees.values()):
            op = ("colour_light", op[1], tuple(short() for _ in range(9)))  # (eight refused draws: no light moves)
        state = apply(state, op)
        calls = {}
        for name, t in trees.items():
            mine = []
            if op[0] == "move_light":
                mine.append(("update_lights", [op[1]]))
            mine.append("update_materials" if r() < 0.5 else "regrow")
            calls[name] = mine
        steps.append(step([op], calls))
        run_step(trees, state, steps[-1])
    return steps
