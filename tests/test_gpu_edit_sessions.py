"""Edit SESSIONS on a real MI355X (-m gpu): one uploaded scene and its stored ray trees, G-buffer and light buffer kept
alive through chains of mt_scene_set_materials, mt_scene_set_texture, mt_scene_set_lights, mt_raytree_update_materials,
mt_raytree_regrow_materials, mt_raytree_update_lights, mt_retexture_gbuffer and mt_update_lightbuffer
(include/mythtracer_hip.h).  The one-hop tests of these calls start from a new scene and tree every time; what decides a
session is the state a call leaves behind for the next one -- the tree's snapshot and generations, the patched layer
table and byte count, the scratch that only grows, the replaced texture entry.

The live scene of a session is NEVER recreated.  The model of tests/edit_session_ref.py (pinned with the oracle alone by
tests/test_edit_sessions_cpu.py) says after every call what it must have returned and what the tree must hold; the truth
for a state is always a scene newly CREATED from the state's description and the oracle built from it.  The bar is
identity -- doubles as uint64 views with NaN = NaN, bytes and indices equal -- except the oracle's frame, held under
the POW-group rule of tests/test_gpu_hostile.py (test_gpu_parity.assert_rgb_close: the tiny materials have Ns != 0).
Everything is the tiny scene at 48 x 32, depth 5: 1 536 primary rays, 12 triangles.  Every test prints its counts.

Sessions a to h take the three newer edits into the chain -- mt_scene_set_triangle_materials, _normals and _uvw -- on
trees with every combination of mt_scene_set_raytree_tri / _uvw (es.NEW_TREES): what they leave behind for the next call
is the assignment snapshot, the two attribute generations and the per-triangle stamps.  After EVERY call: the return
code and the numbers of the message, regrown / kept / traced / dropped, mt_raytree_attr_info_last, kernel_ms == 0 where
promised, every plane (tri included) against a tree newly created on a scene newly created from the state -- or, after
a refusal, against the tree's own previous read-back --, the getters, and the bytes rule (4 per ray for tri, 24 for uvw).
"""
import ctypes
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import assign_ref as ar  # noqa: E402
import edit_session_ref as es  # noqa: E402
import raytree_ref as rr  # noqa: E402
import raytree_update_ref as ru  # noqa: E402
import regrow_ref as rg  # noqa: E402
import texture_edit_ref as te  # noqa: E402
import vertex_attr_ref as va  # noqa: E402
from gbuffer_ref import same_bits  # noqa: E402
from test_gpu_parity import assert_rgb_close  # noqa: E402

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding  # noqa: E402

MT_OK, MT_ERR_ARG, MT_ERR_UNSUPPORTED = 0, -1, -3
STALE = "materials were edited after the ray tree was made"
W, H, DEPTH, CAM = es.W, es.H, es.DEPTH, es.CAM
INFO_KEYS = ("n_layers", "n_rays", "bytes")
COUNTS = ("rays_primary", "rays_secondary", "shaded_hits", "rays_shadow")


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"


@pytest.fixture(scope="module")
def flat0():
    """The tiny scene's flat description; `described` puts a state's tables into it."""
    flat = te.build_tiny(M.MythTracer()).flatten()
    assert [m["tex"] for m in flat["materials"]] == [0, 1, -1, -1, -1]
    for m, want in zip(flat["materials"], dense_materials(es.start_state())):
        assert np.array_equal(m["values"], want["values"]) and m["tex"] == want["tex"]  # (the numbering is es.DENSE)
    return flat


TO_DENSE = np.argsort(np.array(es.DENSE))  # the table's material index -> the description's


def dense_materials(state):
    """A state's materials in the description's numbering, as mt_scene_set_materials takes them."""
    table = es.flat_materials(state)
    return [table[m] for m in es.DENSE]


def dense_plane(material):
    """A restated material plane (the table's numbering) in the description's."""
    material = np.asarray(material)
    return np.where(material >= 0, TO_DENSE[np.maximum(material, 0)], material).astype(np.int32)


def stream_arrays(flat0, state):
    """(tri_material, tri_normal, tri_uvw) of a state in node-stream order and the description's material numbering, as
    the three set calls take them and a description holds them."""
    add = np.asarray(flat0["tri_id"], dtype=np.int64)
    assert sorted(add.tolist()) == list(range(es.N_TRIS)) and es.stream_of() == {int(a): k for k, a in enumerate(add)}
    return (dense_plane(np.array(state["tri_mtl"])[add]),
            np.ascontiguousarray(state["normals"][add]).reshape(np.shape(flat0["tri_normal"])),
            np.ascontiguousarray(state["uvws"][add]).reshape(np.shape(flat0["tri_uvw"])))


def described(flat0, state):
    """The flat description of a scene BUILT from the state: the tables, and tri_material, tri_normal and tri_uvw replaced
    (assign_ref.built, vertex_attr_ref.built)."""
    tri_material, tri_normal, tri_uvw = stream_arrays(flat0, state)
    flat = dict(flat0, materials=dense_materials(state), textures=[dict(texels=np.array(t, copy=True)) for t in state["texs"]])
    return va.built(ar.built(flat, tri_material), tri_normal, tri_uvw)


def sensor():
    return binding.sensor(CAM, W, H)


def differing(a, b, what):
    n = int((a != b).any(axis=-1).sum())
    if n:
        print("%s: %d of %d pixels differ" % (what, n, a.shape[0] * a.shape[1]))
    return n


def planes_differing(got, want, what):
    """Two read-backs (lists of plane dicts): the (layer, plane) pairs that differ in a bit."""
    assert len(got) == len(want), (what, len(got), len(want))
    bad = []
    for k, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w), (what, sorted(g), sorted(w))
        bad += [(k, name) for name in g if not ru.same_plane(g[name], w[name])]
    if bad:
        print("%s: planes differ: %s" % (what, bad))
    return bad


def assert_is_truth(got, truth, keep_uvw, what, keep_tri=False, tri_id=None):
    """A read-back against the restated tree: test_gpu_regrow.assert_restated's rules (the material plane in the
    description's numbering: dense_plane, which flat0 checks by value), plus uvw by bits."""
    assert [len(g["coef"]) for g in got] == truth["n_rays"], (what, [len(g["coef"]) for g in got], truth["n_rays"])
    for k, (g, lay) in enumerate(zip(got, truth["layers"])):
        for name in rr.F64_PLANES + (("uvw",) if keep_uvw else ()):
            assert same_bits(g[name], lay[name], "%s layer %d %s" % (what, k, name)) == 0
        for name in ("in_object", "in_shadow", "child_refl", "child_refr"):
            assert np.array_equal(g[name], lay[name]), (what, k, name)
        assert np.array_equal(g["material"], dense_plane(lay["material"])), (what, k, "material")
        if k == 0:
            assert np.array_equal(g["pixel"], lay["pixel"]), what
        assert ("uvw" in g) == keep_uvw and ("tri" in g) == keep_tri
        if keep_tri:  # the tri plane speaks the node stream's numbering, the truth AddPrimitive's
            assert np.array_equal(np.where(g["tri"] >= 0, np.asarray(tri_id)[np.maximum(g["tri"], 0)], -1), lay["tri"]), (what, k, "tri")


class Live:
    """The live scene of a session, its trees and the model's bookkeeping of them."""

    def __init__(self, flat0, names=(), engine=None):
        self.abi = M.hip_abi()
        self.flat0 = flat0
        self.state = es.start_state()
        self.engine = engine
        self.h = self._scene(self.state, self.state["lights"])
        self.models = es.make_trees(self.state, names)
        self.trees = {}
        self.fresh = {}
        for name in names:
            self.trees[name] = self.make_tree(self.h, name)
        self.first = {name: self.planes(name) for name in names}
        for name in names:
            self.assert_truth(name, self.first[name], name + " at the start")
        for lst, full in (("list", "full"), ("list_tu", "full_tu")):
            if lst in names and full in names:  # the list is layer 1 of the frame's tree, as the GPU made it
                for got, want in zip((self.first[full][1][p][:es.LIST_W] for p in ("ray", "in_object", "coef")), self.models[lst].rays):
                    assert ru.same_plane(got, want)
        self.check_bytes("at the start")

    def assert_truth(self, name, got, what):
        model = self.models[name]
        assert_is_truth(got, model.truth(), model.keep_uvw, what, model.keep_tri, self.flat0["tri_id"])

    def check_bytes(self, what):
        """mt_raytree_info's bytes counts 4 bytes per ray for tri and 24 for uvw: over every pair of live trees of one
        definition that are synced to one state."""
        seen = 0
        for a, ma in self.models.items():
            for b, mb in self.models.items():
                if a < b and ma.spec == mb.spec and ma.synced is mb.synced and ma.held == mb.held:
                    ia, ib = self.abi.raytree_info(self.trees[a]), self.abi.raytree_info(self.trees[b])
                    rays = sum(ia["n_rays"][:ia["n_layers"]])
                    per = 4 * (int(ma.keep_tri) - int(mb.keep_tri)) + 24 * (int(ma.keep_uvw) - int(mb.keep_uvw))
                    assert ia["n_rays"] == ib["n_rays"] and ia["bytes"] - ib["bytes"] == per * rays, (what, a, b, ia["bytes"], ib["bytes"], per, rays)
                    seen += 1
        return seen

    def _scene(self, state, lights):
        h = self.abi.scene_create(described(self.flat0, state))
        if self.engine is not None:
            self.abi.set_engine(h, self.engine)
        self.abi.set_lights(h, lights)
        return h

    def make_tree(self, h, name):
        spec, keep, keep_tri = es.tree_def(name)
        self.abi.set_raytree_uvw(h, keep)
        self.abi.set_raytree_tri(h, keep_tri)
        if spec == "list":
            rays, in_object, coef = es.list_rays(es.start_state())
            t, _ = self.abi.raytree_create_rays(h, rays, in_object=in_object, coef=coef, max_depth=DEPTH)
        else:
            t, _ = self.abi.raytree_create(h, sensor(), W, H, chunk=spec, max_depth=DEPTH)
        assert self.abi.raytree_keeps_uvw(t) == keep and self.abi.raytree_keeps_tri(t) == keep_tri
        return t

    def close(self):
        self.end_step()
        for t in self.trees.values():
            self.abi.raytree_destroy(t)
        self.abi.scene_destroy(self.h)

    # ---- fresh scenes: newly created from a state's description, shared by the checkpoints of one step
    def fresh_scene(self, state, lights):
        key = (es.look_key(state), tuple(lights))
        if key not in self.fresh:
            self.fresh[key] = dict(h=self._scene(state, lights), trees={})
        return self.fresh[key]

    def fresh_tree(self, state, lights, name):
        f = self.fresh_scene(state, lights)
        if name not in f["trees"]:
            f["trees"][name] = self.make_tree(f["h"], name)
        return f["h"], f["trees"][name]

    def end_step(self):
        for f in self.fresh.values():
            for t in f["trees"].values():
                self.abi.raytree_destroy(t)
            self.abi.scene_destroy(f["h"])
        self.fresh = {}

    # ---- the scene's edits
    def apply(self, op):
        self.state = es.apply(self.state, op)
        if op[0] in ("mat", "tex_move"):
            self.abi.set_materials(self.h, dense_materials(self.state))
        elif op[0] == "tex":
            self.abi.set_texture(self.h, op[1], self.state["texs"][op[1]])
        elif op[0] in es.MENUS:
            tri_material, tri_normal, tri_uvw = stream_arrays(self.flat0, self.state)
            if op[0] == "assign":
                self.abi.set_triangle_materials(self.h, tri_material)
            elif op[0] == "normals":
                self.abi.set_triangle_normals(self.h, tri_normal)
            else:
                self.abi.set_triangle_uvw(self.h, tri_uvw)
            self.check_getters("after %s" % op[0])
        else:
            self.abi.set_lights(self.h, self.state["lights"])

    def check_getters(self, what):
        """mt_scene_get_triangle_* return the state's arrays."""
        tri_material, tri_normal, tri_uvw = stream_arrays(self.flat0, self.state)
        assert np.array_equal(self.abi.get_triangle_materials(self.h, es.N_TRIS), tri_material), what
        assert self.abi.get_triangle_normals(self.h, es.N_TRIS).tobytes() == tri_normal.tobytes(), what
        assert self.abi.get_triangle_uvw(self.h, es.N_TRIS).tobytes() == tri_uvw.tobytes(), what

    def frame(self, h, depth=DEPTH, chunk=None):
        return self.abi.render_chunk(h, sensor(), W, H, chunk=chunk, max_depth=depth)["rgb"]

    def checkpoint_b(self, what):
        """After a scene edit, without a tree: the frames at depths 0 and 5 are a fresh scene's and the oracle's, and the
        scene hands back the state's tables."""
        s = self.state
        f = self.fresh_scene(s, s["lights"])["h"]
        for depth in (0, DEPTH):
            got = self.frame(self.h, depth)
            assert differing(got, self.frame(f, depth), "%s: depth %d vs a fresh scene" % (what, depth)) == 0
            assert_rgb_close(got, es.oracle_frame(s, depth), "%s: depth %d vs the oracle" % (what, depth))
        for got, want in zip(self.abi.get_materials(self.h, len(s["mats"])), dense_materials(s)):
            assert got["tex"] == want["tex"] and got["values"].tobytes() == want["values"].tobytes(), what
        for i, t in enumerate(s["texs"]):
            want = dict(width=t.shape[1], height=t.shape[0], format=binding.MT_TEX_RGB8 if t.dtype == np.uint8 else binding.MT_TEX_F64)
            assert self.abi.get_texture_info(self.h, i) == want, (what, i)
        self.check_getters(what)

    # ---- the trees
    def planes(self, name):
        return self.planes_of(self.trees[name])

    def planes_of(self, t):
        out = []
        for k in range(self.abi.raytree_info(t)["n_layers"]):
            lay = self.abi.raytree_read_layer(t, k)
            if self.abi.raytree_keeps_uvw(t):
                lay["uvw"] = self.abi.raytree_read_uvw(t, k)
            if self.abi.raytree_keeps_tri(t):
                lay["tri"] = self.abi.raytree_read_tri(t, k)
            out.append(lay)
        return out

    def info(self, name):
        i = self.abi.raytree_info(self.trees[name])
        return {k: i[k] for k in INFO_KEYS}

    def raw_sync(self, name, call):
        """(rc, message, dict of info and stats) of mt_raytree_update_materials / mt_raytree_regrow_materials."""
        t = self.trees[name]
        st, info = binding.mt_stats(), binding.mt_raytree_regrow_info()
        if call == "regrow":
            rc = self.abi.lib.mt_raytree_regrow_materials(t, ctypes.addressof(info), ctypes.addressof(st))
        else:
            rc = self.abi.lib.mt_raytree_update_materials(t, ctypes.addressof(st))
        out = st.as_dict()
        if call == "regrow":
            out.update(info.as_dict())
        return rc, self.abi.last_error() if rc != MT_OK else "", out

    def assert_stale(self, name, what, lights=None):
        lights = self.state["lights"] if lights is None else lights
        with pytest.raises(RuntimeError, match=STALE):
            self.abi.raytree_shade(self.trees[name], lights)
        with pytest.raises(RuntimeError, match=STALE):
            self.abi.raytree_shade_colors(self.trees[name], lights)

    def call(self, name, call, check=True, what=""):
        """One call of a step on one tree, and checkpoint A behind it."""
        what = "%s %s %s" % (what, name, call if isinstance(call, str) else "update_lights%s" % (call[1],))
        model, t, s = self.models[name], self.trees[name], self.state
        p = model.predict(s, call)
        if not isinstance(call, str):
            if p["outcome"] == "stale":
                before = self.planes(name)
                with pytest.raises(RuntimeError, match=STALE):
                    self.abi.raytree_update_lights(t, call[1])
                assert not planes_differing(self.planes(name), before, what + " refused as stale")
                print("%s: stale" % what)
                return p
            st = self.abi.raytree_update_lights(t, call[1])
            assert st["rays_primary"] == st["rays_secondary"] == st["shaded_hits"] == 0
            model.update_lights(s, call[1])
            print("%s: ok, rays_shadow %d" % (what, st["rays_shadow"]))
            if check and None not in model.held:
                self.check_tree(name, what)
            return p
        before, info_before = self.planes(name), self.info(name)
        rc, text, out = self.raw_sync(name, call)
        print("%s: predicted %s, rc %d %s" % (what, p["outcome"], rc, text))
        if p["outcome"] == "light_count":  # the regrow's check (4): before any device call, the tree untouched
            assert rc == MT_ERR_ARG and ("the scene has %d lights, the ray tree was made with %d" % (p["scene"], p["tree"])) in text, (what, rc, text)
            assert not planes_differing(self.planes(name), before, what + ": after the light count refusal")
            assert self.info(name) == info_before and all(out[k] == 0 for k in COUNTS), (what, out)
            assert self.abi.raytree_attr_info(t) == dict(renormaled=0, reuvwed=0, respawned=0), what
            # still stale (shaded under as many lights as the tree was made with: the stale check is a shade call's last)
            self.assert_stale(name, what, model.synced["lights"])
            return p
        if p["outcome"].startswith("unsupported"):
            assert rc == MT_ERR_UNSUPPORTED, (what, rc, text)
            if p["outcome"] == "unsupported_shape":
                m = re.search(r"change the shape of the ray tree: (\d+) rays spawn other children, the first in layer (\d+) at ray (\d+)", text)
                assert m, (what, text)
                assert (int(m.group(1)), (int(m.group(2)), int(m.group(3)))) == (p["count"], p["first"]), (what, text, p["count"], p["first"])
            elif p["outcome"] == "unsupported_textured":
                assert ("material %d has a texture and its ambient or tex changed" % TO_DENSE[p["material"]]) in text, (what, text)
            elif p["outcome"] == "unsupported_no_tri":
                assert ("%d triangles were given another material after the ray tree was made, the first is triangle %d:" % (
                    p["count"], p["first"])) in text and "keeps no tri" in text, (what, text, p)
            elif p["outcome"] == "unsupported_textured_target":
                assert ("triangle %d was given material %d, which has a texture" % (p["triangle"], TO_DENSE[p["material"]])) in text, (what, text, p)
            elif p["outcome"] == "unsupported_attr_no_tri":
                assert ("the %s of %d triangles was set after the ray tree was made, the first is triangle %d:" % (
                    p["attr"], p["count"], p["first"])) in text and "keeps no tri" in text, (what, text, p)
            elif p["outcome"] == "unsupported_normals":
                m = re.search(r"the new normals move reflected rays of the ray tree: (\d+) rays on edited triangles have a reflected "
                              r"child, the first in layer (\d+) at ray (\d+)", text)
                assert m, (what, text)
                assert (int(m.group(1)), (int(m.group(2)), int(m.group(3)))) == (p["count"], p["first"]), (what, text, p)
            else:
                assert ("texture %d was set after the ray tree was made and material %d uses it" % (p["texture"], TO_DENSE[p["material"]])) in text, (what, text)
            assert not planes_differing(self.planes(name), before, what + ": after the refusal")
            assert self.info(name) == info_before, what
            assert all(out[k] == 0 for k in COUNTS), (what, out)
            assert self.abi.raytree_attr_info(t) == dict(renormaled=0, reuvwed=0, respawned=0), what
            self.assert_stale(name, what)
            return p
        assert rc == MT_OK, (what, rc, text)
        if p["outcome"] == "ok_nothing_to_do":
            assert out["kernel_ms"] == 0.0 and all(out[k] == 0 for k in COUNTS), (what, out)
            assert not planes_differing(self.planes(name), before, what + ": nothing to do")
            assert self.info(name) == info_before, what
        else:
            assert out["kernel_ms"] > 0.0, (what, out)
        model.commit(s, p)
        attr = self.abi.raytree_attr_info(t)
        assert attr == {k: p[k] for k in es.ATTR_COUNTS}, (what, attr, {k: p[k] for k in es.ATTR_COUNTS})
        got = {k: out[k] for k in COUNTS}
        assert got == dict(rays_primary=0, rays_secondary=p["rays_secondary"], shaded_hits=p["shaded_hits"], rays_shadow=p["rays_shadow"]), (what, got, p)
        if call == "regrow":
            print("%s: regrown %d, rays %s, kept %s traced %s dropped %s, shadow %d, attr %s" % (
                what, out["regrown"], p["n_rays"], out["kept"], out["traced"], out["dropped"], out["rays_shadow"], attr))
            assert out["regrown"] == p["regrown"], what
            assert (out["kept"], out["traced"], out["dropped"]) == (p["kept"], p["traced"], p["dropped"]), (what, out, p)
            assert out["n_layers_before"] == len(p["dropped"]) and out["n_layers_after"] == len(p["n_rays"])
        assert self.info(name)["n_rays"][:len(p["n_rays"])] == p["n_rays"] and self.info(name)["n_layers"] == len(p["n_rays"]), what
        if check and None not in model.held:
            self.check_tree(name, what)
            # a second sync call has nothing to do, and says so
            rc, text, again = self.raw_sync(name, call)
            assert rc == MT_OK and again["kernel_ms"] == 0.0 and all(again[k] == 0 for k in COUNTS), (what, rc, text, again)
        return p

    def check_tree(self, name, what):
        """Checkpoint A, 2 to 4, of a tree the model calls fresh: the truth, a tree newly created on a scene newly
        created from the state's description, mt_raytree_info, the shaded frame."""
        model, t, s = self.models[name], self.trees[name], self.state
        assert not model.stale(s)
        lights = es.lights_at(s, model.held)  # the state's colours, the tree's positions
        got = self.planes(name)
        self.assert_truth(name, got, what + " vs the truth")
        fh, ft = self.fresh_tree(model.synced, lights, name)
        want = self.planes_of(ft)
        assert not planes_differing(got, want, what + " vs a fresh tree on a fresh scene")
        self.check_bytes(what)
        fi = self.abi.raytree_info(ft)
        assert self.info(name) == {k: fi[k] for k in INFO_KEYS}, (what, self.info(name), fi)
        rgb = self.abi.raytree_shade(t, lights)["rgb"]
        assert differing(rgb, self.abi.raytree_shade(ft, lights)["rgb"], what + ": shaded vs the fresh tree, shaded") == 0
        spec = model.spec
        if spec != "list":
            assert differing(rgb, self.frame(fh, DEPTH, spec), what + ": shaded vs mt_render_chunk on the fresh scene") == 0
            if model.settled(s):
                assert differing(rgb, self.frame(self.h, DEPTH, spec), what + ": shaded vs mt_render_chunk on the live scene") == 0
            assert_rgb_close(rgb, es.oracle_frame(s, DEPTH, spec, held=model.held), what + ": shaded vs the oracle")
        colors = self.abi.raytree_shade_colors(t, lights)["color"]
        assert differing(rr.v3d_to_rgb(colors.reshape(-1, 3)).reshape(rgb.shape), rgb, what + ": colours, quantised") == 0

    def run(self, steps, what, scene_checks=True, claims=False):
        """claims: every step's claim is held on the trees es.CLAIM_TREES (es.hold_claim), on the predictions
        the calls were held to and on the model's trees, which the read-backs were held to."""
        for i, st in enumerate(steps):
            before = {name: es.copy_tree(m.tree) for name, m in self.models.items()} if claims else {}
            for op in st["ops"]:
                self.apply(op)
            label = "%s step %d" % (what, i)
            if scene_checks and st["ops"]:
                self.checkpoint_b(label)
            for name, calls in st["calls"].items():
                mine = [(call, self.call(name, call, st["check"], label)) for call in calls]
                if claims and st["claim"] and name in es.CLAIM_TREES:
                    es.hold_claim(st["claim"], mine, before[name], self.models[name], self.state)
            self.end_step()


@pytest.fixture
def live(flat0):
    made = []

    def _make(names=(), engine=None):
        made.append(Live(flat0, names, engine))
        return made[-1]
    yield _make
    for s in made:
        s.close()


# ---- session 1: the shape walk

def test_session_1_shape_walk(live):
    """The eight states of the shape walk, one set_materials + regrow per step on the frame's, the chunk's and the ray
    list's tree: the layer count goes 3 -> 6 -> 4 -> 4 -> 2 -> 2 -> 4 -> 3, so every scratch buffer shrinks and grows
    again and mt_raytree_info's bytes is patched seven times.  Back under A the trees are the first read-back."""
    s = live(es.WALK_TREES)
    steps = es.session_shape_walk()
    for i, (st, row) in enumerate(zip(steps, es.SHAPE_WALK)):
        s.run([st], "shape walk, %s:" % row[0])
        assert s.info("full")["n_rays"][:len(row[2])] == row[2]
    for name in es.WALK_TREES:
        assert not planes_differing(s.planes(name), s.first[name], "shape walk: %s back under A vs the first read-back" % name)


# ---- session 2: pending edits

def test_session_2a_a_pile_of_edits_then_one_regrow(live):
    s = live(es.WALK_TREES)
    s.run(es.session_pile(), "pile")
    assert s.info("full")["n_rays"][:6] == [1536, 1100, 668, 248, 33, 5]


def test_session_2b_refused_then_one_edit_reverted(live):
    """update_materials refuses the pile for the shape and must leave nothing half-applied: with the matte edit alone
    reverted it takes the rest -- a retexture from both texture sets and the moved tex, no shadow ray."""
    s = live(("full", "chunk"))
    steps = es.session_refused_then_reverted()
    s.run(steps[:1], "refused")
    for name in ("full", "chunk"):
        assert s.models[name].stale(s.state)
    s.run(steps[1:], "reverted")
    for name in ("full", "chunk"):
        assert not s.models[name].stale(s.state)
        changed = sum(not ru.same_plane(g["albedo"], w["albedo"]) for g, w in zip(s.planes(name), s.first[name]))
        assert changed > 0, name


def test_session_2c_a_net_zero_pile(live):
    """Edits all undone before the sync, and one set of a texture no material uses: the generation moved, the diff asks
    for nothing -- no kernel, no bit."""
    s = live(("full", "chunk", "list", "plain"))
    s.run(es.session_net_zero(), "net zero")
    for name in s.trees:
        assert not planes_differing(s.planes(name), s.first[name], "net zero: %s vs the first read-back" % name)
        s.abi.raytree_shade(s.trees[name], s.state["lights"])  # (fresh)


def test_session_2d_three_rhythms(live):
    """The frame's tree syncs after every op, the chunk's once at the end, the tree without uvw is asked at every op."""
    s = live(("full", "chunk", "plain"))
    steps = es.session_three_rhythms()
    outcomes = []
    for i, st in enumerate(steps):
        for op in st["ops"]:
            s.apply(op)
        for name, calls in st["calls"].items():
            for call in calls:
                p = s.call(name, call, True, "rhythms step %d" % i)
                if name == "plain":
                    outcomes.append(p["outcome"])
        s.end_step()
    print("the tree without uvw:", outcomes)
    assert outcomes == ["ok", "ok", "unsupported_textured", "ok_nothing_to_do", "unsupported_texture_set",
                        "unsupported_texture_set", "unsupported_texture_set", "unsupported_textured"]
    # the two trees with uvw, synced in different rhythms, each against its own truth on the common state
    for name in ("full", "chunk"):
        assert not s.models[name].stale(s.state)
        s.check_tree(name, "rhythms: %s at the end" % name)
    s.end_step()


# ---- session 3: lights interleaved

def test_session_3_lights_interleaved(live):
    s = live(es.LIGHT_TREES)
    steps = es.session_lights()
    for i, st in enumerate(steps):
        before = {name: s.planes(name) for name in s.trees}
        s.run([st], "lights")
        kind, index = st["claim"]
        if kind == "mixed":  # (the regrow changed the tree's shape; its checkpoint is the next step's)
            continue
        for name in s.trees:
            bad = planes_differing(s.planes(name), before[name], "lights step %d %s (%s)" % (i, name, kind))
            if kind == "no bit":   # the shadow-relevant update before it traced ALL lights at the scene's positions
                assert not bad, (i, name)
            elif kind in ("light", "new position") and name != "list":
                assert bad and {p for _, p in bad} <= {"power", "in_shadow"}, (i, name, bad)
            elif kind == "old position":
                assert {p for _, p in bad} <= {"albedo"}, (i, name, bad)
                assert s.models[name].pending_lights(s.state) == [index]


# ---- session 4: the deferred planes

def test_session_4_deferred_planes(live):
    """The G-buffer and the light buffer of the start state, caller-owned planes on the host, taken through the shape
    walk plus texture steps and a moved light: mt_retexture_gbuffer after each edit, mt_update_lightbuffer over all
    lights after a shadow-relevant edit and over the moved index after a moved light."""
    s = live(())
    abi = s.abi
    gb = abi.render_gbuffer(s.h, sensor(), W, H)
    gb.pop("stats")
    lb = abi.render_lightbuffer(s.h, sensor(), W, H, 2)
    lb = dict(power=lb["power"], in_shadow=lb["in_shadow"])
    for i, st in enumerate(es.session_deferred()):
        was = s.state
        for op in st["ops"]:
            s.apply(op)
        now = s.state
        what = "deferred step %d" % i
        out = abi.retexture_gbuffer(s.h, gb)
        assert all(out["stats"][k] == 0 for k in binding.STAT_NAMES)
        gb["albedo"] = out["albedo"]
        moved = [k for k, (a, b) in enumerate(zip(es.positions(was), es.positions(now))) if a != b]
        which = [0, 1] if rg.shadow_relevant(es.oracle_materials(was), es.oracle_materials(now)) else moved
        if which:
            abi.update_lightbuffer(s.h, gb, lb, which)
        print("%s: %s, lights traced again %s" % (what, [op[0] for op in st["ops"]], which))
        f = s.fresh_scene(now, now["lights"])["h"]
        want = te.albedo(dense_materials(now), now["texs"], gb["material"], gb["uvw"]).reshape(gb["albedo"].shape)
        assert same_bits(gb["albedo"], want, what + ": albedo vs the restatement") == 0
        fg = abi.render_gbuffer(f, sensor(), W, H)
        assert same_bits(gb["albedo"], fg["albedo"], what + ": albedo vs a fresh G-buffer") == 0
        fl = abi.render_lightbuffer(f, sensor(), W, H, 2)
        assert same_bits(lb["power"], fl["power"], what + ": power vs a fresh light buffer") == 0
        assert np.array_equal(lb["in_shadow"], fl["in_shadow"]), what
        direct = abi.shade_direct(s.h, sensor(), W, H, gb, lb, now["lights"])["rgb"]
        assert differing(direct, s.frame(f, 0), what + ": mt_shade_direct vs depth 0 on a fresh scene") == 0
        assert differing(direct, s.frame(s.h, 0), what + ": mt_shade_direct vs depth 0 on the live scene") == 0
        assert_rgb_close(direct, es.oracle_frame(now, 0), what + ": mt_shade_direct vs the oracle's depth-0 frame")
        if i + 1 == len(es.session_deferred()):  # no edit of the session moved a primary hit
            for name in ("material", "uvw", "point", "normal", "prim", "depth", "line_no"):
                assert ru.same_plane(gb[name], fg[name]), name
        s.end_step()


# ---- session 5: frames between edits, with a warmed history

@pytest.mark.parametrize("engine", ["state_machine", "ray_pool", "hybrid", "auto"])
def test_session_5_frames_between_edits(engine, live):
    """Four frames of one camera -- the cost history, the forecasts and, where its conditions hold, the lean kernel are
    in play --, then per step of the shape walk one edit and two frames: every frame is the FIRST frame of a scene newly
    created from the state (which has no history), byte for byte, while the ray counts triple between two frames."""
    number = {"state_machine": 1, "ray_pool": 2, "hybrid": 3, "auto": 0}[engine]
    for knob in (1, 2):  # (2 only if the automatic rule declines on this camera: tests/test_gpu_lean_kernel.py)
        s = live((), engine=number)
        s.abi.set_tuning(s.h, "LEAN_KERNEL", float(knob))
        lean_after_an_edit = 0

        def frames(n, what, after_edit):
            nonlocal lean_after_an_edit
            want = s.frame(s.fresh_scene(s.state, s.state["lights"])["h"])
            for k in range(n):
                got = s.frame(s.h)
                info = s.abi.lean_info(s.h)
                print("%s %s frame %d: lean %d handed_over %d units %d redo %d" % (
                    engine, what, k, info["lean"], info["handed_over"], info["units"], info["redo_units"]))
                assert differing(got, want, "%s %s frame %d vs a fresh scene's first frame" % (engine, what, k)) == 0
                lean_after_an_edit += int(after_edit and info["lean"] == 1)
            s.end_step()

        frames(4, "start", False)
        for st, row in zip(es.session_shape_walk(), es.SHAPE_WALK):
            for op in st["ops"]:
                s.apply(op)
            frames(2, row[0], True)
        print("%s, LEAN_KERNEL %d: %d frames after an edit ran lean" % (engine, knob, lean_after_an_edit))
        if engine != "state_machine" or lean_after_an_edit:
            break
    if engine == "state_machine":
        assert lean_after_an_edit >= 1


# ---- session 6: seeded

@pytest.mark.parametrize("seed", es.SEEDS, ids=hex)
def test_session_6_seeded(seed, live):
    """24 ops on all four trees, a sync call after every op (update_materials or the regrow, the generator's choice; a
    moved light's update_lights first), checkpoint A every time."""
    s = live(es.ALL_TREES)
    s.run(es.generate(seed), "seed %#x" % seed, scene_checks=False)
    s.checkpoint_b("seed %#x at the end" % seed)
    s.end_step()


# ---- session 7: the facade

def test_session_7_facade():
    """UpdateTexture, UpdateMaterials, RegrowRayTree, UpdateRayTree in one chain on one MythTracer: session 2a's pile and
    a moved light, against a facade object that loaded the edited scene."""
    state = es.start_state()
    m = es.build_scene(M.MythTracer(), state)
    m.set_lights(state["lights"])
    m.set_max_level(DEPTH)
    m.set_raytree_keep_uvw(True)
    first = m.render(CAM, W, H)["rgb"]
    field = {"Ka": "ka", "Kd": "kd", "Ks": "ks", "Ns": "ns", "Refl": "refl", "Tr": "tr", "Tf": "tf", "Ni": "ni"}
    with m.raytree(CAM, W, H) as tree:
        for op, _ in es.PILE:
            state = es.apply(state, op)
            if op[0] == "mat":
                m.update_materials({es.NAMES[op[1]]: {field[k]: v for k, v in op[2].items()}})
            elif op[0] == "tex":
                m.update_texture("tex%d" % op[1], te.texel_values(state["texs"][op[1]]))
            else:
                m.set_material_texture(op[1], op[2])
                m.update_materials()
        with pytest.raises(RuntimeError, match=STALE):
            tree.shade()
        with pytest.raises(RuntimeError, match="change the shape"):
            tree.update_materials()
        out = tree.regrow()
        print("facade: regrow", out["counters"], tree.info["n_rays"])
        state = es.apply(state, ("move_light", 1, es.LIGHT_MOVES[0][1]))
        up = tree.update([1], lights=state["lights"])
        print("facade: update", up["counters"])
        built = es.build_scene(M.MythTracer(), state)
        built.set_lights(state["lights"])
        built.set_max_level(DEPTH)
        built.set_raytree_keep_uvw(True)
        want = built.render(CAM, W, H)["rgb"]
        got = m.render(CAM, W, H)["rgb"]
        assert differing(got, first, "facade: the edited frame vs the first (expected to differ)") > 0
        assert differing(got, want, "facade: the edited frame vs a facade that loaded the edited scene") == 0
        assert_rgb_close(got, es.oracle_frame(state), "facade: the edited frame vs the oracle")
        assert differing(tree.shade()["rgb"], want, "facade: the tree, shaded") == 0
        with built.raytree(CAM, W, H) as fresh:
            gi, wi = tree.info, fresh.info
            assert (gi["n_layers"], gi["n_rays"], gi["bytes"]) == (wi["n_layers"], wi["n_rays"], wi["bytes"])
            assert out["counters"]["rays_secondary"] == sum(wi["n_rays"]) - sum(es.SHAPE_WALK_A)
            abi = M.hip_abi()
            for k in range(gi["n_layers"]):
                a, b = tree.layer(k), fresh.layer(k)
                a["uvw"], b["uvw"] = abi.raytree_read_uvw(tree._tree(), k), abi.raytree_read_uvw(fresh._tree(), k)
                assert not planes_differing([a], [b], "facade: layer %d vs the loaded scene's tree" % k)
        built.close()
    m.close()


# ---- the newer edit kinds in the chain: mt_scene_set_triangle_materials / _normals / _uvw, trees with every switch
# combination (es.NEW_TREES, all made on ONE live scene by toggling the two switches between creations).  Checkpoint A
# after every call, as above, plus the tri plane, mt_raytree_attr_info_last, the getters and the bytes rule.

def tri_trees(names):
    return [n for n in names if es.NEW_TREES[n][2]]


def test_session_a_stamp_walk(live):
    """Normals of the matte box, uvw of the floor, normals of the mirror (the update refused, the tree untouched and still
    stale, the regrow respawns and renormals mirror rays ONLY), the same set again (nothing moves), the mirror back
    (A -> B -> A is dirty: refused again; after the regrow every plane is the read-back after step 1)."""
    s = live(tuple(es.NEW_TREES))
    steps = es.session_stamp_walk()
    s.run(steps[:2], "stamp walk a", claims=True)
    after_uvw = {n: s.planes(n) for n in tri_trees(s.trees)}
    s.run(steps[2:3], "stamp walk b", claims=True)
    assert s.abi.raytree_attr_info(s.trees["full_tu"]) == dict(renormaled=0, reuvwed=0, respawned=0)  # (the second sync's)
    s.run(steps[3:], "stamp walk c", claims=True)
    for n in after_uvw:
        assert not planes_differing(s.planes(n), after_uvw[n], "stamp walk: %s with the mirror back vs after step 1" % n)


def test_session_b_assignment_walk(live):
    """matte -> mirror (grows), pane -> wall (shadow-visible, subtrees drop), the box -> the textured floor (the tree with
    tri but without uvw refuses, naming triangle and material, and stays stale), everything back: CHANGED against the
    LAST SUCCESSFUL sync decides.  Back under the start state every tree is its first read-back."""
    s = live(tuple(es.NEW_TREES))
    s.run(es.session_assignment_walk(), "assignment walk", claims=True)
    assert s.info("full_tu")["n_rays"][:3] == es.SHAPE_WALK_A
    for n in s.trees:
        assert not s.models[n].stale(s.state), n
        assert not planes_differing(s.planes(n), s.first[n], "assignment walk: %s back under the start vs the first read-back" % n)


def test_session_c_the_pile_in_both_orders(live):
    """Six edits before one sync -- the floor's Refl flipped, one matte triangle given the mirror's material, the matte
    normals tilted (the new reflected children start from the NEW normal), floor uvw x 2, texture 0 replaced, the other
    matte triangle given the textured floor's material --: the update refuses for the shape, one regrow takes all six.
    The same pile in the other order on a second scene gives the same trees."""
    a, b = live(es.PILE_TREES), live(es.PILE_TREES)
    a.run(es.session_new_pile(), "pile", claims=True)
    b.run(es.session_new_pile(reverse=True), "pile reversed", claims=True)
    assert a.info("full_tu")["n_rays"][:4] == es.NEW_PILE_FULL[1]
    for n in es.PILE_TREES:
        assert not planes_differing(a.planes(n), b.planes(n), "pile: %s vs the other order" % n)


def test_session_d_trees_in_different_rhythms(live):
    """The full tree syncs after every op, the chunk after every third, the list once at the end; the trees without tri
    are asked at every op and stay refused from the first attribute set on, with counts that grow with the stamps."""
    s = live(es.RHYTHM_TREES)
    told = []
    for i, st in enumerate(es.session_new_rhythms()):
        for op in st["ops"]:
            s.apply(op)
        for name, calls in st["calls"].items():
            for call in calls:
                p = s.call(name, call, True, "rhythms step %d" % i)
                if name == "full_u":
                    told.append((p["outcome"], p.get("count")))
        s.end_step()
    print("the tree with uvw and without tri:", told)
    assert told[0] == ("ok", None) and all(o.startswith("unsupported") for o, _ in told[1:])
    assert told[1] == ("unsupported_attr_no_tri", 2) and told[-1] == ("unsupported_attr_no_tri", 4)
    for name in ("full_tu", "chunk_tu", "list_tu"):
        assert not s.models[name].stale(s.state)
        s.check_tree(name, "rhythms: %s at the end" % name)
    s.end_step()


def test_session_e_lights_between_the_new_edits(live):
    """A moved light pending across a shadow-visible reassignment: all lights are traced again at the current positions,
    and update_lights then changes no bit.  A moved light pending across a uvw-only edit: the old planes are kept, then
    update_lights catches up.  A normal edit's regrow under another light COUNT is refused by check (4) (MT_ERR_ARG) with
    the tree untouched, and taken once the count is restored."""
    s = live(es.NEW_LIGHT_TREES)
    for i, st in enumerate(es.session_new_lights()):
        before = {name: s.planes(name) for name in s.trees}
        s.run([st], "new lights", claims=True)
        kind, index = st["claim"]
        for name in s.trees:
            bad = planes_differing(s.planes(name), before[name], "new lights step %d %s (%s)" % (i, name, kind))
            if name not in st["calls"]:
                continue
            if kind in ("no bit", "light count"):
                assert not bad, (i, name)
            elif kind == "all lights" and name != "list_tu":  # the moved light's planes of layer 0 hold the new position
                assert (s.planes(name)[0]["in_shadow"][index] != before[name][0]["in_shadow"][index]).any(), (i, name)
                assert s.models[name].settled(s.state)
            elif kind == "respawn":
                assert (0, "normal") in bad and (1, "ray") in bad, (i, name, bad)  # (the children start from the new normal)
            elif kind == "old position":
                assert {p for _, p in bad} <= {"albedo", "uvw"}, (i, name, bad)
                assert s.models[name].pending_lights(s.state) == [index]
            elif kind == "new position" and name != "list_tu":
                assert bad and {p for _, p in bad} <= {"power", "in_shadow"}, (i, name, bad)


@pytest.mark.parametrize("seed", es.NEW_SEEDS, ids=hex)
def test_session_h_seeded_with_the_new_kinds(seed, live):
    """24 ops, about half of them reassignments and attribute sets and their inverses, on all six tree kinds, a sync call
    per tree after every op, checkpoint A every time."""
    s = live(tuple(es.NEW_TREES))
    s.run(es.generate_new(seed), "seed %#x" % seed, scene_checks=False)
    s.checkpoint_b("seed %#x at the end" % seed)
    s.end_step()


@pytest.mark.parametrize("engine", ["state_machine", "ray_pool", "hybrid", "auto"])
def test_session_f_frames_between_the_new_edits(engine, live):
    """Session 5 with the newer kinds: four frames of one camera warm the cost history (MT_TUNE_LEAN_KERNEL = 2), then
    per op of es.FRAME_OPS one edit and one frame: the FIRST frame of a scene newly created from the state, byte for
    byte, and the oracle's under the pow rule.  After three of the ops also the supersampled and adaptive frames, a new
    G-buffer and a new light buffer against the fresh scene's."""
    number = {"state_machine": 1, "ray_pool": 2, "hybrid": 3, "auto": 0}[engine]
    s = live((), engine=number)
    s.abi.set_tuning(s.h, "LEAN_KERNEL", 2.0)
    for k in range(4):
        assert differing(s.frame(s.h), s.frame(s.fresh_scene(s.state, s.state["lights"])["h"]), "%s warm frame %d" % (engine, k)) == 0
        s.end_step()
    sens, sens2 = sensor(), binding.sensor(CAM, 2 * W, 2 * H)
    lean = 0
    for i, op in enumerate(es.FRAME_OPS):
        s.apply(op)
        what = "%s frame after op %d (%s)" % (engine, i, op[0])
        f = s.fresh_scene(s.state, s.state["lights"])["h"]
        got = s.frame(s.h)
        lean += s.abi.lean_info(s.h)["lean"] == 1
        assert differing(got, s.frame(f), what + " vs a fresh scene's first frame") == 0
        assert_rgb_close(got, es.oracle_frame(s.state), what + " vs the oracle")
        if i in es.FRAME_EXTRAS:
            abi = s.abi
            assert differing(abi.render_chunk_ss(s.h, sens2, W, H, 2)["rgb"], abi.render_chunk_ss(f, sens2, W, H, 2)["rgb"], what + " ss = 2") == 0
            a, b = abi.render_chunk_adaptive(s.h, sens, sens2, W, H, 2, 16), abi.render_chunk_adaptive(f, sens, sens2, W, H, 2, 16)
            assert differing(a["rgb"], b["rgb"], what + " adaptive") == 0 and np.array_equal(a["mask"], b["mask"])
            gb, gbf = abi.render_gbuffer(s.h, sens, W, H), abi.render_gbuffer(f, sens, W, H)
            for plane in binding.GBUFFER_PLANES:
                assert ru.same_plane(gb[plane], gbf[plane]), (what, plane)
            lb, lbf = abi.render_lightbuffer(s.h, sens, W, H, 2), abi.render_lightbuffer(f, sens, W, H, 2)
            assert ru.same_plane(lb["power"], lbf["power"]) and np.array_equal(lb["in_shadow"], lbf["in_shadow"]), what
        s.end_step()
    print("%s: %d of %d frames after an edit ran lean" % (engine, lean, len(es.FRAME_OPS)))
    if engine == "state_machine":  # (the lean kernel is the state machine's: as session 5)
        assert lean >= 1


def test_session_g_facade_chain():
    """UpdateTriangleMaterials, UpdateTriangleAttributes, UpdateRayTreeMaterials and RegrowRayTree in one short session,
    against a facade object BUILT from the state after every sync.  The facade refuses a RayTree with several devices, so
    the same edit calls go to two objects: `m`, whose tree is held to the truth, and `two`, with two replicas on one
    device, whose frame (the W x H overload, both replicas) is held to the built scene's."""
    state = es.start_state()
    abi = M.hip_abi()

    def facade(state, devices=None):
        f = es.build_scene(M.MythTracer(), state)
        if devices:
            f.set_devices(devices)
        f.set_lights(state["lights"])
        f.set_max_level(DEPTH)
        f.set_raytree_keep_uvw(True)
        f.set_raytree_keep_triangles(True)
        return f
    m, two = facade(state), facade(state, [0, 0])
    assert differing(two.render_image(CAM, W, H), m.render(CAM, W, H)["rgb"], "facade chain: two replicas at the start") == 0

    def push(op):
        tris = sorted(op[1])
        for f in (m, two):
            if op[0] == "assign":
                for t in tris:
                    f.assign_material([t], es.NAMES[op[1][t]] if op[1][t] >= 0 else None)
                f.update_triangle_materials()
            else:
                (f.set_triangle_normals if op[0] == "normals" else f.set_triangle_uvw)(tris, [op[1][t] for t in tris])
                f.update_triangle_attributes()

    chain = [
        ([es.edit("assign", "matte->mirror"), es.edit("normals", "matte tilt"), es.edit("uvws", "floor x2")], "change the shape"),
        ([es.edit("uvws", "nan swap"), es.edit("normals", "mirror tilt")], "the new normals move reflected rays"),
        ([es.original("assign", (6, 7)), es.edit("assign", "floor->none"), es.original("normals", (4, 5, 6, 7)), es.original("uvws", (0, 1))],
         "change the shape"),
    ]
    model = es.Tree("full_tu", state)
    with m.raytree(CAM, W, H) as tree:
        for i, (ops, refusal) in enumerate(chain):
            for op in ops:
                state = es.apply(state, op)
                push(op)
            what = "facade chain step %d" % i
            with pytest.raises(RuntimeError, match=STALE):
                tree.shade()
            refused = model.predict(state, "update_materials")["outcome"]
            assert refused == ("unsupported_shape" if refusal.startswith("change") else "unsupported_normals"), (what, refused)
            with pytest.raises(RuntimeError, match=refusal):
                tree.update_materials()
            p = model.predict(state, "regrow")
            out = tree.regrow()
            model.commit(state, p)
            print(what, out["counters"], tree.info["n_rays"], tree.attr_info())
            assert tree.attr_info() == {k: p[k] for k in es.ATTR_COUNTS}, what
            assert out["counters"]["rays_secondary"] == p["rays_secondary"] and out["counters"]["rays_shadow"] == p["rays_shadow"], what
            built = facade(state)
            want = built.render(CAM, W, H)["rgb"]
            got = m.render(CAM, W, H)["rgb"]
            assert differing(got, want, what + ": the frame vs a facade built from the state") == 0
            assert_rgb_close(got, es.oracle_frame(state), what + ": the frame vs the oracle")
            assert differing(two.render_image(CAM, W, H), want, what + ": the two replicas' frame") == 0
            assert differing(tree.shade()["rgb"], want, what + ": the tree, shaded") == 0
            with built.raytree(CAM, W, H) as fresh:
                gi, wi = tree.info, fresh.info
                assert (gi["n_layers"], gi["n_rays"], gi["bytes"]) == (wi["n_layers"], wi["n_rays"], wi["bytes"]), what
                assert gi["n_rays"][:gi["n_layers"]] == p["n_rays"]
                for k in range(gi["n_layers"]):
                    a, b = tree.layer(k), fresh.layer(k)
                    a["uvw"], b["uvw"] = abi.raytree_read_uvw(tree._tree(), k), abi.raytree_read_uvw(fresh._tree(), k)
                    a["tri"], b["tri"] = abi.raytree_read_tri(tree._tree(), k), abi.raytree_read_tri(fresh._tree(), k)
                    # (a facade numbers its materials by first use, so the built one's numbering is another after a
                    # reassignment: the material plane is held to the model's, in m's numbering)
                    assert np.array_equal(a.pop("material"), dense_plane(model.tree["layers"][k]["material"])), (what, k)
                    b.pop("material")
                    assert not planes_differing([a], [b], what + ": layer %d vs the built scene's tree" % k)
            built.close()
    m.close()
    two.close()
