"""The edit sessions of tests/edit_session_ref.py pinned with the oracle alone (no GPU): the model's `chained` tree
equals a fresh raytree_ref.build at every sync of every scripted session and every seed; every op of the scripted
sessions changes what it claims to change; session 1's shapes are the literal numbers of its table; the seeded
generator meets its conditions.  tests/test_gpu_edit_sessions.py holds the kernels to the same model.

The second half does the same for the newer edit kinds (reassignments, vertex normals, texture coordinates; the sessions
of es.NEW_SCRIPTED and the seeds es.NEW_SEEDS): the state builds the scene triangle by triangle, the generations and
stamps move as the header says, every op of the menus changes what it claims, every scripted step holds its claim, the
pinned literals of sessions a to e, the per-seed floors, and vertex_attr_ref.match against regrow_ref.match where no
normal changed.
"""
import collections
import hashlib

import numpy as np
import pytest

import edit_session_ref as es
import material_edit_ref as me
import orclib
import regrow_ref as rg
import texture_edit_ref as te
import vertex_attr_ref as va

SESSIONS = list(es.SCRIPTED) + ["seed %#x" % s for s in es.SEEDS]


def script_of(name):
    if name in es.SCRIPTED:
        fn, trees = es.SCRIPTED[name]
        return fn(), trees
    return es.generate(int(name.split()[1], 16)), es.ALL_TREES


def replay(name):
    """Yields (step index, step, state before, state after, trees, log) with the model's side of the step done."""
    steps, names = script_of(name)
    state = es.start_state()
    trees = es.make_trees(state, names)
    for i, st in enumerate(steps):
        before = state
        for op in st["ops"]:
            state = es.apply(state, op)
        log = []
        es.run_step(trees, state, st, log)
        yield i, st, before, state, trees, log


def test_the_state_builds_the_tiny_scene():
    """The model's tables are the oracle's: a scene built from the start state is texture_edit_ref's tiny scene, and one
    built from an edited state holds the edit."""
    a = es.start_state()
    want = te.build_tiny(orclib.OracleScene(), textures=te.tiny_textures())
    for (n1, v1, t1), (n2, v2, t2), (n3, v3, t3) in zip(es.oracle(a).materials(), want.materials(), es.oracle_materials(a)):
        assert n1 == n2 == n3 and t1 == t2 == t3 and np.array_equal(v1, v2) and np.array_equal(v1, v3)
    b = es.apply(es.apply(a, es.mat(es.PANE, Tf=(0.5, 0.25, 1.0), Ni=1.5)), ("tex_move", es.MATTE, 2))
    for (n1, v1, t1), (n3, v3, t3) in zip(es.oracle(b).materials(), es.oracle_materials(b)):
        assert n1 == n3 and t1 == t3 and np.array_equal(v1, v3)
    assert b["gen"] == 2 and b["tex_gen"] == [0, 0, 0]
    assert es.apply(b, es.mat(es.PANE, Ni=1.5))["gen"] == 2  # (no bit changed: the generation stays)
    assert es.apply(b, ("tex", 2, "original"))["gen"] == 3     # (a texture set always counts)


@pytest.mark.parametrize("name", SESSIONS)
def test_chained_equals_a_fresh_build_at_every_sync(name):
    """`chained` -- regrow_ref.regrow / the commit rule, fed the assembled tree of the step before -- against `truth`, a
    fresh build on an oracle scene built from the synced state: every plane of every layer, uvw included, doubles by
    bits with NaN = NaN.  After a refusal the assembled tree is the one before."""
    syncs = 0
    for i, st, _, state, trees, log in replay(name):
        for tree, call, p in log:
            t = trees[tree]
            if None in t.held:
                assert not st["check"], (name, i, tree)
                continue
            bad = es.differing_planes(t.tree, t.truth(), t.keep_uvw)
            assert not bad, (name, i, tree, call, p["outcome"], bad)
            if p["outcome"] in ("ok", "ok_nothing_to_do") and call in ("update_materials", "regrow"):
                assert t.tree["n_rays"] == p["n_rays"] and not t.stale(state)
                syncs += 1
    print("%s: %d successful syncs held to a fresh build" % (name, syncs))
    assert syncs > 0


def frame_pixels_changed(a, b):
    return int((es.oracle_frame(a) != es.oracle_frame(b)).any(axis=-1).sum())


def tree_of(state):
    return es.truth_tree(state, None, es.positions(state))


@pytest.mark.parametrize("name", list(es.SCRIPTED))
def test_every_op_changes_what_it_claims(name):
    """Per op of the scripted sessions, against the state just before it.  A material or texture op: at least 20 rays'
    values in one stored plane of the frame's fresh tree (or 20 rays more or fewer) -- unless only Kd / Ks / Ns / Ni
    change: then at least 20 pixels of the oracle's frame and no stored plane.  A texture no material uses: nothing at
    all.  A moved light: in_shadow of that light in layer 0 and in some layer >= 1, the other light's planes
    untouched.  A light's colours: the frame, no plane."""
    steps, _ = script_of(name)
    state = es.start_state()
    for i, st in enumerate(steps):
        for op in st["ops"]:
            after = es.apply(state, op)
            a, b = tree_of(state), tree_of(after)
            changed = es.changed_rays(a, b)
            what = "%s step %d %s" % (name, i, op)
            print(what, changed)
            if op[0] == "mat" and set(op[2]) <= set(es.SHADE_ONLY) or op[0] == "colour_light":
                assert not changed, what
                assert frame_pixels_changed(state, after) >= 20, what
            elif op[0] == "tex" and op[1] not in after["tex_of"]:
                assert not changed and frame_pixels_changed(state, after) == 0, what
                assert after["gen"] == state["gen"] + 1
            elif op[0] == "move_light":
                assert set(changed) <= {"power", "in_shadow"}, what
                per = [int((x["in_shadow"][op[1]] != y["in_shadow"][op[1]]).sum()) for x, y in zip(a["layers"], b["layers"])]
                other = [int((x["in_shadow"][1 - op[1]] != y["in_shadow"][1 - op[1]]).sum()) +
                         me.differing_entries(dict(p=x["power"][1 - op[1]]), dict(p=y["power"][1 - op[1]]), "p")
                         for x, y in zip(a["layers"], b["layers"])]
                assert per[0] > 0 and sum(per[1:]) > 0 and not any(other), (what, per, other)
            else:
                assert changed and max(changed.values()) >= 20, what
            state = after


def test_the_light_moves_are_the_measured_ones():
    a = es.start_state()
    base = tree_of(a)
    for index, pos, want in es.LIGHT_MOVES:
        b = tree_of(es.apply(a, ("move_light", index, pos)))
        per = [int((x["in_shadow"][index] != y["in_shadow"][index]).sum()) for x, y in zip(base["layers"], b["layers"])]
        assert per == want, (index, pos, per)


def test_regrow_steps_have_their_patterns():
    """Every step whose claim names a pattern: grow = rays traced and none dropped, drop = the reverse, both = both, in
    the frame's tree; a refused step is refused for the shape; a retexture runs no shadow ray; the mixed step leaves
    mixed positions and the next one settles them."""
    seen = collections.Counter()
    for name in es.SCRIPTED:
        for i, st, _, state, trees, log in replay(name):
            if not st["claim"]:
                continue
            kind, arg = st["claim"]
            for tree, call, p in log:
                if tree != "full":
                    continue
                what = (name, i, call, p["outcome"])
                if kind == "regrow":
                    t, d = sum(p["traced"]), sum(p["dropped"])
                    assert p["regrown"] == 1 and (t > 0, d > 0) == dict(grow=(True, False), drop=(False, True), both=(True, True))[arg], (what, t, d)
                elif kind == "refused":
                    assert p["outcome"] == arg, what
                elif kind == "retexture":
                    assert p["outcome"] == "ok" and p["regrown"] == 0 and p["rays_shadow"] == 0, what
                elif kind == "nothing":
                    assert p["outcome"] == "ok_nothing_to_do", what
                elif kind == "all lights":
                    assert p["outcome"] == "ok" and p["rays_shadow"] > 0 and trees[tree].settled(state), what
                elif kind == "old position":
                    assert p["outcome"] == "ok" and p["rays_shadow"] == 0 and trees[tree].pending_lights(state) == [arg], what
                elif kind == "mixed":
                    assert p["outcome"] == "ok" and p["regrown"] == 1 and sum(p["traced"]) > 0 and trees[tree].held[arg] is None, what
                elif kind in ("light", "no bit", "new position"):
                    assert p["outcome"] == "ok" and trees[tree].settled(state), what
                seen[kind] += 1
    print(dict(seen))
    assert all(seen[k] for k in ("regrow", "refused", "retexture", "nothing", "all lights", "old position", "mixed", "no bit"))


def test_session_1_shapes():
    """Depth 5, the full 48 x 32 chunk: rays per layer, kept, traced and dropped of the shape walk, as literal numbers;
    the layer count goes 3 -> 6 -> 4 -> 4 -> 2 -> 2 -> 4 -> 3."""
    assert tree_of(es.start_state())["n_rays"] == es.SHAPE_WALK_A == [1536, 715, 170]
    layers = [3]
    for (i, st, _, _, trees, log), row in zip(replay("shape walk"), es.SHAPE_WALK):
        name, _, n_rays, kept, traced, dropped, _ = row
        p = [p for tree, _, p in log if tree == "full"][0]
        print(name, p["n_rays"], p["kept"], p["traced"], p["dropped"])
        assert p["outcome"] == "ok" and p["regrown"] == 1 and p["n_rays"] == n_rays, name
        for got, want in ((p["kept"], kept), (p["traced"], traced), (p["dropped"], dropped)):
            assert want is None or got == want, (name, got, want)
        assert [k + t for k, t in zip(p["kept"], p["traced"])] == n_rays
        layers.append(len(n_rays))
    assert layers == [3, 6, 4, 4, 2, 2, 4, 3]
    rows = {r[0]: r for r in es.SHAPE_WALK}
    assert rows["matte Refl 0.5"][2:5] == ([1536, 1100, 668, 248, 33, 5], [1536, 715, 170, 0, 0, 0], [0, 385, 498, 248, 33, 5])
    assert rows["mirror Refl 0"][2] == [1536, 918, 362, 66] and rows["mirror Refl 0"][5] == [0, 182, 306, 182, 33, 5]
    assert rows["pane Tr 0"][2] == [1536, 792, 248, 34] and rows["floor Refl 0"][2] == [1536, 385]
    assert rows["wall Refl 0.6, Tr 0.3, Tf"][2] == [1536, 1103] and rows["wall Refl 0.6, Tr 0.3, Tf"][4] == [0, 718]
    assert rows["mirror Refl 0.9"][2] == [1536, 1285, 537, 219]
    assert rows["back to A"][2:6] == ([1536, 715, 170], [1536, 182, 0], [0, 533, 170], [0, 1103, 537, 219])


def test_generator_conditions():
    """Over all committed seeds: every op kind at least 3 times; every predicted outcome at least twice; at least a third
    of the sync calls that return MT_OK (those with nothing to do counted) regrow the tree with rays traced AND rays
    dropped; at most a fifth of the ops leave the state as it is; layer 0 always hits a material; and no regrow traces
    rays while a moved light is pending on its tree (no mixed positions: that case is the scripted session's)."""
    kinds, outcomes = collections.Counter(), collections.Counter()
    ok = both = noops = ops = 0
    for seed in es.SEEDS:
        assert len(es.generate(seed)) == es.N_OPS
        for i, st, before, state, trees, log in replay("seed %#x" % seed):
            assert len(st["ops"]) == 1 and set(st["calls"]) == set(es.ALL_TREES)
            kinds[st["ops"][0][0]] += 1
            ops += 1
            noops += es.net_noop(before, state)
            assert (tree_of(state)["layers"][0]["material"] >= 0).any()
            for tree, call, p in log:
                outcomes[p["outcome"]] += 1
                assert None not in trees[tree].held, (seed, i, tree)
                if call in ("update_materials", "regrow") and p["outcome"] in ("ok", "ok_nothing_to_do"):
                    ok += 1
                    both += bool(p["regrown"] and sum(p["traced"]) and sum(p["dropped"]))
    print(dict(kinds), dict(outcomes), "MT_OK syncs %d, regrown both ways %d, no-ops %d of %d" % (ok, both, noops, ops))
    assert all(kinds[k] >= 3 for k in ("mat", "tex", "tex_move", "move_light", "colour_light")), kinds
    assert all(outcomes[o] >= 2 for o in es.OUTCOMES), outcomes
    assert 3 * both >= ok
    assert 5 * noops <= ops


def test_the_generator_is_deterministic():
    def plain(steps):
        return repr([(s["ops"], s["calls"]) for s in steps])
    assert plain(es.generate(es.SEEDS[0])) == plain(es.generate(es.SEEDS[0]))
    assert plain(es.generate(es.SEEDS[0])) != plain(es.generate(es.SEEDS[1]))


# ---- the newer edit kinds: reassignments and vertex attributes in the chain

NEW_SESSIONS = list(es.NEW_SCRIPTED) + ["seed %#x" % s for s in es.NEW_SEEDS]
# the floors a seed of the newer kinds must reach with the model alone, and what the committed seeds reach
# (test_new_seed_floors prints the counts; they were written here from its output)
FLOORS = dict(assign=4, normals=4, uvws=4, respawned=2, unsupported_no_tri=1, unsupported_textured_target=1,
              unsupported_attr_no_tri=1, unsupported_normals=1, aba_nothing=2, all_three_pending=1)
REACHED = {
    0xa5e5e2: dict(assign=7, normals=6, uvws=5, respawned=5, unsupported_no_tri=14, unsupported_textured_target=2,
                   unsupported_attr_no_tri=12, unsupported_normals=8, aba_nothing=9, all_three_pending=1),
    0xa5e60f: dict(assign=4, normals=5, uvws=4, respawned=5, unsupported_no_tri=7, unsupported_textured_target=2,
                   unsupported_attr_no_tri=21, unsupported_normals=6, aba_nothing=6, all_three_pending=1),
    0xa5e645: dict(assign=5, normals=4, uvws=6, respawned=5, unsupported_no_tri=29, unsupported_textured_target=11,
                   unsupported_attr_no_tri=8, unsupported_normals=1, aba_nothing=2, all_three_pending=1),
}


def new_script_of(name):
    if name in es.NEW_SCRIPTED:
        fn, trees = es.NEW_SCRIPTED[name]
        return fn(), trees
    return es.generate_new(int(name.split()[1], 16)), tuple(es.NEW_TREES)


def new_replay(name, steps=None):
    if steps is None:
        steps, names = new_script_of(name)
    else:
        names = es.NEW_SCRIPTED[name][1]
    state = es.start_state()
    trees = es.make_trees(state, names)
    for i, st in enumerate(steps):
        before = state
        for op in st["ops"]:
            state = es.apply(state, op)
        log = []
        es.run_step(trees, state, st, log)
        yield i, st, before, state, trees, log


def test_the_start_state_builds_the_tiny_scene_triangle_by_triangle():
    """build_scene adds every triangle with the state's normals, uvw and material: under start_state() the oracle's frame
    and tree are the tiny scene's own, and an edited state's scene holds the edit (the oracle hands the arrays back)."""
    a = es.start_state()
    want = te.build_tiny(orclib.OracleScene(), textures=te.tiny_textures())
    want.set_lights(a["lights"])
    assert np.array_equal(es.oracle_frame(a), want.render(es.CAM, es.W, es.H, max_level=es.DEPTH)["rgb"])
    assert tree_of(a)["n_rays"] == [1536, 715, 170]
    data, mtl, _ = es.oracle(a).triangles()
    data0, mtl0, _ = want.triangles()
    assert data.tobytes() == data0.tobytes() and np.array_equal(mtl, mtl0)
    b = es.apply(es.apply(es.apply(a, es.edit("assign", "floor->none")), es.edit("normals", "floor#2 zero")), es.edit("uvws", "nan swap"))
    data, mtl, _ = es.oracle(b).triangles()
    assert mtl.tolist() == b["tri_mtl"] and b["tri_mtl"][:2] == [-1, -1]
    assert data[:, 9:18].tobytes() == b["normals"].tobytes() and data[:, 18:27].tobytes() == b["uvws"].tobytes()


def test_the_generations_and_stamps_move_as_the_header_says():
    a = es.start_state()
    b = es.apply(a, es.edit("assign", "matte->mirror"))
    assert (b["gen"], b["asg_gen"], b["attr_gen"]) == (1, 1, [0, 0])
    assert es.apply(b, es.edit("assign", "matte->mirror")) ["gen"] == 1          # a set that changes nothing changes nothing
    c = es.apply(b, es.edit("normals", "matte tilt"))
    assert (c["gen"], c["attr_gen"]) == (2, [1, 0]) and c["stamp"][0].tolist() == [0] * 6 + [1, 1] + [0] * 4
    d = es.apply(c, es.edit("normals", "mirror tilt"))
    assert d["stamp"][0].tolist() == [0] * 4 + [2, 2, 1, 1] + [0] * 4            # only the changed triangles are stamped
    assert es.apply(d, es.edit("normals", "mirror tilt"))["gen"] == d["gen"]
    e = es.apply(d, es.original("normals", (4, 5, 6, 7)))
    assert e["attr_gen"] == [3, 0] and e["stamp"][0].tolist() == [0] * 4 + [3] * 4 + [0] * 4
    assert e["normals"].tobytes() == a["normals"].tobytes()
    # -0.0: bit-different, value-equal -- it is an edit
    f = es.apply(a, es.edit("normals", "matte#1 -0.0"))
    assert np.array_equal(f["normals"], a["normals"]) and f["attr_gen"] == [1, 0] and f["stamp"][0].tolist().count(1) == 1
    # the NaN texture coordinates of triangle 10 set again with the same bits: no edit
    g = es.apply(a, ("uvws", {10: a["uvws"][10].copy()}))
    assert g["gen"] == 0 and g["attr_gen"] == [0, 0]
    h = es.apply(a, es.edit("uvws", "nan swap"))
    assert h["stamp"][1].tolist() == [1] + [0] * 9 + [1, 0]


def test_every_new_op_changes_what_it_claims():
    """Per op of the three menus, against the start state, in the frame's fresh tree: a reassignment moves the ray
    counts or at least 20 rays' material; a normal edit at least 20 rays' normal plane, on exactly the rays of the edited
    triangles (the -0.0 edit: none needed, it is value-equal); a uvw edit the uvw plane on exactly vertex_attr_ref's
    pinned dirty counts.  Every op but the value-equal one and the untextured matte's uvw changes at least 20 pixels."""
    a = es.start_state()
    ta = tree_of(a)
    for kind, menu in es.MENUS.items():
        for name in menu:
            b = es.apply(a, es.edit(kind, name))
            tb = tree_of(b)
            changed = es.changed_rays(ta, tb)
            per = [int(va.dirty(lay["tri"], sorted(menu[name])).sum()) for lay in ta["layers"]]
            pixels = frame_pixels_changed(a, b)
            print(kind, name, changed, per, pixels)
            assert b["gen"] == 1
            if kind == "assign":
                assert changed.get("shape", 0) >= 20 or changed.get("material", 0) >= 20, (name, changed)
                assert pixels >= 20 and sum(per) >= 20
            elif kind == "normals":
                if name == "matte#1 -0.0":
                    assert "shape" not in changed and pixels == 0
                else:
                    assert "shape" in changed or changed.get("normal", 0) >= 20, (name, changed)
                    assert pixels >= 20 and sum(per) >= 20
            else:
                assert per == va.UVW_ROWS[name]["dirty"], (name, per)
                assert "shape" not in changed and set(changed) <= {"uvw", "albedo"}
                assert pixels == va.UVW_ROWS[name]["frame"]


def test_new_claims_and_pinned_literals():
    """Sessions a, b and c: the numbers of the frame's tree with tri and uvw are the literal ones (the steps' claims:
    test_new_steps_hold_their_claims; sessions d and e: test_sessions_d_and_e_pinned_literals)."""
    for (i, st, _, state, trees, log), row in zip(new_replay("stamp walk"), es.STAMP_WALK):
        mine = [(call, p) for tree, call, p in log if tree == "full_tu"]
        refusal, regrown, kept, traced, renormaled, reuvwed, respawned = row
        print("stamp walk", i, [(c, p["outcome"]) for c, p in mine])
        if refusal:
            assert mine[0][1]["outcome"] == "unsupported_normals" and (mine[0][1]["count"], mine[0][1]["first"]) == refusal
        p = mine[-1][1]
        assert p["outcome"] == ("ok_nothing_to_do" if st["claim"][0] == "nothing" else "ok")
        assert (p["regrown"], p["kept"], p["traced"]) == (regrown, kept, traced), (i, p)
        assert (p["renormaled"], p["reuvwed"], p["respawned"]) == (renormaled, reuvwed, respawned), (i, p)
        for tree, call, q in log:  # the trees without tri: refused at every step, the count grows with the stamps
            if not es.NEW_TREES[tree][2]:
                assert q["outcome"] == "unsupported_attr_no_tri" and q["attr"] == "normal", (i, tree, q)
                assert (q["count"], q["first"]) == ((2, es.stream_of()[6]) if i < 2 else (4, es.stream_of()[4]))
        if i == 1:
            after_uvw = {n: es.copy_tree(t.tree) for n, t in trees.items()}
    for n, t in trees.items():  # the mirror back: the tree of step 1, bit for bit
        if es.NEW_TREES[n][2]:
            assert not es.differing_planes(t.tree, after_uvw[n], t.keep_uvw, True), n
    # the mirror rays alone: 383 is the kept rays on triangles 4 and 5 -- the matte's 531, stamped in step 0, are older
    assert es.STAMP_WALK[2][4] == 383 and es.STAMP_WALK[0][4] == 531
    for (i, st, _, state, trees, log), row, tri_only in zip(new_replay("assignment walk"), es.ASSIGN_WALK, es.ASSIGN_WALK_TRI_ONLY):
        by = {tree: p for tree, _, p in log}
        p = by["full_tu"]
        print("assignment walk", i, {t: q["outcome"] for t, q in by.items()})
        assert (p["regrown"], p["n_rays"], p["kept"], p["traced"], p["dropped"], p["rays_shadow"]) == row, (i, p)
        q = by["full_t"]
        assert q["outcome"] == tri_only if isinstance(tri_only, str) else \
            (q["outcome"], q["triangle"], q["material"]) == ("unsupported_textured_target", es.stream_of()[tri_only[0]], tri_only[1])
        for tree in ("full_u", "full_0"):
            assert by[tree]["outcome"] == ("unsupported_no_tri" if i < 3 else "ok_nothing_to_do"), (i, tree)
        if i < 3:
            assert (by["full_0"]["count"], by["full_0"]["first"]) == ((2, 6), (4, 6), (4, 6))[i]
    for n, t in trees.items():  # back under the start state: the first tree
        assert not es.differing_planes(t.tree, es.Tree(n, es.start_state(), t.rays).tree, t.keep_uvw, t.keep_tri), n
    # c, the pile, and the same pile in the other order
    refusal, n_rays, kept, traced, dropped, renormaled, reuvwed = es.NEW_PILE_FULL
    finals = []
    for reverse in (False, True):
        for i, st, _, state, trees, log in new_replay("new pile", es.session_new_pile(reverse)):
            mine = [p for tree, _, p in log if tree == "full_tu"]
            assert (mine[0]["outcome"], mine[0]["count"], mine[0]["first"]) == ("unsupported_shape",) + refusal
            p = mine[1]
            assert (p["regrown"], p["n_rays"], p["kept"], p["traced"], p["dropped"]) == (1, n_rays, kept, traced, dropped), p
            assert (p["renormaled"], p["reuvwed"]) == (renormaled, reuvwed)
            d = p["plan"][0]
            assert d["changed"] == [6, 7] and d["texture_set"] is not None and len(d["dirty"][0]) and len(d["dirty"][1])
        finals.append((state, trees))
    assert es.same_look(finals[0][0], finals[1][0])
    for n in es.PILE_TREES:
        assert not es.differing_planes(finals[0][1][n].tree, finals[1][1][n].tree, True, True)


def test_new_steps_hold_their_claims():
    """Every step of the new scripted sessions that carries a claim, on the frame's and the chunk's tree with tri and uvw
    (es.hold_claim): grow / drop / both; an update refused before the regrow, for the shape or for the blocked
    normals; a same-shape attribute update that rewrites its plane alone; a respawn; nothing to do; a retexture with no
    shadow ray; all lights traced again; the old position kept and the new one caught up; no bit; the light count
    refusal that leaves the tree untouched and stale.  Every kind is seen, on the frame's tree."""
    seen = collections.Counter()
    for name, (fn, names) in es.NEW_SCRIPTED.items():
        state = es.start_state()
        trees = es.make_trees(state, names)
        for i, st in enumerate(fn()):
            before = {n: es.copy_tree(t.tree) for n, t in trees.items()}
            state = es.after(state, [st])
            log = []
            es.run_step(trees, state, st, log)
            if not st["claim"]:
                continue
            for n in st["calls"]:
                if n in es.CLAIM_TREES:
                    kind = es.hold_claim(st["claim"], [(c, p) for tree, c, p in log if tree == n], before[n], trees[n], state)
                    seen[kind] += n == "full_tu"
    print(dict(seen))
    assert all(seen[k] for k in ("regrow", "retexture", "nothing", "attr", "respawn", "all lights", "old position",
                                 "new position", "no bit", "light count")), seen
    assert all(st["claim"] for name in ("stamp walk", "assignment walk", "new pile", "new lights") for st in es.NEW_SCRIPTED[name][0]())


def test_sessions_d_and_e_pinned_literals():
    """The frame's tree with tri and uvw through the rhythms and the lights sessions: regrown, rays per layer, kept,
    traced, dropped, rays_shadow and the three attribute counts of every sync, as literal numbers."""
    for name, rows in (("new rhythms", es.RHYTHMS_FULL), ("new lights", es.NEW_LIGHTS_FULL)):
        steps = list(new_replay(name))
        assert len(steps) == len(rows)
        for (i, st, _, state, trees, log), row in zip(steps, rows):
            mine = [p for tree, call, p in log if tree == "full_tu" and call in ("update_materials", "regrow")]
            print(name, i, [p["outcome"] for p in mine], row)
            if row is None:
                assert all(p["outcome"] == "light_count" for p in mine) and len(mine) == (name == "new lights" and i == 4)
                continue
            p, = mine
            assert p["outcome"] == "ok", (name, i, p["outcome"])
            got = (p["regrown"], p["n_rays"], p["kept"], p["traced"], p["dropped"], p["rays_shadow"], tuple(p[k] for k in es.ATTR_COUNTS))
            assert got == row, (name, i, got, row)
            assert [k + t for k, t in zip(p["kept"], p["traced"])] == p["n_rays"]
    assert es.RHYTHMS_FULL[2][1] == [1536, 589, 89] and es.RHYTHMS_FULL[5][2:5] == ([1536, 407, 33], [0, 182, 56], [0, 182, 56])
    assert es.RHYTHMS_FULL[7][6] == (856, 0, 232) and es.NEW_LIGHTS_FULL[0][4:6] == ([0, 126, 81], 3906)
    assert es.NEW_LIGHTS_FULL[5][6] == (232, 0, 232)


def test_the_stream_order_is_the_facades():
    """es.STREAM_ORDER, pinned so that the model does not ask the product, is the numbering flatten() gives the tiny scene."""
    import mythtracer_amd as M
    tri_id = te.build_tiny(M.MythTracer()).flatten()["tri_id"]
    assert [int(a) for a in tri_id] == list(es.STREAM_ORDER) == list(range(es.N_TRIS))
    assert es.stream_of() == {int(a): k for k, a in enumerate(tri_id)}


@pytest.mark.parametrize("name", NEW_SESSIONS)
def test_new_sessions_hold_together(name):
    """Every sync of every new session and seed: kept + traced is the new tree's rays, the tree is fresh afterwards and
    is the truth of its synced state; a refusal leaves the tree and its snapshot alone; no mixed light positions."""
    syncs = refusals = 0
    for i, st, before, state, trees, log in new_replay(name):
        for tree, call, p in log:
            t = trees[tree]
            assert None not in t.held, (name, i, tree)
            if call not in ("update_materials", "regrow"):
                continue
            if p["outcome"] in ("ok", "ok_nothing_to_do"):
                assert not t.stale(state) and t.tree["n_rays"] == p["n_rays"]
                if p["outcome"] == "ok":
                    assert [k + r for k, r in zip(p["kept"], p["traced"])] == p["n_rays"], (name, i, tree, p)
                assert not es.differing_planes(t.tree, t.truth(), t.keep_uvw, t.keep_tri), (name, i, tree)
                syncs += 1
            else:
                assert p["outcome"].startswith("unsupported") or p["outcome"] == "light_count", (name, i, tree, p)
                refusals += 1
    print("%s: %d successful syncs, %d refusals" % (name, syncs, refusals))
    assert syncs > 0


def test_the_rhythms_session_counts_per_snapshot():
    """Session d: each tree's renormaled / reuvwed is the count for ITS snapshot -- the chunk's sync after op 5 takes the
    uvw set of op 3 and the normal set of op 5 at once, the frame's tree only op 5's --, and the trees without tri stay
    refused from the first attribute set on, also after the return to the original arrays."""
    seen = {}
    for i, st, _, state, trees, log in new_replay("new rhythms"):
        for tree, call, p in log:
            seen[(i, tree)] = p
    assert (seen[(5, "full_tu")]["renormaled"], seen[(5, "full_tu")]["reuvwed"]) == (232, 0)
    assert (seen[(5, "chunk_tu")]["renormaled"], seen[(5, "chunk_tu")]["reuvwed"]) == (156, 234)
    assert seen[(2, "chunk_tu")]["renormaled"] == 234 and seen[(8, "list_tu")]["renormaled"] == 21
    for i in range(1, 9):
        for tree in ("full_u", "full_0"):
            assert seen[(i, tree)]["outcome"].startswith("unsupported"), (i, tree)
    assert seen[(8, "full_u")]["outcome"] == "unsupported_attr_no_tri" and seen[(8, "full_u")]["count"] == 4
    assert seen[(1, "full_u")]["count"] == 2


def test_match_with_no_attribute_edit_is_regrow_refs_match():
    """vertex_attr_ref.match generalises regrow_ref.match: on the assignment walk and the shape walk, where no normal
    changed, the two give the same source index for every ray."""
    compared = 0
    states = [es.start_state()]
    for st in es.session_assignment_walk() + es.session_shape_walk():
        states.append(es.after(states[-1], [st]))
    for a, b in zip(states, states[1:]):
        ta, tb = tree_of(a), tree_of(b)
        m1, m2 = rg.match(ta, tb), va.match(ta["layers"], tb["layers"], [], [])
        assert all(np.array_equal(x, y) for x, y in zip(m1["src"], m2["src"]))
        assert (m1["kept"], m1["traced"]) == (m2["kept"], m2["traced"]) and m2["respawned"] == m2["renormaled"] == 0
        compared += sum(m1["traced"]) > 0
    assert compared >= 4


def floors_of(seed):
    got = collections.Counter()
    for i, st, before, state, trees, log in new_replay("seed %#x" % seed):
        got[st["ops"][0][0]] += 1
        for tree, call, p in log:
            if call not in ("update_materials", "regrow"):
                continue
            if p["outcome"] in es.NEW_OUTCOMES:
                got[p["outcome"]] += 1
            if p["outcome"] == "ok" and p["regrown"] and p["respawned"] > 0:
                got["respawned"] += 1
            d = p["plan"][0] if p.get("plan") else None
            if d is not None and p["outcome"] == "ok_nothing_to_do" and d["aba"]:
                got["aba_nothing"] += 1
            if d is not None and p["outcome"] == "ok" and d["changed"] and (len(d["dirty"][0]) or len(d["dirty"][1])) and d["texture_set"]:
                got["all_three_pending"] += 1
    return got


@pytest.mark.parametrize("seed", es.NEW_SEEDS, ids=hex)
def test_new_seed_floors(seed):
    """A seed cannot pass by never reaching the hard cases: FLOORS, per seed, with the model alone."""
    steps = es.generate_new(seed)
    assert len(steps) == es.NEW_N_OPS and all(len(st["ops"]) == 1 and set(st["calls"]) == set(es.NEW_TREES) for st in steps)
    got = floors_of(seed)
    print("seed %#x:" % seed, {k: got[k] for k in FLOORS})
    assert all(got[k] >= v for k, v in FLOORS.items()), {k: (got[k], v) for k, v in FLOORS.items() if got[k] < v}
    assert {k: got[k] for k in FLOORS} == REACHED[seed]
    new_kind = sum(got[k] for k in ("assign", "normals", "uvws"))
    assert es.NEW_N_OPS // 3 <= new_kind <= 2 * es.NEW_N_OPS // 3 + 2, new_kind  # about half


def test_the_new_generator_is_deterministic_and_leaves_the_old_one_alone():
    def plain(steps):
        return repr([(s["ops"], s["calls"]) for s in steps])
    assert len(es.NEW_SEEDS) == 3
    assert plain(es.generate_new(es.NEW_SEEDS[0])) == plain(es.generate_new(es.NEW_SEEDS[0]))
    assert plain(es.generate_new(es.NEW_SEEDS[0])) != plain(es.generate_new(es.NEW_SEEDS[1]))
    # the old seeds' streams did not move: the digests of their steps, taken from the model as it was before the newer
    # kinds went in
    for seed, digest in zip(es.SEEDS, ("bce7f58620326ff359769bd889dfb969a60362c9", "d94394cde6e190071bb290fef50d6adf006237c5",
                                       "2ae6827972de6a63a9b3934a53f42b3c218d2bcc")):
        steps = es.generate(seed)
        assert all(op[0] in ("mat", "tex", "tex_move", "move_light", "colour_light") for st in steps for op in st["ops"])
        assert hashlib.sha1(plain(steps).encode()).hexdigest() == digest, hex(seed)
