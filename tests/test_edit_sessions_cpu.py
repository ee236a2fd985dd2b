"""The edit sessions of tests/edit_session_ref.py pinned with the oracle alone (no GPU): the model's `chained` tree
equals a fresh raytree_ref.build at every sync of every scripted session and every seed; every op of the scripted
sessions changes what it claims to change; session 1's shapes are the literal numbers of its table; the seeded
generator meets its conditions.  tests/test_gpu_edit_sessions.py holds the kernels to the same model.
"""
import collections

import numpy as np
import pytest

import edit_session_ref as es
import material_edit_ref as me
import orclib
import texture_edit_ref as te

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
