"""tests/list_lengths.py against the oracle and the host builder alone (no GPU): the planted lists are what they claim to
be, every aimed ray's answer is its own triangle, and the lengths sit on the boundaries DESIGN 3.1.2 names.  These are
conditions of the GPU tests, not floors: the share of aimed rays that return their triangle is 100 %."""
import numpy as np
import pytest

import list_lengths as ll

import mythtracer_amd as M


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    """The host builder lives in the native library: built (if stale) before the first test of this file."""


IDS = ["%d-%d%s" % (l, l2, "-tie" if tie else "") for l, l2, tie in ll.CASES]


def test_the_cases_cover_the_table():
    roots = {l for l, _, _ in ll.CASES}
    children = {l2 for _, l2, _ in ll.CASES}
    for n in ll.SHORT + ll.LONG + ll.DESCENT_ROOT:
        assert n in roots and n in children, n
    have = {(l, l2) for l, l2, _ in ll.CASES}
    for pair in ll.DESCENT_CHILD + ll.SECOND_LONG + ll.FRAMES + ((0, 33), (33, 0)):
        assert pair in have, pair
    assert max(l + l2 for l, l2, _ in ll.CASES) <= 3700


def test_the_lengths_sit_on_the_boundaries():
    """n_sup = (n + 63) >> 6, nb = the 16-blocks of the stream that [pb, pb + pc) touches, pb % 16: restated in
    list_lengths.py, and here what the table says they are at its lengths."""
    # short lists: whole and partial quads, the mask's two arms, the switch to the sorted copy
    assert [(n + 3) >> 2 for n in ll.SHORT] == [1, 1, 1, 2, 4, 4, 5, 7, 8, 8, 8]
    assert max(ll.SHORT) == ll.K_SHORT and min(ll.LONG) == ll.K_SHORT + 1
    # long lists: supers
    assert [ll.n_sup(n) for n in ll.LONG] == [1, 1, 2, 2, 3, 3, 4, 4, 5, 6, 7, 7, 8, 28, 29, 29, 30, 57]
    assert ll.n_sup(128) == ll.K_DIRECT and ll.n_sup(129) == ll.K_DIRECT + 1        # direct -> super level
    assert (ll.n_sup(256) + 3) >> 2 == 1 and (ll.n_sup(257) + 3) >> 2 == 2          # one super quad -> two
    assert 256 == ll.K_PAD                                                          # the pad boundary
    assert ll.n_sup(384) == 6 and ll.n_sup(385) == 7                                # the gather of six
    assert ll.n_sup(449) == 8 and 449 - 7 * 64 == 1                                 # an 8th super of one entry
    assert ll.n_sup(1792) == ll.K_ROUND and ll.n_sup(1793) == ll.K_ROUND + 1 and 1793 - 28 * 64 == 1
    assert ll.n_sup(1857) - ll.K_ROUND == 2 and ll.n_sup(3585) == 2 * ll.K_ROUND + 1  # a third round, of one entry
    # the descent: root lists begin at stream position 0
    assert [n >= ll.K_BIG for n in ll.DESCENT_ROOT] == [False, True, True, True, True]
    assert ll.n_blocks(0, 1024) == 64 and ll.n_blocks(0, 1025) == 65
    # child 0's list begins at pb = L
    got = [(pb % 16, ll.n_blocks(pb, pc), pc >= ll.K_BIG) for pb, pc in ll.DESCENT_CHILD]
    assert got == [(15, 11, True), (15, 12, True), (0, 11, True), (0, 12, True), (1, 2, False), (1, 3, True),
                   (1, 3, True)]
    assert ll.K_SUPER_MIN == 12
    for pb, pc in ll.DESCENT_CHILD[:2] + ll.DESCENT_CHILD[5:]:  # clipped first block; clipped last block where it ends inside one
        assert pb // 16 * 16 < pb
    assert [(pb + pc) % 16 for pb, pc in ll.DESCENT_CHILD] == [0, 1, 0, 1, 0, 1, 0]
    # the second long list of a scene begins at a multiple of the pad that is not zero
    assert [ll.ll_begins(p) for p in ll.SECOND_LONG] == [[0, 512], [0, 2048], [0, 256]]


@pytest.mark.parametrize("l,l2,tie", ll.CASES, ids=IDS)
def test_the_lists_are_as_planted(l, l2, tie):
    c = ll.case(l, l2, tie)
    t = c["tree"]
    m = M.MythTracer()
    for k, v in enumerate(c["tris"]):
        m.add_triangle(v, None, mtl=-1, line_no=k)
    tm = m.tree()
    assert tm["depth"] == t["depth"]
    for k in ("aabb", "first_child", "prim_begin", "prim_count", "prim_ids"):
        assert np.array_equal(tm[k], t[k]), k
    assert np.array_equal(t["aabb"][0], [0, 0, 0, 128, 128, 128])
    assert t["first_child"][0] == 1                      # child 0 is node 1
    assert np.array_equal(t["aabb"][1], [0, 0, 0, 64, 64, 64])
    assert t["prim_count"][0] == l and t["prim_begin"][0] == 0
    assert t["prim_count"][1] == l2 and t["prim_begin"][1] == l
    assert np.array_equal(t["prim_ids"][:l + l2], np.arange(l + l2))  # the list order is the add order
    assert t["prim_count"][2:].max() < 16                # no other list of any length
    assert (t["first_child"][1] != 0) == (l2 >= 16)


@pytest.mark.parametrize("l,l2,tie", ll.CASES, ids=IDS)
def test_every_aimed_ray_returns_its_own_triangle(l, l2, tie):
    c = ll.case(l, l2, tie)
    n = len(c["rays"])
    assert n % 64 == 0 and n < 30000 and np.isfinite(c["rays"]).all()
    aimed = c["node"] >= 0
    wrong = np.nonzero(c["want"]["line"] != c["own"])[0]
    assert len(wrong) == 0, ll.describe(c, int(wrong[0]))
    assert (c["want"]["line"][~aimed] == -1).all()       # every padding ray misses
    if tie:
        first = aimed & (c["pos"] == 0)
        assert first.any() and (c["own"][first] != c["pos"][first] + np.where(c["node"][first] == 1, l, 0)).all()
    for node, length in ((0, l), (1, l2)):
        mine = c["node"] == node
        assert mine.any() == (length > 0)
        if length == 0:
            continue
        for kind in range(3):  # O1 aims every kind at every position; O2 too, but for one lane a wave where it has to
            assert set(c["pos"][mine & (c["kind"] == kind) & (c["order"] == 0)]) == set(range(length))  # reach the last run
            assert len(set(c["pos"][mine & (c["kind"] == kind) & (c["order"] == 1)])) >= length - (length + 63) // 64
        # the kinds are what they say
        zeros = (c["rays"][mine, 3:] == 0.0).sum(axis=1)
        assert np.array_equal(zeros, np.array([0, 2, 1])[c["kind"][mine]])
        # O2: a wave's 64 targets fall into at least min(n_sup, 7) different runs of 64 list positions
        o2 = np.nonzero(mine & (c["order"] == 1))[0]
        assert len(o2) % 64 == 0 and (o2 % 64 == np.arange(len(o2)) % 64).all()
        for w in o2.reshape(-1, 64):
            assert len(set(c["pos"][w] // 64)) >= min(ll.n_sup(length), 7)
            blocks = set(c["pos"][w] // 16)
            if length == 1024:  # the descent: all 64 blocks of the chunk are live, one run up to bit 63
                assert blocks == set(range(64))
            if length == 1025:  # ... and the 65th block, a second chunk, in every wave
                assert 64 in blocks and len(blocks) >= 60
        if length == 1025:
            assert any({62, 63} <= set(c["pos"][w] // 16) for w in o2.reshape(-1, 64))
        # O3: one lane of the wave is aimed, the first two and last two positions are among them, no lane twice
        o3 = np.nonzero(mine & (c["order"] == 2))[0]
        lanes = o3 % 64
        assert len(set(lanes)) == len(lanes) == min(length, 20)
        assert {0, 1, length - 2, length - 1} & set(range(length)) <= set(c["pos"][o3])
        for r in o3:
            wave = slice(r // 64 * 64, r // 64 * 64 + 64)
            assert (c["node"][wave] >= 0).sum() == 1 and (c["order"][wave] == 2).all()
        # O4: 1, 3, 8 and 9 irregular lanes among regular ones
        o4 = np.nonzero(mine & (c["order"] == 3))[0].reshape(-1, 64)
        assert [(c["kind"][w] != 0).sum() for w in o4] == [1, 3, 8, 9]


@pytest.mark.parametrize("l,l2,levels", ll.DEEP)
def test_the_deep_variants_are_that_deep(l, l2, levels):
    c = ll.case(l, l2, False, levels)
    t = c["tree"]
    assert t["depth"] == levels
    assert (t["prim_count"][0], t["prim_count"][1], t["prim_begin"][1]) == (l, l2, l)
    assert np.array_equal(c["want"]["line"], c["own"])
