"""mt_raytree_regrow_materials, the parts that need no GPU (include/mythtracer_hip.h).

a. The symbols exist, the ABI version is still 5, a NULL tree is refused before any device call, and the facade refuses
   before it needs a device.
b. What a regrow keeps, traces and drops, by the oracle alone (tests/regrow_ref.py over tests/raytree_ref.py) on
   two_way.obj at 96x54, the bench's lights, depth 5, whole frame and off-grid chunk: for the five edits of
   regrow_ref.EDITS, in both directions, the numbers this file's tables record -- the reverse of an edit swaps traced and
   dropped.  The traced lists cross the 64- and 128-ray work-item boundaries, and "matte" leaves layer 0 alone.
c. The restated regrow -- kept rays copied from tree A by src, with B's coef, the new ambient where it changed and, for a
   shadow-relevant edit, B's light planes; traced rays from the restatement -- IS tree B in every plane of every layer:
   what the call takes over from the old tree depends on no material.
"""
import ctypes
import os

import numpy as np
import pytest

import material_edit_ref as me
import orclib
import raytree_ref as rr
import raytree_update_ref as ru
import regrow_ref as rg
from conftest import ROOT

import mythtracer_amd as M
from mythtracer_amd import binding

MT_ERR_ARG, MT_ERR_HIP = -1, -2
W, H = me.W, me.H
CAM = rr.CAMERAS["two_way"]


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    return native_libs


# ---- a. symbols, argument checks, facade

def test_symbols_and_abi_version():
    abi = M.hip_abi()
    assert binding.MT_ABI_VERSION == 5 == abi.lib.mt_abi_version()
    assert "mt_raytree_regrow_materials" in M.HIP_SYMBOLS and abi.lib.mt_raytree_regrow_materials is not None
    assert M.host_lib().mth_raytree_regrow is not None
    assert callable(abi.raytree_regrow) and callable(binding.RayTree.regrow)
    # the struct is the header's: three int32, padding, three arrays of MT_MAX_RECURSION + 1 int64
    assert ctypes.sizeof(binding.mt_raytree_regrow_info) == 16 + 3 * 8 * (binding.MT_MAX_RECURSION + 1)
    header = open(os.path.join(ROOT, "include", "mythtracer_hip.h")).read()
    assert "mt_raytree_regrow_info" in header and "#define MT_ABI_VERSION 5" in header


def test_a_null_tree_is_refused_before_any_device_call():
    abi = M.hip_abi()
    st = binding.mt_stats()
    info = binding.mt_raytree_regrow_info()
    for i in (None, ctypes.addressof(info)):
        for stats in (None, ctypes.addressof(st)):
            rc = abi.lib.mt_raytree_regrow_materials(None, i, stats)
            assert rc == MT_ERR_ARG and rc != MT_ERR_HIP, (rc, abi.last_error())
            assert abi.last_error() == "the ray tree is NULL"
    with pytest.raises(RuntimeError, match="ray tree is NULL"):
        abi.raytree_regrow(None)


def test_facade_refuses_before_it_needs_a_device():
    m = M.MythTracer()
    m.set_devices([0, 0])
    assert not m.L.mth_raytree_regrow(m.h, None, None, None)
    assert "several devices" in m.last_error()
    m2 = M.MythTracer(rr.TWO_WAY)
    assert not m2.L.mth_raytree_regrow(m2.h, None, None, None)
    assert "RayTree is NULL" in m2.last_error()
    closed = binding.RayTree(m2, None, {}, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="closed"):
        closed.regrow()


# ---- b. and c. the restated regrow

@pytest.fixture(scope="module")
def base():
    orc = orclib.OracleScene(rr.TWO_WAY)
    return orc, {chunk: rr.build(orc, CAM, W, H, me.LIGHTS, 5, chunk=chunk) for chunk in me.CHUNKS}


@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    made = {}

    def get(name, chunk):
        if name not in made:
            d = tmp_path_factory.mktemp("variant")
            made[name] = [orclib.OracleScene(me.variant(rr.TWO_WAY, rg.EDITS[name], str(d))), {}]
        orc, trees = made[name]
        if chunk not in trees:
            trees[chunk] = rr.build(orc, CAM, W, H, me.LIGHTS, 5, chunk=chunk)
        return orc, trees[chunk]
    return get


def test_the_variants_hold_the_edits_numbers_and_nothing_else(base, variants):
    orc, trees = base
    assert trees[None]["n_rays"] == me.TREE_A and trees[me.OFF_GRID]["n_rays"] == rg.CHUNK_A
    for name, edit in rg.EDITS.items():
        orc_b, _ = variants(name, None)
        me.check_variant(orc.materials(), orc_b.materials(), edit)
        assert rg.shadow_relevant(orc.materials(), orc_b.materials()) == (name in rg.SHADOW_EDITS), name


@pytest.mark.parametrize("chunk", me.CHUNKS, ids=["frame", "chunk"])
@pytest.mark.parametrize("name", list(rg.EDITS))
def test_what_a_regrow_keeps_traces_and_drops(name, chunk, base, variants):
    orc_a, trees = base
    a = trees[chunk]
    orc_b, b = variants(name, chunk)
    shadow = name in rg.SHADOW_EDITS
    want_rays, want_traced, want_dropped = rg.table(chunk)[name]
    fwd = rg.match(a, b, shadow)
    back = rg.match(b, a, shadow)
    print("%s %s: B %s kept %s traced %s dropped %s; secondary %d hits %d shadow %d; back: secondary %d hits %d shadow %d"
          % (name, "chunk" if chunk else "frame", b["n_rays"], fwd["kept"], fwd["traced"], fwd["dropped"],
             fwd["rays_secondary"], fwd["shaded_hits"], fwd["rays_shadow"], back["rays_secondary"], back["shaded_hits"],
             back["rays_shadow"]))
    assert b["n_rays"] == want_rays
    assert fwd["traced"] == want_traced and fwd["dropped"] == want_dropped
    assert [k + t for k, t in zip(fwd["kept"], fwd["traced"])] == b["n_rays"]
    # the reverse swaps traced and dropped (per layer of the longer tree, zero beyond the shorter one's end)
    pad = lambda v, n: list(v) + [0] * (n - len(v))  # noqa: E731
    n = max(len(a["n_rays"]), len(b["n_rays"]))
    assert pad(back["traced"], n) == pad(fwd["dropped"], n) and pad(back["dropped"], n) == pad(fwd["traced"], n)
    assert [k + t for k, t in zip(back["kept"], back["traced"])] == a["n_rays"]
    assert pad(back["kept"], n) == pad(fwd["kept"], n)
    assert fwd["src"][0].tolist() == list(range(a["n_rays"][0]))
    # the shape changes: the check pass of mt_raytree_update_materials finds mismatches, in both directions
    assert me.check_pass(a, orc_b.materials())["count"] > 0 and me.check_pass(b, orc_a.materials())["count"] > 0
    assert fwd["rays_secondary"] == sum(want_traced) and back["rays_secondary"] == sum(want_dropped)
    assert fwd["rays_shadow"] >= (b["rays_shadow"] if shadow else 0)


def test_the_traced_lists_cross_the_item_boundaries(base, variants):
    """A work item of the tracing launch is 64 consecutive traced rays: lists below 64, between 64 and 128 and above 128."""
    _, trees = base
    sizes = set()
    for chunk in me.CHUNKS:
        for name in rg.EDITS:
            _, b = variants(name, chunk)
            for m in (rg.match(trees[chunk], b), rg.match(b, trees[chunk])):
                sizes.update(m["traced"])
    sizes.discard(0)
    print(sorted(sizes))
    assert any(s < 64 for s in sizes) and any(64 < s < 128 for s in sizes) and any(s > 128 for s in sizes)


@pytest.mark.parametrize("chunk", me.CHUNKS, ids=["frame", "chunk"])
@pytest.mark.parametrize("name", list(rg.EDITS))
def test_the_restated_regrow_is_the_tree_built_with_the_new_materials(name, chunk, base, variants):
    orc_a, trees = base
    orc_b, tree_b = variants(name, chunk)
    shadow = name in rg.SHADOW_EDITS
    for what, a, b, ma, mb in (("A -> B", trees[chunk], tree_b, orc_a.materials(), orc_b.materials()),
                               ("B -> A", tree_b, trees[chunk], orc_b.materials(), orc_a.materials())):
        m = rg.match(a, b, shadow)
        got = rg.regrow(a, b, m["src"], ma, mb, shadow)
        assert len(got) == len(b["layers"])
        bad = []
        for k, (g, lay) in enumerate(zip(got, b["layers"])):
            for plane in me.PLANES + ("prim",):
                if not ru.same_plane(g[plane], lay[plane]):
                    bad.append((k, plane))
        assert np.array_equal(got[0]["pixel"], b["layers"][0]["pixel"])
        print("%s %s %s: %d planes differ %s" % (name, "chunk" if chunk else "frame", what, len(bad), bad))
        assert not bad
        if not shadow:
            continue
        # a shadow-relevant edit does change light planes of kept rays: without the re-trace the tree would be wrong
        stale = rg.regrow(a, b, m["src"], ma, mb, False)
        assert any(not ru.same_plane(g["power"], lay["power"]) for g, lay in zip(stale, b["layers"])), (name, what)
