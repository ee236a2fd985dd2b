"""The hostile scene family (tests/hostile_scenes.py) on the CPU: material tables, normals and lights at which the
comparisons of TraceRayWorker (mythtracer.cc:13-228) are decided by the unusual value.

a. The ORACLE against the compiled reference's own frames (tests/golden/hostile_<case>.npz, made by
   tests/golden/make_hostile_golden.py): rgb byte for byte, line_no exactly, point bit for bit, in both groups -- both
   sides call glibc's pow.  depth_16 has no reference frame (the reference's depth is a compile-time 5).
b. The numpy RESTATEMENTS against the oracle, on every case, identity: raytree_ref (rays per layer as the oracle counts
   them, the composite frame), lightbuffer_ref (the shadow loops and the direct frame at depth 0), raylist_ref (the
   layered tree over the sensor's rays plane for plane against raytree_ref's, its linear colours through V3DtoRGB
   against the frame, and the recursive trace_ray against the layered colours bit for bit).
c. material_edit_ref.check_pass's prediction for base -> case (same shape, or refused at a first ray) against two
   restated trees.
d. The Ni cases render the base frame.
e. Every case still bites: its own counter is at least half of what the maker recorded in hostile.json.

DESIGN.md section 4 lists which one-token change of oracle/mt_oracle.c which of these cases notices.
"""
import os

import numpy as np
import pytest

import gbuffer_ref
import hostile_scenes as hs
import lightbuffer_ref as lr
import material_edit_ref as me
import raylist_ref as rl
import raytree_ref as rr

NAMES = list(hs.CASES)
PINNED = [n for n in NAMES if hs.CASES[n]["reference"]]
TABLE_ONLY = [n for n in NAMES if hs.CASES[n]["normals"] == "unit" and hs.CASES[n]["depth"] == hs.DEPTH and hs.CASES[n]["edit"]]


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    return hs.Family(str(tmp_path_factory.mktemp("hostile")))


def differing(a, b, what):
    n = int((np.asarray(a) != np.asarray(b)).sum())
    print("%s: %d of %d differ" % (what, n, np.asarray(a).size))
    return n


def test_the_pin_lists_every_case():
    pin = hs.pinned()
    assert sorted(pin["cases"]) == sorted(NAMES)
    assert pin["image"] == [hs.W, hs.H]
    unplanned = [n for n in pin["dropped"] if hs.CASES[n]["reference"]]
    assert len(unplanned) <= 2 and all(pin["dropped"][n] for n in pin["dropped"])
    for name, entry in pin["cases"].items():
        c = hs.CASES[name]
        assert (entry["group"], entry["counter"], entry["normals"]) == (c["group"], c["counter"], c["normals"]), name
        assert entry["count"] >= 20, name
        assert os.path.exists(hs.golden_path(name)) == (name not in pin["dropped"]), name
        # the pow group is exactly the cases that edit Ns; every other table keeps Ns 0 on every material
        assert (c["group"] == "pow") == any("Ns" in f for f in c["edit"].values()), name
        assert c["group"] == "pow" or (hs.table(c["edit"])[:, 9] == 0.0).all(), name
        assert np.isfinite(hs.table(c["edit"])).all() and np.isfinite(np.array(c["lights"])).all(), name
    size = sum(os.path.getsize(hs.golden_path(n)) for n in NAMES if n not in pin["dropped"])
    assert size < 1024 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_the_oracle_reads_the_table_the_case_states(name, family):
    c = family(name)
    mats = c["orc"].materials()
    assert [m[0] for m in mats] == list(hs.BASE)
    got = np.array([m[1] for m in mats])
    assert differing(got.view(np.uint64), hs.table(c["edit"]).view(np.uint64), name + " table bits") == 0  # (-0.0 too)
    assert all(m[2] < 0 for m in mats)
    assert (c["orc"].triangles()[1] >= 0).all()  # no occluder without a material


@pytest.mark.parametrize("name", PINNED)
def test_oracle_against_the_references_frame(name, family):
    c = family(name)
    if name in hs.pinned()["dropped"]:
        pytest.fail("%s was dropped from the reference pin: %s" % (name, hs.pinned()["dropped"][name]))
    g = hs.load_golden(name)
    assert np.array_equal(g["cam"], np.array(c["camera"])) and np.array_equal(g["lights"], np.array(c["lights"]))
    assert int(g["depth"]) == c["depth"] == 5 and tuple(g["image"]) == (hs.W, hs.H)
    want = c["want"]
    assert differing(want["rgb"], g["rgb"], name + " rgb bytes") == 0
    assert differing(want["line"], g["line"], name + " line_no") == 0
    assert gbuffer_ref.same_bits(want["point"], g["point"], name + " point") == 0


@pytest.mark.parametrize("name", NAMES)
def test_raytree_ref_against_the_oracle(name, family):
    c = family(name)
    tree, want = c["tree"], c["want"]
    print(name, "rays per layer", tree["n_rays"])
    for k in ("rays_primary", "rays_secondary", "rays_shadow", "shaded_hits"):
        assert tree[k] == want["counters"][k], (k, tree[k], want["counters"][k])
    got = rr.shade(c["orc"], tree, c["lights"], hs.W, hs.H)
    assert differing(got, want["rgb"], name + " composite frame bytes") == 0
    assert tree["n_rays"] == hs.pinned()["cases"][name]["rays_per_layer"]


@pytest.mark.parametrize("name", NAMES)
def test_lightbuffer_ref_against_the_oracle(name, family):
    c = family(name)
    orc = c["orc"]
    gb = gbuffer_ref.oracle_gbuffer(orc, c["camera"], hs.W, hs.H)
    lb = lr.ref_lightbuffer(orc, gb, c["lights"])
    direct = orc.render(c["camera"], hs.W, hs.H, max_level=0, debug=True)
    assert lb["rays_shadow"] == direct["counters"]["rays_shadow"]
    assert differing(lr.shade(orc, gb, lb, c["lights"]), direct["rgb"], name + " direct frame bytes") == 0
    assert differing(gb["line_no"], direct["line"], name + " line_no") == 0
    assert gbuffer_ref.same_bits(gb["point"], direct["point"], name + " point") == 0
    # the planes are the tree's layer 0 (tiling order), bit for bit
    lay = c["tree"]["layers"][0]
    n = hs.W * hs.H
    assert gbuffer_ref.same_bits(lb["power"].reshape(-1, n, 3)[:, lay["pixel"]], lay["power"], name + " power") == 0
    assert np.array_equal(lb["in_shadow"].reshape(-1, n)[:, lay["pixel"]], lay["in_shadow"])


@pytest.mark.parametrize("name", NAMES)
def test_raylist_ref_against_the_oracle(name, family):
    c = family(name)
    orc, want = c["orc"], c["want"]
    rays = gbuffer_ref.pixel_rays(c["camera"], hs.W, hs.H).reshape(-1, 6)
    tree = rl.build_from_rays(orc, rays, hs.W, hs.H, c["lights"], c["depth"])
    assert tree["n_rays"] == c["tree"]["n_rays"]
    for a, b in zip(tree["layers"], c["tree"]["layers"]):
        for plane in rr.F64_PLANES:
            assert gbuffer_ref.same_bits(a[plane], b[plane], "%s %s" % (name, plane)) == 0
        for plane in rr.INT_PLANES:
            assert np.array_equal(a[plane], b[plane]), plane
    colors = rl.colors(orc, tree, c["lights"])
    assert differing(rr.v3d_to_rgb(colors).reshape(hs.H, hs.W, 3), want["rgb"], name + " linear colours, quantised") == 0
    pick = np.arange(5, len(rays), 13)  # the recursive restatement is slow: every 13th ray
    alone = rl.trace_rays(orc, rays[pick], c["lights"], c["depth"])
    assert gbuffer_ref.same_bits(alone, colors[pick], name + " trace_ray against the layered colours") == 0


@pytest.mark.parametrize("name", TABLE_ONLY)
def test_material_edit_prediction(name, family):
    """base -> case with base's lights and camera: check_pass walks base's tree with the case's table."""
    base, c = family("base"), family(name)
    tree_b = c["tree"] if c["lights"] == base["lights"] else rr.build(c["orc"], base["camera"], hs.W, hs.H,
                                                                      base["lights"], hs.DEPTH)
    predicted = me.check_pass(base["tree"], c["orc"].materials())
    seen = hs.first_difference(base["tree"], tree_b)
    print("%s: predicted %s (%d rays), two trees say %s" % (name, predicted["first"], predicted["count"], seen))
    assert predicted["first"] == seen
    assert (predicted["count"] == 0) == me.same_shape(base["tree"], tree_b)
    if seen is None:  # same shape: the predicted coefficients are the fresh tree's
        for k, lay in enumerate(tree_b["layers"]):
            assert gbuffer_ref.same_bits(predicted["coef"][k], lay["coef"], "%s coef of layer %d" % (name, k)) == 0


def test_the_edits_cover_both_outcomes(family):
    base = family("base")
    kinds = {n: me.check_pass(base["tree"], family(n)["orc"].materials())["count"] == 0 for n in TABLE_ONLY}
    print(kinds)
    assert sum(kinds.values()) >= 5 and sum(not v for v in kinds.values()) >= 5


@pytest.mark.parametrize("name", hs.NI_CASES)
def test_ni_cases_are_the_base_frame(name, family):
    base, c = family("base")["want"], family(name)["want"]
    assert differing(c["rgb"], base["rgb"], name + " rgb against base") == 0
    assert c["counters"] == base["counters"]
    assert np.array_equal(hs.load_golden(name)["rgb"], hs.load_golden("base")["rgb"])


@pytest.mark.parametrize("name", NAMES)
def test_every_case_bites(name, family):
    c = family(name)
    entry = hs.pinned()["cases"][name]
    count = hs.bite(c["orc"], c["tree"], c["lights"])[c["counter"]]
    print("%s: %s = %d (recorded %d)" % (name, c["counter"], count, entry["count"]))
    assert count >= max(20, entry["count"] // 2)
