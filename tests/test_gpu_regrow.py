"""mt_raytree_regrow_materials on a real MI355X (-m gpu): a stored ray tree brought to edited materials that change its
SHAPE (include/mythtracer_hip.h; the kernels are mt::raytree_regrow_*_kernel in mythtracer_amd/csrc/mt_raytree.h).

The bar is identity, no tolerance.  The truth for materials B always comes from a scene BUILT with B
(material_edit_ref.variant), never from the edit call: a tree made under A and regrown is held plane by plane and layer
by layer to a fresh mt_raytree_create on the variant's scene and to the restatement of tests/raytree_ref.py (doubles as
uint64 views with NaN = NaN, bytes and indices equal, every ray), its mt_raytree_info to the fresh tree's, and what the
call reports -- kept, traced, dropped, the work counters -- to tests/regrow_ref.py, whose numbers
tests/test_regrow_cpu.py pins with the oracle alone.  Every test prints its counts.
"""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import lightupdate_ref as lu  # noqa: E402
import material_edit_ref as me  # noqa: E402
import orclib  # noqa: E402
import raylist_ref as rl  # noqa: E402
import raytree_ref as rr  # noqa: E402
import raytree_update_ref as ru  # noqa: E402
import regrow_ref as rg  # noqa: E402
from gbuffer_ref import same_bits  # noqa: E402

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding, scenegen  # noqa: E402

W, H = me.W, me.H
OFF_GRID = me.OFF_GRID
LIGHTS = me.LIGHTS
CAM = rr.CAMERAS["two_way"]
NINE = [(40.0 * i, 150.0 + 10 * i, 380.0 - 40 * i, 0.02, 0.01 * i, 0.03, 0.2, 0.15, 0.1 + 0.02 * i, 0.1, 0.2, 0.1)
        for i in range(9)]
MT_ERR_ARG, MT_ERR_UNSUPPORTED = -1, -3
STALE = "materials were edited after the ray tree was made"
INFO_KEYS = ("n_rays", "n_layers", "bytes", "n_lights", "chunk", "max_depth")


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"


class Scene:
    def __init__(self, obj=None, flat=None):
        self.abi = M.hip_abi()
        self.flat = flat if flat is not None else M.MythTracer(obj).flatten()
        self.h = self.abi.scene_create(self.flat)
        self.trees = []

    def close(self):
        for t in self.trees:
            self.abi.raytree_destroy(t)
        self.abi.scene_destroy(self.h)

    @property
    def materials(self):
        return self.flat["materials"]

    def set_lights(self, lights):
        self.abi.set_lights(self.h, lights)

    def set_materials(self, mats):
        self.abi.set_materials(self.h, mats)

    def tree(self, cam, w, h, chunk=None, depth=5):
        t, stats = self.abi.raytree_create(self.h, binding.sensor(cam, w, h), w, h, chunk=chunk, max_depth=depth)
        self.trees.append(t)
        return t, stats

    def tree_rays(self, rays, list_w, depth=5):
        t, stats = self.abi.raytree_create_rays(self.h, rays, list_w=list_w, max_depth=depth)
        self.trees.append(t)
        return t, stats

    def destroy(self, t):
        self.trees.remove(t)
        self.abi.raytree_destroy(t)

    def frame(self, cam, w, h, chunk=None, depth=5):
        return self.abi.render_chunk(self.h, binding.sensor(cam, w, h), w, h, chunk=chunk, max_depth=depth)

    def planes(self, t):
        """Every plane of every layer of a tree, read back."""
        return [self.abi.raytree_read_layer(t, k) for k in range(self.abi.raytree_info(t)["n_layers"])]


@pytest.fixture
def make(scenes):
    made = []

    def _make(name=None, obj=None, flat=None):
        made.append(Scene(obj if obj is not None else (me.obj_of(scenes, name) if name else None), flat))
        return made[-1]
    yield _make
    for s in made:
        s.close()


@pytest.fixture(scope="module")
def variant_of(scenes, tmp_path_factory):
    """(scene name, name in regrow_ref.EDITS / material_edit_ref.EDITS or an edit) -> the variant's .obj, written once."""
    made = {}
    named = dict(me.EDITS, **rg.EDITS)

    def get(scene, edit):
        key = (scene, edit if isinstance(edit, str) else repr(edit))
        if key not in made:
            d = tmp_path_factory.mktemp("variant")
            made[key] = me.variant(me.obj_of(scenes, scene), named[edit] if isinstance(edit, str) else edit, str(d))
        return made[key]
    return get


@pytest.fixture(scope="module")
def restated(variant_of):
    """(edit name or None for the scene as it is, chunk) -> (oracle scene, restated tree of two_way at depth 5), once."""
    orcs, trees = {}, {}

    def get(name, chunk):
        if name not in orcs:
            orcs[name] = orclib.OracleScene(variant_of("two_way", name) if name else rr.TWO_WAY)
            orcs[name].set_lights(LIGHTS)
        if (name, chunk) not in trees:
            trees[name, chunk] = rr.build(orcs[name], CAM, W, H, LIGHTS, 5, chunk=chunk)
        return orcs[name], trees[name, chunk]
    return get


def differing(a, b, what):
    n = int((a != b).any(axis=-1).sum())
    print("%s: %d of %d pixels differ" % (what, n, a.shape[0] * a.shape[1]))
    return n


def planes_differing(got, want, what):
    """Two trees as Scene.planes returns them: the number of (layer, plane) pairs that differ in a bit."""
    assert len(got) == len(want), (what, len(got), len(want))
    bad = 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w)
        for name in g:
            if not ru.same_plane(g[name], w[name]):
                print("%s: layer %d plane %s differs" % (what, k, name))
                bad += 1
    print("%s: %d layers, rays %s, %d planes differ" % (what, len(got), [len(g["coef"]) for g in got], bad))
    return bad


def dense_materials(flat, orc, lay):
    """A restated layer's material plane in the numbering of the scene description the kernel was given, after checking by
    value that it IS the oracle's material.  (test_gpu_raytree.py's helper.)"""
    pos = np.full(len(flat["tri_id"]), -1, dtype=np.int64)
    pos[flat["tri_id"]] = np.arange(len(flat["tri_id"]))
    mats = orc.materials()
    want = np.full(lay["prim"].shape, -1, dtype=np.int32)
    hit = lay["prim"] >= 0
    want[hit] = flat["tri_material"][pos[lay["prim"][hit]]]
    assert np.array_equal(want < 0, lay["material"] < 0)
    for dense, om in set(zip(want[want >= 0].tolist(), lay["material"][want >= 0].tolist())):
        assert np.array_equal(flat["materials"][dense]["values"], mats[om][1])
    return want


def assert_restated(flat, orc, got, want, what):
    """Every plane of every layer of a read-back tree against the restated tree `want`; `flat` = the description whose
    materials `orc` holds."""
    assert [len(g["coef"]) for g in got] == want["n_rays"], what
    for k, (g, lay) in enumerate(zip(got, want["layers"])):
        for name in rr.F64_PLANES:
            assert same_bits(g[name], lay[name], "%s layer %d %s" % (what, k, name)) == 0
        for name in ("in_object", "in_shadow", "child_refl", "child_refr"):
            assert np.array_equal(g[name], lay[name]), (what, k, name)
        assert np.array_equal(g["material"], dense_materials(flat, orc, lay)), (what, k)
        if k == 0:
            assert np.array_equal(g["pixel"], lay["pixel"])


def same_info(abi, t, tf, what):
    """mt_raytree_info of a regrown tree against a fresh one's: layers, rays, bytes."""
    got, want = abi.raytree_info(t), abi.raytree_info(tf)
    for key in INFO_KEYS:
        assert got[key] == want[key], (what, key, got[key], want[key])
    return got


def regrow_to(s, t, mats, fresh, tf_args, what, lights=LIGHTS):
    """set_materials(mats) + the regrow of `t`; holds the tree and its info to a fresh tree of `fresh` (made by
    fresh.tree(*tf_args)) and returns (the call's dict, the regrown tree's planes)."""
    s.set_materials(mats)
    out = s.abi.raytree_regrow(t)
    tf, _ = fresh.tree(*tf_args)
    got = s.planes(t)
    assert planes_differing(got, fresh.planes(tf), what + " vs a fresh tree") == 0
    info = same_info(s.abi, t, tf, what)
    assert out["n_layers_after"] == info["n_layers"]
    assert [k + n for k, n in zip(out["kept"], out["traced"])] == info["n_rays"][:info["n_layers"]], what
    fresh.destroy(tf)
    print("%s: regrown %d, layers %d -> %d, kept %s traced %s dropped %s, secondary %d hits %d shadow %d, %.3f ms kernels"
          % (what, out["regrown"], out["n_layers_before"], out["n_layers_after"], out["kept"], out["traced"],
             out["dropped"], out["rays_secondary"], out["shaded_hits"], out["rays_shadow"], out["kernel_ms"]))
    return out, got


# ---- 1. every edit, both directions

@pytest.mark.parametrize("chunk", me.CHUNKS, ids=["frame", "chunk"])
@pytest.mark.parametrize("name", list(rg.EDITS))
def test_every_edit_in_both_directions(name, chunk, make, variant_of, restated):
    """A tree under A regrown to B and back: every plane of every layer and mt_raytree_info against a fresh tree on the
    scene BUILT with the target materials and against the restatement; kept, traced, dropped and the work counters
    against regrow_ref; the shaded frame against mt_render_chunk on the built scene and the oracle; the colours
    quantise to the same bytes; after A -> B -> A the tree is bit-identical to the original."""
    vobj = variant_of("two_way", name)
    s, built_a, built_b = make("two_way"), make("two_way"), make(obj=vobj)
    for x in (s, built_a, built_b):
        x.set_lights(LIGHTS)
    A, B = s.materials, built_b.materials
    orc_a, tree_a = restated(None, chunk)
    orc_b, tree_b = restated(name, chunk)
    shadow = name in rg.SHADOW_EDITS
    assert tree_b["n_rays"] == rg.table(chunk)[name][0]
    t, _ = s.tree(CAM, W, H, chunk)
    original = s.planes(t)
    assert_restated(s.flat, orc_a, original, tree_a, name + ": the tree under A")
    steps = (("A -> B", B, built_b, orc_b, tree_a, tree_b), ("B -> A", A, built_a, orc_a, tree_b, tree_a))
    for what, mats, built, orc, tree_from, tree_to in steps:
        what = "%s %s %s" % (name, "chunk" if chunk else "frame", what)
        want = rg.match(tree_from, tree_to, shadow)
        out, got = regrow_to(s, t, mats, built, (CAM, W, H, chunk), what)
        assert_restated(built.flat, orc, got, tree_to, what + " vs the restatement")
        assert out["regrown"] == 1
        assert out["n_layers_before"] == len(tree_from["n_rays"]) and out["n_layers_after"] == len(tree_to["n_rays"])
        assert out["kept"] == want["kept"] and out["traced"] == want["traced"] and out["dropped"] == want["dropped"]
        print(what, "restated: secondary %d hits %d shadow %d" % (want["rays_secondary"], want["shaded_hits"], want["rays_shadow"]))
        assert out["rays_primary"] == 0
        assert out["rays_secondary"] == want["rays_secondary"]
        assert out["shaded_hits"] == want["shaded_hits"]
        assert out["rays_shadow"] == want["rays_shadow"]
        assert out["kernel_ms"] > 0 and out["total_ms"] >= out["kernel_ms"]
        trace_ms = s.abi.raytree_info(t)["trace_ms"]
        for k, n in enumerate(out["traced"]):
            assert (trace_ms[k] > 0) == (n > 0), (what, k, trace_ms[k], n)
        rgb = s.abi.raytree_shade(t, LIGHTS)["rgb"]
        assert differing(rgb, built.frame(CAM, W, H, chunk)["rgb"], what + " vs mt_render_chunk on the built scene") == 0
        assert differing(rgb, orc.render(CAM, W, H, chunk=chunk, max_level=5)["rgb"], what + " vs the oracle") == 0
        colors = s.abi.raytree_shade_colors(t, LIGHTS)["color"]
        assert differing(rr.v3d_to_rgb(colors.reshape(-1, 3)).reshape(rgb.shape), rgb, what + " colours, quantised") == 0
    assert planes_differing(s.planes(t), original, name + ": A -> B -> A vs the original") == 0


# ---- 2. edits that keep the shape

def test_same_shape_edits_do_what_update_materials_does(make, variant_of):
    """The seven same-shape edits at depth 5 and mirror 0.125 at depth 2, on two trees of one scene: one regrown, one
    updated -- the same planes, the same counters, regrown = 0, nothing traced or dropped."""
    s = make("two_way")
    s.set_lights(LIGHTS)
    A = s.materials
    for name, depth in [(n, 5) for n in me.SAME_SHAPE] + [("mirror 0.125", 2)]:
        B = M.MythTracer(variant_of("two_way", name)).flatten()["materials"]
        s.set_materials(A)
        t1, _ = s.tree(CAM, W, H, OFF_GRID, depth)
        t2, _ = s.tree(CAM, W, H, OFF_GRID, depth)
        before = s.abi.raytree_info(t1)
        s.set_materials(B)
        out = s.abi.raytree_regrow(t1)
        st = s.abi.raytree_update_materials(t2)
        n = before["n_layers"]
        print(name, depth, {k: out[k] for k in ("regrown", "kept", "traced", "dropped", "rays_shadow")})
        assert out["regrown"] == 0 and out["n_layers_before"] == out["n_layers_after"] == n
        assert out["kept"] == before["n_rays"][:n] and out["traced"] == [0] * n and out["dropped"] == [0] * n
        for key in ("rays_primary", "rays_secondary", "rays_shadow", "shaded_hits", "box_tests"):
            assert out[key] == st[key], (name, key)
        assert planes_differing(s.planes(t1), s.planes(t2), name + ": regrow vs update") == 0
        after = s.abi.raytree_info(t1)
        for key in INFO_KEYS:
            assert after[key] == before[key], (name, key)
        assert differing(s.abi.raytree_shade(t1, LIGHTS)["rgb"], s.frame(CAM, W, H, OFF_GRID, depth)["rgb"], name + ", shaded") == 0
        s.destroy(t1)
        s.destroy(t2)


# ---- 3. the argument checks, in order

def refused(abi, t, code, match):
    """mt_raytree_regrow_materials refuses with `code` and a message matching `match`; returns (info, stats)."""
    st, info = binding.mt_stats(), binding.mt_raytree_regrow_info()
    rc = abi.lib.mt_raytree_regrow_materials(t, binding.C.addressof(info), binding.C.addressof(st))
    text = abi.last_error()
    print("refused (%d): %s" % (rc, text))
    assert rc == code and re.search(match, text), (rc, text)
    return info, st.as_dict()


def test_argument_checks_in_order(make, variant_of):
    scene = "room_tex"
    cam = scenegen.ROOM_CAMERA
    w, h = 48, 27
    s, fresh = make(scene), make(obj=variant_of(scene, me.SCENE_EDITS[scene]))
    abi = s.abi
    s.set_lights(LIGHTS)
    t, _ = s.tree(cam, w, h)
    before = s.planes(t)
    n_layers = abi.raytree_info(t)["n_layers"]
    # (1) the tree
    refused(abi, None, MT_ERR_ARG, r"the ray tree is NULL")
    # (2) equal generations: nothing to do, whatever the lights are
    s.set_lights(LIGHTS[:1])
    out = abi.raytree_regrow(t)
    assert out["n_layers_before"] == out["n_layers_after"] == n_layers
    assert all(not np.any(v) for k, v in out.items() if k not in ("n_layers_before", "n_layers_after")), out
    # (3) before (4): a textured material's ambient together with a reflectance, with the light count wrong as well
    both = [dict(values=np.array(m["values"]).copy(), tex=m["tex"]) for m in fresh.materials]
    both[0]["values"][10] = 0.25
    s.set_materials(both)
    abi.read_stats(s.h)
    info, st = refused(abi, t, MT_ERR_UNSUPPORTED, r"has a texture and its ambient or tex changed")
    assert all(v == 0 for v in st.values()) and info.regrown == 0 and sum(info.traced) == 0
    scene_st = abi.read_stats(s.h)
    assert scene_st["rays_shadow"] == 0 and scene_st["box_tests"] == 0
    assert planes_differing(s.planes(t), before, "textured ambient: after the refusal") == 0
    # (4) before (5): a reflectance alone, which mt_raytree_update_materials would take to its check pass
    refl = [dict(values=np.array(m["values"]).copy(), tex=m["tex"]) for m in s.materials]
    refl[0]["values"][10] = 0.25
    s.set_materials(refl)
    refused(abi, t, MT_ERR_ARG, r"the scene has 1 lights, the ray tree was made with %d" % len(LIGHTS))
    assert planes_differing(s.planes(t), before, "light count: after the refusal") == 0
    with pytest.raises(RuntimeError, match=STALE):
        abi.raytree_shade(t, LIGHTS)
    # with the count right the call goes through
    s.set_lights(LIGHTS)
    out = abi.raytree_regrow(t)
    print("room_tex, material 0 reflective:", out["regrown"], out["traced"], out["dropped"])
    built = make(flat=dict(s.flat, materials=refl))
    built.set_lights(LIGHTS)
    tf, _ = built.tree(cam, w, h)
    assert planes_differing(s.planes(t), built.planes(tf), "room_tex regrown vs a fresh tree") == 0


# ---- 4. the update still refuses

def test_update_materials_still_refuses_and_the_regrow_then_succeeds(make, variant_of):
    s, built = make("two_way"), make(obj=variant_of("two_way", "pane opaque"))
    for x in (s, built):
        x.set_lights(LIGHTS)
    t, _ = s.tree(CAM, W, H)
    before = s.planes(t)
    s.set_materials(built.materials)
    with pytest.raises(RuntimeError, match=r"change the shape of the ray tree: \d+ rays spawn other children.*a new tree is needed"):
        s.abi.raytree_update_materials(t)
    assert planes_differing(s.planes(t), before, "after the update's refusal") == 0
    out, _ = regrow_to(s, t, built.materials, built, (CAM, W, H), "pane opaque after a refused update")
    assert out["regrown"] == 1 and out["dropped"] == rg.FRAME["pane opaque"][2]
    assert differing(s.abi.raytree_shade(t, LIGHTS)["rgb"], built.frame(CAM, W, H)["rgb"], "shaded") == 0


# ---- 5. a light that moved before the regrow

def test_a_moved_light_then_the_regrow_then_update_lights(make, variant_of):
    """Kept rays hold the old position's planes, traced rays the new one's: update_lights over the moved index makes the
    tree the fresh tree under B and the new lights."""
    s, built = make("two_way"), make(obj=variant_of("two_way", "blue refl"))
    moved = lu.moved([tuple(float(v) for v in l) for l in LIGHTS], 1, (150.0, 120.0, 250.0))
    s.set_lights(LIGHTS)
    t, _ = s.tree(CAM, W, H)
    s.set_materials(built.materials)
    s.set_lights(moved)
    out = s.abi.raytree_regrow(t)
    assert out["regrown"] == 1 and out["traced"] == rg.FRAME["blue refl"][1]
    built.set_lights(moved)
    tf, _ = built.tree(CAM, W, H)
    want = built.planes(tf)
    assert planes_differing(s.planes(t), want, "before update_lights (expected to differ)") > 0
    s.abi.raytree_update_lights(t, [1])
    assert planes_differing(s.planes(t), want, "a moved light, the regrow, update_lights") == 0
    assert differing(s.abi.raytree_shade(t, moved)["rgb"], built.frame(CAM, W, H)["rgb"], "shaded under the moved light") == 0


# ---- 6. ray lists, nine lights, no light

def test_a_ray_list_tree_nine_lights_and_zero_lights(make, variant_of):
    s, built = make("two_way"), make(obj=variant_of("two_way", "blue refl"))
    A = s.materials
    orc = orclib.OracleScene(variant_of("two_way", "blue refl"))
    rays = rl.panorama_rays(40, 20)
    for x in (s, built):
        x.set_lights(LIGHTS)
    t, _ = s.tree_rays(rays, 40)
    s.set_materials(built.materials)
    out = s.abi.raytree_regrow(t)
    tf, _ = built.tree_rays(rays, 40)
    got = s.planes(t)
    print("panorama:", out["regrown"], out["kept"], out["traced"], out["dropped"])
    assert out["regrown"] == 1 and sum(out["traced"]) > 0
    assert planes_differing(got, built.planes(tf), "panorama vs a fresh tree") == 0
    same_info(s.abi, t, tf, "panorama")
    assert_restated(built.flat, orc, got, rl.build_from_rays(orc, rays, 40, 20, LIGHTS, 5), "panorama vs the restatement")
    assert differing(s.abi.raytree_shade(t, LIGHTS)["rgb"], built.abi.raytree_shade(tf, LIGHTS)["rgb"], "panorama, shaded") == 0
    # nine lights: the all-lights re-trace hands its list over in a buffer
    built9 = make(obj=variant_of("two_way", "grow and drop"))
    s.set_materials(A)
    for x in (s, built9):
        x.set_lights(NINE)
    t9, _ = s.tree(CAM, W, H, OFF_GRID)
    out, _ = regrow_to(s, t9, built9.materials, built9, (CAM, W, H, OFF_GRID), "nine lights", NINE)
    assert out["regrown"] == 1 and out["traced"] == rg.CHUNK["grow and drop"][1] and out["rays_shadow"] > 0
    assert differing(s.abi.raytree_shade(t9, NINE)["rgb"], built9.frame(CAM, W, H, OFF_GRID)["rgb"], "nine lights, shaded") == 0
    out, _ = regrow_to(s, t9, A, s, (CAM, W, H, OFF_GRID), "nine lights, back", NINE)
    assert out["dropped"] == rg.CHUNK["grow and drop"][1]
    # no light: nothing to re-trace, the traced rays run no loop
    s.set_materials(A)
    for x in (s, built9):
        x.set_lights([])
    t0, _ = s.tree(CAM, W, H, OFF_GRID)
    s.abi.read_stats(s.h)
    out, _ = regrow_to(s, t0, built9.materials, built9, (CAM, W, H, OFF_GRID), "zero lights", [])
    assert out["regrown"] == 1 and out["traced"] == rg.CHUNK["grow and drop"][1] and out["rays_shadow"] == 0
    assert differing(s.abi.raytree_shade(t0, [])["rgb"], built9.frame(CAM, W, H, OFF_GRID)["rgb"], "zero lights, shaded") == 0
    # a tree of zero lights under a scene that now has some: refused, untouched
    before = s.planes(t0)
    s.set_materials(A)
    s.set_lights(LIGHTS)
    refused(s.abi, t0, MT_ERR_ARG, r"the scene has 3 lights, the ray tree was made with 0")
    assert planes_differing(s.planes(t0), before, "zero-light tree under a lit scene") == 0


# ---- 7. chunk shapes

@pytest.mark.parametrize("chunk", [(17, 30, 63, 5), (17, 30, 64, 5), (17, 30, 65, 5), (48, 40, 1, 1)], ids=str)
def test_chunk_shapes(chunk, make, variant_of):
    """Layer 0 one short of, at and one past a multiple of 64, and a single pixel: to matte (every layer below 0 dropped)
    and back (every one traced), then blue refl."""
    s, matte, blue = make("two_way"), make(obj=variant_of("two_way", "matte")), make(obj=variant_of("two_way", "blue refl"))
    A = s.materials
    for x in (s, matte, blue):
        x.set_lights(LIGHTS)
    t, _ = s.tree(CAM, W, H, chunk)
    original = s.planes(t)
    n_a = s.abi.raytree_info(t)["n_rays"][:len(original)]
    assert n_a[0] == chunk[2] * chunk[3]
    out, _ = regrow_to(s, t, matte.materials, matte, (CAM, W, H, chunk), "chunk %s to matte" % (chunk,))
    assert out["kept"] == n_a[:1] and out["dropped"] == [0] + n_a[1:]
    assert differing(s.abi.raytree_shade(t, LIGHTS)["rgb"], matte.frame(CAM, W, H, chunk)["rgb"], "matte, shaded") == 0
    out, got = regrow_to(s, t, A, s, (CAM, W, H, chunk), "chunk %s back from matte" % (chunk,))
    assert out["traced"] == [0] + n_a[1:]
    assert planes_differing(got, original, "chunk %s: back vs the original" % (chunk,)) == 0
    out, _ = regrow_to(s, t, blue.materials, blue, (CAM, W, H, chunk), "chunk %s to blue refl" % (chunk,))
    assert differing(s.abi.raytree_shade(t, LIGHTS)["rgb"], blue.frame(CAM, W, H, chunk)["rgb"], "blue refl, shaded") == 0


def test_a_chunk_that_only_misses(make, variant_of):
    s, matte = make("two_way"), make(obj=variant_of("two_way", "matte"))
    away = (200.0, 110.0, -50.0, 0.0, 180.0, 0.0, 100.0)  # turned away from the room
    s.set_lights(LIGHTS)
    t, _ = s.tree(away, W, H, (8, 8, 20, 10))
    before = s.planes(t)
    assert s.abi.raytree_info(t)["n_rays"] == [200] and (before[0]["material"] == -1).all()
    s.set_materials(matte.materials)
    out = s.abi.raytree_regrow(t)
    assert out["regrown"] == 0 and out["kept"] == [200] and out["traced"] == [0] and out["dropped"] == [0]
    assert out["rays_secondary"] == 0 and out["rays_shadow"] == 0
    assert planes_differing(s.planes(t), before, "misses only") == 0
    s.abi.raytree_shade(t, LIGHTS)  # (fresh)


# ---- 8. the deep layout

@pytest.mark.parametrize("layout", [0, 1])
def test_deep_layout(layout, make, variant_of):
    """An octree of 16 levels, both settings of MT_TUNE_DEEP_LAYOUT: the DEEP instantiations of raytree_trace_kernel over
    a dense list of traced rays -- the wood made reflective --, and back."""
    w, h = 32, 18
    edit = {"wood": {"Refl": 0.3}}
    s, built = make("loft"), make(obj=variant_of("loft", edit))
    assert s.flat["tree_depth"] >= 16
    cam = scenegen.ROOM_CAMERA
    for x in (s, built):
        x.abi.set_tuning(x.h, "DEEP_LAYOUT", float(layout))
        x.set_lights(LIGHTS)
    A = s.materials
    t, _ = s.tree(cam, w, h)
    original = s.planes(t)
    out, _ = regrow_to(s, t, built.materials, built, (cam, w, h), "loft, layout %d" % layout)
    assert out["regrown"] == 1 and sum(out["traced"]) > 0 and out["rays_secondary"] == sum(out["traced"])
    assert differing(s.abi.raytree_shade(t, LIGHTS)["rgb"], built.frame(cam, w, h)["rgb"], "loft, layout %d" % layout) == 0
    out, got = regrow_to(s, t, A, s, (cam, w, h), "loft, layout %d, back" % layout)
    assert out["regrown"] == 1 and sum(out["dropped"]) > 0 and sum(out["traced"]) == 0
    assert planes_differing(got, original, "loft: back vs the original") == 0


# ---- 9. two trees

def test_two_trees_of_one_scene_in_either_order(make, variant_of):
    s, built = make("two_way"), make(obj=variant_of("two_way", "grow and drop"))
    for x in (s, built):
        x.set_lights(LIGHTS)
    A, B = s.materials, built.materials
    full, _ = s.tree(CAM, W, H, None, 5)
    part, _ = s.tree(CAM, W, H, OFF_GRID, 4)
    part_a = s.planes(part)
    for order in ((full, part), (part, full)):
        s.set_materials(B)
        s.abi.raytree_regrow(order[0])
        with pytest.raises(RuntimeError, match=STALE):  # (the other one is still stale, and untouched)
            s.abi.raytree_shade(order[1], LIGHTS)
        if order[1] is part:
            assert planes_differing(s.planes(part), part_a, "the other tree") == 0
        s.abi.raytree_regrow(order[1])
        ff, _ = built.tree(CAM, W, H, None, 5)
        fp, _ = built.tree(CAM, W, H, OFF_GRID, 4)
        assert planes_differing(s.planes(full), built.planes(ff), "the full tree") == 0
        assert planes_differing(s.planes(part), built.planes(fp), "the chunk's tree") == 0
        built.destroy(ff)
        built.destroy(fp)
        s.set_materials(A)
        for t in order:
            assert s.abi.raytree_regrow(t)["regrown"] == 1
        assert planes_differing(s.planes(part), part_a, "back under A") == 0


# ---- 10. the frame kernels

def test_frame_kernels_and_cost_history_are_untouched(make, variant_of):
    """test_gpu_material_edit.py's recipe around a regrow there and back: a depth-5 frame before and after has the same
    bytes, the regrows add no entry to mt_scene_kernel_times, and the second frame is the repeated launch it would have
    been."""
    w, h = 1920, 1080
    cam = scenegen.ROOM_CAMERA
    sens = binding.sensor(cam, w, h)
    s = make("room")
    B = M.MythTracer(variant_of("room", {"mirror": {"Refl": 0}})).flatten()["materials"]
    A = s.materials
    s.set_lights(LIGHTS)
    s.abi.set_engine(s.h, 1)
    t, _ = s.tree(cam, w, h)
    s.abi.kernel_times(s.h)
    f1 = s.abi.render_chunk(s.h, sens, w, h)["rgb"]
    s.set_materials(B)
    assert s.abi.raytree_regrow(t)["regrown"] == 1
    s.set_materials(A)
    assert s.abi.raytree_regrow(t)["regrown"] == 1
    f2 = s.abi.render_chunk(s.h, sens, w, h)["rgb"]
    assert np.array_equal(f1, f2)
    pm, rm = s.abi.kernel_times(s.h)
    print("primary_ms", pm, "render_ms", rm)
    assert len(pm) == 2, pm
    assert pm[1] < pm[0] / 3, pm  # second frame: the order kernels, not primary_kernel (see test_gpu_gbuffer.py)


# ---- 11. facade and Python

def test_facade_and_python(make, variant_of):
    """MythTracer.update_materials + RayTree.regrow (UpdateMaterials, RegrowRayTree through the ctypes shim)."""
    w, h = 61, 37
    built = make(obj=variant_of("two_way", "pane opaque"))
    built.set_lights(LIGHTS)
    want = built.abi.render_chunk(built.h, binding.sensor(CAM, w, h), w, h, max_depth=5)["rgb"]
    m = M.MythTracer(rr.TWO_WAY)
    m.set_lights(LIGHTS)
    tree = m.raytree(CAM, w, h, max_depth=5)
    before = tree.shade()["rgb"]
    n_before = tree.info["n_rays"]
    m.update_materials({"pane": {"tr": 0}})
    with pytest.raises(RuntimeError, match="change the shape"):
        tree.update_materials()
    with pytest.raises(RuntimeError, match=STALE):
        tree.shade()
    out = tree.regrow()
    print("facade:", n_before, "->", tree.info["n_rays"], out)
    assert tree.info["n_rays"] != n_before
    assert out["kernel_ms"] > 0 and out["counters"]["rays_primary"] == 0 and out["counters"]["rays_secondary"] == 0
    assert out["counters"]["rays_shadow"] > 0
    after = tree.shade()["rgb"]
    assert differing(after, want, "facade: regrow + shade vs a scene built with the edit") == 0
    assert differing(after, m.render(CAM, w, h)["rgb"], "facade: regrow + shade vs render") == 0
    m.update_materials({"pane": {"tr": 0.6}})
    out = tree.regrow()
    assert out["counters"]["rays_secondary"] > 0 and tree.info["n_rays"] == n_before
    assert differing(tree.shade()["rgb"], before, "facade: back under A") == 0
    tree.close()
    with pytest.raises(RuntimeError, match="closed"):
        tree.regrow()
    m.close()


# ---- 12. the workload's size

def test_a_drop_only_regrow_costs_less_than_a_new_tree_at_1080p(make, variant_of):
    """The one test of this size: room, 1920x1080, bench camera and lights, d = 5.  Asserted, an ordering only: the regrow
    after the mirror is switched off -- it traces no ray, against the 2.6 M of a new tree -- takes less device time than
    mt_raytree_create on the same scene in the same run.  The grow case (the mirror back on) is printed beside it."""
    w, h = 1920, 1080
    cam = scenegen.ROOM_CAMERA
    s = make("room")
    A = s.materials
    B = M.MythTracer(variant_of("room", {"mirror": {"Refl": 0}})).flatten()["materials"]
    s.set_lights(LIGHTS)
    t, _ = s.tree(cam, w, h)
    s.set_materials(B)  # warm-up, there and back
    s.abi.raytree_regrow(t)
    s.set_materials(A)
    s.abi.raytree_regrow(t)
    s.set_materials(B)
    drop = s.abi.raytree_regrow(t)
    assert drop["regrown"] == 1 and sum(drop["traced"]) == 0 and sum(drop["dropped"]) > 0 and drop["rays_shadow"] == 0
    fresh, fst = s.tree(cam, w, h)
    assert s.abi.raytree_info(fresh)["n_rays"] == s.abi.raytree_info(t)["n_rays"]
    rgb = s.abi.raytree_shade(t, LIGHTS)["rgb"]
    assert differing(rgb, s.abi.raytree_shade(fresh, LIGHTS)["rgb"], "1080p drop vs a new tree, shaded") == 0
    s.destroy(fresh)
    s.set_materials(A)
    grow = s.abi.raytree_regrow(t)
    print("1080p room, mirror off: regrow %.3f ms kernels / %.3f ms wall, dropped %d; new tree %.3f ms kernels / %.3f ms wall"
          % (drop["kernel_ms"], drop["total_ms"], sum(drop["dropped"]), fst["kernel_ms"], fst["total_ms"]))
    print("1080p room, mirror back on (not asserted): regrow %.3f ms kernels / %.3f ms wall, traced %d of %d rays"
          % (grow["kernel_ms"], grow["total_ms"], sum(grow["traced"]), sum(s.abi.raytree_info(t)["n_rays"])))
    assert drop["kernel_ms"] < fst["kernel_ms"]
