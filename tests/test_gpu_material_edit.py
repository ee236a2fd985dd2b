"""Material edits in place on a real MI355X (-m gpu): mt_scene_set_materials / mt_scene_get_materials,
mt_raytree_update_materials, MythTracer::UpdateMaterials / UpdateRayTreeMaterials (include/mythtracer_hip.h; the kernels
are mt::raytree_recoef_kernel and mt::raytree_recommit_kernel in mythtracer_amd/csrc/mt_raytree.h).

The bar is identity, no tolerance.  The truth for materials B always comes from a scene BUILT with B -- a .mtl with the
edited numbers next to a copy of the .obj (material_edit_ref.variant), or the same add_material / add_triangle calls --,
never from the edit call: after set_materials(B) every rendering call is held to a FRESH scene made from that variant and
to the oracle that loaded it; a tree made under A and updated is held plane by plane and layer by layer to a fresh
mt_raytree_create on the variant's scene and to the restatement of tests/raytree_ref.py (doubles as uint64 views with
NaN = NaN, bytes and indices equal, every ray).  The edits are those of tests/material_edit_ref.py, which
tests/test_material_edit_cpu.py shows to change what they claim.  Every test prints its counts.
"""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gbuffer_ref  # noqa: E402
import lightupdate_ref as lu  # noqa: E402
import material_edit_ref as me  # noqa: E402
import orclib  # noqa: E402
import raylist_ref as rl  # noqa: E402
import raytree_ref as rr  # noqa: E402
import raytree_update_ref as ru  # noqa: E402
from gbuffer_ref import same_bits  # noqa: E402

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding, scenegen, tiling  # noqa: E402

W, H = me.W, me.H
OFF_GRID = me.OFF_GRID
DEPTHS = (0, 1, 2, 5)
LIGHTS = me.LIGHTS
CAM = rr.CAMERAS["two_way"]
NINE = [(40.0 * i, 150.0 + 10 * i, 380.0 - 40 * i, 0.02, 0.01 * i, 0.03, 0.2, 0.15, 0.1 + 0.02 * i, 0.1, 0.2, 0.1)
        for i in range(9)]
MT_ERR_ARG, MT_ERR_UNSUPPORTED = -1, -3
STALE = "materials were edited after the ray tree was made"


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
    """(scene name, edit name or edit) -> the variant's .obj, written once."""
    made = {}

    def get(scene, edit):
        key = (scene, edit if isinstance(edit, str) else repr(edit))
        if key not in made:
            d = tmp_path_factory.mktemp("variant")
            made[key] = me.variant(me.obj_of(scenes, scene), me.EDITS[edit] if isinstance(edit, str) else edit, str(d))
        return made[key]
    return get


def same_geometry(a, b):
    for name in ("node_aabb", "node_first_child", "node_prim_begin", "node_prim_count", "tri_id", "tri_vertex", "tri_material"):
        assert np.array_equal(a.flat[name], b.flat[name]), name
    assert len(a.materials) == len(b.materials)


def same_materials(got, want):
    return len(got) == len(want) and all(
        np.array_equal(np.asarray(g["values"]).view(np.uint64), np.asarray(w["values"], dtype=np.float64).view(np.uint64))
        and g["tex"] == w["tex"] for g, w in zip(got, want))


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


def refused(abi, t, code, match):
    """mt_raytree_update_materials refuses with `code` and a message matching `match`; returns the message."""
    st = binding.mt_stats()
    rc = abi.lib.mt_raytree_update_materials(t, binding.C.addressof(st))
    text = abi.last_error()
    print("refused (%d): %s" % (rc, text))
    assert rc == code and re.search(match, text), (rc, text)
    return text, st.as_dict()


# ---- 1. the scene contract

@pytest.mark.parametrize("scene", list(me.SCENE_EDITS))
def test_scene_contract(scene, scenes, make, variant_of):
    """After set_materials(B): mt_render_chunk at depths 0 and 5, _ss with s = 2, the G-buffer's albedo and material
    planes, the light buffer + mt_shade_direct and every plane of mt_raytree_create equal a fresh scene BUILT with B and
    the oracle that loaded it; get_materials returns B; A -> B -> A gives A's frame."""
    edit = me.SCENE_EDITS[scene]
    cam = rr.CAMERAS.get(scene, scenegen.ROOM_CAMERA)
    vobj = variant_of(scene, edit)
    s, fresh = make(scene), make(obj=vobj)
    same_geometry(s, fresh)
    A, B = s.materials, fresh.materials
    assert not same_materials(A, B)
    orc_a, orc = orclib.OracleScene(me.obj_of(scenes, scene)), orclib.OracleScene(vobj)
    me.check_variant(orc_a.materials(), orc.materials(), edit)
    orc.set_lights(LIGHTS)
    abi = s.abi
    for x in (s, fresh):
        x.set_lights(LIGHTS)
    frame_a = s.frame(cam, W, H)["rgb"]
    assert same_materials(abi.get_materials(s.h, len(A)), A)
    s.set_materials(B)
    assert same_materials(abi.get_materials(s.h, len(B)), B)
    sens = binding.sensor(cam, W, H)
    for d in (0, 5):
        got = s.frame(cam, W, H, None, d)["rgb"]
        assert differing(got, fresh.frame(cam, W, H, None, d)["rgb"], "%s d=%d vs a fresh scene" % (scene, d)) == 0
        assert differing(got, orc.render(cam, W, H, max_level=d)["rgb"], "%s d=%d vs the oracle" % (scene, d)) == 0
    assert differing(s.frame(cam, W, H)["rgb"], frame_a, "%s: B vs A (expected to differ)" % scene) > 0
    for chunk in (None, OFF_GRID):
        got = abi.render_chunk_ss(s.h, binding.sensor(cam, 2 * W, 2 * H), W, H, 2, chunk=chunk)["rgb"]
        want = abi.render_chunk_ss(fresh.h, binding.sensor(cam, 2 * W, 2 * H), W, H, 2, chunk=chunk)["rgb"]
        assert differing(got, want, "%s ss=2 %s vs a fresh scene" % (scene, chunk)) == 0
    samples = orc.render(cam, 2 * W, 2 * H)["rgb"]
    got = abi.render_chunk_ss(s.h, binding.sensor(cam, 2 * W, 2 * H), W, H, 2)["rgb"]
    assert differing(got, tiling.resolve_ss(samples, 2), "%s ss=2 vs the oracle's resolved sample frame" % scene) == 0
    # the G-buffer's planes that hold a material
    gb = abi.render_gbuffer(s.h, sens, W, H, channels=("point", "normal", "albedo", "material"))
    gbf = abi.render_gbuffer(fresh.h, sens, W, H, channels=("point", "normal", "albedo", "material"))
    want = gbuffer_ref.oracle_gbuffer(orc, cam, W, H)
    assert same_bits(gb["albedo"], gbf["albedo"], scene + " albedo vs a fresh scene") == 0
    assert same_bits(gb["albedo"], want["albedo"], scene + " albedo vs the oracle") == 0
    assert np.array_equal(gb["material"], gbf["material"])
    # the light buffer and the deferred relight
    lb = abi.render_lightbuffer(s.h, sens, W, H, len(LIGHTS))
    lbf = abi.render_lightbuffer(fresh.h, sens, W, H, len(LIGHTS))
    assert same_bits(lb["power"], lbf["power"], scene + " power vs a fresh scene") == 0
    assert np.array_equal(lb["in_shadow"], lbf["in_shadow"])
    direct = abi.shade_direct(s.h, sens, W, H, gb, lb, LIGHTS)["rgb"]
    assert differing(direct, abi.shade_direct(fresh.h, sens, W, H, gbf, lbf, LIGHTS)["rgb"], scene + " shade_direct vs a fresh scene") == 0
    assert differing(direct, orc.render(cam, W, H, max_level=0)["rgb"], scene + " shade_direct vs the oracle at depth 0") == 0
    # a tree made after the edit
    t, _ = s.tree(cam, W, H)
    tf, _ = fresh.tree(cam, W, H)
    got = s.planes(t)
    assert planes_differing(got, fresh.planes(tf), scene + " tree vs a fresh scene's") == 0
    assert_restated(fresh.flat, orc, got, rr.build(orc, cam, W, H, LIGHTS, 5), scene + " tree vs the restatement")
    assert differing(abi.raytree_shade(t, LIGHTS)["rgb"], s.frame(cam, W, H)["rgb"], scene + " shaded tree") == 0
    # and back
    s.set_materials(A)
    assert same_materials(abi.get_materials(s.h, len(A)), A)
    assert differing(s.frame(cam, W, H)["rgb"], frame_a, "%s: A -> B -> A" % scene) == 0


def test_set_materials_argument_checks_in_order(make):
    s = make("two_way")
    abi = s.abi
    A = s.materials
    n = len(A)
    frame = s.frame(CAM, W, H)["rgb"]
    arr = abi._material_array(A)
    for fn in (abi.lib.mt_scene_set_materials, abi.lib.mt_scene_get_materials):
        for k in (n - 1, n + 1, 0, -1):  # the count before the array
            for p in (arr, None):
                assert fn(s.h, p, k) == MT_ERR_ARG
                assert abi.last_error() == "%d materials for a scene made with %d" % (k, n)
        assert fn(s.h, None, n) == MT_ERR_ARG and abi.last_error() == "the material array is NULL"
    bad = [dict(m) for m in A]
    bad[2]["tex"] = 0  # two_way has no texture
    with pytest.raises(RuntimeError, match="material 2: texture index 0 outside -1..-1"):
        s.set_materials(bad)
    bad[2]["tex"] = -2
    with pytest.raises(RuntimeError, match="material 2: texture index -2 outside -1..-1"):
        s.set_materials(bad)
    assert same_materials(abi.get_materials(s.h, n), A)
    assert differing(s.frame(CAM, W, H)["rgb"], frame, "after the refusals") == 0


# ---- 2. the tree contract

@pytest.mark.parametrize("name", list(me.SAME_SHAPE))
def test_tree_contract(name, make, variant_of):
    """A tree under A, set_materials(B), the update: every plane of every layer is a fresh tree's on a scene BUILT with B
    and the restatement's; info unchanged; the shaded frame is mt_render_chunk's under B and the oracle's;
    mt_raytree_shade_colors quantises to the same bytes -- whole frame and off-grid chunk, max_depth 0, 1, 2 and 5."""
    edit = me.EDITS[name]
    vobj = variant_of("two_way", name)
    s, fresh = make("two_way"), make(obj=vobj)
    same_geometry(s, fresh)
    A, B = s.materials, fresh.materials
    orc = orclib.OracleScene(vobj)
    orc.set_lights(LIGHTS)
    shadow_edit = any(k in f for f in edit.values() for k in ("Tr", "Tf"))
    for x in (s, fresh):
        x.set_lights(LIGHTS)
    for chunk in me.CHUNKS:
        want5 = rr.build(orc, CAM, W, H, LIGHTS, 5, chunk=chunk)
        for d in DEPTHS:
            what = "%s %s d=%d" % (name, "chunk" if chunk else "frame", d)
            s.set_materials(A)
            t, _ = s.tree(CAM, W, H, chunk, d)
            info = s.abi.raytree_info(t)
            s.set_materials(B)
            with pytest.raises(RuntimeError, match=STALE):
                s.abi.raytree_shade(t, LIGHTS)
            st = s.abi.raytree_update_materials(t)
            after = s.abi.raytree_info(t)
            for key in ("n_rays", "bytes", "n_layers", "n_lights", "chunk", "max_depth"):
                assert after[key] == info[key], (what, key)
            tf, _ = fresh.tree(CAM, W, H, chunk, d)
            got = s.planes(t)
            assert planes_differing(got, fresh.planes(tf), what + " vs a fresh tree") == 0
            want = rr.truncated(want5, d)
            assert_restated(fresh.flat, orc, got, want, what)
            print(what, "rays_shadow", st["rays_shadow"], "restated", want["rays_shadow"], "kernel_ms %.3f" % st["kernel_ms"])
            assert st["rays_primary"] == st["rays_secondary"] == st["shaded_hits"] == 0
            assert st["rays_shadow"] == (want["rays_shadow"] if shadow_edit else 0)
            assert st["kernel_ms"] > 0 and st["total_ms"] >= st["kernel_ms"]
            rgb = s.abi.raytree_shade(t, LIGHTS)["rgb"]
            assert differing(rgb, fresh.frame(CAM, W, H, chunk, d)["rgb"], what + " vs mt_render_chunk on a fresh scene") == 0
            assert differing(rgb, s.frame(CAM, W, H, chunk, d)["rgb"], what + " vs mt_render_chunk after the edit") == 0
            assert differing(rgb, orc.render(CAM, W, H, chunk=chunk, max_level=d)["rgb"], what + " vs oracle") == 0
            colors = s.abi.raytree_shade_colors(t, LIGHTS)["color"]
            assert differing(rr.v3d_to_rgb(colors.reshape(-1, 3)).reshape(rgb.shape), rgb, what + " colours, quantised") == 0
            fresh.destroy(tf)
            s.destroy(t)


def test_ray_list_tree_and_nine_lights(make, variant_of):
    """The composite edit on a tree over the caller's rays (a 40x20 panorama) and on a tree of nine lights."""
    vobj = variant_of("two_way", "composite")
    s, fresh = make("two_way"), make(obj=vobj)
    A, B = s.materials, fresh.materials
    orc = orclib.OracleScene(vobj)
    rays = rl.panorama_rays(40, 20)
    for x in (s, fresh):
        x.set_lights(LIGHTS)
    t, _ = s.tree_rays(rays, 40)
    s.set_materials(B)
    st = s.abi.raytree_update_materials(t)
    tf, fst = fresh.tree_rays(rays, 40)
    got = s.planes(t)
    assert planes_differing(got, fresh.planes(tf), "panorama vs a fresh tree") == 0
    want = rl.build_from_rays(orc, rays, 40, 20, LIGHTS, 5)
    assert_restated(fresh.flat, orc, got, want, "panorama vs the restatement")
    assert st["rays_shadow"] == fst["rays_shadow"] > 0
    assert differing(s.abi.raytree_shade(t, LIGHTS)["rgb"], fresh.abi.raytree_shade(tf, LIGHTS)["rgb"], "panorama, shaded") == 0
    s.set_materials(A)
    for x in (s, fresh):
        x.set_lights(NINE)
    t9, _ = s.tree(CAM, W, H, OFF_GRID)
    s.set_materials(B)
    st = s.abi.raytree_update_materials(t9)
    tf9, fst = fresh.tree(CAM, W, H, OFF_GRID)
    assert planes_differing(s.planes(t9), fresh.planes(tf9), "nine lights vs a fresh tree") == 0
    assert st["rays_shadow"] == fst["rays_shadow"] > 0
    assert differing(s.abi.raytree_shade(t9, NINE)["rgb"], fresh.frame(CAM, W, H, OFF_GRID)["rgb"], "nine lights, shaded") == 0


# ---- 3. refusals

@pytest.mark.parametrize("name", list(me.SHAPE_BREAKING))
def test_a_shape_breaking_edit_is_refused_and_the_tree_is_untouched(name, make, variant_of):
    vobj = variant_of("two_way", name)
    s = make("two_way")
    A, B = s.materials, M.MythTracer(vobj).flatten()["materials"]
    abi = s.abi
    orc_a, orc_b = orclib.OracleScene(rr.TWO_WAY), orclib.OracleScene(vobj)
    restated = rr.build(orc_a, CAM, W, H, LIGHTS, 5)
    cp = me.check_pass(restated, orc_b.materials())
    s.set_lights(LIGHTS)
    t, _ = s.tree(CAM, W, H)
    before = s.planes(t)
    frame_a = abi.raytree_shade(t, LIGHTS)["rgb"]
    assert_restated(s.flat, orc_a, before, restated, name + ": the tree under A")
    s.set_materials(B)
    text, st = refused(abi, t, MT_ERR_UNSUPPORTED, r"change the shape")
    m = re.search(r"(\d+) rays spawn other children, the first in layer (\d+) at ray (\d+)", text)
    print(name, "restated: %d mismatches, the first at %s" % (cp["count"], cp["first"]))
    assert m and (int(m.group(2)), int(m.group(3))) == cp["first"] and int(m.group(1)) == cp["count"]
    assert st["rays_shadow"] == 0 and st["box_tests"] == 0
    assert planes_differing(s.planes(t), before, name + ": after the refusal") == 0
    with pytest.raises(RuntimeError, match=STALE):
        abi.raytree_shade(t, LIGHTS)
    with pytest.raises(RuntimeError, match=STALE):
        abi.raytree_shade_colors(t, LIGHTS)
    with pytest.raises(RuntimeError, match=STALE):
        abi.raytree_update_lights(t, [1])
    assert abi.raytree_info(t)["n_rays"] == me.TREE_A
    refused(abi, t, MT_ERR_UNSUPPORTED, r"change the shape")  # (and again: still refused, still untouched)
    assert planes_differing(s.planes(t), before, name + ": after the second refusal") == 0
    s.set_materials(A)
    st = abi.raytree_update_materials(t)
    assert st["kernel_ms"] == 0 and st["rays_shadow"] == 0  # (the snapshot is A's: nothing to launch)
    assert planes_differing(s.planes(t), before, name + ": A set back") == 0
    assert differing(abi.raytree_shade(t, LIGHTS)["rgb"], frame_a, name + ": A set back, shaded") == 0


def test_mirror_0125_at_depth_2_succeeds(make, variant_of):
    """The layer the edit would change does not exist at depth 2: the update must succeed."""
    vobj = variant_of("two_way", "mirror 0.125")
    s, fresh = make("two_way"), make(obj=vobj)
    for x in (s, fresh):
        x.set_lights(LIGHTS)
    for chunk in me.CHUNKS:
        s.set_materials(s.materials)
        t, _ = s.tree(CAM, W, H, chunk, 2)
        s.set_materials(fresh.materials)
        s.abi.raytree_update_materials(t)
        tf, _ = fresh.tree(CAM, W, H, chunk, 2)
        assert planes_differing(s.planes(t), fresh.planes(tf), "mirror 0.125, depth 2, %s" % (chunk,)) == 0
        assert differing(s.abi.raytree_shade(t, LIGHTS)["rgb"], fresh.frame(CAM, W, H, chunk, 2)["rgb"], "mirror 0.125, depth 2") == 0


def test_a_textured_ambient_edit_is_unsupported(make, variant_of):
    scene = "room_tex"
    cam = scenegen.ROOM_CAMERA
    w, h = 48, 27
    s, fresh = make(scene), make(obj=variant_of(scene, me.SCENE_EDITS[scene]))
    abi = s.abi
    s.set_lights(LIGHTS)
    t, _ = s.tree(cam, w, h)
    before = s.planes(t)
    s.set_materials(fresh.materials)
    abi.read_stats(s.h)
    text, st = refused(abi, t, MT_ERR_UNSUPPORTED, r"has a texture and its ambient or tex changed")
    assert all(v == 0 for k, v in st.items() if k not in ("kernel_ms", "total_ms")) and st["kernel_ms"] == 0
    scene_st = abi.read_stats(s.h)
    assert scene_st["rays_shadow"] == 0 and scene_st["box_tests"] == 0
    assert planes_differing(s.planes(t), before, "textured ambient: after the refusal") == 0
    # Kd / Ks / Ns of the same textured material alone: nothing to do, and the shade follows
    kd_only = [dict(m) for m in s.materials]
    for i, (a, b) in enumerate(zip(s.materials, fresh.materials)):
        v = np.array(b["values"])
        v[0:3] = a["values"][0:3]
        kd_only[i] = dict(values=v, tex=a["tex"])
    s.set_materials(kd_only)
    st = abi.raytree_update_materials(t)
    assert st["kernel_ms"] == 0
    assert planes_differing(s.planes(t), before, "Kd / Ks / Ns only") == 0
    assert differing(abi.raytree_shade(t, LIGHTS)["rgb"], s.frame(cam, w, h)["rgb"], "Kd / Ks / Ns only, shaded") == 0


# ---- 4. edges

@pytest.mark.parametrize("chunk", [(17, 30, 63, 5), (17, 30, 64, 5), (17, 30, 65, 5), (48, 40, 1, 1)], ids=str)
def test_chunk_shapes(chunk, make, variant_of):
    s, fresh = make("two_way"), make(obj=variant_of("two_way", "composite"))
    for x in (s, fresh):
        x.set_lights(LIGHTS)
    t, _ = s.tree(CAM, W, H, chunk)
    s.set_materials(fresh.materials)
    s.abi.raytree_update_materials(t)
    tf, _ = fresh.tree(CAM, W, H, chunk)
    info = s.abi.raytree_info(t)
    print("chunk %s: layers %s" % (chunk, info["n_rays"][:info["n_layers"]]))
    assert info["n_rays"][0] == chunk[2] * chunk[3]
    assert planes_differing(s.planes(t), fresh.planes(tf), "chunk %s" % (chunk,)) == 0
    assert differing(s.abi.raytree_shade(t, LIGHTS)["rgb"], fresh.frame(CAM, W, H, chunk)["rgb"], "chunk %s" % (chunk,)) == 0


def test_a_chunk_that_only_misses_and_a_tree_of_zero_lights(make, variant_of):
    s, fresh = make("two_way"), make(obj=variant_of("two_way", "composite"))
    A, B = s.materials, fresh.materials
    away = (200.0, 110.0, -50.0, 0.0, 180.0, 0.0, 100.0)  # turned away from the room
    s.set_lights(LIGHTS)
    t, _ = s.tree(away, W, H, (8, 8, 20, 10))
    before = s.planes(t)
    assert s.abi.raytree_info(t)["n_rays"] == [200] and (before[0]["material"] == -1).all()
    s.set_materials(B)
    st = s.abi.raytree_update_materials(t)
    assert st["rays_shadow"] == 0 and st["kernel_ms"] > 0
    assert planes_differing(s.planes(t), before, "misses only") == 0
    # zero lights and the pane's transparency: no re-trace, and it succeeds
    s.set_materials(A)
    for x in (s, fresh):
        x.set_lights([])
    vtr = make(obj=variant_of("two_way", "pane Tr"))
    vtr.set_lights([])
    t0, _ = s.tree(CAM, W, H, OFF_GRID)
    s.set_materials(vtr.materials)
    s.abi.read_stats(s.h)
    st = s.abi.raytree_update_materials(t0)
    assert st["rays_shadow"] == 0 and st["box_tests"] == 0 and s.abi.read_stats(s.h)["box_tests"] == 0
    tf, _ = vtr.tree(CAM, W, H, OFF_GRID)
    assert planes_differing(s.planes(t0), vtr.planes(tf), "zero lights") == 0
    assert differing(s.abi.raytree_shade(t0, [])["rgb"], vtr.frame(CAM, W, H, OFF_GRID)["rgb"], "zero lights, shaded") == 0


def test_a_pane_no_ray_hits_but_a_shadow_ray_crosses(make):
    """material_edit_ref.hidden_pane_scene: the pane is outside the camera's view, between the floor and the light.  Its
    transparency changes no ray's material, coefficient or child -- only the light planes, which must follow."""
    w, h = me.HIDDEN_SIZE
    built = []
    for tr in (0.6, 0.5):
        m = M.MythTracer()
        floor, pane = me.hidden_pane_scene(m, tr)
        built.append(make(flat=m.flatten()))
        built[-1].set_lights(me.HIDDEN_LIGHTS)
    s, fresh = built
    same_geometry(s, fresh)
    t, _ = s.tree(me.HIDDEN_CAMERA, w, h)
    before = s.planes(t)
    assert len(before) == 1 and len(set(before[0]["material"].tolist())) == 1  # every ray hits the floor, none the pane
    s.set_materials(fresh.materials)
    st = s.abi.raytree_update_materials(t)
    tf, fst = fresh.tree(me.HIDDEN_CAMERA, w, h)
    got = s.planes(t)
    changed = int((got[0]["power"] != before[0]["power"]).sum())
    print("hidden pane: %d doubles of power changed, rays_shadow %d" % (changed, st["rays_shadow"]))
    assert changed == 672  # (tests/test_material_edit_cpu.py)
    assert planes_differing(got, fresh.planes(tf), "hidden pane vs a fresh tree") == 0
    assert st["rays_shadow"] == fst["rays_shadow"] > 0
    assert differing(s.abi.raytree_shade(t, me.HIDDEN_LIGHTS)["rgb"], fresh.frame(me.HIDDEN_CAMERA, w, h)["rgb"], "hidden pane") == 0


def test_an_edit_of_nothing_and_two_trees_in_either_order(make, variant_of):
    s, fresh = make("two_way"), make(obj=variant_of("two_way", "composite"))
    A, B = s.materials, fresh.materials
    abi = s.abi
    for x in (s, fresh):
        x.set_lights(LIGHTS)
    full, _ = s.tree(CAM, W, H, None, 5)
    part, _ = s.tree(CAM, W, H, OFF_GRID, 2)
    part_before = s.planes(part)
    frame = abi.raytree_shade(full, LIGHTS)["rgb"]
    # the same materials again: the generation stays, nothing is stale
    s.set_materials(A)
    s.set_materials([dict(values=np.array(m["values"]).copy(), tex=m["tex"]) for m in A])
    assert differing(abi.raytree_shade(full, LIGHTS)["rgb"], frame, "after an edit of nothing") == 0
    st = abi.raytree_update_materials(full)
    assert all(v == 0 for v in st.values())
    # two trees, updated in either order
    for order in ((full, part), (part, full)):
        s.set_materials(B)
        for t in order:
            with pytest.raises(RuntimeError, match=STALE):
                abi.raytree_shade(t, LIGHTS)
        abi.raytree_update_materials(order[0])
        with pytest.raises(RuntimeError, match=STALE):  # (the other one is still stale, and untouched)
            abi.raytree_shade(order[1], LIGHTS)
        if order[1] is part:
            assert planes_differing(s.planes(part), part_before, "the other tree") == 0
        abi.raytree_update_materials(order[1])
        ff, _ = fresh.tree(CAM, W, H, None, 5)
        fp, _ = fresh.tree(CAM, W, H, OFF_GRID, 2)
        assert planes_differing(s.planes(full), fresh.planes(ff), "the full tree") == 0
        assert planes_differing(s.planes(part), fresh.planes(fp), "the chunk's tree") == 0
        fresh.destroy(ff)
        fresh.destroy(fp)
        s.set_materials(A)
        for t in order:
            abi.raytree_update_materials(t)
        assert planes_differing(s.planes(part), part_before, "back under A") == 0


def test_an_edit_then_a_moved_light(make, variant_of):
    s, fresh = make("two_way"), make(obj=variant_of("two_way", "composite"))
    moved = lu.moved([tuple(float(v) for v in l) for l in LIGHTS], 1, (150.0, 120.0, 250.0))
    s.set_lights(LIGHTS)
    t, _ = s.tree(CAM, W, H)
    s.set_materials(fresh.materials)
    s.abi.raytree_update_materials(t)
    s.set_lights(moved)
    s.abi.raytree_update_lights(t, [1])
    fresh.set_lights(moved)
    tf, _ = fresh.tree(CAM, W, H)
    assert planes_differing(s.planes(t), fresh.planes(tf), "edit, then a moved light") == 0
    assert differing(s.abi.raytree_shade(t, moved)["rgb"], fresh.frame(CAM, W, H)["rgb"], "edit, then a moved light") == 0


@pytest.mark.parametrize("layout", [0, 1])
def test_deep_layout(layout, scenes, make, variant_of):
    """An octree of 16 levels, both settings of MT_TUNE_DEEP_LAYOUT: the re-trace through the DEEP instantiations of
    raytree_update_kernel after the glass's transparency changed."""
    w, h = 32, 18
    edit = {"glass": {"Tr": 0.5}}
    s, fresh = make("loft"), make(obj=variant_of("loft", edit))
    assert s.flat["tree_depth"] >= 16
    cam = scenegen.ROOM_CAMERA
    for x in (s, fresh):
        x.abi.set_tuning(x.h, "DEEP_LAYOUT", float(layout))
        x.set_lights(LIGHTS)
    t, _ = s.tree(cam, w, h)
    before = s.planes(t)
    s.set_materials(fresh.materials)
    st = s.abi.raytree_update_materials(t)
    tf, fst = fresh.tree(cam, w, h)
    got = s.planes(t)
    assert planes_differing(got, before, "loft: the update (expected to differ)") > 0
    assert planes_differing(got, fresh.planes(tf), "loft, layout %d, vs a fresh tree" % layout) == 0
    assert st["rays_shadow"] == fst["rays_shadow"] > 0
    assert differing(s.abi.raytree_shade(t, LIGHTS)["rgb"], fresh.frame(cam, w, h)["rgb"], "loft, layout %d" % layout) == 0


# ---- 5. the frame kernels

def test_frame_kernels_are_untouched_by_the_edit_calls(make):
    """test_gpu_raytree_update.py's recipe: a depth-5 frame before and after a set_materials of the SAME materials and
    a tree update is byte-identical, the calls add no entry to mt_scene_kernel_times, and the second frame is the
    repeated launch it would have been."""
    w, h = 1920, 1080
    cam = scenegen.ROOM_CAMERA
    sens = binding.sensor(cam, w, h)
    s = make("room")
    s.set_lights(LIGHTS)
    s.abi.set_engine(s.h, 1)
    t, _ = s.tree(cam, w, h)
    s.abi.kernel_times(s.h)
    f1 = s.abi.render_chunk(s.h, sens, w, h)["rgb"]
    A = s.materials
    B = [dict(values=np.array(m["values"]).copy(), tex=m["tex"]) for m in A]
    B[0]["values"][3:6] = (0.2, 0.3, 0.9)  # a diffuse colour: nothing for the tree to do
    s.set_materials(B)
    s.abi.raytree_update_materials(t)
    s.set_materials(A)
    s.abi.raytree_update_materials(t)
    f2 = s.abi.render_chunk(s.h, sens, w, h)["rgb"]
    assert np.array_equal(f1, f2)
    pm, rm = s.abi.kernel_times(s.h)
    print("primary_ms", pm, "render_ms", rm)
    assert len(pm) == 2, pm
    assert pm[1] < pm[0] / 3, pm  # second frame: the order kernels, not primary_kernel (see test_gpu_gbuffer.py)


# ---- 6. facade and Python

def test_facade_and_python_round_trip(make, tmp_path, variant_of):
    """MythTracer.update_materials / RayTree.update_materials (UpdateMaterials, UpdateRayTreeMaterials through the ctypes
    shim) and a C++ program against the facade's headers (tests/seam/material_edit_driver.cc)."""
    from mythtracer_amd import build
    w, h = 61, 37
    edit = {"mirror": {"Refl": 0.5, "Ka": (0.9, 0.5, 0.25)}}
    fresh = make(obj=variant_of("two_way", edit))
    fresh.set_lights(LIGHTS)
    want = fresh.abi.render_chunk(fresh.h, binding.sensor(CAM, w, h), w, h, max_depth=3)["rgb"]
    m = M.MythTracer(rr.TWO_WAY)
    m.set_lights(LIGHTS)
    tree = m.raytree(CAM, w, h, max_depth=3)
    before = tree.shade()["rgb"]
    m.update_materials({"mirror": {"refl": 0.5, "ka": (0.9, 0.5, 0.25)}})
    assert m.get_material("mirror")[0][10] == 0.5
    with pytest.raises(RuntimeError, match=STALE):
        tree.shade()
    up = tree.update_materials()
    print("facade:", tree.info["n_rays"], up)
    assert up["kernel_ms"] > 0 and up["counters"]["rays_shadow"] == 0 and up["counters"]["rays_primary"] == 0
    after = tree.shade()["rgb"]
    assert differing(after, want, "facade: update + shade vs a fresh scene built with the edit") == 0
    assert differing(after, m.render(CAM, w, h)["rgb"], "facade: update + shade vs render") == 0
    assert (after != before).any()
    m.update_materials({"pane": {"tr": 0}})  # (opaque: the refracted children are no longer spawned)
    with pytest.raises(RuntimeError, match="change the shape"):
        tree.update_materials()
    m.update_materials({"pane": {"tr": 0.6}, "mirror": {"refl": 0.6, "ka": (0.1, 0.1, 0.1)}})
    tree.update_materials()
    assert differing(tree.shade()["rgb"], before, "facade: back under A") == 0
    n_layers = tree.info["n_layers"]
    tree.close()
    with pytest.raises(RuntimeError, match="closed"):
        tree.update_materials()
    m.close()
    # the C++ driver
    exe = str(tmp_path / "material_edit_driver")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "seam", "material_edit_driver.cc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(build.HOST, "include"), "-I", build.INC,
                           "-o", exe, src, "-L", build.LIB, "-lmythtracer_host", "-lmythtracer_hip",
                           "-Wl,-rpath," + build.LIB])
    out = str(tmp_path / "t.bin")
    args = [exe, rr.TWO_WAY, str(w), str(h), "3"] + [repr(float(c)) for c in CAM] + ["mirror", "0.5", "0.9", "0.5", "0.25"]
    args += [str(len(LIGHTS))] + [repr(float(v)) for l in LIGHTS for v in l] + [out]
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    words = r.stdout.decode().split()
    print("driver:", words)
    assert words == ["layers", str(n_layers), "shadow", "0"]
    frames = np.frombuffer(open(out, "rb").read(), dtype=np.uint8).reshape(4, h, w, 3)
    assert differing(frames[0], before, "driver, the tree under A") == 0
    assert differing(frames[1], frames[2], "driver, UpdateRayTreeMaterials + ShadeRayTree vs RayTrace under B") == 0
    assert differing(frames[1], want, "driver vs a fresh scene built with the edit") == 0
    assert differing(frames[3], want, "driver, two replicas after UpdateMaterials") == 0


# ---- 7. the workload's size

def test_update_and_shade_cost_less_than_a_frame_at_1080p(make, variant_of):
    """The one test of this size: room, 1920x1080, bench camera and lights, d = 5.  Single runs after one warm-up.
    Asserted, orderings only: update + shade after a COLOUR edit takes less device time than the frame under B in the same
    process; update + shade after the mirror's reflectance 0.6 -> 0.5 takes less than a fresh mt_raytree_create.  The
    update after a glass Tr edit re-traces every light's planes: printed beside the frame, not asserted."""
    w, h = 1920, 1080
    cam = scenegen.ROOM_CAMERA
    s = make("room")
    A = s.materials
    edits = {"colour": {"blue": {"Ka": (0.9, 0.5, 0.25)}, "red": {"Kd": (0.2, 0.3, 0.9), "Ks": (0.5, 0.5, 0.5), "Ns": 12}},
             "mirror 0.5": {"mirror": {"Refl": 0.5}}, "glass Tr": {"glass": {"Tr": 0.5}}}
    tables = {k: M.MythTracer(variant_of("room", e)).flatten()["materials"] for k, e in edits.items()}
    s.set_lights(LIGHTS)
    t, _ = s.tree(cam, w, h)
    got = {}
    for k in ("colour", "mirror 0.5", "glass Tr"):
        s.set_materials(tables[k])  # warm-up
        s.abi.raytree_update_materials(t)
        s.abi.raytree_shade(t, LIGHTS)
        s.set_materials(A)
        s.abi.raytree_update_materials(t)
        s.set_materials(tables[k])
        up = s.abi.raytree_update_materials(t)
        sh = s.abi.raytree_shade(t, LIGHTS)
        frame = s.frame(cam, w, h)
        frame = s.frame(cam, w, h)  # (the repeated launch: ordered by the first one's costs)
        assert differing(sh["rgb"], frame["rgb"], "1080p %s: update + shade vs mt_render_chunk under B" % k) == 0
        got[k] = (up, sh["stats"], frame["stats"])
        print("1080p room, %s: update %.3f ms (wall %.3f) + shade %.3f ms = %.3f ms; frame under B %.3f ms; rays_shadow %d"
              % (k, up["kernel_ms"], up["total_ms"], sh["stats"]["kernel_ms"], up["kernel_ms"] + sh["stats"]["kernel_ms"],
                 frame["stats"]["kernel_ms"], up["rays_shadow"]))
        s.set_materials(A)
        s.abi.raytree_update_materials(t)
    fresh, fst = s.tree(cam, w, h)
    s.destroy(fresh)
    fresh, fst = s.tree(cam, w, h)
    print("1080p room: fresh create %.3f ms kernels / %.3f ms wall" % (fst["kernel_ms"], fst["total_ms"]))
    up, sh, frame = got["colour"]
    assert up["rays_shadow"] == 0 and up["kernel_ms"] + sh["kernel_ms"] < frame["kernel_ms"]
    up, sh, frame = got["mirror 0.5"]
    assert up["rays_shadow"] == 0 and up["kernel_ms"] + sh["kernel_ms"] < fst["kernel_ms"]
    assert got["glass Tr"][0]["rays_shadow"] > 0
