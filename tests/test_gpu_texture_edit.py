"""Texture edits in place on a real MI355X (-m gpu): mt_scene_set_texture / mt_scene_get_texture_info, ray trees that
keep uvw (mt_scene_set_raytree_uvw, mt_raytree_read_uvw), the lifted refusal of mt_raytree_update_materials and
mt_raytree_regrow_materials, and mt_retexture_gbuffer (include/mythtracer_hip.h; the device side is retextured_albedo and
mt::gbuffer_retexture_kernel in mythtracer_amd/csrc/mt_gbuffer.h, used by mt::raytree_recommit_kernel and
mt::raytree_regrow_copy_kernel in mt_raytree.h).

The bar is identity, no tolerance: doubles as uint64 views with NaN = NaN, bytes and indices equal.  The truth for an
edited state always comes from a scene newly CREATED from the same description with the edited materials and textures
(mt_scene_create), never from the edit calls; one frame per replacement texture is also held to the oracle, built with
that texture.  Two scenes: room_tex as the ragged chunk (5, 3, 61, 45) of a 96 x 64 image at depth 3 under two lights,
and the tiny scene of tests/texture_edit_ref.py (a textured floor with coordinates from -0.5 to 2, a second textured wall,
a mirror, a pane, a matte wall, a triangle whose uvw is NaN).  Every test prints its counts.
"""
import copy
import ctypes
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import lightbuffer_ref as lr  # noqa: E402
import orclib  # noqa: E402
import raytree_update_ref as ru  # noqa: E402
import texture_edit_ref as te  # noqa: E402
from gbuffer_ref import same_bits  # noqa: E402

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding, scenegen  # noqa: E402

MT_OK, MT_ERR_ARG, MT_ERR_UNSUPPORTED = 0, -1, -3
STALE = "materials were edited after the ray tree was made"
TEXTURED_AMBIENT = "has a texture and its ambient or tex changed: the ray tree keeps neither the texel nor the primitive"
NO_UVW = r"texture %d was set after the ray tree was made and material %d uses it: the ray tree keeps no uvw"

SETUPS = {
    "tiny": dict(cam=te.TINY_CAMERA, image=te.TINY_IMAGE, chunk=None, depth=te.TINY_DEPTH, lights=te.TINY_LIGHTS),
    "room_tex": dict(cam=scenegen.ROOM_CAMERA, image=(96, 64), chunk=(5, 3, 61, 45), depth=3, lights=lr.BENCH_LIGHTS[:2]),
}
REPLACEMENTS = ("1x1", "2x2", "3x5_f64", "original")


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"


# ---- the descriptions, and what an edit is

@pytest.fixture(scope="module")
def descriptions(scenes):
    """name -> the flat description (MythTracer.flatten()) with one more texture at the end that no material uses."""
    out = {}
    tiny = te.build_tiny(M.MythTracer()).flatten()
    room = M.MythTracer(scenes["room_tex"]).flatten()
    for name, flat in (("tiny", tiny), ("room_tex", room)):
        flat["textures"] = list(flat["textures"]) + [dict(texels=te.tiny_textures()[2])]
        out[name] = flat
    assert [m["tex"] for m in tiny["materials"]] == [0, 1, -1, -1, -1]
    for got, want in zip(tiny["textures"], te.tiny_textures()):
        assert np.array_equal(got["texels"], want) and got["texels"].dtype == np.uint8
    return out


def state_of(flat):
    """(materials, textures): deep copies of a description's tables, free to edit."""
    mats = [dict(values=np.array(m["values"], dtype=np.float64), tex=int(m["tex"])) for m in flat["materials"]]
    return mats, [np.array(t["texels"], copy=True) for t in flat["textures"]]


def described(flat, mats, texs):
    return dict(flat, materials=mats, textures=[dict(texels=t) for t in texs])


class Scene:
    def __init__(self, flat, setup, keep_uvw=None):
        self.abi = M.hip_abi()
        self.flat, self.setup = flat, setup
        self.h = self.abi.scene_create(flat)
        self.abi.set_lights(self.h, setup["lights"])
        if keep_uvw is not None:
            self.abi.set_raytree_uvw(self.h, keep_uvw)
        self.trees = []

    def close(self):
        for t in self.trees:
            self.abi.raytree_destroy(t)
        self.abi.scene_destroy(self.h)

    def sensor(self):
        return binding.sensor(self.setup["cam"], *self.setup["image"])

    def tree(self):
        W, H = self.setup["image"]
        t, stats = self.abi.raytree_create(self.h, self.sensor(), W, H, chunk=self.setup["chunk"], max_depth=self.setup["depth"])
        self.trees.append(t)
        return t

    def tree_rays(self, rays, in_object, coef):
        t, _ = self.abi.raytree_create_rays(self.h, rays, in_object=in_object, coef=coef, max_depth=self.setup["depth"])
        self.trees.append(t)
        return t

    def frame(self, depth=None):
        W, H = self.setup["image"]
        return self.abi.render_chunk(self.h, self.sensor(), W, H, chunk=self.setup["chunk"],
                                     max_depth=self.setup["depth"] if depth is None else depth)["rgb"]

    def gbuffer(self, channels):
        W, H = self.setup["image"]
        return self.abi.render_gbuffer(self.h, self.sensor(), W, H, chunk=self.setup["chunk"], channels=channels)

    def planes(self, t):
        """Every plane of every layer of a tree, read back; uvw too where the tree keeps it."""
        out = []
        for k in range(self.abi.raytree_info(t)["n_layers"]):
            lay = self.abi.raytree_read_layer(t, k)
            if self.abi.raytree_keeps_uvw(t):
                lay["uvw"] = self.abi.raytree_read_uvw(t, k)
            out.append(lay)
        return out

    def apply(self, mats, texs, set_textures):
        """The edit calls: mt_scene_set_texture for the listed textures, mt_scene_set_materials."""
        for i in set_textures:
            self.abi.set_texture(self.h, i, texs[i])
        self.abi.set_materials(self.h, mats)


@pytest.fixture
def make(descriptions):
    made = []

    def _make(name, mats=None, texs=None, keep_uvw=None):
        flat = descriptions[name]
        if mats is not None:
            flat = described(flat, mats, texs)
        made.append(Scene(flat, SETUPS[name], keep_uvw))
        return made[-1]
    yield _make
    for s in made:
        s.close()


def planes_differing(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    bad = 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w), (sorted(g), sorted(w))
        for name in g:
            if not ru.same_plane(g[name], w[name]):
                print("%s: layer %d plane %s differs" % (what, k, name))
                bad += 1
    print("%s: %d layers, rays %s, planes %s, %d planes differ" % (what, len(got), [len(g["coef"]) for g in got], len(got[0]), bad))
    return bad


def differing(a, b, what):
    n = int((a != b).any(axis=-1).sum())
    print("%s: %d of %d pixels differ" % (what, n, a.shape[0] * a.shape[1]))
    return n


def roles(scene, mats):
    """Which materials and textures the edits use: (material with texture 0, material with texture 1, an untextured
    matte material that layer 0 of the scene's tree hits most)."""
    m_a = [i for i, m in enumerate(mats) if m["tex"] == 0][0]
    m_b = [i for i, m in enumerate(mats) if m["tex"] == 1][0]
    t = scene.tree()
    hit = scene.abi.raytree_read_layer(t, 0, planes=("material",))["material"]
    scene.trees.remove(t)
    scene.abi.raytree_destroy(t)
    plain = [i for i, m in enumerate(mats) if m["tex"] < 0 and m["values"][10] == 0.0 and m["values"][11] == 0.0]
    counts = [(int((hit == i).sum()), i) for i in plain]
    assert max(counts)[0] > 0
    return m_a, m_b, max(counts)[1]


def edit(name, mats, texs, role, original):
    """The edited tables and the textures to set, for the edit called `name`."""
    m_a, m_b, m_plain = role
    rep = te.replacements(original)
    mats, texs = copy.deepcopy(mats), [t.copy() for t in texs]
    set_textures = []
    if name in ("texture", "all", "regrow"):
        texs[0] = rep["2x2" if name == "texture" else "3x5_f64" if name == "all" else "1x1"]
        set_textures.append(0)
    if name in ("ambient", "all"):
        mats[m_a]["values"][0:3] = (0.9, 0.5, 0.25)
    if name in ("tex moved", "all"):
        mats[m_b]["tex"] = -1
        if name == "tex moved":
            mats[m_a]["tex"] = 1
    if name in ("plain textured", "all"):
        mats[m_plain]["tex"] = 0
    if name == "regrow":
        mats[m_plain]["values"][10] = 0.5  # a matte surface made reflective: the tree's shape changes
    return mats, texs, set_textures


# ---- 0. the argument checks that need a live scene, in the documented order

def test_argument_checks_behind_a_live_scene(make):
    s = make("tiny")
    abi = s.abi
    texels = np.zeros((2, 2, 3), dtype=np.uint8)
    good = binding.mt_texture(2, 2, binding.MT_TEX_RGB8, 0, texels.ctypes.data)
    n_tex = len(s.flat["textures"])

    def refused(rc, message):
        assert rc == MT_ERR_ARG and abi.last_error() == message, (rc, abi.last_error())

    for index in (-1, n_tex, 10 ** 6):  # the index comes before the texture
        for tex in (None, ctypes.byref(good)):
            refused(abi.lib.mt_scene_set_texture(s.h, index, tex), "texture index %d outside 0..%d" % (index, n_tex - 1))
            refused(abi.lib.mt_scene_get_texture_info(s.h, index, tex), "texture index %d outside 0..%d" % (index, n_tex - 1))
    refused(abi.lib.mt_scene_set_texture(s.h, 1, None), "the mt_texture is NULL")
    refused(abi.lib.mt_scene_get_texture_info(s.h, 1, None), "the mt_texture is NULL")
    for bad in (binding.mt_texture(0, 2, 0, 0, texels.ctypes.data), binding.mt_texture(2, -1, 0, 0, texels.ctypes.data),
                binding.mt_texture(30001, 2, 0, 0, texels.ctypes.data), binding.mt_texture(2, 2, 0, 0, None),
                binding.mt_texture(2, 2, 2, 0, texels.ctypes.data)):
        refused(abi.lib.mt_scene_set_texture(s.h, 1, ctypes.byref(bad)), "texture 1: bad size/format")
    # nothing of this changed the scene
    for i, t in enumerate(s.flat["textures"]):
        h, w = t["texels"].shape[:2]
        assert abi.get_texture_info(s.h, i) == dict(width=w, height=h, format=binding.MT_TEX_RGB8)
    refused(abi.lib.mt_scene_set_raytree_uvw(s.h, 2), "keep must be 0 or 1")
    refused(abi.lib.mt_scene_set_raytree_uvw(s.h, -1), "keep must be 0 or 1")
    # mt_raytree_read_uvw: tree, layer, out, then a tree without the plane
    plain = s.tree()
    n_layers = abi.raytree_info(plain)["n_layers"]
    out = np.zeros((abi.raytree_info(plain)["n_rays"][0], 3))
    assert abi.lib.mt_raytree_keeps_uvw(plain) == 0
    for layer in (-1, n_layers):
        for o in (None, out.ctypes.data):
            refused(abi.lib.mt_raytree_read_uvw(plain, layer, o), "layer %d outside the ray tree's %d layers" % (layer, n_layers))
    refused(abi.lib.mt_raytree_read_uvw(plain, 0, None), "the uvw output is NULL")
    refused(abi.lib.mt_raytree_read_uvw(plain, 0, out.ctypes.data),
            "the ray tree keeps no uvw: it was made with mt_scene_set_raytree_uvw at 0")
    abi.set_raytree_uvw(s.h, True)
    kept = s.tree()
    assert abi.lib.mt_raytree_keeps_uvw(kept) == 1 and abi.lib.mt_raytree_keeps_uvw(plain) == 0
    refused(abi.lib.mt_raytree_read_uvw(kept, 0, None), "the uvw output is NULL")
    assert abi.lib.mt_raytree_read_uvw(kept, 0, out.ctypes.data) == MT_OK
    # mt_retexture_gbuffer: uvw may be missing only while no current material has a texture
    m = np.zeros((2, 2), dtype=np.int32)
    a = np.zeros((2, 2, 3))
    g = binding.mt_gbuffer(material=m.ctypes.data, albedo=a.ctypes.data)
    for fn in (abi.lib.mt_retexture_gbuffer, abi.lib.mt_retexture_gbuffer_device):
        refused(fn(s.h, 0, 2, ctypes.byref(g), None),
                "material 0 has a texture: the retexture needs the uvw plane of the mt_gbuffer")


# ---- 1. the scene contract

@pytest.mark.parametrize("rep", REPLACEMENTS)
@pytest.mark.parametrize("name", list(SETUPS))
def test_set_texture_is_a_scene_created_with_that_texture(name, rep, make, descriptions):
    """mt_scene_set_texture, then mt_render_chunk, mt_render_gbuffer's albedo and every plane of mt_raytree_create equal
    the same calls on a scene newly created with that texture; the tiny scene's frame also equals the oracle's."""
    mats, texs = state_of(descriptions[name])
    original = texs[0].copy()
    new = te.replacements(original)[rep]
    s = make(name)
    abi = s.abi
    frame_a = s.frame()
    albedo_a = s.gbuffer(("albedo",))["albedo"]
    stale = s.tree()
    texs[0] = new
    abi.set_texture(s.h, 0, new)
    fresh = make(name, mats, texs)
    want_info = dict(width=new.shape[1], height=new.shape[0],
                     format=binding.MT_TEX_RGB8 if new.dtype == np.uint8 else binding.MT_TEX_F64)
    assert abi.get_texture_info(s.h, 0) == want_info == abi.get_texture_info(fresh.h, 0)
    got = s.frame()
    assert differing(got, fresh.frame(), "%s %s frame vs a fresh scene" % (name, rep)) == 0
    n = differing(got, frame_a, "%s %s frame vs before (expected to differ unless the bytes are the original's)" % (name, rep))
    assert (n == 0) == (rep == "original")
    g, gf = s.gbuffer(("albedo", "uvw", "material")), fresh.gbuffer(("albedo", "uvw", "material"))
    assert same_bits(g["albedo"], gf["albedo"], "%s %s albedo vs a fresh scene" % (name, rep)) == 0
    assert (same_bits(g["albedo"], albedo_a, "albedo vs before") == 0) == (rep == "original")
    # ... and the restatement, from the planes themselves
    want = te.albedo(mats, texs, g["material"], g["uvw"]).reshape(g["albedo"].shape)
    assert same_bits(g["albedo"], want, "%s %s albedo vs the restatement" % (name, rep)) == 0
    t, tf = s.tree(), fresh.tree()
    assert planes_differing(s.planes(t), fresh.planes(tf), "%s %s tree vs a fresh scene's" % (name, rep)) == 0
    assert differing(abi.raytree_shade(t, s.setup["lights"])["rgb"], got, "shaded tree vs the frame") == 0
    # every set makes the trees of the scene stale, the original bytes too: no texels are compared
    with pytest.raises(RuntimeError, match=STALE):
        abi.raytree_shade(stale, s.setup["lights"])
    if name == "tiny":
        orc = te.build_tiny(orclib.OracleScene(), textures=[new, texs[1]])
        orc.set_lights(s.setup["lights"])
        W, H = s.setup["image"]
        assert differing(got, orc.render(s.setup["cam"], W, H, max_level=s.setup["depth"])["rgb"], "tiny %s vs the oracle" % rep) == 0


# ---- 2. a plain tree keeps every refusal, and gets the new one

@pytest.mark.parametrize("name", list(SETUPS))
def test_a_plain_tree_is_refused_and_untouched(name, make, descriptions):
    mats, texs = state_of(descriptions[name])
    s = make(name)
    abi = s.abi
    role = roles(s, mats)
    m_a = role[0]
    t = s.tree()
    before = s.planes(t)
    assert "uvw" not in before[0] and not abi.raytree_keeps_uvw(t)

    def refused(match):
        for fn, args in ((abi.lib.mt_raytree_update_materials, ()), (abi.lib.mt_raytree_regrow_materials, (None,))):
            st = binding.mt_stats()
            rc = fn(t, *args, ctypes.addressof(st))
            text = abi.last_error()
            print("refused (%d): %s" % (rc, text))
            assert rc == MT_ERR_UNSUPPORTED and re.search(match, text), (rc, text)
        assert planes_differing(s.planes(t), before, "the refused tree") == 0
        with pytest.raises(RuntimeError, match=STALE):
            abi.raytree_shade(t, s.setup["lights"])

    # (a) the ambient of a textured material: today's message
    b, _, _ = edit("ambient", mats, texs, role, texs[0])
    s.apply(b, texs, [])
    refused(re.escape("material %d %s" % (m_a, TEXTURED_AMBIENT)))
    s.apply(mats, texs, [])
    assert abi.raytree_update_materials(t)["kernel_ms"] == 0.0  # (back to the snapshot: nothing to do)
    # (b) a texture in use was set: the new refusal, naming the texture and the first material that uses it
    new = te.replacements(texs[0])["2x2"]
    abi.set_texture(s.h, 0, new)
    refused(NO_UVW % (0, m_a))
    # a new tree is what the message asks for
    t2 = s.tree()
    assert differing(abi.raytree_shade(t2, s.setup["lights"])["rgb"], s.frame(), "a new tree after the set") == 0
    # (c) a texture no material uses: MT_OK, and nothing is launched
    spare = len(texs) - 1
    assert all(m["tex"] != spare for m in mats)
    abi.set_texture(s.h, spare, te.replacements(texs[spare])["1x1"])
    with pytest.raises(RuntimeError, match=STALE):
        abi.raytree_shade(t2, s.setup["lights"])
    stats = abi.raytree_update_materials(t2)
    print("unused texture: %s" % stats)
    assert stats["kernel_ms"] == 0.0 and stats["rays_shadow"] == 0
    assert differing(abi.raytree_shade(t2, s.setup["lights"])["rgb"], s.frame(), "fresh again after an unused texture") == 0


# ---- 3. and 4. a tree with uvw takes the edit

EDITS = ("texture", "ambient", "tex moved", "plain textured", "all", "regrow")


@pytest.mark.parametrize("what", EDITS)
@pytest.mark.parametrize("name", list(SETUPS))
def test_a_tree_with_uvw_takes_the_edit(name, what, make, descriptions):
    """mt_raytree_update_materials (regrow: mt_raytree_regrow_materials) on a tree with uvw and on a 64 x 1 ray-list tree
    made from its layer 1: every plane of every layer, uvw included, and mt_raytree_info's counts equal a tree newly
    created on a scene newly created with the edited tables; the shaded tree is mt_render_chunk's frame."""
    mats, texs = state_of(descriptions[name])
    s = make(name, keep_uvw=True)
    abi = s.abi
    role = roles(s, mats)
    t = s.tree()
    assert abi.raytree_keeps_uvw(t)
    base = s.planes(t)
    assert len(base) >= 2 and len(base[1]["coef"]) >= 64
    # uvw is the G-buffer's, bit for bit (layer 0 in raytree_layer0_index's order: through the pixel plane)
    gb = s.gbuffer(("uvw",))["uvw"].reshape(-1, 3)
    assert same_bits(base[0]["uvw"], gb[base[0]["pixel"]], name + " layer 0 uvw vs mt_render_gbuffer") == 0
    hits = ~np.isnan(base[0]["point"][:, 0])
    assert np.isnan(base[0]["uvw"][~hits]).all()
    if name == "tiny":  # a hit whose uvw is NaN
        assert (hits & np.isnan(base[0]["uvw"][:, 0])).any()
    rays, in_object, coef = base[1]["ray"][:64], base[1]["in_object"][:64], base[1]["coef"][:64]
    tl = s.tree_rays(rays, in_object, coef)
    assert abi.raytree_keeps_uvw(tl)
    b_mats, b_texs, set_textures = edit(what, mats, texs, role, texs[0])
    s.apply(b_mats, b_texs, set_textures)
    fresh = make(name, b_mats, b_texs, keep_uvw=True)
    for tree, fresh_tree, kind in ((t, fresh.tree(), "chunk"), (tl, fresh.tree_rays(rays, in_object, coef), "ray list")):
        with pytest.raises(RuntimeError, match=STALE):
            abi.raytree_shade(tree, s.setup["lights"])
        label = "%s %s %s" % (name, what, kind)
        if what == "regrow":
            if kind == "chunk":  # (the 64 rays of the list need not see the new mirror)
                with pytest.raises(RuntimeError, match="change the shape"):
                    abi.raytree_update_materials(tree)
            out = abi.raytree_regrow(tree)
            print("%s: regrown %d kept %s traced %s dropped %s" % (label, out["regrown"], out["kept"], out["traced"], out["dropped"]))
            if kind == "chunk":
                assert out["regrown"] == 1 and sum(out["traced"]) > 0
        else:
            out = abi.raytree_update_materials(tree)
            print("%s: kernel_ms %.3f rays_shadow %d" % (label, out["kernel_ms"], out["rays_shadow"]))
            assert out["rays_shadow"] == 0 and out["rays_primary"] == 0 and out["rays_secondary"] == 0
            assert out["kernel_ms"] > 0.0
        got = s.planes(tree)
        assert planes_differing(got, fresh.planes(fresh_tree), label + " vs a fresh tree") == 0
        gi, wi = abi.raytree_info(tree), abi.raytree_info(fresh_tree)
        assert (gi["n_layers"], gi["n_rays"], gi["bytes"]) == (wi["n_layers"], wi["n_rays"], wi["bytes"])
        if kind == "chunk":
            assert differing(abi.raytree_shade(tree, s.setup["lights"])["rgb"], s.frame(), label + " shaded vs the frame") == 0
            changed = sum(not ru.same_plane(g["albedo"], w["albedo"]) for g, w in zip(got, base) if len(g["coef"]) == len(w["coef"]))
            print("%s: albedo changed in %d layers" % (label, changed))
            assert changed > 0
        else:
            want = abi.raytree_shade_colors(fresh_tree, s.setup["lights"])["color"]
            assert same_bits(abi.raytree_shade_colors(tree, s.setup["lights"])["color"], want, label + " colours") == 0
        # a second call has nothing to do
        assert abi.raytree_update_materials(tree)["kernel_ms"] == 0.0


# ---- 5. the switch

@pytest.mark.parametrize("name", list(SETUPS))
def test_the_switch_costs_24_bytes_per_ray_and_nothing_when_off(name, make):
    never, s = make(name), make(name)
    abi = s.abi
    t_never = never.tree()
    abi.set_raytree_uvw(s.h, True)
    t_on = s.tree()
    abi.set_raytree_uvw(s.h, False)
    t_off = s.tree()
    i_never, i_on, i_off = (abi.raytree_info(t) for t in (t_never, t_on, t_off))
    print("%s: rays %s bytes %d without uvw, %d with" % (name, i_never["n_rays"], i_never["bytes"], i_on["bytes"]))
    assert i_off["bytes"] == i_never["bytes"] and i_off["n_rays"] == i_never["n_rays"] == i_on["n_rays"]
    assert i_on["bytes"] - i_never["bytes"] == 24 * sum(i_never["n_rays"])
    assert not abi.raytree_keeps_uvw(t_off) and abi.raytree_keeps_uvw(t_on) and not abi.raytree_keeps_uvw(t_never)
    p_never, p_off, p_on = never.planes(t_never), s.planes(t_off), s.planes(t_on)
    assert planes_differing(p_off, p_never, name + " switch off vs a scene that never heard of it") == 0
    for lay in p_on:  # the switch moves no bit of any other plane
        lay.pop("uvw")
    assert planes_differing(p_on, p_never, name + " switch on, the other planes") == 0


# ---- 6. mt_retexture_gbuffer

@pytest.mark.parametrize("name", list(SETUPS))
def test_retextured_planes_are_the_gbuffer_after_the_edit(name, make, descriptions):
    mats, texs = state_of(descriptions[name])
    s = make(name)
    abi = s.abi
    role = roles(s, mats)
    W, H = s.setup["image"]
    lights = s.setup["lights"]
    before = s.gbuffer(("point", "normal", "uvw", "albedo", "material"))
    b_mats, b_texs, set_textures = edit("all", mats, texs, role, texs[0])
    s.apply(b_mats, b_texs, set_textures)
    out = abi.retexture_gbuffer(s.h, before)
    print("%s: retexture %s" % (name, out["stats"]))
    after = s.gbuffer(("albedo",))
    assert same_bits(out["albedo"], after["albedo"], name + " retextured albedo vs mt_render_gbuffer after the edit") == 0
    assert same_bits(out["albedo"], before["albedo"], name + " retextured albedo vs before (expected to differ)") > 0
    st = out["stats"]
    assert st["kernel_ms"] > 0.0 and all(st[k] == 0 for k in binding.STAT_NAMES)
    gb = dict(before, albedo=out["albedo"])
    lb = abi.render_lightbuffer(s.h, s.sensor(), W, H, len(lights), chunk=s.setup["chunk"])
    direct = abi.shade_direct(s.h, s.sensor(), W, H, gb, lb, lights, chunk=s.setup["chunk"])["rgb"]
    assert differing(direct, s.frame(depth=0), name + " mt_shade_direct over the retextured planes vs depth 0") == 0


def test_retexture_on_planes_no_scene_produces(make, descriptions):
    """Data only: material -1, -7, n_materials and beyond, uvw NaN, +-1e300, -0.0, integral; NaN = NaN."""
    mats, texs = state_of(descriptions["tiny"])
    texs[0] = te.replacements(texs[0])["3x5_f64"]
    mats[te.MATTE]["tex"] = 1
    s = make("tiny", mats, texs)
    abi = s.abi
    material, uvw = te.synthetic_planes(len(mats))
    assert (material == -7).any() and (material == len(mats)).any() and np.isnan(uvw).any() and (uvw == 1e300).any()
    want = te.albedo(mats, texs, material, uvw).reshape(uvw.shape)
    got = abi.retexture_gbuffer(s.h, dict(material=material, uvw=uvw))["albedo"]
    assert same_bits(got, want, "synthetic planes vs the restatement") == 0
    outside = (material < 0) | (material >= len(mats))
    assert np.isnan(got[outside]).all() and not np.isnan(got[material == te.MIRROR]).any()
    # the device form writes the same bits
    import torch
    dev = torch.device("cuda", 0)
    d_m = torch.from_numpy(material).to(dev)
    d_u = torch.from_numpy(uvw).to(dev)
    d_a = torch.zeros(uvw.shape, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    h, w = material.shape
    abi.retexture_gbuffer_device(s.h, w, h, dict(material=d_m.data_ptr(), uvw=d_u.data_ptr(), albedo=d_a.data_ptr()))
    torch.cuda.synchronize()
    assert same_bits(d_a.cpu().numpy(), want, "the device form vs the restatement") == 0
    # without a texture in use uvw may be missing
    for m in mats:
        m["tex"] = -1
    abi.set_materials(s.h, mats)
    got = abi.retexture_gbuffer(s.h, dict(material=material))["albedo"]
    assert same_bits(got, te.albedo(mats, texs, material, None).reshape(uvw.shape), "no texture in use, no uvw") == 0


# ---- 7. the facade

def test_facade_update_texture_and_keep_uvw():
    W, H = te.TINY_IMAGE
    m = te.build_tiny(M.MythTracer())
    m.set_lights(te.TINY_LIGHTS)
    m.set_max_level(te.TINY_DEPTH)
    m.set_raytree_keep_uvw(True)
    frame_a = m.render(te.TINY_CAMERA, W, H)["rgb"]
    floor = te.tiny_textures()[0]
    new = te.replacements(floor)["3x5_f64"]
    with m.raytree(te.TINY_CAMERA, W, H) as tree:
        assert M.hip_abi().raytree_keeps_uvw(tree._tree())
        m.update_texture("tex0", new)
        frame_b = m.render(te.TINY_CAMERA, W, H)["rgb"]
        assert differing(frame_b, frame_a, "facade: B vs A (expected to differ)") > 0
        fresh = te.build_tiny(M.MythTracer(), textures=[new, te.tiny_textures()[1]])
        fresh.set_lights(te.TINY_LIGHTS)
        fresh.set_max_level(te.TINY_DEPTH)
        assert differing(frame_b, fresh.render(te.TINY_CAMERA, W, H)["rgb"], "facade: UpdateTexture vs a scene built with it") == 0
        with pytest.raises(RuntimeError, match=STALE):
            tree.shade()
        tree.update_materials()
        assert differing(tree.shade()["rgb"], frame_b, "facade: the updated tree vs the frame") == 0
    with pytest.raises(RuntimeError, match="no texture named"):
        m.update_texture("nothing", new)
    # a texture of the table that was not uploaded (no triangle's material uses it) is refused by the facade
    m.add_texture("loose", te.texel_values(floor))
    with pytest.raises(RuntimeError, match="was not uploaded"):
        m.update_texture("loose")
    # without the switch the tree refuses a texture edit
    m.set_raytree_keep_uvw(False)
    with m.raytree(te.TINY_CAMERA, W, H) as plain:
        m.update_texture("tex0", te.texel_values(floor))
        with pytest.raises(RuntimeError, match="keeps no uvw"):
            plain.update_materials()
