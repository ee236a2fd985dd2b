"""Vertex normals and texture coordinates edited in place, on a real MI355X (-m gpu): mt_scene_set_triangle_normals /
_uvw and their getters, and the attribute edit mt_raytree_update_materials / mt_raytree_regrow_materials take for a tree
that keeps tri (include/mythtracer_hip.h; the kernels are in mythtracer_amd/csrc/mt_raytree.h).

The bar is identity, no tolerance.  The truth for an edit always comes from a scene BUILT with it, never from the edit
call: mt_scene_create on the flat description with the array replaced (vertex_attr_ref.built), for frames also the
oracle on a scene filled through add_triangle with the edited arrays.  Trees are compared plane by plane and layer by
layer, tri and uvw included where kept, doubles as uint64 with NaN = NaN.  The edits and their counts are
vertex_attr_ref's, which tests/test_vertex_attr_cpu.py pins with the oracle alone.  Every test prints its counts.
"""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import assign_ref as ar  # noqa: E402
import orclib  # noqa: E402
import raytree_ref as rr  # noqa: E402
import raytree_update_ref as ru  # noqa: E402
import texture_edit_ref as te  # noqa: E402
import vertex_attr_ref as va  # noqa: E402

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding, scenegen  # noqa: E402

W, H = va.W, va.H
OFF_GRID = va.OFF_GRID
LIGHTS = va.LIGHTS
CAM = va.CAM
TW, TH = te.TINY_IMAGE
MT_ERR_ARG, MT_ERR_UNSUPPORTED = -1, -3
STALE = "materials were edited after the ray tree was made"
INFO_KEYS = ("n_rays", "n_layers", "bytes", "n_lights", "chunk", "max_depth")
TWO_WAY = dict(cam=CAM, w=W, h=H, depth=va.DEPTH, lights=LIGHTS)
TINY = dict(cam=te.TINY_CAMERA, w=TW, h=TH, depth=te.TINY_DEPTH, lights=te.TINY_LIGHTS)
KEY = {"normal": "tri_normal", "uvw": "tri_uvw"}


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"


class Scene:
    def __init__(self, flat, setup, tri=False, uvw=False):
        self.abi = M.hip_abi()
        self.flat, self.setup = flat, setup
        self.h = self.abi.scene_create(flat)
        self.trees = []
        self.abi.set_raytree_tri(self.h, tri)
        self.abi.set_raytree_uvw(self.h, uvw)
        self.abi.set_lights(self.h, setup["lights"])

    def close(self):
        for t in self.trees:
            self.abi.raytree_destroy(t)
        self.abi.scene_destroy(self.h)

    @property
    def n_tris(self):
        return len(self.flat["tri_material"])

    def set(self, which, array):
        (self.abi.set_triangle_normals if which == "normal" else self.abi.set_triangle_uvw)(self.h, array)

    def get(self, which):
        return (self.abi.get_triangle_normals if which == "normal" else self.abi.get_triangle_uvw)(self.h, self.n_tris).reshape(-1, 9)

    def sensor(self):
        return binding.sensor(self.setup["cam"], self.setup["w"], self.setup["h"])

    def tree(self, chunk=None, depth=None):
        t, _ = self.abi.raytree_create(self.h, self.sensor(), self.setup["w"], self.setup["h"], chunk=chunk,
                                       max_depth=self.setup["depth"] if depth is None else depth)
        self.trees.append(t)
        return t

    def tree_rays(self, rays):
        t, _ = self.abi.raytree_create_rays(self.h, rays, max_depth=self.setup["depth"])
        self.trees.append(t)
        return t

    def destroy(self, t):
        self.trees.remove(t)
        self.abi.raytree_destroy(t)

    def frame(self, chunk=None, depth=None):
        return self.abi.render_chunk(self.h, self.sensor(), self.setup["w"], self.setup["h"], chunk=chunk,
                                     max_depth=self.setup["depth"] if depth is None else depth)["rgb"]

    def planes(self, t):
        """Every plane of every layer of a tree, read back, with tri and uvw where the tree keeps them."""
        out = []
        for k in range(self.abi.raytree_info(t)["n_layers"]):
            lay = self.abi.raytree_read_layer(t, k)
            if self.abi.raytree_keeps_tri(t):
                lay["tri"] = self.abi.raytree_read_tri(t, k)
            if self.abi.raytree_keeps_uvw(t):
                lay["uvw"] = self.abi.raytree_read_uvw(t, k)
            out.append(lay)
        return out


@pytest.fixture
def make():
    made = []

    def _make(flat, setup, **kw):
        made.append(Scene(flat, setup, **kw))
        return made[-1]
    yield _make
    for s in made:
        s.close()


@pytest.fixture(scope="module")
def flat_two():
    return M.MythTracer(rr.TWO_WAY).flatten()


@pytest.fixture(scope="module")
def flat_tiny():
    return te.build_tiny(M.MythTracer()).flatten()


@pytest.fixture(scope="module")
def orc_two():
    orc = orclib.OracleScene(rr.TWO_WAY)
    orc.set_lights(LIGHTS)
    return orc


def normal_case(name, flat, orc_a):
    """(the edit, flat's tri_normal with it, the oracle BUILT with it)"""
    edit = va.two_way_edit(name, orc_a)
    orc = va.oracle_with(orc_a, normals=edit)
    orc.set_lights(LIGHTS)
    return edit, va.replaced(flat, "tri_normal", edit), orc


def uvw_case(name, flat):
    edit = va.UVW_EDITS[name]()
    orc = va.build_tiny(orclib.OracleScene(), uvw=edit)
    orc.finalize()
    orc.set_lights(te.TINY_LIGHTS)
    return edit, va.replaced(flat, "tri_uvw", edit), orc


def stream_indices(flat, edit):
    """the edited triangles in node-stream numbering (the tri plane's)"""
    return [s for s, add in enumerate(flat["tri_id"]) if int(add) in edit]


def differing(a, b, what):
    n = int((a != b).any(axis=-1).sum())
    print("%s: %d of %d pixels differ" % (what, n, a.shape[0] * a.shape[1]))
    return n


def planes_differing(got, want, what):
    """Two trees as Scene.planes returns them: the number of (layer, plane) pairs that differ in a bit."""
    assert len(got) == len(want), (what, len(got), len(want))
    bad = 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w), what
        for name in g:
            if not ru.same_plane(g[name], w[name]):
                print("%s: layer %d plane %s differs" % (what, k, name))
                bad += 1
    print("%s: %d layers, rays %s, %d planes differ" % (what, len(got), [len(g["coef"]) for g in got], bad))
    return bad


def same_info(abi, t, tf, what):
    got, want = abi.raytree_info(t), abi.raytree_info(tf)
    for key in INFO_KEYS:
        assert got[key] == want[key], (what, key, got[key], want[key])
    return got


def refused(abi, fn, t, code, match):
    """An update (fn = "update") or regrow of `t` refuses with `code` and a message matching `match`."""
    st = binding.mt_stats()
    if fn == "update":
        rc = abi.lib.mt_raytree_update_materials(t, binding.C.addressof(st))
    else:
        info = binding.mt_raytree_regrow_info()
        rc = abi.lib.mt_raytree_regrow_materials(t, binding.C.addressof(info), binding.C.addressof(st))
    text = abi.last_error()
    print("%s refused (%d): %s" % (fn, rc, text))
    assert rc == code and re.search(match, text), (rc, text)
    return text


def assert_stale(s, t):
    with pytest.raises(RuntimeError, match=STALE):
        s.abi.raytree_shade(t, s.setup["lights"])
    with pytest.raises(RuntimeError, match=STALE):
        s.abi.raytree_update_lights(t, [0])


# ---- 1. the scene contract

def scene_contract(name, which, flat, B, orc, setup, make, chunks, expect_frame_change=True):
    key = KEY[which]
    A = np.array(flat[key], dtype=np.float64).reshape(-1, 9)
    w, h, depth, lights = setup["w"], setup["h"], setup["depth"], setup["lights"]
    s, s2 = make(flat, setup), make(flat, setup)
    fresh, fresh2 = make(va.built(flat, **{key: B}), setup), make(va.built(flat, **{key: B}), setup)
    abi = s.abi
    assert ru.same_plane(s.get(which), A)
    frame_a = s.frame()  # (a frame under A first: the cost history the frames under B are scheduled by is A's)
    t_before = s.tree(depth=2)
    s.set(which, B)
    s2.set(which, B)
    assert ru.same_plane(s.get(which), B) and ru.same_plane(fresh.get(which), B), "the getters' round trip"
    other = "uvw" if which == "normal" else "normal"
    assert ru.same_plane(s.get(other), np.array(flat[KEY[other]], dtype=np.float64).reshape(-1, 9))
    assert_stale(s, t_before)
    s.destroy(t_before)
    # a no-change set leaves the generations alone: a tree made now stays fresh across it
    t_now = s.tree(depth=2)
    s.set(which, B)
    shaded = abi.raytree_shade(t_now, lights)["rgb"]
    assert differing(shaded, s.frame(depth=2), name + ": a tree across a no-change set") == 0
    changed = differing(s.frame(), frame_a, name + ": B vs A")
    assert (changed > 0) == expect_frame_change
    oracle_frames = {}
    for engine in (1, 2, 3, 0):
        for x in (s, fresh):
            abi.set_engine(x.h, engine)
        for chunk in chunks:
            for d in (0, depth):
                what = "%s engine %d %s d=%d" % (name, engine, "chunk" if chunk else "frame", d)
                got = s.frame(chunk=chunk, depth=d)
                assert differing(got, fresh.frame(chunk=chunk, depth=d), what + " vs a built scene") == 0
                if (chunk, d) not in oracle_frames:
                    oracle_frames[chunk, d] = orc.render(setup["cam"], w, h, chunk=chunk, max_level=d)["rgb"]
                assert differing(got, oracle_frames[chunk, d], what + " vs the oracle") == 0
    # engine 1, the lean kernel and its redo launch: the second frame of one geometry
    for x in (s, fresh):
        abi.set_engine(x.h, 1)
        abi.set_tuning(x.h, "LEAN_KERNEL", 2.0)  # (2: also with pixels whose primary ray has a zero component)
    for i in range(2):
        got, want = s.frame(), fresh.frame()
        info = abi.lean_info(s.h)
        print("%s: engine 1 frame %d, lean info %s" % (name, i, info))
        assert differing(got, want, "%s lean frame %d vs a built scene" % (name, i)) == 0
        assert differing(got, oracle_frames[None, depth], "%s lean frame %d vs the oracle" % (name, i)) == 0
    if setup is TWO_WAY:
        assert info["lean"] == 1
    for x in (s, fresh):
        abi.set_engine(x.h, 0)
    sens, sens2 = binding.sensor(setup["cam"], w, h), binding.sensor(setup["cam"], 2 * w, 2 * h)
    for chunk in chunks:
        got = abi.render_chunk_ss(s.h, sens2, w, h, 2, chunk=chunk)["rgb"]
        assert differing(got, abi.render_chunk_ss(fresh.h, sens2, w, h, 2, chunk=chunk)["rgb"], "%s ss=2 %s" % (name, chunk)) == 0
        got = abi.render_chunk_adaptive(s.h, sens, sens2, w, h, 2, 16, chunk=chunk)
        want = abi.render_chunk_adaptive(fresh.h, sens, sens2, w, h, 2, 16, chunk=chunk)
        assert differing(got["rgb"], want["rgb"], "%s adaptive %s" % (name, chunk)) == 0
        gb, gbf = abi.render_gbuffer(s.h, sens, w, h, chunk=chunk), abi.render_gbuffer(fresh.h, sens, w, h, chunk=chunk)
        for plane in binding.GBUFFER_PLANES:
            assert ru.same_plane(gb[plane], gbf[plane]), (name, chunk, plane)
        lb = abi.render_lightbuffer(s.h, sens, w, h, len(lights), chunk=chunk)
        lbf = abi.render_lightbuffer(fresh.h, sens, w, h, len(lights), chunk=chunk)
        assert ru.same_plane(lb["power"], lbf["power"]) and np.array_equal(lb["in_shadow"], lbf["in_shadow"]), (name, chunk)
    # the G-buffer planes the edit moves: the uvw plane alone where no albedo depends on it
    gb, gba = abi.render_gbuffer(s.h, sens, w, h), abi.render_gbuffer(make(flat, setup).h, sens, w, h)
    moved = [p for p in binding.GBUFFER_PLANES if not ru.same_plane(gb[p], gba[p])]
    print("%s: G-buffer planes that moved: %s" % (name, moved))
    assert set(moved) <= ({"normal"} if which == "normal" else {"uvw", "albedo"})
    if not expect_frame_change:
        assert moved == ["uvw"]
    rays, _ = rr.layer0_rays(setup["cam"], w, h)
    rays = np.ascontiguousarray(rays[(np.arange(130) * 11 + 7) % len(rays)])
    traced, tracedf = abi.trace_rays(s.h, rays), abi.trace_rays(fresh.h, rays)
    assert ru.same_plane(traced["color"], tracedf["color"]) and np.array_equal(traced["rgb"], tracedf["rgb"])
    # two replicas that share a device
    multi = abi.render_frame_multi([s.h, s2.h], sens, w, h, tile_w=32, tile_h=32, max_depth=depth)["rgb"]
    multif = abi.render_frame_multi([fresh.h, fresh2.h], sens, w, h, tile_w=32, tile_h=32, max_depth=depth)["rgb"]
    assert differing(multi, multif, name + " two replicas vs built scenes") == 0
    assert differing(multi, oracle_frames[None, depth], name + " two replicas vs the oracle") == 0
    # a tree made after the set, in all four switch combinations
    for tri, uvw in ((False, False), (True, False), (False, True), (True, True)):
        for x in (s, fresh):
            abi.set_raytree_tri(x.h, tri)
            abi.set_raytree_uvw(x.h, uvw)
        t, tf = s.tree(), fresh.tree()
        assert planes_differing(s.planes(t), fresh.planes(tf), "%s tree (tri %d, uvw %d) vs a built scene's" % (name, tri, uvw)) == 0
        same_info(abi, t, tf, name)
    # and back
    s.set(which, A)
    assert ru.same_plane(s.get(which), A)
    assert differing(s.frame(), frame_a, name + ": A -> B -> A") == 0


@pytest.mark.parametrize("name", list(va.NORMAL_EDITS))
def test_scene_contract_normals(name, flat_two, orc_two, make):
    edit, B, orc = normal_case(name, flat_two, orc_two)
    scene_contract(name, "normal", flat_two, B, orc, TWO_WAY, make, (None, OFF_GRID))


@pytest.mark.parametrize("name", list(va.UVW_EDITS))
def test_scene_contract_uvw(name, flat_tiny, make):
    edit, B, orc = uvw_case(name, flat_tiny)
    scene_contract(name, "uvw", flat_tiny, B, orc, TINY, make, (None, (5, 3, 31, 22)), expect_frame_change=name not in va.UVW_ONLY)


def test_argument_checks_in_order_and_generations(flat_two, orc_two, make):
    s = make(flat_two, TWO_WAY, tri=True)
    abi = s.abi
    n = s.n_tris
    A = np.array(flat_two["tri_normal"], dtype=np.float64).reshape(-1, 9)
    frame = s.frame()
    for fn, what in ((abi.lib.mt_scene_set_triangle_normals, "normal"), (abi.lib.mt_scene_get_triangle_normals, "normal"),
                     (abi.lib.mt_scene_set_triangle_uvw, "uvw"), (abi.lib.mt_scene_get_triangle_uvw, "uvw")):
        for k in (n - 1, n + 1, 0, -1):  # the count before the array
            for p in (A.ctypes.data, None):
                assert fn(s.h, p, k) == MT_ERR_ARG
                assert abi.last_error() == "%d triangles for a scene made with %d" % (k, n)
        assert fn(s.h, None, n) == MT_ERR_ARG and abi.last_error() == "the triangle %s array is NULL" % what
    assert ru.same_plane(s.get("normal"), A)
    assert differing(s.frame(), frame, "after the refusals") == 0
    # a set that changes nothing bumps nothing: the tree stays fresh; -0.0 for 0.0 is a change, by the bits
    t = s.tree(depth=1)
    s.set("normal", A)
    s.set("uvw", flat_two["tri_uvw"])
    abi.raytree_shade(t, LIGHTS)
    assert abi.raytree_update_materials(t)["rays_shadow"] == 0
    B = A.copy()
    zero = np.nonzero(B == 0.0)
    assert len(zero[0]), "the scene has no zero component to flip"
    B[zero[0][0], zero[1][0]] = -0.0
    s.set("normal", B)
    assert_stale(s, t)
    assert np.signbit(s.get("normal")[zero[0][0], zero[1][0]])
    abi.raytree_regrow(t)
    print("the -0.0 edit:", abi.raytree_attr_info(t))
    abi.raytree_shade(t, LIGHTS)
    # values are not checked: NaN normals are legal input
    s.set("normal", np.full_like(A, np.nan))
    assert np.isnan(s.get("normal")).all()
    s.frame(depth=0)


# ---- 2. the tree contract

def take(abi, t, restated_blocked, what):
    """update, or -- where the restatement says the update refuses -- the refusal with the tree untouched and stale,
    then the regrow.  Returns the stats of the call that succeeded."""
    if restated_blocked:
        return abi.raytree_regrow(t)
    out = abi.raytree_update_materials(t)
    print("%s: update %s" % (what, {k: out[k] for k in ("rays_primary", "rays_secondary", "rays_shadow")}))
    return out


@pytest.mark.parametrize("chunk", [False, True])
@pytest.mark.parametrize("name", list(va.NORMAL_EDITS))
def test_tree_contract_normals(name, chunk, flat_two, orc_two, make):
    edit, B, orc = normal_case(name, flat_two, orc_two)
    A = np.array(flat_two["tri_normal"], dtype=np.float64).reshape(-1, 9)
    row = va.ROWS[name][chunk]
    ch = OFF_GRID if chunk else None
    changed = stream_indices(flat_two, edit)
    for uvw in (False, True):
        what = "%s %s uvw %d" % (name, "chunk" if chunk else "frame", uvw)
        s, fresh = make(flat_two, TWO_WAY, tri=True, uvw=uvw), make(va.built(flat_two, tri_normal=B), TWO_WAY, tri=True, uvw=uvw)
        abi = s.abi
        t = s.tree(chunk=ch)
        original = s.planes(t)
        s.set("normal", B)
        assert_stale(s, t)
        m = va.match(original, fresh.planes(fresh.tree(chunk=ch)), changed)
        assert m["blocked"] == row["blocked"] and m["traced"] == row["traced"], (m["blocked"], m["traced"])
        if row["blocked"]:
            text = refused(abi, "update", t, MT_ERR_UNSUPPORTED, "the new normals move reflected rays")
            assert ("%d rays on edited triangles" % row["blocked"]) in text
            assert planes_differing(s.planes(t), original, what + ": after the refusal") == 0
            assert_stale(s, t)
        out = take(abi, t, row["blocked"], what)
        tf = fresh.tree(chunk=ch)
        assert planes_differing(s.planes(t), fresh.planes(tf), what + " vs a fresh tree on the built scene") == 0
        info = same_info(abi, t, tf, what)
        assert info["n_rays"][:info["n_layers"]] == row["n_rays"]
        assert differing(abi.raytree_shade(t, LIGHTS)["rgb"], fresh.frame(chunk=ch), what + ": shaded") == 0
        attr = abi.raytree_attr_info(t)
        print("%s: attr info %s, restated %s" % (what, attr, {k: m[k] for k in ("renormaled", "respawned")}))
        assert attr == dict(renormaled=row["renormaled"], reuvwed=0, respawned=row["respawned"])
        assert out["rays_primary"] == 0 and out["rays_secondary"] == sum(row["traced"])
        if row["blocked"]:
            assert out["regrown"] == 1 and out["traced"] == row["traced"]
        else:
            assert out["rays_shadow"] == 0
        # back to A, bit for bit
        s.set("normal", A)
        take(abi, t, row["blocked"], what + ", back")
        assert planes_differing(s.planes(t), original, what + ": back vs the original") == 0
        assert abi.raytree_info(t)["bytes"] == abi.raytree_info(s.tree(chunk=ch))["bytes"]


@pytest.mark.parametrize("name", list(va.UVW_EDITS))
def test_tree_contract_uvw(name, flat_tiny, make):
    edit, B, orc = uvw_case(name, flat_tiny)
    A = np.array(flat_tiny["tri_uvw"], dtype=np.float64).reshape(-1, 9)
    row = va.UVW_ROWS[name]
    changed = stream_indices(flat_tiny, edit)
    for uvw in (False, True):
        for fn in ("update", "regrow"):
            what = "%s uvw %d %s" % (name, uvw, fn)
            s, fresh = make(flat_tiny, TINY, tri=True, uvw=uvw), make(va.built(flat_tiny, tri_uvw=B), TINY, tri=True, uvw=uvw)
            abi = s.abi
            t = s.tree()
            original = s.planes(t)
            assert [int(va.dirty(l["tri"], changed).sum()) for l in original] == row["dirty"]
            s.set("uvw", B)
            assert_stale(s, t)
            out = abi.raytree_update_materials(t) if fn == "update" else abi.raytree_regrow(t)
            tf = fresh.tree()
            got = s.planes(t)
            assert planes_differing(got, fresh.planes(tf), what + " vs a fresh tree on the built scene") == 0
            info = same_info(abi, t, tf, what)
            assert info["n_rays"][:info["n_layers"]] == va.TINY_A
            moved = [int((~(np.ascontiguousarray(g["albedo"]).view(np.uint64) == np.ascontiguousarray(o["albedo"]).view(np.uint64)).all(axis=1)).sum())
                     for g, o in zip(got, original)]
            assert moved == row["albedo"], moved
            assert differing(abi.raytree_shade(t, te.TINY_LIGHTS)["rgb"], fresh.frame(), what + ": shaded") == 0
            assert differing(abi.raytree_shade(t, te.TINY_LIGHTS)["rgb"], orc.render(te.TINY_CAMERA, TW, TH, max_level=te.TINY_DEPTH)["rgb"],
                             what + ": shaded vs the oracle") == 0
            attr = abi.raytree_attr_info(t)
            print("%s: attr info %s" % (what, attr))
            assert attr == dict(renormaled=0, reuvwed=sum(row["dirty"]), respawned=0)
            assert out["rays_primary"] == 0 and out["rays_secondary"] == 0 and out["rays_shadow"] == 0
            if fn == "regrow":
                assert out["regrown"] == 0
            s.set("uvw", A)
            abi.raytree_update_materials(t)
            assert planes_differing(s.planes(t), original, what + ": back vs the original") == 0


# ---- 3. refusals

def test_a_tree_without_tri_refuses_and_the_right_switch_succeeds(flat_two, flat_tiny, orc_two, make):
    edit, B, _ = normal_case("mirror tilt", flat_two, orc_two)
    first = min(stream_indices(flat_two, edit))
    for uvw in (False, True):
        s = make(flat_two, TWO_WAY, tri=False, uvw=uvw)
        abi = s.abi
        t = s.tree()
        original = s.planes(t)
        s.set("normal", B)
        for fn in ("update", "regrow"):
            text = refused(abi, fn, t, MT_ERR_UNSUPPORTED, "the ray tree keeps no tri")
            assert text.startswith("the normal of %d triangles was set after the ray tree was made, the first is triangle %d" % (len(edit), first))
            assert planes_differing(s.planes(t), original, "after the refusal") == 0
            assert_stale(s, t)
        # the right switch: a tree made now keeps tri, is fresh, and takes the way back
        abi.set_raytree_tri(s.h, True)
        t2 = s.tree()
        abi.raytree_shade(t2, LIGHTS)
        s.set("normal", flat_two["tri_normal"])
        abi.raytree_regrow(t2)
        assert abi.raytree_attr_info(t2)["respawned"] > 0
        assert differing(abi.raytree_shade(t2, LIGHTS)["rgb"], s.frame(), "the tree with tri, back at A") == 0
    # the uvw attribute
    edit, B, _ = uvw_case("floor x2", flat_tiny)
    s = make(flat_tiny, TINY, tri=False, uvw=True)
    t = s.tree()
    s.set("uvw", B)
    text = refused(abi, "update", t, MT_ERR_UNSUPPORTED, "the ray tree keeps no tri")
    assert text.startswith("the uvw of 2 triangles was set")
    assert_stale(s, t)


def test_light_count_mismatch(flat_two, orc_two, make):
    edit, B, _ = normal_case("mirror tilt", flat_two, orc_two)
    s, fresh = make(flat_two, TWO_WAY, tri=True), make(va.built(flat_two, tri_normal=B), TWO_WAY, tri=True)
    abi = s.abi
    t = s.tree()
    original = s.planes(t)
    s.set("normal", B)
    abi.set_lights(s.h, LIGHTS[:1])
    text = refused(abi, "regrow", t, MT_ERR_ARG, "the scene has 1 lights, the ray tree was made with %d" % len(LIGHTS))
    assert planes_differing(s.planes(t), original, "after the refusal") == 0
    with pytest.raises(RuntimeError, match=STALE):
        abi.raytree_shade(t, LIGHTS)
    abi.set_lights(s.h, LIGHTS)
    assert_stale(s, t)
    abi.raytree_regrow(t)
    assert planes_differing(s.planes(t), fresh.planes(fresh.tree()), "after the lights are back") == 0


# ---- 4. shapes and combinations

@pytest.mark.parametrize("chunk", [(5, 3, 63, 37), (5, 3, 64, 37), (5, 3, 65, 37), (40, 30, 1, 1), (0, 0, 20, 3)])
def test_chunk_shapes(chunk, flat_two, orc_two, make):
    """Chunks 63, 64 and 65 wide, one pixel, and the frame's top-left corner (which only misses or only sees a wall)."""
    for name in ("mirror tilt", "blue smooth"):
        edit, B, _ = normal_case(name, flat_two, orc_two)
        s, fresh = make(flat_two, TWO_WAY, tri=True), make(va.built(flat_two, tri_normal=B), TWO_WAY, tri=True)
        t = s.tree(chunk=chunk)
        s.set("normal", B)
        out = s.abi.raytree_regrow(t)
        tf = fresh.tree(chunk=chunk)
        what = "%s chunk %s" % (name, chunk)
        assert planes_differing(s.planes(t), fresh.planes(tf), what) == 0
        same_info(s.abi, t, tf, what)
        print(what, "traced", out["traced"], s.abi.raytree_attr_info(t))
        assert differing(s.abi.raytree_shade(t, LIGHTS)["rgb"], fresh.frame(chunk=chunk), what + ": shaded") == 0


def test_a_chunk_that_only_misses(flat_two, orc_two, make):
    edit, B, _ = normal_case("mirror tilt", flat_two, orc_two)
    s, fresh = make(flat_two, TWO_WAY, tri=True), make(va.built(flat_two, tri_normal=B), TWO_WAY, tri=True)
    cam = (200.0, 110.0, 10.0, 0.0, 180.0, 0.0, 100.0)  # (turned away from the room)
    setup = dict(TWO_WAY, cam=cam)
    s.setup = fresh.setup = setup
    t = s.tree(chunk=(3, 2, 17, 9))
    assert all((l["tri"] < 0).all() for l in s.planes(t)), "the chunk sees something"
    s.set("normal", B)
    for fn in (s.abi.raytree_update_materials, s.abi.raytree_regrow):
        fn(t)
    assert s.abi.raytree_attr_info(t) == dict(renormaled=0, reuvwed=0, respawned=0)
    assert planes_differing(s.planes(t), fresh.planes(fresh.tree(chunk=(3, 2, 17, 9))), "a chunk of misses") == 0


def test_a_ray_list_tree(flat_two, orc_two, make):
    rays = ar.list_rays()
    assert len(rays) == 130
    for name in ("pane tilt", "blue smooth"):
        edit, B, _ = normal_case(name, flat_two, orc_two)
        s, fresh = make(flat_two, TWO_WAY, tri=True, uvw=True), make(va.built(flat_two, tri_normal=B), TWO_WAY, tri=True, uvw=True)
        t = s.tree_rays(rays)
        original = s.planes(t)
        s.set("normal", B)
        out = s.abi.raytree_regrow(t)
        tf = fresh.tree_rays(rays)
        want = fresh.planes(tf)
        m = va.match(original, want, stream_indices(flat_two, edit))
        print(name, "list tree: traced", out["traced"], s.abi.raytree_attr_info(t), "restated", m["traced"], m["respawned"])
        assert planes_differing(s.planes(t), want, name + " list tree") == 0
        same_info(s.abi, t, tf, name)
        assert s.abi.raytree_attr_info(t) == dict(renormaled=m["renormaled"], reuvwed=0, respawned=m["respawned"])
        assert out["traced"] == m["traced"][:len(out["traced"])]
        a, b = s.abi.raytree_shade_colors(t, LIGHTS), fresh.abi.raytree_shade_colors(tf, LIGHTS)
        assert ru.same_plane(a["color"], b["color"])


@pytest.mark.parametrize("layout", [0, 1])
def test_deep_layout(layout, scenes, make):
    """An octree of 16 levels, both settings of MT_TUNE_DEEP_LAYOUT: the DEEP instantiations of raytree_trace_kernel over
    the respawned reflected rays after the reflective materials' normals were tilted."""
    flat = M.MythTracer(scenes["loft"]).flatten()
    assert flat["tree_depth"] >= 16
    setup = dict(cam=scenegen.ROOM_CAMERA, w=32, h=18, depth=5, lights=LIGHTS)
    refl = [i for i, m in enumerate(flat["materials"]) if m["values"][10] > 0.0]
    A = np.array(flat["tri_normal"], dtype=np.float64).reshape(-1, 3, 3)
    B = A.copy()
    sel = np.isin(np.asarray(flat["tri_material"]), refl)
    B[sel] = B[sel] + np.array([0.03, 0.02, 0.01])
    B[sel] /= np.sqrt((B[sel] ** 2).sum(axis=-1, keepdims=True))
    s, fresh = make(flat, setup, tri=True), make(va.built(flat, tri_normal=B), setup, tri=True)
    for x in (s, fresh):
        x.abi.set_tuning(x.h, "DEEP_LAYOUT", float(layout))
    t = s.tree()
    original = s.planes(t)
    s.set("normal", B)
    out = s.abi.raytree_regrow(t)
    attr = s.abi.raytree_attr_info(t)
    print("loft, layout %d: traced %s, %s" % (layout, out["traced"], attr))
    assert out["regrown"] == 1 and sum(out["traced"]) > 0 and attr["respawned"] > 0
    assert planes_differing(s.planes(t), fresh.planes(fresh.tree()), "loft, layout %d" % layout) == 0
    assert differing(s.abi.raytree_shade(t, LIGHTS)["rgb"], fresh.frame(), "loft, layout %d: shaded" % layout) == 0
    s.set("normal", A)
    s.abi.raytree_regrow(t)
    assert planes_differing(s.planes(t), original, "loft: back vs the original") == 0


def test_one_session_of_everything(flat_tiny, make):
    """A normal edit, a uvw edit, a texture replacement, a constants edit and a moved light, taken in a single update
    (the mirror keeps its normals: no reflected ray moves) and in a single regrow (the mirror's are tilted too)."""
    texs = te.tiny_textures()
    new_tex = te.replacements(texs[0])["2x2"]
    uvw_edit = va.UVW_EDITS["floor x2"]()
    lights = [list(l) for l in te.TINY_LIGHTS]
    lights[1][0:3] = (2.0, 7.0, -2.0)
    for mirror in (False, True):
        A = np.array(flat_tiny["tri_normal"], dtype=np.float64).reshape(-1, 3, 3)
        Bn = A.copy()
        tilt = [s for s, add in enumerate(flat_tiny["tri_id"]) if int(add) in ((6, 7, 4, 5) if mirror else (6, 7))]
        Bn[tilt] = Bn[tilt] + np.array([0.02, 0.03, 0.01])
        Bn[tilt] /= np.sqrt((Bn[tilt] ** 2).sum(axis=-1, keepdims=True))
        Bu = va.replaced(flat_tiny, "tri_uvw", uvw_edit)
        mats = [dict(m, values=list(m["values"])) for m in flat_tiny["materials"]]
        mats[te.MATTE]["values"][0:3] = (0.5, 0.25, 0.125)
        built = va.built(flat_tiny, tri_normal=Bn, tri_uvw=Bu)
        built["materials"] = mats
        built["textures"] = [dict(texels=new_tex)] + list(flat_tiny["textures"])[1:]
        s = make(flat_tiny, TINY, tri=True, uvw=True)
        fresh = make(built, dict(TINY, lights=lights), tri=True, uvw=True)
        abi = s.abi
        t = s.tree()
        s.set("normal", Bn)
        s.set("uvw", Bu)
        abi.set_texture(s.h, 0, new_tex)
        abi.set_materials(s.h, mats)
        abi.set_lights(s.h, lights)
        if mirror:
            refused(abi, "update", t, MT_ERR_UNSUPPORTED, "the new normals move reflected rays")
            out = abi.raytree_regrow(t)
            assert out["regrown"] == 1 and sum(out["traced"]) > 0
        else:
            abi.raytree_update_materials(t)
        abi.raytree_update_lights(t, [1])
        attr = abi.raytree_attr_info(t)
        print("session (mirror %d): %s" % (mirror, attr))
        assert attr["renormaled"] > 0 and attr["reuvwed"] > 0 and (attr["respawned"] > 0) == mirror
        assert planes_differing(s.planes(t), fresh.planes(fresh.tree()), "session (mirror %d)" % mirror) == 0
        assert differing(abi.raytree_shade(t, lights)["rgb"], fresh.frame(), "session (mirror %d): shaded" % mirror) == 0


def test_two_trees_with_different_snapshots(flat_two, orc_two, make):
    _, B1, _ = normal_case("blue smooth", flat_two, orc_two)
    edit2, _, _ = normal_case("pane tilt", flat_two, orc_two)
    B2 = B1.copy()
    for s_, add in enumerate(flat_two["tri_id"]):
        if int(add) in edit2:
            B2[s_] = edit2[int(add)].reshape(9)
    s, fresh = make(flat_two, TWO_WAY, tri=True), make(va.built(flat_two, tri_normal=B2), TWO_WAY, tri=True)
    abi = s.abi
    t1 = s.tree()
    s.set("normal", B1)
    t2 = s.tree()  # (its snapshot holds the first edit)
    s.set("normal", B2)
    want = fresh.planes(fresh.tree())
    abi.raytree_regrow(t2)
    a2 = abi.raytree_attr_info(t2)
    abi.raytree_regrow(t1)
    a1 = abi.raytree_attr_info(t1)
    print("snapshots: the older tree %s, the newer %s" % (a1, a2))
    assert a1["renormaled"] > a2["renormaled"] > 0 and a1["respawned"] == a2["respawned"] > 0
    assert planes_differing(s.planes(t1), want, "the older tree") == 0
    assert planes_differing(s.planes(t2), want, "the newer tree") == 0
    # both fresh now: a further call does nothing
    assert abi.raytree_update_materials(t1)["rays_secondary"] == 0
    assert abi.raytree_attr_info(t1) == dict(renormaled=0, reuvwed=0, respawned=0)


def test_frame_kernels_are_untouched_by_the_edit_calls(scenes, make):
    """A depth-5 frame before and after a set of the SAME arrays and a tree update is byte-identical, and the calls add
    no entry to mt_scene_kernel_times."""
    flat = M.MythTracer(scenes["room"]).flatten()
    setup = dict(cam=scenegen.ROOM_CAMERA, w=480, h=270, depth=5, lights=LIGHTS)
    s = make(flat, setup, tri=True)
    s.abi.set_engine(s.h, 1)
    t = s.tree()
    s.abi.kernel_times(s.h)
    f1 = s.frame()
    s.set("normal", flat["tri_normal"])
    s.set("uvw", flat["tri_uvw"])
    s.abi.raytree_update_materials(t)
    f2 = s.frame()
    assert np.array_equal(f1, f2)
    pm, rm = s.abi.kernel_times(s.h)
    print("primary_ms", pm, "render_ms", rm)
    assert len(pm) == 2, pm


# ---- 5. the facade and Python

def test_facade_round_trip(flat_two, orc_two):
    edit, B, orc = normal_case("pane tilt", flat_two, orc_two)
    m = M.MythTracer(rr.TWO_WAY)
    m.set_lights(LIGHTS)
    m.set_max_level(va.DEPTH)
    m.set_raytree_keep_triangles(True)
    frame_a = m.render(CAM, W, H)["rgb"]
    tree = m.raytree(CAM, W, H)
    m.set_triangle_normals(sorted(edit), [edit[i] for i in sorted(edit)])
    m.update_triangle_attributes()
    frame_b = m.render(CAM, W, H)["rgb"]
    assert differing(frame_b, orc.render(CAM, W, H)["rgb"], "facade: UpdateTriangleAttributes vs the oracle") == 0
    assert differing(frame_b, frame_a, "facade: B vs A (expected to differ)") > 0
    with pytest.raises(RuntimeError, match=STALE):
        tree.shade()
    with pytest.raises(RuntimeError, match="the new normals move reflected rays"):
        tree.update_materials()
    tree.regrow()
    attr = tree.attr_info()
    print("facade:", attr)
    assert attr == dict(renormaled=va.ROWS["pane tilt"][False]["renormaled"], reuvwed=0, respawned=va.ROWS["pane tilt"][False]["respawned"])
    assert differing(tree.shade()["rgb"], frame_b, "facade: the regrown tree's frame") == 0
    assert ru.same_plane(M.hip_abi().get_triangle_normals(m.device_scene(), len(B)).reshape(-1, 9), B)
    tree.close()
