"""Triangles given another material in place, on a real MI355X (-m gpu): mt_scene_set_triangle_materials, the `tri` plane
of a ray tree (mt_scene_set_raytree_tri) and the reassignment mt_raytree_update_materials / mt_raytree_regrow_materials
take (include/mythtracer_hip.h; the kernels are in mythtracer_amd/csrc/mt_raytree.h).

The bar is identity, no tolerance.  The truth for an assignment always comes from a scene BUILT with it, never from the
edit call: for the kernel's planes mt_scene_create on the flat description with tri_material replaced
(assign_ref.built), for frames also the oracle on a variant .obj whose usemtl lines were rewritten
(assign_ref.variant_obj).  Trees are compared plane by plane and layer by layer, tri and uvw included where kept,
doubles as uint64 with NaN = NaN.  The reassignments and their ray counts are assign_ref's, which
tests/test_assign_cpu.py pins with the oracle alone.  Every test prints its counts.

rays_shadow: a call that traces no ray of the tree itself (mt_raytree_update_materials, and a regrow whose check pass
finds the shape intact) reports 0 exactly where the shadow-visible rule says "not visible"; a regrow that traces new
rays counts their shadow loops too, so there the figure is only printed.
"""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import assign_ref as ar  # noqa: E402
import lightbuffer_ref as lr  # noqa: E402
import orclib  # noqa: E402
import raytree_ref as rr  # noqa: E402
import raytree_update_ref as ru  # noqa: E402

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding, scenegen  # noqa: E402

W, H = ar.W, ar.H
OFF_GRID = ar.OFF_GRID
LIGHTS = ar.LIGHTS
CAM = ar.CAM
DEPTHS = ar.DEPTHS
MT_ERR_ARG, MT_ERR_UNSUPPORTED = -1, -3
STALE = "materials were edited after the ray tree was made"
INFO_KEYS = ("n_rays", "n_layers", "bytes", "n_lights", "chunk", "max_depth")
ALL_ROWS = dict(ar.ROWS, **ar.EXTRA)


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"


class Scene:
    def __init__(self, flat, tri=False, uvw=False, lights=LIGHTS):
        self.abi = M.hip_abi()
        self.flat = flat
        self.h = self.abi.scene_create(flat)
        self.trees = []
        self.abi.set_raytree_tri(self.h, tri)
        self.abi.set_raytree_uvw(self.h, uvw)
        self.abi.set_lights(self.h, lights)

    def close(self):
        for t in self.trees:
            self.abi.raytree_destroy(t)
        self.abi.scene_destroy(self.h)

    @property
    def n_tris(self):
        return len(self.flat["tri_material"])

    def assign(self, tri_material):
        self.abi.set_triangle_materials(self.h, tri_material)

    def assignment(self):
        return self.abi.get_triangle_materials(self.h, self.n_tris)

    def tree(self, cam=CAM, w=W, h=H, chunk=None, depth=5):
        t, stats = self.abi.raytree_create(self.h, binding.sensor(cam, w, h), w, h, chunk=chunk, max_depth=depth)
        self.trees.append(t)
        return t

    def tree_rays(self, rays, depth=5):
        t, stats = self.abi.raytree_create_rays(self.h, rays, max_depth=depth)
        self.trees.append(t)
        return t

    def destroy(self, t):
        self.trees.remove(t)
        self.abi.raytree_destroy(t)

    def frame(self, cam=CAM, w=W, h=H, chunk=None, depth=5):
        return self.abi.render_chunk(self.h, binding.sensor(cam, w, h), w, h, chunk=chunk, max_depth=depth)["rgb"]

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

    def _make(flat, **kw):
        made.append(Scene(flat, **kw))
        return made[-1]
    yield _make
    for s in made:
        s.close()


@pytest.fixture(scope="module")
def flat_a():
    return M.MythTracer(rr.TWO_WAY).flatten()


@pytest.fixture(scope="module")
def oracle_of(tmp_path_factory):
    """row name -> the oracle on the scene BUILT with that assignment (a variant .obj, or added triangle by triangle
    where no usemtl line spells it), the bench's lights set; None -> two_way as it is."""
    made = {}

    def get(name):
        if name not in made:
            if name is None:
                orc = orclib.OracleScene(rr.TWO_WAY)
            elif name in ar.ROWS:
                orc = orclib.OracleScene(ar.variant_obj(rr.TWO_WAY, ar.ROWS[name][0], str(tmp_path_factory.mktemp("variant"))))
            else:
                orc = ar.oracle_with(rr.TWO_WAY, ar.EXTRA[name][0])
            orc.set_lights(LIGHTS)
            made[name] = orc
        return made[name]
    return get


def differing(a, b, what):
    n = int((a != b).any(axis=-1).sum())
    print("%s: %d of %d pixels differ" % (what, n, a.shape[0] * a.shape[1]))
    return n


def planes_differing(got, want, what, skip=()):
    """Two trees as Scene.planes returns them: the number of (layer, plane) pairs that differ in a bit."""
    assert len(got) == len(want), (what, len(got), len(want))
    bad = 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert sorted(n for n in g if n not in skip) == sorted(n for n in w if n not in skip), what
        for name in g:
            if name not in skip and not ru.same_plane(g[name], w[name]):
                print("%s: layer %d plane %s differs" % (what, k, name))
                bad += 1
    print("%s: %d layers, rays %s, %d planes differ" % (what, len(got), [len(g["coef"]) for g in got], bad))
    return bad


def same_info(abi, t, tf, what):
    got, want = abi.raytree_info(t), abi.raytree_info(tf)
    for key in INFO_KEYS:
        assert got[key] == want[key], (what, key, got[key], want[key])
    return got


def same_shape(a, b):
    return [len(x["coef"]) for x in a] == [len(x["coef"]) for x in b] and all(
        np.array_equal(x[p], y[p]) for x, y in zip(a, b) for p in ("child_refl", "child_refr"))


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


def assert_stale(s, t, lights=LIGHTS):
    with pytest.raises(RuntimeError, match=STALE):
        s.abi.raytree_shade(t, lights)
    with pytest.raises(RuntimeError, match=STALE):
        s.abi.raytree_update_lights(t, [0])


def rule(flat, was, now, mats_was=None):
    return ar.shadow_visible(mats_was or ar.flat_values(flat), ar.flat_values(flat), ar.changed_pairs(was, now))


# ---- 1. the scene contract

@pytest.mark.parametrize("name", list(ALL_ROWS))
def test_scene_contract(name, flat_a, make, oracle_of):
    """After the set, every rendering and shading call gives what it gives on a scene BUILT with the assignment, and the
    frames what the oracle renders on the variant."""
    moves = ALL_ROWS[name][0]
    A = np.array(flat_a["tri_material"], dtype=np.int32)
    B = ar.reassigned(flat_a, rr.TWO_WAY, moves)
    orc = oracle_of(name)
    s, s2 = make(flat_a), make(flat_a)
    fresh, fresh2 = make(ar.built(flat_a, B)), make(ar.built(flat_a, B))
    abi = s.abi
    assert np.array_equal(s.assignment(), A)
    frame_a = s.frame()  # (a frame under A first: the cost history the frames under B are scheduled by is A's)
    t_before = s.tree(depth=2)
    s.assign(B)
    s2.assign(B)
    assert np.array_equal(s.assignment(), B) and np.array_equal(fresh.assignment(), B)
    assert_stale(s, t_before)
    s.destroy(t_before)
    # a no-op set leaves both generations alone: a tree made now stays fresh across it
    t_now = s.tree(depth=2)
    s.assign(B)
    shaded = abi.raytree_shade(t_now, LIGHTS)["rgb"]
    assert differing(shaded, s.frame(depth=2), name + ": a tree across a no-op set") == 0
    assert differing(s.frame(), frame_a, name + ": B vs A (expected to differ)") > 0
    oracle_frames = {}
    for engine in (1, 2, 3, 0):
        for x in (s, fresh):
            abi.set_engine(x.h, engine)
        for chunk in (None, OFF_GRID):
            for d in DEPTHS:
                what = "%s engine %d %s d=%d" % (name, engine, "chunk" if chunk else "frame", d)
                got = s.frame(chunk=chunk, depth=d)
                assert differing(got, fresh.frame(chunk=chunk, depth=d), what + " vs a built scene") == 0
                if (chunk, d) not in oracle_frames:
                    oracle_frames[chunk, d] = orc.render(CAM, W, H, chunk=chunk, max_level=d)["rgb"]
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
        assert differing(got, oracle_frames[None, 5], "%s lean frame %d vs the oracle" % (name, i)) == 0
    assert info["lean"] == 1
    for x in (s, fresh):
        abi.set_engine(x.h, 0)
    sens, sens2 = binding.sensor(CAM, W, H), binding.sensor(CAM, 2 * W, 2 * H)
    for chunk in (None, OFF_GRID):
        got = abi.render_chunk_ss(s.h, sens2, W, H, 2, chunk=chunk)["rgb"]
        assert differing(got, abi.render_chunk_ss(fresh.h, sens2, W, H, 2, chunk=chunk)["rgb"], "%s ss=2 %s" % (name, chunk)) == 0
        got = abi.render_chunk_adaptive(s.h, sens, sens2, W, H, 2, 16, chunk=chunk)
        want = abi.render_chunk_adaptive(fresh.h, sens, sens2, W, H, 2, 16, chunk=chunk)
        assert differing(got["rgb"], want["rgb"], "%s adaptive %s" % (name, chunk)) == 0
        assert np.array_equal(got["mask"], want["mask"])
        gb, gbf = abi.render_gbuffer(s.h, sens, W, H, chunk=chunk), abi.render_gbuffer(fresh.h, sens, W, H, chunk=chunk)
        for plane in binding.GBUFFER_PLANES:
            assert ru.same_plane(gb[plane], gbf[plane]), (name, chunk, plane)
        lb = abi.render_lightbuffer(s.h, sens, W, H, len(LIGHTS), chunk=chunk)
        lbf = abi.render_lightbuffer(fresh.h, sens, W, H, len(LIGHTS), chunk=chunk)
        assert ru.same_plane(lb["power"], lbf["power"]) and np.array_equal(lb["in_shadow"], lbf["in_shadow"]), (name, chunk)
    rays = ar.list_rays()
    hit, hitf = abi.intersect_rays(s.h, rays), abi.intersect_rays(fresh.h, rays)
    for key in ("tri", "line", "t", "point"):
        assert ru.same_plane(hit[key], hitf[key]), key
    traced, tracedf = abi.trace_rays(s.h, rays), abi.trace_rays(fresh.h, rays)
    assert ru.same_plane(traced["color"], tracedf["color"]) and np.array_equal(traced["rgb"], tracedf["rgb"])
    # two replicas that share a device
    multi = abi.render_frame_multi([s.h, s2.h], sens, W, H, tile_w=32, tile_h=32)["rgb"]
    multif = abi.render_frame_multi([fresh.h, fresh2.h], sens, W, H, tile_w=32, tile_h=32)["rgb"]
    assert differing(multi, multif, name + " two replicas vs built scenes") == 0
    assert differing(multi, oracle_frames[None, 5], name + " two replicas vs the oracle") == 0
    # a tree made after the set
    t, tf = s.tree(), fresh.tree()
    got = s.planes(t)
    assert planes_differing(got, fresh.planes(tf), name + " tree vs a built scene's") == 0
    assert [len(g["coef"]) for g in got] == ALL_ROWS[name][1]
    # and back
    s.assign(A)
    assert np.array_equal(s.assignment(), A)
    assert differing(s.frame(), frame_a, name + ": A -> B -> A") == 0


def test_set_triangle_materials_argument_checks_in_order(flat_a, make):
    s = make(flat_a)
    abi = s.abi
    n, n_mtl = s.n_tris, len(flat_a["materials"])
    A = np.array(flat_a["tri_material"], dtype=np.int32)
    frame = s.frame()
    for fn in (abi.lib.mt_scene_set_triangle_materials, abi.lib.mt_scene_get_triangle_materials):
        for k in (n - 1, n + 1, 0, -1):  # the count before the array
            for p in (A.ctypes.data, None):
                assert fn(s.h, p, k) == MT_ERR_ARG
                assert abi.last_error() == "%d triangles for a scene made with %d" % (k, n)
        assert fn(s.h, None, n) == MT_ERR_ARG and abi.last_error() == "the triangle material array is NULL"
    for at, bad in ((3, n_mtl), (0, -2), (n - 1, 1000)):
        B = A.copy()
        B[at] = bad
        B[(at + 1) % n] = (A[(at + 1) % n] + 1) % n_mtl  # (a valid change next to it must not get through either)
        with pytest.raises(RuntimeError, match=re.escape("triangle %d: material index %d outside -1..%d" % (at, bad, n_mtl - 1))):
            s.assign(B)
    with pytest.raises(RuntimeError, match="keep must be 0 or 1"):
        abi.check(abi.lib.mt_scene_set_raytree_tri(s.h, 2))
    assert np.array_equal(s.assignment(), A)
    assert differing(s.frame(), frame, "after the refusals") == 0


# ---- 2. the tri plane, with no reassignment at all

def test_the_tri_plane_and_the_four_switch_combinations(flat_a, make):
    s = make(flat_a)
    abi = s.abi
    tri_material = np.array(flat_a["tri_material"])
    sens = binding.sensor(CAM, W, H)
    rays = ar.list_rays()
    trace_off = abi.trace_rays(s.h, rays)
    for chunk in (None, OFF_GRID):
        abi.set_raytree_tri(s.h, False)
        abi.set_raytree_uvw(s.h, False)
        plain = s.tree(chunk=chunk)
        want, info0 = s.planes(plain), abi.raytree_info(plain)
        assert not abi.raytree_keeps_tri(plain)
        with pytest.raises(RuntimeError, match="the ray tree keeps no tri"):
            abi.raytree_read_tri(plain, 0)
        total = sum(info0["n_rays"])
        gb = abi.render_gbuffer(s.h, sens, W, H, chunk=chunk, channels=("prim",))["prim"].reshape(-1)
        for tri, uvw in ((True, False), (False, True), (True, True)):
            abi.set_raytree_tri(s.h, tri)
            abi.set_raytree_uvw(s.h, uvw)
            t = s.tree(chunk=chunk)
            info = abi.raytree_info(t)
            assert abi.raytree_keeps_tri(t) == tri and abi.raytree_keeps_uvw(t) == uvw
            assert info["n_rays"] == info0["n_rays"]
            print("tri %d uvw %d %s: bytes %d (plain %d), %d rays" % (tri, uvw, chunk, info["bytes"], info0["bytes"], total))
            assert info["bytes"] - info0["bytes"] == (4 * total if tri else 0) + (24 * total if uvw else 0)
            got = s.planes(t)
            assert planes_differing(got, want, "tri %d uvw %d vs the plain tree" % (tri, uvw), skip=("tri", "uvw")) == 0
            if tri:
                for k, lay in enumerate(got):
                    hit = lay["tri"] >= 0
                    assert np.array_equal(hit, ~np.isnan(lay["point"][:, 0])), k
                    assert lay["tri"].max() < len(tri_material) and lay["tri"].min() >= -1
                    assert np.array_equal(lay["material"][hit], tri_material[lay["tri"][hit]]), k
                    assert (lay["material"][~hit] == -1).all() and (lay["tri"][~hit] == -1).all()
                    assert np.array_equal(lay["tri"], abi.intersect_rays(s.h, lay["ray"])["tri"]), k
                lay = got[0]
                prim = np.where(lay["tri"] >= 0, flat_a["tri_id"][np.maximum(lay["tri"], 0)], -1)
                assert np.array_equal(prim, gb[lay["pixel"]])
            s.destroy(t)
        s.destroy(plain)
    # a ray-list tree (the last wave is partial) and the tree inside mt_trace_rays
    abi.set_raytree_tri(s.h, False)
    abi.set_raytree_uvw(s.h, False)
    plain = s.tree_rays(rays)
    abi.set_raytree_tri(s.h, True)
    t = s.tree_rays(rays)
    got = s.planes(t)
    assert planes_differing(got, s.planes(plain), "a ray-list tree with tri vs without", skip=("tri",)) == 0
    assert abi.raytree_info(t)["bytes"] - abi.raytree_info(plain)["bytes"] == 4 * sum(abi.raytree_info(t)["n_rays"])
    for k, lay in enumerate(got):
        assert np.array_equal(lay["tri"], abi.intersect_rays(s.h, lay["ray"])["tri"]), k
    trace_on = abi.trace_rays(s.h, rays)
    assert ru.same_plane(trace_on["color"], trace_off["color"]) and np.array_equal(trace_on["rgb"], trace_off["rgb"])
    # the device form of the list
    import torch
    d = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    td, _ = abi.raytree_create_rays(s.h, d, max_depth=5, device=True)
    s.trees.append(td)
    assert planes_differing(s.planes(td), got, "the device form's tree") == 0
    # the read's checks, in order
    assert abi.lib.mt_raytree_read_tri(t, 99, None) == MT_ERR_ARG and "layer 99 outside" in abi.last_error()
    assert abi.lib.mt_raytree_read_tri(t, 0, None) == MT_ERR_ARG and abi.last_error() == "the tri output is NULL"
    assert abi.lib.mt_raytree_read_tri(plain, 0, None) == MT_ERR_ARG and abi.last_error() == "the tri output is NULL"


# ---- 3. the tree contract

def tree_contract(name, s, fresh, A, B, make_tree, what, shadow_rule, depth=5, moved_light=None):
    """Two trees of `s` under A -- one for the update, one for the regrow --, the set, and both calls held to a fresh
    tree of `fresh` (BUILT with B).  make_tree(scene, depth) -> tree.  Returns the regrow's dict."""
    abi = s.abi
    s.assign(A)
    tu, tr = make_tree(s, depth), make_tree(s, depth)
    original = s.planes(tu)
    tf = make_tree(fresh, depth)
    want = fresh.planes(tf)
    keeps = same_shape(original, want)
    s.assign(B)
    assert_stale(s, tu)
    # mt_raytree_update_materials succeeds exactly when the shape is the fresh tree's
    if keeps:
        st = abi.raytree_update_materials(tu)
        assert planes_differing(s.planes(tu), want, what + " updated vs a fresh tree") == 0
        same_info(abi, tu, tf, what)
        print("%s update: shadow %d, %.3f ms kernels" % (what, st["rays_shadow"], st["kernel_ms"]))
        assert (st["rays_shadow"] == 0) == (not shadow_rule), (what, st["rays_shadow"])
        assert st["rays_primary"] == st["rays_secondary"] == st["shaded_hits"] == 0
    else:
        refused(abi, "update", tu, MT_ERR_UNSUPPORTED, "change the shape of the ray tree")
        assert planes_differing(s.planes(tu), original, what + " after the refused update") == 0
        assert_stale(s, tu)
    # mt_raytree_regrow_materials always does
    out = abi.raytree_regrow(tr)
    got = s.planes(tr)
    assert planes_differing(got, want, what + " regrown vs a fresh tree") == 0
    info = same_info(abi, tr, tf, what)
    print("%s regrow: regrown %d, layers %d -> %d, kept %s traced %s dropped %s, secondary %d shadow %d, %.3f ms kernels"
          % (what, out["regrown"], out["n_layers_before"], out["n_layers_after"], out["kept"][:info["n_layers"]],
             out["traced"][:info["n_layers"]], out["dropped"][:len(original)], out["rays_secondary"], out["rays_shadow"],
             out["kernel_ms"]))
    assert out["regrown"] == (0 if keeps else 1)
    assert out["n_layers_before"] == len(original) and out["n_layers_after"] == info["n_layers"]
    assert [k + n for k, n in zip(out["kept"], out["traced"])][:info["n_layers"]] == info["n_rays"][:info["n_layers"]], what
    assert out["rays_primary"] == 0 and out["rays_secondary"] == sum(out["traced"])
    if not out["regrown"]:
        assert (out["rays_shadow"] == 0) == (not shadow_rule), (what, out["rays_shadow"])
    elif shadow_rule:
        assert out["rays_shadow"] > 0
    if keeps:  # (the refused tree too, now)
        pass
    else:
        abi.raytree_regrow(tu)
        assert planes_differing(s.planes(tu), want, what + " regrown after the refusal") == 0
    if moved_light is not None:
        # mt_raytree_update_lights works on the result
        k, lights = moved_light
        for x in (s, fresh):
            x.abi.set_lights(x.h, lights)
        abi.raytree_update_lights(tr, [k])
        tm = make_tree(fresh, depth)
        assert planes_differing(s.planes(tr), fresh.planes(tm), what + " after a moved light") == 0
        fresh.destroy(tm)
        for x in (s, fresh):
            x.abi.set_lights(x.h, LIGHTS)
        abi.raytree_update_lights(tr, [k])
    for t in (tu, tr):
        s.destroy(t)
    fresh.destroy(tf)
    return out


MOVED = (1, [tuple(l) if i != 1 else (150.0, 120.0, 250.0) + tuple(l[3:]) for i, l in enumerate(LIGHTS)])


@pytest.mark.parametrize("name", list(ALL_ROWS))
def test_tree_contract(name, flat_a, make, oracle_of):
    """A tree made under A with tri on, the set, the update and the regrow: frame and off-grid chunk, depths 0, 1, 2, 5;
    the chunk's trees keep uvw too.  At depth 5 the shaded result is mt_render_chunk's frame and the oracle's, and
    mt_raytree_update_lights works on it."""
    moves, n_rays, shadow = ALL_ROWS[name]
    A = np.array(flat_a["tri_material"], dtype=np.int32)
    B = ar.reassigned(flat_a, rr.TWO_WAY, moves)
    assert rule(flat_a, A, B) == shadow
    orc = oracle_of(name)
    for chunk in (None, OFF_GRID):
        s = make(flat_a, tri=True, uvw=chunk is not None)
        fresh = make(ar.built(flat_a, B), tri=True, uvw=chunk is not None)
        for d in DEPTHS:
            what = "%s %s d=%d" % (name, "chunk" if chunk else "frame", d)
            tree_contract(name, s, fresh, A, B, lambda x, depth: x.tree(chunk=chunk, depth=depth), what, shadow, depth=d,
                          moved_light=MOVED if d == 5 else None)
        # the shaded result at depth 5
        s.assign(A)
        t = s.tree(chunk=chunk)
        s.assign(B)
        out = s.abi.raytree_regrow(t)
        if chunk is None:
            assert s.abi.raytree_info(t)["n_rays"] == n_rays
            assert (name in ar.SAME_SHAPE) == (out["regrown"] == 0)
        rgb = s.abi.raytree_shade(t, LIGHTS)["rgb"]
        assert differing(rgb, s.frame(chunk=chunk), what + " shaded vs mt_render_chunk") == 0
        assert differing(rgb, fresh.frame(chunk=chunk), what + " shaded vs the built scene's frame") == 0
        assert differing(rgb, orc.render(CAM, W, H, chunk=chunk, max_level=5)["rgb"], what + " shaded vs the oracle") == 0
        # and back: A -> B -> A ends at the original tree
        s.assign(A)
        s.abi.raytree_regrow(t)
        ta = s.tree(chunk=chunk)
        assert planes_differing(s.planes(t), s.planes(ta), what + " and back") == 0


@pytest.mark.parametrize("name", list(ALL_ROWS))
def test_ray_list_tree(name, flat_a, make):
    """The same for a ray-list tree of 130 rays, n x 1: the last wave is partial."""
    moves, _, shadow = ALL_ROWS[name]
    A = np.array(flat_a["tri_material"], dtype=np.int32)
    B = ar.reassigned(flat_a, rr.TWO_WAY, moves)
    rays = ar.list_rays(130)
    s, fresh = make(flat_a, tri=True), make(ar.built(flat_a, B), tri=True)
    for d in (5, 1):
        tree_contract(name, s, fresh, A, B, lambda x, depth: x.tree_rays(rays, depth=depth), "%s list d=%d" % (name, d),
                      shadow, depth=d, moved_light=MOVED if d == 5 else None)
    s.assign(A)
    t = s.tree_rays(rays)
    s.assign(B)
    s.abi.raytree_regrow(t)
    colors = s.abi.raytree_shade_colors(t, LIGHTS)["color"]
    assert ru.same_plane(colors, s.abi.trace_rays(fresh.h, rays)["color"])


def test_one_triangle_of_a_quad(make):
    """assign_ref.quad_scene: the second triangle of the floor quad given the pane's material -- refracted children
    appear under half of the floor, and a shadow ray may see it."""
    a, b = M.MythTracer(), M.MythTracer()
    ar.quad_scene(a)
    ar.quad_scene(b, True)
    flat, flat_b = a.flatten(), b.flatten()
    assert all(np.array_equal(x["values"], y["values"]) for x, y in zip(flat["materials"], flat_b["materials"]))
    A, B = np.array(flat["tri_material"], dtype=np.int32), np.array(flat_b["tri_material"], dtype=np.int32)
    assert int((A != B).sum()) == 1 and rule(flat, A, B)
    w, h = ar.QUAD_SIZE
    s, fresh = make(flat, tri=True, lights=ar.QUAD_LIGHTS), make(ar.built(flat, B), tri=True, lights=ar.QUAD_LIGHTS)
    orc = orclib.OracleScene()
    ar.quad_scene(orc, True)
    orc.finalize()
    orc.set_lights(ar.QUAD_LIGHTS)
    t, ta = s.tree(ar.QUAD_CAMERA, w, h), s.tree(ar.QUAD_CAMERA, w, h)
    assert s.abi.raytree_info(t)["n_rays"] == ar.QUAD_A
    s.assign(B)
    refused(s.abi, "update", t, MT_ERR_UNSUPPORTED, "change the shape of the ray tree")
    out = s.abi.raytree_regrow(t)
    tf = fresh.tree(ar.QUAD_CAMERA, w, h)
    assert planes_differing(s.planes(t), fresh.planes(tf), "quad regrown vs a fresh tree") == 0
    assert s.abi.raytree_info(t)["n_rays"] == ar.QUAD_B and out["regrown"] == 1
    rgb = s.abi.raytree_shade(t, ar.QUAD_LIGHTS)["rgb"]
    assert differing(rgb, s.frame(ar.QUAD_CAMERA, w, h), "quad shaded vs mt_render_chunk") == 0
    assert differing(rgb, orc.render(ar.QUAD_CAMERA, w, h, max_level=5)["rgb"], "quad shaded vs the oracle") == 0
    s.assign(A)
    s.abi.raytree_regrow(t)
    assert planes_differing(s.planes(t), s.planes(ta)[:1], "quad and back") == 0


# ---- 4. refusals and compositions

def test_a_tree_without_tri_is_refused_untouched_and_stale(flat_a, make):
    moves = ar.ROWS["blue->mirror"][0]
    A = np.array(flat_a["tri_material"], dtype=np.int32)
    B = ar.reassigned(flat_a, rr.TWO_WAY, moves)
    changed = np.nonzero(A != B)[0]
    for uvw in (False, True):
        s = make(flat_a, tri=False, uvw=uvw)
        t = s.tree()
        original = s.planes(t)
        s.assign(B)
        for fn in ("update", "regrow"):
            text = refused(s.abi, fn, t, MT_ERR_UNSUPPORTED, "the ray tree keeps no tri")
            assert "%d triangles" % len(changed) in text and "triangle %d:" % changed[0] in text
            assert planes_differing(s.planes(t), original, "without tri, after the refused " + fn) == 0
            assert_stale(s, t)
        # A -> B -> A: nothing to do, no kernel
        s.assign(A)
        st = s.abi.raytree_update_materials(t)
        assert st["kernel_ms"] == 0 and st["rays_shadow"] == 0
        assert planes_differing(s.planes(t), original, "without tri, A -> B -> A") == 0
        assert differing(s.abi.raytree_shade(t, LIGHTS)["rgb"], s.frame(), "without tri, fresh again") == 0


def test_a_b_a_is_ok_with_zero_kernels(flat_a, make):
    A = np.array(flat_a["tri_material"], dtype=np.int32)
    s = make(flat_a, tri=True)
    t, t2 = s.tree(), s.tree()
    original = s.planes(t)
    for name in ("pane->blue", "left->right"):
        s.assign(ar.reassigned(flat_a, rr.TWO_WAY, ar.ROWS[name][0]))
        assert_stale(s, t)
    s.assign(A)
    assert_stale(s, t)
    st = s.abi.raytree_update_materials(t)
    out = s.abi.raytree_regrow(t2)
    for x in (st, out):
        assert x["kernel_ms"] == 0 and all(x[k] == 0 for k in ("rays_primary", "rays_secondary", "rays_shadow", "box_tests"))
    assert out["regrown"] == 0 and out["n_layers_before"] == out["n_layers_after"] == len(original)
    for x in (t, t2):
        assert planes_differing(s.planes(x), original, "A -> B -> A") == 0
        assert differing(s.abi.raytree_shade(x, LIGHTS)["rgb"], s.frame(), "A -> B -> A, fresh again") == 0


def test_a_textured_target_needs_uvw(scenes, make):
    """room_tex: the red wall given the textured floor material.  A tree with tri but without uvw is refused, with uvw the
    update restates the albedo from the stored uvw."""
    obj = scenes["room_tex"]
    flat = M.MythTracer(obj).flatten()
    A = np.array(flat["tri_material"], dtype=np.int32)
    B = ar.reassigned(flat, obj, ar.ROOM_TEX_MOVES)
    floor = ar.dense_index(flat, obj)["floor"]
    assert flat["materials"][floor]["tex"] >= 0
    changed = np.nonzero(A != B)[0]
    (w, h), chunk, depth = ar.ROOM_TEX["image"], ar.ROOM_TEX["chunk"], ar.ROOM_TEX["depth"]
    lights = lr.BENCH_LIGHTS[:ar.ROOM_TEX["n_lights"]]
    cam = scenegen.ROOM_CAMERA
    s = make(flat, tri=True, uvw=False, lights=lights)
    fresh = make(ar.built(flat, B), tri=True, uvw=True, lights=lights)
    t = s.tree(cam, w, h, chunk, depth)
    assert s.abi.raytree_info(t)["n_rays"] == ar.ROOM_TEX_A
    s.abi.set_raytree_uvw(s.h, True)
    tu, tr = s.tree(cam, w, h, chunk, depth), s.tree(cam, w, h, chunk, depth)
    original = s.planes(t)
    s.assign(B)
    for fn in ("update", "regrow"):
        text = refused(s.abi, fn, t, MT_ERR_UNSUPPORTED, "which has a texture: the ray tree keeps no uvw")
        assert "triangle %d was given material %d" % (changed[0], floor) in text
        assert planes_differing(s.planes(t), original, "room_tex without uvw, after the refused " + fn) == 0
        assert_stale(s, t, lights)
    tf = fresh.tree(cam, w, h, chunk, depth)
    want = fresh.planes(tf)
    assert [len(x["coef"]) for x in want] == ar.ROOM_TEX_B
    refused(s.abi, "update", tu, MT_ERR_UNSUPPORTED, "change the shape of the ray tree")
    out = s.abi.raytree_regrow(tr)
    print("room_tex regrow: kept %s traced %s, shadow %d" % (out["kept"][:4], out["traced"][:4], out["rays_shadow"]))
    assert planes_differing(s.planes(tr), want, "room_tex regrown vs a fresh tree") == 0
    same_info(s.abi, tr, tf, "room_tex")
    moved = int(sum((a["material"] != b["material"]).sum() for a, b in zip(original[:1], want[:1])))
    assert moved > 0  # (layer 0 holds rays whose albedo came from the texture through the stored uvw)
    assert differing(s.abi.raytree_shade(tr, lights)["rgb"], s.frame(cam, w, h, chunk, depth), "room_tex shaded") == 0
    # at depth 0 the shape cannot change: the update itself restates the textured albedo
    s.assign(A)
    t0 = s.tree(cam, w, h, chunk, 0)
    s.assign(B)
    s.abi.raytree_update_materials(t0)
    tf0 = fresh.tree(cam, w, h, chunk, 0)
    assert planes_differing(s.planes(t0), fresh.planes(tf0), "room_tex updated at depth 0") == 0


def test_a_reassignment_with_a_constants_edit_and_a_moved_light(flat_a, make):
    """One session: triangles reassigned, a material's constants edited and a light moved before the tree is asked to
    follow; after update_lights over the moved light it is the fresh tree."""
    A = np.array(flat_a["tri_material"], dtype=np.int32)
    mats_b = [dict(m, values=m["values"].copy()) for m in flat_a["materials"]]
    index = ar.dense_index(flat_a, rr.TWO_WAY)
    mats_b[index["mirror"]]["values"][10] = 0.5        # reflectance
    mats_b[index["left"]]["values"][0:3] = (0.2, 0.3, 0.9)  # ambient
    k, lights = MOVED
    for name in ("left->right", "blue->pane", "mirror->none"):
        B = ar.reassigned(flat_a, rr.TWO_WAY, ALL_ROWS[name][0])
        s = make(flat_a, tri=True)
        built = dict(ar.built(flat_a, B), materials=mats_b)
        fresh = make(built, tri=True, lights=lights)
        t = s.tree()
        s.assign(B)
        s.abi.set_materials(s.h, mats_b)
        s.abi.set_lights(s.h, lights)
        out = s.abi.raytree_regrow(t)
        s.abi.raytree_update_lights(t, [k])
        tf = fresh.tree()
        what = name + " + constants + a moved light"
        assert planes_differing(s.planes(t), fresh.planes(tf), what) == 0
        same_info(s.abi, t, tf, what)
        print("%s: regrown %d kept %s traced %s" % (what, out["regrown"], out["kept"][:6], out["traced"][:6]))
        assert differing(s.abi.raytree_shade(t, lights)["rgb"], fresh.frame(), what + " shaded") == 0


def test_regrows_light_count_check_fires_for_a_reassignment(flat_a, make):
    A = np.array(flat_a["tri_material"], dtype=np.int32)
    B = ar.reassigned(flat_a, rr.TWO_WAY, ar.ROWS["left->right"][0])
    s = make(flat_a, tri=True)
    t = s.tree()
    original = s.planes(t)
    s.assign(B)
    s.abi.set_lights(s.h, LIGHTS[:1])
    refused(s.abi, "regrow", t, MT_ERR_ARG, "the scene has 1 lights, the ray tree was made with %d" % len(LIGHTS))
    assert planes_differing(s.planes(t), original, "after the refused regrow") == 0
    s.abi.set_lights(s.h, LIGHTS)
    s.abi.raytree_regrow(t)
    assert differing(s.abi.raytree_shade(t, LIGHTS)["rgb"], s.frame(), "after the regrow") == 0


# ---- 5. the facade

def test_facade_and_python_round_trip(flat_a, oracle_of):
    name = "blue->pane"
    moves = ar.ROWS[name][0]
    orc = oracle_of(name)
    to = ar.targets(rr.TWO_WAY, ar.add_order_lines(flat_a), moves)
    m = M.MythTracer(rr.TWO_WAY)
    m.set_lights(LIGHTS)
    m.set_raytree_keep_triangles(True)
    frame_a = m.render(CAM, W, H)["rgb"]
    tree = m.raytree(CAM, W, H)
    assert M.hip_abi().raytree_keeps_tri(tree._tree())
    m.assign_material(list(to), "pane")
    m.update_triangle_materials()
    want = orc.render(CAM, W, H)["rgb"]
    assert differing(m.render(CAM, W, H)["rgb"], want, "facade: the frame after the reassignment vs the oracle") == 0
    with pytest.raises(RuntimeError, match=STALE):
        tree.shade()
    with pytest.raises(RuntimeError, match="change the shape"):
        tree.update_materials()
    tree.regrow()
    assert tree.info["n_rays"] == ar.ROWS[name][1]
    assert differing(tree.shade()["rgb"], want, "facade: the regrown tree shaded vs the oracle") == 0
    # a material no triangle used at the upload is not in the uploaded table: the call edits, it does not add
    assert m.add_material("spare", (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), (0, 0, 0)) >= 0
    m.assign_material([0], "spare")
    with pytest.raises(RuntimeError, match="triangle 0 points at a material that was not uploaded"):
        m.update_triangle_materials()
    assert differing(m.render(CAM, W, H)["rgb"], want, "facade: after the refusal") == 0
    m.assign_material([0], "floor")
    m.assign_material(list(to), "blue")
    m.update_triangle_materials()
    assert differing(m.render(CAM, W, H)["rgb"], frame_a, "facade: and back") == 0
    tree.regrow()
    assert tree.info["n_rays"] == ar.TREE_A
    tree.close()
    # before the first upload the call is Prepare; two replicas on one device both take the set.  (One face only: a
    # material that lost ALL its triangles before the upload is not uploaded, and there is no way back to it.)
    one = ar.targets(rr.TWO_WAY, ar.add_order_lines(flat_a), ar.ROWS["blue#2->pane"][0])
    want = oracle_of("blue#2->pane").render(CAM, W, H)["rgb"]
    multi = M.MythTracer(rr.TWO_WAY)
    multi.set_lights(LIGHTS)
    multi.set_devices([0, 0])
    multi.assign_material(list(one), "pane")
    multi.update_triangle_materials()
    assert differing(multi.render_image(CAM, W, H), want, "facade: assigned before the upload, two replicas") == 0
    multi.assign_material(list(one), "blue")
    multi.update_triangle_materials()
    assert differing(multi.render_image(CAM, W, H), frame_a, "facade: two replicas and back") == 0
    multi.assign_material(list(one), "pane")
    multi.update_triangle_materials()
    assert differing(multi.render_image(CAM, W, H), want, "facade: two replicas and there again") == 0
