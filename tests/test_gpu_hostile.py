"""The hostile scene family (tests/hostile_scenes.py) on a real MI355X (-m gpu): every device copy of TraceRayWorker
-- the state machine with its quarter and cell roles, the ray pool, the light-buffer kernels, the ray-tree kernels and
the material-edit kernels -- under material tables, normals and lights at which its comparisons are decided by the
unusual value.  tests/test_hostile_cpu.py pins the truths used here (the oracle to the compiled reference, the numpy
restatements to the oracle).

Bars.  GPU against oracle or restatement, EXACT group (Ns 0 on every material: pow is exactly 1): zero differing bytes
and bits.  POW group: test_gpu_parity.assert_rgb_close for bitmaps and test_gpu_raylist.specular_bound for linear
colours, both imported.  GPU against GPU (the header's byte-identity contracts): identity in both groups.  Every test
prints its differing counts.  All frames are 64 x 48.
"""
import ctypes
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gbuffer_ref  # noqa: E402
import hostile_scenes as hs  # noqa: E402
import lightbuffer_ref as lr  # noqa: E402
import material_edit_ref as me  # noqa: E402
import raylist_ref as rl  # noqa: E402
import raytree_ref as rr  # noqa: E402
import test_gpu_material_edit as gme  # noqa: E402
import test_gpu_raytree as grt  # noqa: E402
from gbuffer_ref import same_bits  # noqa: E402
from test_gpu_parity import assert_rgb_close, counters_match  # noqa: E402
from test_gpu_raylist import specular_bound  # noqa: E402

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding  # noqa: E402

W, H = hs.W, hs.H
NAMES = list(hs.CASES)
TABLE_ONLY = [n for n in NAMES if hs.CASES[n]["normals"] == "unit" and hs.CASES[n]["depth"] == hs.DEPTH and hs.CASES[n]["edit"]]
MOVED = ["light_in_stack", "light_1e-6_above_pane", "light_5e-8_above_pane", "light_at_camera", "light_behind_wall"]
COUNTERS = ("rays_primary", "rays_secondary", "rays_shadow", "shaded_hits")
RELIGHT = ("point", "normal", "albedo", "material")
MT_ERR_UNSUPPORTED = -3


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    return hs.Family(str(tmp_path_factory.mktemp("hostile")))


@pytest.fixture
def make(family):
    made = []

    def _make(name):
        made.append(gme.Scene(family(name)["obj"]))
        return made[-1]
    yield _make
    for s in made:
        s.close()


def differing(a, b, what):
    n = int((np.asarray(a) != np.asarray(b)).sum())
    print("%s: %d of %d differ" % (what, n, np.asarray(a).size))
    return n


def assert_frame(got, want, group, what):
    """A device frame (rgb, line, point, stats) against the oracle's (rgb, line, point, counters)."""
    if group == "exact":
        assert differing(got["rgb"], want["rgb"], what + " rgb bytes") == 0
    else:
        assert_rgb_close(got["rgb"], want["rgb"], what)
    if "line" in got:
        assert differing(got["line"], want["line"], what + " line_no") == 0
        assert same_bits(got["point"], want["point"], what + " point") == 0
    print(what, {k: (got["stats"][k], want["counters"][k]) for k in COUNTERS})
    counters_match({k: got["stats"][k] for k in COUNTERS}, {k: want["counters"][k] for k in COUNTERS})


def render(s, c, depth=None, debug=True):
    return s.abi.render_chunk(s.h, binding.sensor(c["camera"], W, H), W, H, max_depth=c["depth"] if depth is None else depth,
                              debug=debug)


# ---- frames

@pytest.mark.parametrize("name", NAMES)
def test_frames_under_every_engine(name, family, make):
    """mt_render_chunk with a debug buffer and stats under the state machine, the ray pool and the hybrid (its later
    frames, without a debug buffer, are scheduled from the first one's costs), then the state machine forced into quarters and into cells
    (test_state_machine_cells_for_blocks_with_zero_component_rays' knobs): the oracle's rgb, line_no, point bits and ray
    counts -- rays_shadow is the sharp check of the shadow loop's thresholds -- and, engine against engine, identity."""
    c = family(name)
    s = make(name)
    s.set_lights(c["lights"])
    first = None
    # (a launch with a debug buffer has no cost history: the hybrid, the quarters and the cells need launches without)
    for engine, launches in ((1, (True,)), (2, (True,)), (3, (True, False, False, False))):
        s.abi.set_engine(s.h, engine)
        for launch, debug in enumerate(launches):
            r = render(s, c, debug=debug)
            what = "%s engine %d launch %d" % (name, engine, launch)
            assert_frame(r, c["want"], c["group"], what)
            first = first or r
            assert differing(r["rgb"], first["rgb"], what + " rgb against engine 1") == 0
    s.abi.set_engine(s.h, 1)
    for share, quad in ((1e-6, 0.05), (1e-6, 0.95), (0.8, 0.95)):
        s.abi.set_tuning(s.h, "SM_CELL_SHARE", share)
        s.abi.set_tuning(s.h, "QUAD_SHARE", quad)
        for launch in range(3):  # (the first one after set_tuning has no cost history)
            r = render(s, c, debug=False)
            what = "%s cell share %g quad share %g launch %d" % (name, share, quad, launch)
            assert_frame(r, c["want"], c["group"], what)
            assert differing(r["rgb"], first["rgb"], what + " rgb against the unordered launch") == 0


@pytest.mark.parametrize("name", hs.NI_CASES)
def test_ni_cases_are_the_base_frame(name, family, make):
    base, s = make("base"), make(name)
    frames = []
    for x, n in ((base, "base"), (s, name)):
        x.set_lights(family(n)["lights"])
        frames.append(render(x, family(n)))
    assert differing(frames[1]["rgb"], frames[0]["rgb"], name + " rgb against base") == 0
    assert same_bits(frames[1]["point"], frames[0]["point"], name + " point against base") == 0
    assert {k: frames[1]["stats"][k] for k in COUNTERS} == {k: frames[0]["stats"][k] for k in COUNTERS}


# ---- G-buffer, light buffer, deferred shade

@pytest.mark.parametrize("name", NAMES)
def test_lightbuffer_and_deferred_shade(name, family, make):
    """power and in_shadow against lightbuffer_ref (NaN = NaN, bytes exact), mt_shade_direct equal to
    mt_render_chunk(max_depth 0) and to the oracle's direct frame; the host forms and, on a stream, the device forms."""
    import torch
    c = family(name)
    orc, lights = c["orc"], c["lights"]
    s = make(name)
    s.set_lights(lights)
    sens = binding.sensor(c["camera"], W, H)
    gb = gbuffer_ref.oracle_gbuffer(orc, c["camera"], W, H)
    want = lr.ref_lightbuffer(orc, gb, lights)
    got = s.abi.render_lightbuffer(s.h, sens, W, H, len(lights), gbuffer_channels=RELIGHT)
    assert same_bits(got["power"], want["power"], name + " power") == 0
    assert differing(got["in_shadow"], want["in_shadow"], name + " in_shadow") == 0
    print(name, "rays_shadow", got["stats"]["rays_shadow"], want["rays_shadow"])
    assert got["stats"]["rays_shadow"] == want["rays_shadow"]
    for plane in ("point", "normal", "albedo"):
        assert same_bits(got[plane], gb[plane], "%s G-buffer %s" % (name, plane)) == 0
    direct = orc.render(c["camera"], W, H, max_level=0, debug=True)
    frame0 = render(s, c, depth=0)
    assert_frame(frame0, direct, c["group"], name + " mt_render_chunk at depth 0")
    shaded = s.abi.shade_direct(s.h, sens, W, H, {p: got[p] for p in RELIGHT}, got, lights)
    assert differing(shaded["rgb"], frame0["rgb"], name + " mt_shade_direct against mt_render_chunk(0)") == 0
    # the device forms
    stream = torch.cuda.Stream()
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    g = dict(point=f64(H, W, 3), normal=f64(H, W, 3), albedo=f64(H, W, 3),
             material=torch.zeros((H, W), dtype=torch.int32, device="cuda"))
    lb = dict(power=f64(len(lights), H, W, 3), in_shadow=torch.full((len(lights), H, W), 77, dtype=torch.uint8, device="cuda"))
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        sp = ctypes.c_void_p(stream.cuda_stream)
        s.abi.render_lightbuffer_device(s.h, sens, W, H, (0, 0, W, H), {n: t.data_ptr() for n, t in lb.items()},
                                        {n: t.data_ptr() for n, t in g.items()}, sp)
        s.abi.shade_direct_device(s.h, sens, W, H, (0, 0, W, H), {n: t.data_ptr() for n, t in g.items()},
                                  {n: t.data_ptr() for n, t in lb.items()}, lights, rgb.data_ptr(), sp)
    stream.synchronize()
    assert same_bits(lb["power"].cpu().numpy(), got["power"], name + " device power against the host form") == 0
    assert differing(lb["in_shadow"].cpu().numpy(), got["in_shadow"], name + " device in_shadow") == 0
    assert differing(rgb.cpu().numpy(), frame0["rgb"], name + " device relight") == 0


# ---- ray trees

@pytest.mark.parametrize("name", NAMES)
def test_ray_trees(name, family, make):
    """Every plane of every layer against raytree_ref (coef bits, child_refl and child_refr, rays per layer);
    mt_raytree_shade equal to mt_render_chunk; mt_raytree_shade_colors against raylist_ref; mt_trace_rays over the
    sensor's rays equal to the frame.  depth_16 runs at MT_MAX_RECURSION."""
    c = family(name)
    orc, lights, depth = c["orc"], c["lights"], c["depth"]
    s = make(name)
    s.set_lights(lights)
    t, st = s.tree(c["camera"], W, H, None, depth)
    grt.assert_tree_equal(s, t, orc, c["tree"], name)
    for k in COUNTERS:
        assert st[k] == c["tree"][k], (k, st[k], c["tree"][k])
    frame = render(s, c, debug=False)["rgb"]
    rgb = s.abi.raytree_shade(t, lights)["rgb"]
    assert differing(rgb, frame, name + " mt_raytree_shade against mt_render_chunk") == 0
    color = s.abi.raytree_shade_colors(t, lights)["color"].reshape(-1, 3)
    assert differing(rr.v3d_to_rgb(color).reshape(H, W, 3), rgb, name + " colours, quantised") == 0
    term = {}
    ref = rl.colors(orc, c["tree"], lights, term)
    spec = term["specular"] if c["group"] == "pow" else np.zeros(len(ref), dtype=bool)
    assert same_bits(color[~spec], ref[~spec], name + " colours of the rays that call no pow") == 0
    if spec.any():
        d = np.abs(color[spec] - ref[spec])
        print("%s: %d rays with a specular term, largest |d| %.3e (largest colour %.3e), %d channels not bit-equal"
              % (name, int(spec.sum()), d.max(), np.abs(ref[spec]).max(), int((d > 0).sum())))
        assert (d <= specular_bound(ref[spec])).all()
    rays = gbuffer_ref.pixel_rays(c["camera"], W, H).reshape(W * H, 6)
    traced = s.abi.trace_rays(s.h, rays, W, max_depth=depth)
    assert differing(traced["rgb"], frame, name + " mt_trace_rays against the frame") == 0
    assert same_bits(traced["color"].reshape(-1, 3), color, name + " mt_trace_rays colours") == 0


# ---- moved lights

@pytest.mark.parametrize("name", MOVED)
def test_a_light_moved_to_a_hostile_place(name, family, make):
    """Light 0 moves from open space (the base's lights) to the case's place: mt_update_lightbuffer gives the planes of
    a fresh light buffer and mt_raytree_update_lights a fresh tree, bit for bit."""
    base, c = family("base"), family(name)
    s = make("base")
    sens = binding.sensor(base["camera"], W, H)
    s.set_lights(base["lights"])
    lb = s.abi.render_lightbuffer(s.h, sens, W, H, 2, gbuffer_channels=("point", "material"))
    t, _ = s.tree(base["camera"], W, H)
    s.set_lights(c["lights"])
    s.abi.update_lightbuffer(s.h, {p: lb[p] for p in ("point", "material")}, {p: lb[p] for p in ("power", "in_shadow")}, [0])
    fresh = s.abi.render_lightbuffer(s.h, sens, W, H, 2)
    assert same_bits(lb["power"], fresh["power"], name + " updated power against a fresh buffer") == 0
    assert differing(lb["in_shadow"], fresh["in_shadow"], name + " updated in_shadow") == 0
    s.abi.raytree_update_lights(t, [0])
    tf, _ = s.tree(base["camera"], W, H)
    assert gme.planes_differing(s.planes(t), s.planes(tf), name + " updated tree against a fresh tree") == 0
    grt.assert_tree_equal(s, t, c["orc"], c["tree"], name + " updated tree")


# ---- material edits

@pytest.mark.parametrize("name", TABLE_ONLY)
def test_materials_edited_in_place(name, family, make):
    """mt_scene_set_materials(base -> case) renders what a scene BUILT with the case's table renders (frame, G-buffer,
    light buffer); mt_raytree_update_materials succeeds exactly where material_edit_ref predicts, and the tree is then
    a fresh tree's; otherwise MT_ERR_UNSUPPORTED names the predicted first ray, every plane is untouched, and with the
    base set back the update succeeds."""
    base, c = family("base"), family(name)
    lights, cam = base["lights"], base["camera"]
    sens = binding.sensor(cam, W, H)
    s, fresh = make("base"), make(name)
    gme.same_geometry(s, fresh)
    A, B = s.materials, fresh.materials
    for x in (s, fresh):
        x.set_lights(lights)
    t, _ = s.tree(cam, W, H)
    before = s.planes(t)
    s.set_materials(B)
    assert gme.same_materials(s.abi.get_materials(s.h, len(B)), B)
    got, want = render(s, base), render(fresh, base)
    assert differing(got["rgb"], want["rgb"], name + " frame after the edit against a fresh scene") == 0
    assert {k: got["stats"][k] for k in COUNTERS} == {k: want["stats"][k] for k in COUNTERS}
    got = s.abi.render_lightbuffer(s.h, sens, W, H, len(lights), gbuffer_channels=RELIGHT)
    want = fresh.abi.render_lightbuffer(fresh.h, sens, W, H, len(lights), gbuffer_channels=RELIGHT)
    for plane in ("power", "albedo", "normal", "point"):
        assert same_bits(got[plane], want[plane], "%s %s after the edit" % (name, plane)) == 0
    assert np.array_equal(got["in_shadow"], want["in_shadow"]) and np.array_equal(got["material"], want["material"])
    predicted = me.check_pass(base["tree"], c["orc"].materials())
    print("%s: predicted %s" % (name, "same shape" if predicted["count"] == 0 else "refused, %d rays, the first at %s"
                               % (predicted["count"], predicted["first"])))
    if predicted["count"] == 0:
        s.abi.raytree_update_materials(t)
        tf, _ = fresh.tree(cam, W, H)
        assert gme.planes_differing(s.planes(t), fresh.planes(tf), name + " updated tree against a fresh tree") == 0
        assert differing(s.abi.raytree_shade(t, lights)["rgb"], render(fresh, base, debug=False)["rgb"],
                         name + " updated tree, shaded") == 0
    else:
        text, _ = gme.refused(s.abi, t, MT_ERR_UNSUPPORTED, r"change the shape")
        m = re.search(r"(\d+) rays spawn other children, the first in layer (\d+) at ray (\d+)", text)
        assert m and (int(m.group(2)), int(m.group(3))) == predicted["first"] and int(m.group(1)) == predicted["count"]
        assert gme.planes_differing(s.planes(t), before, name + " after the refusal") == 0
    s.set_materials(A)
    s.abi.raytree_update_materials(t)
    assert gme.planes_differing(s.planes(t), before, name + " base set back") == 0
