"""What the host entry points of include/mythtracer_hip.h do AROUND their launches, on a real MI355X (-m gpu): a host
call that is given an mt_stats counts whatever mt_scene_set_stats says, and leaves the scene's switch as it found it --
when it succeeds, when it fails half way, and when its argument check refuses it.  The host calls without work counters
report zero work and a kernel time.

Every case runs on the `mini` scene under scenegen.ROOM_LIGHTS and ROOM_CAMERA, a 64x36 frame at depth 3.  "The switch
is off" is shown the way tests/test_gpu_parity.py::test_work_counters_can_be_switched_off shows it: a
mt_render_chunk_device launch after which mt_scene_read_stats finds no ray counted.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding, scenegen  # noqa: E402
from test_gpu_parity import RAY_KEYS  # noqa: E402

W, H, DEPTH = 64, 36, 3
LIGHTS = scenegen.ROOM_LIGHTS
CAM = scenegen.ROOM_CAMERA
TIMES = ("kernel_ms", "total_ms")
MT_ERR_ARG, MT_ERR_UNSUPPORTED = -1, -3
REFL, TR, TF = 10, 11, 12  # places in a material's 16 values (binding.HipAbi._material_array)


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"


@pytest.fixture(scope="module")
def flat(scenes):
    return M.MythTracer(scenes["mini"]).flatten()


class Session:
    """One scene of `flat` with the room's lights, its trees destroyed with it."""

    def __init__(self, flat):
        self.abi = M.hip_abi()
        self.flat = flat
        self.h = self.abi.scene_create(flat)
        self.abi.set_lights(self.h, LIGHTS)
        self.sens = binding.sensor(CAM, W, H)
        self.trees = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for t in self.trees:
            self.abi.raytree_destroy(t)
        self.abi.scene_destroy(self.h)

    def frame(self):
        return self.abi.render_chunk(self.h, self.sens, W, H, max_depth=DEPTH)

    def tree(self):
        t, stats = self.abi.raytree_create(self.h, self.sens, W, H, max_depth=DEPTH)
        self.trees.append(t)
        return t, stats

    def planes(self):
        """(G-buffer planes, light-buffer planes) of the frame, as the relight and the update read them"""
        r = self.abi.render_lightbuffer(self.h, self.sens, W, H, len(LIGHTS),
                                        gbuffer_channels=binding.RELIGHT_GBUFFER_PLANES)
        return ({n: r[n] for n in binding.RELIGHT_GBUFFER_PLANES}, {n: r[n] for n in binding.LIGHTBUFFER_PLANES})

    def edit(self, change):
        """set_materials with change(values) applied to a copy of every material's 16 values"""
        mats = []
        for m in self.flat["materials"]:
            v = np.array(m["values"], dtype=np.float64)
            change(v)
            mats.append(dict(values=v, tex=m["tex"]))
        self.abi.set_materials(self.h, mats)

    def edit_shadows(self):
        """Another transmission filter for the glass: shadow rays see it, no ray spawns other children -> a retrace."""
        def change(v):
            if v[TR] != 0.0:
                v[TF:TF + 3] = (0.5, 0.4, 0.3)
        self.edit(change)

    def edit_shape(self):
        """Reflectances swapped between none and some: floor and mirror stop reflecting, every other surface starts."""
        def change(v):
            v[REFL] = 0.4 if v[REFL] == 0.0 else 0.0
        self.edit(change)

    def device_rays(self):
        """The ray counters one mt_render_chunk_device launch leaves for mt_scene_read_stats."""
        import torch
        buf = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        self.abi.render_chunk_device(self.h, self.sens, W, H, (0, 0, W, H), DEPTH, ctypes.c_void_p(buf.data_ptr()))
        torch.cuda.synchronize()
        st = self.abi.read_stats(self.h)
        return {k: st[k] for k in RAY_KEYS}

    def switch_is(self, enabled):
        got = self.device_rays()
        print("switch %s: a device launch counted %s" % ("on" if enabled else "off", got))
        return (sum(got.values()) > 0) if enabled else all(v == 0 for v in got.values())


def rays(stats):
    return {k: stats[k] for k in RAY_KEYS}


def ray_list(sens):
    """The frame's primary rays as a ray list: (n, 6) origin and direction, row by row."""
    o, start, ds, dp = (np.asarray(sens[i:i + 3]) for i in (0, 3, 6, 9))
    y, x = np.mgrid[0:H, 0:W]
    d = start + ds * y[..., None] + dp * x[..., None]
    return np.concatenate([np.broadcast_to(o, d.shape), d], axis=-1).reshape(-1, 6)


# ---- the host calls that take `stats` and have work counters: name -> the call on a fresh Session, returning its stats
def _chunk(s):
    return s.frame()["stats"]


def _chunk_ss(s):
    return s.abi.render_chunk_ss(s.h, binding.sensor(CAM, 2 * W, 2 * H), W, H, 2, max_depth=DEPTH)["stats"]


def _chunk_adaptive(s):
    r = s.abi.render_chunk_adaptive(s.h, s.sens, binding.sensor(CAM, 2 * W, 2 * H), W, H, 2, 8, max_depth=DEPTH)
    assert r["info"]["n_refined"] > 0  # (the refinement launch ran too)
    return r["stats"]


def _gbuffer(s):
    return s.abi.render_gbuffer(s.h, s.sens, W, H)["stats"]


def _lightbuffer(s):
    return s.abi.render_lightbuffer(s.h, s.sens, W, H, len(LIGHTS))["stats"]


def _update_lightbuffer(s):
    gb, lb = s.planes()
    return s.abi.update_lightbuffer(s.h, gb, lb, [0, 2])["stats"]


def _raytree_create(s):
    return s.tree()[1]


def _raytree_update_lights(s):
    return s.abi.raytree_update_lights(s.tree()[0], [1])


def _raytree_update_materials(s):
    t, _ = s.tree()
    s.edit_shadows()
    return s.abi.raytree_update_materials(t)


def _raytree_regrow(s):
    t, _ = s.tree()
    s.edit_shape()
    r = s.abi.raytree_regrow(t)
    assert r["regrown"] == 1 and sum(r["traced"]) > 0, r
    return r


def _trace_rays(s):
    return s.abi.trace_rays(s.h, ray_list(s.sens), list_w=W, max_depth=DEPTH)["stats"]


COUNTED = {"mt_render_chunk": _chunk, "mt_render_chunk_ss": _chunk_ss, "mt_render_chunk_adaptive": _chunk_adaptive,
           "mt_render_gbuffer": _gbuffer, "mt_render_lightbuffer": _lightbuffer,
           "mt_update_lightbuffer": _update_lightbuffer, "mt_raytree_create": _raytree_create,
           "mt_raytree_update_lights": _raytree_update_lights, "mt_raytree_update_materials": _raytree_update_materials,
           "mt_raytree_regrow_materials": _raytree_regrow, "mt_trace_rays": _trace_rays}


@pytest.mark.parametrize("name", list(COUNTED))
def test_host_call_counts_with_the_switch_off_and_leaves_it_off(name, flat):
    """The call's ray counters with mt_scene_set_stats(scene, 0) equal those with the switch on (and are not all zero:
    every one of these calls traces rays); afterwards the switch is where the caller put it."""
    got = {}
    for enabled in (True, False):
        with Session(flat) as s:
            s.abi.set_stats(s.h, enabled)
            got[enabled] = rays(COUNTED[name](s))
            assert s.switch_is(enabled), (name, enabled)
    print("%s: switch on %s, off %s" % (name, got[True], got[False]))
    assert sum(got[True].values()) > 0, name
    assert got[False] == got[True], name


# ---- the host calls without work counters
def _shade_direct(s):
    gb, lb = s.planes()
    return s.abi.shade_direct(s.h, s.sens, W, H, gb, lb, LIGHTS)["stats"]


def _retexture(s):
    g = s.abi.render_gbuffer(s.h, s.sens, W, H, channels=("material", "uvw"))
    return s.abi.retexture_gbuffer(s.h, g)["stats"]


def _raytree_shade(s):
    return s.abi.raytree_shade(s.tree()[0], LIGHTS)["stats"]


COUNTERLESS = {"mt_shade_direct": _shade_direct, "mt_retexture_gbuffer": _retexture, "mt_raytree_shade": _raytree_shade}


@pytest.mark.parametrize("name", list(COUNTERLESS))
@pytest.mark.parametrize("enabled", [True, False])
def test_counterless_host_call_reports_no_work_and_a_kernel_time(name, enabled, flat):
    with Session(flat) as s:
        s.abi.set_stats(s.h, enabled)
        st = COUNTERLESS[name](s)
        print(name, st)
        assert {k: v for k, v in st.items() if k not in TIMES} == {k: 0 for k in st if k not in TIMES}
        assert st["kernel_ms"] > 0 and st["total_ms"] > 0
        assert s.switch_is(enabled)


def test_a_call_that_fails_half_way_leaves_the_switch_and_the_counters_alone(flat):
    """mt_raytree_update_materials after an edit that changes the tree's shape gives up behind its check pass
    (MT_ERR_UNSUPPORTED): the switch is still off, the next counted call counts what it counted before, and
    mt_raytree_regrow_materials takes the edit -- the tree then shades to the bytes of a tree made afresh."""
    with Session(flat) as s:
        s.abi.set_stats(s.h, False)
        t, _ = s.tree()
        s.edit_shape()
        before = rays(s.frame()["stats"])
        st = binding.mt_stats()
        rc = s.abi.lib.mt_raytree_update_materials(t, ctypes.addressof(st))
        print("mt_raytree_update_materials: %d, %s" % (rc, s.abi.last_error()))
        assert rc == MT_ERR_UNSUPPORTED and "spawn other children" in s.abi.last_error()
        assert s.switch_is(False)
        assert rays(s.frame()["stats"]) == before
        r = s.abi.raytree_regrow(t)
        assert r["regrown"] == 1, r
        new, _ = s.tree()
        assert np.array_equal(s.abi.raytree_shade(t, LIGHTS)["rgb"], s.abi.raytree_shade(new, LIGHTS)["rgb"])
        assert s.switch_is(False)


def test_a_call_refused_by_its_argument_check_leaves_the_switch_and_the_counters_alone(flat):
    """A NULL output: MT_ERR_ARG from mt_render_chunk, mt_render_gbuffer and mt_raytree_shade, each asked for stats."""
    with Session(flat) as s:
        s.abi.set_stats(s.h, False)
        before = rays(s.frame()["stats"])
        t, _ = s.tree()
        st = binding.mt_stats()
        sensor = s.abi.make_sensor(s.sens)
        lights = np.ascontiguousarray(LIGHTS, dtype=np.float64)
        refused = {
            "mt_render_chunk": lambda: s.abi.lib.mt_render_chunk(s.h, ctypes.byref(sensor), W, H, 0, 0, W, H, DEPTH, None,
                                                                 None, ctypes.addressof(st)),
            "mt_render_gbuffer": lambda: s.abi.lib.mt_render_gbuffer(s.h, ctypes.byref(sensor), W, H, 0, 0, W, H, None,
                                                                     ctypes.addressof(st)),
            "mt_raytree_shade": lambda: s.abi.lib.mt_raytree_shade(t, lights.ctypes.data, len(LIGHTS), None,
                                                                   ctypes.addressof(st))}
        for name, call in refused.items():
            rc = call()
            print("%s: %d, %s" % (name, rc, s.abi.last_error()))
            assert rc == MT_ERR_ARG and "NULL" in s.abi.last_error(), name
            assert s.switch_is(False), name
            assert rays(s.frame()["stats"]) == before, name
