"""MT_TUNE_SHADOW_BOUND (mt_shadow_bound.h; mt_trace.h, the BOUNDED walk): a shadow iteration of the frame kernels does
not walk into what its ray enters beyond the light.  The picture must not know: with the work counters off, frames
at knob 0, 1 and 2 are byte-equal to each other and to the oracle's; with them on at knob 2 the ray counts and shaded
hits are the oracle's, and under a light at mid-room -- the ceiling and the far walls a hundred units behind it --
the node visits are strictly below knob 0's for the state machine, lean and full (the ray pool's own shadow records
carry no bound: engine 2, and a hybrid launch of 96x64, which the pool takes whole, may only be equal).

Scenes: `mini` (2 128 triangles) under the bench's lights and under the mid-room light, and the planted scene of
shadow_bound_ref.py (occluders at, just before and just behind a light, glass in between), 96x64, depth 5.  Edge
cases: a light outside the scene's box, non-finite light positions, and a description whose triangle pokes out of
its cell -- not eligible: knob 2 must leave every counter where knob 0 has it.  The TIE scene (a light on the root's
centre line, triangles with a vertex at the light in the cells around that edge) sends lanes through kTraceRedo and
MODE_SHADOW_AGAIN, with whole blocks, quarters, cells and in the lean kernel; and a hybrid launch large enough for its
state machine to get units shows that part bounded."""
import ctypes

import numpy as np
import pytest

import orclib
import shadow_bound_ref as sb

pytestmark = pytest.mark.gpu

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding, scenegen  # noqa: E402

W, H, DEPTH = sb.W, sb.H, sb.DEPTH
RAY_KEYS = ("rays_primary", "rays_secondary", "rays_shadow", "shaded_hits")
# (name, engine, MT_TUNE_LEAN_KERNEL)
CONFIGS = [("state machine", 1, 0), ("ray pool", 2, 1), ("hybrid", 3, 1), ("lean kernel", 1, 2)]
CASES = {"mini, bench lights": ("mini", scenegen.ROOM_CAMERA, scenegen.ROOM_LIGHTS),
         "mini, mid-room light": ("mini", scenegen.ROOM_CAMERA, sb.MID_LIGHT),
         "planted": ("planted", sb.PLANTED_CAM, sb.PLANTED_LIGHTS)}


@pytest.fixture(scope="module")
def world(scenes, native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"
    mini = M.MythTracer(scenes["mini"])
    planted, planted_o = M.MythTracer(), orclib.OracleScene()
    sb.fill(planted)
    sb.fill(planted_o)
    tie, tie_o = M.MythTracer(), orclib.OracleScene()
    sb.fill(tie, sb.tie_triangles())
    sb.fill(tie_o, sb.tie_triangles())
    return dict(flat={"mini": mini.flatten(), "planted": planted.flatten(), "tie": tie.flatten()},
                oracle={"mini": orclib.OracleScene(scenes["mini"]), "planted": planted_o, "tie": tie_o},
                keep=(mini, planted, tie), want={})


def oracle_frame(world, scene, cam, lights, size=(W, H)):
    """The oracle's frame and counters, computed once per (scene, camera, lights, size)."""
    key = (scene, tuple(cam), repr(lights), size)
    if key not in world["want"]:
        world["oracle"][scene].set_lights(lights)
        world["want"][key] = world["oracle"][scene].render(cam, size[0], size[1], max_level=DEPTH)
    return world["want"][key]


def new_scene(flat, lights, engine, lean):
    abi = M.hip_abi()
    h = abi.scene_create(flat)
    abi.set_engine(h, engine)
    abi.set_lights(h, lights)
    abi.set_tuning(h, "LEAN_KERNEL", float(lean))
    return h


def frames_off(h, cam, knob, n=3):
    """n frames with the work counters off and the knob at `knob`: the first without a cost history (set_tuning
    forgets it), the others with -- where the lean kernel runs, if it is allowed to.  Returns the frames and whether
    any was lean."""
    import torch
    abi = M.hip_abi()
    abi.set_tuning(h, "SHADOW_BOUND", float(knob))
    abi.set_stats(h, False)
    sens = binding.sensor(cam, W, H)
    buf = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    out, lean = [], False
    for _ in range(n):
        buf.zero_()
        abi.render_chunk_device(h, sens, W, H, (0, 0, W, H), DEPTH, ctypes.c_void_p(buf.data_ptr()))
        torch.cuda.synchronize()
        out.append(buf.cpu().numpy())
        lean = lean or abi.lean_info(h)["lean"] != 0
    abi.set_stats(h, True)
    return out, lean


def frames_on(h, cam, knob, n=3, size=(W, H)):
    abi = M.hip_abi()
    abi.set_tuning(h, "SHADOW_BOUND", float(knob))
    return [abi.render_chunk(h, binding.sensor(cam, size[0], size[1]), size[0], size[1], max_depth=DEPTH) for _ in range(n)]


@pytest.mark.parametrize("config", CONFIGS, ids=[c[0] for c in CONFIGS])
@pytest.mark.parametrize("case", list(CASES))
def test_the_picture_does_not_know(world, case, config):
    scene, cam, lights = CASES[case]
    want = oracle_frame(world, scene, cam, lights)
    abi = M.hip_abi()
    h = new_scene(world["flat"][scene], lights, config[1], config[2])
    try:
        for knob in (0, 1, 2):
            got, lean = frames_off(h, cam, knob)
            for i, f in enumerate(got):
                assert np.array_equal(f, want["rgb"]), (case, config[0], knob, i, int((f != want["rgb"]).any(axis=2).sum()))
            if config[0] == "lean kernel":
                assert lean, "no frame of the forced configuration ran the lean kernel"
        # counters on: knob 1 counts the unbounded traversal (knob 0's work), knob 2 the bounded one
        on = {knob: frames_on(h, cam, knob) for knob in (0, 1, 2)}
        for knob, fs in on.items():
            for i, f in enumerate(fs):
                assert np.array_equal(f["rgb"], want["rgb"]), (case, config[0], knob, i)
                assert {k: f["stats"][k] for k in RAY_KEYS} == {k: want["counters"][k] for k in RAY_KEYS}, (case, config[0], knob, i)
        assert [f["stats"]["node_visits"] for f in on[1]] == [f["stats"]["node_visits"] for f in on[0]]
        v0, v2 = on[0][-1]["stats"]["node_visits"], on[2][-1]["stats"]["node_visits"]
        print("%s, %s: node visits %d at knob 0, %d at knob 2 (%.3f); mt_tests %d, %d" % (
            case, config[0], v0, v2, v2 / v0, on[0][-1]["stats"]["mt_tests"], on[2][-1]["stats"]["mt_tests"]))
        assert v2 <= v0
        if case == "mini, mid-room light" and config[0] in ("state machine", "lean kernel"):
            assert v2 < v0
    finally:
        abi.scene_destroy(h)


@pytest.mark.parametrize("lights", [sb.OUTSIDE_LIGHT, sb.NONFINITE_LIGHTS], ids=["light outside the box", "non-finite lights"])
def test_lights_a_bound_must_survive(world, lights):
    want = oracle_frame(world, "mini", scenegen.ROOM_CAMERA, lights)
    abi = M.hip_abi()
    for config in (CONFIGS[0], CONFIGS[3]):
        h = new_scene(world["flat"]["mini"], lights, config[1], config[2])
        try:
            for knob in (0, 2):
                for i, f in enumerate(frames_off(h, scenegen.ROOM_CAMERA, knob)[0]):
                    assert np.array_equal(f, want["rgb"]), (config[0], knob, i)
                for i, f in enumerate(frames_on(h, scenegen.ROOM_CAMERA, knob)):
                    assert np.array_equal(f["rgb"], want["rgb"]), (config[0], knob, i)
                    assert {k: f["stats"][k] for k in RAY_KEYS} == {k: want["counters"][k] for k in RAY_KEYS}
        finally:
            abi.scene_destroy(h)


def test_a_scene_that_is_not_eligible_traces_as_before(world):
    """A triangle poking out of its node's cell: the walk still renders the description, but nothing may be concluded
    from cells -- no bound, whatever the knob says: every counter of knob 2 is knob 0's.  (The same description
    without the poke does get fewer node visits: the check above is not vacuous.)"""
    abi = M.hip_abi()
    poked, _ = sb.poking(world["flat"]["planted"])
    visits = {}
    for name, flat in (("poked", poked), ("planted", world["flat"]["planted"])):
        h = new_scene(flat, sb.PLANTED_LIGHTS, 1, 0)
        try:
            a, b = frames_on(h, sb.PLANTED_CAM, 0, n=2), frames_on(h, sb.PLANTED_CAM, 2, n=2)
            for x, y in zip(a, b):
                assert np.array_equal(x["rgb"], y["rgb"]), name
            visits[name] = (a[-1]["stats"], b[-1]["stats"])
        finally:
            abi.scene_destroy(h)
    a, b = visits["poked"]
    assert {k: v for k, v in a.items() if not k.endswith("_ms")} == {k: v for k, v in b.items() if not k.endswith("_ms")}
    a, b = visits["planted"]
    assert b["node_visits"] < a["node_visits"]


# QUAD_SHARE, SM_CELL_SHARE (mt_order.h): all blocks whole / all as quarters (four lanes per pixel, the lights of a pixel
# side by side) / 2x2 cells on the blocks that hold a zero-component ray (the axis camera's pixel column and row)
FORMS = {"whole": (1e6, 0.8), "quarters": (1e-3, 1e6), "cells": (1e-6, 1e-6)}
CAM_AXIS = (24.0, 12.0, -20.0, 0.0, 0.0, 0.0, 80.0)
TIE_CASES = [("state machine, whole blocks", 0, "whole", sb.PLANTED_CAM), ("state machine, quarters", 0, "quarters", sb.PLANTED_CAM),
             ("state machine, cells", 0, "cells", CAM_AXIS), ("lean kernel, whole blocks", 2, "whole", sb.PLANTED_CAM),
             ("lean kernel, quarters", 2, "quarters", sb.PLANTED_CAM)]


@pytest.mark.parametrize("case", TIE_CASES, ids=[c[0] for c in TIE_CASES])
def test_ties_are_not_decided_with_a_bound(world, case):
    """The tie scene of shadow_bound_ref.py: light E on the root's centre line, fans of triangles with a vertex at the
    light in the four cells around that edge.  tests/test_shadow_bound_cpu.py shows on the same scene, camera and lights
    that 397 of 35 821 shadow iterations meet a tie that brings a hit and are repeated without a bound, and that a
    walk which decided them with the bound takes the wrong branch of mythtracer.cc:109-118 on eight.  Here the lanes
    that get kTraceRedo go through MODE_SHADOW_AGAIN -- with whole blocks, in four-lane rounds (quarters, cells: five
    lights, two rounds per pixel) and in the lean kernel: the frames and the ray counts must be the oracle's."""
    name, lean, forms, cam = case
    want = oracle_frame(world, "tie", cam, sb.TIE_LIGHTS)
    abi = M.hip_abi()
    h = new_scene(world["flat"]["tie"], sb.TIE_LIGHTS, 1, lean)
    try:
        abi.set_tuning(h, "QUAD_SHARE", FORMS[forms][0])
        abi.set_tuning(h, "SM_CELL_SHARE", FORMS[forms][1])
        for knob in (0, 2):
            got, ran_lean = frames_off(h, cam, knob)  # (knob 1 is knob 2 with the counters off)
            for i, f in enumerate(got):
                assert np.array_equal(f, want["rgb"]), (name, knob, i, int((f != want["rgb"]).any(axis=2).sum()))
            assert ran_lean == (lean == 2), name
            for i, f in enumerate(frames_on(h, cam, knob)):
                assert np.array_equal(f["rgb"], want["rgb"]), (name, knob, i)
                assert {k: f["stats"][k] for k in RAY_KEYS} == {k: want["counters"][k] for k in RAY_KEYS}, (name, knob, i)
    finally:
        abi.scene_destroy(h)


def test_the_hybrid_launch_bounds_its_state_machine_part(world):
    """Engine 3 at 96x64 hands every unit to the ray pool, whose records carry no bound.  At 480x270 the state machine
    gets most of the frame's units: under the mid-room light the node visits at knob 2 must lie strictly below knob 0's."""
    size = (480, 270)
    want = oracle_frame(world, "mini", scenegen.ROOM_CAMERA, sb.MID_LIGHT, size)
    abi = M.hip_abi()
    h = new_scene(world["flat"]["mini"], sb.MID_LIGHT, 3, 1)
    try:
        on = {knob: frames_on(h, scenegen.ROOM_CAMERA, knob, n=3, size=size) for knob in (0, 2)}
        for knob, fs in on.items():
            for i, f in enumerate(fs):
                assert np.array_equal(f["rgb"], want["rgb"]), (knob, i)
                assert {k: f["stats"][k] for k in RAY_KEYS} == {k: want["counters"][k] for k in RAY_KEYS}, (knob, i)
        v0, v2 = on[0][-1]["stats"]["node_visits"], on[2][-1]["stats"]["node_visits"]
        print("hybrid, mini, mid-room light, 480x270: node visits %d at knob 0, %d at knob 2 (%.3f)" % (v0, v2, v2 / v0))
        assert v2 < v0
    finally:
        abi.scene_destroy(h)
