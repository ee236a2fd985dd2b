"""The shadow rays' distance bound without a GPU: tests/native/shadow_bound_check.cc, a stand-alone program around
mythtracer_amd/csrc/mt_shadow_bound.h, built with the address and undefined-behaviour sanitizers (their runtimes linked
statically) and run as a program of its own.  (a) the two facts about the reference's Moeller-Trumbore arithmetic that
the bound's constants rest on, and mu's inequality, on adversarial triangle/ray pairs; (b) a recursive port of the
reference's traversal, every shadow iteration of a depth-5 recursion once with the bound emptying subtrees and once
without: `mini` at 96x64 under the bench's lights and under a light at mid-room, the planted scene of
shadow_bound_ref.py, a description with a triangle poking out of its cell, which must get no bound, and the TIE scene,
which must repeat iterations -- and must FAIL the port when its tie handling is switched off.  Then the knob's entry
point, which needs no device."""
import os
import subprocess

import numpy as np
import pytest

import shadow_bound_ref as sb

import mythtracer_amd as M
from mythtracer_amd import binding, build, scenegen

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    return native_libs


@pytest.fixture(scope="module")
def dumps(scenes, tmp_path_factory):
    d = tmp_path_factory.mktemp("shadow_bound")
    mini = M.MythTracer(scenes["mini"]).flatten()
    planted = M.MythTracer()
    sb.fill(planted)
    planted = planted.flatten()
    poked, _ = sb.poking(planted)
    tie = M.MythTracer()
    sb.fill(tie, sb.tie_triangles())
    tie = tie.flatten()
    assert tie["node_center"][0][0] == sb.S / 2 and tie["node_center"][0][2] == sb.S / 2  # light E is ON the root's centre line
    room_sensor = binding.sensor(scenegen.ROOM_CAMERA, sb.W, sb.H)
    return [sb.dump(mini, room_sensor, scenegen.ROOM_LIGHTS, str(d / "mini_bench_lights.bin")),
            sb.dump(mini, room_sensor, sb.MID_LIGHT, str(d / "mini_mid_light.bin")),
            sb.dump(planted, binding.sensor(sb.PLANTED_CAM, sb.W, sb.H), sb.PLANTED_LIGHTS, str(d / "planted.bin")),
            sb.dump(poked, binding.sensor(sb.PLANTED_CAM, sb.W, sb.H), sb.PLANTED_LIGHTS, str(d / "planted_poking.bin")),
            sb.dump(tie, binding.sensor(sb.PLANTED_CAM, sb.W, sb.H), sb.TIE_LIGHTS, str(d / "planted_tie.bin"))]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shadow_bound_exe") / "shadow_bound_check")
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(build.HIPCC)), "include")  # (mt_device.h includes hip_runtime.h)
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Wextra",
                         "-D__HIP_PLATFORM_AMD__", "-I", rocm_inc, "-I", build.INC, "-I", build.CSRC, "-o", exe,
                         os.path.join(HERE, "native", "shadow_bound_check.cc")],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert cc.returncode == 0, cc.stdout.decode()
    return exe


def test_shadow_bound_check(exe, dumps):
    r = subprocess.run([exe] + dumps, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    print(r.stdout.decode())
    assert r.returncode == 0, r.stdout.decode()
    assert "all checks held" in r.stdout.decode()


def test_the_tie_scene_fails_a_port_that_decides_ties_with_a_bound(exe, dumps):
    """The same program with the tie handling of DESIGN 3.1.3 item 4 switched off in the port (no look at the children
    at a candidate's key, no repetition): on the tie scene the bounded run must then take another branch of
    mythtracer.cc:109-118 than the reference -- the scene constructs the hazard, the handling is what removes it."""
    tie = [p for p in dumps if p.endswith("planted_tie.bin")]
    r = subprocess.run([exe, "--without-tie-handling"] + tie, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 1 and "the loop takes branch" in out and "planted_tie.bin" in out


def test_planted_scene_is_what_its_name_promises():
    tris = sb.planted_triangles()
    assert 700 <= len(tris) <= 1200
    v = np.array([t[0] for t in tris])
    assert v.min() >= -6.0 and v.max() <= sb.S + 6.0  # (the clutter may reach through a wall)
    assert {t[1] for t in tris} == {0, 1, 2}
    for name, dy in (("A", 0.0), ("B", -1e-6), ("C", 1e-6)):
        x, z = sb._LIGHT_XZ[name]
        near = [t for t in v if np.all(t[:, 1] == sb.LIGHT_Y + dy) and abs(t[:, 0].mean() - x) < 1 and abs(t[:, 2].mean() - z) < 1]
        assert len(near) == 1, name


def test_the_knob_is_refused_without_a_scene_and_outside_its_values():
    abi = M.hip_abi()
    assert binding.TUNE_EXTRA == {"SHADOW_BOUND": 1000} and not set(binding.TUNE_EXTRA) & set(binding.TUNE)
    assert abi.lib.mt_scene_set_tuning(None, binding.TUNE_EXTRA["SHADOW_BOUND"], 1.0) == -1
    assert "MT_TUNE_SHADOW_BOUND 1000" in open(os.path.join(build.INC, "mythtracer_hip.h")).read()
