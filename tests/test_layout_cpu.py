"""mt_layout.h on the CPU: tests/native/layout_check.cc, a stand-alone program around the header that checks
check_scene_desc's refusals word for word and every array of derive_layout (sizes, paddings, unions, quads, sorted
lists) against brute-force restatements, at the list lengths of tests/list_lengths.py.  Built with the address and
undefined-behaviour sanitizers (their runtimes linked statically, so the program does not depend on the order in which
the loader brings libraries) and run as a program of its own: nothing of it is loaded into Python, and no GPU is
needed."""
import os
import subprocess

from mythtracer_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))


def test_layout_check(tmp_path):
    exe = str(tmp_path / "layout_check")
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(build.HIPCC)), "include")  # (mt_device.h includes hip_runtime.h)
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__",
                         "-I", rocm_inc, "-I", build.INC, "-I", build.CSRC,
                         "-o", exe, os.path.join(HERE, "native", "layout_check.cc")],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert cc.returncode == 0, cc.stdout.decode()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    print(r.stdout.decode())
    assert r.returncode == 0, r.stdout.decode()
    assert "all checks held" in r.stdout.decode()
