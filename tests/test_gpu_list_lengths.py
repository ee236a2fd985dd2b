"""The walk's and the ordered descent's scans of a node's own list at every length boundary of their data layout, on a
real MI355X (-m gpu).

tests/list_lengths.py plants a root list of exactly L and a child list of exactly L2 triangles (L2 begins at stream
position L) and aims rays so that each depends on ONE list entry: whatever entry a scan drops -- the last of a
33-long list, the seventh live super of a round, the one entry of a list's 29th super, the entries of a clipped first
block -- is some ray's wrong answer.  tests/test_list_lengths_cpu.py asserts the construction.  The reference for every
comparison is the oracle, by the rule of test_gpu_boundary_rays.compare; DESIGN 3.1.2 has the lengths and which planted
mistake fails which case.
"""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import list_lengths as ll  # noqa: E402
import orclib  # noqa: E402

import mythtracer_amd as M  # noqa: E402
from test_gpu_boundary_rays import ALL_MODES, compare, device_scene  # noqa: E402
from test_gpu_parity import _render_both  # noqa: E402

IDS = ["%d-%d%s" % (l, l2, "-tie" if tie else "") for l, l2, tie in ll.CASES]


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"
    t0 = time.time()
    yield
    print("test_gpu_list_lengths.py: %.1f s wall" % (time.time() - t0))


@pytest.fixture(params=["state_machine", "ray_pool", "hybrid", "auto"])
def engine(request):
    """The frame tests run through the frame engines and the automatic choice (mt_scene_set_engine), selected through
    the API for the scenes created from now on."""
    abi = M.hip_abi()
    abi.set_default_engine({"state_machine": 1, "ray_pool": 2, "hybrid": 3, "auto": 0}[request.param])
    yield request.param
    abi.set_default_engine(0)


def check(c, what, layout=None):
    """Modes 0-7 against the oracle.  The sharp assertion is compare's first: the line of every aimed ray is its own
    triangle (c["want"]["line"] is c["own"]: asserted by the callers, and on the CPU), and the message of a wrong one
    names the list position, the list length and the ray order."""
    m = device_scene(c["tris"])
    if layout is not None:
        M.hip_abi().set_tuning(m.device_scene(), "DEEP_LAYOUT", float(layout))
    compare(m, c["rays"], c["want"], ALL_MODES, what=what, describe=lambda r: ll.describe(c, r))


@pytest.mark.parametrize("l,l2,tie", ll.CASES, ids=IDS)
def test_aimed_rays_at_list_length_boundaries(l, l2, tie):
    """Root list of l, child list of l2 at stream position l; every list position under rays of three kinds (oblique;
    two zero direction components; one) in list order, strided over the list, alone in their wave, and a few irregular
    lanes among regular ones: modes 0-7 against the oracle."""
    c = ll.case(l, l2, tie)
    assert np.array_equal(c["want"]["line"], c["own"])
    check(c, "lists %d / %d%s" % (l, l2, " with ties" if tie else ""))


@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("l,l2,levels", ll.DEEP)
def test_planted_lists_inside_a_deep_tree(l, l2, levels, layout):
    """The same lists in a tree of 12 levels (one frame level in global memory) and of 17 (DEEP = 2), both layouts."""
    c = ll.case(l, l2, False, levels)
    assert c["tree"]["depth"] == levels and np.array_equal(c["want"]["line"], c["own"])
    check(c, "lists %d / %d, %d levels, layout %d" % (l, l2, levels, layout), layout)


FRAME_CAM = (34.0, 33.0, -40.0, 0.0, 0.0, 0.0, 60.0)
FRAME_LIGHTS = [(20.0, 100.0, 5.0, .2, .2, .2, .8, .8, .8, .4, .4, .4)]


@pytest.mark.parametrize("l,l2", ll.FRAMES)
def test_frames_over_planted_lists(l, l2, engine):
    """One 64 x 48 frame at depth 5 over the planted lists, one material of reflectance 0.2, one light: the frame
    kernels are other instantiations of the same walk, and their shadow and secondary rays start on the lists."""
    tris = ll.scene(l, l2)
    m, o = M.MythTracer(), orclib.OracleScene()
    for s in (m, o):
        s.add_material("a", (.2, .2, .2), (.7, .6, .5), (.3, .3, .3), ns=6, refl=0.2)
        for k, v in enumerate(tris):
            s.add_triangle(v, None, mtl=0, line_no=k)
    g = _render_both(m, o, FRAME_CAM, 64, 48, FRAME_LIGHTS)
    on_root = ((g["line"] >= 0) & (g["line"] < l)).mean()
    on_child = ((g["line"] >= l) & (g["line"] < l + l2)).mean()
    print("lists %d / %d (%s): %.1f %% of the pixels on the root list, %.1f %% on child 0's, %d secondary and %d "
          "shadow rays" % (l, l2, engine, 100 * on_root, 100 * on_child, g["counters"]["rays_secondary"],
                           g["counters"]["rays_shadow"]))
    assert on_root >= 0.03 and on_child >= 0.03 and g["counters"]["rays_secondary"] > 0
