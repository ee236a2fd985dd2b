"""The light moves of the ray-tree update tests (mt_raytree_update_lights), shared by tests/test_raytree_update_cpu.py --
which shows with the oracle alone that the moves are worth testing at DEPTH -- and tests/test_gpu_raytree_update.py.
Test infrastructure.

No new restatement: the updated tree is raytree_ref.build(..., lights B), and a moved light's planes in a layer are
lightbuffer_ref.shadow_loops from that layer's stored point and lit mask.

Per scene: the light set A (lightbuffer_ref's), the index of the light that moves, and its new position -- the moves of
lightupdate_ref for cornell, f2_decal, mini and room, and the same move of the bench's light 1 for two_way.
"""
import numpy as np

import lightbuffer_ref as lr
import lightupdate_ref as lu
import raytree_ref as rr

W, H = 96, 54
OFF_GRID = lu.OFF_GRID
CHUNKS = (None, OFF_GRID)
MOVES = dict(lu.MOVES, two_way=("bench", 1, (150.0, 120.0, 250.0)))
SCENES = ["cornell", "f2_decal", "mini", "room", "two_way"]
DEEP_SCENES = ("mini", "room", "two_way")  # the moved light's in_shadow changes in layers >= 1
UNCHANGED_PLANES = ("ray", "coef", "in_object", "point", "normal", "albedo", "material", "child_refl", "child_refr")


def obj_of(scenes, name):
    return rr.TWO_WAY if name == "two_way" else scenes[name]


def lights_before_and_after(scene):
    """(A, B, index of the moved light) for a scene of MOVES."""
    key, index, position = MOVES[scene]
    a = [tuple(float(v) for v in l) for l in lr.light_sets(scene)[key]]
    return a, lu.moved(a, index, position), index


def lit_of(lay):
    """The rays of a restated layer whose loops the update runs, from the planes it reads."""
    return ~np.isnan(lay["point"][:, 0]) & (lay["material"] >= 0)


def same_plane(a, b):
    """Bit identity of two planes: doubles as uint64 (NaN = NaN), everything else by value."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        return not ((a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))).any()
    return np.array_equal(a, b)
