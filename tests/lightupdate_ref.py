"""The light moves of the light-buffer update tests (mt_update_lightbuffer), shared by tests/test_lightupdate_cpu.py --
which shows with the oracle alone that every move is worth testing -- and tests/test_gpu_lightupdate.py.  Test
infrastructure; the restatement itself is tests/lightbuffer_ref.py (shadow_loops takes a stored point and lit).

Per scene: the light set A (lightbuffer_ref's), the index of the light that moves, and its new position.  cornell,
mini and room keep the moved light inside the scene's bounding box.  f2_decal cannot: the scene is a slab 10 units high
(floor, a pane of glass at y = 10, an opaque decal 5e-6 above it), its own light of lightbuffer_ref.ONE_LIGHT stands at
y = 60, far above the box, and a light below the decal has no opaque surface between it and anything the camera sees,
so in_shadow = 1 could not occur.  The moved light stays above the slab, over its footprint.

Every move has to change in_shadow inside the off-grid chunk of the GPU tests as well as in the whole frame.  cornell's
camera sees the back wall and a strip of floor below the chunk's last row; a light behind the box moves only the
shadow on that strip.  The moved light therefore stands low and in FRONT of the box and throws its shadow up the back
wall, into the chunk.
"""
import lightbuffer_ref as lr

OFF_GRID = (5, 3, 61, 37)  # x, y, w, h at 96x54: neither origin nor size a multiple of 8

MOVES = {
    "cornell": ("one", 0, (40.0, 2.0, 4.0)),
    "f2_decal": ("one", 0, (20.0, 30.0, 20.0)),
    "mini": ("bench", 1, (150.0, 120.0, 250.0)),
    "room": ("bench", 1, (150.0, 120.0, 250.0)),
}
GLASS_SCENES = ("f2_decal", "room")


def moved(lights, index, position):
    """`lights` with the position of light `index` replaced, colours untouched."""
    out = [tuple(float(v) for v in l) for l in lights]
    out[index] = tuple(float(v) for v in position) + out[index][3:]
    return out


def lights_before_and_after(scene):
    """(A, B, index of the moved light) for a scene of MOVES."""
    key, index, position = MOVES[scene]
    a = [tuple(float(v) for v in l) for l in lr.light_sets(scene)[key]]
    return a, moved(a, index, position), index


def lit_of(gb, n_materials=None):
    """The pixels whose loops the update runs, from the planes it reads: point[0] not NaN, 0 <= material < n_materials."""
    import numpy as np
    lit = ~np.isnan(gb["point"][..., 0]) & (gb["material"] >= 0)
    if n_materials is not None:
        lit &= gb["material"] < n_materials
    return lit
