"""Texture edits in place, the parts that need no GPU (include/mythtracer_hip.h, mt_scene_set_texture ff.).

a. The symbols exist, the ABI version is still 5, mt_raytree_layer is still 12 pointers, and every argument check that can
   be reached without a device -- a scene cannot be created without one, so: the NULL scene and the NULL tree of every
   new call, and ALL checks of mt_retexture_gbuffer[_device], whose scene comes last -- is refused with its code and
   message, in the documented order.  (The checks behind a live scene -- the texture index, the NULL mt_texture, the size
   and format -- are in tests/test_gpu_texture_edit.py.)  The facade's shim refuses an unknown texture key itself.
b. tests/texture_edit_ref.py restates albedo = ambient * Texture::GetColorAt(u, v) in numpy.  It is pinned to the oracle
   (orclib.OracleScene.tex_color_at) bit for bit on the textures of the tiny scene and on the replacement textures --
   1 x 1, 2 x 2, 3 x 5 -- for several hundred (u, v): outside [0, 1), negative, exactly 0 and 1, tiny negatives that
   become exactly 1, +-1e300, -0.0 and NaN; and to the oracle's G-buffer albedo (gbuffer_ref.oracle_gbuffer) on the tiny
   scene, whose floor has texture coordinates from -0.5 to 2 and a triangle with NaN ones.
c. The tiny scene shows what the GPU tests need of it: every material in its tree, a hit with NaN uvw, children of both
   kinds.
"""
import ctypes

import numpy as np
import pytest

import gbuffer_ref
import orclib
import raytree_ref as rr
import texture_edit_ref as te
from gbuffer_ref import same_bits

import mythtracer_amd as M
from mythtracer_amd import binding

MT_ERR_ARG, MT_ERR_HIP = -1, -2
SYMBOLS = ("mt_scene_set_texture", "mt_scene_get_texture_info", "mt_scene_set_raytree_uvw", "mt_raytree_read_uvw",
           "mt_raytree_keeps_uvw", "mt_retexture_gbuffer", "mt_retexture_gbuffer_device")


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    return native_libs


# ---- a. symbols, argument checks, facade

def test_symbols_abi_version_and_the_layer_struct():
    abi = M.hip_abi()
    assert binding.MT_ABI_VERSION == 5 == abi.lib.mt_abi_version()
    for name in SYMBOLS:
        assert name in M.HIP_SYMBOLS and getattr(abi.lib, name) is not None
    for name in ("mth_update_texture", "mth_set_raytree_keep_uvw"):
        assert getattr(M.host_lib(), name) is not None
    assert ctypes.sizeof(binding.mt_raytree_layer) == 12 * ctypes.sizeof(ctypes.c_void_p)
    assert "uvw" not in binding.RAYTREE_PLANES
    for fn in (abi.set_texture, abi.get_texture_info, abi.set_raytree_uvw, abi.raytree_read_uvw, abi.raytree_keeps_uvw,
               abi.retexture_gbuffer, abi.retexture_gbuffer_device, binding.MythTracer.update_texture,
               binding.MythTracer.set_raytree_keep_uvw):
        assert callable(fn)


def _refused(abi, rc, message):
    assert rc == MT_ERR_ARG and rc != MT_ERR_HIP, (rc, abi.last_error())
    assert abi.last_error() == message, abi.last_error()


def test_a_null_scene_or_tree_is_refused_before_any_device_call():
    abi = M.hip_abi()
    texels = np.zeros((2, 2, 3), dtype=np.uint8)
    good = binding.mt_texture(2, 2, binding.MT_TEX_RGB8, 0, texels.ctypes.data)
    bad = binding.mt_texture(0, -1, 7, 0, None)
    # the scene comes first: its message wins over everything about the index and the texture
    for index in (0, -1, 10 ** 6):
        for tex in (good, bad, None):
            _refused(abi, abi.lib.mt_scene_set_texture(None, index, ctypes.byref(tex) if tex is not None else None),
                     "scene is NULL")
            _refused(abi, abi.lib.mt_scene_get_texture_info(None, index, ctypes.byref(tex) if tex is not None else None),
                     "scene is NULL")
    for keep in (0, 1, 2, -1):
        _refused(abi, abi.lib.mt_scene_set_raytree_uvw(None, keep), "scene is NULL")
    out = np.zeros((4, 3))
    for layer in (0, -1, 99):
        for o in (out.ctypes.data, None):
            _refused(abi, abi.lib.mt_raytree_read_uvw(None, layer, o), "the ray tree is NULL")
    rc = abi.lib.mt_raytree_keeps_uvw(None)
    assert rc < 0
    _refused(abi, rc, "the ray tree is NULL")
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.set_texture(None, 0, texels)
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.get_texture_info(None, 0)
    with pytest.raises(RuntimeError, match="scene is NULL"):
        abi.set_raytree_uvw(None, True)
    with pytest.raises(RuntimeError, match="ray tree is NULL"):
        abi.raytree_keeps_uvw(None)
    with pytest.raises(ValueError, match="uint8 or float64"):
        abi.set_texture(None, 0, np.zeros((2, 2, 3), dtype=np.float32))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_retexture_checks_in_order_before_any_device_call(device):
    """gb NULL; material or albedo missing; (uvw missing where needed: it needs a scene to ask, so a NULL scene passes
    it); chunk_w / chunk_h outside 1 .. 100000; then the scene."""
    abi = M.hip_abi()
    fn = abi.lib.mt_retexture_gbuffer_device if device else abi.lib.mt_retexture_gbuffer
    m = np.zeros((2, 2), dtype=np.int32)
    a = np.zeros((2, 2, 3))
    u = np.zeros((2, 2, 3))
    full = binding.mt_gbuffer(material=m.ctypes.data, albedo=a.ctypes.data, uvw=u.ctypes.data)
    _refused(abi, fn(None, 0, 0, None, None), "the mt_gbuffer is NULL")
    needs = "the retexture needs the material and albedo planes of the mt_gbuffer"
    for g in (binding.mt_gbuffer(), binding.mt_gbuffer(material=m.ctypes.data), binding.mt_gbuffer(albedo=a.ctypes.data),
              binding.mt_gbuffer(uvw=u.ctypes.data, point=a.ctypes.data)):
        _refused(abi, fn(None, 0, 0, ctypes.byref(g), None), needs)
    for cw, ch in ((0, 2), (2, 0), (-1, 2), (2, 100001), (100001, 2)):
        _refused(abi, fn(None, cw, ch, ctypes.byref(full), None), "chunk size %dx%d out of range" % (cw, ch))
    no_uvw = binding.mt_gbuffer(material=m.ctypes.data, albedo=a.ctypes.data)
    for g in (full, no_uvw):
        _refused(abi, fn(None, 2, 2, ctypes.byref(g), None), "scene is NULL")
    if not device:
        with pytest.raises(RuntimeError, match="scene is NULL"):
            abi.retexture_gbuffer(None, dict(material=m, uvw=u))
        with pytest.raises(ValueError, match="'material'"):
            abi.retexture_gbuffer(None, dict(uvw=u))


def test_facade_refuses_before_it_needs_a_device():
    m = M.MythTracer()
    te.build_tiny(m)
    m.set_raytree_keep_uvw(True)   # before the upload: remembered, no device needed
    m.set_raytree_keep_uvw(False)
    assert not m.L.mth_update_texture(m.h, b"no such texture", 1, 1, np.zeros(3).ctypes.data)
    assert m.last_error() == "no texture named no such texture"
    assert not m.L.mth_update_texture(m.h, None, 0, 0, None)
    assert m.last_error() == "the texture key is NULL"
    assert not m.L.mth_update_texture(m.h, b"tex0", 0, 3, np.zeros(3).ctypes.data)
    assert m.last_error() == "texture size out of range"
    with pytest.raises(ValueError, match="height, width, 3"):
        m.update_texture("tex0", np.zeros((2, 2)))


# ---- b. the restatement, pinned to the oracle

@pytest.fixture(scope="module")
def tiny_oracle():
    orc = te.build_tiny(orclib.OracleScene())
    orc.finalize()
    return orc


def _pin(texels, u, v, what):
    """color_at against an oracle scene that holds `texels` as its texture 0, for every (u, v)."""
    orc = orclib.OracleScene()
    orc.add_texture("t", te.texel_values(texels))
    want = np.array([orc.tex_color_at(0, a, b) for a, b in zip(u, v)])
    got = te.color_at(texels, u, v)
    assert same_bits(got, want, what) == 0
    return got


def test_color_at_is_the_oracles_on_every_texture_and_edge():
    u, v = te.edge_uv()
    assert len(u) > 600 and np.isnan(u).any() and (u == 1.0).any() and (u < 0).any() and (u > 1).any() and (u == 0).any()
    floor, wall, spare = te.tiny_textures()
    textures = dict(te.replacements(floor), wall=wall, spare=spare)
    assert textures["3x5_f64"].shape == (5, 3, 3) and textures["3x5_f64"].dtype == np.float64
    assert textures["1x1"].shape == (1, 1, 3) and textures["2x2"].shape == (2, 2, 3)
    for name, texels in textures.items():
        got = _pin(texels, u, v, name)
        nan = np.isnan(u) | np.isnan(v)
        assert np.isnan(got[nan]).all() and not np.isnan(got[~nan]).any(), name
    # the clamp of the last column and row IS hit: v exactly 0 is the last row, a tiny negative u the last column
    t = te.texel_values(textures["3x5_f64"])
    assert np.array_equal(te.color_at(t, [0.0], [0.0])[0], t[4, 0])
    assert np.array_equal(te.color_at(t, [-2.0 ** -60], [0.0])[0], t[4, 2])
    assert np.array_equal(te.color_at(t, [-2.0 ** -60], [0.5])[0], t[2, 2])
    # a 1 x 1 texture is its texel everywhere
    one = te.texel_values(textures["1x1"])[0, 0]
    assert (te.color_at(textures["1x1"], u[~nan], v[~nan]) == one).all()


def test_albedo_is_the_oracles_gbuffer_on_the_tiny_scene(tiny_oracle):
    W, H = te.TINY_IMAGE
    want = gbuffer_ref.oracle_gbuffer(tiny_oracle, te.TINY_CAMERA, W, H)
    mats = [dict(values=v, tex=t) for _, v, t in tiny_oracle.materials()]
    assert [m["tex"] for m in mats] == [0, 1, -1, -1, -1]
    got = te.albedo(mats, te.tiny_textures()[:2], want["material"], want["uvw"].reshape(-1, 3)).reshape(H, W, 3)
    assert same_bits(got, want["albedo"], "restated albedo vs the oracle's G-buffer") == 0
    hit = want["material"] >= 0
    uv = want["uvw"][hit][:, :2]
    print("hits %d, u in [%g, %g], NaN uvw at %d hits" % (hit.sum(), np.nanmin(uv), np.nanmax(uv), np.isnan(uv[:, 0]).sum()))
    assert np.nanmin(uv) < 0.0 and np.nanmax(uv) > 1.0 and np.isnan(uv[:, 0]).any()
    # NaN coordinates at a hit of a textured material: a NaN albedo
    nan_hit = hit & np.isnan(want["uvw"][..., 0])
    assert (want["material"][nan_hit] == te.FLOOR).all() and np.isnan(got[nan_hit]).all()


# ---- c. the tiny scene has what the GPU tests need

def test_the_tiny_scene_shows_every_material_and_both_kinds_of_children(tiny_oracle):
    W, H = te.TINY_IMAGE
    tree = rr.build(tiny_oracle, te.TINY_CAMERA, W, H, te.TINY_LIGHTS, te.TINY_DEPTH)
    print("rays per layer %s" % tree["n_rays"])
    assert len(tree["n_rays"]) >= 3 and tree["n_rays"][1] > 64
    seen = set()
    for lay in tree["layers"]:
        seen.update(int(m) for m in np.unique(lay["material"]))
    assert seen >= {-1, te.FLOOR, te.WALL, te.MIRROR, te.PANE, te.MATTE}, seen
    l0 = tree["layers"][0]
    assert (l0["child_refl"] >= 0).any() and (l0["child_refr"] >= 0).any()
    # textured materials are hit in the deeper layers too: a retexture has work below layer 0
    assert np.isin(tree["layers"][1]["material"], (te.FLOOR, te.WALL)).any()
