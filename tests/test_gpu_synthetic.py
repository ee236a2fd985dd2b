"""The kernels that trace nothing on inputs no scene produces, on a real MI355X (-m gpu): refine_mask_kernel /
refine_compact_kernel past 1024 blocks, shade_direct_kernel on planes of tests/synthetic_inputs.py, both relight kernels
under light colours no scene file holds, resolve_kernel<2 .. 4> on chosen samples, tile_cost_kernel / tile_order_kernel /
deal_tiles_kernel on chosen cost maps.

The expected values are the numpy restatements the other tests pin to the oracle and the reference (mythtracer_amd/
tiling.py, tests/lightbuffer_ref.py, tests/raytree_ref.py); tests/test_synthetic_cpu.py holds them, and the inputs, to
plain Python arithmetic.  The bar is identity.  pow is the one operation whose GPU implementation is not glibc's: the
pixels for which the restatement takes the specular branch carry test_gpu_parity.py's assert_rgb_close rule among
themselves (1 LSB on at most max(1, n // 10000) of them), every other pixel zero differing bytes.  Every test prints its
counts.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gbuffer_ref  # noqa: E402
import lightbuffer_ref as lr  # noqa: E402
import orclib  # noqa: E402
import raytree_ref as rr  # noqa: E402
import synthetic_inputs as si  # noqa: E402

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding, tiling  # noqa: E402

RELIGHT = binding.RELIGHT_GBUFFER_PLANES
THRESHOLD = 16


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"


@pytest.fixture
def scene(scenes):
    """A scene handle for the calls that need one for its device and its scratch buffers only."""
    abi = M.hip_abi()
    h = abi.scene_create(M.MythTracer(scenes["cornell"]).flatten())
    yield abi, h
    abi.scene_destroy(h)


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def split_compare(got, want, specular, what):
    """Zero differing bytes among the pixels off the specular branch; assert_rgb_close's rule among those on it.
    Returns (differing bytes of the exact group, differing pixels of the pow group)."""
    exact = ~specular
    n_bytes = int((got[exact] != want[exact]).sum())
    d = np.abs(got[specular].astype(np.int16) - want[specular].astype(np.int16))
    n_px = int((d != 0).any(axis=-1).sum())
    print("%s: exact group %d of %d bytes differ; pow group %d of %d pixels differ, max |diff| %d"
          % (what, n_bytes, 3 * int(exact.sum()), n_px, int(specular.sum()), int(d.max(initial=0))))
    assert n_bytes == 0, what
    assert d.max(initial=0) <= 1, what
    assert n_px <= max(1, int(specular.sum()) // 10000), what
    return n_bytes, n_px


# ---- 1. the block list past 1024 blocks

@functools.lru_cache(maxsize=None)
def mask_case(W, H, chunk):
    """name -> (bitmap, mask, list) by tiling.refine_mask, made once."""
    chunk_ = chunk or (0, 0, W, H)
    return {name: (f,) + tiling.refine_mask(f, W, H, chunk_, THRESHOLD) for name, f in si.mask_frames(W, H, chunk).items()}


@pytest.mark.parametrize("W,H,chunk", si.MASK_GEOMETRIES)
def test_block_list_past_1024_blocks(W, H, chunk, scene):
    """mt_refine_mask_device where a thread of refine_compact_kernel owns more than one flag (and, at 1023 .. 1025
    blocks, where it begins to): count, list, the list's untouched tail and the mask, with and without a mask."""
    import torch
    abi, h = scene
    chunk_, (_, _, mw, mh), n, per = si.mask_geometry(W, H, chunk)
    n_diff = 0
    for name, (f, want_mask, want_list) in mask_case(W, H, chunk).items():
        d_rgb = torch.from_numpy(f).cuda()
        want_full = np.concatenate([want_list, np.full(n - len(want_list), -7, dtype=np.int32)])
        for with_mask in (True, False):
            d_mask = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
            d_list = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            d_count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            abi.refine_mask_device(h, W, H, chunk_, THRESHOLD, vp(d_rgb), vp(d_mask) if with_mask else None, vp(d_list), vp(d_count))
            torch.cuda.synchronize()
            what = (name, W, H, chunk, with_mask)
            count, got_list, got_mask = int(d_count.cpu()[0]), d_list.cpu().numpy(), d_mask.cpu().numpy()
            want_m = want_mask.astype(np.uint8).reshape(-1) if with_mask else np.full(n, 9, dtype=np.uint8)
            n_diff += int((got_list != want_full).sum()) + int((got_mask != want_m).sum()) + (count != len(want_list))
            assert count == len(want_list), what
            assert (np.diff(got_list[:count]) > 0).all(), what          # ascending
            assert np.array_equal(got_list[:count], want_list), what
            assert (got_list[count:] == -7).all(), what                 # the untouched tail
            assert np.array_equal(got_mask, want_m), what
    print("%dx%d %s: %d blocks, %d per thread, %d differing elements" % (W, H, chunk, n, per, n_diff))
    assert n_diff == 0


def test_adaptive_frame_past_1024_blocks(scenes):
    """mask -> list -> refinement launch -> refine_resolve_kernel at two flags per thread: test_gpu_adaptive.py's
    contract on a frame of 37 x 35 = 1295 blocks (the automatic engine)."""
    from test_gpu_adaptive import CORNELL_CAM, CORNELL_LIGHTS, check_contract
    abi = M.hip_abi()
    h = abi.scene_create(M.MythTracer(scenes["cornell"]).flatten())
    try:
        abi.set_lights(h, CORNELL_LIGHTS)
        W, H, s = 296, 280, 2
        got, mask = check_contract(abi, h, CORNELL_CAM, W, H, s, THRESHOLD, what=("cornell", s, W, H))
        print("cornell %dx%d ss %d: refined %d of %d" % (W, H, s, mask.sum(), mask.size), got["info"])
        assert mask.size == 1295 and 0 < mask.sum() < mask.size
        assert np.nonzero(mask.reshape(-1))[0].max() >= 1024  # (a flagged block beyond the first 1024)
    finally:
        abi.scene_destroy(h)


# ---- 2. mt_shade_direct on synthetic planes

@functools.lru_cache(maxsize=None)
def shade_rays(image, chunk):
    return gbuffer_ref.pixel_rays(si.SHADE_CAMERA, image[0], image[1], chunk)


@functools.lru_cache(maxsize=None)
def shade_case(image, chunk, n_lights, kind):
    """(gb, lb, lights, the restated frame, the pixels on the specular branch), made once."""
    gb, lb, _, lights = si.shade_case(shade_rays(image, chunk), n_lights, kind)
    info = {}
    with np.errstate(all="ignore"):
        want = lr.shade(None, gb, lb, lights, materials=si.MATERIALS, hit=gb["hit"], info=info)
    return gb, lb, lights, want, info["specular"]


@pytest.fixture
def table_scene(scenes):
    """A scene whose only purpose is its material table: si.MATERIALS in place of the cornell box's four."""
    abi = M.hip_abi()
    flat = dict(M.MythTracer(scenes["cornell"]).flatten())
    assert int(np.max(flat["tri_material"])) < si.N_MATERIALS
    flat["materials"] = [dict(values=v, tex=-1) for v in si.MATERIALS]
    h = abi.scene_create(flat)
    yield abi, h
    abi.scene_destroy(h)


def shade_both_forms(abi, h, image, chunk, gb, lb, lights):
    """mt_shade_direct and mt_shade_direct_device over the same planes."""
    import torch
    W, H = image
    sens = binding.sensor(si.SHADE_CAMERA, W, H)
    host = abi.shade_direct(h, sens, W, H, gb, lb, lights, chunk=chunk)["rgb"]
    dt = dict(point=np.float64, normal=np.float64, albedo=np.float64, material=np.int32)
    d_gb = {n: torch.from_numpy(np.ascontiguousarray(gb[n], dtype=dt[n])).cuda() for n in RELIGHT}
    d_lb = dict(power=torch.from_numpy(np.ascontiguousarray(lb["power"])).cuda(),
                in_shadow=torch.from_numpy(np.ascontiguousarray(lb["in_shadow"])).cuda())
    d_rgb = torch.full((chunk[3], chunk[2], 3), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    abi.shade_direct_device(h, sens, W, H, chunk, {n: t.data_ptr() for n, t in d_gb.items()},
                            {n: t.data_ptr() for n, t in d_lb.items()}, lights, d_rgb.data_ptr())
    torch.cuda.synchronize()
    return host, d_rgb.cpu().numpy()


@pytest.mark.parametrize("n_lights", si.SHADE_LIGHT_COUNTS)
def test_shade_direct_on_synthetic_planes(n_lights, table_scene):
    """Every chunk under the tame lights, the off-grid chunk under every hostile edit too; the host and the device call."""
    abi, h = table_scene
    total_bytes = total_px = 0
    for image, chunk in si.SHADE_CHUNKS:
        for kind in ((None,) + si.HOSTILE_KINDS if chunk == si.OFF_GRID else (None,)):
            gb, lb, lights, want, spec = shade_case(image, chunk, n_lights, kind)
            host, dev = shade_both_forms(abi, h, image, chunk, gb, lb, lights)
            for form, got in (("host", host), ("device", dev)):
                b, p = split_compare(got, want, spec, "%s %s %d lights %s %s" % (image, chunk, n_lights, kind, form))
                total_bytes += b
                total_px += p
            assert (host[~gb["hit"]] == 0).all()  # a miss is black whatever the other planes hold
    print("%d lights: %d differing bytes in the exact groups, %d differing pixels in the pow groups" % (n_lights, total_bytes, total_px))
    # the same planes at another place of the image are other rays: other bytes
    at_offset = shade_case(si.SHADE_IMAGE, si.OFF_GRID, n_lights, None)
    at_origin = shade_case(si.SHADE_IMAGE, (0, 0, 61, 37), n_lights, None)
    a = shade_both_forms(abi, h, si.SHADE_IMAGE, si.OFF_GRID, *at_offset[:3])[1]
    b = shade_both_forms(abi, h, si.SHADE_IMAGE, (0, 0, 61, 37), *at_origin[:3])[1]
    assert (a != b).any(axis=-1).mean() > 0.1


# ---- 3. hostile light colours for both relight kernels

W3, H3 = 61, 37
DEPTHS = (0, 2)


@functools.lru_cache(maxsize=None)
def relight_reference(obj, name):
    """The restated planes and trees of a scene under its tame lights, made once: (oracle, gb, lb, {depth: tree})."""
    orc = orclib.OracleScene(obj)
    cam = rr.CAMERAS[name]
    gb = gbuffer_ref.oracle_gbuffer(orc, cam, W3, H3)
    base, _ = si.relight_base(name, lr.BENCH_LIGHTS, lr.ONE_LIGHT["cornell"])
    lb = lr.ref_lightbuffer(orc, gb, base)
    deep = rr.build(orc, cam, W3, H3, base, max(DEPTHS))
    return orc, gb, lb, {d: rr.truncated(deep, d) for d in DEPTHS}


@pytest.mark.parametrize("name", ["cornell", "two_way"])
def test_hostile_light_colours(name, scenes):
    """Planes and trees made once under the scene's tame lights; mt_shade_direct and mt_raytree_shade under every
    hostile edit of one light against the restatements, and against a fresh mt_render_chunk under the same lights."""
    obj = rr.TWO_WAY if name == "two_way" else scenes[name]
    orc, gb, lb, trees = relight_reference(obj, name)
    base, which = si.relight_base(name, lr.BENCH_LIGHTS, lr.ONE_LIGHT["cornell"])
    cam = rr.CAMERAS[name]
    sens = binding.sensor(cam, W3, H3)
    abi = M.hip_abi()
    h = abi.scene_create(M.MythTracer(obj).flatten())
    made = []
    total_bytes = total_px = 0
    try:
        abi.set_lights(h, base)
        b = abi.render_lightbuffer(h, sens, W3, H3, len(base), gbuffer_channels=RELIGHT)
        for d in DEPTHS:
            made.append(abi.raytree_create(h, sens, W3, H3, max_depth=d)[0])
        value = si.stored_power_value(lb["power"][which])
        assert (b["power"][which] == value).any()
        for kind in si.HOSTILE_KINDS:
            new = si.hostile_lights(base, kind, which=which, power_value=value)
            abi.set_lights(h, new)  # (neither shade reads the scene's lights; the fresh frames do)
            info = {}
            with np.errstate(all="ignore"):
                want = lr.shade(orc, gb, lb, new, info=info)
            got = abi.shade_direct(h, sens, W3, H3, b, b, new)["rgb"]
            what = "%s %s" % (name, kind)
            nb, npx = split_compare(got, want, info["specular"], what + " mt_shade_direct")
            fresh = abi.render_chunk(h, sens, W3, H3, max_depth=0)["rgb"]
            n_fresh = int((got != fresh).sum())
            print("%s mt_shade_direct vs mt_render_chunk: %d bytes differ" % (what, n_fresh))
            assert n_fresh == 0, what
            total_bytes, total_px = total_bytes + nb, total_px + npx
            for d, t in zip(DEPTHS, made):
                info = {}
                with np.errstate(all="ignore"):
                    want = rr.shade(orc, trees[d], new, W3, H3, info=info)
                got = abi.raytree_shade(t, new)["rgb"]
                nb, npx = split_compare(got, want, info["specular"], "%s mt_raytree_shade depth %d" % (what, d))
                fresh = abi.render_chunk(h, sens, W3, H3, max_depth=d)["rgb"]
                n_fresh = int((got != fresh).sum())
                print("%s mt_raytree_shade depth %d vs mt_render_chunk: %d bytes differ" % (what, d, n_fresh))
                assert n_fresh == 0, (what, d)
                total_bytes, total_px = total_bytes + nb, total_px + npx
        print("%s: %d differing bytes in the exact groups, %d differing pixels in the pow groups" % (name, total_bytes, total_px))
    finally:
        for t in made:
            abi.raytree_destroy(t)
        abi.scene_destroy(h)


# ---- 4. mt_resolve_tiles_device on synthetic samples

@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("geometry", si.RESOLVE_GEOMETRIES)
def test_resolve_on_synthetic_samples(geometry, s, scene):
    """Every pattern through the strided form and the list form, the destination and the samples 0 .. 3 bytes into
    their tensors; every byte outside the clipped tiles' cw x ch x 3 keeps its 0xA5."""
    import torch
    abi, h = scene
    W, H, tw, th = geometry
    tx, ty = tiling.tile_grid(W, H, tw, th)
    n_diff = launches = 0
    for p, pattern in enumerate(si.RESOLVE_PATTERNS):
        for k, (first, stride, lst, tiles) in enumerate(si.resolve_forms(tx * ty)):
            smp, want = si.resolve_case(pattern, geometry, s, tiles)
            for off_out, off_in in {((p + k) % 4, (p + 2 * k + 1) % 4), ((p + k + 1) % 4, (2 * p + k) % 4)}:
                d_smp = torch.zeros(smp.size + 8, dtype=torch.uint8, device="cuda")
                d_smp[off_in:off_in + smp.size] = torch.from_numpy(smp).cuda()
                d_out = torch.full((want.size + 8,), 0xA5, dtype=torch.uint8, device="cuda")
                d_lst = torch.from_numpy(lst).cuda() if lst is not None else None
                torch.cuda.synchronize()
                abi.resolve_tiles_device(h, W, H, tw, th, first, stride, vp(d_lst) if lst is not None else None, len(tiles), s,
                                         ctypes.c_void_p(d_smp.data_ptr() + off_in), ctypes.c_void_p(d_out.data_ptr() + off_out))
                torch.cuda.synchronize()
                got = d_out.cpu().numpy()
                what = (pattern, geometry, s, first, stride, None if lst is None else lst.tolist(), off_out, off_in)
                launches += 1
                n_diff += int((got[off_out:off_out + want.size] != want).sum())
                assert np.array_equal(got[off_out:off_out + want.size], want), what
                assert (got[:off_out] == 0xA5).all() and (got[off_out + want.size:] == 0xA5).all(), what
    print("%s ss %d: %d launches, %d differing bytes" % (geometry, s, launches, n_diff))
    assert n_diff == 0


# ---- 5. mt_order_tiles_device / mt_deal_tiles_device on synthetic cost maps

@pytest.mark.parametrize("geometry", si.ORDER_GEOMETRIES)
def test_order_and_deal_on_synthetic_cost_maps(geometry, scene):
    import torch
    abi, h = scene
    W, H, tw, th = geometry
    tx, ty = tiling.tile_grid(W, H, tw, th)
    total = tx * ty
    n_diff = 0
    orders = {}
    for kind in si.COST_MAPS:
        m = si.cost_map(kind, geometry)
        want = tiling.order_tiles(m, W, H, tw, th)
        d_map = torch.from_numpy(m.view(np.int32).copy()).cuda()
        d_order = torch.full((total + 4,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        abi.order_tiles_device(h, vp(d_map), m.shape[1], m.shape[0], W, H, tw, th, vp(d_order))
        torch.cuda.synchronize()
        got = d_order.cpu().numpy()
        n_diff += int((got[:total] != want).sum())
        assert np.array_equal(got[:total], want), (kind, geometry)
        assert (got[total:] == -7).all(), (kind, geometry)
        orders[kind] = (d_order, want)
    # the deal: the order of the random map, and no order at all (positions are tile numbers)
    lst = torch.empty((total + 4,), dtype=torch.int32, device="cuda")
    for d_order, want in (orders["random_u32"], (None, None)):
        for world in si.deal_worlds(total):
            owned = []
            for rank in range(world):
                lst.fill_(-7)
                n = abi.deal_tiles_device(h, vp(d_order) if d_order is not None else None, W, H, tw, th, world, rank, vp(lst))
                torch.cuda.synchronize()
                got = lst.cpu().numpy()
                want_list = tiling.deal_tiles(want, total, world, rank)
                what = (geometry, world, rank, d_order is not None)
                assert n == len(want_list) == tiling.dealt_tile_count(total, world, rank) == abi.dealt_tile_count(W, H, tw, th, world, rank), what
                n_diff += int((got[:n] != want_list).sum())
                assert np.array_equal(got[:n], want_list), what
                assert (got[n:] == -7).all(), what
                owned += got[:n].tolist()
            assert sorted(owned) == list(range(total)), (geometry, world)  # every tile has exactly one owner
    print("%s: %d tiles, %d differing elements" % (geometry, total, n_diff))
    assert n_diff == 0
