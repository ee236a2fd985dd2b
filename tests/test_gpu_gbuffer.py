"""The primary-hit G-buffer on a real MI355X (-m gpu): mt_render_gbuffer, mt_render_gbuffer_device,
MythTracer::RayTraceGBuffer (include/mythtracer_hip.h; the kernel is mythtracer_amd/csrc/mt_gbuffer.h).

The bar is bit identity, no tolerance: the kernel's arithmetic is the frame kernels' (mt_shade.h, built without FMA
contraction), which already meet it.  depth, point, normal, uvw and line_no are held to goldens the compiled REFERENCE
wrote (tests/golden/gbuffer_*.npz, tests/golden/make_gbuffer_golden.py); prim, material and albedo to the CPU oracle,
whose derivation of them tests/test_gbuffer_cpu.py states and pins (tests/gbuffer_ref.py).  For the textured scene
(room_tex) the oracle's Texture::GetColorAt is itself unpinned -- the reference build has no texture.cc (SDL2), see
`made_by` in tests/golden/frames.json -- so albedo there is identity with the oracle, not with the reference.
f64 planes are compared as uint64 views with NaN = NaN (gbuffer_ref.same_bits); every test prints its counts.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gbuffer_ref  # noqa: E402
import orclib  # noqa: E402
from gbuffer_ref import ALL_PLANES, F64_PLANES, I32_PLANES, same_bits  # noqa: E402

import mythtracer_amd as M  # noqa: E402
from mythtracer_amd import binding, scenegen  # noqa: E402

W, H = 96, 54


@pytest.fixture(scope="module", autouse=True)
def _libs(native_libs):
    assert M.hip_abi().device_count() >= 1, "no GPU visible: the HIP path cannot run"


class Scene:
    def __init__(self, obj):
        self.abi = M.hip_abi()
        self.flat = M.MythTracer(obj).flatten()
        self.h = self.abi.scene_create(self.flat)

    def close(self):
        self.abi.scene_destroy(self.h)

    def gbuffer(self, cam, w, h, chunk=None, channels=None):
        return self.abi.render_gbuffer(self.h, binding.sensor(cam, w, h), w, h, chunk=chunk, channels=channels)


@pytest.fixture
def make(scenes):
    made = []

    def _make(name):
        made.append(Scene(scenes[name]))
        return made[-1]
    yield _make
    for s in made:
        s.close()


def golden_cam(scene):
    return tuple(float(v) for v in gbuffer_ref.load_golden(scene)["cam"])


def assert_planes_equal(got, want, what, planes=ALL_PLANES):
    for p in planes:
        if p in F64_PLANES:
            assert same_bits(got[p], want[p], "%s %s" % (what, p)) == 0, (what, p)
        else:
            n = int((got[p] != want[p]).sum())
            print("%s %s: %d of %d elements differ" % (what, p, n, got[p].size))
            assert n == 0, (what, p)


def expected_material(flat, orc, o):
    """The oracle's material plane in the numbering of the scene description the kernel was given: the material of
    the stream triangle whose AddPrimitive index is the oracle's `prim` -- after checking, by value, that this IS the
    oracle's material of that triangle."""
    pos = np.full(len(flat["tri_id"]), -1, dtype=np.int64)
    pos[flat["tri_id"]] = np.arange(len(flat["tri_id"]))
    values = gbuffer_ref.material_values(orc)
    want = np.full(o["prim"].shape, -1, dtype=np.int32)
    for idx in zip(*np.nonzero(o["prim"] >= 0)):
        dense = int(flat["tri_material"][pos[o["prim"][idx]]])
        om = int(o["material"][idx])
        assert (dense < 0) == (om < 0)
        if dense >= 0:
            assert np.array_equal(flat["materials"][dense]["values"], values[om][0])
            assert (flat["materials"][dense]["tex"] >= 0) == values[om][1]
        want[idx] = dense
    return want


@pytest.mark.parametrize("scene", ["cornell", "mini", "room"])
def test_bit_identity_against_the_reference_made_goldens(scene, make):
    g = gbuffer_ref.load_golden(scene)
    s = make(scene)
    got = s.gbuffer(golden_cam(scene), W, H)
    want = dict(depth=g["t"], point=g["point"], normal=g["normal"], uvw=g["uvw"], line_no=g["line"])
    assert_planes_equal(got, want, "golden " + scene, ("depth", "point", "normal", "uvw", "line_no"))
    miss = g["line"] < 0
    assert np.array_equal(got["prim"] < 0, miss) and np.array_equal(got["material"] < 0, miss)
    assert got["stats"]["rays_primary"] == W * H and got["stats"]["shaded_hits"] == int((~miss).sum())
    assert got["stats"]["kernel_ms"] > 0


@pytest.mark.parametrize("scene", ["cornell", "mini", "room", "room_tex", "mini_nomtl"])
def test_bit_identity_against_the_oracle_for_every_plane(scene, scenes, make):
    """prim, material, albedo (and the five other planes once more) against the oracle.  room_tex: textured, the
    oracle's GetColorAt is unpinned (this file's docstring); mini_nomtl: material = -1 and albedo NaN on every hit."""
    cam = golden_cam(scene) if scene in ("cornell", "mini", "room") else scenegen.ROOM_CAMERA
    orc = orclib.OracleScene(scenes[scene])
    o = gbuffer_ref.oracle_gbuffer(orc, cam, W, H)
    s = make(scene)
    got = s.gbuffer(cam, W, H)
    want = dict(o, material=expected_material(s.flat, orc, o))
    assert_planes_equal(got, want, "oracle " + scene)
    hit = o["prim"] >= 0
    if scene == "mini_nomtl":
        assert hit.any() and (got["material"] == -1).all() and np.isnan(got["albedo"]).all()
        assert not np.isnan(got["normal"][hit]).any()
    if scene == "room_tex":
        textured = np.zeros(hit.shape, dtype=bool)
        textured[hit] = [s.flat["materials"][m]["tex"] >= 0 for m in got["material"][hit]]
        print("room_tex: %d of %d hits on textured materials" % (int(textured.sum()), int(hit.sum())))
        assert textured.any()


def test_agrees_with_the_debug_buffer_and_with_intersect_rays(make):
    """What the project already returns: line_no and point = the debug buffer of mt_render_chunk for the same camera;
    depth and line_no = mt_intersect_rays over the same rays (and its stream index, through tri_id, = prim)."""
    s = make("mini")
    s.abi.set_lights(s.h, scenegen.ROOM_LIGHTS)
    w, h = 101, 67
    cam = scenegen.ROOM_CAMERA
    got = s.gbuffer(cam, w, h)
    frame = s.abi.render_chunk(s.h, binding.sensor(cam, w, h), w, h, debug=True)
    assert np.array_equal(got["line_no"], frame["line"])
    assert same_bits(got["point"], frame["point"], "point vs debug buffer") == 0
    rays = gbuffer_ref.pixel_rays(cam, w, h)
    r = s.abi.intersect_rays(s.h, rays.reshape(-1, 6))
    assert same_bits(got["depth"], r["t"].reshape(h, w), "depth vs mt_intersect_rays") == 0
    assert np.array_equal(got["line_no"], r["line"].reshape(h, w))
    tri = r["tri"].reshape(h, w)
    assert np.array_equal(got["prim"], np.where(tri >= 0, s.flat["tri_id"][np.maximum(tri, 0)], -1))


def test_shapes_chunks_and_plane_subsets(scenes, make):
    """Ragged sizes, chunks that cut 8x8 blocks, a 1x1 chunk, every single plane, a mixed subset."""
    s = make("mini")
    cam = (120.0, 90.0, 60.0, 5.0, 20.0, -3.0, 100.0)
    orc = orclib.OracleScene(scenes["mini"])
    for w, h in ((61, 37), (8, 8), (9, 1), (1, 9)):
        o = gbuffer_ref.oracle_gbuffer(orc, cam, w, h)
        got = s.gbuffer(cam, w, h)
        for p in ALL_PLANES:
            assert got[p].shape[:2] == (h, w)
        assert_planes_equal(got, dict(o, material=expected_material(s.flat, orc, o)), "%dx%d" % (w, h))
        assert got["stats"]["rays_primary"] == w * h
    w, h = 160, 90
    full = s.gbuffer(cam, w, h)
    for chunk in ((0, 0, 1, 1), (159, 89, 1, 1), (3, 5, 7, 5), (150, 0, 10, 90), (0, 80, 160, 10), (8, 8, 8, 8),
                  (13, 27, 65, 33), (7, 9, 17, 1)):
        cx, cy, cw, ch = chunk
        got = s.gbuffer(cam, w, h, chunk=chunk)
        part = {p: full[p][cy:cy + ch, cx:cx + cw] for p in ALL_PLANES}
        assert_planes_equal(got, part, "chunk %s" % (chunk,))
        assert got["stats"]["rays_primary"] == cw * ch
        assert got["stats"]["shaded_hits"] == int((part["prim"] >= 0).sum())
    for p in ALL_PLANES:
        got = s.gbuffer(cam, w, h, channels=(p,))
        assert set(got) == {p, "stats"}
        assert_planes_equal(got, full, "only " + p, (p,))
    got = s.gbuffer(cam, w, h, chunk=(13, 27, 65, 33), channels=("albedo", "prim", "depth"))
    assert set(got) == {"albedo", "prim", "depth", "stats"}
    assert_planes_equal(got, {p: full[p][27:60, 13:78] for p in ALL_PLANES}, "mixed subset", ("albedo", "prim", "depth"))
    for bad in [(-1, 0, 4, 4), (0, 0, 0, 4), (156, 86, 8, 8), (0, 0, 161, 1)]:
        with pytest.raises(RuntimeError, match="outside image"):
            s.gbuffer(cam, w, h, chunk=bad)
    with pytest.raises(RuntimeError, match="no plane"):
        s.gbuffer(cam, w, h, channels=())


def _device_planes(torch, ch, cw, names, sentinel=False):
    out = {}
    for n in names:
        dt, k = binding.GBUFFER_PLANES[n]
        shape = (ch, cw) + ((k,) if k > 1 else ())
        tdt = torch.float64 if dt is np.float64 else torch.int32
        out[n] = torch.full(shape, -12345, dtype=tdt, device="cuda") if sentinel else torch.zeros(shape, dtype=tdt, device="cuda")
    return out


def test_device_call_on_a_stream_leaves_unrequested_planes_alone(make):
    import torch
    s = make("room")
    cam = scenegen.ROOM_CAMERA
    w, h = 101, 67
    sens = binding.sensor(cam, w, h)
    want = s.gbuffer(cam, w, h)
    stream = torch.cuda.Stream()
    planes = _device_planes(torch, h, w, ALL_PLANES)
    chunk = (13, 27, 65, 33)
    part = _device_planes(torch, 33, 65, ALL_PLANES, sentinel=True)
    asked = ("normal", "material")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        sp = ctypes.c_void_p(stream.cuda_stream)
        s.abi.render_gbuffer_device(s.h, sens, w, h, (0, 0, w, h), {n: t.data_ptr() for n, t in planes.items()}, sp)
        s.abi.render_gbuffer_device(s.h, sens, w, h, chunk, {n: part[n].data_ptr() for n in asked}, sp)
        host = {n: t.cpu().numpy() for n, t in planes.items()}
        host_part = {n: t.cpu().numpy() for n, t in part.items()}
    stream.synchronize()
    st = s.abi.read_stats(s.h)
    assert st["rays_primary"] == w * h + 65 * 33
    assert_planes_equal(host, want, "device call")
    assert_planes_equal(host_part, {p: want[p][27:60, 13:78] for p in asked}, "device chunk", asked)
    for n in ALL_PLANES:
        if n not in asked:
            assert (host_part[n] == -12345).all(), "plane %s was not asked for and was written" % n
    with pytest.raises(RuntimeError, match="no plane"):
        s.abi.render_gbuffer_device(s.h, sens, w, h, (0, 0, w, h), {})


def test_two_scenes_on_two_streams(make):
    import torch
    a, b = make("mini"), make("room")
    w, h = 120, 68
    cams = (scenegen.ROOM_CAMERA, (330.0, 60.0, 380.0, -5.0, 200.0, 0.0, 90.0))
    wants = [a.gbuffer(cams[0], w, h), b.gbuffer(cams[1], w, h)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [_device_planes(torch, h, w, ALL_PLANES) for _ in range(2)]
    torch.cuda.synchronize()
    for rep in range(3):
        for k, s in enumerate((a, b)):
            s.abi.render_gbuffer_device(s.h, binding.sensor(cams[k], w, h), w, h, (0, 0, w, h),
                                        {n: t.data_ptr() for n, t in outs[k].items()},
                                        ctypes.c_void_p(streams[k].cuda_stream))
    for st in streams:
        st.synchronize()
    for k, s in enumerate((a, b)):
        s.abi.read_stats(s.h)
        assert_planes_equal({n: t.cpu().numpy() for n, t in outs[k].items()}, wants[k], "stream %d" % k)


@pytest.mark.parametrize("scene", ["loft", "loft_fine"])
def test_deep_layouts(scene, scenes, make):
    """Octrees of 16 and 20 levels: the DEEP instantiations of the kernel (mt_device.h, deep_layout)."""
    orc = orclib.OracleScene(scenes[scene])
    w, h = 48, 27
    o = gbuffer_ref.oracle_gbuffer(orc, scenegen.ROOM_CAMERA, w, h)
    s = make(scene)
    print(scene, "tree depth", s.flat["tree_depth"])
    assert s.flat["tree_depth"] >= 16
    got = s.gbuffer(scenegen.ROOM_CAMERA, w, h)
    assert_planes_equal(got, dict(o, material=expected_material(s.flat, orc, o)), scene)


def test_traversal_modes_give_identical_planes(make):
    s = make("mini")
    cam = scenegen.ROOM_CAMERA
    first = None
    for mode in range(8):
        s.abi.set_traversal_mode(s.h, mode)
        got = s.gbuffer(cam, W, H)
        if first is None:
            first = got
        assert_planes_equal(got, first, "mode %d" % mode)


def test_counters(scenes, make):
    """rays_primary = chunk pixels, shaded_hits = hits; in traversal mode 7 (no subtree skipped) the box / node /
    triangle / Moeller-Trumbore counts are the oracle's for the same rays."""
    s = make("mini")
    orc = orclib.OracleScene(scenes["mini"])
    cam = scenegen.ROOM_CAMERA
    s.abi.set_traversal_mode(s.h, 7)
    for chunk in (None, (5, 3, 61, 37)):
        o = gbuffer_ref.oracle_gbuffer(orc, cam, W, H, chunk)
        got = s.gbuffer(cam, W, H, chunk=chunk)
        n = o["prim"].size
        print(chunk, {k: (got["stats"][k], o["counters"][k]) for k in gbuffer_ref.TRAVERSAL_COUNTERS})
        assert got["stats"]["rays_primary"] == n
        assert got["stats"]["shaded_hits"] == int((o["prim"] >= 0).sum())
        assert got["stats"]["rays_secondary"] == 0 and got["stats"]["rays_shadow"] == 0
        for k in gbuffer_ref.TRAVERSAL_COUNTERS:
            assert got["stats"][k] == o["counters"][k], k
    # counters off: the device call leaves them at zero, the planes are the same
    import torch
    s.abi.set_traversal_mode(s.h, 0)
    s.abi.set_stats(s.h, False)
    want = s.gbuffer(cam, W, H, channels=("depth",))["depth"]
    d = torch.zeros((H, W), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.abi.render_gbuffer_device(s.h, binding.sensor(cam, W, H), W, H, (0, 0, W, H), {"depth": d.data_ptr()})
    torch.cuda.synchronize()
    assert s.abi.read_stats(s.h)["rays_primary"] == 0
    assert same_bits(d.cpu().numpy(), want, "depth without counters") == 0


def test_a_gbuffer_call_between_two_frames_changes_nothing_about_them(make):
    """Frame, G-buffer, frame with the camera at rest: the second frame is byte-equal to the first and is a launch
    with cost history, exactly as in a scene without the G-buffer call in between.  What mt_scene_kernel_times can show
    of that: with the state machine (engine 1) a launch WITHOUT history spends its `primary` time in primary_kernel
    (every primary ray of the 1080p frame), one WITH history in the three order kernels (a few words per block) --
    more than an order of magnitude apart on this frame; the bound below is a factor 3."""
    w, h = 1920, 1080
    cam = scenegen.ROOM_CAMERA
    sens = binding.sensor(cam, w, h)
    a, b = make("room"), make("room")  # b: the control, no G-buffer call
    times = {}
    for name, s in (("with", a), ("control", b)):
        s.abi.set_lights(s.h, scenegen.ROOM_LIGHTS)
        s.abi.set_engine(s.h, 1)
        s.abi.kernel_times(s.h)
        f1 = s.abi.render_chunk(s.h, sens, w, h)["rgb"]
        if name == "with":
            g = s.gbuffer(cam, w, h, channels=("depth", "normal"))
            assert g["stats"]["rays_primary"] == w * h
        f2 = s.abi.render_chunk(s.h, sens, w, h)["rgb"]
        assert np.array_equal(f1, f2), name
        pm, rm = s.abi.kernel_times(s.h)
        assert len(pm) == 2, (name, pm)  # the G-buffer call is not a launch of mt_scene_kernel_times
        times[name] = (pm, rm)
        print(name, "primary_ms", pm, "render_ms", rm)
    for name, (pm, rm) in times.items():
        assert pm[1] < pm[0] / 3, (name, pm)  # second frame: order kernels, not primary_kernel
    # the other way round: a G-buffer call before the first frame does not make that frame a repeated launch
    c = make("room")
    c.abi.set_lights(c.h, scenegen.ROOM_LIGHTS)
    c.abi.set_engine(c.h, 1)
    c.gbuffer(cam, w, h, channels=("depth",))
    c.abi.kernel_times(c.h)
    f = c.abi.render_chunk(c.h, sens, w, h)["rgb"]
    pm, _ = c.abi.kernel_times(c.h)
    print("gbuffer first: primary_ms", pm)
    assert len(pm) == 1 and pm[0] > 3 * times["control"][0][1]
    assert np.array_equal(f, a.abi.render_chunk(a.h, sens, w, h)["rgb"])


def test_facade(scenes, make, tmp_path):
    """MythTracer.gbuffer (RayTraceGBuffer through the ctypes shim) and a C++ program compiled against the facade's
    headers (tests/seam/gbuffer_driver.cc) give the C ABI's planes; SetSupersampling is ignored."""
    from mythtracer_amd import build
    cam = (120.0, 90.0, 60.0, 5.0, 20.0, -3.0, 100.0)
    w, h = 61, 37
    s = make("mini")
    want = s.gbuffer(cam, w, h)
    m = M.MythTracer(scenes["mini"])
    m.set_supersampling(2)
    got = m.gbuffer(cam, w, h)
    assert_planes_equal(got, want, "facade")
    assert got["counters"]["rays_primary"] == w * h and got["kernel_ms"] > 0
    part = m.gbuffer(cam, w, h, chunk=(5, 3, 33, 17), channels=("uvw", "line_no"))
    assert set(part) == {"uvw", "line_no", "counters", "kernel_ms", "total_ms"}
    assert_planes_equal(part, {p: want[p][3:20, 5:38] for p in ALL_PLANES}, "facade chunk", ("uvw", "line_no"))
    m.set_devices([0, 0])
    with pytest.raises(RuntimeError, match="several devices"):
        m.gbuffer(cam, w, h)
    # the C++ driver
    exe = str(tmp_path / "gbuffer_driver")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "seam", "gbuffer_driver.cc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(build.HOST, "include"), "-I", build.INC,
                           "-o", exe, src, "-L", build.LIB, "-lmythtracer_host", "-lmythtracer_hip",
                           "-Wl,-rpath," + build.LIB])
    out, chunk_out = str(tmp_path / "g.bin"), str(tmp_path / "c.bin")
    chunk = (5, 3, 33, 17)
    r = subprocess.run([exe, scenes["mini"], str(w), str(h)] + [repr(float(c)) for c in cam] + [out] +
                       [str(c) for c in chunk] + [chunk_out], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode().split() == ["primary", str(w * h), "hits", str(int((want["prim"] >= 0).sum()))]
    raw = open(out, "rb").read()
    at = 0
    drv = {}
    for p in ALL_PLANES:
        dt, k = binding.GBUFFER_PLANES[p]
        n = w * h * k
        drv[p] = np.frombuffer(raw, dtype=dt, count=n, offset=at).reshape((h, w) + ((k,) if k > 1 else ()))
        at += n * np.dtype(dt).itemsize
    assert at == len(raw)
    assert_planes_equal(drv, want, "C++ driver")
    raw = open(chunk_out, "rb").read()
    n = 33 * 17
    assert len(raw) == n * 12
    assert same_bits(np.frombuffer(raw, dtype=np.float64, count=n).reshape(17, 33), want["depth"][3:20, 5:38], "driver chunk depth") == 0
    assert np.array_equal(np.frombuffer(raw, dtype=np.int32, count=n, offset=n * 8).reshape(17, 33), want["line_no"][3:20, 5:38])
