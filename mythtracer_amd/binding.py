"""ctypes bindings of the two native libraries (see package docstring)."""
from __future__ import annotations

import ctypes as C
import os
import weakref

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
HIP_LIB = os.path.join(PKG, "lib", "libmythtracer_hip.so")
HOST_LIB = os.path.join(PKG, "lib", "libmythtracer_host.so")

MT_OK = 0
MT_ABI_VERSION = 5
MT_TEX_RGB8, MT_TEX_F64 = 0, 1

# every symbol include/mythtracer_hip.h declares
HIP_SYMBOLS = [
    "mt_last_error", "mt_abi_version", "mt_device_count", "mt_scene_create",
    "mt_scene_destroy", "mt_scene_set_lights", "mt_render_chunk",
    "mt_render_chunk_device", "mt_render_tiles_device", "mt_blit_tiles_device",
    "mt_scene_read_stats", "mt_intersect_rays", "mt_scene_set_traversal_mode",
    "mt_scene_kernel_times", "mt_scene_lean_info", "mt_scene_set_scheduling", "mt_scene_set_engine",
    "mt_scene_set_stats", "mt_set_default_engine", "mt_scene_set_tuning",
    "mt_render_frame_multi", "mt_scene_export_costs_device", "mt_scene_import_costs_device",
    "mt_order_tiles_device", "mt_dealt_tile_count", "mt_deal_tiles_device",
    "mt_render_tile_list_device", "mt_blit_tile_list_device",
    "mt_render_chunk_ss", "mt_render_chunk_ss_device", "mt_resolve_tiles_device",
    "mt_render_gbuffer", "mt_render_gbuffer_device",
    "mt_render_lightbuffer", "mt_render_lightbuffer_device", "mt_shade_direct", "mt_shade_direct_device",
    "mt_update_lightbuffer", "mt_update_lightbuffer_device",
    "mt_refine_mask_device", "mt_render_chunk_adaptive", "mt_render_chunk_adaptive_device",
    "mt_raytree_create", "mt_raytree_destroy", "mt_raytree_info", "mt_raytree_read_layer",
    "mt_raytree_shade", "mt_raytree_shade_device",
    "mt_raytree_update_lights", "mt_raytree_update_lights_device",
    "mt_raytree_create_rays", "mt_raytree_create_rays_device", "mt_raytree_shade_colors",
    "mt_raytree_shade_colors_device", "mt_trace_rays",
    "mt_scene_set_materials", "mt_scene_get_materials", "mt_raytree_update_materials",
    "mt_raytree_regrow_materials",
    "mt_scene_set_texture", "mt_scene_get_texture_info", "mt_scene_set_raytree_uvw", "mt_raytree_read_uvw",
    "mt_raytree_keeps_uvw", "mt_retexture_gbuffer", "mt_retexture_gbuffer_device",
    "mt_scene_set_triangle_materials", "mt_scene_get_triangle_materials", "mt_scene_set_raytree_tri",
    "mt_raytree_read_tri", "mt_raytree_keeps_tri",
    "mt_scene_set_triangle_normals", "mt_scene_set_triangle_uvw", "mt_scene_get_triangle_normals",
    "mt_scene_get_triangle_uvw", "mt_raytree_attr_info_last",
    "mt_octree_build", "mt_octree_info", "mt_octree_read", "mt_octree_destroy", "mt_scene_create_triangles",
    "mt_scene_read_tree",
    "mt_scene_set_triangle_vertices", "mt_scene_get_triangle_vertices", "mt_scene_move_times_last",
    "mt_scene_edit_triangles",
]
MT_MAX_RECURSION = 16

# mt_scene_set_tuning knobs, in the order of the enum in include/mythtracer_hip.h
TUNE = {name: i for i, name in enumerate([
    "POOL_BELOW", "POOL_CAP", "PACKED_STACK", "BLOCKS_PER_CU", "FORECAST_RADIUS", "BLEND", "FORMS",
    "POOL_CUT_SHARE", "POOL_PIECE_TIME1", "POOL_PIECE_TIME2", "POOL_PIECE_WORK1", "POOL_PIECE_WORK2",
    "POOL_CELL_FACTOR", "QUAD_SHARE", "QUAD_SHARE_MOVING", "QUAD_KEEP", "QUAD_WORK", "QUAD_WORK_MOVING",
    "POOL_SCRATCH_MB", "HYBRID_POOL_SHARE", "HYBRID_QUAD_SHARE", "HYBRID_WORK1", "HYBRID_WORK2", "FORECAST_STEP",
    "HYBRID_STARTER_SHARE", "DEEP_LAYOUT", "MULTI_FORCE_PEER_COPY", "MULTI_BALANCE", "XCD_QUEUES",
    "ORDER_GROUPS", "SM_CELL_SHARE", "SM_CELL_TIME", "SM_CELL_WORK", "HYBRID_CELL_FACTOR", "LEAN_KERNEL"])}
# knob ids outside the enum's dense range (include/mythtracer_hip.h: ids from 1000 on); set_tuning looks a name up in TUNE, then here
TUNE_EXTRA = {"SHADOW_BOUND": 1000}  # MT_TUNE_SHADOW_BOUND: 0 | 1 | 2

STAT_NAMES = ["rays_primary", "rays_secondary", "rays_shadow", "box_tests",
              "node_visits", "tri_tests", "mt_tests", "shaded_hits"]


class NativeLibraryMissing(RuntimeError):
    pass


class mt_material(C.Structure):
    _fields_ = [("ambient", C.c_double * 3), ("diffuse", C.c_double * 3),
                ("specular", C.c_double * 3), ("specular_exp", C.c_double),
                ("reflectance", C.c_double), ("transparency", C.c_double),
                ("transmission_filter", C.c_double * 3),
                ("refraction_index", C.c_double), ("tex", C.c_int32),
                ("reserved", C.c_int32)]


class mt_light(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("ambient", C.c_double * 3),
                ("diffuse", C.c_double * 3), ("specular", C.c_double * 3)]


class mt_texture(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("format", C.c_int32),
                ("reserved", C.c_int32), ("texels", C.c_void_p)]


class mt_sensor(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("start_point", C.c_double * 3),
                ("delta_scanline", C.c_double * 3), ("delta_pixel", C.c_double * 3)]


class mt_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in STAT_NAMES] + [
        ("wave_node_steps", C.c_uint64), ("wave_tri_steps", C.c_uint64),
        ("kernel_ms", C.c_double), ("total_ms", C.c_double),
        ("bytes_scalar", C.c_uint64), ("bytes_vector", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class mt_adaptive_info(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_blocks", "n_refined", "plain_history", "refine_history")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class mt_raytree_regrow_info(C.Structure):
    _fields_ = [("regrown", C.c_int32), ("n_layers_before", C.c_int32), ("n_layers_after", C.c_int32),
                ("kept", C.c_int64 * (MT_MAX_RECURSION + 1)), ("traced", C.c_int64 * (MT_MAX_RECURSION + 1)), ("dropped", C.c_int64 * (MT_MAX_RECURSION + 1))]

    def as_dict(self):
        """kept / traced per layer of the new tree, dropped per layer of the old one."""
        return dict(regrown=int(self.regrown), n_layers_before=int(self.n_layers_before),
                    n_layers_after=int(self.n_layers_after),
                    kept=[int(v) for v in self.kept][:self.n_layers_after],
                    traced=[int(v) for v in self.traced][:self.n_layers_after],
                    dropped=[int(v) for v in self.dropped][:self.n_layers_before])


class mt_raytree_attr_info(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("renormaled", "reuvwed", "respawned")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class mt_build_info(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("depth", C.c_int32), ("levels", C.c_int32),
                ("kernel_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class mt_octree_arrays(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("n_tris", C.c_int32), ("depth", C.c_int32)] + [
        (n, C.c_void_p) for n in ("node_aabb", "node_center", "first_child", "prim_begin", "prim_count", "tri_id",
                                  "tri_aabb")]


class mt_triangle_desc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("device", C.c_int32),
                ("n_tris", C.c_int32), ("n_materials", C.c_int32), ("n_textures", C.c_int32),
                ("tri_vertex", C.c_void_p), ("tri_normal", C.c_void_p), ("tri_uvw", C.c_void_p),
                ("tri_material", C.c_void_p), ("tri_line_no", C.c_void_p),
                ("materials", C.c_void_p), ("textures", C.c_void_p)]


class mt_lean_info(C.Structure):
    _fields_ = [("lean", C.c_int32), ("handed_over", C.c_int32), ("units", C.c_uint32), ("redo_units", C.c_uint32),
                ("lean_ms", C.c_double), ("redo_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class mt_scene_desc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32),
                ("device", C.c_int32), ("n_nodes", C.c_int32), ("n_tris", C.c_int32),
                ("n_materials", C.c_int32), ("n_textures", C.c_int32),
                ("tree_depth", C.c_int32),
                ("node_aabb", C.c_void_p), ("node_center", C.c_void_p),
                ("node_first_child", C.c_void_p), ("node_prim_begin", C.c_void_p),
                ("node_prim_count", C.c_void_p),
                ("tri_vertex", C.c_void_p), ("tri_normal", C.c_void_p),
                ("tri_uvw", C.c_void_p), ("tri_aabb", C.c_void_p),
                ("tri_material", C.c_void_p), ("tri_line_no", C.c_void_p),
                ("tri_id", C.c_void_p),
                ("materials", C.c_void_p), ("textures", C.c_void_p)]


class mt_gbuffer(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("depth", "point", "normal", "uvw", "albedo", "prim", "line_no", "material")]


# the planes of mt_gbuffer in declaration order: name -> (dtype, values per pixel); bit i of the facade's
# GBuffer::channels is plane i
GBUFFER_PLANES = {"depth": (np.float64, 1), "point": (np.float64, 3), "normal": (np.float64, 3),
                  "uvw": (np.float64, 3), "albedo": (np.float64, 3), "prim": (np.int32, 1),
                  "line_no": (np.int32, 1), "material": (np.int32, 1)}


def _gbuffer_arrays(channels, cw, ch):
    names = list(GBUFFER_PLANES) if channels is None else list(channels)
    for n in names:
        if n not in GBUFFER_PLANES:
            raise ValueError("unknown G-buffer plane %r (planes: %s)" % (n, ", ".join(GBUFFER_PLANES)))
    out = {}
    for n in names:
        dt, k = GBUFFER_PLANES[n]
        out[n] = np.zeros((max(ch, 0), max(cw, 0)) + ((k,) if k > 1 else ()), dtype=dt)
    return out


class mt_lightbuffer(C.Structure):
    _fields_ = [("power", C.c_void_p), ("in_shadow", C.c_void_p)]


# the planes of mt_lightbuffer: name -> (dtype, values per pixel and light); arrays are (n_lights, ch, cw[, 3])
LIGHTBUFFER_PLANES = {"power": (np.float64, 3), "in_shadow": (np.uint8, 1)}
# what a relight reads of the G-buffer
RELIGHT_GBUFFER_PLANES = ("point", "normal", "albedo", "material")


def _lightbuffer_arrays(channels, n_lights, cw, ch):
    names = list(LIGHTBUFFER_PLANES) if channels is None else list(channels)
    for n in names:
        if n not in LIGHTBUFFER_PLANES:
            raise ValueError("unknown light-buffer plane %r (planes: %s)" % (n, ", ".join(LIGHTBUFFER_PLANES)))
    out = {}
    for n in names:
        dt, k = LIGHTBUFFER_PLANES[n]
        out[n] = np.zeros((n_lights, max(ch, 0), max(cw, 0)) + ((k,) if k > 1 else ()), dtype=dt)
    return out


def _relight_planes(gbuffer, lightbuffer, cw, ch):
    """The six planes of a relight as contiguous arrays of the right type and shape; n_lights from `power`."""
    g = {}
    for n in RELIGHT_GBUFFER_PLANES:
        if n not in gbuffer:
            raise ValueError("the relight pass needs the G-buffer plane %r" % n)
        dt, k = GBUFFER_PLANES[n]
        g[n] = np.ascontiguousarray(gbuffer[n], dtype=dt)
        if g[n].shape != (ch, cw) + ((k,) if k > 1 else ()):
            raise ValueError("G-buffer plane %r has shape %s, not that of the %dx%d chunk" % (n, g[n].shape, cw, ch))
    for n in LIGHTBUFFER_PLANES:
        if n not in lightbuffer:
            raise ValueError("the relight pass needs the light-buffer plane %r" % n)
    power = np.ascontiguousarray(lightbuffer["power"], dtype=np.float64)
    shadow = np.ascontiguousarray(lightbuffer["in_shadow"], dtype=np.uint8)
    n_l = power.shape[0]
    if power.shape != (n_l, ch, cw, 3) or shadow.shape != (n_l, ch, cw):
        raise ValueError("light-buffer planes of shape %s / %s do not fit the %dx%d chunk" % (power.shape, shadow.shape, cw, ch))
    return g, dict(power=power, in_shadow=shadow), n_l


# what a light-buffer update reads of the G-buffer
UPDATE_GBUFFER_PLANES = ("point", "material")


def _update_planes(gbuffer, lightbuffer):
    """The planes of a light-buffer update, checked: the two G-buffer planes as contiguous arrays, the light-buffer
    planes present (at least one) AS THEY ARE -- they are updated in place, so they must be C-contiguous numpy arrays of
    the plane's dtype.  Returns (g, lb, n_lights, cw, ch)."""
    g = {}
    for n in UPDATE_GBUFFER_PLANES:
        if n not in gbuffer:
            raise ValueError("the light-buffer update needs the G-buffer plane %r" % n)
        dt, k = GBUFFER_PLANES[n]
        a = np.asarray(gbuffer[n])
        if a.dtype != dt:
            raise ValueError("G-buffer plane %r has dtype %s, not %s" % (n, a.dtype, np.dtype(dt)))
        g[n] = np.ascontiguousarray(a)
    if g["material"].ndim != 2:
        raise ValueError("G-buffer plane 'material' has shape %s, not (rows, columns)" % (g["material"].shape,))
    ch, cw = g["material"].shape
    if g["point"].shape != (ch, cw, 3):
        raise ValueError("G-buffer plane 'point' has shape %s, not that of the %dx%d chunk" % (g["point"].shape, cw, ch))
    lb = {n: lightbuffer[n] for n in LIGHTBUFFER_PLANES if n in lightbuffer}
    if not lb:
        raise ValueError("the light-buffer update needs a light-buffer plane (%s)" % ", ".join(LIGHTBUFFER_PLANES))
    n_l = None
    for n, a in lb.items():
        dt, k = LIGHTBUFFER_PLANES[n]
        if not isinstance(a, np.ndarray) or a.dtype != dt or not a.flags.c_contiguous or not a.flags.writeable:
            raise ValueError("light-buffer plane %r must be a writeable C-contiguous numpy array of dtype %s (it is "
                             "updated in place)" % (n, np.dtype(dt)))
        if n_l is None:
            n_l = a.shape[0] if a.ndim else -1
        if a.shape != (n_l, ch, cw) + ((k,) if k > 1 else ()):
            raise ValueError("light-buffer plane %r of shape %s does not fit the %dx%d chunk" % (n, a.shape, cw, ch))
    return g, lb, n_l, cw, ch


DEBUG_PX_DTYPE = np.dtype([("line_no", "<i4"), ("reserved", "<i4"), ("point", "<f8", 3)])


class mt_raytree_desc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_layers", "n_lights", "image_w", "image_h", "chunk_x", "chunk_y", "chunk_w",
                                         "chunk_h", "max_depth", "from_rays")] + [
        ("n_rays", C.c_int64 * (MT_MAX_RECURSION + 1)), ("trace_ms", C.c_double * (MT_MAX_RECURSION + 1)),
        ("bytes", C.c_uint64)]

    def as_dict(self):
        n = int(self.n_layers)
        return dict(n_layers=n, n_lights=int(self.n_lights), image=(int(self.image_w), int(self.image_h)),
                    chunk=(int(self.chunk_x), int(self.chunk_y), int(self.chunk_w), int(self.chunk_h)),
                    max_depth=int(self.max_depth), from_rays=int(self.from_rays), n_rays=[int(v) for v in self.n_rays[:n]],
                    trace_ms=[float(v) for v in self.trace_ms[:n]], bytes=int(self.bytes))


class mt_ray_list(C.Structure):
    _fields_ = [("ray", C.c_void_p), ("in_object", C.c_void_p), ("coef", C.c_void_p), ("list_w", C.c_int32),
                ("list_h", C.c_int32)]


# the planes of mt_raytree_layer in declaration order: name -> (dtype, values per ray, per light?)
RAYTREE_PLANES = {"ray": (np.float64, 6, False), "in_object": (np.uint8, 1, False), "coef": (np.float64, 1, False),
                  "point": (np.float64, 3, False), "normal": (np.float64, 3, False), "albedo": (np.float64, 3, False),
                  "material": (np.int32, 1, False), "power": (np.float64, 3, True), "in_shadow": (np.uint8, 1, True),
                  "child_refl": (np.int32, 1, False), "child_refr": (np.int32, 1, False), "pixel": (np.int32, 1, False)}


class mt_raytree_layer(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in RAYTREE_PLANES]


def _load(path):
    if not os.path.exists(path):
        raise NativeLibraryMissing(
            "%s is missing: run `python -m mythtracer_amd.build` (needs hipcc); "
            "there is no CPU fallback" % path)
    return C.CDLL(path)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _f64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64))


def _i32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.int32))


class HipAbi:
    """libmythtracer_hip.so — the C ABI, one method per entry point."""

    def __init__(self, lib_path=None):
        L = self.lib = _load(lib_path or HIP_LIB)
        vp, ci = C.c_void_p, C.c_int
        L.mt_last_error.restype = C.c_char_p
        L.mt_scene_create.restype = vp
        L.mt_scene_create.argtypes = [C.POINTER(mt_scene_desc)]
        L.mt_scene_destroy.argtypes = [vp]
        L.mt_scene_destroy.restype = None
        L.mt_scene_set_lights.argtypes = [vp, vp, ci]
        L.mt_scene_set_materials.argtypes = [vp, vp, ci]
        L.mt_scene_get_materials.argtypes = [vp, vp, ci]
        L.mt_raytree_update_materials.argtypes = [vp, vp]
        L.mt_raytree_regrow_materials.argtypes = [vp, vp, vp]
        L.mt_scene_set_texture.argtypes = [vp, ci, C.POINTER(mt_texture)]
        L.mt_scene_get_texture_info.argtypes = [vp, ci, C.POINTER(mt_texture)]
        L.mt_scene_set_raytree_uvw.argtypes = [vp, ci]
        L.mt_raytree_read_uvw.argtypes = [vp, ci, vp]
        L.mt_raytree_keeps_uvw.argtypes = [vp]
        L.mt_scene_set_triangle_materials.argtypes = [vp, vp, ci]
        L.mt_scene_get_triangle_materials.argtypes = [vp, vp, ci]
        L.mt_scene_set_raytree_tri.argtypes = [vp, ci]
        L.mt_raytree_read_tri.argtypes = [vp, ci, vp]
        L.mt_raytree_keeps_tri.argtypes = [vp]
        L.mt_scene_set_triangle_normals.argtypes = [vp, vp, ci]
        L.mt_scene_set_triangle_uvw.argtypes = [vp, vp, ci]
        L.mt_scene_get_triangle_normals.argtypes = [vp, vp, ci]
        L.mt_scene_get_triangle_uvw.argtypes = [vp, vp, ci]
        L.mt_raytree_attr_info_last.argtypes = [vp, C.POINTER(mt_raytree_attr_info)]
        L.mt_octree_build.restype = vp
        L.mt_octree_build.argtypes = [ci, ci, vp, C.POINTER(mt_build_info)]
        L.mt_octree_info.argtypes = [vp, C.POINTER(mt_build_info)]
        L.mt_octree_read.argtypes = [vp, C.POINTER(mt_octree_arrays)]
        L.mt_octree_destroy.argtypes = [vp]
        L.mt_octree_destroy.restype = None
        L.mt_scene_create_triangles.restype = vp
        L.mt_scene_create_triangles.argtypes = [C.POINTER(mt_triangle_desc), C.POINTER(mt_build_info)]
        L.mt_scene_read_tree.argtypes = [vp, C.POINTER(mt_octree_arrays)]
        L.mt_scene_set_triangle_vertices.argtypes = [vp, vp, ci, vp, C.POINTER(mt_build_info)]
        L.mt_scene_get_triangle_vertices.argtypes = [vp, vp, ci]
        L.mt_scene_move_times_last.argtypes = [vp, vp]
        L.mt_scene_edit_triangles.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp, vp, C.POINTER(mt_build_info)]
        L.mt_retexture_gbuffer.argtypes = [vp, ci, ci, C.POINTER(mt_gbuffer), vp]
        L.mt_retexture_gbuffer_device.argtypes = [vp, ci, ci, C.POINTER(mt_gbuffer), vp]
        L.mt_render_chunk.argtypes = [vp, C.POINTER(mt_sensor)] + [ci] * 7 + [vp, vp, vp]
        L.mt_render_chunk_device.argtypes = [vp, C.POINTER(mt_sensor)] + [ci] * 7 + [vp, vp, vp]
        L.mt_render_tiles_device.argtypes = [vp, C.POINTER(mt_sensor)] + [ci] * 8 + [vp, vp]
        L.mt_blit_tiles_device.argtypes = [vp] + [ci] * 7 + [vp, vp, vp]
        L.mt_scene_read_stats.argtypes = [vp, C.POINTER(mt_stats)]
        L.mt_intersect_rays.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
        L.mt_scene_set_traversal_mode.argtypes = [vp, ci]
        L.mt_scene_kernel_times.argtypes = [vp, ci, vp, vp]
        L.mt_scene_lean_info.argtypes = [vp, C.POINTER(mt_lean_info)]
        L.mt_scene_set_scheduling.argtypes = [vp, ci]
        L.mt_scene_set_engine.argtypes = [vp, ci]
        L.mt_scene_set_stats.argtypes = [vp, ci]
        L.mt_set_default_engine.argtypes = [ci]
        L.mt_scene_set_tuning.argtypes = [vp, ci, C.c_double]
        L.mt_render_frame_multi.argtypes = [vp, ci, C.POINTER(mt_sensor)] + [ci] * 5 + [vp, vp]
        L.mt_scene_export_costs_device.argtypes = [vp, vp, ci, ci, vp]
        L.mt_scene_import_costs_device.argtypes = [vp, vp, ci, ci, vp]
        L.mt_order_tiles_device.argtypes = [vp, vp] + [ci] * 6 + [vp, vp]
        L.mt_dealt_tile_count.argtypes = [ci] * 6
        L.mt_deal_tiles_device.argtypes = [vp, vp] + [ci] * 6 + [vp, vp]
        L.mt_render_tile_list_device.argtypes = [vp, C.POINTER(mt_sensor)] + [ci] * 4 + [vp, ci, C.c_uint64, ci, vp, vp]
        L.mt_blit_tile_list_device.argtypes = [vp] + [ci] * 4 + [vp, ci, vp, vp, vp]
        L.mt_render_chunk_ss.argtypes = [vp, C.POINTER(mt_sensor)] + [ci] * 8 + [vp, vp]
        L.mt_render_chunk_ss_device.argtypes = [vp, C.POINTER(mt_sensor)] + [ci] * 8 + [vp, vp]
        L.mt_resolve_tiles_device.argtypes = [vp] + [ci] * 6 + [vp, ci, ci, vp, vp, vp]
        L.mt_render_gbuffer.argtypes = [vp, C.POINTER(mt_sensor)] + [ci] * 6 + [C.POINTER(mt_gbuffer), vp]
        L.mt_render_gbuffer_device.argtypes = [vp, C.POINTER(mt_sensor)] + [ci] * 6 + [C.POINTER(mt_gbuffer), vp]
        gl = [C.POINTER(mt_gbuffer), C.POINTER(mt_lightbuffer)]
        L.mt_render_lightbuffer.argtypes = [vp, C.POINTER(mt_sensor)] + [ci] * 6 + gl + [vp]
        L.mt_render_lightbuffer_device.argtypes = [vp, C.POINTER(mt_sensor)] + [ci] * 6 + gl + [vp]
        L.mt_shade_direct.argtypes = [vp, C.POINTER(mt_sensor)] + [ci] * 6 + gl + [vp, ci, vp, vp]
        L.mt_shade_direct_device.argtypes = [vp, C.POINTER(mt_sensor)] + [ci] * 6 + gl + [vp, ci, vp, vp]
        L.mt_update_lightbuffer.argtypes = [vp, ci, ci, C.POINTER(mt_gbuffer), vp, ci, C.POINTER(mt_lightbuffer), vp]
        L.mt_update_lightbuffer_device.argtypes = L.mt_update_lightbuffer.argtypes
        L.mt_refine_mask_device.argtypes = [vp] + [ci] * 7 + [vp] * 5
        L.mt_raytree_create.restype = vp
        L.mt_raytree_create.argtypes = [vp, C.POINTER(mt_sensor)] + [ci] * 7 + [vp]
        L.mt_raytree_destroy.argtypes = [vp]
        L.mt_raytree_destroy.restype = None
        L.mt_raytree_info.argtypes = [vp, C.POINTER(mt_raytree_desc)]
        L.mt_raytree_read_layer.argtypes = [vp, ci, C.POINTER(mt_raytree_layer)]
        L.mt_raytree_shade.argtypes = [vp, vp, ci, vp, vp]
        L.mt_raytree_shade_device.argtypes = [vp, vp, ci, vp, vp]
        L.mt_raytree_update_lights.argtypes = [vp, vp, ci, vp]
        L.mt_raytree_update_lights_device.argtypes = [vp, vp, ci, vp]
        L.mt_raytree_create_rays.restype = vp
        L.mt_raytree_create_rays.argtypes = [vp, vp, ci, vp]
        L.mt_raytree_create_rays_device.restype = vp
        L.mt_raytree_create_rays_device.argtypes = [vp, vp, ci, vp]
        L.mt_raytree_shade_colors.argtypes = [vp, vp, ci, vp, vp]
        L.mt_raytree_shade_colors_device.argtypes = [vp, vp, ci, vp, vp]
        L.mt_trace_rays.argtypes = [vp, vp, ci, vp, vp, vp]
        ps = C.POINTER(mt_sensor)
        L.mt_render_chunk_adaptive.argtypes = [vp, ps, ps] + [ci] * 9 + [vp, vp, C.POINTER(mt_adaptive_info), vp]
        L.mt_render_chunk_adaptive_device.argtypes = [vp, ps, ps] + [ci] * 9 + [vp, vp, C.POINTER(mt_adaptive_info), vp]

    def last_error(self) -> str:
        return self.lib.mt_last_error().decode(errors="replace")

    def check(self, rc):
        if rc != MT_OK:
            raise RuntimeError("mythtracer_hip error %d: %s" % (rc, self.last_error()))

    def device_count(self) -> int:
        return self.lib.mt_device_count()

    @staticmethod
    def make_sensor(sensor12) -> mt_sensor:
        s = _f64(sensor12).reshape(12)
        out = mt_sensor()
        for i, name in enumerate(["origin", "start_point", "delta_scanline", "delta_pixel"]):
            for k in range(3):
                getattr(out, name)[k] = s[i * 3 + k]
        return out

    @staticmethod
    def _material_array(mats):
        """mt_material[max(n, 1)] from a list of dict(values = ka kd ks ns refl tr tf ni (16 doubles), tex = index or
        -1): the `materials` of MythTracer.flatten()."""
        marr = (mt_material * max(len(mats), 1))()
        for i, m in enumerate(mats):
            v = _f64(m["values"])  # ka kd ks ns refl tr tf ni
            for k in range(3):
                marr[i].ambient[k] = v[k]
                marr[i].diffuse[k] = v[3 + k]
                marr[i].specular[k] = v[6 + k]
                marr[i].transmission_filter[k] = v[12 + k]
            marr[i].specular_exp, marr[i].reflectance, marr[i].transparency = v[9], v[10], v[11]
            marr[i].refraction_index = v[15]
            marr[i].tex = int(m.get("tex", -1))
        return marr

    def scene_create(self, flat: dict, device: int = 0):
        """flat: dict of numpy arrays in the layout of mt_scene_desc (see
        MythTracer.flatten()).  Returns an opaque handle."""
        keep = []

        def arr(name, dt):
            a = np.ascontiguousarray(flat[name], dtype=dt)
            keep.append(a)
            return a.ctypes.data

        d = mt_scene_desc()
        d.struct_size = C.sizeof(mt_scene_desc)
        d.abi_version = MT_ABI_VERSION
        d.device = device
        d.n_nodes = len(flat["node_first_child"])
        d.n_tris = len(flat["tri_material"])
        d.tree_depth = int(flat["tree_depth"])
        d.node_aabb = arr("node_aabb", np.float64)
        d.node_center = arr("node_center", np.float64)
        d.node_first_child = arr("node_first_child", np.int32)
        d.node_prim_begin = arr("node_prim_begin", np.int32)
        d.node_prim_count = arr("node_prim_count", np.int32)
        d.tri_vertex = arr("tri_vertex", np.float64)
        d.tri_normal = arr("tri_normal", np.float64)
        d.tri_uvw = arr("tri_uvw", np.float64)
        d.tri_aabb = arr("tri_aabb", np.float64)
        d.tri_material = arr("tri_material", np.int32)
        d.tri_line_no = arr("tri_line_no", np.int32)
        d.tri_id = arr("tri_id", np.int32)
        mats = flat.get("materials", [])
        marr = self._material_array(mats)
        texs = flat.get("textures", [])
        tarr = self._texture_array(texs, keep)
        keep += [marr, tarr]
        d.n_materials = len(mats)
        d.n_textures = len(texs)
        d.materials = C.cast(marr, C.c_void_p)
        d.textures = C.cast(tarr, C.c_void_p)
        h = self.lib.mt_scene_create(C.byref(d))
        if not h:
            raise RuntimeError("mt_scene_create failed: " + self.last_error())
        return h

    def scene_destroy(self, h):
        self.lib.mt_scene_destroy(h)

    def _texture_array(self, texs, keep):
        tarr = (mt_texture * max(len(texs), 1))()
        for i, t in enumerate(texs):
            texels = np.ascontiguousarray(t["texels"])
            keep.append(texels)
            tarr[i].height, tarr[i].width = texels.shape[0], texels.shape[1]
            tarr[i].format = MT_TEX_RGB8 if texels.dtype == np.uint8 else MT_TEX_F64
            tarr[i].texels = texels.ctypes.data
        return tarr

    def _read_tree(self, fn, h) -> dict:
        """The arrays of mt_octree_arrays through `fn` (mt_octree_read / mt_scene_read_tree): first the counts, then
        the arrays."""
        a = mt_octree_arrays()
        self.check(fn(h, C.byref(a)))
        nn, nt = int(a.n_nodes), int(a.n_tris)
        out = dict(node_aabb=np.zeros((nn, 6)), node_center=np.zeros((nn, 3)),
                   first_child=np.zeros(nn, dtype=np.int32), prim_begin=np.zeros(nn, dtype=np.int32),
                   prim_count=np.zeros(nn, dtype=np.int32), tri_id=np.zeros(max(nt, 1), dtype=np.int32),
                   tri_aabb=np.zeros((max(nt, 1), 6)))
        for name, arr in out.items():
            setattr(a, name, arr.ctypes.data)
        self.check(fn(h, C.byref(a)))
        out["tri_id"], out["tri_aabb"] = out["tri_id"][:nt], out["tri_aabb"][:nt]
        out["depth"] = int(a.depth)
        return out

    def octree_build(self, tri_vertex, device: int = 0):
        """mt_octree_build: the octree of the triangles `tri_vertex` ((n, 3, 3) or (n, 9) doubles in add order) built on
        the GPU.  Returns (handle, info) with info = dict(n_nodes, depth, levels, kernel_ms, total_ms); the handle goes to
        octree_read / octree_destroy.  RuntimeError with the library's message when the build fails."""
        v = np.ascontiguousarray(tri_vertex, dtype=np.float64)
        if v.size % 9:
            raise ValueError("a triangle has 9 doubles, not %d in all" % v.size)
        info = mt_build_info()
        h = self.lib.mt_octree_build(device, v.size // 9, v.ctypes.data if v.size else None, C.byref(info))
        if not h:
            raise RuntimeError("mt_octree_build failed: " + self.last_error())
        return h, info.as_dict()

    def octree_read(self, tree) -> dict:
        """mt_octree_read: dict(depth, node_aabb, node_center, first_child, prim_begin, prim_count, tri_id, tri_aabb);
        tri_aabb is in add order."""
        return self._read_tree(self.lib.mt_octree_read, tree)

    def octree_destroy(self, tree):
        self.lib.mt_octree_destroy(tree)

    def scene_read_tree(self, h) -> dict:
        """mt_scene_read_tree: the same arrays from any scene made with tri_id."""
        return self._read_tree(self.lib.mt_scene_read_tree, h)

    def scene_set_triangle_vertices(self, h, add_idx, vertices) -> dict:
        """mt_scene_set_triangle_vertices: the triangles `add_idx` (ADD-order indices, each at most once) of the uploaded
        scene moved to `vertices` ((len(add_idx), 3, 3) or (len(add_idx), 9) doubles).  The scene's node-stream order is
        the new tree's afterwards (scene_read_tree).  Returns the build's info, all zero when no listed triangle
        changed by its bits.  RuntimeError with the library's message on a refusal: the scene is then as it was."""
        idx = np.ascontiguousarray(add_idx, dtype=np.int32).reshape(-1)
        v = np.ascontiguousarray(vertices, dtype=np.float64)
        if v.size != idx.size * 9:
            raise ValueError("%d triangles listed, %d doubles of vertices (9 per triangle)" % (idx.size, v.size))
        info = mt_build_info()
        self.check(self.lib.mt_scene_set_triangle_vertices(h, idx.ctypes.data if idx.size else None, int(idx.size),
                                                           v.ctypes.data if v.size else None, C.byref(info)))
        return info.as_dict()

    def scene_edit_triangles(self, h, remove, add) -> dict:
        """mt_scene_edit_triangles: the triangles `remove` (ADD-order indices of the scene as it is, each at most once)
        taken out and the triangles of `add` appended.  add: None, or a dict of tri_vertex, tri_normal, tri_uvw
        ((k, 9) or (k, 3, 3) doubles), tri_material and tri_line_no (k int32), as scene_create_triangles takes them;
        tri_material indexes the scene's existing materials or is -1.  The new add order is numpy.delete followed by
        concatenate; n_tris and the node-stream order are the new scene's afterwards.  Returns the build's info, all
        zero when both lists are empty.  RuntimeError with the library's message on a refusal: the scene is then as it
        was."""
        idx = np.ascontiguousarray([] if remove is None else remove, dtype=np.int32).reshape(-1)
        n_add, ptr = 0, [None] * 5
        if add is not None:
            v, nrm, uvw = (np.ascontiguousarray(add[k], dtype=np.float64) for k in ("tri_vertex", "tri_normal", "tri_uvw"))
            mtl, line = (np.ascontiguousarray(add[k], dtype=np.int32).reshape(-1) for k in ("tri_material", "tri_line_no"))
            n_add = int(mtl.size)
            if not (v.size == nrm.size == uvw.size == 9 * n_add and line.size == n_add):
                raise ValueError("%d added triangles: %d / %d / %d doubles of vertices, normals, uvw (9 per triangle), "
                                 "%d line numbers" % (n_add, v.size, nrm.size, uvw.size, line.size))
            if n_add:
                ptr = [a.ctypes.data for a in (v, nrm, uvw, mtl, line)]
        info = mt_build_info()
        self.check(self.lib.mt_scene_edit_triangles(h, idx.ctypes.data if idx.size else None, int(idx.size), n_add, *ptr,
                                                    C.byref(info)))
        return info.as_dict()

    def scene_get_triangle_vertices(self, h, n_tris) -> np.ndarray:
        """mt_scene_get_triangle_vertices: all vertices of the scene in ADD order, (n_tris, 3, 3) float64."""
        out = np.zeros((max(n_tris, 0), 3, 3), dtype=np.float64)
        self.check(self.lib.mt_scene_get_triangle_vertices(h, out.ctypes.data if out.size else None, n_tris))
        return out

    def scene_move_times(self, h) -> dict:
        """mt_scene_move_times_last: wall times in ms of the parts of the scene's last set_triangle_vertices that
        changed a triangle, or of its last edit_triangles: build, regather, readback, layout, upload."""
        out = np.zeros(5, dtype=np.float64)
        self.check(self.lib.mt_scene_move_times_last(h, out.ctypes.data))
        return dict(zip(("build", "regather", "readback", "layout", "upload"), (float(x) for x in out)))

    def scene_create_triangles(self, tris: dict, device: int = 0):
        """mt_scene_create_triangles.  tris: tri_vertex, tri_normal, tri_uvw ((n, 9) doubles), tri_material, tri_line_no
        (n int32) in ADD order, materials and textures as in scene_create's flat.  Returns (scene handle, build info)."""
        keep = []

        def arr(name, dt):
            a = np.ascontiguousarray(tris[name], dtype=dt)
            keep.append(a)
            return a.ctypes.data if a.size else None

        d = mt_triangle_desc()
        d.struct_size = C.sizeof(mt_triangle_desc)
        d.abi_version = MT_ABI_VERSION
        d.device = device
        d.n_tris = len(tris["tri_material"])
        d.tri_vertex = arr("tri_vertex", np.float64)
        d.tri_normal = arr("tri_normal", np.float64)
        d.tri_uvw = arr("tri_uvw", np.float64)
        d.tri_material = arr("tri_material", np.int32)
        d.tri_line_no = arr("tri_line_no", np.int32)
        mats = tris.get("materials", [])
        texs = tris.get("textures", [])
        marr = self._material_array(mats)
        tarr = self._texture_array(texs, keep)
        d.n_materials, d.n_textures = len(mats), len(texs)
        d.materials = C.cast(marr, C.c_void_p)
        d.textures = C.cast(tarr, C.c_void_p)
        info = mt_build_info()
        h = self.lib.mt_scene_create_triangles(C.byref(d), C.byref(info))
        if not h:
            raise RuntimeError("mt_scene_create_triangles failed: " + self.last_error())
        return h, info.as_dict()

    def set_lights(self, h, lights):
        l = _f64(lights).reshape(-1, 12)
        self.check(self.lib.mt_scene_set_lights(h, _ptr(l), l.shape[0]))

    def set_materials(self, h, mats):
        """mt_scene_set_materials: the constants of ALL the scene's materials replaced.  `mats` as flat["materials"] of
        MythTracer.flatten(): a list, in the scene's order, of dict(values = 16 doubles, tex = index or -1)."""
        mats = list(mats)
        marr = self._material_array(mats)
        self.check(self.lib.mt_scene_set_materials(h, C.cast(marr, C.c_void_p) if mats else None, len(mats)))

    def get_materials(self, h, n):
        """mt_scene_get_materials: the scene's current `n` materials in set_materials' form."""
        marr = (mt_material * max(n, 1))()
        self.check(self.lib.mt_scene_get_materials(h, C.cast(marr, C.c_void_p), n))
        out = []
        for i in range(n):
            m = marr[i]
            v = np.array(list(m.ambient) + list(m.diffuse) + list(m.specular) +
                         [m.specular_exp, m.reflectance, m.transparency] + list(m.transmission_filter) +
                         [m.refraction_index], dtype=np.float64)
            out.append(dict(values=v, tex=int(m.tex)))
        return out

    def set_texture(self, h, index, texels):
        """mt_scene_set_texture: texture `index` of the uploaded scene replaced by `texels`, an array (height, width, 3)
        of uint8 (MT_TEX_RGB8) or float64 (MT_TEX_F64) as in flat["textures"] of MythTracer.flatten().  Size and
        format may change.  Every ray tree of the scene is stale afterwards."""
        texels = np.ascontiguousarray(texels)
        if texels.ndim != 3 or texels.shape[2] != 3 or texels.dtype not in (np.uint8, np.float64):
            raise ValueError("texels must be (height, width, 3) of uint8 or float64")
        t = mt_texture()
        t.height, t.width = texels.shape[0], texels.shape[1]
        t.format = MT_TEX_RGB8 if texels.dtype == np.uint8 else MT_TEX_F64
        t.texels = texels.ctypes.data
        self.check(self.lib.mt_scene_set_texture(h, index, C.byref(t)))

    def get_texture_info(self, h, index) -> dict:
        """mt_scene_get_texture_info: dict(width, height, format) of the scene's texture `index` as it now is."""
        t = mt_texture()
        self.check(self.lib.mt_scene_get_texture_info(h, index, C.byref(t)))
        return dict(width=int(t.width), height=int(t.height), format=int(t.format))

    def set_raytree_uvw(self, h, keep: bool):
        """mt_scene_set_raytree_uvw: ray trees made from now on keep (True) or do not keep (False, the default) a uvw
        plane per layer, which update_materials / regrow need to take texture edits."""
        self.check(self.lib.mt_scene_set_raytree_uvw(h, 1 if keep else 0))

    def set_triangle_materials(self, h, tri_material):
        """mt_scene_set_triangle_materials: the whole per-triangle material index array replaced, in node-stream order
        as flat["tri_material"] of MythTracer.flatten() has it (-1 = no material).  Every ray tree of the scene is
        stale afterwards when an entry changed."""
        a = np.ascontiguousarray(tri_material, dtype=np.int32).reshape(-1)
        self.check(self.lib.mt_scene_set_triangle_materials(h, a.ctypes.data if a.size else None, int(a.size)))

    def get_triangle_materials(self, h, n_tris) -> np.ndarray:
        """mt_scene_get_triangle_materials: the scene's current assignment, (n_tris,) int32."""
        out = np.zeros(max(n_tris, 0), dtype=np.int32)
        self.check(self.lib.mt_scene_get_triangle_materials(h, out.ctypes.data if out.size else None, n_tris))
        return out

    def set_raytree_tri(self, h, keep: bool):
        """mt_scene_set_raytree_tri: ray trees made from now on keep (True) or do not keep (False, the default) a tri
        plane per layer, which update_materials / regrow need to take a set_triangle_materials."""
        self.check(self.lib.mt_scene_set_raytree_tri(h, 1 if keep else 0))

    def _set_triangle_attr(self, fn, h, attr):
        a = np.ascontiguousarray(attr, dtype=np.float64)
        if a.size % 9:
            raise ValueError("a triangle attribute array holds 9 doubles per triangle, not %d in all" % a.size)
        self.check(fn(h, a.ctypes.data if a.size else None, a.size // 9))

    def _get_triangle_attr(self, fn, h, n_tris) -> np.ndarray:
        out = np.zeros((max(n_tris, 0), 3, 3), dtype=np.float64)
        self.check(fn(h, out.ctypes.data if out.size else None, n_tris))
        return out

    def set_triangle_normals(self, h, tri_normal):
        """mt_scene_set_triangle_normals: the whole per-vertex normal array replaced, (n_tris, 3, 3) doubles in
        node-stream order as flat["tri_normal"] of MythTracer.flatten() has it.  Every ray tree of the scene is stale
        afterwards when a triangle changed."""
        self._set_triangle_attr(self.lib.mt_scene_set_triangle_normals, h, tri_normal)

    def set_triangle_uvw(self, h, tri_uvw):
        """mt_scene_set_triangle_uvw: the same for the per-vertex texture coordinates, flat["tri_uvw"]."""
        self._set_triangle_attr(self.lib.mt_scene_set_triangle_uvw, h, tri_uvw)

    def get_triangle_normals(self, h, n_tris) -> np.ndarray:
        """mt_scene_get_triangle_normals: the scene's current normals, (n_tris, 3, 3) float64, read from the device."""
        return self._get_triangle_attr(self.lib.mt_scene_get_triangle_normals, h, n_tris)

    def get_triangle_uvw(self, h, n_tris) -> np.ndarray:
        """mt_scene_get_triangle_uvw: the scene's current texture coordinates, (n_tris, 3, 3) float64."""
        return self._get_triangle_attr(self.lib.mt_scene_get_triangle_uvw, h, n_tris)

    def raytree_attr_info(self, tree) -> dict:
        """mt_raytree_attr_info_last: what the tree's last update_materials / regrow did for edited vertex attributes
        -- renormaled, reuvwed (rays whose planes were rewritten), respawned (reflected children traced again)."""
        info = mt_raytree_attr_info()
        self.check(self.lib.mt_raytree_attr_info_last(tree, C.byref(info)))
        return info.as_dict()

    def retexture_gbuffer(self, h, gbuffer) -> dict:
        """mt_retexture_gbuffer: the albedo plane of `gbuffer` (dict with `material` (ch, cw) int32 and, unless no
        current material has a texture, `uvw` (ch, cw, 3) float64) under the scene's CURRENT materials and textures.
        Returns dict(albedo (ch, cw, 3), stats); the caller's planes are not written."""
        if "material" not in gbuffer:
            raise ValueError("the retexture needs the G-buffer plane 'material'")
        m = np.ascontiguousarray(gbuffer["material"], dtype=np.int32)
        if m.ndim != 2:
            raise ValueError("G-buffer plane 'material' has shape %s, not (rows, columns)" % (m.shape,))
        ch, cw = m.shape
        uvw = None
        if gbuffer.get("uvw") is not None:
            uvw = np.ascontiguousarray(gbuffer["uvw"], dtype=np.float64)
            if uvw.shape != (ch, cw, 3):
                raise ValueError("G-buffer plane 'uvw' has shape %s, not that of the %dx%d chunk" % (uvw.shape, cw, ch))
        albedo = np.zeros((ch, cw, 3), dtype=np.float64)
        g = mt_gbuffer(material=m.ctypes.data, uvw=_ptr(uvw), albedo=albedo.ctypes.data)
        st = mt_stats()
        self.check(self.lib.mt_retexture_gbuffer(h, cw, ch, C.byref(g), C.addressof(st)))
        return dict(albedo=albedo, stats=st.as_dict())

    def retexture_gbuffer_device(self, h, chunk_w, chunk_h, d_gb_planes, stream=None):
        """mt_retexture_gbuffer_device: dict plane name -> device pointer (material, albedo, uvw); asynchronous."""
        for n in d_gb_planes:
            if n not in GBUFFER_PLANES:
                raise ValueError("unknown G-buffer plane %r" % (n,))
        val = lambda p: p.value if isinstance(p, C.c_void_p) else p  # noqa: E731
        g = mt_gbuffer(**{n: val(p) for n, p in d_gb_planes.items()})
        self.check(self.lib.mt_retexture_gbuffer_device(h, chunk_w, chunk_h, C.byref(g), stream))

    def set_traversal_mode(self, h, mode: int):
        self.check(self.lib.mt_scene_set_traversal_mode(h, mode))

    def render_chunk(self, h, sensor12, image_w, image_h, chunk=None, max_depth=5, debug=False):
        cx, cy, cw, ch = chunk if chunk else (0, 0, image_w, image_h)
        rgb = np.zeros((max(ch, 0), max(cw, 0), 3), dtype=np.uint8)
        dbg = np.zeros((max(ch, 0), max(cw, 0)), dtype=DEBUG_PX_DTYPE) if debug else None
        st = mt_stats()
        s = self.make_sensor(sensor12)
        self.check(self.lib.mt_render_chunk(h, C.byref(s), image_w, image_h, cx, cy, cw, ch,
                                            max_depth, _ptr(rgb), _ptr(dbg), C.addressof(st)))
        out = dict(rgb=rgb, stats=st.as_dict())
        if debug:
            out["line"] = dbg["line_no"].copy()
            out["point"] = dbg["point"].copy()
        return out

    def render_chunk_device(self, h, sensor12, image_w, image_h, chunk, max_depth, d_rgb,
                            d_debug=None, stream=None):
        s = self.make_sensor(sensor12)
        self.check(self.lib.mt_render_chunk_device(h, C.byref(s), image_w, image_h, *chunk,
                                                   max_depth, d_rgb, d_debug, stream))

    def render_tiles_device(self, h, sensor12, image_w, image_h, tile_w, tile_h, first_tile,
                            tile_stride, n_tiles, max_depth, d_rgb, stream=None):
        s = self.make_sensor(sensor12)
        self.check(self.lib.mt_render_tiles_device(h, C.byref(s), image_w, image_h, tile_w, tile_h,
                                                   first_tile, tile_stride, n_tiles, max_depth,
                                                   d_rgb, stream))

    def blit_tiles_device(self, h, image_w, image_h, tile_w, tile_h, first_tile, tile_stride,
                          n_tiles, d_tiles, d_image, stream=None):
        self.check(self.lib.mt_blit_tiles_device(h, image_w, image_h, tile_w, tile_h, first_tile,
                                                 tile_stride, n_tiles, d_tiles, d_image, stream))

    # ---- cost-balanced tile ownership (include/mythtracer_hip.h, mt_order_tiles_device ff.)
    def order_tiles_device(self, h, d_cost_map, map_w, map_h, image_w, image_h, tile_w, tile_h, d_order, stream=None):
        self.check(self.lib.mt_order_tiles_device(h, d_cost_map, map_w, map_h, image_w, image_h, tile_w, tile_h,
                                                  d_order, stream))

    def dealt_tile_count(self, image_w, image_h, tile_w, tile_h, world, rank) -> int:
        n = self.lib.mt_dealt_tile_count(image_w, image_h, tile_w, tile_h, world, rank)
        if n < 0:
            self.check(n)
        return n

    def deal_tiles_device(self, h, d_order, image_w, image_h, tile_w, tile_h, world, rank, d_list, stream=None) -> int:
        n = self.lib.mt_deal_tiles_device(h, d_order, image_w, image_h, tile_w, tile_h, world, rank, d_list, stream)
        if n < 0:
            self.check(n)
        return n

    def render_tile_list_device(self, h, sensor12, image_w, image_h, tile_w, tile_h, d_list, n_tiles, list_id,
                                max_depth, d_rgb, stream=None):
        s = self.make_sensor(sensor12)
        self.check(self.lib.mt_render_tile_list_device(h, C.byref(s), image_w, image_h, tile_w, tile_h, d_list,
                                                       n_tiles, int(list_id), max_depth, d_rgb, stream))

    def blit_tile_list_device(self, h, image_w, image_h, tile_w, tile_h, d_list, n_tiles, d_tiles, d_image,
                              stream=None):
        self.check(self.lib.mt_blit_tile_list_device(h, image_w, image_h, tile_w, tile_h, d_list, n_tiles,
                                                     d_tiles, d_image, stream))

    # ---- supersampled frames (include/mythtracer_hip.h, mt_render_chunk_ss ff.): sensor12 is the sensor of the SAMPLE
    # grid, ss image_w x ss image_h; image_*, chunk and tile_* are the output geometry
    def render_chunk_ss(self, h, sensor12, image_w, image_h, ss, chunk=None, max_depth=5):
        cx, cy, cw, ch = chunk if chunk else (0, 0, image_w, image_h)
        rgb = np.zeros((max(ch, 0), max(cw, 0), 3), dtype=np.uint8)
        st = mt_stats()
        s = self.make_sensor(sensor12)
        self.check(self.lib.mt_render_chunk_ss(h, C.byref(s), image_w, image_h, cx, cy, cw, ch, ss, max_depth,
                                               _ptr(rgb), C.addressof(st)))
        return dict(rgb=rgb, stats=st.as_dict())

    def render_chunk_ss_device(self, h, sensor12, image_w, image_h, chunk, ss, max_depth, d_rgb, stream=None):
        s = self.make_sensor(sensor12)
        self.check(self.lib.mt_render_chunk_ss_device(h, C.byref(s), image_w, image_h, *chunk, ss, max_depth,
                                                      d_rgb, stream))

    def resolve_tiles_device(self, h, image_w, image_h, tile_w, tile_h, first_tile, tile_stride, d_list, n_tiles,
                             ss, d_samples, d_tiles, stream=None):
        self.check(self.lib.mt_resolve_tiles_device(h, image_w, image_h, tile_w, tile_h, first_tile, tile_stride,
                                                    d_list, n_tiles, ss, d_samples, d_tiles, stream))

    # ---- adaptive supersampling (include/mythtracer_hip.h, mt_render_chunk_adaptive ff.): sensor12 is the sensor of
    # the output grid, sensor12_ss the sensor of the sample grid (None with ss = 1 only)
    def render_chunk_adaptive(self, h, sensor12, sensor12_ss, image_w, image_h, ss, threshold, chunk=None, max_depth=5):
        """mt_render_chunk_adaptive: dict rgb (the chunk), mask (bool [mask_h][mask_w], tiling.chunk_blocks), info
        (mt_adaptive_info as a dict), stats."""
        from .tiling import chunk_blocks
        cx, cy, cw, ch = chunk if chunk else (0, 0, image_w, image_h)
        rgb = np.zeros((max(ch, 0), max(cw, 0), 3), dtype=np.uint8)
        _, _, mw, mh = chunk_blocks((cx, cy, max(cw, 1), max(ch, 1)))
        mask = np.zeros((mh, mw), dtype=np.uint8)
        st, info = mt_stats(), mt_adaptive_info()
        s = self.make_sensor(sensor12)
        s_ss = C.byref(self.make_sensor(sensor12_ss)) if sensor12_ss is not None else None
        self.check(self.lib.mt_render_chunk_adaptive(h, C.byref(s), s_ss, image_w, image_h, cx, cy, cw, ch, ss,
                                                     threshold, max_depth, _ptr(rgb), _ptr(mask), C.byref(info),
                                                     C.addressof(st)))
        return dict(rgb=rgb, mask=mask.astype(bool), info=info.as_dict(), stats=st.as_dict())

    def render_chunk_adaptive_device(self, h, sensor12, sensor12_ss, image_w, image_h, chunk, ss, threshold, max_depth,
                                     d_rgb, d_mask=None, stream=None):
        """mt_render_chunk_adaptive_device (synchronises `stream` once, see the header); returns the info dict."""
        info = mt_adaptive_info()
        s = self.make_sensor(sensor12)
        s_ss = C.byref(self.make_sensor(sensor12_ss)) if sensor12_ss is not None else None
        self.check(self.lib.mt_render_chunk_adaptive_device(h, C.byref(s), s_ss, image_w, image_h, *chunk, ss, threshold,
                                                            max_depth, d_rgb, d_mask, C.byref(info), stream))
        return info.as_dict()

    def refine_mask_device(self, h, image_w, image_h, chunk, threshold, d_rgb, d_mask, d_list, d_count, stream=None):
        self.check(self.lib.mt_refine_mask_device(h, image_w, image_h, *chunk, threshold, d_rgb, d_mask, d_list,
                                                  d_count, stream))

    # ---- the primary-hit G-buffer (include/mythtracer_hip.h, mt_render_gbuffer)
    def render_gbuffer(self, h, sensor12, image_w, image_h, chunk=None, channels=None):
        """mt_render_gbuffer: dict plane name -> numpy array of the chunk ((ch, cw) or (ch, cw, 3)) for the planes
        named in `channels` (None = all of GBUFFER_PLANES), plus "stats"."""
        cx, cy, cw, ch = chunk if chunk else (0, 0, image_w, image_h)
        out = _gbuffer_arrays(channels, cw, ch)
        g = mt_gbuffer(**{n: a.ctypes.data for n, a in out.items()})
        st = mt_stats()
        s = self.make_sensor(sensor12)
        self.check(self.lib.mt_render_gbuffer(h, C.byref(s), image_w, image_h, cx, cy, cw, ch, C.byref(g),
                                              C.addressof(st)))
        out["stats"] = st.as_dict()
        return out

    def render_gbuffer_device(self, h, sensor12, image_w, image_h, chunk, d_planes, stream=None):
        """mt_render_gbuffer_device: d_planes = dict plane name -> device pointer (int or c_void_p) of the planes
        wanted; asynchronous on `stream`."""
        for n in d_planes:
            if n not in GBUFFER_PLANES:
                raise ValueError("unknown G-buffer plane %r" % (n,))
        g = mt_gbuffer(**{n: (p.value if isinstance(p, C.c_void_p) else p) for n, p in d_planes.items()})
        s = self.make_sensor(sensor12)
        self.check(self.lib.mt_render_gbuffer_device(h, C.byref(s), image_w, image_h, *chunk, C.byref(g), stream))

    # ---- the direct-light buffer and the relight pass (include/mythtracer_hip.h, mt_render_lightbuffer)
    def render_lightbuffer(self, h, sensor12, image_w, image_h, n_lights, chunk=None, channels=None,
                           gbuffer_channels=()):
        """mt_render_lightbuffer for a scene whose n_lights lights are set: dict with the light-buffer planes named in
        `channels` (None = both; (n_lights, ch, cw, 3) float64 `power`, (n_lights, ch, cw) uint8 `in_shadow`), the
        G-buffer planes named in `gbuffer_channels` (None = all, default none) from the same launch, and "stats"."""
        cx, cy, cw, ch = chunk if chunk else (0, 0, image_w, image_h)
        out = _lightbuffer_arrays(channels, n_lights, cw, ch)
        lb = mt_lightbuffer(**{n: a.ctypes.data for n, a in out.items()})
        planes = _gbuffer_arrays(gbuffer_channels, cw, ch)
        g = mt_gbuffer(**{n: a.ctypes.data for n, a in planes.items()})
        st = mt_stats()
        s = self.make_sensor(sensor12)
        self.check(self.lib.mt_render_lightbuffer(h, C.byref(s), image_w, image_h, cx, cy, cw, ch,
                                                  C.byref(g) if planes else None, C.byref(lb), C.addressof(st)))
        out.update(planes)
        out["stats"] = st.as_dict()
        return out

    def render_lightbuffer_device(self, h, sensor12, image_w, image_h, chunk, d_lb_planes, d_gb_planes=None, stream=None):
        """mt_render_lightbuffer_device: dicts plane name -> device pointer; asynchronous on `stream`."""
        for n in d_lb_planes:
            if n not in LIGHTBUFFER_PLANES:
                raise ValueError("unknown light-buffer plane %r" % (n,))
        for n in d_gb_planes or {}:
            if n not in GBUFFER_PLANES:
                raise ValueError("unknown G-buffer plane %r" % (n,))
        val = lambda p: p.value if isinstance(p, C.c_void_p) else p  # noqa: E731
        lb = mt_lightbuffer(**{n: val(p) for n, p in d_lb_planes.items()})
        g = mt_gbuffer(**{n: val(p) for n, p in (d_gb_planes or {}).items()})
        s = self.make_sensor(sensor12)
        self.check(self.lib.mt_render_lightbuffer_device(h, C.byref(s), image_w, image_h, *chunk,
                                                         C.byref(g) if d_gb_planes else None, C.byref(lb), stream))

    def shade_direct(self, h, sensor12, image_w, image_h, gbuffer, lightbuffer, lights, chunk=None):
        """mt_shade_direct: the frame of the direct term from the planes of render_gbuffer / render_lightbuffer (dicts
        of numpy arrays of the chunk) under `lights` (n x 12: position, ambient, diffuse, specular -- positions and
        count as when the light buffer was made).  Returns dict(rgb, stats)."""
        cx, cy, cw, ch = chunk if chunk else (0, 0, image_w, image_h)
        gp, lp, n_l = _relight_planes(gbuffer, lightbuffer, cw, ch)
        l = _f64(lights).reshape(-1, 12)
        if l.shape[0] != n_l:
            raise ValueError("%d lights for a light buffer of %d" % (l.shape[0], n_l))
        g = mt_gbuffer(**{n: a.ctypes.data for n, a in gp.items()})
        lb = mt_lightbuffer(**{n: a.ctypes.data for n, a in lp.items()})
        rgb = np.zeros((ch, cw, 3), dtype=np.uint8)
        st = mt_stats()
        s = self.make_sensor(sensor12)
        self.check(self.lib.mt_shade_direct(h, C.byref(s), image_w, image_h, cx, cy, cw, ch, C.byref(g), C.byref(lb),
                                            _ptr(l), n_l, _ptr(rgb), C.addressof(st)))
        return dict(rgb=rgb, stats=st.as_dict())

    def shade_direct_device(self, h, sensor12, image_w, image_h, chunk, d_gb_planes, d_lb_planes, lights, d_rgb,
                            stream=None):
        """mt_shade_direct_device: dicts plane name -> device pointer, `lights` a host array (n x 12)."""
        val = lambda p: p.value if isinstance(p, C.c_void_p) else p  # noqa: E731
        g = mt_gbuffer(**{n: val(p) for n, p in d_gb_planes.items()})
        lb = mt_lightbuffer(**{n: val(p) for n, p in d_lb_planes.items()})
        l = _f64(lights).reshape(-1, 12)
        s = self.make_sensor(sensor12)
        self.check(self.lib.mt_shade_direct_device(h, C.byref(s), image_w, image_h, *chunk, C.byref(g), C.byref(lb),
                                                   _ptr(l), l.shape[0], d_rgb, stream))

    def update_lightbuffer(self, h, gbuffer, lightbuffer, light_indices):
        """mt_update_lightbuffer after set_lights(the moved lights): the planes of the lights in `light_indices` of
        `lightbuffer` (dict with `power` and / or `in_shadow`, numpy arrays of the chunk for the scene's current number
        of lights) traced again from the `point` and `material` planes of `gbuffer`.  The arrays are updated IN PLACE
        -- the planes of the other lights are neither read nor written.  Returns dict(those arrays, stats)."""
        g, lb, n_l, cw, ch = _update_planes(gbuffer, lightbuffer)
        idx = _i32(light_indices).reshape(-1)
        gs = mt_gbuffer(**{n: a.ctypes.data for n, a in g.items()})
        ls = mt_lightbuffer(**{n: a.ctypes.data for n, a in lb.items()})
        st = mt_stats()
        self.check(self.lib.mt_update_lightbuffer(h, cw, ch, C.byref(gs), _ptr(idx), len(idx), C.byref(ls),
                                                  C.addressof(st)))
        out = dict(lb)
        out["stats"] = st.as_dict()
        return out

    def update_lightbuffer_device(self, h, chunk_w, chunk_h, d_gb_planes, d_lb_planes, light_indices, stream=None):
        """mt_update_lightbuffer_device: dicts plane name -> device pointer, `light_indices` a host list."""
        for n in d_lb_planes:
            if n not in LIGHTBUFFER_PLANES:
                raise ValueError("unknown light-buffer plane %r" % (n,))
        for n in d_gb_planes:
            if n not in GBUFFER_PLANES:
                raise ValueError("unknown G-buffer plane %r" % (n,))
        val = lambda p: p.value if isinstance(p, C.c_void_p) else p  # noqa: E731
        g = mt_gbuffer(**{n: val(p) for n, p in d_gb_planes.items()})
        lb = mt_lightbuffer(**{n: val(p) for n, p in d_lb_planes.items()})
        idx = _i32(light_indices).reshape(-1)
        self.check(self.lib.mt_update_lightbuffer_device(h, chunk_w, chunk_h, C.byref(g), _ptr(idx), len(idx),
                                                         C.byref(lb), stream))

    # ---- the ray-tree buffer (include/mythtracer_hip.h, mt_raytree_create)
    def raytree_create(self, h, sensor12, image_w, image_h, chunk=None, max_depth=5):
        """mt_raytree_create under the scene's current lights: (tree handle, stats dict).  raytree_destroy it before
        the scene."""
        cx, cy, cw, ch = chunk if chunk else (0, 0, image_w, image_h)
        st = mt_stats()
        s = self.make_sensor(sensor12) if sensor12 is not None else None
        t = self.lib.mt_raytree_create(h, C.byref(s) if s is not None else None, image_w, image_h, cx, cy, cw, ch,
                                       max_depth, C.addressof(st))
        if not t:
            raise RuntimeError("mythtracer_hip error: mt_raytree_create: %s" % self.last_error())
        return t, st.as_dict()

    def raytree_destroy(self, tree):
        self.lib.mt_raytree_destroy(tree)

    def raytree_info(self, tree) -> dict:
        d = mt_raytree_desc()
        self.check(self.lib.mt_raytree_info(tree, C.byref(d)))
        return d.as_dict()

    def raytree_read_layer(self, tree, layer, planes=None) -> dict:
        """mt_raytree_read_layer: dict plane name -> numpy array of the layer's n rays ((n,), (n, 3), (n, 6); power
        (n_lights, n, 3), in_shadow (n_lights, n)) for the planes named (None = all; `pixel` for layer 0 only)."""
        info = self.raytree_info(tree)
        if not 0 <= layer < info["n_layers"]:
            raise ValueError("layer %d outside the tree's %d layers" % (layer, info["n_layers"]))
        names = [n for n in RAYTREE_PLANES if n != "pixel" or layer == 0] if planes is None else list(planes)
        n, n_l = info["n_rays"][layer], info["n_lights"]
        out = {}
        for name in names:
            if name not in RAYTREE_PLANES:
                raise ValueError("unknown ray-tree plane %r (planes: %s)" % (name, ", ".join(RAYTREE_PLANES)))
            dt, k, per_light = RAYTREE_PLANES[name]
            out[name] = np.zeros(((n_l,) if per_light else ()) + (n,) + ((k,) if k > 1 else ()), dtype=dt)
        ls = mt_raytree_layer(**{name: (a.ctypes.data if a.size else None) for name, a in out.items()})
        self.check(self.lib.mt_raytree_read_layer(tree, layer, C.byref(ls)))
        return out

    def raytree_keeps_uvw(self, tree) -> bool:
        """mt_raytree_keeps_uvw: was the tree made while the scene's set_raytree_uvw switch was on?"""
        rc = self.lib.mt_raytree_keeps_uvw(tree)
        if rc < 0:
            self.check(rc)
        return bool(rc)

    def raytree_read_uvw(self, tree, layer) -> np.ndarray:
        """mt_raytree_read_uvw: the layer's uvw plane, (n, 3) float64, NaN for a miss; a RuntimeError for a tree that
        keeps none."""
        info = self.raytree_info(tree)
        if not 0 <= layer < info["n_layers"]:
            raise ValueError("layer %d outside the tree's %d layers" % (layer, info["n_layers"]))
        out = np.zeros((info["n_rays"][layer], 3), dtype=np.float64)
        self.check(self.lib.mt_raytree_read_uvw(tree, layer, out.ctypes.data))
        return out

    def raytree_keeps_tri(self, tree) -> bool:
        """mt_raytree_keeps_tri: was the tree made while the scene's set_raytree_tri switch was on?"""
        rc = self.lib.mt_raytree_keeps_tri(tree)
        if rc < 0:
            self.check(rc)
        return bool(rc)

    def raytree_read_tri(self, tree, layer) -> np.ndarray:
        """mt_raytree_read_tri: the layer's tri plane, (n,) int32 stream indices, -1 for a miss; a RuntimeError for a
        tree that keeps none."""
        info = self.raytree_info(tree)
        if not 0 <= layer < info["n_layers"]:
            raise ValueError("layer %d outside the tree's %d layers" % (layer, info["n_layers"]))
        out = np.zeros(info["n_rays"][layer], dtype=np.int32)
        self.check(self.lib.mt_raytree_read_tri(tree, layer, out.ctypes.data if out.size else None))
        return out

    def raytree_shade(self, tree, lights) -> dict:
        """mt_raytree_shade under `lights` (n x 12; count and positions as when the tree was made): dict(rgb, stats)."""
        info = self.raytree_info(tree)
        l = _f64(lights).reshape(-1, 12)
        _, _, cw, ch = info["chunk"]
        rgb = np.zeros((ch, cw, 3), dtype=np.uint8)
        st = mt_stats()
        self.check(self.lib.mt_raytree_shade(tree, _ptr(l), l.shape[0], _ptr(rgb), C.addressof(st)))
        return dict(rgb=rgb, stats=st.as_dict())

    def raytree_shade_device(self, tree, lights, d_rgb, stream=None):
        """mt_raytree_shade_device: `lights` a host array (n x 12), d_rgb a device pointer; asynchronous on `stream`."""
        l = _f64(lights).reshape(-1, 12)
        self.check(self.lib.mt_raytree_shade_device(tree, _ptr(l), l.shape[0], d_rgb, stream))

    def raytree_update_lights(self, tree, light_indices) -> dict:
        """mt_raytree_update_lights after set_lights(the moved lights): the planes of the lights in `light_indices`
        in every layer of `tree` traced again from the stored hits.  Returns the stats dict."""
        idx = _i32(light_indices).reshape(-1)
        st = mt_stats()
        self.check(self.lib.mt_raytree_update_lights(tree, _ptr(idx), len(idx), C.addressof(st)))
        return st.as_dict()

    def raytree_update_materials(self, tree) -> dict:
        """mt_raytree_update_materials after set_materials: `tree` brought to the scene's current materials, or a
        RuntimeError (code -3: the edit changes the tree's shape or, for a tree without uvw, a textured material's
        ambient or a texture in use) with the tree as it was.  Returns the stats dict."""
        st = mt_stats()
        self.check(self.lib.mt_raytree_update_materials(tree, C.addressof(st)))
        return st.as_dict()

    def raytree_regrow(self, tree) -> dict:
        """mt_raytree_regrow_materials after set_materials: `tree` brought to the scene's current materials whatever
        the edit does to its shape -- surviving rays kept, dead subtrees dropped, new rays traced.  Returns
        mt_raytree_regrow_info's fields (regrown, n_layers_before / _after, kept, traced, dropped per layer) and the
        stats, in one dict."""
        st = mt_stats()
        info = mt_raytree_regrow_info()
        self.check(self.lib.mt_raytree_regrow_materials(tree, C.addressof(info), C.addressof(st)))
        out = info.as_dict()
        out.update(st.as_dict())
        return out

    def raytree_update_lights_device(self, tree, light_indices, stream=None):
        """mt_raytree_update_lights_device: `light_indices` a host list; asynchronous on `stream`."""
        idx = _i32(light_indices).reshape(-1)
        self.check(self.lib.mt_raytree_update_lights_device(tree, _ptr(idx), len(idx), stream))

    # ---- ray-list trees and linear colours (include/mythtracer_hip.h, mt_raytree_create_rays)
    @staticmethod
    def _ray_list(rays, list_w, in_object, coef, device):
        """(mt_ray_list, what must stay alive, (list_w, list_h)).  Host form: array-likes, (n, 6) / (n,) / (n,).  Device
        form: tensors on the scene's GPU (anything with data_ptr() and numel(): float64, uint8, float64)."""
        if device:
            n = int(rays.numel()) // 6
            keep = [rays, in_object, coef]
            ptr = [None if a is None else a.data_ptr() for a in keep]
            sizes = [int(rays.numel()), None if in_object is None else int(in_object.numel()),
                     None if coef is None else int(coef.numel())]
        else:
            r = _f64(rays).reshape(-1, 6)
            n = r.shape[0]
            keep = [r, None if in_object is None else np.ascontiguousarray(np.asarray(in_object, dtype=np.uint8)).reshape(-1),
                    None if coef is None else _f64(coef).reshape(-1)]
            ptr = [_ptr(a) for a in keep]
            sizes = [r.size] + [None if a is None else a.size for a in keep[1:]]
        if sizes[0] != n * 6 or any(v is not None and v != n for v in sizes[1:]):
            raise ValueError("rays (n, 6), in_object (n,) and coef (n,) must describe the same n rays")
        if list_w is None:
            list_w = n
        if n == 0 or list_w < 1 or n % list_w:
            raise ValueError("a list of %d rays cannot be %s wide" % (n, list_w))
        rl = mt_ray_list(ptr[0], ptr[1], ptr[2], list_w, n // list_w)
        return rl, keep, (list_w, n // list_w)

    def raytree_create_rays(self, h, rays, list_w=None, in_object=None, coef=None, max_depth=5, device=False):
        """mt_raytree_create_rays[_device] under the scene's current lights: (tree handle, stats dict).  `rays` (n, 6)
        in the caller's order, list_w None = an n x 1 list; device=True: tensors on the scene's GPU, finished."""
        rl, keep, _ = self._ray_list(rays, list_w, in_object, coef, device)
        st = mt_stats()
        fn = self.lib.mt_raytree_create_rays_device if device else self.lib.mt_raytree_create_rays
        t = fn(h, C.addressof(rl), max_depth, C.addressof(st))
        del keep
        if not t:
            raise RuntimeError("mythtracer_hip error: %s: %s" % (
                "mt_raytree_create_rays_device" if device else "mt_raytree_create_rays", self.last_error()))
        return t, st.as_dict()

    def raytree_shade_colors(self, tree, lights) -> dict:
        """mt_raytree_shade_colors under `lights`: dict(color (chunk_h, chunk_w, 3) float64 before V3DtoRGB, stats)."""
        info = self.raytree_info(tree)
        l = _f64(lights).reshape(-1, 12)
        _, _, cw, ch = info["chunk"]
        color = np.zeros((ch, cw, 3), dtype=np.float64)
        st = mt_stats()
        self.check(self.lib.mt_raytree_shade_colors(tree, _ptr(l), l.shape[0], _ptr(color), C.addressof(st)))
        return dict(color=color, stats=st.as_dict())

    def raytree_shade_colors_device(self, tree, lights, d_color, stream=None):
        """mt_raytree_shade_colors_device: `lights` a host array (n x 12), d_color a device pointer to n x 3 doubles;
        asynchronous on `stream`."""
        l = _f64(lights).reshape(-1, 12)
        self.check(self.lib.mt_raytree_shade_colors_device(tree, _ptr(l), l.shape[0], d_color, stream))

    def trace_rays(self, h, rays, list_w=None, in_object=None, coef=None, max_depth=5, color=True, rgb=True) -> dict:
        """mt_trace_rays under the scene's current lights: dict(color (list_h, list_w, 3) float64 and / or rgb
        (list_h, list_w, 3) uint8 -- whichever was asked for --, stats)."""
        rl, keep, (w, hh) = self._ray_list(rays, list_w, in_object, coef, False)
        out = {}
        if color:
            out["color"] = np.zeros((hh, w, 3), dtype=np.float64)
        if rgb:
            out["rgb"] = np.zeros((hh, w, 3), dtype=np.uint8)
        st = mt_stats()
        self.check(self.lib.mt_trace_rays(h, C.addressof(rl), max_depth, _ptr(out.get("color")), _ptr(out.get("rgb")),
                                          C.addressof(st)))
        del keep
        out["stats"] = st.as_dict()
        return out

    def read_stats(self, h) -> dict:
        st = mt_stats()
        self.check(self.lib.mt_scene_read_stats(h, C.byref(st)))
        return st.as_dict()

    def set_stats(self, h, enabled: bool):
        """Work counters of the *_device calls on (default) or off."""
        self.check(self.lib.mt_scene_set_stats(h, 1 if enabled else 0))

    def set_engine(self, h, engine: int):
        """0 = automatic, 1 = throughput engine (state machine), 2 = latency engine (ray pool), 3 = hybrid."""
        self.check(self.lib.mt_scene_set_engine(h, int(engine)))

    def set_default_engine(self, engine: int):
        """Engine of the scenes created from now on (also those the C++ facade creates)."""
        self.check(self.lib.mt_set_default_engine(int(engine)))

    def set_tuning(self, h, knob: str, value: float):
        """mt_scene_set_tuning; knob = a key of TUNE (e.g. "POOL_CAP") or of TUNE_EXTRA ("SHADOW_BOUND")."""
        self.check(self.lib.mt_scene_set_tuning(h, TUNE[knob] if knob in TUNE else TUNE_EXTRA[knob], float(value)))

    def render_frame_multi(self, handles, sensor12, image_w, image_h, tile_w=64, tile_h=64, max_depth=5,
                           want_stats=True):
        """mt_render_frame_multi: one frame on the replicas `handles` (one per GPU)."""
        n = len(handles)
        arr = (C.c_void_p * n)(*handles)
        rgb = np.zeros((image_h, image_w, 3), dtype=np.uint8)
        st = (mt_stats * n)()
        s = self.make_sensor(sensor12)
        self.check(self.lib.mt_render_frame_multi(C.cast(arr, C.c_void_p), n, C.byref(s), image_w, image_h,
                                                  tile_w, tile_h, max_depth, _ptr(rgb),
                                                  C.cast(st, C.c_void_p) if want_stats else None))
        return dict(rgb=rgb, stats=[st[i].as_dict() for i in range(n)])

    def export_costs_device(self, h, d_map, map_w, map_h, stream=None):
        self.check(self.lib.mt_scene_export_costs_device(h, d_map, map_w, map_h, stream))

    def import_costs_device(self, h, d_map, map_w, map_h, stream=None):
        self.check(self.lib.mt_scene_import_costs_device(h, d_map, map_w, map_h, stream))

    def set_scheduling(self, h, use_cost_history: bool):
        self.check(self.lib.mt_scene_set_scheduling(h, 1 if use_cost_history else 0))

    def kernel_times(self, h, max_n: int = 64):
        """(primary_ms[], render_ms[]) of the launches since the previous call."""
        a = np.zeros(max_n)
        b = np.zeros(max_n)
        n = self.lib.mt_scene_kernel_times(h, max_n, a.ctypes.data_as(C.c_void_p),
                                           b.ctypes.data_as(C.c_void_p))
        if n < 0:
            self.check(n)
        return a[:n].copy(), b[:n].copy()

    def lean_info(self, h):
        """mt_scene_lean_info: what the scene's last launch was (dict: lean, handed_over, units, redo_units, lean_ms,
        redo_ms).  Waits for the device."""
        info = mt_lean_info()
        self.check(self.lib.mt_scene_lean_info(h, C.byref(info)))
        return info.as_dict()

    def intersect_rays(self, h, rays):
        rays = _f64(rays).reshape(-1, 6)
        n = rays.shape[0]
        tri = np.zeros(n, dtype=np.int32)
        line = np.zeros(n, dtype=np.int32)
        t = np.zeros(n)
        point = np.zeros((n, 3))
        st = mt_stats()
        self.check(self.lib.mt_intersect_rays(h, n, _ptr(rays), _ptr(tri), _ptr(line), _ptr(t),
                                              _ptr(point), C.addressof(st)))
        return dict(tri=tri, line=line, t=t, point=point, stats=st.as_dict())


_hip = None
_host = None


def hip_abi() -> HipAbi:
    global _hip
    if _hip is None:
        _hip = HipAbi()
    return _hip


def host_lib():
    global _host
    if _host is not None:
        return _host
    L = _load(HOST_LIB)
    vp, ci, cd, cs = C.c_void_p, C.c_int, C.c_double, C.c_char_p
    L.mth_new.restype = vp
    L.mth_new.argtypes = [ci, ci]
    L.mth_free.argtypes = [vp]
    L.mth_free.restype = None
    L.mth_set_devices.argtypes = [vp, vp, ci]
    L.mth_set_devices.restype = None
    L.mth_last_error.restype = cs
    L.mth_last_error.argtypes = [vp]
    L.mth_load_obj.argtypes = [vp, cs]
    L.mth_add_material.argtypes = [vp, cs, vp, vp, vp, cd, cd, cd, vp, cd]
    L.mth_add_texture.argtypes = [vp, cs, ci, ci, vp]
    L.mth_material_set_texture.argtypes = [vp, ci, ci]
    L.mth_add_triangle.argtypes = [vp, vp, vp, vp, ci, ci]
    L.mth_set_lights.argtypes = [vp, vp, ci]
    L.mth_set_lights.restype = None
    L.mth_set_max_level.argtypes = [vp, ci]
    L.mth_set_max_level.restype = None
    L.mth_set_supersampling.argtypes = [vp, ci]
    L.mth_set_supersampling.restype = None
    L.mth_set_adaptive_supersampling.argtypes = [vp, ci, ci]
    L.mth_set_adaptive_supersampling.restype = None
    L.mth_finalize.argtypes = [vp]
    L.mth_finalize.restype = None
    L.mth_prepare.argtypes = [vp]
    L.mth_device_scene.argtypes = [vp]
    L.mth_device_scene.restype = vp
    L.mth_root_aabb.argtypes = [vp, vp]
    L.mth_root_aabb.restype = None
    L.mth_tree_info.argtypes = [vp, vp, vp, vp]
    L.mth_tree_info.restype = None
    L.mth_tree_dump.argtypes = [vp] * 7
    L.mth_triangles.argtypes = [vp, vp, vp, vp]
    L.mth_triangles.restype = None
    L.mth_flatten.argtypes = [vp] * 12
    L.mth_flatten_texels.argtypes = [vp, ci, vp]
    L.mth_num_materials.argtypes = [vp]
    L.mth_get_material.argtypes = [vp, cs, vp, vp]
    L.mth_sensor.argtypes = [vp, ci, ci, vp]
    L.mth_sensor.restype = None
    L.mth_sensor_ray.argtypes = [vp, ci, ci, ci, ci, vp]
    L.mth_sensor_ray.restype = None
    L.mth_render_chunk.argtypes = [vp, vp] + [ci] * 6 + [vp] * 5
    L.mth_render_image.argtypes = [vp, vp, ci, ci, vp]
    L.mth_render_gbuffer.argtypes = [vp, vp] + [ci] * 6 + [C.c_uint, vp, vp, vp]
    L.mth_render_lightbuffer.argtypes = [vp, vp] + [ci] * 6 + [C.c_uint, vp, C.c_uint, vp, ci, vp, vp]
    L.mth_shade_direct.argtypes = [vp, vp] + [ci] * 6 + [vp, ci, vp, vp, vp]
    L.mth_update_lightbuffer.argtypes = [vp, ci, ci, vp, vp, ci, C.c_uint, vp, ci, vp, vp]
    L.mth_num_lights.argtypes = [vp]
    L.mth_raytree_build.restype = vp
    L.mth_raytree_build.argtypes = [vp, vp] + [ci] * 6 + [vp, vp]
    L.mth_raytree_free.argtypes = [vp]
    L.mth_raytree_free.restype = None
    L.mth_raytree_handle.argtypes = [vp]
    L.mth_raytree_handle.restype = vp
    L.mth_raytree_shade.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.mth_raytree_update.argtypes = [vp, vp, vp, ci, vp, vp]
    L.mth_update_materials.argtypes = [vp, cs, vp]
    L.mth_raytree_update_materials.argtypes = [vp, vp, vp, vp]
    L.mth_raytree_regrow.argtypes = [vp, vp, vp, vp]
    L.mth_update_texture.argtypes = [vp, cs, ci, ci, vp]
    L.mth_set_raytree_keep_uvw.argtypes = [vp, ci]
    L.mth_set_raytree_keep_uvw.restype = None
    L.mth_assign_material.argtypes = [vp, vp, ci, C.c_char_p]
    L.mth_update_triangle_materials.argtypes = [vp]
    L.mth_set_raytree_keep_triangles.argtypes = [vp, ci]
    L.mth_set_raytree_keep_triangles.restype = None
    L.mth_set_triangle_attr.argtypes = [vp, ci, vp, ci, vp]
    L.mth_update_triangle_attributes.argtypes = [vp]
    L.mth_set_device_tree_build.argtypes = [vp, ci]
    L.mth_set_device_tree_build.restype = None
    L.mth_set_triangle_vertices.argtypes = [vp, vp, ci, vp]
    L.mth_update_geometry.argtypes = [vp]
    L.mth_update_geometry.restype = None
    L.mth_update_geometry_in_place.argtypes = [vp]
    L.mth_add_triangles.argtypes = [vp, ci, vp, vp, vp, C.c_char_p, vp]
    L.mth_remove_triangles.argtypes = [vp, vp, ci]
    L.mth_update_triangles_in_place.argtypes = [vp]
    L.mth_raytree_build_rays.restype = vp
    L.mth_raytree_build_rays.argtypes = [vp, vp, C.c_longlong, ci, vp, vp]
    L.mth_raytree_shade_colors.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.mth_trace_rays.argtypes = [vp, vp, C.c_longlong, ci, vp, vp, vp, vp]
    L.mth_frame_loop.argtypes = [vp, vp, ci, ci, ci, cd, ci, vp, vp]
    L.mth_intersect.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    L.mth_chunk_serialize_input.argtypes = [vp, vp]
    L.mth_chunk_deserialize_input.argtypes = [vp, ci, vp]
    L.mth_chunk_output_roundtrip.argtypes = [ci, ci, vp, ci, vp, ci, vp]
    L.mth_chunk_deserialize_output.argtypes = [ci, ci, vp, ci]
    L.mth_camera_roundtrip.argtypes = [vp, vp, vp]
    _host = L
    return L


def sensor(cam7, w, h):
    """Camera::GetSensor on the host -> origin, start, delta_scanline, delta_pixel."""
    out = np.zeros(12)
    cam = _f64(cam7)  # bound to a name: must outlive the call
    host_lib().mth_sensor(_ptr(cam), w, h, _ptr(out))
    return out


def sensor_ray(cam7, w, h, x, y):
    d = np.zeros(3)
    cam = _f64(cam7)
    host_lib().mth_sensor_ray(_ptr(cam), w, h, x, y, _ptr(d))
    return d


class RayTree:
    """raytracer::RayTree as MythTracer.raytree returns it: `.info`, `.layer(k)`, `.shade(lights=None)`,
    `.update(light_indices, lights=None)`, `.close()`.  Close it before its MythTracer."""

    def __init__(self, mt, handle, counters, kernel_ms, total_ms):
        self.mt, self.h = mt, handle
        self.counters, self.kernel_ms, self.total_ms = counters, kernel_ms, total_ms

    def _tree(self):
        if not self.h:
            raise RuntimeError("the RayTree is closed")
        return self.mt.L.mth_raytree_handle(self.h)

    @property
    def info(self) -> dict:
        return hip_abi().raytree_info(self._tree())

    def layer(self, k, planes=None) -> dict:
        return hip_abi().raytree_read_layer(self._tree(), k, planes)

    def attr_info(self) -> dict:
        """mt_raytree_attr_info_last: renormaled, reuvwed, respawned of the tree's last update_materials / regrow."""
        return hip_abi().raytree_attr_info(self._tree())

    def shade(self, lights=None) -> dict:
        """MythTracer::ShadeRayTree.  `lights` (n x 12) replaces the facade's lights first, as set_lights does; None
        keeps them.  Returns dict(rgb, kernel_ms, total_ms)."""
        self._tree()
        if lights is not None:
            self.mt.set_lights(lights)
        _, _, cw, ch = self.info["chunk"]
        rgb = np.zeros((ch, cw, 3), dtype=np.uint8)
        ms = np.zeros(2)
        if not self.mt.L.mth_raytree_shade(self.mt.h, self.h, _ptr(rgb), rgb.size, _ptr(ms)):
            raise RuntimeError("ShadeRayTree failed: " + self.mt.last_error())
        return dict(rgb=rgb, kernel_ms=float(ms[0]), total_ms=float(ms[1]))

    def shade_colors(self, lights=None) -> dict:
        """MythTracer::ShadeRayTree(tree, &colours): the colours before V3DtoRGB.  `lights` as in shade.  Returns
        dict(color (chunk_h, chunk_w, 3) float64, kernel_ms, total_ms)."""
        self._tree()
        if lights is not None:
            self.mt.set_lights(lights)
        _, _, cw, ch = self.info["chunk"]
        color = np.zeros((ch, cw, 3), dtype=np.float64)
        ms = np.zeros(2)
        if not self.mt.L.mth_raytree_shade_colors(self.mt.h, self.h, _ptr(color), cw * ch, _ptr(ms)):
            raise RuntimeError("ShadeRayTree failed: " + self.mt.last_error())
        return dict(color=color, kernel_ms=float(ms[0]), total_ms=float(ms[1]))

    def update(self, light_indices, lights=None) -> dict:
        """MythTracer::UpdateRayTree: the planes of the lights in `light_indices`, in every layer, traced again under
        the facade's lights (the moved ones among them).  `lights` (n x 12) replaces the facade's lights first, as in
        shade; None keeps them.  Returns dict(counters, kernel_ms, total_ms)."""
        self._tree()
        if lights is not None:
            self.mt.set_lights(lights)
        idx = _i32(light_indices).reshape(-1)
        st = np.zeros(8, dtype=np.uint64)
        ms = np.zeros(2)
        if not self.mt.L.mth_raytree_update(self.mt.h, self.h, _ptr(idx), len(idx), _ptr(st), _ptr(ms)):
            raise RuntimeError("UpdateRayTree failed: " + self.mt.last_error())
        return dict(counters=dict(zip(STAT_NAMES, (int(x) for x in st))), kernel_ms=float(ms[0]), total_ms=float(ms[1]))

    def update_materials(self) -> dict:
        """MythTracer::UpdateRayTreeMaterials after MythTracer.update_materials: the tree brought to the edited
        materials without a primary or secondary ray, or a RuntimeError with the tree as it was (the edit changes its
        shape, or a textured material's ambient).  Returns dict(counters, kernel_ms, total_ms)."""
        self._tree()
        st = np.zeros(8, dtype=np.uint64)
        ms = np.zeros(2)
        if not self.mt.L.mth_raytree_update_materials(self.mt.h, self.h, _ptr(st), _ptr(ms)):
            raise RuntimeError("UpdateRayTreeMaterials failed: " + self.mt.last_error())
        return dict(counters=dict(zip(STAT_NAMES, (int(x) for x in st))), kernel_ms=float(ms[0]), total_ms=float(ms[1]))

    def regrow(self) -> dict:
        """MythTracer::RegrowRayTree after MythTracer.update_materials: like update_materials, but an edit that changes
        the tree's shape is followed -- surviving rays kept, dead subtrees dropped, new rays traced -- instead of
        refused; `.info` follows.  Returns dict(counters, kernel_ms, total_ms); counters["rays_secondary"] is the
        number of rays traced."""
        self._tree()
        st = np.zeros(8, dtype=np.uint64)
        ms = np.zeros(2)
        if not self.mt.L.mth_raytree_regrow(self.mt.h, self.h, _ptr(st), _ptr(ms)):
            raise RuntimeError("RegrowRayTree failed: " + self.mt.last_error())
        return dict(counters=dict(zip(STAT_NAMES, (int(x) for x in st))), kernel_ms=float(ms[0]), total_ms=float(ms[1]))

    def close(self):
        if getattr(self, "h", None):
            self.mt.L.mth_raytree_free(self.h)
            self.h = None

    def __del__(self):
        if getattr(self, "h", None) and getattr(self.mt, "h", None):  # (after its MythTracer the tree is gone already)
            self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class MythTracer:
    """raytracer::MythTracer (host facade) through the ctypes shim."""

    def __init__(self, obj_path=None, device=0, quiet=True):
        self.L = host_lib()
        self.h = self.L.mth_new(device, 1 if quiet else 0)
        if obj_path is not None and not self.load_obj(obj_path):
            raise RuntimeError("LoadObj failed for %s" % obj_path)

    def close(self):
        if getattr(self, "h", None):
            for ref in getattr(self, "_trees", []):  # a RayTree goes before the scene it lives on
                t = ref()
                if t is not None:
                    t.close()
            self._trees = []
            self.L.mth_free(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def last_error(self):
        return self.L.mth_last_error(self.h).decode(errors="replace")

    def set_devices(self, devices):
        """MythTracer::SetDevices: the W x H overload of RayTrace renders on all of them."""
        d = _i32(devices)
        self.L.mth_set_devices(self.h, _ptr(d), len(d))

    def load_obj(self, path) -> bool:
        return bool(self.L.mth_load_obj(self.h, os.fsencode(path)))

    def add_material(self, name, ka, kd, ks, ns=0.0, refl=0.0, tr=0.0, tf=(0, 0, 0), ni=0.0):
        # every converted array is bound to a name so that it outlives the call
        # (a temporary's buffer is recycled by numpy before the C side reads it)
        ka, kd, ks, tf = _f64(ka).reshape(3), _f64(kd).reshape(3), _f64(ks).reshape(3), _f64(tf).reshape(3)
        return self.L.mth_add_material(self.h, name.encode(), _ptr(ka), _ptr(kd), _ptr(ks),
                                       float(ns), float(refl), float(tr), _ptr(tf), float(ni))

    def add_texture(self, name, rgb):
        rgb = _f64(rgb)
        h, w, _ = rgb.shape
        return self.L.mth_add_texture(self.h, name.encode(), w, h, _ptr(rgb))

    def set_material_texture(self, mtl, tex):
        assert self.L.mth_material_set_texture(self.h, mtl, tex)

    def add_triangle(self, v, n=None, uvw=None, mtl=-1, line_no=0):
        v = _f64(v).reshape(9)
        n = None if n is None else _f64(n).reshape(9)
        uvw = None if uvw is None else _f64(uvw).reshape(9)
        return self.L.mth_add_triangle(self.h, _ptr(v), _ptr(n), _ptr(uvw), mtl, line_no)

    def set_lights(self, lights):
        l = _f64(lights).reshape(-1, 12)
        self.L.mth_set_lights(self.h, _ptr(l), l.shape[0])

    def set_max_level(self, level):
        self.L.mth_set_max_level(self.h, level)

    def set_supersampling(self, s):
        """MythTracer::SetSupersampling: s x s samples per pixel in render / render_image (1 .. 4, default 1)."""
        self.L.mth_set_supersampling(self.h, int(s))

    def set_adaptive_supersampling(self, s, threshold):
        """MythTracer::SetAdaptiveSupersampling: s x s samples only in the 8 x 8 blocks whose neighbouring pixels differ
        by more than `threshold`; s <= 1 switches it off.  Wins over set_supersampling."""
        self.L.mth_set_adaptive_supersampling(self.h, int(s), int(threshold))

    def finalize(self):
        self.L.mth_finalize(self.h)

    def prepare(self):
        if not self.L.mth_prepare(self.h):
            raise RuntimeError("MythTracer::Prepare failed: " + self.last_error())

    def device_scene(self):
        self.prepare()
        return self.L.mth_device_scene(self.h)

    def root_aabb(self):
        o = np.zeros(6)
        self.L.mth_root_aabb(self.h, _ptr(o))
        return o

    def tree(self):
        self.finalize()
        nn, nt, dd = C.c_int(), C.c_int(), C.c_int()
        self.L.mth_tree_info(self.h, C.addressof(nn), C.addressof(nt), C.addressof(dd))
        n = nn.value
        t = dict(depth=dd.value, aabb=np.zeros((n, 6)), center=np.zeros((n, 3)),
                 first_child=np.zeros(n, dtype=np.int32), prim_begin=np.zeros(n, dtype=np.int32),
                 prim_count=np.zeros(n, dtype=np.int32),
                 prim_ids=np.zeros(max(nt.value, 1), dtype=np.int32))
        if not self.L.mth_tree_dump(self.h, _ptr(t["aabb"]), _ptr(t["center"]), _ptr(t["first_child"]),
                                    _ptr(t["prim_begin"]), _ptr(t["prim_count"]), _ptr(t["prim_ids"])):
            raise RuntimeError("tree failed: " + self.last_error())
        t["prim_ids"] = t["prim_ids"][:nt.value]
        return t

    def triangles(self):
        nn, nt, dd = C.c_int(), C.c_int(), C.c_int()
        self.L.mth_tree_info(self.h, C.addressof(nn), C.addressof(nt), C.addressof(dd))
        n = nt.value
        data = np.zeros((max(n, 1), 33))
        line = np.zeros(max(n, 1), dtype=np.int32)
        has = np.zeros(max(n, 1), dtype=np.int32)
        self.L.mth_triangles(self.h, _ptr(data), _ptr(line), _ptr(has))
        return data[:n], line[:n], has[:n]

    def flatten(self) -> dict:
        """The flattened scene exactly as MythTracer::Prepare passes it to
        mt_scene_create (input of HipAbi.scene_create)."""
        t = self.tree()
        nt, nm, nx = C.c_int(), C.c_int(), C.c_int()
        a = [C.addressof(nt), C.addressof(nm), C.addressof(nx)]
        if not self.L.mth_flatten(self.h, *a, *([None] * 8)):
            raise RuntimeError("flatten failed: " + self.last_error())
        n, m, x = nt.value, nm.value, nx.value
        vertex, normal, uvw = (np.zeros((max(n, 1), 9)) for _ in range(3))
        aabb = np.zeros((max(n, 1), 6))
        material = np.zeros(max(n, 1), dtype=np.int32)
        line_no = np.zeros(max(n, 1), dtype=np.int32)
        mats = np.zeros((max(m, 1), 17))
        whf = np.zeros((max(x, 1), 3), dtype=np.int32)
        assert self.L.mth_flatten(self.h, *a, _ptr(vertex), _ptr(normal), _ptr(uvw), _ptr(aabb),
                                  _ptr(material), _ptr(line_no), _ptr(mats), _ptr(whf))
        textures = []
        for i in range(x):
            w, h, fmt = (int(v) for v in whf[i])
            tex = np.zeros((h, w, 3), dtype=np.uint8 if fmt == MT_TEX_RGB8 else np.float64)
            assert self.L.mth_flatten_texels(self.h, i, _ptr(tex))
            textures.append(dict(texels=tex))
        return dict(tree_depth=t["depth"], node_aabb=t["aabb"], node_center=t["center"],
                    node_first_child=t["first_child"], node_prim_begin=t["prim_begin"],
                    node_prim_count=t["prim_count"], tri_id=t["prim_ids"],
                    tri_vertex=vertex[:n], tri_normal=normal[:n], tri_uvw=uvw[:n],
                    tri_aabb=aabb[:n], tri_material=material[:n], tri_line_no=line_no[:n],
                    materials=[dict(values=mats[i, :16], tex=int(mats[i, 16])) for i in range(m)],
                    textures=textures)

    def get_material(self, name):
        d = np.zeros(16)
        has_tex = C.c_int()
        if not self.L.mth_get_material(self.h, name.encode(), _ptr(d), C.addressof(has_tex)):
            return None
        return d, bool(has_tex.value)

    MATERIAL_FIELDS = dict(ka=(0, 3), kd=(3, 3), ks=(6, 3), ns=(9, 1), refl=(10, 1), tr=(11, 1), tf=(12, 3), ni=(15, 1))

    def update_materials(self, edits=None):
        """MythTracer::UpdateMaterials after an edit by material name and field: `edits` = {name: {field: value}} with
        the fields ka kd ks (3 numbers each) ns refl tr (one) tf (3) ni (one) -- add_material's names; the other fields
        keep their values.  None or {} only pushes the scene's current materials.  The constants are replaced on every
        device replica without uploading the geometry again; RayTrees made before are stale until their
        update_materials().  RuntimeError for an unknown name or field."""
        edits = edits or {}
        staged = []
        for name, fields in edits.items():
            got = self.get_material(name)
            if got is None:
                raise RuntimeError("UpdateMaterials failed: no material named %s" % name)
            v = got[0].copy()
            for field, value in fields.items():
                if field not in self.MATERIAL_FIELDS:
                    raise RuntimeError("UpdateMaterials failed: no material field %r (fields: %s)"
                                       % (field, " ".join(self.MATERIAL_FIELDS)))
                at, k = self.MATERIAL_FIELDS[field]
                v[at:at + k] = _f64(value).reshape(k)
            staged.append((name, v))
        for name, v in staged or [(None, None)]:
            if not self.L.mth_update_materials(self.h, name.encode() if name is not None else None, _ptr(v)):
                raise RuntimeError("UpdateMaterials failed: " + self.last_error())

    def update_texture(self, name, rgb=None):
        """MythTracer::UpdateTexture: the texture with the scene's key `name` (add_texture's name, or the file name an
        .mtl gave) replaced on every device replica by `rgb`, (height, width, 3) doubles -- size free to change --, or
        by the scene's entry as it is when `rgb` is None.  RayTrees made before are stale until their
        update_materials(), which takes the edit only for a tree built after set_raytree_keep_uvw(True)."""
        a = None
        w = hgt = 0
        if rgb is not None:
            a = _f64(rgb)
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("rgb must be (height, width, 3)")
            hgt, w = a.shape[0], a.shape[1]
        if not self.L.mth_update_texture(self.h, name.encode(), w, hgt, _ptr(a)):
            raise RuntimeError("UpdateTexture failed: " + self.last_error())

    def set_raytree_keep_uvw(self, keep: bool):
        """MythTracer::SetRayTreeKeepUVW: RayTrees built from now on keep each ray's texture coordinates."""
        self.L.mth_set_raytree_keep_uvw(self.h, 1 if keep else 0)

    def assign_material(self, add_indices, name):
        """Triangle::mtl of the triangles `add_indices` (add_triangle / .obj order) pointed at the scene's material
        `name`, or at none for None.  Only the host scene changes: update_triangle_materials() pushes it.  RuntimeError
        for an unknown name or an index outside the scene's triangles; no triangle is changed then."""
        a = np.ascontiguousarray(add_indices, dtype=np.int32).reshape(-1)
        if not self.L.mth_assign_material(self.h, a.ctypes.data if a.size else None, int(a.size),
                                          name.encode() if name is not None else None):
            raise RuntimeError("assign_material failed: " + self.last_error())

    def update_triangle_materials(self):
        """MythTracer::UpdateTriangleMaterials: the triangles' current materials, as indices into the uploaded dense
        table, replaced on every device replica without uploading the geometry again.  RuntimeError when a triangle
        points at a material that was not uploaded.  RayTrees made before are stale until their update_materials() or
        regrow(), which take the edit only for a tree built after set_raytree_keep_triangles(True)."""
        if not self.L.mth_update_triangle_materials(self.h):
            raise RuntimeError("UpdateTriangleMaterials failed: " + self.last_error())

    def _set_triangle_attr(self, which, add_indices, attr):
        a = np.ascontiguousarray(add_indices, dtype=np.int32).reshape(-1)
        v = np.ascontiguousarray(attr, dtype=np.float64)
        if v.size != a.size * 9:
            raise ValueError("%d triangles need %d doubles, not %d" % (a.size, a.size * 9, v.size))
        if not self.L.mth_set_triangle_attr(self.h, which, a.ctypes.data if a.size else None, int(a.size),
                                            v.ctypes.data if v.size else None):
            raise RuntimeError("set_triangle_%s failed: %s" % (("normals", "uvw")[which], self.last_error()))

    def set_triangle_normals(self, add_indices, normals):
        """Triangle::normal of the triangles `add_indices` (add_triangle / .obj order) replaced by `normals`
        (n x 3 x 3).  Only the host scene changes: update_triangle_attributes() pushes it.  RuntimeError for an index
        outside the scene's triangles; no triangle is changed then."""
        self._set_triangle_attr(0, add_indices, normals)

    def set_triangle_uvw(self, add_indices, uvw):
        """The same for Triangle::uvw, `uvw` (n x 3 x 3)."""
        self._set_triangle_attr(1, add_indices, uvw)

    def update_triangle_attributes(self):
        """MythTracer::UpdateTriangleAttributes: the triangles' current normals and texture coordinates replaced on
        every device replica.  RayTrees built before are stale until update_materials() / regrow(), which need a tree
        that keeps triangles."""
        if not self.L.mth_update_triangle_attributes(self.h):
            raise RuntimeError("UpdateTriangleAttributes failed: " + self.last_error())

    def set_device_tree_build(self, on: bool):
        """MythTracer::SetDeviceTreeBuild: the next finalize / prepare builds the octree on the GPU (mt_octree_build),
        bit for bit the host builder's tree.  Off by default; with it on, no GPU or a failed build is an error, never
        the host builder instead."""
        self.L.mth_set_device_tree_build(self.h, 1 if on else 0)

    def set_triangle_vertices(self, add_indices, vertices):
        """MythTracer::SetTriangleVertices: the vertices of the triangles `add_indices` (add_triangle / .obj order)
        replaced by `vertices` (n x 3 x 3) and their boxes cached again.  Only the host scene changes:
        update_geometry() must follow.  RuntimeError for an index outside the scene's triangles; no triangle is
        changed then."""
        a = np.ascontiguousarray(add_indices, dtype=np.int32).reshape(-1)
        v = np.ascontiguousarray(vertices, dtype=np.float64)
        if v.size != a.size * 9:
            raise ValueError("%d triangles need %d doubles, not %d" % (a.size, a.size * 9, v.size))
        if not self.L.mth_set_triangle_vertices(self.h, a.ctypes.data if a.size else None, int(a.size),
                                                v.ctypes.data if v.size else None):
            raise RuntimeError("set_triangle_vertices failed: " + self.last_error())

    def update_geometry(self):
        """MythTracer::UpdateGeometry: the root box again over all triangles, the tree unfinalized and the device
        scenes dropped; the next prepare / render builds and uploads again, with either builder.  The RayTrees of this
        object live on the dropped scene: they are closed first (a closed RayTree raises on use, it never reports
        itself fresh)."""
        for ref in getattr(self, "_trees", []):
            t = ref()
            if t is not None:
                t.close()
        self._trees = []
        self.L.mth_update_geometry(self.h)

    def update_geometry_in_place(self):
        """MythTracer::UpdateGeometryInPlace: after set_triangle_vertices, the uploaded scenes take the moved triangles
        in place (mt_scene_set_triangle_vertices): the tree is built again on the GPU, the device arrays are
        re-ordered, and materials, textures, lights, tuning and cost history stay.  update_triangle_materials,
        update_triangle_attributes and flatten() speak the new order afterwards.  With nothing uploaded yet it is
        update_geometry() and prepare().  The RayTrees of this object belong to the old geometry: they are closed
        first.  RuntimeError with the library's message when a device refuses; its scene is then as it was."""
        for ref in getattr(self, "_trees", []):
            t = ref()
            if t is not None:
                t.close()
        self._trees = []
        if not self.L.mth_update_geometry_in_place(self.h):
            raise RuntimeError("update_geometry_in_place failed: " + self.last_error())

    def add_triangles(self, vertices, normals=None, uvw=None, material=None, line_no=None):
        """MythTracer::AddTriangle for every triangle of `vertices` ((n, 3, 3) or (n, 9)), with `normals` and `uvw` of the
        same shape (None: the Triangle's defaults), all of the scene's material `material` (a name; None: no material)
        and the line numbers `line_no` (one int for all, n ints, or None for 0).  The triangles get the last add
        indices.  Only the host scene changes: update_triangles_in_place() pushes the batch.  RuntimeError for an
        unknown material; no triangle is added then."""
        v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 9)
        n = v.shape[0]
        nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 9)
        tex = None if uvw is None else np.ascontiguousarray(uvw, dtype=np.float64).reshape(-1, 9)
        for a in (nrm, tex):
            if a is not None and a.shape[0] != n:
                raise ValueError("%d triangles need %d doubles, not %d" % (n, n * 9, a.size))
        line = None if line_no is None else np.ascontiguousarray(np.broadcast_to(np.asarray(line_no, dtype=np.int32), (n,)))
        if not self.L.mth_add_triangles(self.h, n, _ptr(v) if n else None, _ptr(nrm), _ptr(tex),
                                        material.encode() if material is not None else None, _ptr(line)):
            raise RuntimeError("add_triangles failed: " + self.last_error())

    def remove_triangles(self, add_indices):
        """MythTracer::RemoveTriangles: the triangles `add_indices` (add_triangle / .obj order, each at most once) deleted
        from the host scene; the survivors keep their order and are numbered densely.  At most once, and before any
        add_triangles, since the last upload or update: the indices are the uploaded scene's.  RuntimeError with the
        facade's message otherwise, or for a bad index; nothing is removed then."""
        a = np.ascontiguousarray(add_indices, dtype=np.int32).reshape(-1)
        if not self.L.mth_remove_triangles(self.h, a.ctypes.data if a.size else None, int(a.size)):
            raise RuntimeError("remove_triangles failed: " + self.last_error())

    def update_triangles_in_place(self):
        """MythTracer::UpdateTrianglesInPlace: after remove_triangles / add_triangles, the uploaded scenes take the batch
        in place (mt_scene_edit_triangles): the tree is built again on the GPU with the new count, the device arrays are
        re-ordered, and materials, textures, lights, tuning and cost history stay.  update_triangle_materials,
        update_triangle_attributes, set_triangle_vertices and flatten() speak the new count and order afterwards.  With
        nothing uploaded yet it is update_geometry() and prepare().  The RayTrees of this object belong to the old
        geometry: they are closed first.  RuntimeError with the message when the facade or a device refuses; after a
        device's refusal every device scene is dropped and the next prepare uploads the host's state anew."""
        for ref in getattr(self, "_trees", []):
            t = ref()
            if t is not None:
                t.close()
        self._trees = []
        if not self.L.mth_update_triangles_in_place(self.h):
            raise RuntimeError("update_triangles_in_place failed: " + self.last_error())

    def set_raytree_keep_triangles(self, keep: bool):
        """MythTracer::SetRayTreeKeepTriangles: RayTrees built from now on keep the triangle each ray hit."""
        self.L.mth_set_raytree_keep_triangles(self.h, 1 if keep else 0)

    @property
    def num_materials(self):
        return self.L.mth_num_materials(self.h)

    def render(self, cam, image_w, image_h, chunk=None, debug=False):
        """MythTracer::RayTrace(WorkChunk*)."""
        cx, cy, cw, ch = chunk if chunk else (0, 0, image_w, image_h)
        rgb = np.zeros((max(ch, 0), max(cw, 0), 3), dtype=np.uint8)
        dl = np.zeros((max(ch, 0), max(cw, 0)), dtype=np.int32) if debug else None
        dp = np.zeros((max(ch, 0), max(cw, 0), 3)) if debug else None
        st = np.zeros(8, dtype=np.uint64)
        ms = np.zeros(2)
        cam = _f64(cam)
        ok = self.L.mth_render_chunk(self.h, _ptr(cam), image_w, image_h, cx, cy, cw, ch,
                                     _ptr(rgb), _ptr(dl), _ptr(dp), _ptr(st), _ptr(ms))
        if not ok:
            raise RuntimeError("RayTrace failed: " + self.last_error())
        return dict(rgb=rgb, line=dl, point=dp,
                    counters=dict(zip(STAT_NAMES, (int(x) for x in st))),
                    kernel_ms=float(ms[0]), total_ms=float(ms[1]))

    def gbuffer(self, cam, image_w, image_h, chunk=None, channels=None):
        """MythTracer::RayTraceGBuffer: dict plane name -> numpy array of the chunk for the planes named in `channels`
        (None = all of GBUFFER_PLANES), plus counters, kernel_ms, total_ms."""
        cx, cy, cw, ch = chunk if chunk else (0, 0, image_w, image_h)
        out = _gbuffer_arrays(channels, cw, ch)
        names = list(GBUFFER_PLANES)
        bits = sum(1 << names.index(n) for n in out)
        planes = (C.c_void_p * 8)(*[out[n].ctypes.data if n in out else None for n in names])
        st = np.zeros(8, dtype=np.uint64)
        ms = np.zeros(2)
        cam = _f64(cam)
        if not self.L.mth_render_gbuffer(self.h, _ptr(cam), image_w, image_h, cx, cy, cw, ch, bits, planes,
                                         _ptr(st), _ptr(ms)):
            raise RuntimeError("RayTraceGBuffer failed: " + self.last_error())
        out.update(counters=dict(zip(STAT_NAMES, (int(x) for x in st))), kernel_ms=float(ms[0]), total_ms=float(ms[1]))
        return out

    def lightbuffer(self, cam, image_w, image_h, chunk=None, channels=None, gbuffer_channels=None):
        """MythTracer::RayTraceLightBuffer under the lights of set_lights: dict with the light-buffer planes named in
        `channels` (None = both: `power` (n_lights, ch, cw, 3) float64, `in_shadow` (n_lights, ch, cw) uint8), the
        G-buffer planes named in `gbuffer_channels` from the same launch (None = the four a relight reads; () = none),
        plus counters, kernel_ms, total_ms."""
        cx, cy, cw, ch = chunk if chunk else (0, 0, image_w, image_h)
        n_l = self.L.mth_num_lights(self.h)
        out = _lightbuffer_arrays(channels, n_l, cw, ch)
        planes = _gbuffer_arrays(RELIGHT_GBUFFER_PLANES if gbuffer_channels is None else gbuffer_channels, cw, ch)
        names = list(GBUFFER_PLANES)
        gbits = sum(1 << names.index(n) for n in planes)
        gptrs = (C.c_void_p * 8)(*[planes[n].ctypes.data if n in planes else None for n in names])
        lnames = list(LIGHTBUFFER_PLANES)
        lbits = sum(1 << lnames.index(n) for n in out)
        lptrs = (C.c_void_p * 2)(*[out[n].ctypes.data if n in out else None for n in lnames])
        st = np.zeros(8, dtype=np.uint64)
        ms = np.zeros(2)
        cam = _f64(cam)
        if not self.L.mth_render_lightbuffer(self.h, _ptr(cam), image_w, image_h, cx, cy, cw, ch, gbits, gptrs, lbits,
                                             lptrs, n_l, _ptr(st), _ptr(ms)):
            raise RuntimeError("RayTraceLightBuffer failed: " + self.last_error())
        out.update(planes)
        out.update(counters=dict(zip(STAT_NAMES, (int(x) for x in st))), kernel_ms=float(ms[0]), total_ms=float(ms[1]))
        return out

    def relight(self, cam, image_w, image_h, gbuffer, lightbuffer, lights=None, chunk=None):
        """MythTracer::ShadeDirect: the frame of the direct term (what render gives at max level 0) from stored planes,
        without tracing a ray.  `lights` (n x 12) replaces the facade's lights first, as set_lights does; None keeps
        them.  They may differ from the lights the light buffer was made with in their colours only: after a light has
        moved, update_lightbuffer first.  Returns dict(rgb, kernel_ms, total_ms)."""
        cx, cy, cw, ch = chunk if chunk else (0, 0, image_w, image_h)
        if lights is not None:
            self.set_lights(lights)
        gp, lp, n_l = _relight_planes(gbuffer, lightbuffer, cw, ch)
        gptrs = (C.c_void_p * 4)(*[gp[n].ctypes.data for n in RELIGHT_GBUFFER_PLANES])
        lptrs = (C.c_void_p * 2)(lp["power"].ctypes.data, lp["in_shadow"].ctypes.data)
        rgb = np.zeros((ch, cw, 3), dtype=np.uint8)
        ms = np.zeros(2)
        cam = _f64(cam)
        if not self.L.mth_shade_direct(self.h, _ptr(cam), image_w, image_h, cx, cy, cw, ch, gptrs, n_l, lptrs,
                                       _ptr(rgb), _ptr(ms)):
            raise RuntimeError("ShadeDirect failed: " + self.last_error())
        return dict(rgb=rgb, kernel_ms=float(ms[0]), total_ms=float(ms[1]))

    def update_lightbuffer(self, gbuffer, lightbuffer, light_indices):
        """MythTracer::UpdateLightBuffer under the lights of set_lights (the moved ones among them): the planes of the
        lights in `light_indices` of `lightbuffer` traced again from the `point` and `material` planes of `gbuffer`
        (dicts as lightbuffer() returns them).  Returns a NEW dict with the updated light-buffer planes (the planes of
        the other lights copied as they were) plus counters, kernel_ms, total_ms; the arguments are not changed."""
        g, lb, n_l, cw, ch = _update_planes(gbuffer, {n: np.array(a) for n, a in lightbuffer.items()
                                                      if n in LIGHTBUFFER_PLANES})
        idx = _i32(light_indices).reshape(-1)
        gptrs = (C.c_void_p * 2)(*[g[n].ctypes.data for n in UPDATE_GBUFFER_PLANES])
        lnames = list(LIGHTBUFFER_PLANES)
        lbits = sum(1 << lnames.index(n) for n in lb)
        lptrs = (C.c_void_p * 2)(*[lb[n].ctypes.data if n in lb else None for n in lnames])
        st = np.zeros(8, dtype=np.uint64)
        ms = np.zeros(2)
        if not self.L.mth_update_lightbuffer(self.h, cw, ch, gptrs, _ptr(idx), len(idx), lbits, lptrs, n_l,
                                             _ptr(st), _ptr(ms)):
            raise RuntimeError("UpdateLightBuffer failed: " + self.last_error())
        out = dict(lb)
        out.update(counters=dict(zip(STAT_NAMES, (int(x) for x in st))), kernel_ms=float(ms[0]), total_ms=float(ms[1]))
        return out

    def raytree(self, cam, image_w, image_h, chunk=None, max_depth=None) -> RayTree:
        """MythTracer::BuildRayTree under the lights of set_lights: the whole call tree of the chunk's pixels, kept on
        the GPU.  max_depth (None = the facade's level) goes through set_max_level first.  The object's .counters are
        those of render() for the same frame."""
        cx, cy, cw, ch = chunk if chunk else (0, 0, image_w, image_h)
        if max_depth is not None:
            self.set_max_level(int(max_depth))
        st = np.zeros(8, dtype=np.uint64)
        ms = np.zeros(2)
        cam = _f64(cam)
        t = self.L.mth_raytree_build(self.h, _ptr(cam), image_w, image_h, cx, cy, cw, ch, _ptr(st), _ptr(ms))
        if not t:
            raise RuntimeError("BuildRayTree failed: " + self.last_error())
        tree = RayTree(self, t, dict(zip(STAT_NAMES, (int(x) for x in st))), float(ms[0]), float(ms[1]))
        self._trees = [r for r in getattr(self, "_trees", []) if r() is not None] + [weakref.ref(tree)]
        return tree

    def raytree_rays(self, rays, list_width=0, max_depth=None) -> RayTree:
        """MythTracer::BuildRayTree(rays, list_width, &tree) under the lights of set_lights: `rays` (n, 6) in the
        caller's order, list_width 0 = an n x 1 list.  Close the RayTree before this MythTracer."""
        if max_depth is not None:
            self.set_max_level(int(max_depth))
        r = _f64(rays).reshape(-1, 6)
        st = np.zeros(8, dtype=np.uint64)
        ms = np.zeros(2)
        t = self.L.mth_raytree_build_rays(self.h, _ptr(r), r.shape[0], int(list_width), _ptr(st), _ptr(ms))
        if not t:
            raise RuntimeError("BuildRayTree failed: " + self.last_error())
        tree = RayTree(self, t, dict(zip(STAT_NAMES, (int(x) for x in st))), float(ms[0]), float(ms[1]))
        self._trees = [r for r in getattr(self, "_trees", []) if r() is not None] + [weakref.ref(tree)]
        return tree

    def trace_rays(self, rays, list_width=0, max_depth=None, color=True, rgb=True) -> dict:
        """MythTracer::TraceRays: dict(color (n, 3) float64 and / or rgb (n, 3) uint8 -- whichever was asked for --,
        counters, kernel_ms, total_ms), in the caller's order."""
        if max_depth is not None:
            self.set_max_level(int(max_depth))
        r = _f64(rays).reshape(-1, 6)
        n = r.shape[0]
        out = {}
        if color:
            out["color"] = np.zeros((n, 3), dtype=np.float64)
        if rgb:
            out["rgb"] = np.zeros((n, 3), dtype=np.uint8)
        st = np.zeros(8, dtype=np.uint64)
        ms = np.zeros(2)
        if not self.L.mth_trace_rays(self.h, _ptr(r), n, int(list_width), _ptr(out.get("color")), _ptr(out.get("rgb")),
                                     _ptr(st), _ptr(ms)):
            raise RuntimeError("TraceRays failed: " + self.last_error())
        out.update(counters=dict(zip(STAT_NAMES, (int(x) for x in st))), kernel_ms=float(ms[0]), total_ms=float(ms[1]))
        return out

    def render_image(self, cam, image_w, image_h):
        """MythTracer::RayTrace(int, int, Camera*, vector<uint8_t>*)."""
        rgb = np.zeros((image_h, image_w, 3), dtype=np.uint8)
        cam = _f64(cam)
        if not self.L.mth_render_image(self.h, _ptr(cam), image_w, image_h, _ptr(rgb)):
            raise RuntimeError("RayTrace failed: " + self.last_error())
        return rgb

    def frame_loop(self, cam, image_w, image_h, n_frames, dyaw=2.0, collect_stats=False):
        """The frame loop of main_local.cc:51-132 through the facade (host_capi.cc mth_frame_loop): lights pushed again
        every frame, a Camera per frame, RayTrace(W, H, &cam, &bitmap) into ONE vector.  Returns (wall ms per frame,
        the last frame)."""
        rgb = np.zeros((image_h, image_w, 3), dtype=np.uint8)
        ms = np.zeros(n_frames, dtype=np.float64)
        cam = _f64(cam)
        if not self.L.mth_frame_loop(self.h, _ptr(cam), image_w, image_h, n_frames, float(dyaw),
                                     1 if collect_stats else 0, _ptr(ms), _ptr(rgb)):
            raise RuntimeError("RayTrace failed: " + self.last_error())
        return ms, rgb

    def intersect(self, rays):
        rays = _f64(rays).reshape(-1, 6)
        n = rays.shape[0]
        out = dict(tri=np.zeros(n, dtype=np.int32), line=np.zeros(n, dtype=np.int32),
                   t=np.full(n, np.nan), point=np.full((n, 3), np.nan))
        if not self.L.mth_intersect(self.h, n, _ptr(rays), _ptr(out["tri"]), _ptr(out["line"]),
                                    _ptr(out["t"]), _ptr(out["point"])):
            raise RuntimeError("IntersectRays failed: " + self.last_error())
        return out
