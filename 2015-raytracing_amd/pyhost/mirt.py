"""ctypes binding of include/mirt.h -- tooling for tests/, bench.py and smoke().

The product host is JavaScript (2015-raytracing_amd/host/, over the N-API addon); this
module exists because the driver's bench/test contract is Python.  It adds nothing to
the C ABI: every method is one mirt_* call, errors become MirtError carrying
mirt_last_error().  There is NO CPU fallback here or below: without libmirt.so or without
a gfx950 device every entry point raises.
"""
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MIRT_CONTRACT=default: the library built for the reference's own build options (AMD's default 2.5-ulp division and 3-ulp sqrt: csrc/build.sh,
# DESIGN.md section 2) instead of the correctly rounded contract; MIRT_LIB_PATH: an A/B build
LIB_PATH = os.environ.get("MIRT_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "libmirt_default.so" if os.environ.get("MIRT_CONTRACT") == "default" else "libmirt.so")

MEM_READ_WRITE, MEM_WRITE_ONLY, MEM_READ_ONLY = 1, 2, 4
MAX_LIGHTS, MAX_MESHES = 8, 16


class MirtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mirt error {code}: {msg}")
        self.code = code


class _Grid(C.Structure):
    _fields_ = [("prims", C.c_void_p), ("normals", C.c_void_p), ("matid", C.c_void_p), ("cell_offsets", C.c_void_p),
                ("bounds", C.c_float * 8), ("n_slabs", C.c_uint32), ("mesh_matid", C.c_uint32)]


class _GridBuildDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_uint32), ("count", C.c_uint32), ("n_slabs", C.c_uint32),
                ("bounds", C.c_double * 6), ("prims_f64", C.c_void_p)]


class _MeshIngestDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_vertices", C.c_uint32), ("n_corners", C.c_uint32), ("first_corner", C.c_uint32),
                ("model", C.c_float * 16), ("normal_mat", C.c_float * 9), ("positions_f64", C.c_void_p), ("normals_f64", C.c_void_p),
                ("indices_u32", C.c_void_p)]


class _Light(C.Structure):
    _fields_ = [("shadow", C.c_float * 16), ("scene", C.c_float * 16), ("light", C.c_float * 16)]


class _PassDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("rays_per_pixel", C.c_uint32),
                ("row0", C.c_uint32), ("nrows", C.c_uint32), ("bounces", C.c_uint32), ("pass_index", C.c_uint32),
                ("cam", C.c_float * 16), ("scene_bounds", C.c_float * 8), ("focal_length", C.c_float), ("lens_rad", C.c_float),
                ("n_lights", C.c_uint32), ("n_meshes", C.c_uint32),
                ("spheres", C.POINTER(_Grid)), ("triangles", C.POINTER(_Grid)), ("meshes", C.POINTER(_Grid)),
                ("lights", C.POINTER(_Light)),
                ("material", C.c_void_p), ("seeds", C.c_void_p), ("acu", C.c_void_p), ("pixel", C.c_void_p), ("radiance", C.c_void_p)]


class _FrameDesc(C.Structure):   # mirt_frame_desc
    _fields_ = [("struct_size", C.c_uint32), ("assign", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("cam", C.c_float * 16), ("bounds", C.c_float * 8), ("t_size", C.c_uint32), ("s_size", C.c_uint32),
                ("t_pos", C.c_void_p), ("t_normal", C.c_void_p), ("t_mindex", C.c_void_p), ("t_mcolor", C.c_void_p),
                ("s_atoms", C.c_void_p), ("s_mindex", C.c_void_p), ("s_mcolor", C.c_void_p),
                ("n_slabs", C.c_uint32), ("reserved", C.c_uint32),
                ("t_slab_size", C.c_void_p), ("s_slab_size", C.c_void_p), ("pixel", C.c_void_p), ("rays", C.c_void_p)]


class _FilterDesc(C.Structure):   # mirt_filter_desc
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("iterations", C.c_uint32), ("flags", C.c_uint32),
                ("normal_power_log2", C.c_uint32), ("tone", C.c_float), ("sigma_depth", C.c_float), ("sigma_colour", C.c_float),
                ("radiance", C.c_void_p), ("normal_hits", C.c_void_p), ("albedo_depth", C.c_void_p), ("filtered", C.c_void_p), ("pixel", C.c_void_p)]


class _UpsampleDesc(C.Structure):   # mirt_upsample_desc
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("factor", C.c_uint32), ("flags", C.c_uint32),
                ("normal_power_log2", C.c_uint32), ("tone", C.c_float), ("sigma_depth", C.c_float),
                ("radiance_lo", C.c_void_p), ("normal_hits_lo", C.c_void_p), ("albedo_depth_lo", C.c_void_p),
                ("normal_hits", C.c_void_p), ("albedo_depth", C.c_void_p), ("upsampled", C.c_void_p), ("pixel", C.c_void_p)]


class _AoDesc(C.Structure):   # mirt_ao_desc
    _fields_ = [("struct_size", C.c_uint32), ("samples", C.c_uint32), ("radius", C.c_float), ("bias", C.c_float)]


class _RadianceDesc(C.Structure):   # mirt_radiance_desc
    _fields_ = [("struct_size", C.c_uint32), ("samples", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class _ViewDesc(C.Structure):   # mirt_view_desc
    _fields_ = [("struct_size", C.c_uint32), ("model", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("k", C.c_uint32),
                ("row0", C.c_uint32), ("nrows", C.c_uint32), ("flags", C.c_uint32),
                ("eye", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3), ("forward", C.c_float * 3),
                ("half_w", C.c_float), ("half_h", C.c_float), ("half_angle", C.c_float), ("t_min", C.c_float), ("t_max", C.c_float), ("tone", C.c_float)]


_lib = None

VIEW_ORTHOGRAPHIC, VIEW_EQUIRECT, VIEW_FISHEYE = 0, 1, 2   # MIRT_VIEW_* models (include/mirt.h)
VIEW_ACCUMULATE = 1   # MIRT_VIEW_ACCUMULATE
VIEW_MODELS = {"ortho": VIEW_ORTHOGRAPHIC, "orthographic": VIEW_ORTHOGRAPHIC, "equirect": VIEW_EQUIRECT, "fisheye": VIEW_FISHEYE}

RADIANCE_ACCUMULATE, RADIANCE_NO_EMITTERS, RADIANCE_MAX_SAMPLES = 1, 2, 64   # MIRT_RADIANCE_* (include/mirt.h)
AO_MAX_SAMPLES, AO_DEFAULT_SAMPLES, AO_DEFAULT_BIAS = 64, 4, 0.001   # MIRT_AO_* (include/mirt.h)

PASSES_FRESH = 1   # MIRT_PASSES_FRESH (include/mirt.h)
PASSES_EVERY_FRAME = 2   # MIRT_PASSES_EVERY_FRAME (include/mirt.h)
MAX_PASSES_PER_CALL = 64   # MIRT_MAX_PASSES_PER_CALL (include/mirt.h)

FILTER_DEMODULATE, FILTER_DIRECT, FILTER_TILED = 1, 2, 4   # MIRT_FILTER_* (include/mirt.h)
# MIRT_FILTER_DEFAULT_*: the shipped parameters of the a-trous filter (with FILTER_DEMODULATE)
FILTER_DEFAULTS = {"iterations": 3, "normal_power_log2": 5, "sigma_depth": 0.1, "sigma_colour": 1.0, "demodulate": True}

UPSAMPLE_DEMODULATE = 1   # MIRT_UPSAMPLE_DEMODULATE (include/mirt.h)
# MIRT_UPSAMPLE_DEFAULT_*: the shipped parameters of the guide-driven upsampler (with UPSAMPLE_DEMODULATE)
UPSAMPLE_DEFAULTS = {"normal_power_log2": 5, "sigma_depth": 0.1, "demodulate": True}

# name -> (restype, argtypes): every symbol include/mirt.h declares
SYMBOLS = {
    "mirt_device_count": (C.c_int, []),
    "mirt_device_name": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t]),
    "mirt_version": (C.c_char_p, []),
    "mirt_abi_version": (C.c_int, []),
    "mirt_ctx_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "mirt_ctx_destroy": (C.c_int, [C.c_void_p]),
    "mirt_last_error": (C.c_char_p, [C.c_void_p]),
    "mirt_ctx_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mirt_finish": (C.c_int, [C.c_void_p]),
    "mirt_buf_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint, C.POINTER(C.c_void_p)]),
    "mirt_buf_wrap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "mirt_buf_release": (C.c_int, [C.c_void_p]),
    "mirt_buf_size": (C.c_size_t, [C.c_void_p]),
    "mirt_buf_device_ptr": (C.c_void_p, [C.c_void_p]),
    "mirt_buf_write": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int]),
    "mirt_buf_read": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int]),
    "mirt_program_check": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t]),
    "mirt_program_dialect": (C.c_int, [C.c_char_p]),
    "mirt_kernel_get": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "mirt_kernel_release": (C.c_int, [C.c_void_p]),
    "mirt_kernel_num_args": (C.c_int, [C.c_void_p]),
    "mirt_kernel_set_arg": (C.c_int, [C.c_void_p, C.c_uint, C.c_size_t, C.c_void_p]),
    "mirt_kernel_set_arg_buf": (C.c_int, [C.c_void_p, C.c_uint, C.c_void_p]),
    "mirt_kernel_preferred_multiple": (C.c_int, [C.c_void_p]),
    "mirt_enqueue": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "mirt_render_pass": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc)]),
    "mirt_render_first_pass": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc)]),
    "mirt_render_passes": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc), C.c_uint32, C.c_uint32]),
    "mirt_render_guides": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc), C.c_void_p, C.c_void_p]),
    "mirt_render_first_pass_guided": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc), C.c_void_p, C.c_void_p]),
    "mirt_render_passes_guided": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mirt_ctx_guided_passes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "mirt_trace_closest": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "mirt_trace_occluded": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc), C.c_void_p, C.c_uint64, C.c_void_p]),
    "mirt_trace_deferred": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "mirt_trace_radiance": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc), C.POINTER(_RadianceDesc), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "mirt_radiance_deferred": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "mirt_view_rays": (C.c_int, [C.c_void_p, C.POINTER(_ViewDesc), C.c_void_p]),
    "mirt_render_view": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc), C.POINTER(_ViewDesc), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mirt_view_deferred": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "mirt_view_rays_batch": (C.c_int, [C.c_void_p, C.POINTER(_ViewDesc), C.c_void_p, C.c_uint32, C.c_void_p]),
    "mirt_render_view_batch": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc), C.POINTER(_ViewDesc), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mirt_view_guides": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc), C.POINTER(_ViewDesc), C.c_void_p, C.c_void_p]),
    "mirt_render_view_guided": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc), C.POINTER(_ViewDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mirt_ctx_guided_views": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "mirt_render_ao": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc), C.POINTER(_AoDesc), C.c_void_p]),
    "mirt_ao_deferred": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "mirt_view_ao": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc), C.POINTER(_ViewDesc), C.POINTER(_AoDesc), C.c_void_p, C.c_void_p]),
    "mirt_view_ao_deferred": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "mirt_view_guides_batch": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc), C.POINTER(_ViewDesc), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mirt_render_view_guided_batch": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc), C.POINTER(_ViewDesc), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p]),
    "mirt_view_ao_batch": (C.c_int, [C.c_void_p, C.POINTER(_PassDesc), C.POINTER(_ViewDesc), C.c_void_p, C.c_uint32, C.POINTER(_AoDesc), C.c_void_p, C.c_void_p]),
    "mirt_filter_atrous": (C.c_int, [C.c_void_p, C.POINTER(_FilterDesc)]),
    "mirt_upsample_guided": (C.c_int, [C.c_void_p, C.POINTER(_UpsampleDesc)]),
    "mirt_pass_deferred": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "mirt_ctx_set_exact_only": (C.c_int, [C.c_void_p, C.c_int]),
    "mirt_ctx_set_fusion": (C.c_int, [C.c_void_p, C.c_int]),
    "mirt_ctx_fused_passes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "mirt_render_frame": (C.c_int, [C.c_void_p, C.POINTER(_FrameDesc)]),
    "mirt_render_frame_aa": (C.c_int, [C.c_void_p, C.POINTER(_FrameDesc), C.c_uint32]),
    "mirt_ctx_set_frame_fusion": (C.c_int, [C.c_void_p, C.c_int]),
    "mirt_ctx_fused_frames": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "mirt_seed_fill": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32]),
    "mirt_zero": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mirt_timer_start": (C.c_int, [C.c_void_p]),
    "mirt_timer_stop_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mirt_ctx_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "mirt_pass_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "mirt_grid_build": (C.c_int, [C.c_void_p, C.POINTER(_GridBuildDesc), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]),
    "mirt_grid_gather_triangles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_int32),
                                             C.POINTER(C.c_double), C.c_float, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "mirt_grid_gather_spheres": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mirt_grid_gather_u32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mirt_debug_divcheck": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]),
    "mirt_capture_begin": (C.c_int, [C.c_void_p]),
    "mirt_capture_end": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "mirt_graph_launch": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mirt_graph_release": (C.c_int, [C.c_void_p]),
    "mirt_debug_prepared": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "mirt_debug_numerics": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "mirt_buf_invalidate": (C.c_int, [C.c_void_p]),
    "mirt_mesh_ingest": (C.c_int, [C.c_void_p, C.POINTER(_MeshIngestDesc), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mirt_group_create": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    "mirt_group_size": (C.c_int, [C.c_void_p]),
    "mirt_group_ctx": (C.c_void_p, [C.c_void_p, C.c_int]),
    "mirt_group_destroy": (C.c_int, [C.c_void_p]),
    "mirt_group_finish": (C.c_int, [C.c_void_p]),
    "mirt_tile_rows": (None, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mirt_gather": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "mirt_group_peer_access": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mirt_gather_route": (C.c_int, [C.c_void_p, C.c_int]),
    "mirt_filter_window_rows": (None, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mirt_upsample_low_rows": (None, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mirt_filter_atrous_rows": (C.c_int, [C.c_void_p, C.POINTER(_FilterDesc), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "mirt_upsample_guided_rows": (C.c_int, [C.c_void_p, C.POINTER(_UpsampleDesc), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "mirt_exchange_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int, C.c_size_t]),
}


def lib():
    """Load libmirt.so (built in-tree by __graft_entry__.build()).  Raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MirtError(-7, f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            if os.environ.get("MIRT_LIB_PATH") and not hasattr(l, name):
                continue   # an A/B build of an older tree (profiles/ab.sh): it lacks the newer entry points, which its runs do not call
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def device_count():
    return lib().mirt_device_count()


def filter_window_rows(image_height, row0, nrows, iterations):
    """-> (win_row0, win_nrows): the input rows that rows [row0, row0 + nrows) of the filtered image depend on (mirt_filter_window_rows);
    (0, 0) on bad input"""
    a, b = C.c_uint32(), C.c_uint32()
    lib().mirt_filter_window_rows(int(image_height), int(row0), int(nrows), int(iterations), C.byref(a), C.byref(b))
    return a.value, b.value


def upsample_low_rows(height, factor, row0, nrows):
    """-> (lo_row0, lo_nrows): the low rows that high rows [row0, row0 + nrows) of a `height`-row image read (mirt_upsample_low_rows); (0, 0) on
    bad input"""
    a, b = C.c_uint32(), C.c_uint32()
    lib().mirt_upsample_low_rows(int(height), int(factor), int(row0), int(nrows), C.byref(a), C.byref(b))
    return a.value, b.value


class Buffer:
    def __init__(self, ctx, handle, nbytes):
        self.ctx, self.h, self.nbytes = ctx, handle, nbytes

    def write(self, arr, offset=0):
        a = np.ascontiguousarray(arr)
        self.ctx._chk(lib().mirt_buf_write(self.h, offset, a.nbytes, a.ctypes.data_as(C.c_void_p), 0))
        return self

    def read(self, dtype, count=None, offset=0):
        dt = np.dtype(dtype)
        n = (self.nbytes - offset) // dt.itemsize if count is None else count
        out = np.empty(n, dt)
        self.ctx._chk(lib().mirt_buf_read(self.h, offset, out.nbytes, out.ctypes.data_as(C.c_void_p), 1))
        return out

    @property
    def device_ptr(self):
        return lib().mirt_buf_device_ptr(self.h)

    def invalidate(self):
        """the contents were changed behind the runtime (through device_ptr): mirt_buf_invalidate"""
        self.ctx._chk(lib().mirt_buf_invalidate(self.h))
        return self

    def release(self):
        if self.h:
            self.ctx._chk(lib().mirt_buf_release(self.h))
            self.h = None


class Kernel:
    """program.createKernel(name): setArg takes a Buffer or a numpy array, as WebCL takes a typed array."""

    def __init__(self, ctx, name):
        self.ctx, self.name = ctx, name
        h = C.c_void_p()
        ctx._chk(lib().mirt_kernel_get(ctx.h, name.encode(), C.byref(h)))
        self.h = h

    def set_arg(self, i, v):
        if isinstance(v, Buffer):
            self.ctx._chk(lib().mirt_kernel_set_arg_buf(self.h, i, v.h))
        else:
            a = np.ascontiguousarray(v)
            self.ctx._chk(lib().mirt_kernel_set_arg(self.h, i, a.nbytes, a.ctypes.data_as(C.c_void_p)))
        return self

    def set_args(self, *vals):
        for i, v in enumerate(vals):
            if v is not None:
                self.set_arg(i, v)
        return self

    def enqueue(self, global_ws, local_ws=None):
        g = (C.c_size_t * len(global_ws))(*global_ws)
        l = (C.c_size_t * len(local_ws))(*local_ws) if local_ws else None
        self.ctx._chk(lib().mirt_enqueue(self.ctx.h, self.h, len(global_ws), g, l))

    def release(self):
        if self.h:
            self.ctx._chk(lib().mirt_kernel_release(self.h))
            self.h = None


class Context:
    """webcl.createContext(device) + ctx.createCommandQueue()."""

    def __init__(self, device=0, _handle=None):
        if _handle is not None:            # a context owned by a DeviceGroup
            self.h, self.device, self.owned = C.c_void_p(_handle), device, False
            return
        h = C.c_void_p()
        rc = lib().mirt_ctx_create(device, C.byref(h))
        if rc != 0:
            raise MirtError(rc, lib().mirt_last_error(None).decode())
        self.h = h
        self.device = device
        self.owned = True

    def _chk(self, rc):
        if rc != 0:
            raise MirtError(rc, lib().mirt_last_error(self.h).decode())

    def last_error(self):
        return lib().mirt_last_error(self.h).decode()

    def _deferred(self, fn):
        """one mirt_*_deferred counter"""
        n = C.c_uint64()
        self._chk(fn(self.h, C.byref(n)))
        return n.value

    def buffer(self, nbytes, flags=MEM_READ_WRITE):
        h = C.c_void_p()
        self._chk(lib().mirt_buf_create(self.h, nbytes, flags, C.byref(h)))
        return Buffer(self, h, nbytes)

    def buffer_from(self, arr, flags=MEM_READ_ONLY):
        a = np.ascontiguousarray(arr)
        return self.buffer(max(a.nbytes, 1), flags).write(a) if a.nbytes else self.buffer(16, flags)

    def wrap(self, device_ptr, nbytes):
        h = C.c_void_p()
        self._chk(lib().mirt_buf_wrap(self.h, C.c_void_p(device_ptr), nbytes, C.byref(h)))
        return Buffer(self, h, nbytes)

    def kernel(self, name):
        return Kernel(self, name)

    def set_stream(self, hip_stream):
        self._chk(lib().mirt_ctx_set_stream(self.h, C.c_void_p(hip_stream)))

    def finish(self):
        self._chk(lib().mirt_finish(self.h))

    def seed_fill(self, buf, first_ray, count, seed_base=0):
        self._chk(lib().mirt_seed_fill(self.h, buf.h, first_ray, count, seed_base))

    def zero(self, buf):
        self._chk(lib().mirt_zero(self.h, buf.h))

    # launch-bound sequences as HIP graphs (mirt.h "launch-bound sequences")
    def capture_begin(self):
        self._chk(lib().mirt_capture_begin(self.h))

    def capture_end(self):
        g = C.c_void_p()
        self._chk(lib().mirt_capture_end(self.h, C.byref(g)))
        return g

    def graph_launch(self, g):
        self._chk(lib().mirt_graph_launch(self.h, g))

    def graph_release(self, g):
        lib().mirt_graph_release(g)

    def timer_start(self):
        self._chk(lib().mirt_timer_start(self.h))

    def timer_stop_ms(self):
        ms = C.c_float()
        self._chk(lib().mirt_timer_stop_ms(self.h, C.byref(ms)))
        return ms.value

    def pass_deferred(self):
        return self._deferred(lib().mirt_pass_deferred)

    def set_exact_only(self, on=True):
        self._chk(lib().mirt_ctx_set_exact_only(self.h, 1 if on else 0))

    def set_fusion(self, level=2):
        """command-stream fusion (include/mirt.h): 2 = whole executeRender passes issued kernel by kernel run as one fused launch"""
        self._chk(lib().mirt_ctx_set_fusion(self.h, int(level)))

    def fused_passes(self):
        n = C.c_uint64()
        self._chk(lib().mirt_ctx_fused_passes(self.h, C.byref(n)))
        return n.value

    def set_frame_fusion(self, on=True):
        """command-stream fusion of the Assign04 / Assign07 frame stream (include/mirt.h): initTrace + molTrace / meshTrace run as one launch"""
        self._chk(lib().mirt_ctx_set_frame_fusion(self.h, 1 if on else 0))

    def fused_frames(self):
        n = C.c_uint64()
        self._chk(lib().mirt_ctx_fused_frames(self.h, C.byref(n)))
        return n.value

    @staticmethod
    def frame_desc(assign, width, height, cam, pixel, bounds=None, n_slabs=0, mesh=None, mol=None, rays=None):
        """the mirt_frame_desc of render_frame's arguments"""
        d = _FrameDesc()
        d.struct_size, d.assign, d.width, d.height, d.n_slabs = C.sizeof(_FrameDesc), int(assign), int(width), int(height), int(n_slabs)
        d.cam = _f(cam, 16)
        if bounds is not None:
            d.bounds = _f(bounds, 8)
        h = lambda b: b.h if b is not None else None   # noqa: E731
        if mesh:
            d.t_size = int(mesh.get("t_size", 0))
            d.t_pos, d.t_normal, d.t_mindex, d.t_mcolor = h(mesh.get("pos")), h(mesh.get("normal")), h(mesh.get("mindex")), h(mesh.get("mcolor"))
            d.t_slab_size = h(mesh.get("slab_size"))
        if mol:
            d.s_size = int(mol.get("s_size", 0))
            d.s_atoms, d.s_mindex, d.s_mcolor, d.s_slab_size = h(mol.get("atoms")), h(mol.get("mindex")), h(mol.get("mcolor")), h(mol.get("slab_size"))
        d.pixel, d.rays = h(pixel), h(rays)
        return d

    def render_frame(self, assign, width, height, cam, pixel, bounds=None, n_slabs=0, mesh=None, mol=None, rays=None, aa=1):
        """mirt_render_frame: a whole Assign04 / Assign07 frame in one launch.  aa > 1: mirt_render_frame_aa, each of the width x height pixels the
        box average of aa x aa samples (no ray buffer then).  mesh: dict(t_size, pos, normal, mindex, mcolor[, slab_size]) of
        Buffers, mol: dict(s_size, atoms, mindex, mcolor, slab_size); both: the molecule, then the mesh.  rays: optional 48-byte-per-pixel Buffer."""
        d = self.frame_desc(assign, width, height, cam, pixel, bounds, n_slabs, mesh, mol, rays)
        if aa == 1:
            self._chk(lib().mirt_render_frame(self.h, C.byref(d)))
        else:
            self._chk(lib().mirt_render_frame_aa(self.h, C.byref(d), int(aa)))

    def set_profiling(self, on=True):
        self._chk(lib().mirt_ctx_set_profiling(self.h, 1 if on else 0))

    def pass_timing(self):
        a, b = C.c_float(), C.c_float()
        self._chk(lib().mirt_pass_timing(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def program_check(self, source):
        miss = C.create_string_buffer(1024)
        n = lib().mirt_program_check(self.h, source.encode(), miss, 1024)
        if n < 0:
            self._chk(n)
        return n, miss.value.decode()

    def debug_numerics(self, op, a, b=None):
        """op 0..14: one float per element; 20..28 except 25: float3 arguments as three consecutive floats (include/mirt.h).
        Op 28 (ray_guard) takes the origins as a and the directions as b, three floats each per ray, and returns one float per ray."""
        a = np.ascontiguousarray(a, np.float32)
        vec = op >= 20 and op != 25
        n = a.size // 3 if vec else a.size
        out_w = 3 if op in (21, 24) else 4 if op == 27 else 1
        da = self.buffer_from(a, MEM_READ_WRITE)
        db = self.buffer_from(np.ascontiguousarray(b, np.float32), MEM_READ_WRITE) if b is not None else None
        do = self.buffer(max(4 * n * out_w, 16))
        self._chk(lib().mirt_debug_numerics(self.h, op, da.h, db.h if db else None, do.h, n))
        out = do.read(np.float32, n * out_w)
        for x in (da, db, do):
            if x:
                x.release()
        return out

    def grid_build(self, kind, prims_f64, bounds6, n_slabs):
        """splitSphereData / splitTriangleData / splitMeshData on the device.  Returns (offsets Buffer, order Buffer, total)."""
        prims = np.ascontiguousarray(prims_f64, np.float64)
        per = 9 if kind else 4
        count = prims.size // per
        pb = self.buffer_from(prims, MEM_READ_WRITE) if count else None
        d = _GridBuildDesc()
        d.struct_size, d.kind, d.count, d.n_slabs = C.sizeof(_GridBuildDesc), kind, count, n_slabs
        d.bounds = (C.c_double * 6)(*[float(x) for x in bounds6])
        d.prims_f64 = pb.h if pb else None
        off, order, total = C.c_void_p(), C.c_void_p(), C.c_uint32()
        try:
            self._chk(lib().mirt_grid_build(self.h, C.byref(d), C.byref(off), C.byref(order), C.byref(total)))
        finally:
            if pb:
                pb.release()
        return Buffer(self, off, (n_slabs ** 3 + 1) * 4), Buffer(self, order, max(total.value * 4, 16)), total.value

    def grid_gather_triangles(self, order, total, pos_f64, nor_f64=None, steps=(), pad_w=0.0):
        pb = self.buffer_from(np.ascontiguousarray(pos_f64, np.float64), MEM_READ_WRITE)
        nb = self.buffer_from(np.ascontiguousarray(nor_f64, np.float64), MEM_READ_WRITE) if nor_f64 is not None else None
        ops = (C.c_int32 * 4)(*([s[0] for s in steps] + [0] * (4 - len(steps))))
        vecs = (C.c_double * 12)(*([float(x) for s in steps for x in s[1]] + [0.0] * (12 - 3 * len(steps))))
        po, no = C.c_void_p(), C.c_void_p()
        try:
            self._chk(lib().mirt_grid_gather_triangles(self.h, order.h, total, pb.h, nb.h if nb else None, len(steps), ops, vecs, pad_w,
                                                       C.byref(po), C.byref(no) if nb else None))
        finally:
            pb.release()
            if nb:
                nb.release()
        return Buffer(self, po, max(total * 48, 16)), (Buffer(self, no, max(total * 48, 16)) if nb else None)

    def grid_gather_spheres(self, order, total, sph_f64):
        sb = self.buffer_from(np.ascontiguousarray(sph_f64, np.float64), MEM_READ_WRITE)
        out = C.c_void_p()
        try:
            self._chk(lib().mirt_grid_gather_spheres(self.h, order.h, total, sb.h, C.byref(out)))
        finally:
            sb.release()
        return Buffer(self, out, max(total * 16, 16))

    def grid_gather_u32(self, order, total, values_u32):
        vb = self.buffer_from(np.ascontiguousarray(values_u32, np.uint32), MEM_READ_WRITE)
        out = C.c_void_p()
        try:
            self._chk(lib().mirt_grid_gather_u32(self.h, order.h, total, vb.h, C.byref(out)))
        finally:
            vb.release()
        return Buffer(self, out, max(total * 4, 16))

    def divcheck(self, mode, seed, count):
        out = self.buffer(16 * 8)
        self._chk(lib().mirt_debug_divcheck(self.h, mode, seed, count, out.h))
        r = out.read(np.uint64, 16)
        out.release()
        return r

    def prepared(self, positions, count):
        """the runtime's prepared copy of a triangle position buffer (records, group spheres, plane list) as bytes"""
        total = C.c_size_t(0)
        self._chk(lib().mirt_debug_prepared(self.h, positions.h, count, None, 0, C.byref(total)))
        out = np.zeros(total.value, np.uint8)
        self._chk(lib().mirt_debug_prepared(self.h, positions.h, count, out.ctypes.data_as(C.c_void_p), out.nbytes, C.byref(total)))
        return out

    def render_pass(self, desc, fresh=False):
        """fresh: the frame's first pass with initAcu folded in (mirt_render_first_pass): acu is not read."""
        f = lib().mirt_render_first_pass if fresh else lib().mirt_render_pass
        self._chk(f(self.h, C.byref(desc)))

    def render_passes(self, desc, n_passes, fresh=False, every_frame=False):
        """n_passes progressive passes from desc.pass_index on in one call (mirt_render_passes); fresh: the first of them starts the frame
        (MIRT_PASSES_FRESH: acu is not read, and may be None where the passes resolve their own pixels).  every_frame: desc.pixel / desc.radiance
        hold n_passes frames back to back, the frame after each pass (MIRT_PASSES_EVERY_FRAME)."""
        flags = (PASSES_FRESH if fresh else 0) | (PASSES_EVERY_FRAME if every_frame else 0)
        self._chk(lib().mirt_render_passes(self.h, C.byref(desc), int(n_passes), flags))

    def render_guides(self, desc, normal_hits=None, albedo_depth=None):
        """First-hit guide buffers of desc's row tile (mirt_render_guides): float4 per pixel, (sum of the hit samples' normals, hits) and
        (sum of their material colours, sum of their hit distances).  Either buffer may be None, not both; desc.seeds / acu are not touched."""
        self._chk(lib().mirt_render_guides(self.h, C.byref(desc), normal_hits.h if normal_hits else None, albedo_depth.h if albedo_depth else None))

    def render_first_pass_guided(self, desc, normal_hits=None, albedo_depth=None):
        """A frame's first pass and its guide buffers in one call (mirt_render_first_pass_guided): every buffer ends as after
        render_pass(desc, fresh=True) followed by render_guides(desc, normal_hits, albedo_depth).  Either guide may be None, not both."""
        self._chk(lib().mirt_render_first_pass_guided(self.h, C.byref(desc), normal_hits.h if normal_hits else None, albedo_depth.h if albedo_depth else None))

    def render_passes_guided(self, desc, n_passes, fresh=False, every_frame=False, normal_hits=None, albedo_depth=None):
        """n_passes progressive passes and the frame's guide buffers in one call (mirt_render_passes_guided): every buffer ends as after
        render_passes(desc, n_passes, fresh, every_frame) followed by render_guides(desc, normal_hits, albedo_depth).  Either guide may be None,
        not both."""
        flags = (PASSES_FRESH if fresh else 0) | (PASSES_EVERY_FRAME if every_frame else 0)
        self._chk(lib().mirt_render_passes_guided(self.h, C.byref(desc), int(n_passes), flags, normal_hits.h if normal_hits else None,
                                                  albedo_depth.h if albedo_depth else None))

    def guided_passes(self):
        """how many render_first_pass_guided / render_passes_guided calls of this context wrote the guides from the pass's own launch (mirt_ctx_guided_passes)"""
        n = C.c_uint64()
        self._chk(lib().mirt_ctx_guided_passes(self.h, C.byref(n)))
        return n.value

    def trace_closest(self, desc, rays, count, hits, sets=None):
        """The closest hit of `count` caller-supplied rays (mirt_trace_closest): rays holds 32-byte records {o, mint, d, maxt}, hits receives
        {normal, t, p, mat_id} (32 bytes) and sets (optional) a uint32 per ray, the index of the set that won.  Of desc only the primitive sets
        are read.  hits or sets may be None, not both."""
        self._chk(lib().mirt_trace_closest(self.h, C.byref(desc) if desc is not None else None, rays.h if rays else None, int(count),
                                           hits.h if hits else None, sets.h if sets else None))

    def trace_occluded(self, desc, rays, count, occluded):
        """Whether anything blocks each of `count` caller-supplied rays (mirt_trace_occluded): occluded receives a uint8 per ray, 1 iff the
        any-hit stage leaves mint == maxt (a ray that enters dead is reported 1)."""
        self._chk(lib().mirt_trace_occluded(self.h, C.byref(desc) if desc is not None else None, rays.h if rays else None, int(count),
                                            occluded.h if occluded else None))

    def trace_deferred(self):
        """how many rays the last trace_closest / trace_occluded call re-ran in the exact kernel (mirt_trace_deferred)"""
        return self._deferred(lib().mirt_trace_deferred)

    def trace_radiance(self, desc, rays, count, seeds, radiance, samples=1, flags=0):
        """Path radiance of `count` caller-supplied rays in one launch (mirt_trace_radiance): the pass's path -- closest hit, lightRender, per-light
        shadow and shade, desc.bounces bounces -- from each 32-byte ray record on, `samples` times per ray.  seeds (int32 per ray) is advanced in
        place; radiance (float4 per ray) receives the accumulator: rgb sums and the number of contributions, continued from its contents with
        RADIANCE_ACCUMULATE.  Of desc the primitive sets, lights, material and bounces are read.  A _RadianceDesc may be given in place of `samples`."""
        rd = samples if isinstance(samples, _RadianceDesc) else _RadianceDesc(C.sizeof(_RadianceDesc), int(samples), int(flags), 0)
        self._chk(lib().mirt_trace_radiance(self.h, C.byref(desc) if desc is not None else None, C.byref(rd) if rd is not None else None,
                                            rays.h if rays else None, int(count), seeds.h if seeds else None, radiance.h if radiance else None))

    def radiance_deferred(self):
        """how many rays the last trace_radiance call re-ran in the exact kernel (mirt_radiance_deferred)"""
        return self._deferred(lib().mirt_radiance_deferred)

    def view_rays(self, view, rays):
        """The rays of a panoramic, fisheye or orthographic camera's row tile as 32-byte records (mirt_view_rays): view.width * nrows * k * k of
        them, in (pixel, sy, sx) order.  view: a _ViewDesc (view_desc())."""
        self._chk(lib().mirt_view_rays(self.h, C.byref(view) if view is not None else None, rays.h if rays else None))

    def render_view(self, scene_desc, view, seeds, radiance=None, pixel=None):
        """A frame of a panoramic, fisheye or orthographic camera in one launch (mirt_render_view): the rays of view_rays, the pass's path along
        each (the sets, lights, material and bounces of scene_desc), and the per-pixel sums in copyToPixel's order -- into radiance (float4 per tile
        pixel, continued from its contents with VIEW_ACCUMULATE in view.flags) and / or pixel (RGBA8, tone-mapped with view.tone).  seeds (int32
        per tile ray) is advanced in place."""
        self._chk(lib().mirt_render_view(self.h, C.byref(scene_desc) if scene_desc is not None else None, C.byref(view) if view is not None else None,
                                         seeds.h if seeds else None, radiance.h if radiance else None, pixel.h if pixel else None))

    def view_deferred(self):
        """how many rays the last render_view, render_view_batch or render_view_guided_batch call re-ran in the exact kernel, in whole blocks of 256 (mirt_view_deferred)"""
        return self._deferred(lib().mirt_view_deferred)

    @staticmethod
    def _cameras(cameras):
        """-> (host pointer or None, n_frames, the array that keeps the pointer alive): cameras is None or anything np.asarray(..., float32)
        turns into [N, 12] -- eye, right, up, forward per frame (mirt_view_camera)"""
        if cameras is None:
            return None, 0, None
        cam = np.ascontiguousarray(np.asarray(cameras, np.float32))
        if cam.size == 0:
            return None, 0, cam
        if cam.ndim != 2 or cam.shape[1] != 12:
            raise ValueError(f"cameras: expected [N, 12] floats (eye, right, up, forward per frame), got {cam.shape}")
        return cam.ctypes.data_as(C.c_void_p), cam.shape[0], cam

    def view_rays_batch(self, view, cameras, rays):
        """The rays of N cameras' frames of one descriptor, frame after frame (mirt_view_rays_batch): N * view.width * view.height * k * k
        records, frame f's as view_rays writes them for `view` with the basis cameras[f].  cameras: [N, 12], a host array."""
        ptr, n, keep = self._cameras(cameras)
        self._chk(lib().mirt_view_rays_batch(self.h, C.byref(view) if view is not None else None, ptr, n, rays.h if rays else None))

    def render_view_batch(self, scene_desc, view, cameras, seeds, radiance=None, pixel=None):
        """N cameras' frames of one descriptor in one launch (mirt_render_view_batch): the buffers hold the frames back to back, and frame f
        ends in each as after render_view on its slice with the basis cameras[f] ([N, 12] floats on the host: eye, right, up, forward;
        view's own basis is not read).  VIEW_ACCUMULATE and view.tone apply to every frame."""
        ptr, n, keep = self._cameras(cameras)
        self._chk(lib().mirt_render_view_batch(self.h, C.byref(scene_desc) if scene_desc is not None else None, C.byref(view) if view is not None else None,
                                               ptr, n, seeds.h if seeds else None, radiance.h if radiance else None, pixel.h if pixel else None))

    def view_guides(self, scene_desc, view, normal_hits=None, albedo_depth=None):
        """The first-hit guides of a panoramic, fisheye or orthographic camera's row tile in one launch (mirt_view_guides): float4 per tile pixel
        each, as render_guides writes them for the thin lens -- what filter_atrous reads.  Either may be None, not both.  Depth is in units of
        |forward| and the basis as given."""
        self._chk(lib().mirt_view_guides(self.h, C.byref(scene_desc) if scene_desc is not None else None, C.byref(view) if view is not None else None,
                                         normal_hits.h if normal_hits else None, albedo_depth.h if albedo_depth else None))

    def render_view_guided(self, scene_desc, view, seeds, radiance=None, pixel=None, normal_hits=None, albedo_depth=None):
        """render_view and view_guides in one call (mirt_render_view_guided): the same bytes in every buffer; at k = 1, 2, 4 and 8 the frame's own
        launch writes the guides (guided_views counts those calls).  The outputs are final in stream order."""
        self._chk(lib().mirt_render_view_guided(self.h, C.byref(scene_desc) if scene_desc is not None else None, C.byref(view) if view is not None else None,
                                                seeds.h if seeds else None, radiance.h if radiance else None, pixel.h if pixel else None,
                                                normal_hits.h if normal_hits else None, albedo_depth.h if albedo_depth else None))

    def guided_views(self):
        """how many render_view_guided and render_view_guided_batch calls of this context wrote the guides from the frame's own launch (mirt_ctx_guided_views)"""
        n = C.c_uint64()
        self._chk(lib().mirt_ctx_guided_views(self.h, C.byref(n)))
        return n.value

    def render_ao(self, desc, ao_out, samples=AO_DEFAULT_SAMPLES, radius=float("inf"), bias=AO_DEFAULT_BIAS):
        """Ambient occlusion of the first hit of desc's row tile in one launch (mirt_render_ao): ao_out receives uint32 {open, cast} per pixel --
        per hit primary sample `samples` hemisphere rays of length `radius` from the hit point, displaced by `bias` along the normal; cast counts
        them, open those nothing blocks.  desc.seeds is read and not written.  An _AoDesc may be given in place of `samples`."""
        ao = samples if isinstance(samples, _AoDesc) else _AoDesc(C.sizeof(_AoDesc), int(samples), float(radius), float(bias))
        self._chk(lib().mirt_render_ao(self.h, C.byref(desc) if desc is not None else None, C.byref(ao) if ao is not None else None,
                                       ao_out.h if ao_out else None))

    def ao_deferred(self):
        """how many pixels the last render_ao call re-ran in the exact kernel (mirt_ao_deferred)"""
        return self._deferred(lib().mirt_ao_deferred)

    def view_ao(self, scene_desc, view, seeds, ao_out, samples=AO_DEFAULT_SAMPLES, radius=float("inf"), bias=AO_DEFAULT_BIAS):
        """Ambient occlusion of a panoramic, fisheye or orthographic camera's row tile in one launch (mirt_view_ao): ao_out receives uint32
        {open, cast} per tile pixel, as render_ao writes them for the thin lens, from the rays of view_rays.  seeds (int32 per tile ray) is read
        and not written; of scene_desc only the primitive sets are read.  An _AoDesc may be given in place of `samples`."""
        ao = samples if isinstance(samples, _AoDesc) else _AoDesc(C.sizeof(_AoDesc), int(samples), float(radius), float(bias))
        self._chk(lib().mirt_view_ao(self.h, C.byref(scene_desc) if scene_desc is not None else None, C.byref(view) if view is not None else None,
                                     C.byref(ao) if ao is not None else None, seeds.h if seeds else None, ao_out.h if ao_out else None))

    def view_ao_deferred(self):
        """how many pixels the last view_ao or view_ao_batch call re-ran in the exact kernel (mirt_view_ao_deferred)"""
        return self._deferred(lib().mirt_view_ao_deferred)

    def view_guides_batch(self, scene_desc, view, cameras, normal_hits=None, albedo_depth=None):
        """The first-hit guides of N cameras' frames in one launch (mirt_view_guides_batch): the buffers hold the frames back to back, and
        frame f ends in each as after view_guides on its slice with the basis cameras[f] ([N, 12] floats on the host)."""
        ptr, n, keep = self._cameras(cameras)
        self._chk(lib().mirt_view_guides_batch(self.h, C.byref(scene_desc) if scene_desc is not None else None, C.byref(view) if view is not None else None,
                                               ptr, n, normal_hits.h if normal_hits else None, albedo_depth.h if albedo_depth else None))

    def render_view_guided_batch(self, scene_desc, view, cameras, seeds, radiance=None, pixel=None, normal_hits=None, albedo_depth=None):
        """render_view_batch and view_guides_batch in one call (mirt_render_view_guided_batch): the same bytes in every buffer; at k = 1, 2, 4
        and 8 the frames' own launch writes the guides (guided_views counts the call once).  The outputs are final in stream order."""
        ptr, n, keep = self._cameras(cameras)
        self._chk(lib().mirt_render_view_guided_batch(self.h, C.byref(scene_desc) if scene_desc is not None else None,
                                                      C.byref(view) if view is not None else None, ptr, n, seeds.h if seeds else None,
                                                      radiance.h if radiance else None, pixel.h if pixel else None,
                                                      normal_hits.h if normal_hits else None, albedo_depth.h if albedo_depth else None))

    def view_ao_batch(self, scene_desc, view, cameras, seeds, ao_out, samples=AO_DEFAULT_SAMPLES, radius=float("inf"), bias=AO_DEFAULT_BIAS):
        """Ambient occlusion of N cameras' frames in one launch (mirt_view_ao_batch): seeds (int32 per ray of the batch, read and not written)
        and ao_out (uint32 {open, cast} per pixel) hold the frames back to back, frame f's as view_ao leaves them with the basis cameras[f].
        An _AoDesc may be given in place of `samples`."""
        ao = samples if isinstance(samples, _AoDesc) else _AoDesc(C.sizeof(_AoDesc), int(samples), float(radius), float(bias))
        ptr, n, keep = self._cameras(cameras)
        self._chk(lib().mirt_view_ao_batch(self.h, C.byref(scene_desc) if scene_desc is not None else None, C.byref(view) if view is not None else None,
                                           ptr, n, C.byref(ao) if ao is not None else None, seeds.h if seeds else None, ao_out.h if ao_out else None))

    def filter_atrous(self, width, height, tone, radiance, normal_hits, albedo_depth, filtered=None, pixel=None, iterations=None,
                      normal_power_log2=None, sigma_depth=None, sigma_colour=None, demodulate=None, structure=None):
        """The edge-avoiding a-trous filter (mirt_filter_atrous, defined in include/mirt.h) of a width x height frame on the device: radiance as a
        pass writes it, the guides as render_guides writes them, tone = 1 / (rays_per_pixel * passes).  Writes `filtered` (float4 per pixel,
        un-scaled like radiance) and / or `pixel` (RGBA8).  Parameters left None are FILTER_DEFAULTS; structure: None (the measured choice per
        step), "direct" or "tiled"."""
        d = self._filter_desc(width, height, tone, radiance, normal_hits, albedo_depth, filtered, pixel, iterations, normal_power_log2, sigma_depth,
                              sigma_colour, demodulate, structure)
        self._chk(lib().mirt_filter_atrous(self.h, C.byref(d)))

    def filter_atrous_rows(self, width, image_height, win_row0, win_nrows, row0, nrows, tone, radiance, normal_hits, albedo_depth, filtered=None,
                           pixel=None, **params):
        """filter_atrous on rows [row0, row0 + nrows) of a width x image_height image (mirt_filter_atrous_rows): the three inputs hold the image
        rows [win_row0, win_row0 + win_nrows), a window that contains filter_window_rows(image_height, row0, nrows, iterations); `filtered` /
        `pixel` hold the nrows own rows alone and end as those rows of the whole-frame call, bit for bit.  params as filter_atrous."""
        d = self._filter_desc(width, win_nrows, tone, radiance, normal_hits, albedo_depth, filtered, pixel, **params)
        self._chk(lib().mirt_filter_atrous_rows(self.h, C.byref(d), int(image_height), int(win_row0), int(row0), int(nrows)))

    @staticmethod
    def _filter_desc(width, height, tone, radiance, normal_hits, albedo_depth, filtered=None, pixel=None, iterations=None,
                     normal_power_log2=None, sigma_depth=None, sigma_colour=None, demodulate=None, structure=None):
        v = dict(FILTER_DEFAULTS)
        for k, x in (("iterations", iterations), ("normal_power_log2", normal_power_log2), ("sigma_depth", sigma_depth), ("sigma_colour", sigma_colour),
                     ("demodulate", demodulate)):
            if x is not None:
                v[k] = x
        d = _FilterDesc()
        d.struct_size = C.sizeof(_FilterDesc)
        d.width, d.height, d.iterations, d.normal_power_log2 = int(width), int(height), int(v["iterations"]), int(v["normal_power_log2"])
        d.flags = (FILTER_DEMODULATE if v["demodulate"] else 0) | {None: 0, "direct": FILTER_DIRECT, "tiled": FILTER_TILED}[structure]
        d.tone, d.sigma_depth, d.sigma_colour = float(tone), float(v["sigma_depth"]), float(v["sigma_colour"])
        d.radiance, d.normal_hits, d.albedo_depth = (b.h if b else None for b in (radiance, normal_hits, albedo_depth))
        d.filtered, d.pixel = (filtered.h if filtered else None), (pixel.h if pixel else None)
        return d

    def upsample_guided(self, width, height, factor, tone, radiance_lo, normal_hits_lo, albedo_depth_lo, normal_hits, albedo_depth,
                        upsampled=None, pixel=None, normal_power_log2=None, sigma_depth=None, demodulate=None):
        """Guide-driven upsampling (mirt_upsample_guided, defined in include/mirt.h) on the device: the radiance of a (width / factor) x
        (height / factor) frame -- as a pass or filter_atrous wrote it, tone = that frame's 1 / (rays_per_pixel * passes) -- rebuilt at
        width x height from the guides of both resolutions (render_guides at each size).  Writes `upsampled` (float4 per high pixel, un-scaled
        like radiance) and / or `pixel` (RGBA8).  Parameters left None are UPSAMPLE_DEFAULTS."""
        d = self._upsample_desc(width, height, factor, tone, radiance_lo, normal_hits_lo, albedo_depth_lo, normal_hits, albedo_depth, upsampled, pixel,
                                normal_power_log2, sigma_depth, demodulate)
        self._chk(lib().mirt_upsample_guided(self.h, C.byref(d)))

    def upsample_guided_rows(self, width, height, factor, row0, nrows, lo_row0, lo_nrows, tone, radiance_lo, normal_hits_lo, albedo_depth_lo,
                             normal_hits, albedo_depth, upsampled=None, pixel=None, **params):
        """upsample_guided on high rows [row0, row0 + nrows) of the width x height image (mirt_upsample_guided_rows): the high guides and the outputs
        hold those rows alone, the three low inputs the low rows [lo_row0, lo_row0 + lo_nrows), a range that contains upsample_low_rows(height,
        factor, row0, nrows).  The outputs end as those rows of the whole-frame call, bit for bit.  params as upsample_guided."""
        d = self._upsample_desc(width, height, factor, tone, radiance_lo, normal_hits_lo, albedo_depth_lo, normal_hits, albedo_depth, upsampled, pixel, **params)
        self._chk(lib().mirt_upsample_guided_rows(self.h, C.byref(d), int(row0), int(nrows), int(lo_row0), int(lo_nrows)))

    @staticmethod
    def _upsample_desc(width, height, factor, tone, radiance_lo, normal_hits_lo, albedo_depth_lo, normal_hits, albedo_depth,
                       upsampled=None, pixel=None, normal_power_log2=None, sigma_depth=None, demodulate=None):
        v = dict(UPSAMPLE_DEFAULTS)
        for k, x in (("normal_power_log2", normal_power_log2), ("sigma_depth", sigma_depth), ("demodulate", demodulate)):
            if x is not None:
                v[k] = x
        d = _UpsampleDesc()
        d.struct_size = C.sizeof(_UpsampleDesc)
        d.width, d.height, d.factor, d.normal_power_log2 = int(width), int(height), int(factor), int(v["normal_power_log2"])
        d.flags = UPSAMPLE_DEMODULATE if v["demodulate"] else 0
        d.tone, d.sigma_depth = float(tone), float(v["sigma_depth"])
        d.radiance_lo, d.normal_hits_lo, d.albedo_depth_lo = (b.h if b else None for b in (radiance_lo, normal_hits_lo, albedo_depth_lo))
        d.normal_hits, d.albedo_depth = (b.h if b else None for b in (normal_hits, albedo_depth))
        d.upsampled, d.pixel = (upsampled.h if upsampled else None), (pixel.h if pixel else None)
        return d

    def destroy(self):
        if self.h:
            lib().mirt_ctx_destroy(self.h)
            self.h = None


def view_desc(model, width, height, k=1, eye=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), half_w=1.0, half_h=1.0,
              half_angle=float(np.pi) / 2, t_min=0.0, t_max=float("inf"), tone=1.0, row0=0, nrows=0, flags=0):
    """-> a _ViewDesc (mirt_view_desc) for a camera at `eye` looking at `look_at`: forward = normalize(look_at - eye), right = normalize(forward x
    up), up' = right x forward -- computed in double and narrowed to fp32 once.  model: VIEW_* or one of VIEW_MODELS' names.  The fields stay
    writable: a caller with a basis of its own assigns eye / right / up / forward afterwards."""
    def norm(a):
        l = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
        return [a[0] / l, a[1] / l, a[2] / l]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    e, t, u = ([float(c) for c in v] for v in (eye, look_at, up))   # the same double operations as host/renderer.js makeView
    f = norm([t[0] - e[0], t[1] - e[1], t[2] - e[2]])
    r = norm(cross(f, u))
    u = cross(r, f)
    d = _ViewDesc()
    d.struct_size = C.sizeof(_ViewDesc)
    d.model = VIEW_MODELS[model] if isinstance(model, str) else int(model)
    d.width, d.height, d.k, d.row0, d.nrows, d.flags = int(width), int(height), int(k), int(row0), int(nrows), int(flags)
    for name, v in (("eye", e), ("right", r), ("up", u), ("forward", f)):
        setattr(d, name, (C.c_float * 3)(*(float(np.float32(c)) for c in v)))
    d.half_w, d.half_h, d.half_angle, d.t_min, d.t_max, d.tone = (float(np.float32(x)) for x in (half_w, half_h, half_angle, t_min, t_max, tone))
    return d


def _f(arr, n):
    return (C.c_float * n)(*[float(x) for x in np.asarray(arr, np.float32).ravel()[:n]])


class DeviceScene:
    """Uploads the packed kernel inputs of one scene (the arrays the reference host would
    enqueueWriteBuffer: A10 code.js:1183-1185, 1231-1234, 1276-1278, 1379) and keeps the
    handles.  `s` is a pyhost.scene.PackedScene (or anything with its attributes)."""

    def __init__(self, ctx, s):
        self.ctx, self.s = ctx, s
        self.bufs = []
        up = self._up
        self.sph = self.tri = None
        if s.has_spheres:
            self.sph = dict(prims=up(s.spheres), matid=up(s.s_matid), off=up(s.s_box), bounds=s.sphere_bounds, n=s.n_slabs)
        if s.has_triangles:
            self.tri = dict(prims=up(s.t_pos), normals=up(s.t_normal), matid=up(s.t_matid), off=up(s.t_box),
                            bounds=s.triangle_bounds, n=s.n_slabs)
        self.meshes = [dict(prims=up(m["pos"]), normals=up(m["normal"]), off=up(m["box"]), bounds=m["bounds"],
                            n=m["nslabs"], matid=m["matid"]) for m in s.meshes]
        self.material = up(s.materials)

    def _up(self, arr):
        b = self.ctx.buffer_from(arr)
        self.bufs.append(b)
        return b

    def _grid(self, g, mesh=False):
        out = _Grid()
        out.prims = g["prims"].h
        out.normals = g["normals"].h if "normals" in g else None
        out.matid = None if mesh else g["matid"].h
        out.cell_offsets = g["off"].h
        out.bounds = _f(g["bounds"], 8)
        out.n_slabs = int(g["n"])
        out.mesh_matid = int(g["matid"]) if mesh else 0
        return out

    def pass_desc(self, seeds, acu, pixel=None, radiance=None, pass_index=1, bounces=5, row0=0, nrows=0):
        s = self.s
        d = _PassDesc()
        d.struct_size = C.sizeof(_PassDesc)
        d.width, d.height, d.rays_per_pixel = s.width, s.height, s.rpp
        d.row0, d.nrows, d.bounces, d.pass_index = row0, nrows, bounces, pass_index
        d.cam = _f(s.cam, 16)
        d.scene_bounds = _f(s.bounds, 8)
        d.focal_length, d.lens_rad = s.focal_length, s.lens_rad
        keep = []
        if self.sph:
            g = self._grid(self.sph); keep.append(g); d.spheres = C.pointer(g)
        if self.tri:
            g = self._grid(self.tri); keep.append(g); d.triangles = C.pointer(g)
        if self.meshes:
            arr = (_Grid * len(self.meshes))(*[self._grid(m, mesh=True) for m in self.meshes])
            keep.append(arr); d.meshes = C.cast(arr, C.POINTER(_Grid))
        d.n_meshes = len(self.meshes)
        larr = (_Light * max(1, len(s.lights)))()
        for i, l in enumerate(s.lights):
            larr[i].shadow, larr[i].scene, larr[i].light = _f(l["shadow"], 16), _f(l["scene"], 16), _f(l["light"], 16)
        keep.append(larr)
        d.lights = C.cast(larr, C.POINTER(_Light))
        d.n_lights = len(s.lights)
        d.material = self.material.h
        d.seeds, d.acu = (seeds.h if seeds else None), (acu.h if acu else None)   # acu None: a frame's first pass that resolves its pixels itself (include/mirt.h)
        d.pixel = pixel.h if pixel else None
        d.radiance = radiance.h if radiance else None
        d._keep = keep
        return d

    def release(self):
        for b in self.bufs:
            b.release()
        self.bufs = []


class DeviceGroup:
    """mirt_group: N contexts in one process (one per device) + mirt_gather, the one exchange of the path."""

    def __init__(self, devices):
        ids = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        rc = lib().mirt_group_create(ids, len(devices), C.byref(h))
        if rc != 0:
            raise MirtError(rc, lib().mirt_last_error(None).decode())
        self.h = h
        self.contexts = [Context(d, _handle=lib().mirt_group_ctx(h, i)) for i, d in enumerate(devices)]

    def tile_rows(self, height, index):
        r0, n = C.c_uint32(), C.c_uint32()
        lib().mirt_tile_rows(height, len(self.contexts), index, C.byref(r0), C.byref(n))
        return r0.value, n.value

    GATHER_AUTO, GATHER_RCCL, GATHER_COPY = 0, 1, 2

    def gather(self, tiles, tile_bytes, out, root=0, use_rccl=False, transport=None):
        """transport: GATHER_AUTO (RCCL for N > 1 distinct devices, copies otherwise), GATHER_RCCL, GATHER_COPY; use_rccl=True == GATHER_RCCL"""
        n = len(tiles)
        hs = (C.c_void_p * n)(*[t.h for t in tiles])
        bs = (C.c_size_t * n)(*tile_bytes)
        if transport is None:
            transport = self.GATHER_RCCL if use_rccl else self.GATHER_AUTO
        rc = lib().mirt_gather(self.h, hs, bs, n, out.h, root, transport)
        if rc != 0:
            raise MirtError(rc, lib().mirt_last_error(self.contexts[0].h).decode())

    def exchange_rows(self, src, src_rows, dst, dst_rows, row_bytes):
        """The halo exchange (mirt_exchange_rows).  Per context i: src[i] (a Buffer or None) holds, from its first byte on, the image rows
        src_rows[i] = (row0, nrows) that the context owns; dst[i] (a Buffer or None) ends holding the image rows dst_rows[i] = (row0, nrows),
        each copied from whichever context owns it.  Rows are row_bytes bytes.  Ordered after the work queued on the sources; a source may be
        overwritten right after the call; complete after finish() of the destination's context."""
        n = len(src)
        hs = (C.c_void_p * n)(*[b.h if b else None for b in src])
        hd = (C.c_void_p * max(1, len(dst)))(*[b.h if b else None for b in dst])
        u = lambda rows, k: (C.c_uint32 * max(1, len(rows)))(*[int(r[k]) for r in rows])
        rc = lib().mirt_exchange_rows(self.h, hs, u(src_rows, 0), u(src_rows, 1), hd, u(dst_rows, 0), u(dst_rows, 1), n, int(row_bytes))
        if rc != 0:
            raise MirtError(rc, lib().mirt_last_error(self.contexts[0].h).decode())

    ROUTES = {0: "none", 1: "rccl", 2: "peer", 3: "staged", 4: "local"}

    def routes(self):
        """how the last gather moved each tile (mirt_gather_route)"""
        return [self.ROUTES.get(lib().mirt_gather_route(self.h, i), "?") for i in range(len(self.contexts))]

    def peer_access(self, i, j):
        return lib().mirt_group_peer_access(self.h, i, j)

    def finish(self):
        rc = lib().mirt_group_finish(self.h)
        if rc != 0:
            raise MirtError(rc, lib().mirt_last_error(self.contexts[0].h).decode())

    def destroy(self):
        if self.h:
            lib().mirt_group_destroy(self.h)
            self.h = None
