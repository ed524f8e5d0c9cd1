"""ctypes binding of the C ABI in ``include/pt_abi.h`` (``lib/libpt.so``).

This is the Python-side equivalent of the ``extern "C"`` block a Rust host
would declare.  There is no fallback: if the HIP library is
missing the import of anything that renders raises immediately.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_size_t, c_uint8, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpt.so")

PT_OK = 0
PT_ERR_INVALID = -1
PT_ERR_HIP = -2
PT_ERR_UNSUPPORTED = -3
PT_ERR_STATE = -4
PT_ERR_RCCL = -5
PT_ERR_SIZE = -6

PT_NODE_UNION, PT_NODE_SPHERE, PT_NODE_CUBE, PT_NODE_TORUS, PT_NODE_OCTAHEDRON, PT_NODE_PLANE = range(6)
PT_UNION_TYPE_UNION, PT_UNION_TYPE_SUBTRACTION = 0, 1
PT_OP_UNION_BEGIN, PT_OP_SHAPE, PT_OP_UNION_END = 0, 1, 2
PT_COMBINE_ASSIGN, PT_COMBINE_UNION, PT_COMBINE_SUBTRACTION = 0, 1, 2
PT_SO_SCALAR, PT_SO_VEC3, PT_SO_ONE, PT_SO_TORUS = 0, 1, 2, 3
PT_COMM_ID_BYTES = 128
PT_DISPLAY_RGBA32F, PT_DISPLAY_SRGB8 = 0, 1
PT_DENOISE_LINEAR = 2  # pt_denoise only: linear RGBA32F in accumulation order
PT_STAT_COUNT = 32
STAT_NAMES = (
    "samples", "segments", "march_steps", "normal_maps", "shaded", "aabb_tests", "xform_union", "xform_shape",
    "sdf_sphere", "sdf_cube", "sdf_torus", "sdf_octahedron", "comb_union", "comb_sub", "comb_assign", "rr_break",
    "wave_maps", "wave_shapes", "wave_iters", "lane_idle", "idle_shade", "idle_free",
    # wavefront kernel, wave-clock cycles (s_memtime) per phase, summed over waves
    "cyc_refill", "cyc_bounds", "cyc_map", "cyc_shade", "cyc_total",
    "culled", "wave_evals", "bounds_waves", "bounds_exact",
    "shaded_first",  # binned pipeline: hits shaded in shade pass 0
)

PT_ST_COUNT = len(STAT_NAMES)  # device counters (pt_device.h PT_ST_COUNT)

PT_PROBE_INTERP, PT_PROBE_TABLE, PT_PROBE_BAKED = 0, 1, 2  # which map() / bounds() a probe runs
PT_PROBE_MAP, PT_PROBE_MAP_B0, PT_PROBE_MAP_B1 = 0, 1, 2  # pt_probe_map's variant: JitMap, JitMapB0, JitMapB1

PT_MATH = {"max": 0, "min": 1, "sqrt": 2, "sqrtf": 3, "sin": 4, "cos": 5, "div": 6, "fma": 7}


class Constants(Structure):
    """== ``Constants`` UBO (path_tracer.rs:149-155)."""

    _fields_ = [("time", c_float), ("frame", c_int32), ("aspect", c_float), ("last_clear", c_int32)]


class Settings(Structure):
    """== ``Settings`` UBO (path_tracer.rs:157-163); defaults match the reference sliders."""

    _fields_ = [("debug", c_int32), ("bounces", c_int32), ("scale", c_float), ("fov", c_float), ("aabb", c_int32)]


class Camera(Structure):
    """pt_camera: pose and lens of ``pt_set_camera`` (new; the reference's
    view is fixed at origin (0, 0, -3) with the identity basis)."""

    _fields_ = [("origin", c_float * 3), ("right", c_float * 3), ("up", c_float * 3), ("forward", c_float * 3),
                ("aperture", c_float), ("focus", c_float)]


class Sky(Structure):
    """pt_sky: gradient and sun of ``pt_set_sky`` (new; in the reference a ray
    that leaves the scene adds nothing)."""

    _fields_ = [("bottom", c_float * 3), ("top", c_float * 3), ("sun_dir", c_float * 3), ("sun_color", c_float * 3),
                ("sun_cos", c_float)]


class DenoiseParams(Structure):
    """pt_denoise_params: the a-trous filter of ``pt_denoise`` (new)."""

    _fields_ = [("iterations", c_uint32), ("normal_power_log2", c_uint32), ("sigma_color", c_float),
                ("sigma_depth", c_float), ("sigma_albedo", c_float)]


class GuidedParams(Structure):
    """pt_guided_params: the variance-guided filter of ``pt_denoise_guided`` (new)."""

    _fields_ = [("iterations", c_uint32), ("normal_power_log2", c_uint32), ("sigma_variance", c_float),
                ("sigma_depth", c_float), ("sigma_albedo", c_float)]


class TemporalParams(Structure):
    """pt_temporal_params: the history cap and the reprojection tests of ``pt_temporal_accumulate`` (new)."""

    _fields_ = [("max_history", c_float), ("depth_tolerance", c_float), ("normal_cos", c_float),
                ("albedo_tolerance", c_float)]


PT_MESH_BRICK, PT_MESH_MAX_CELLS, PT_MESH_MAX_PROJECT = 8, 1024, 8
PT_RAYS_MAX = 1 << 26  # rays or pixels per pt_trace_rays / pt_pick_pixels / pt_trace_radiance call
PT_RADIANCE_RAY, PT_RADIANCE_HEMISPHERE = 0, 1  # pt_radiance_params.mode
PT_RADIANCE_MAX_SPP = 65536


class RadianceParams(Structure):
    """pt_radiance_params: the samples, stream, depth and mode of ``pt_trace_radiance`` (new)."""

    _fields_ = [("spp", c_uint32), ("sample0", c_uint32), ("seed", c_uint32), ("bounces", c_int32), ("mode", c_int32)]


PT_PREVIEW_MAX_SHADOW_STEPS = 64


class PreviewParams(Structure):
    """pt_preview_params: the key light, ambient gradient, shadow march, occlusion taps and highlight of
    ``pt_render_preview`` (new)."""

    _fields_ = [("light_dir", c_float * 3), ("light_color", c_float * 3), ("ambient_bottom", c_float * 3),
                ("ambient_top", c_float * 3), ("shadow_steps", c_uint32), ("shadow_k", c_float),
                ("shadow_cull", c_uint32), ("ao_strength", c_float), ("ao_radius", c_float), ("highlight", c_int32),
                ("highlight_color", c_float * 3), ("highlight_mix", c_float)]


class MeshDesc(Structure):
    """pt_mesh_desc: the grid, iso value and projection steps of ``pt_mesh_extract`` (new)."""

    _fields_ = [("origin", c_float * 3), ("cell", c_float), ("cells", c_uint32 * 3), ("iso", c_float),
                ("project", c_uint32)]


class MeshInfo(Structure):
    """pt_mesh_info: what ``pt_mesh_extract`` made and what it cost."""

    _fields_ = [("n_vertices", c_uint32), ("n_triangles", c_uint32), ("clipped_edges", c_uint32),
                ("void_cells", c_uint32), ("dropped_quads", c_uint32), ("bricks", c_uint32),
                ("bricks_evaluated", c_uint32), ("reserved", c_uint32), ("corner_evals", c_uint64),
                ("device_bytes", c_uint64)]


class SceneNode(Structure):
    _fields_ = [
        ("kind", c_int32), ("parent", c_int32), ("union_type", c_int32), ("aabb", c_int32),
        ("scale", c_float), ("position", c_float * 3), ("rotation", c_float * 3), ("aabb_exaggeration", c_float),
        ("size", c_float * 3), ("material", c_float * 18),
    ]


PT_NODE_FLOATS = 29


class FloatKey(Structure):
    """pt_float_key: a Float's u128 serde hash (lo, hi); {0, 0} = anonymous."""

    _fields_ = [("lo", c_uint64), ("hi", c_uint64)]


class Op(Structure):
    _fields_ = [
        ("opcode", c_uint32), ("shape", c_uint32), ("combine", c_uint32), ("check", c_int32),
        ("scale", c_uint32), ("position", c_uint32 * 3), ("rotation", c_uint32 * 3), ("aabb_exaggeration", c_uint32),
        ("size", c_uint32 * 3), ("material", c_uint32 * 18),
    ]


class Aabb(Structure):
    _fields_ = [
        ("back", c_int32), ("so_kind", c_uint32), ("union_position", c_uint32 * 3), ("union_scale", c_uint32),
        ("shape_position", c_uint32 * 3), ("shape_scale", c_uint32), ("size", c_uint32 * 3),
        ("aabb_exaggeration", c_uint32),
    ]


assert ctypes.sizeof(Constants) == 16 and ctypes.sizeof(Settings) == 20
assert ctypes.sizeof(Camera) == 56 and ctypes.sizeof(Sky) == 52 and ctypes.sizeof(DenoiseParams) == 20
assert ctypes.sizeof(GuidedParams) == 20 and ctypes.sizeof(TemporalParams) == 16
assert ctypes.sizeof(MeshDesc) == 36 and ctypes.sizeof(MeshInfo) == 48 and ctypes.sizeof(RadianceParams) == 20
assert ctypes.sizeof(PreviewParams) == 88
assert ctypes.sizeof(SceneNode) == 132 and ctypes.sizeof(Op) == 132 and ctypes.sizeof(Aabb) == 56


# Every entry point include/pt_abi.h declares: name -> (restype, argtypes).
_ctx = c_void_p
_u32p, _f32p = POINTER(c_uint32), POINTER(c_float)
_u64p = POINTER(c_uint64)
SIGNATURES = {
    "pt_compile_scene": (c_int, [POINTER(SceneNode), c_uint32, POINTER(Op), c_uint32, _u32p, POINTER(Aabb), c_uint32,
                                 _u32p, _f32p, c_uint32, _u32p, _u32p]),
    "pt_compile_scene_keyed": (c_int, [POINTER(SceneNode), c_uint32, POINTER(FloatKey), POINTER(Op), c_uint32, _u32p,
                                       POINTER(Aabb), c_uint32, _u32p, _f32p, c_uint32, _u32p, _u32p]),
    "pt_save_rgba8": (c_int, [_f32p, c_uint32, c_uint32, POINTER(c_uint8), c_size_t]),
    "pt_create": (c_int, [c_int, c_uint32, c_uint32, POINTER(_ctx)]),
    "pt_resize_clear": (c_int, [_ctx, c_uint32, c_uint32]),
    "pt_set_program": (c_int, [_ctx, POINTER(Op), c_uint32, POINTER(Aabb), c_uint32, c_uint32]),
    "pt_set_data": (c_int, [_ctx, _f32p, c_uint32]),
    "pt_set_tiles": (c_int, [_ctx, c_uint32, c_uint32]),
    "pt_set_camera": (c_int, [_ctx, POINTER(Camera)]),
    "pt_get_camera": (c_int, [_ctx, POINTER(Camera), POINTER(c_int)]),
    "pt_set_sky": (c_int, [_ctx, POINTER(Sky)]),
    "pt_get_sky": (c_int, [_ctx, POINTER(Sky), POINTER(c_int)]),
    "pt_dispatch": (c_int, [_ctx, POINTER(Constants), POINTER(Settings), c_uint32]),
    "pt_read_accum": (c_int, [_ctx, _f32p, c_size_t]),
    "pt_accum_device_ptr": (c_int, [_ctx, POINTER(c_void_p), POINTER(c_size_t)]),
    "pt_get_size": (c_int, [_ctx, _u32p, _u32p]),
    "pt_comm_get_unique_id": (c_int, [POINTER(c_uint8)]),
    "pt_comm_init": (c_int, [_ctx, c_uint32, c_uint32, POINTER(c_uint8)]),
    "pt_comm_size": (c_int, [_ctx, _u32p]),
    "pt_reduce_accum": (c_int, [_ctx, c_int]),
    "pt_read_reduced": (c_int, [_ctx, _f32p, c_size_t]),
    "pt_sync": (c_int, [_ctx]),
    "pt_last_dispatch_ms": (c_int, [_ctx, _f32p]),
    "pt_dispatch_stats": (c_int, [_ctx, POINTER(Constants), POINTER(Settings), c_uint32, POINTER(c_uint64)]),
    "pt_set_option": (c_int, [_ctx, c_char_p, c_int]),
    "pt_get_option": (c_int, [_ctx, c_char_p, POINTER(ctypes.c_double)]),
    "pt_jit_log": (c_char_p, [_ctx]),
    "pt_jit_compile": (c_int, [POINTER(Op), c_uint32, POINTER(Aabb), c_uint32, _f32p, c_uint32, c_char_p,
                               c_size_t, POINTER(c_size_t)]),
    "pt_scene_kernel_source": (c_int, [POINTER(Op), c_uint32, POINTER(Aabb), c_uint32, _f32p, c_uint32,
                                       c_int, c_char_p, c_size_t, POINTER(c_size_t)]),
    "pt_last_error": (c_char_p, [_ctx]),
    "pt_destroy": (None, [_ctx]),
    "pt_abi_version": (c_int, []),
    "pt_device_math": (c_int, [c_int, c_int, _f32p, _f32p, _f32p, c_uint32]),
    "pt_check_sqrt_exhaustive": (c_int, [c_int, POINTER(c_uint64), POINTER(c_uint32)]),
    "pt_check_div_exhaustive": (c_int, [c_int, c_uint32, c_uint32, c_uint32, c_uint32, POINTER(c_uint64),
                                        POINTER(c_uint64)]),
    "pt_check_div_random": (c_int, [c_int, c_uint32, c_uint32, POINTER(c_uint64), POINTER(c_uint64)]),
    "pt_check_box_random": (c_int, [c_int, c_uint32, c_uint32, c_int, POINTER(c_uint64)]),
    "pt_check_div_k": (c_int, [c_int, c_float, c_uint32, c_uint32, POINTER(c_uint64), POINTER(c_uint64)]),
    "pt_traffic_probe": (c_int, [c_int, c_uint32, _f32p, POINTER(c_uint64)]),
    "pt_display": (c_int, [c_void_p, c_int, c_void_p, c_size_t]),
    "pt_write_accum": (c_int, [c_void_p, _f32p, c_size_t]),
    "pt_render_guides": (c_int, [_ctx, POINTER(Constants), POINTER(Settings)]),
    "pt_read_guides": (c_int, [_ctx, _f32p, _f32p, c_size_t]),
    "pt_denoise": (c_int, [_ctx, POINTER(DenoiseParams), c_int, c_void_p, c_size_t]),
    "pt_read_moments": (c_int, [_ctx, _f32p, c_size_t]),
    "pt_write_moments": (c_int, [_ctx, _f32p, c_size_t, c_uint32]),
    "pt_read_variance": (c_int, [_ctx, _f32p, c_size_t]),
    "pt_denoise_guided": (c_int, [_ctx, POINTER(GuidedParams), c_int, c_void_p, c_size_t]),
    "pt_temporal_accumulate": (c_int, [_ctx, POINTER(TemporalParams)]),
    "pt_temporal_reset": (c_int, [_ctx]),
    "pt_read_history": (c_int, [_ctx, _f32p, _f32p, _f32p, c_size_t]),
    "pt_denoise_history": (c_int, [_ctx, POINTER(GuidedParams), c_int, c_void_p, c_size_t]),
    "pt_sample_field": (c_int, [_ctx, _f32p, c_uint32, _f32p, POINTER(c_int32)]),
    "pt_mesh_extract": (c_int, [_ctx, POINTER(MeshDesc), POINTER(MeshInfo)]),
    "pt_mesh_read": (c_int, [_ctx, _f32p, _f32p, POINTER(c_int32), _u32p, c_size_t, c_size_t]),
    "pt_trace_rays": (c_int, [_ctx, _f32p, _f32p, c_uint32, _f32p, POINTER(c_int32), _f32p]),
    "pt_pick_pixels": (c_int, [_ctx, POINTER(Constants), POINTER(Settings), POINTER(c_int32), c_uint32, _f32p,
                               POINTER(c_int32), _f32p]),
    "pt_trace_radiance": (c_int, [_ctx, _f32p, _f32p, c_uint32, POINTER(RadianceParams), _f32p, _f32p]),
    "pt_render_preview": (c_int, [_ctx, POINTER(Constants), POINTER(Settings), POINTER(PreviewParams), c_int, c_void_p,
                                  c_size_t]),
    "pt_probe_map": (c_int, [_ctx, c_int, c_int, c_uint32, _f32p, _u64p, _f32p, _u64p, c_int, _f32p, POINTER(c_int32),
                             _u64p, _u64p]),
    "pt_probe_taps": (c_int, [_ctx, c_int, c_uint32, _f32p, _u64p, _f32p, _f32p, POINTER(c_int32), _u64p, _u64p]),
    "pt_probe_bounds": (c_int, [_ctx, c_int, c_uint32, _f32p, _f32p, c_int, _u32p, _u64p, _u64p]),
    "pt_probe_kernel_source": (c_int, [POINTER(Op), c_uint32, POINTER(Aabb), c_uint32, _f32p, c_uint32,
                                       c_int, c_char_p, c_size_t, POINTER(c_size_t)]),
    "pt_probe_jit_compile": (c_int, [POINTER(Op), c_uint32, POINTER(Aabb), c_uint32, _f32p, c_uint32, c_int, c_char_p,
                                     c_size_t, POINTER(c_size_t)]),
}
SYMBOLS = tuple(SIGNATURES)


class NativeError(RuntimeError):
    def __init__(self, fn: str, code: int, msg: str):
        super().__init__(f"{fn} failed ({code}): {msg}")
        self.code = code


_lib = None


def lib() -> ctypes.CDLL:
    """Load ``libpt.so`` (the HIP build).  Raises if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("PT_LIB") or LIB_PATH  # PT_LIB: an in-tree A/B variant (build.build_variant)
    if not os.path.exists(path):
        raise ImportError(f"HIP library {path} missing: run __graft_entry__.build() (no CPU fallback exists)")
    L = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        if os.environ.get("PT_LIB") and not hasattr(L, name):
            continue  # an older A/B variant may predate a self-test entry point
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def ptr(array, ctype):
    """A numpy array's data as a ``ctype`` pointer (the array must outlive the call)."""
    return array.ctypes.data_as(POINTER(ctype))


def fptr(array):
    return ptr(array, c_float)


def scene_kernel_source(prog, data=None, baked: int = 0, entry: str = "pt_scene_kernel_source") -> str:
    """The scene-kernel source generated for ``prog`` with ``data`` (default:
    the program's own values), not compiled: ``pt_scene_kernel_source``'s
    two-call pattern."""
    import numpy as np

    d = np.ascontiguousarray(prog.data if data is None else data, np.float32)
    args = (prog.ops, prog.n_ops, prog.aabbs, prog.n_aabb, fptr(d), len(d), int(baked))
    n = c_size_t()
    fn = getattr(lib(), entry)
    assert fn(*args, None, 0, ctypes.byref(n)) == PT_OK
    buf = ctypes.create_string_buffer(n.value)
    assert fn(*args, buf, n.value, ctypes.byref(n)) == PT_OK
    return buf.value.decode()


def probe_kernel_source(prog, data=None, baked: int = 0) -> str:
    """The probe module's source (``pt_probe_kernel_source``): the scene-kernel
    source up to its kernel list, then the probe kernels."""
    return scene_kernel_source(prog, data, baked, entry="pt_probe_kernel_source")


def check(fn: str, rc: int, ctx=None) -> None:
    if rc != PT_OK:
        msg = ""
        if ctx is not None:
            raw = lib().pt_last_error(ctx)
            msg = raw.decode() if raw else ""
        raise NativeError(fn, rc, msg)
