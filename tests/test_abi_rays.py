"""The ray queries at the C boundary, without a GPU: the two
symbols and their signatures, PT_RAYS_MAX against its mirror, the ABI version,
and the null-context refusals."""
import ctypes
import os
import re

import numpy as np

from compute_path_tracer_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "pt_abi.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_symbols_exist_with_their_signatures():
    assert {"pt_trace_rays", "pt_pick_pixels"} <= set(N.SYMBOLS)
    L = N.lib()
    for name in ("pt_trace_rays", "pt_pick_pixels"):
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int, name
        assert list(fn.argtypes) == list(N.SIGNATURES[name][1]), name
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    assert N.SIGNATURES["pt_trace_rays"][1] == [ctypes.c_void_p, fp, fp, ctypes.c_uint32, fp, ip, fp]
    assert N.SIGNATURES["pt_pick_pixels"][1] == [ctypes.c_void_p, ctypes.POINTER(N.Constants), ctypes.POINTER(N.Settings),
                                                 ip, ctypes.c_uint32, fp, ip, fp]


def test_the_header_declares_them_and_the_version_stays():
    text = _header()
    assert re.search(r"int pt_trace_rays\(pt_ctx \*ctx, const float \*ro, const float \*rd, uint32_t n,\s*float \*t, "
                     r"int32_t \*shape, float \*normal\);", text)
    assert re.search(r"int pt_pick_pixels\(pt_ctx \*ctx, const pt_constants \*c, const pt_settings \*s,\s*"
                     r"const int32_t \*xy, uint32_t n,\s*float \*t,\s*int32_t \*shape, float \*normal\);", text)
    assert re.search(r"#define PT_ABI_VERSION 1\b", text)
    assert N.lib().pt_abi_version() == 1


def test_rays_max_equals_its_mirror():
    m = re.search(r"^#define PT_RAYS_MAX[ \t]+(\d+)[ \t]*$", _header(), flags=re.M)
    assert m and int(m.group(1)) == N.PT_RAYS_MAX == 1 << 26


def test_entry_points_reject_a_null_context():
    L = N.lib()
    rays = np.zeros((2, 3), np.float32)
    rays[:, 2] = 1.0
    t, shape, nrm = np.full(2, 5.0, np.float32), np.full(2, 7, np.int32), np.full((2, 3), 9.0, np.float32)
    xy = np.zeros((2, 2), np.int32)
    k, s = N.Constants(0.0, 1, 1.0, 1), N.Settings(0, 2, 1.0, 1.0, 0)
    out = (N.fptr(t), N.ptr(shape, ctypes.c_int32), N.fptr(nrm))
    assert L.pt_trace_rays(None, N.fptr(rays), N.fptr(rays), 2, *out) == N.PT_ERR_INVALID
    assert L.pt_trace_rays(None, None, None, 0, None, None, None) == N.PT_ERR_INVALID
    assert L.pt_pick_pixels(None, ctypes.byref(k), ctypes.byref(s), N.ptr(xy, ctypes.c_int32), 2, *out) == N.PT_ERR_INVALID
    assert L.pt_pick_pixels(None, ctypes.byref(k), ctypes.byref(s), None, 0, None, None, None) == N.PT_ERR_INVALID
    assert (t == 5.0).all() and (shape == 7).all() and (nrm == 9.0).all()  # outputs left untouched
