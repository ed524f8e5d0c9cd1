"""The radiance query at the C boundary, without a GPU: the
symbol and its signature, the parameter structure's size and fields, the
defines against their mirror, the ABI version, and the refusals that need no
context."""
import ctypes
import os
import re

import numpy as np

from compute_path_tracer_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _raw():
    with open(os.path.join(ROOT, "include", "pt_abi.h")) as f:
        return f.read()


def _header():
    return re.sub(r"/\*.*?\*/", "", _raw(), flags=re.S)


def test_symbol_exists_with_its_signature():
    assert "pt_trace_radiance" in N.SYMBOLS
    fn = N.lib().pt_trace_radiance
    fp = ctypes.POINTER(ctypes.c_float)
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == N.SIGNATURES["pt_trace_radiance"][1] == [
        ctypes.c_void_p, fp, fp, ctypes.c_uint32, ctypes.POINTER(N.RadianceParams), fp, fp]


def test_the_header_declares_it_and_the_version_stays():
    text = _header()
    assert re.search(r"int pt_trace_radiance\(pt_ctx \*ctx, const float \*ro, const float \*rd, uint32_t n,\s*"
                     r"const pt_radiance_params \*p,\s*float \*mean,\s*float \*moment\);", text)
    assert re.search(r"#define PT_ABI_VERSION 1\b", text)
    assert N.lib().pt_abi_version() == 1
    for key in ("radiance_samples", "radiance_ms", "radiance_first_ms", "radiance_bytes"):
        assert f'"{key}"' in _raw(), key  # the option comments name the new keys


def test_the_structure_equals_its_mirror():
    m = re.search(r"typedef struct pt_radiance_params\s*\{([^}]*)\}\s*pt_radiance_params\s*;", _header())
    assert m
    fields = re.findall(r"(uint32_t|int32_t)\s+(\w+)\s*;", m.group(1))
    ctype = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32}
    assert [(name, ctype[t]) for t, name in fields] == list(N.RadianceParams._fields_)
    assert [name for _, name in fields] == ["spp", "sample0", "seed", "bounces", "mode"]
    assert ctypes.sizeof(N.RadianceParams) == 20


def test_defines_equal_their_mirror():
    defines = dict(re.findall(r"^#define (PT_RADIANCE_\w+)[ \t]+(\d+)[ \t]*$", _header(), flags=re.M))
    assert {k: int(v) for k, v in defines.items()} == {"PT_RADIANCE_RAY": 0, "PT_RADIANCE_HEMISPHERE": 1,
                                                       "PT_RADIANCE_MAX_SPP": 65536}
    assert (N.PT_RADIANCE_RAY, N.PT_RADIANCE_HEMISPHERE, N.PT_RADIANCE_MAX_SPP) == (0, 1, 65536)


def test_a_null_context_is_refused():
    L = N.lib()
    rays = np.zeros((2, 3), np.float32)
    rays[:, 2] = 1.0
    mean, moment = np.full((2, 3), 5.0, np.float32), np.full((2, 3), 9.0, np.float32)
    p = N.RadianceParams(spp=4, sample0=0, seed=1, bounces=2, mode=N.PT_RADIANCE_RAY)
    assert L.pt_trace_radiance(None, N.fptr(rays), N.fptr(rays), 2, ctypes.byref(p), N.fptr(mean),
                               N.fptr(moment)) == N.PT_ERR_INVALID
    assert L.pt_trace_radiance(None, None, None, 0, None, None, None) == N.PT_ERR_INVALID
    assert (mean == 5.0).all() and (moment == 9.0).all()  # outputs left untouched
