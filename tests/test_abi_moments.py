"""The second moments and the guided filter at the C boundary without a GPU:
pt_guided_params' layout from a C11 compile (tests/abi_moments_layout.c, the
flags of test_abi_denoise.py), the ctypes mirror against the header's text
(the struct carries a tag, so test_abi_mirror.py's list of untagged structs
does not hold it: it is read here), and the null-context errors."""
import ctypes
import os
import re
import subprocess

import numpy as np

from compute_path_tracer_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"float": ctypes.c_float, "uint32_t": ctypes.c_uint32}


def test_moments_layout_compiles_as_c11(tmp_path):
    cmd = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
           os.path.join(ROOT, "tests", "abi_moments_layout.c"), "-o", str(tmp_path / "abi_moments_layout.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_ctypes_params_match_the_header():
    P = N.GuidedParams
    assert ctypes.sizeof(P) == 20
    offs = {name: (getattr(P, name).offset, getattr(P, name).size) for name, _ in P._fields_}
    assert offs == {"iterations": (0, 4), "normal_power_log2": (4, 4), "sigma_variance": (8, 4), "sigma_depth": (12, 4),
                    "sigma_albedo": (16, 4)}
    with open(os.path.join(ROOT, "include", "pt_abi.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"typedef struct pt_guided_params\s*\{([^}]*)\}\s*pt_guided_params\s*;", text)
    assert m, "pt_guided_params is not declared"
    fields = [re.fullmatch(r"(\w+)\s+(\w+)", d.strip()).groups() for d in m.group(1).split(";") if d.strip()]
    assert [(name, SCALARS[t]) for t, name in fields] == list(P._fields_)
    # only the differing field's name tells the two filters' blocks apart
    assert [t for _n, t in P._fields_] == [t for _n, t in N.DenoiseParams._fields_]


def test_symbols_are_checked_by_the_build():
    assert {"pt_read_moments", "pt_write_moments", "pt_read_variance", "pt_denoise_guided"} <= set(N.SYMBOLS)
    assert N.SIGNATURES["pt_write_moments"][1][-1] is ctypes.c_uint32


def test_entry_points_reject_a_null_context():
    L = N.lib()
    p = N.GuidedParams(iterations=5, normal_power_log2=5, sigma_variance=2.0, sigma_depth=0.05, sigma_albedo=0.1)
    buf = np.full(16, 5.0, np.float32)
    fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert L.pt_read_moments(None, fp, buf.nbytes) == N.PT_ERR_INVALID
    assert L.pt_write_moments(None, fp, buf.nbytes, 4) == N.PT_ERR_INVALID
    assert L.pt_read_variance(None, fp, buf.nbytes) == N.PT_ERR_INVALID
    for fmt in (N.PT_DENOISE_LINEAR, N.PT_DISPLAY_RGBA32F, N.PT_DISPLAY_SRGB8):
        assert L.pt_denoise_guided(None, ctypes.byref(p), fmt, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes) == \
            N.PT_ERR_INVALID
    assert L.pt_denoise_guided(None, None, N.PT_DENOISE_LINEAR, None, 0) == N.PT_ERR_INVALID
    assert (buf == 5.0).all()  # outputs left untouched
