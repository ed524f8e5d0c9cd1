"""The denoiser at the C boundary without a GPU: pt_denoise_params' layout
from a C11 compile (tests/abi_denoise_layout.c, the flags of test_abi_sky.py),
the ctypes mirror, and the null-context errors."""
import ctypes
import os
import subprocess

import numpy as np

from compute_path_tracer_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_denoise_layout_compiles_as_c11(tmp_path):
    cmd = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
           os.path.join(ROOT, "tests", "abi_denoise_layout.c"), "-o", str(tmp_path / "abi_denoise_layout.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_ctypes_params_match_the_header_layout():
    P = N.DenoiseParams
    assert ctypes.sizeof(P) == 20
    offs = {name: (getattr(P, name).offset, getattr(P, name).size) for name, _ in P._fields_}
    assert offs == {"iterations": (0, 4), "normal_power_log2": (4, 4), "sigma_color": (8, 4), "sigma_depth": (12, 4),
                    "sigma_albedo": (16, 4)}
    assert (N.PT_DISPLAY_RGBA32F, N.PT_DISPLAY_SRGB8, N.PT_DENOISE_LINEAR) == (0, 1, 2)


def test_denoise_symbols_are_checked_by_the_build():
    assert {"pt_render_guides", "pt_read_guides", "pt_denoise"} <= set(N.SYMBOLS)


def test_denoise_entry_points_reject_a_null_context():
    L = N.lib()
    k = N.Constants(time=0.0, frame=1, aspect=1.5, last_clear=1)
    s = N.Settings(debug=0, bounces=4, scale=1.0, fov=1.0, aabb=0)
    p = N.DenoiseParams(iterations=5, normal_power_log2=5, sigma_color=4.0, sigma_depth=0.05, sigma_albedo=0.1)
    g0 = np.full(16, 7.0, np.float32)
    g1 = np.full(16, 9.0, np.float32)
    out = np.full(16, 5.0, np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    assert L.pt_render_guides(None, ctypes.byref(k), ctypes.byref(s)) == N.PT_ERR_INVALID
    assert L.pt_render_guides(None, None, None) == N.PT_ERR_INVALID
    assert L.pt_read_guides(None, g0.ctypes.data_as(fp), g1.ctypes.data_as(fp), g0.nbytes) == N.PT_ERR_INVALID
    for fmt in (N.PT_DENOISE_LINEAR, N.PT_DISPLAY_RGBA32F, N.PT_DISPLAY_SRGB8):
        assert L.pt_denoise(None, ctypes.byref(p), fmt, out.ctypes.data_as(ctypes.c_void_p), out.nbytes) == \
            N.PT_ERR_INVALID
    assert L.pt_denoise(None, None, N.PT_DENOISE_LINEAR, None, 0) == N.PT_ERR_INVALID
    assert (g0 == 7.0).all() and (g1 == 9.0).all() and (out == 5.0).all()  # outputs left untouched
