"""pt_sky at the C boundary without a GPU: the struct's layout from a C11
compile (tests/abi_sky_layout.c, the flags of test_abi_camera.py), the ctypes
mirror, and the null-context errors."""
import ctypes
import os
import subprocess

from compute_path_tracer_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sky_layout_compiles_as_c11(tmp_path):
    cmd = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
           os.path.join(ROOT, "tests", "abi_sky_layout.c"), "-o", str(tmp_path / "abi_sky_layout.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_ctypes_sky_matches_the_header_layout():
    assert ctypes.sizeof(N.Sky) == 52
    offs = {name: (getattr(N.Sky, name).offset, getattr(N.Sky, name).size) for name, _ in N.Sky._fields_}
    assert offs == {"bottom": (0, 12), "top": (12, 12), "sun_dir": (24, 12), "sun_color": (36, 12), "sun_cos": (48, 4)}


def test_sky_symbols_are_checked_by_the_build():
    assert "pt_set_sky" in N.SYMBOLS and "pt_get_sky" in N.SYMBOLS


def test_sky_entry_points_reject_a_null_context():
    L = N.lib()
    sky = N.Sky(sun_cos=0.25)
    sky.top[1] = 0.5
    before = bytes(sky)
    off = ctypes.c_int(-1)
    assert L.pt_set_sky(None, ctypes.byref(sky)) == N.PT_ERR_INVALID
    assert L.pt_set_sky(None, None) == N.PT_ERR_INVALID
    assert L.pt_get_sky(None, ctypes.byref(sky), ctypes.byref(off)) == N.PT_ERR_INVALID
    assert off.value == -1 and bytes(sky) == before  # outputs left untouched
