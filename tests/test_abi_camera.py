"""pt_camera at the C boundary without a GPU: the struct's layout from a C11
compile (tests/abi_camera_layout.c, the flags of test_abi_harness.py), the
ctypes mirror, and the null-context errors."""
import ctypes
import os
import subprocess

from compute_path_tracer_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_camera_layout_compiles_as_c11(tmp_path):
    cmd = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
           os.path.join(ROOT, "tests", "abi_camera_layout.c"), "-o", str(tmp_path / "abi_camera_layout.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_ctypes_camera_matches_the_header_layout():
    assert ctypes.sizeof(N.Camera) == 56
    offs = {name: (getattr(N.Camera, name).offset, getattr(N.Camera, name).size) for name, _ in N.Camera._fields_}
    assert offs == {"origin": (0, 12), "right": (12, 12), "up": (24, 12), "forward": (36, 12), "aperture": (48, 4),
                    "focus": (52, 4)}


def test_camera_entry_points_reject_a_null_context():
    L = N.lib()
    cam = N.Camera()
    dflt = ctypes.c_int(-1)
    assert L.pt_set_camera(None, ctypes.byref(cam)) == N.PT_ERR_INVALID
    assert L.pt_set_camera(None, None) == N.PT_ERR_INVALID
    assert L.pt_get_camera(None, ctypes.byref(cam), ctypes.byref(dflt)) == N.PT_ERR_INVALID
    assert dflt.value == -1
