"""Mesh export at the C boundary without a GPU: the layouts of pt_mesh_desc and
pt_mesh_info from a C11 compile (tests/abi_mesh_layout.c, the flags of
test_abi_sky.py), the ctypes mirrors, the symbols, and the argument errors a
null context can reach (test_gpu_mesh.py repeats them on a live one)."""
import ctypes
import os
import subprocess

import numpy as np

from compute_path_tracer_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP, IP, UP = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)


def test_mesh_layout_compiles_as_c11(tmp_path):
    cmd = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
           os.path.join(ROOT, "tests", "abi_mesh_layout.c"), "-o", str(tmp_path / "abi_mesh_layout.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def _layout(S):
    return {name: (getattr(S, name).offset, getattr(S, name).size) for name, _ in S._fields_}


def test_ctypes_mirrors_match_the_header_layout():
    assert ctypes.sizeof(N.MeshDesc) == 36 and ctypes.sizeof(N.MeshInfo) == 48
    assert _layout(N.MeshDesc) == {"origin": (0, 12), "cell": (12, 4), "cells": (16, 12), "iso": (28, 4),
                                   "project": (32, 4)}
    assert _layout(N.MeshInfo) == {"n_vertices": (0, 4), "n_triangles": (4, 4), "clipped_edges": (8, 4),
                                   "void_cells": (12, 4), "dropped_quads": (16, 4), "bricks": (20, 4),
                                   "bricks_evaluated": (24, 4), "reserved": (28, 4), "corner_evals": (32, 8),
                                   "device_bytes": (40, 8)}
    assert (N.PT_MESH_BRICK, N.PT_MESH_MAX_CELLS, N.PT_MESH_MAX_PROJECT) == (8, 1024, 8)


def test_mesh_symbols_are_checked_by_the_build():
    assert {"pt_sample_field", "pt_mesh_extract", "pt_mesh_read"} <= set(N.SYMBOLS)
    L = N.lib()
    for name in ("pt_sample_field", "pt_mesh_extract", "pt_mesh_read"):
        assert getattr(L, name).restype is ctypes.c_int
    assert L.pt_abi_version() == 1  # additive: the version stays


def desc(**kw):
    d = N.MeshDesc(cell=0.25, iso=0.0, project=2)
    for k in range(3):
        d.origin[k], d.cells[k] = -2.0, 16
    for name, v in kw.items():
        if name in ("origin", "cells"):
            for k in range(3):
                getattr(d, name)[k] = v[k]
        else:
            setattr(d, name, v)
    return d


NAN, INF = float("nan"), float("inf")
# every description pt_mesh_extract refuses with PT_ERR_INVALID
BAD_DESCS = {
    "nan origin": dict(origin=(NAN, 0.0, 0.0)), "inf origin": dict(origin=(0.0, 0.0, -INF)),
    "nan cell": dict(cell=NAN), "inf cell": dict(cell=INF), "zero cell": dict(cell=0.0), "negative cell": dict(cell=-0.25),
    "nan iso": dict(iso=NAN), "inf iso": dict(iso=INF),
    "zero cells": dict(cells=(16, 0, 16)), "too many cells": dict(cells=(16, 16, 1025)),
    "project 9": dict(project=9),
}


def test_mesh_entry_points_reject_a_null_context_and_leave_outputs_untouched():
    L = N.lib()
    pts = np.zeros((4, 3), np.float32)
    d, s = np.full(4, 7.0, np.float32), np.full(4, 9, np.int32)
    assert L.pt_sample_field(None, pts.ctypes.data_as(FP), 4, d.ctypes.data_as(FP), s.ctypes.data_as(IP)) == \
        N.PT_ERR_INVALID
    assert L.pt_sample_field(None, None, 0, None, None) == N.PT_ERR_INVALID
    info = N.MeshInfo(n_vertices=11, n_triangles=12, corner_evals=13, device_bytes=14)
    before = bytes(info)
    assert L.pt_mesh_extract(None, ctypes.byref(desc()), ctypes.byref(info)) == N.PT_ERR_INVALID
    assert L.pt_mesh_extract(None, None, ctypes.byref(info)) == N.PT_ERR_INVALID
    assert L.pt_mesh_extract(None, ctypes.byref(desc()), None) == N.PT_ERR_INVALID
    for label, kw in BAD_DESCS.items():
        assert L.pt_mesh_extract(None, ctypes.byref(desc(**kw)), ctypes.byref(info)) == N.PT_ERR_INVALID, label
    pos, nrm = np.full((4, 3), 7.0, np.float32), np.full((4, 3), 8.0, np.float32)
    tri = np.full((4, 3), 5, np.uint32)
    assert L.pt_mesh_read(None, pos.ctypes.data_as(FP), nrm.ctypes.data_as(FP), s.ctypes.data_as(IP),
                          tri.ctypes.data_as(UP), 4, 4) == N.PT_ERR_INVALID
    assert L.pt_mesh_read(None, None, None, None, None, 0, 0) == N.PT_ERR_INVALID
    assert bytes(info) == before
    assert (d == 7.0).all() and (s == 9).all() and (pos == 7.0).all() and (nrm == 8.0).all() and (tri == 5).all()
    assert L.pt_last_error(None) == b"null context"
