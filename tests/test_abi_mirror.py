"""The ctypes mirror in _native.py is include/pt_abi.h: its constants, its
eleven structures field by field, and the names of its signature table, read
from the header's text.  No library and no GPU."""
import ctypes
import os
import re

import pytest

from compute_path_tracer_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {
    "pt_constants": N.Constants, "pt_settings": N.Settings, "pt_scene_node": N.SceneNode, "pt_op": N.Op,
    "pt_aabb": N.Aabb, "pt_float_key": N.FloatKey, "pt_camera": N.Camera, "pt_sky": N.Sky,
    "pt_denoise_params": N.DenoiseParams, "pt_mesh_desc": N.MeshDesc, "pt_mesh_info": N.MeshInfo,
}
SCALARS = {"float": ctypes.c_float, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64}
NOT_IN_THE_HEADER = {"PT_ST_COUNT"}  # the device counters' enum, csrc/pt_device.h


def header() -> str:
    with open(os.path.join(ROOT, "include", "pt_abi.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def header_defines() -> dict:
    return {name: int(val) for name, val in re.findall(r"^#define (PT_\w+)[ \t]+(-?\d+)[ \t]*$", header(), flags=re.M)}


def parse_fields(body: str) -> list:
    """[(name, scalar ctype, array length or None)] of a struct body; one
    declaration may hold several declarators (``uint64_t lo, hi;``)."""
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(\w+)\s+(.+)", decl, flags=re.S)
        assert m and m.group(1) in SCALARS, decl
        for d in m.group(2).split(","):
            dm = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", d.strip())
            assert dm, decl
            fields.append((dm.group(1), SCALARS[m.group(1)], int(dm.group(2)) if dm.group(2) else None))
    return fields


def header_structs() -> dict:
    return {name: parse_fields(body) for body, name in re.findall(r"typedef struct\s*\{([^}]*)\}\s*(\w+)\s*;", header())}


def mirror_fields(cls) -> list:
    return [(name, t._type_, t._length_) if issubclass(t, ctypes.Array) else (name, t, None) for name, t in cls._fields_]


def test_parser_reads_declarator_lists():
    assert parse_fields("uint64_t lo, hi;") == [("lo", ctypes.c_uint64, None), ("hi", ctypes.c_uint64, None)]
    assert parse_fields("float origin[3];\n float right[3], up[3];\n int32_t n;") == [
        ("origin", ctypes.c_float, 3), ("right", ctypes.c_float, 3), ("up", ctypes.c_float, 3), ("n", ctypes.c_int32, None)]


def test_defines():
    defines = header_defines()
    assert len(defines) >= 46 and defines["PT_ERR_SIZE"] == -6 and defines["PT_NODE_FLOATS"] == 29
    mirrored = {k: v for k, v in vars(N).items() if k.startswith("PT_") and isinstance(v, int)}
    assert len(mirrored) >= 41
    assert (defines["PT_PROBE_INTERP"], defines["PT_PROBE_TABLE"], defines["PT_PROBE_BAKED"]) == (0, 1, 2)
    assert (defines["PT_PROBE_MAP"], defines["PT_PROBE_MAP_B0"], defines["PT_PROBE_MAP_B1"]) == (0, 1, 2)
    for name, val in defines.items():
        if name in mirrored:
            assert mirrored[name] == val, name
    assert set(mirrored) - set(defines) == NOT_IN_THE_HEADER
    assert N.PT_MATH == {k[len("PT_MATH_"):].lower(): v for k, v in defines.items() if k.startswith("PT_MATH_")}
    assert len(N.PT_MATH) == 8
    assert len(N.STAT_NAMES) == N.PT_STAT_COUNT == defines["PT_STAT_COUNT"]


def test_every_header_struct_has_a_mirror():
    assert set(header_structs()) == set(STRUCTS) and len(STRUCTS) == 11


@pytest.mark.parametrize("name", list(STRUCTS))
def test_struct_fields(name):
    want = header_structs()[name]
    assert len(want) >= 2
    assert mirror_fields(STRUCTS[name]) == want


def test_signature_table_names_the_declared_functions():
    declared = set(re.findall(r"\b(pt_[a-z0-9_]+)\s*\(", header()))
    assert len(declared) >= 56
    assert {"pt_probe_map", "pt_probe_taps", "pt_probe_bounds", "pt_probe_kernel_source", "pt_probe_jit_compile"} <= declared
    assert set(N.SIGNATURES) == declared
    assert N.SYMBOLS == tuple(N.SIGNATURES)
    for name, (restype, argtypes) in N.SIGNATURES.items():
        assert isinstance(argtypes, (list, tuple)), name
