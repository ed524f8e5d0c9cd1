"""The preview shading at the C boundary, without a GPU: the
symbol and its signature, the parameter structure field by field against the
header's text, the define against its mirror, the ABI version, and the refusal
that needs no context."""
import ctypes
import os
import re

import numpy as np

from compute_path_tracer_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"float": ctypes.c_float, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32}


def _raw():
    with open(os.path.join(ROOT, "include", "pt_abi.h")) as f:
        return f.read()


def _header():
    return re.sub(r"/\*.*?\*/", "", _raw(), flags=re.S)


def test_symbol_exists_with_its_signature():
    assert "pt_render_preview" in N.SYMBOLS
    fn = N.lib().pt_render_preview
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == N.SIGNATURES["pt_render_preview"][1] == [
        ctypes.c_void_p, ctypes.POINTER(N.Constants), ctypes.POINTER(N.Settings), ctypes.POINTER(N.PreviewParams),
        ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]


def test_the_header_declares_it_once_and_the_version_stays():
    text = _header()
    assert re.search(r"int pt_render_preview\(pt_ctx \*ctx, const pt_constants \*c, const pt_settings \*s,\s*"
                     r"const pt_preview_params \*p,\s*int format, void \*out, size_t bytes\);", text)
    assert text.count("pt_render_preview(") == 1  # the declaration, nothing else outside the comments
    assert re.search(r"#define PT_ABI_VERSION 1\b", text)
    assert N.lib().pt_abi_version() == 1
    assert '"preview_ms"' in _raw()  # the option comment names the new key


def test_the_structure_equals_its_mirror():
    m = re.search(r"typedef struct pt_preview_params\s*\{([^}]*)\}\s*pt_preview_params\s*;", _header())
    assert m  # (tagged, as pt_guided_params: test_abi_mirror.py counts the untagged ones)
    fields = []
    for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
        dm = re.fullmatch(r"(\w+)\s+(.+)", decl, flags=re.S)
        assert dm and dm.group(1) in SCALARS, decl
        for d in dm.group(2).split(","):
            am = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", d.strip())
            assert am, decl
            fields.append((am.group(1), SCALARS[dm.group(1)], int(am.group(2)) if am.group(2) else None))
    mirror = [(name, t._type_, t._length_) if issubclass(t, ctypes.Array) else (name, t, None)
              for name, t in N.PreviewParams._fields_]
    assert mirror == fields
    assert [f[0] for f in fields] == ["light_dir", "light_color", "ambient_bottom", "ambient_top", "shadow_steps",
                                      "shadow_k", "shadow_cull", "ao_strength", "ao_radius", "highlight",
                                      "highlight_color", "highlight_mix"]
    assert ctypes.sizeof(N.PreviewParams) == 88
    assert N.PreviewParams.shadow_steps.offset == 48 and N.PreviewParams.highlight_mix.offset == 84


def test_the_define_equals_its_mirror():
    defines = dict(re.findall(r"^#define (PT_PREVIEW_\w+)[ \t]+(\d+)[ \t]*$", _header(), flags=re.M))
    assert {k: int(v) for k, v in defines.items()} == {"PT_PREVIEW_MAX_SHADOW_STEPS": 64}
    assert N.PT_PREVIEW_MAX_SHADOW_STEPS == 64


def test_a_null_context_is_refused():
    L = N.lib()
    out = np.full((4, 4, 4), 7.0, np.float32)
    c, s = N.Constants(0.0, 1, 1.0, 1), N.Settings(0, 2, 1.0, 1.0, 0)
    p = N.PreviewParams(shadow_steps=8, shadow_k=2.0, ao_strength=1.0, ao_radius=0.5, highlight=-1)
    p.light_dir[1] = 1.0
    assert L.pt_render_preview(None, ctypes.byref(c), ctypes.byref(s), ctypes.byref(p), N.PT_DENOISE_LINEAR,
                               out.ctypes.data_as(ctypes.c_void_p), out.nbytes) == N.PT_ERR_INVALID
    assert L.pt_render_preview(None, None, None, None, 0, None, 0) == N.PT_ERR_INVALID
    assert (out == 7.0).all()  # the output left untouched
