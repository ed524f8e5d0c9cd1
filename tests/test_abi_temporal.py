"""Temporal accumulation at the C boundary: pt_temporal_params' layout from a
C11 compile (tests/abi_temporal_layout.c, the flags of test_abi_denoise.py),
the ctypes mirror against the header's text (the struct carries a tag, so
test_abi_mirror.py's list of untagged structs does not hold it: it is read
here), the null-context errors -- all without a GPU -- and, where pt_create
finds a device (as test_abi.py asks it), the refusals, the state transitions
and which calls drop the history."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import gpuharness as G
from compute_path_tracer_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 16, 12


def test_temporal_layout_compiles_as_c11(tmp_path):
    cmd = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
           os.path.join(ROOT, "tests", "abi_temporal_layout.c"), "-o", str(tmp_path / "abi_temporal_layout.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_ctypes_params_match_the_header():
    P = N.TemporalParams
    assert ctypes.sizeof(P) == 16
    offs = {name: (getattr(P, name).offset, getattr(P, name).size) for name, _ in P._fields_}
    assert offs == {"max_history": (0, 4), "depth_tolerance": (4, 4), "normal_cos": (8, 4), "albedo_tolerance": (12, 4)}
    with open(os.path.join(ROOT, "include", "pt_abi.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"typedef struct pt_temporal_params\s*\{([^}]*)\}\s*pt_temporal_params\s*;", text)
    assert m, "pt_temporal_params is not declared"
    fields = [re.fullmatch(r"(\w+)\s+(\w+)", d.strip()).groups() for d in m.group(1).split(";") if d.strip()]
    assert [(name, {"float": ctypes.c_float}[t]) for t, name in fields] == list(P._fields_)
    assert re.search(r"#define PT_ABI_VERSION 1\b", text)


def test_symbols_are_checked_by_the_build():
    assert {"pt_temporal_accumulate", "pt_temporal_reset", "pt_read_history", "pt_denoise_history"} <= set(N.SYMBOLS)
    assert N.SIGNATURES["pt_read_history"][1][-1] is ctypes.c_size_t
    L = N.lib()
    for name in ("pt_temporal_accumulate", "pt_temporal_reset", "pt_read_history", "pt_denoise_history"):
        assert hasattr(L, name), name


def test_entry_points_reject_a_null_context():
    L = N.lib()
    p = N.TemporalParams(max_history=32.0, depth_tolerance=0.05, normal_cos=0.9, albedo_tolerance=0.1)
    g = N.GuidedParams(iterations=5, normal_power_log2=5, sigma_variance=2.0, sigma_depth=0.05, sigma_albedo=0.1)
    buf = np.full(16, 5.0, np.float32)
    fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert L.pt_temporal_accumulate(None, ctypes.byref(p)) == N.PT_ERR_INVALID
    assert L.pt_temporal_accumulate(None, None) == N.PT_ERR_INVALID
    assert L.pt_temporal_reset(None) == N.PT_ERR_INVALID
    assert L.pt_read_history(None, fp, fp, fp, buf.nbytes) == N.PT_ERR_INVALID
    for fmt in (N.PT_DENOISE_LINEAR, N.PT_DISPLAY_RGBA32F, N.PT_DISPLAY_SRGB8):
        assert L.pt_denoise_history(None, ctypes.byref(g), fmt, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes) == \
            N.PT_ERR_INVALID
    assert (buf == 5.0).all()  # outputs left untouched


def _device():
    """True where pt_create finds a device (test_abi.py's probe); without one it must say PT_ERR_HIP."""
    ctx = ctypes.c_void_p()
    rc = N.lib().pt_create(0, 8, 8, ctypes.byref(ctx))
    if rc == N.PT_OK:
        N.lib().pt_destroy(ctx)
        return True
    assert rc == N.PT_ERR_HIP and not ctx.value
    return False


def _tracer():
    return G.tracer("c2", W, H, 2, extra=dict(moments=1))


def _view(pt, frame=1, spp=2):
    pt.clear()
    pt.dispatch(G.constants(W, H, frame, 0), spp)
    pt.render_guides()


def _code(call, *args, **kwargs):
    with pytest.raises(N.NativeError) as e:
        call(*args, **kwargs)
    return e.value.code


def _state(pt):
    return pt.get_option("history_valid"), pt.get_option("history_views")


def test_refusals_leave_the_history_as_it_was():
    if not _device():
        return
    pt = _tracer()
    assert _state(pt) == (0.0, 0.0)
    assert _code(pt.read_history) == N.PT_ERR_STATE and _code(pt.denoise_history) == N.PT_ERR_STATE
    pt.reset_history()  # (nothing to drop: no error)
    # state: guides, then moments of at least two frames
    pt.dispatch(G.constants(W, H, 1, 0), 2)
    assert _code(pt.accumulate_history) == N.PT_ERR_STATE and "guides" in str(pt._L.pt_last_error(pt._ctx))
    pt.render_guides()
    pt.clear()
    pt.render_guides()
    assert _code(pt.accumulate_history) == N.PT_ERR_STATE  # no valid moments
    pt.dispatch(G.constants(W, H, 1, 0), 1)
    assert pt.get_option("moment_frames") == 1.0 and _code(pt.accumulate_history) == N.PT_ERR_STATE  # one frame: no variance
    pt.dispatch(G.constants(W, H, 2, 1), 1)
    pt.accumulate_history()
    assert _state(pt) == (1.0, 1.0)
    before = pt.read_history()
    # parameters
    for bad in (dict(max_history=-1.0), dict(max_history=float("nan")), dict(max_history=float("inf")),
                dict(depth_tolerance=-0.01), dict(depth_tolerance=float("inf")), dict(normal_cos=1.5),
                dict(normal_cos=-1.01), dict(normal_cos=float("nan")), dict(albedo_tolerance=-1.0),
                dict(albedo_tolerance=float("nan"))):
        assert _code(pt.accumulate_history, **bad) == N.PT_ERR_INVALID, bad
    assert pt._L.pt_temporal_accumulate(pt._ctx, None) == N.PT_ERR_INVALID
    # part of the image
    pt.set_tiles(0, 2)
    pt.set_option("kernel", "simple")
    pt.dispatch(G.constants(W, H, 1, 0), 2)
    assert pt.get_option("moments_valid") == 1.0 and pt.get_option("guides_valid") == 1.0
    assert _code(pt.accumulate_history) == N.PT_ERR_UNSUPPORTED
    pt.set_tiles(0, 1)
    # pt_read_history: sizes and optional outputs
    n = W * H * 16
    colour = np.zeros((H, W, 4), np.float32)
    count = np.zeros((H, W), np.float32)
    assert pt._L.pt_read_history(pt._ctx, N.fptr(colour), None, None, n - 1) == N.PT_ERR_SIZE and not colour.any()
    assert pt._L.pt_read_history(pt._ctx, None, None, None, n) == N.PT_OK
    assert pt._L.pt_read_history(pt._ctx, N.fptr(colour), None, N.fptr(count), n) == N.PT_OK
    assert np.array_equal(G.bits(colour), G.bits(before[0])) and (count == 2).all()
    # pt_denoise_history: pt_denoise_guided's refusals
    assert _code(pt.denoise_history, iterations=0) == N.PT_ERR_INVALID
    assert _code(pt.denoise_history, iterations=9) == N.PT_ERR_INVALID
    assert _code(pt.denoise_history, sigma_variance=0.0) == N.PT_ERR_INVALID
    assert _code(pt.denoise_history, sigma_depth=-1.0) == N.PT_ERR_INVALID
    assert _code(pt.denoise_history, normal_power_log2=9) == N.PT_ERR_INVALID
    g = N.GuidedParams(iterations=5, normal_power_log2=5, sigma_variance=2.0, sigma_depth=0.05, sigma_albedo=0.1)
    out = np.zeros((H, W, 4), np.float32)
    vp = out.ctypes.data_as(ctypes.c_void_p)
    assert pt._L.pt_denoise_history(pt._ctx, ctypes.byref(g), 7, vp, out.nbytes) == N.PT_ERR_INVALID
    assert pt._L.pt_denoise_history(pt._ctx, ctypes.byref(g), N.PT_DENOISE_LINEAR, vp, out.nbytes - 1) == N.PT_ERR_SIZE
    assert pt._L.pt_denoise_history(pt._ctx, None, N.PT_DENOISE_LINEAR, vp, out.nbytes) == N.PT_ERR_INVALID
    assert not out.any()
    # after all those refusals the history is what it was
    assert _state(pt) == (1.0, 1.0)
    for a, b in zip(pt.read_history(), before):
        assert np.array_equal(G.bits(a), G.bits(b))
    pt.close()


def test_what_drops_the_history_and_what_does_not():
    if not _device():
        return
    from compute_path_tracer_amd import scenes
    from compute_path_tracer_amd.sdf_editor import CompData

    pt = _tracer()
    prog = scenes.SCENES["c2"]().compile(CompData())

    def start(views=2):
        for k in range(views):
            _view(pt, 1 + 2 * k)
            pt.accumulate_history()
        assert _state(pt) == (1.0, float(views))

    def resize_back():
        pt._chk("pt_resize_clear", pt._L.pt_resize_clear(pt._ctx, W + 3, H))
        pt._chk("pt_resize_clear", pt._L.pt_resize_clear(pt._ctx, W, H))

    drops = {"pt_temporal_reset": pt.reset_history, "pt_resize_clear to another size": resize_back,
             "pt_set_program": lambda: (pt.remake_pipeline(prog), pt.set_data(prog.data)),
             "pt_set_data": lambda: pt.set_data(prog.data)}
    for name, call in drops.items():
        start()
        call()
        assert _state(pt) == (0.0, 0.0), name
        assert _code(pt.read_history) == N.PT_ERR_STATE and _code(pt.denoise_history) == N.PT_ERR_STATE, name
    keeps = {"pt_set_camera": lambda: pt.look_at(G.EYE, G.TARGET), "pt_set_camera(NULL)": pt.reset_camera,
             "pt_set_sky": lambda: pt.set_sky(G.sky()), "pt_set_sky(NULL)": pt.clear_sky,
             "a clear": pt.clear, "a dispatch": lambda: pt.dispatch(G.constants(W, H, 9, 0), 1),
             "an option": lambda: pt.set_option("denoise_lds", 0), "moments off": lambda: pt.set_option("moments", 0),
             "moments on": lambda: pt.set_option("moments", 1), "pt_set_tiles": lambda: pt.set_tiles(0, 1),
             "pt_write_accum": lambda: pt.write_image(np.zeros((H, W, 4), np.float32)),
             "pt_render_guides": pt.render_guides, "a refused accumulate": lambda: _code(pt.accumulate_history, normal_cos=2.0)}
    start()
    before = pt.read_history()
    for name, call in keeps.items():
        call()
        assert _state(pt) == (1.0, 2.0), name
        for a, b in zip(pt.read_history(), before):
            assert np.array_equal(G.bits(a), G.bits(b)), name
    # the first accumulate after a drop makes the history a copy of the view; the next one goes on from it
    pt.reset_history()
    _view(pt, 21)
    img, mom = pt.read_image(), pt.read_moments()
    pt.accumulate_history()
    colour, moments, count = pt.read_history()
    assert np.array_equal(G.bits(colour), G.bits(img)) and np.array_equal(G.bits(moments), G.bits(mom))
    assert (count == 2).all() and _state(pt) == (1.0, 1.0)
    _view(pt, 23)
    pt.accumulate_history()
    hit = pt.read_guides()[1][..., 3] != 0
    assert (pt.read_history()[2][hit] == 4).all() and hit.any() and _state(pt) == (1.0, 2.0)
    pt.close()
