"""GPU: the posed pinhole and thin-lens camera (pt_set_camera, DESIGN.md
3.24) through every kernel variant, bit for bit against tests/camref.py --
pyref's path arithmetic over the oracle's map() and bounds(), pinned to the
oracle by tests/test_camera_ref.py.  Every comparison is view(np.uint32)
equality of the whole image.

The camera is look_at((2.0, 1.5, -2.5), (0, 0, 0)); the lens adds aperture
0.05, focus 3.0.  The float32 values look_at returned go to the GPU and to
camref alike, so look_at's own rounding is not under test here.
"""
import ctypes
import functools

import numpy as np
import pytest

import camref
from compute_path_tracer_amd import _native as N
from compute_path_tracer_amd import scenes
from compute_path_tracer_amd.path_tracer import PathTracer, look_at_camera
from compute_path_tracer_amd.sdf_editor import CompData
from oracle import oracle as O

pytestmark = pytest.mark.gpu

# the option table of test_gpu_parity.py
KERNELS = {"simple": {"kernel": "simple", "jit": 0}, "wave": {"kernel": "wave", "jit": 0},
           "jit": {"kernel": "wave", "jit": 1, "jit_bake": 0}, "binned": {"kernel": "binned", "jit": 0},
           "binned_jit": {"kernel": "binned", "jit": 1, "jit_bake": 0},
           "binned_bake": {"kernel": "binned", "jit": 1, "jit_bake": 1},
           "binned_tier": {"kernel": "binned", "jit": 1, "jit_bake": 2},
           "binned_trace_taps": {"kernel": "binned", "jit": 1, "jit_bake": 2, "shade_taps": 0}}
ALL = ["simple", "wave", "jit", "binned", "binned_jit", "binned_bake", "binned_tier", "binned_trace_taps"]

EYE, TARGET = (2.0, 1.5, -2.5), (0.0, 0.0, 0.0)
LOOK = {"pinhole": {}, "lens": {"aperture": 0.05, "focus": 3.0}}
FRAME = LAST_CLEAR = 1


def _aspect(w, h):
    return float(np.float32(w) / np.float32(h))


def _camera(kind):
    return look_at_camera(EYE, TARGET, **LOOK[kind])


@functools.lru_cache(maxsize=None)
def _ref(name, w, h, spp, bounces, kind, debug=0):
    """camref's image, computed once per case and shared (read-only)."""
    img = camref.render(scenes.SCENES[name]().rows(), w, h, FRAME, LAST_CLEAR, _aspect(w, h), bounces, spp,
                        debug=debug, camera=_camera(kind))
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _default_image(name, w, h, spp, bounces, debug=0):
    img = O.OracleScene(scenes.SCENES[name]().rows()).render(
        w, h, O.Constants(0.0, FRAME, _aspect(w, h), LAST_CLEAR), O.Settings(debug, bounces, 1.0, 1.0, 0), spp)
    img.setflags(write=False)
    return img


def _tracer(name, w, h, bounces, kernel, debug=0, extra=None):
    prog = scenes.SCENES[name]().compile(CompData())
    opts = dict(KERNELS[kernel])
    opts.update(extra or {})
    pt = PathTracer(w, h, prog, settings=N.Settings(debug=debug, bounces=bounces, scale=1.0, fov=1.0, aabb=0),
                    options=opts)
    if opts["jit"]:
        assert pt.get_option("jit_active") == 1.0, pt.jit_log()
    if opts.get("jit_bake") == 2:  # wait for the values-baked build, so the test runs on it
        pt.set_option("jit_wait", 1)
        assert pt.get_option("jit_tier_active") == 1.0, pt.jit_log()
    return pt


def _constants(w, h):
    return N.Constants(time=0.0, frame=FRAME, aspect=_aspect(w, h), last_clear=LAST_CLEAR)


def _render(name, w, h, spp, bounces, kernel, kind, debug=0, extra=None):
    """The GPU image with the test camera, and the dispatch's gen_trace / gen_norec."""
    pt = _tracer(name, w, h, bounces, kernel, debug, extra)
    cam = pt.look_at(EYE, TARGET, **LOOK[kind])
    assert bytes(cam) == bytes(_camera(kind))  # the values camref gets
    got, dflt = pt.get_camera()
    assert bytes(got) == bytes(cam) and not dflt
    pt.dispatch(_constants(w, h), spp)
    img = pt.read_image()
    flags = (pt.get_option("gen_trace"), pt.get_option("gen_norec"))
    pt.close()
    return img, flags


def _same_bits(a, b):
    return float(np.mean(a.view(np.uint32) == b.view(np.uint32)))


def _check_reference(ref, name, w, h, spp, bounces, debug=0):
    """The reference shows the scene, and not the default camera's view of it."""
    assert np.isfinite(ref).all() and ref[..., :3].mean() > 0
    assert not np.array_equal(ref, _default_image(name, w, h, spp, bounces, debug))


CASES = [("c2", 24, 16, 2, 4), ("c3", 24, 16, 2, 8),
         ("c2", 20, 13, 2, 4)]  # partial tiles: the binned kernels take the gen pass


@pytest.mark.parametrize("kernel", ALL)
@pytest.mark.parametrize("name,w,h,spp,bounces", CASES)
@pytest.mark.parametrize("kind", ["pinhole", "lens"])
def test_posed_camera_every_kernel(gpu, kind, name, w, h, spp, bounces, kernel):
    ref = _ref(name, w, h, spp, bounces, kind)
    _check_reference(ref, name, w, h, spp, bounces)
    img, (gen_trace, gen_norec) = _render(name, w, h, spp, bounces, kernel, kind)
    exact = _same_bits(img, ref)
    print(f"{kernel} {name} {w}x{h} {kind}: bit-exact={exact:.5f} mean={ref[..., :3].mean():.5f}")
    assert exact == 1.0
    if kernel in ("binned_jit", "binned_tier") and w % 8 == 0 and h % 8 == 0:
        # the first pass made its own camera rays and shade pass 0 made them again
        assert gen_trace == 1.0 and gen_norec == 1.0


def test_pinhole_and_lens_images_differ(gpu):
    a, b = _ref("c2", 8, 8, 70, 4, "pinhole"), _ref("c2", 8, 8, 70, 4, "lens")
    assert np.mean(np.any(a.view(np.uint32) != b.view(np.uint32), axis=-1)) > 0.25


@pytest.mark.parametrize("kernel", ["binned_jit", "binned_tier"])
@pytest.mark.parametrize("bin_lanes", [1, 2])
@pytest.mark.parametrize("kind", ["pinhole", "lens"])
def test_one_pixel_over_64_frames(gpu, kind, bin_lanes, kernel):
    """70 frames of an 8x8 image: a first-pass window is one pixel over 64
    frames -- the shape of the box skip (a lens's lanes share no origin, so it
    must skip nothing) and of the in-order fold."""
    ref = _ref("c2", 8, 8, 70, 4, kind)
    _check_reference(ref, "c2", 8, 8, 70, 4)
    img, (gen_trace, _) = _render("c2", 8, 8, 70, 4, kernel, kind, extra={"bin_lanes": bin_lanes})
    assert gen_trace == 1.0
    assert _same_bits(img, ref) == 1.0


@pytest.mark.parametrize("kernel", ["simple", "jit", "binned_jit"])
@pytest.mark.parametrize("debug", [1, 2, 3])
def test_debug_views_posed(gpu, debug, kernel):
    """Normals, albedo and bounce count from the posed pinhole: every hit
    texel is non-zero there, so a wrong ray cannot hide behind black texels."""
    ref = _ref("c3", 24, 16, 2, 8, "pinhole", debug)
    _check_reference(ref, "c3", 24, 16, 2, 8, debug)
    assert np.mean(np.any(ref[..., :3] != 0, axis=-1)) > 0.5
    img, _ = _render("c3", 24, 16, 2, 8, kernel, "pinhole", debug=debug)
    assert _same_bits(img, ref) == 1.0


@pytest.mark.parametrize("kernel", ["simple", "jit", "binned_tier"])
def test_reset_camera_restores_the_default(gpu, kernel):
    w, h, spp, bounces = 24, 16, 2, 8
    pt = _tracer("c3", w, h, bounces, kernel)
    _, dflt = pt.get_camera()
    assert dflt
    pt.look_at(EYE, TARGET, **LOOK["lens"])
    pt.reset_camera()
    cam, dflt = pt.get_camera()
    assert dflt
    assert (list(cam.origin), list(cam.right), list(cam.up), list(cam.forward)) == \
        ([0.0, 0.0, -3.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0])
    is_default = ctypes.c_int(-1)
    assert N.lib().pt_get_camera(pt._ctx, None, ctypes.byref(is_default)) == N.PT_OK and is_default.value == 1
    pt.dispatch(_constants(w, h), spp)
    img = pt.read_image()
    pt.close()
    assert _same_bits(img, _default_image("c3", w, h, spp, bounces)) == 1.0


@pytest.mark.parametrize("kernel", ["jit", "binned_jit"])
def test_tile_split_with_a_lens(gpu, kernel):
    """Two contexts that own alternate tiles, both with the lens camera: their
    sum is the one-context image (a sample depends on its pixel and frame
    only, whoever renders it)."""
    w, h, spp, bounces = 24, 16, 2, 8
    ref = _ref("c3", w, h, spp, bounces, "lens")
    total = np.zeros((h, w, 4), np.float32)
    for rank in range(2):
        pt = _tracer("c3", w, h, bounces, kernel)
        pt.set_tiles(rank, 2)
        pt.look_at(EYE, TARGET, **LOOK["lens"])
        pt.dispatch(_constants(w, h), spp)
        part = pt.read_image()
        pt.close()
        assert np.any(part != 0) and np.any(np.all(part == 0, axis=-1))  # owns some tiles, not all
        total += part
    assert _same_bits(total, ref) == 1.0


def test_invalid_cameras_are_refused(gpu):
    w, h, spp, bounces = 24, 16, 2, 8
    pt = _tracer("c3", w, h, bounces, "jit")
    good = pt.look_at(EYE, TARGET)
    L = N.lib()

    def variant(**kw):
        cam = N.Camera.from_buffer_copy(bytes(good))
        for k, v in kw.items():
            if k == "origin_x":
                cam.origin[0] = v
            else:
                setattr(cam, k, v)
        return cam

    bad = [variant(origin_x=float("nan")), variant(aperture=-1.0), variant(aperture=0.1, focus=0.0),
           variant(focus=float("inf")), variant(aperture=0.1, focus=-2.0)]
    for cam in bad:
        assert L.pt_set_camera(pt._ctx, ctypes.byref(cam)) == N.PT_ERR_INVALID
        assert b"camera" in L.pt_last_error(pt._ctx)
        got, dflt = pt.get_camera()
        assert bytes(got) == bytes(good) and not dflt  # the previous camera stays in force
    with pytest.raises(N.NativeError) as e:
        pt.set_camera((0, 0, -3), (1, 0, 0), (0, 1, 0), (0, 0, 1), aperture=-1.0)
    assert e.value.code == N.PT_ERR_INVALID
    pt.dispatch(_constants(w, h), spp)
    img = pt.read_image()
    pt.close()
    assert _same_bits(img, _ref("c3", w, h, spp, bounces, "pinhole")) == 1.0


def test_camera_calls_mark_the_renderer_changed(gpu):
    """set_camera, look_at and reset_camera set `changed`, so the next
    update() clears the image as for a settings change: render() after a
    camera change starts a fresh accumulation."""
    w, h, spp, bounces = 24, 16, 2, 8
    pt = _tracer("c3", w, h, bounces, "jit")
    for call in (lambda: pt.set_camera((0, 0, -3), (1, 0, 0), (0, 1, 0), (0, 0, 1)),
                 lambda: pt.look_at(EYE, TARGET), pt.reset_camera):
        pt.changed = False
        call()
        assert pt.changed is True
    pt.update()
    assert pt.changed is False
    pt.render(3)  # frames 2..4 of the default view, to be discarded
    pt.look_at(EYE, TARGET)
    pt.constants.frame = 0  # the next frame is 1, as in the reference image
    pt.render(spp)
    img = pt.read_image()
    pt.close()
    assert pt.constants.last_clear == spp
    assert _same_bits(img, _ref("c3", w, h, spp, bounces, "pinhole")) == 1.0


@pytest.mark.parametrize("kernel", ["simple", "jit", "binned_jit"])
@pytest.mark.parametrize("kind", ["pinhole", "lens"])
def test_stats_count_every_sample(gpu, kind, kernel):
    w, h, spp, bounces = 24, 16, 2, 8
    pt = _tracer("c3", w, h, bounces, kernel)
    pt.look_at(EYE, TARGET, **LOOK[kind])
    st = pt.stats(_constants(w, h), spp)
    pt.close()
    assert st["samples"] == w * h * spp
    assert 0 < st["shaded"] <= st["segments"]  # the camera sees the scene
