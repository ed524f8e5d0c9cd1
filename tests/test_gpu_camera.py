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
import gpuharness as G
from compute_path_tracer_amd import _native as N
from compute_path_tracer_amd import scenes
from gpuharness import ALL, EYE, LOOK, TARGET

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ref(name, w, h, spp, bounces, kind, debug=0):
    """camref's image, computed once per case and shared (read-only)."""
    img = camref.render(scenes.SCENES[name]().rows(), w, h, 1, 1, G.aspect(w, h), bounces, spp, debug=debug,
                        camera=G.camera(kind))
    img.setflags(write=False)
    return img


def _render(name, w, h, spp, bounces, kernel, kind, debug=0, extra=None):
    """The GPU image with the test camera, and the dispatch's gen_trace / gen_norec."""
    pt = G.tracer(name, w, h, bounces, kernel, debug, extra)
    cam = pt.look_at(EYE, TARGET, **LOOK[kind])
    assert bytes(cam) == bytes(G.camera(kind))  # the values camref gets
    got, dflt = pt.get_camera()
    assert bytes(got) == bytes(cam) and not dflt
    pt.dispatch(G.constants(w, h), spp)
    img = pt.read_image()
    flags = (pt.get_option("gen_trace"), pt.get_option("gen_norec"))
    pt.close()
    return img, flags


def _check_reference(ref, name, w, h, spp, bounces, debug=0):
    """The reference shows the scene, and not the default camera's view of it."""
    assert np.isfinite(ref).all() and ref[..., :3].mean() > 0
    assert not np.array_equal(ref, G.oracle_image(name, w, h, spp, bounces, debug))


CASES = [("c2", 24, 16, 2, 4), ("c3", 24, 16, 2, 8),
         ("c2", 20, 13, 2, 4)]  # partial tiles: the binned kernels take the gen pass


@pytest.mark.parametrize("kernel", ALL)
@pytest.mark.parametrize("name,w,h,spp,bounces", CASES)
@pytest.mark.parametrize("kind", ["pinhole", "lens"])
def test_posed_camera_every_kernel(gpu, kind, name, w, h, spp, bounces, kernel):
    ref = _ref(name, w, h, spp, bounces, kind)
    _check_reference(ref, name, w, h, spp, bounces)
    img, (gen_trace, gen_norec) = _render(name, w, h, spp, bounces, kernel, kind)
    exact = G.same_bits(img, ref)
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
    assert G.same_bits(img, ref) == 1.0


@pytest.mark.parametrize("kernel", ["simple", "jit", "binned_jit"])
@pytest.mark.parametrize("debug", [1, 2, 3])
def test_debug_views_posed(gpu, debug, kernel):
    """Normals, albedo and bounce count from the posed pinhole: every hit
    texel is non-zero there, so a wrong ray cannot hide behind black texels."""
    ref = _ref("c3", 24, 16, 2, 8, "pinhole", debug)
    _check_reference(ref, "c3", 24, 16, 2, 8, debug)
    assert np.mean(np.any(ref[..., :3] != 0, axis=-1)) > 0.5
    img, _ = _render("c3", 24, 16, 2, 8, kernel, "pinhole", debug=debug)
    assert G.same_bits(img, ref) == 1.0


@pytest.mark.parametrize("kernel", ["simple", "jit", "binned_tier"])
def test_reset_camera_restores_the_default(gpu, kernel):
    w, h, spp, bounces = 24, 16, 2, 8
    pt = G.tracer("c3", w, h, bounces, kernel)
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
    pt.dispatch(G.constants(w, h), spp)
    img = pt.read_image()
    pt.close()
    assert G.same_bits(img, G.oracle_image("c3", w, h, spp, bounces)) == 1.0


@pytest.mark.parametrize("kernel", ["jit", "binned_jit"])
def test_tile_split_with_a_lens(gpu, kernel):
    """Two contexts that own alternate tiles, both with the lens camera: their
    sum is the one-context image (a sample depends on its pixel and frame
    only, whoever renders it)."""
    w, h, spp, bounces = 24, 16, 2, 8
    ref = _ref("c3", w, h, spp, bounces, "lens")
    total = np.zeros((h, w, 4), np.float32)
    for rank in range(2):
        pt = G.tracer("c3", w, h, bounces, kernel)
        pt.set_tiles(rank, 2)
        pt.look_at(EYE, TARGET, **LOOK["lens"])
        pt.dispatch(G.constants(w, h), spp)
        part = pt.read_image()
        pt.close()
        assert np.any(part != 0) and np.any(np.all(part == 0, axis=-1))  # owns some tiles, not all
        total += part
    assert G.same_bits(total, ref) == 1.0


def test_invalid_cameras_are_refused(gpu):
    w, h, spp, bounces = 24, 16, 2, 8
    pt = G.tracer("c3", w, h, bounces, "jit")
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
    pt.dispatch(G.constants(w, h), spp)
    img = pt.read_image()
    pt.close()
    assert G.same_bits(img, _ref("c3", w, h, spp, bounces, "pinhole")) == 1.0


def test_camera_calls_mark_the_renderer_changed(gpu):
    """set_camera, look_at and reset_camera set `changed`, so the next
    update() clears the image as for a settings change: render() after a
    camera change starts a fresh accumulation."""
    w, h, spp, bounces = 24, 16, 2, 8
    pt = G.tracer("c3", w, h, bounces, "jit")
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
    assert G.same_bits(img, _ref("c3", w, h, spp, bounces, "pinhole")) == 1.0


@pytest.mark.parametrize("kernel", ["simple", "jit", "binned_jit"])
@pytest.mark.parametrize("kind", ["pinhole", "lens"])
def test_stats_count_every_sample(gpu, kind, kernel):
    w, h, spp, bounces = 24, 16, 2, 8
    pt = G.tracer("c3", w, h, bounces, kernel)
    pt.look_at(EYE, TARGET, **LOOK[kind])
    st = pt.stats(G.constants(w, h), spp)
    pt.close()
    assert st["samples"] == w * h * spp
    assert 0 < st["shaded"] <= st["segments"]  # the camera sees the scene
