"""GPU: the second-moment image, the variance of the mean and their state
(pt_set_option "moments", pt_read_moments / pt_write_moments / pt_read_variance,
DESIGN.md 3.28) bit for bit against tests/momentref.py (pinned on the CPU by
test_moment_ref.py).  Every comparison of images is view(np.uint32) equality.
c3 at 48x27 over 16 frames (two lanes of exactly one PT_FOLD_SLICE each) and
c2 at 61x37 over 11 frames: ragged against the 8x8 tiles, the 256-pixel fold
blocks and the fold's 8-frame slices.
"""
import ctypes
import functools

import numpy as np
import pytest

import gpuharness as G
import momentref as MR
from compute_path_tracer_amd import _native as N
from compute_path_tracer_amd import scenes
from gpuharness import EYE, SKY, TARGET
from gpuharness import bits as _bits

pytestmark = pytest.mark.gpu

C3 = ("c3", 48, 27, 16, 8)  # scene, width, height, frames, bounces
C2 = ("c2", 61, 37, 11, 4)


def _tracer(case, kernel=None, moments=1, **options):
    name, w, h, _n, bounces = case
    return G.tracer(name, w, h, bounces, kernel, extra=dict(options, moments=moments))


def _k(case, frame=1, last_clear=0):
    return G.constants(case[1], case[2], frame, last_clear)


def _assert_same(got, want, what, mask=None):
    same = _bits(got) == _bits(want)
    if mask is not None:
        same = same | ~(mask[..., None] if same.ndim == 3 else mask)
    assert same.all(), (what, np.argwhere(~same)[:5])


def _assert_matches(pt, case, what, mask=None):
    """The context's two images and its variance against the reference's (on the texels of `mask`)."""
    A, M, V = MR.folded(*case)
    assert pt.get_option("moments_valid") == 1.0 and pt.get_option("moment_frames") == case[3], what
    _assert_same(pt.read_image(), A, (what, "A"), mask)
    _assert_same(pt.read_moments(), M, (what, "M"), mask)
    _assert_same(pt.variance(), V, (what, "V"), mask)


@pytest.mark.parametrize("kernel", ["simple", "binned", "binned_jit", "binned_bake", None])
def test_images_and_variance_bit_exact(gpu, kernel):
    pt = _tracer(C3, kernel)
    pt.dispatch(_k(C3), C3[3])
    if kernel is None:  # the automatic choice keeps the moments: the binned pipeline, not the wave kernel, at any size
        assert pt.get_option("kernel") == 0.0 and pt.get_option("trace_launches") > 0 and pt.get_option("bin_chunks") == 1.0
    _assert_matches(pt, C3, kernel)
    print(f"{kernel}: variance_ms={pt.get_option('variance_ms'):.4f}")
    assert pt.get_option("variance_ms") > 0.0
    pt.close()


@pytest.mark.parametrize("kernel", ["simple", "binned_jit"])
def test_one_dispatch_or_two(gpu, kernel):
    pt = _tracer(C2, kernel)
    pt.dispatch(_k(C2), 11)
    _assert_matches(pt, C2, "11")
    pt.clear()
    assert pt.get_option("moments_valid") == 0.0
    pt.dispatch(_k(C2), 3)
    assert pt.get_option("moment_frames") == 3.0
    pt.dispatch(_k(C2, frame=4, last_clear=3), 8)  # last_clear goes on: the moments stay valid
    _assert_matches(pt, C2, "3 + 8")
    pt.close()


@pytest.mark.parametrize("bin_lanes", [1, 2, 3])
def test_bin_lanes(gpu, bin_lanes):
    pt = _tracer(C2, "binned_jit", bin_lanes=bin_lanes)
    pt.dispatch(_k(C2), 11)
    _assert_matches(pt, C2, bin_lanes)
    pt.close()


def test_chunks(gpu):
    n_pix = ((C2[1] + 7) // 8) * ((C2[2] + 7) // 8) * 64
    pt = _tracer(C2, "binned_jit", bin_samples=4 * n_pix)  # four frames per chunk: 4 + 4 + 3
    pt.dispatch(_k(C2), 11)
    assert pt.get_option("bin_chunks") == 3.0
    _assert_matches(pt, C2, "chunks")
    pt.close()


@pytest.mark.parametrize("kernel", ["simple", "binned_jit"])
def test_tiles(gpu, kernel):
    pt = _tracer(C2, kernel)
    pt.set_tiles(0, 3)
    pt.dispatch(_k(C2), 11)
    first = pt.owned()
    assert pt.read_moments()[first][:, :3].any()
    pt.set_tiles(1, 3)  # clears both images: rank 0's texels do not stay behind
    assert pt.get_option("moments_valid") == 0.0
    pt.dispatch(_k(C2), 11)
    own = pt.owned()
    assert 0.2 < own.mean() < 0.5 and not (own & first).any()
    _assert_matches(pt, C2, "tiles", own)
    assert not pt.read_image()[~own].any() and not pt.read_moments()[~own].any() and not pt.variance()[~own].any()
    pt.close()


@functools.lru_cache(maxsize=None)
def _posed_sky_reference():
    w, h, n, bounces = 24, 20, 3, 4
    fr = MR.camref_frames(scenes.SCENES["c2"]().rows(), w, h, G.aspect(w, h), bounces, n, camera=G.camera("pinhole"),
                          sky=G.sky())
    A, M = MR.frames_fold(fr)
    return A, M, MR.variance(A, M, n)


@pytest.mark.parametrize("kernel", ["simple", "binned_jit"])
def test_look_at_and_sky(gpu, kernel):
    A, M, V = _posed_sky_reference()
    assert (V > 0).mean() > 0.5  # the sky lights every path that leaves
    pt = G.tracer("c2", 24, 20, 4, kernel, extra={"moments": 1})
    pt.look_at(EYE, TARGET)
    pt.set_sky(**SKY)
    pt.dispatch(G.constants(24, 20, 1, 0), 3)
    _assert_same(pt.read_image(), A, "A")
    _assert_same(pt.read_moments(), M, "M")
    _assert_same(pt.variance(), V, "V")
    pt.close()


def test_the_image_does_not_change(gpu):
    imgs = []
    for moments in (0, 1):
        pt = _tracer(C2, "binned_jit", moments=moments)
        pt.dispatch(_k(C2), 11)
        imgs.append(pt.read_image())
        assert pt.get_option("moments") == moments and pt.get_option("moments_valid") == moments
        pt.close()
    _assert_same(imgs[1], imgs[0], "moments on / off")
    _assert_same(imgs[0], MR.folded(*C2)[0], "the reference")


def _code(fn, *args, **kw):
    with pytest.raises(N.NativeError) as e:
        fn(*args, **kw)
    return e.value.code


def _state(pt):
    return pt.get_option("moments_valid"), pt.get_option("moment_frames")


def test_state(gpu):
    pt = _tracer(C2, "binned_jit", moments=0)
    assert pt.get_option("moments") == 0.0 and _state(pt) == (0.0, 0.0)
    pt.dispatch(_k(C2), 2)
    assert _state(pt) == (0.0, 0.0) and _code(pt.read_moments) == N.PT_ERR_STATE
    assert _code(pt.variance) == N.PT_ERR_STATE
    pt.set_option("moments", 1)
    assert pt.get_option("moments") == 1.0 and _state(pt) == (0.0, 0.0)
    pt.dispatch(_k(C2, 3, 2), 2)  # goes on from an image without moments: not valid
    assert _state(pt) == (0.0, 0.0)
    pt.dispatch(_k(C2), 1)  # last_clear 0 starts them
    assert _state(pt) == (1.0, 1.0)
    pt.render_guides()
    assert _code(pt.variance) == N.PT_ERR_STATE and _code(pt.denoise_guided) == N.PT_ERR_STATE  # n == 1
    pt.read_moments()
    pt.dispatch(_k(C2, 2, 1), 2)
    assert _state(pt) == (1.0, 3.0)
    pt.variance(), pt.denoise_guided()
    before = pt.read_image(), pt.read_moments()
    pt.stats(_k(C2, 4, 3), 2)  # the instrumented run touches nothing
    assert _state(pt) == (1.0, 3.0)
    _assert_same(pt.read_image(), before[0], "stats A")
    _assert_same(pt.read_moments(), before[1], "stats M")
    pt.dispatch(_k(C2, 6, 5), 1)  # last_clear does not go on from 3
    assert _state(pt) == (0.0, 0.0) and _code(pt.read_moments) == N.PT_ERR_STATE
    pt.dispatch(_k(C2, 7, 6), 1)  # (nor from a count that is no longer valid)
    assert _state(pt) == (0.0, 0.0)
    pt.dispatch(_k(C2), 2)
    assert _state(pt) == (1.0, 2.0)
    pt.settings.debug = 3  # a debug view writes the image
    pt.dispatch(_k(C2, 3, 2), 1)
    assert _state(pt) == (0.0, 0.0)
    pt.settings.debug = 0
    pt.dispatch(_k(C2), 2)
    pt.set_option("moments", 1)  # the value it has: nothing changes
    assert _state(pt) == (1.0, 2.0)
    pt.set_option("moments", 0)
    assert _state(pt) == (0.0, 0.0)
    pt.set_option("moments", 1)
    assert _state(pt) == (0.0, 0.0)
    pt.dispatch(_k(C2), 2)
    pt.set_option("moments", 0)
    pt.dispatch(_k(C2, 3, 2), 1)  # a dispatch with the option off
    pt.set_option("moments", 1)
    assert _state(pt) == (0.0, 0.0)
    pt.dispatch(_k(C2), 2)
    img = pt.read_image()
    pt.write_image(img)
    assert _state(pt) == (0.0, 0.0)
    pt.write_moments(before[1], 7)  # write_image, then write_moments: a render resumed
    assert _state(pt) == (1.0, 7.0)
    _assert_same(pt.read_moments(), before[1], "write_moments")
    _assert_same(pt.variance(), MR.variance(img, before[1], 7), "variance of written images")
    pt.dispatch(_k(C2, 8, 7), 1)
    assert _state(pt) == (1.0, 8.0)
    pt.set_tiles(1, 3)
    assert _state(pt) == (0.0, 0.0)
    ones = np.ones_like(img)
    pt.write_moments(ones, 3)
    assert _state(pt) == (1.0, 3.0)
    pt.clear()  # pt_resize_clear: not valid, and M is zeroed as the image is
    assert _state(pt) == (0.0, 0.0)
    pt.dispatch(_k(C2), 2)
    assert _state(pt) == (1.0, 2.0) and not pt.read_moments()[~pt.owned()].any()
    pt.update(resized=True, window=(40, 24))  # a resize
    assert _state(pt) == (0.0, 0.0)
    pt.dispatch(G.constants(40, 24, 1, 0), 2)
    assert pt.read_moments().shape == (24, 40, 4) and pt.variance().shape == (24, 40)
    pt.close()


def test_the_wave_kernel_is_refused(gpu):
    for kernel in ("wave", "jit"):
        pt = _tracer(C2, "binned_jit")
        pt.dispatch(_k(C2), 2)
        before = pt.read_image(), pt.read_moments()
        for k, v in G.KERNELS[kernel].items():
            pt.set_option(k, v)
        assert _code(pt.dispatch, _k(C2, 3, 2), 1) == N.PT_ERR_UNSUPPORTED
        assert _state(pt) == (1.0, 2.0)
        _assert_same(pt.read_image(), before[0], "A")
        _assert_same(pt.read_moments(), before[1], "M")
        pt.settings.debug = 3  # (a debug view keeps no moments: the wave kernel serves it)
        pt.dispatch(_k(C2, 3, 2), 1)
        pt.settings.debug = 0
        pt.set_option("moments", 0)
        pt.dispatch(_k(C2, 3, 2), 1)  # and with the option off it renders as ever
        pt.close()


def test_arguments(gpu):
    name, w, h, _n, _b = C2
    pt = _tracer(C2, "binned_jit", moments=0)
    img = np.ones((h, w, 4), np.float32)
    assert _code(pt.write_moments, img, 3) == N.PT_ERR_STATE  # without the option
    with pytest.raises(N.NativeError):
        pt.set_option("moments", 2)
    pt.set_option("moments", 1)
    assert _code(pt.write_moments, img, 0) == N.PT_ERR_INVALID and _state(pt) == (0.0, 0.0)
    with pytest.raises(ValueError):
        pt.write_moments(img[:-1], 3)
    pt.dispatch(_k(C2), 2)
    pt.render_guides()
    good = pt.denoise_guided()
    L, fp = pt._L, ctypes.POINTER(ctypes.c_float)
    buf = np.zeros((h, w, 4), np.float32)
    p = buf.ctypes.data_as(fp)
    assert L.pt_read_moments(pt._ctx, p, buf.nbytes - 1) == N.PT_ERR_SIZE
    assert L.pt_read_moments(pt._ctx, None, buf.nbytes) == N.PT_ERR_SIZE
    assert L.pt_write_moments(pt._ctx, p, buf.nbytes - 1, 2) == N.PT_ERR_SIZE
    assert L.pt_write_moments(pt._ctx, None, buf.nbytes, 2) == N.PT_ERR_SIZE
    assert L.pt_read_variance(pt._ctx, p, w * h * 4 - 1) == N.PT_ERR_SIZE
    assert L.pt_read_variance(pt._ctx, None, w * h * 4) == N.PT_ERR_SIZE
    assert not buf.any() and _state(pt) == (1.0, 2.0)  # nothing was written, nothing changed
    assert L.pt_read_moments(None, p, buf.nbytes) == N.PT_ERR_INVALID
    assert L.pt_write_moments(None, p, buf.nbytes, 2) == N.PT_ERR_INVALID
    assert L.pt_read_variance(None, p, buf.nbytes) == N.PT_ERR_INVALID
    for bad in (dict(sigma_variance=0.0), dict(sigma_variance=-1.0), dict(sigma_variance=float("nan")),
                dict(sigma_variance=float("inf")), dict(iterations=0), dict(iterations=9), dict(normal_power_log2=9),
                dict(sigma_depth=-0.5), dict(sigma_albedo=float("nan")), dict(sigma_depth=1e-30)):
        assert _code(pt.denoise_guided, **bad) == N.PT_ERR_INVALID, bad
    with pytest.raises(ValueError):
        pt.denoise_guided(output="png")
    gp = N.GuidedParams(iterations=5, normal_power_log2=5, sigma_variance=2.0, sigma_depth=0.05, sigma_albedo=0.1)
    vp = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.pt_denoise_guided(pt._ctx, None, N.PT_DENOISE_LINEAR, vp, buf.nbytes) == N.PT_ERR_INVALID
    assert L.pt_denoise_guided(pt._ctx, ctypes.byref(gp), 3, vp, buf.nbytes) == N.PT_ERR_INVALID
    assert L.pt_denoise_guided(pt._ctx, ctypes.byref(gp), N.PT_DENOISE_LINEAR, vp, buf.nbytes - 1) == N.PT_ERR_SIZE
    assert L.pt_denoise_guided(pt._ctx, ctypes.byref(gp), N.PT_DISPLAY_SRGB8, vp, w * h * 4 - 1) == N.PT_ERR_SIZE
    assert L.pt_denoise_guided(pt._ctx, ctypes.byref(gp), N.PT_DENOISE_LINEAR, None, buf.nbytes) == N.PT_ERR_SIZE
    assert L.pt_denoise_guided(None, ctypes.byref(gp), N.PT_DENOISE_LINEAR, vp, buf.nbytes) == N.PT_ERR_INVALID
    assert not buf.any()
    pt.clear()  # the guides go with the image: PT_ERR_STATE comes before the moments are asked for
    assert _code(pt.denoise_guided) == N.PT_ERR_STATE
    pt.dispatch(_k(C2), 2)
    assert _code(pt.denoise_guided) == N.PT_ERR_STATE
    pt.render_guides()
    _assert_same(pt.denoise_guided(), good, "the next valid call")
    pt.close()
