"""GPU: the denoiser (pt_render_guides / pt_denoise) bit for
bit against tests/denoiseref.py (pinned on the CPU by test_denoise_ref.py),
its state and argument errors, and that it does denoise.  Every comparison of
images is view(np.uint32) equality.  c2 at 61x37 unless said: ragged against
the guides' 8x8 tiles and the filter's 64x4 and 16x16 blocks, and five
iterations reach 32 texels, past every border of a 37-row image.
"""
import ctypes
import functools

import numpy as np
import pytest

import denoiseref as D
import gpuharness as G
from compute_path_tracer_amd import _native as N
from compute_path_tracer_amd import scenes
from compute_path_tracer_amd.sdf_editor import CompData
from gpuharness import EYE, SKY, TARGET  # the camera tests' pose: part of the frame stays empty
from gpuharness import bits as _bits
from oracle import oracle as O
from test_display import SPECIAL

pytestmark = pytest.mark.gpu

W, H = 61, 37
DEFAULTS = dict(iterations=5, sigma_color=2.0, sigma_depth=0.05, sigma_albedo=0.1, normal_power_log2=5)


def _tracer(name="c2", w=W, h=H, bounces=4, **options):
    return G.tracer(name, w, h, bounces, extra=options)


def _constants(w=W, h=H, frame=1):
    return G.constants(w, h, frame, frame)


@functools.lru_cache(maxsize=None)
def _guides_ref(posed):
    """denoiseref's guide images, computed once per view and shared (read-only)."""
    g0, g1 = D.guides(scenes.c2_sphere_box_torus().rows(), W, H, G.aspect(W, H), 1.0,
                      G.camera("pinhole" if posed else "default"))
    g0.setflags(write=False)
    g1.setflags(write=False)
    return g0, g1


def _assert_guides(pt, ref, what):
    got = pt.read_guides()
    for k in (0, 1):
        same = _bits(got[k]) == _bits(ref[k])
        assert same.all(), (what, k, np.argwhere(~same)[:5])


@pytest.mark.parametrize("posed", [False, True], ids=["fixed", "look_at"])
def test_guides_bit_exact(gpu, posed):
    ref = _guides_ref(posed)
    hit = ref[1][..., 3]
    assert 0.2 < hit.mean() < 0.8 and set(np.unique(hit)) == {0.0, 1.0}  # both hit and miss texels occur
    assert (ref[0][..., 3][hit == 0] > 100.0).all() and np.isfinite(ref[0]).all()
    lengths = np.linalg.norm(ref[0][..., :3].astype(np.float64), axis=-1)
    assert np.allclose(lengths[hit == 1], 1.0, atol=1e-5) and (lengths[hit == 0] == 0).all()
    for jit in (0, 1):
        pt = _tracer(jit=jit)
        assert pt.get_option("guides_valid") == 0.0
        if posed:
            pt.look_at(EYE, TARGET)
        pt.render_guides()
        assert pt.get_option("guides_valid") == 1.0
        _assert_guides(pt, ref, f"jit {jit}")
        if posed and jit == 0:  # a lens is taken as its pinhole
            pt.look_at(EYE, TARGET, aperture=0.05, focus=3.0)
            assert pt.get_option("guides_valid") == 0.0
            pt.render_guides(_constants())
            _assert_guides(pt, ref, "lens")
        if jit == 1:  # every pixel, whatever pt_set_tiles says; it keeps guides that are there
            pt.set_tiles(1, 3)
            assert pt.get_option("guides_valid") == 1.0
            _assert_guides(pt, ref, "after set_tiles")
            pt.render_guides()
            _assert_guides(pt, ref, "under set_tiles")
        pt.close()


@functools.lru_cache(maxsize=None)
def _filter_input():
    """The context's own 3-spp image with test_display.py's special values, and its guides."""
    pt = _tracer()
    pt.dispatch(_constants(), 3)
    img = pt.read_image()
    pt.render_guides()
    g0, g1 = pt.read_guides()
    pt.close()
    img.reshape(-1)[:len(SPECIAL)] = np.array(SPECIAL, np.float32)
    for a in (img, g0, g1):
        a.setflags(write=False)
    return img, g0, g1


PARAMS = {"1": dict(DEFAULTS, iterations=1), "3": dict(DEFAULTS, iterations=3), "5": DEFAULTS,
          "5-sigmas-off": dict(DEFAULTS, sigma_color=0.0, sigma_depth=0.0, sigma_albedo=0.0),
          "5-npow-0": dict(DEFAULTS, normal_power_log2=0), "8-tight": dict(iterations=8, sigma_color=0.5,
                                                                         sigma_depth=0.01, sigma_albedo=0.02,
                                                                         normal_power_log2=8)}


@pytest.mark.parametrize("case", list(PARAMS))
def test_filter_bit_exact(gpu, case):
    params = PARAMS[case]
    img, g0, g1 = _filter_input()
    want = D.atrous(img, g0, g1, **params)
    assert not np.array_equal(_bits(want), _bits(img))
    special = np.zeros((H, W), bool)
    special.reshape(-1)[:(len(SPECIAL) + 3) // 4] = True
    assert np.isfinite(want[~special]).all() and not np.isfinite(want[special]).all()
    pt = _tracer()
    pt.write_image(img)
    pt.render_guides()
    for lds in (0, 1):  # the direct and the LDS-staged form run the same operations
        pt.set_option("denoise_lds", lds)
        got = pt.denoise(**params)
        same = _bits(got) == _bits(want)
        print(f"{case} lds={lds}: bit-exact={same.mean():.5f} denoise_ms={pt.get_option('denoise_ms'):.3f}")
        assert same.all(), (lds, np.argwhere(~same)[:5])
    assert np.array_equal(_bits(pt.read_image()), _bits(img))  # the accumulation image is only read
    pt.close()


def test_outputs_and_the_render_going_on(gpu):
    a, b = _tracer(), _tracer()  # b never denoises
    for pt in (a, b):
        pt.dispatch(_constants(), 3)
    before = a.read_image()
    a.render_guides()
    lin = a.denoise()
    assert np.array_equal(_bits(lin), _bits(D.atrous(before, *a.read_guides(), **DEFAULTS)))
    assert np.array_equal(_bits(a.denoise(output="display")), _bits(O.display(lin)))
    assert np.array_equal(a.denoise(output="srgb8"), O.display(lin, srgb8=True))
    assert np.array_equal(_bits(a.denoise(output="linear")), _bits(lin))
    assert np.array_equal(_bits(a.read_image()), _bits(before))
    for pt in (a, b):
        pt.dispatch(_constants(frame=4), 2)
    assert np.array_equal(_bits(a.read_image()), _bits(b.read_image()))
    assert not np.array_equal(_bits(a.read_image()), _bits(before))
    a.close()
    b.close()


def _code(fn, *args, **kw):
    with pytest.raises(N.NativeError) as e:
        fn(*args, **kw)
    return e.value.code


def test_state_errors(gpu):
    prog = scenes.c2_sphere_box_torus().compile(CompData())
    pt = _tracer()
    pt.dispatch(_constants(), 1)
    assert _code(pt.denoise) == N.PT_ERR_STATE and _code(pt.read_guides) == N.PT_ERR_STATE
    pt.render_guides()
    first = pt.denoise()
    pt.clear()
    assert _code(pt.denoise) == N.PT_ERR_STATE
    pt.render_guides()
    pt.denoise()
    pt.remake_pipeline(prog)
    assert _code(pt.denoise) == N.PT_ERR_STATE
    assert _code(pt.render_guides) == N.PT_ERR_STATE  # no data yet
    pt.set_data(prog.data)
    assert _code(pt.denoise) == N.PT_ERR_STATE
    pt.render_guides()
    pt.denoise()
    pt.set_data(prog.data)
    assert _code(pt.denoise) == N.PT_ERR_STATE
    pt.render_guides()
    pt.look_at(EYE, TARGET)
    assert _code(pt.denoise) == N.PT_ERR_STATE
    pt.reset_camera()
    pt.render_guides()
    pt.set_sky(**SKY)
    pt.set_option("denoise_lds", 0)
    pt.denoise()
    pt.dispatch(_constants(frame=2), 1)
    pt.denoise()
    assert pt.get_option("guides_valid") == 1.0
    pt.update(resized=True, window=(40, 24))  # a resize
    assert pt.size == (40, 24) and _code(pt.denoise) == N.PT_ERR_STATE
    pt.render_guides()
    assert pt.denoise().shape == (24, 40, 4) and pt.read_guides()[0].shape == (24, 40, 4)
    assert first.shape == (H, W, 4)
    pt.close()


def test_argument_errors(gpu):
    pt = _tracer()
    pt.dispatch(_constants(), 1)
    pt.render_guides()
    good = pt.denoise()
    for bad in (dict(iterations=0), dict(iterations=9), dict(normal_power_log2=9), dict(sigma_color=-1.0),
                dict(sigma_depth=-0.5), dict(sigma_albedo=float("nan")), dict(sigma_color=float("inf")),
                dict(sigma_depth=1e-30)):  # (1 / (1e-30)^2 is not finite)
        assert _code(pt.denoise, **bad) == N.PT_ERR_INVALID, bad
    with pytest.raises(ValueError):
        pt.denoise(output="png")
    p = N.DenoiseParams(**DEFAULTS)
    buf = np.zeros((H, W, 4), np.float32)
    vp = buf.ctypes.data_as(ctypes.c_void_p)
    L = pt._L
    assert L.pt_denoise(pt._ctx, None, N.PT_DENOISE_LINEAR, vp, buf.nbytes) == N.PT_ERR_INVALID
    assert L.pt_denoise(pt._ctx, ctypes.byref(p), 3, vp, buf.nbytes) == N.PT_ERR_INVALID
    assert L.pt_denoise(pt._ctx, ctypes.byref(p), N.PT_DENOISE_LINEAR, vp, buf.nbytes - 1) == N.PT_ERR_SIZE
    assert L.pt_denoise(pt._ctx, ctypes.byref(p), N.PT_DISPLAY_SRGB8, vp, W * H * 4 - 1) == N.PT_ERR_SIZE
    assert L.pt_denoise(pt._ctx, ctypes.byref(p), N.PT_DENOISE_LINEAR, None, buf.nbytes) == N.PT_ERR_SIZE
    fp = ctypes.POINTER(ctypes.c_float)
    assert L.pt_read_guides(pt._ctx, buf.ctypes.data_as(fp), None, buf.nbytes - 1) == N.PT_ERR_SIZE
    assert not buf.any()  # nothing was written
    assert L.pt_read_guides(pt._ctx, None, buf.ctypes.data_as(fp), buf.nbytes) == N.PT_OK  # either pointer may be NULL
    assert np.array_equal(_bits(buf), _bits(pt.read_guides()[1]))
    assert np.array_equal(_bits(pt.denoise()), _bits(good))  # the next valid call still works
    pt.close()


def test_refusal_order(gpu):
    """A call that is wrong in every way at once is refused by the first rule
    of the list -- null context, null parameters, format, iterations, normal
    power, sigmas, sigma_variance, a constant that is not finite, state
    (guides, then moments; or the history), output size -- and, that fault
    repaired, by the next one, for each of the three filter entry points."""
    w, h = 24, 16
    pt = _tracer(w=w, h=h, moments=1)  # no guides, no moments, no history yet
    L = pt._L
    buf = np.zeros((h, w, 4), np.float32)
    vp = buf.ctypes.data_as(ctypes.c_void_p)
    fns = {name: getattr(L, name) for name in ("pt_denoise", "pt_denoise_guided", "pt_denoise_history")}
    # every field wrong; then (field, its repair, the refusal it ends) in the order of the rules
    wrong = dict(iterations=0, normal_power_log2=9, sigma_depth=-1.0, sigma_albedo=1e-30)
    repairs = [("iterations", 5, "iterations must be in [1, 8]"),
               ("normal_power_log2", 5, "normal_power_log2 must be in [0, 8]"),
               ("sigma_depth", 0.05, "sigma must be finite and >= 0")]
    state = {}  # entry point -> its call, the parameters repaired, the buffer still short
    for name, fn in fns.items():
        fixed = name == "pt_denoise"
        p = N.DenoiseParams(sigma_color=2.0, **wrong) if fixed else N.GuidedParams(sigma_variance=0.0, **wrong)

        def call(fn=fn, ctx=pt._ctx, params=p, fmt=N.PT_DENOISE_LINEAR, nbytes=buf.nbytes - 1):
            rc = fn(ctx, None if params is None else ctypes.byref(params), fmt, vp, nbytes)
            return rc, L.pt_last_error(pt._ctx).decode()

        assert call(ctx=None, params=None, fmt=3)[0] == N.PT_ERR_INVALID, name
        rc, msg = call(params=None, fmt=3)
        assert rc == N.PT_ERR_INVALID and "null denoise parameters" in msg, (name, rc, msg)
        rc, msg = call(fmt=3)
        assert rc == N.PT_ERR_INVALID and "bad denoise format" in msg, (name, rc, msg)
        for field, good, text in repairs:
            rc, msg = call()
            assert rc == N.PT_ERR_INVALID and text in msg, (name, field, rc, msg)
            setattr(p, field, good)
        if not fixed:
            rc, msg = call()
            assert rc == N.PT_ERR_INVALID and "sigma_variance must be finite and > 0" in msg, (name, rc, msg)
            p.sigma_variance = 2.0
        rc, msg = call()
        assert rc == N.PT_ERR_INVALID and "1 / sigma^2 is not finite" in msg, (name, rc, msg)
        p.sigma_albedo = 0.1
        state[name] = call
    # the state rules, each repaired in turn; the short buffer answers last
    guides, variance, history, size = "guides stale", "no variance", "no history", "output buffer too small"

    def expect(**want):
        got = {name: call() for name, call in state.items()}
        for name, (code, text) in want.items():
            assert got[name][0] == code and text in got[name][1], (name, got[name], code, text)

    S, Z = N.PT_ERR_STATE, N.PT_ERR_SIZE
    expect(pt_denoise=(S, guides), pt_denoise_guided=(S, guides), pt_denoise_history=(S, history))
    pt.render_guides()
    expect(pt_denoise=(Z, size), pt_denoise_guided=(S, variance), pt_denoise_history=(S, history))
    pt.dispatch(G.constants(w, h, frame=1, last_clear=0), 2)
    expect(pt_denoise=(Z, size), pt_denoise_guided=(Z, size), pt_denoise_history=(S, history))
    pt.accumulate_history()
    expect(pt_denoise=(Z, size), pt_denoise_guided=(Z, size), pt_denoise_history=(Z, size))
    assert not buf.any()  # nothing was written
    for name, call in state.items():
        assert call(nbytes=buf.nbytes)[0] == N.PT_OK, name
    pt.close()


def test_it_denoises_and_times(gpu):
    """C3 with a sky at 96x54: the denoised 4-spp image (default parameters) is
    closer to the 1024-spp image than the raw 4-spp image is."""
    w, h = 96, 54
    pt = _tracer("c3", w, h, bounces=8)
    pt.set_sky(**SKY)
    pt.dispatch(_constants(w, h), 4)
    noisy = pt.read_image()
    pt.render_guides()
    den = pt.denoise()
    guide_ms, denoise_ms = pt.get_option("guide_ms"), pt.get_option("denoise_ms")
    pt.dispatch(_constants(w, h, frame=5), 1020)
    clean = pt.read_image()
    pt.close()
    ok = np.isfinite(noisy[..., :3]) & np.isfinite(den[..., :3]) & np.isfinite(clean[..., :3])
    assert ok.mean() > 0.99

    def rms(a):
        return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - clean[..., :3].astype(np.float64))[ok] ** 2)))

    print(f"C3 {w}x{h} sky: rms vs 1024 spp: raw 4 spp {rms(noisy):.5f}, denoised {rms(den):.5f}; "
          f"guide_ms={guide_ms:.3f} denoise_ms={denoise_ms:.3f}")
    assert rms(den) < rms(noisy)
    assert guide_ms > 0.0 and denoise_ms > 0.0
