"""GPU: the variance-guided filter (pt_denoise_guided) bit for
bit against tests/momentref.py (pinned on the CPU by test_moment_ref.py), its
outputs, that it denoises where the fixed filter does not, and render_until.
Every comparison of images is view(np.uint32) equality.  c2 at 61x37 unless
said, as test_gpu_denoise.py: ragged against the filter's 64x4 blocks, and
five iterations reach past every border.
"""
import functools

import numpy as np
import pytest

import gpuharness as G
import momentref as MR
from compute_path_tracer_amd import scenes
from gpuharness import bits as _bits
from oracle import oracle as O
from test_display import SPECIAL

pytestmark = pytest.mark.gpu

W, H = 61, 37
DEFAULTS = dict(iterations=5, sigma_variance=2.0, sigma_depth=0.05, sigma_albedo=0.1, normal_power_log2=5)


def _tracer(name="c2", w=W, h=H, bounces=4, **options):
    return G.tracer(name, w, h, bounces, extra=dict(options, moments=1))


def _constants(w=W, h=H, frame=1, last_clear=0):
    return G.constants(w, h, frame, last_clear)


@functools.lru_cache(maxsize=None)
def _filter_input():
    """The context's own 3-frame image and moments with test_display.py's
    special values in the first texels of both, its guides, and the variance
    the reference forms of the two."""
    pt = _tracer()
    pt.dispatch(_constants(), 3)
    img, mom = pt.read_image(), pt.read_moments()
    pt.render_guides()
    g0, g1 = pt.read_guides()
    pt.close()
    special = np.array(SPECIAL, np.float32)
    img.reshape(-1)[:len(SPECIAL)] = special
    mom.reshape(-1)[:len(SPECIAL)] = np.roll(special, -2)  # (shifted: the infinity meets a finite colour, V = inf there)
    V = MR.variance(img, mom, 3)
    for a in (img, mom, g0, g1, V):
        a.setflags(write=False)
    return img, mom, g0, g1, V


PARAMS = {"1": dict(DEFAULTS, iterations=1), "3": dict(DEFAULTS, iterations=3), "5": DEFAULTS,
          "8": dict(DEFAULTS, iterations=8), "5-sigmas-off": dict(DEFAULTS, sigma_depth=0.0, sigma_albedo=0.0),
          "5-npow-0": dict(DEFAULTS, normal_power_log2=0), "8-tight": dict(iterations=8, sigma_variance=0.5,
                                                                         sigma_depth=0.01, sigma_albedo=0.02,
                                                                         normal_power_log2=8)}


@pytest.mark.parametrize("case", list(PARAMS))
def test_filter_bit_exact(gpu, case):
    params = PARAMS[case]
    img, mom, g0, g1, V = _filter_input()
    assert not np.isfinite(V).all() and (V[np.isfinite(V)] >= 0).all() and (V > 0).any() and (V == 0).any()
    want = MR.guided(img, V, g0, g1, **params)
    assert not np.array_equal(_bits(want), _bits(img))
    special = np.zeros((H, W), bool)
    special.reshape(-1)[:(len(SPECIAL) + 3) // 4] = True
    assert np.isfinite(want[~special]).all() and not np.isfinite(want[special]).all()
    pt = _tracer()
    pt.render_guides()
    pt.write_image(img)
    pt.write_moments(mom, 3)
    fixed_before = pt.denoise()  # (pt_denoise must answer the same afterwards)
    same = _bits(pt.variance()) == _bits(V)
    assert same.all(), np.argwhere(~same)[:5]
    for lds in (0, 1):
        pt.set_option("denoise_lds", lds)
        got = pt.denoise_guided(**params)
        same = _bits(got) == _bits(want)
        print(f"{case} lds={lds}: bit-exact={same.mean():.5f} guided_ms={pt.get_option('guided_ms'):.3f} "
              f"variance_ms={pt.get_option('variance_ms'):.3f}")
        assert same.all(), (lds, np.argwhere(~same)[:5])
    pt.set_option("denoise_lds", 1)
    assert np.array_equal(_bits(pt.read_image()), _bits(img))  # both images are only read
    assert np.array_equal(_bits(pt.read_moments()), _bits(mom))
    assert pt.get_option("moments_valid") == 1.0 and pt.get_option("moment_frames") == 3.0
    assert np.array_equal(_bits(pt.denoise()), _bits(fixed_before))  # pt_denoise is as it was
    pt.close()


def test_outputs_and_the_render_going_on(gpu):
    a, b = _tracer(), _tracer()  # b never denoises
    for pt in (a, b):
        pt.dispatch(_constants(), 3)
    before, mom = a.read_image(), a.read_moments()
    a.render_guides()
    lin = a.denoise_guided()
    want = MR.guided(before, MR.variance(before, mom, 3), *a.read_guides(), **DEFAULTS)
    assert np.array_equal(_bits(lin), _bits(want)) and lin.shape == (H, W, 4)
    assert np.array_equal(_bits(a.denoise_guided(output="display")), _bits(O.display(lin)))
    srgb = a.denoise_guided(output="srgb8")
    assert srgb.dtype == np.uint8 and srgb.shape == (H, W, 4) and np.array_equal(srgb, O.display(lin, srgb8=True))
    assert np.array_equal(_bits(a.denoise_guided(output="linear")), _bits(lin))
    assert np.array_equal(_bits(a.read_image()), _bits(before)) and np.array_equal(_bits(a.read_moments()), _bits(mom))
    for pt in (a, b):
        pt.dispatch(_constants(frame=4, last_clear=3), 2)
        assert pt.get_option("moment_frames") == 5.0
    assert np.array_equal(_bits(a.read_image()), _bits(b.read_image()))
    assert np.array_equal(_bits(a.read_moments()), _bits(b.read_moments()))
    assert not np.array_equal(_bits(a.read_image()), _bits(before))
    a.close()
    b.close()


def test_it_denoises_where_the_fixed_filter_does_not(gpu):
    """C3 without a sky at 96x54, 8 bounces, default parameters: frames 1..n
    against the 1024-frame image from frame 5000.  The GPU image is the
    oracle's bit for bit, so these are test_moment_ref.py's numbers."""
    w, h = 96, 54
    pt = _tracer("c3", w, h, bounces=8)
    pt.render_guides()
    rows, done = [], 0
    for n in (4, 16, 64):
        pt.dispatch(_constants(w, h, frame=1 + done, last_clear=done), n - done)
        done = n
        assert pt.get_option("moment_frames") == n
        rows.append((n, pt.read_image(), pt.denoise(), pt.denoise_guided(), pt.get_option("variance_ms"),
                     pt.get_option("guided_ms"), pt.get_option("denoise_ms")))
    pt.clear()
    pt.dispatch(_constants(w, h, frame=5000), 1024)
    clean = pt.read_image()
    pt.close()
    assert np.isfinite(clean).all()

    def rms(a):
        return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - clean[..., :3].astype(np.float64)) ** 2)))

    for n, raw, fixed, guided, variance_ms, guided_ms, denoise_ms in rows:
        print(f"C3 {w}x{h} {n} spp: rms vs 1024 spp: raw {rms(raw):.4f}, pt_denoise {rms(fixed):.4f}, "
              f"pt_denoise_guided {rms(guided):.4f}; variance_ms={variance_ms:.4f} guided_ms={guided_ms:.3f} "
              f"denoise_ms={denoise_ms:.3f}")
        assert rms(guided) < rms(raw) and rms(guided) < rms(fixed)
        assert variance_ms > 0.0 and guided_ms > 0.0


def test_render_until(gpu):
    max_spp, batch, bar = 64, 8, 1.6
    frames = MR.oracle_frames(scenes.SCENES["c2"]().rows(), W, H, G.aspect(W, H), 4, max_spp)
    want, levels = None, []
    for n in range(batch, max_spp + 1, batch):  # what the reference says of the same frames
        A, M = MR.frames_fold(frames[:n])
        levels.append(MR.noise(A, MR.variance(A, M, n)))
        if want is None and levels[-1] < bar:
            want = n
    print("noise by batch:", " ".join(f"{v:.4f}" for v in levels))
    assert want is not None and batch < want < max_spp  # a bar this render reaches, after more than one batch
    pt = G.tracer("c2", W, H, 4)  # (render_until switches the option on itself)
    assert pt.render_until(bar, max_spp, batch) == want
    assert pt.get_option("moments_valid") == 1.0 and pt.get_option("moment_frames") == want
    assert abs(pt.noise() - levels[want // batch - 1]) < 1e-6
    assert np.array_equal(_bits(pt.read_image()), _bits(MR.frames_fold(frames[:want])[0]))
    pt.render(1)  # render() goes on from them
    assert pt.get_option("moment_frames") == want + 1
    assert np.array_equal(_bits(pt.read_image()), _bits(MR.frames_fold(frames[:want + 1])[0]))
    assert pt.render_until(0.0, 24, batch) == 24  # a bar no render reaches
    assert pt.get_option("moment_frames") == 24.0
    pt.close()
