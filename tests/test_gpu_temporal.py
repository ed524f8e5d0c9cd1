"""GPU: temporal accumulation (pt_temporal_accumulate / pt_denoise_history,
DESIGN.md 3.30) bit for bit against tests/temporalref.py (pinned on the CPU by
test_temporal_ref.py), the conditions that keep those comparisons from
passing vacuously, and that a history carried along a camera path beats the
last view alone.  Every comparison of images is view(np.uint32) equality, on
the context's own images and guides.  c3 at 61x37 and 4 bounces unless said,
the filter tests' ragged size.
"""
import functools

import numpy as np
import pytest

import gpuharness as G
import temporalref as T
from compute_path_tracer_amd import _native as N
from compute_path_tracer_amd.path_tracer import look_at_camera
from gpuharness import bits as _bits
from oracle import oracle as O
from test_display import SPECIAL

pytestmark = pytest.mark.gpu

W, H, SPP = 61, 37, 4
TOL = dict(depth_tolerance=0.05, normal_cos=0.9, albedo_tolerance=0.1)
A = look_at_camera(G.EYE, G.TARGET)
MOVED = look_at_camera((2.3, 1.4, -2.4), G.TARGET)


def _flat():
    """A's pose with up = right: pt_set_camera takes it, and its basis has no reciprocal."""
    cam = look_at_camera(G.EYE, G.TARGET)
    for k in range(3):
        cam.up[k] = cam.right[k]
    return cam


# name -> (the views in a row, max_history)
CASES = {
    "same": ((A, A), 32.0),
    "small-move": ((A, MOVED), 32.0),
    "fixed-to-posed": ((None, look_at_camera((0.4, 0.3, -3.0), G.TARGET)), 32.0),
    "looking-away": ((look_at_camera(G.EYE, (4, 3, -5)), A), 32.0),  # every point is behind the previous eye
    "three-views": ((A, MOVED, look_at_camera((2.6, 1.3, -2.3), G.TARGET)), 32.0),
    "cap-0": ((A, MOVED), 0.0),
    "cap-3": ((A, MOVED, A), 3.0),
    "degenerate-previous": ((_flat(), A), 32.0),  # determinant 0: nothing can be projected, nothing is taken
}
MOVING = ("small-move", "fixed-to-posed", "three-views", "cap-3")


def _tracer(name="c3", w=W, h=H, bounces=4):
    return G.tracer(name, w, h, bounces, extra=dict(moments=1))


def _render(pt, cam, frame, w=W, h=H, spp=SPP):
    """`cam`'s view on a cleared image: spp frames from `frame`, the guides.  Returns the reference's inputs."""
    pt._set_camera(cam)
    pt.clear()
    pt.dispatch(G.constants(w, h, frame, 0), spp)
    pt.render_guides()
    assert pt.get_option("moment_frames") == spp
    return pt.read_image(), pt.read_moments(), *pt.read_guides(), T.View(cam, G.aspect(w, h), 1.0)


def _same(pt, hist):
    got = pt.read_history()
    return [bool(np.array_equal(_bits(g), _bits(w))) for g, w in zip(got, hist[:3])]


@functools.lru_cache(maxsize=None)
def _case(name):
    """Run a case on the GPU and through the reference: per view, (colour, moments, count agree?, the reference's
    counts, its history, the current image)."""
    cams, cap = CASES[name]
    pt = _tracer()
    hist, steps = None, []
    for k, cam in enumerate(cams):
        img, mom, g0, g1, view = _render(pt, cam, 1 + 16 * k)
        pt.accumulate_history(max_history=cap, **TOL)
        hist, counts = T.accumulate(img, mom, g0, g1, SPP, view, hist, cap, **TOL)
        steps.append((_same(pt, hist), counts, hist, img))
        assert pt.get_option("history_valid") == 1.0 and pt.get_option("history_views") == k + 1
        assert pt.get_option("temporal_ms") > 0.0
        # the accumulate reads the view and writes none of it
        assert np.array_equal(_bits(pt.read_image()), _bits(img)) and np.array_equal(_bits(pt.read_moments()), _bits(mom))
    pt.close()
    return steps


@pytest.mark.parametrize("name", list(CASES))
def test_accumulate_bit_exact(gpu, name):
    steps = _case(name)
    for k, (same, counts, hist, img) in enumerate(steps):
        print(f"{name} view {k}: colour / moments / count bit-exact {same}; {counts}")
        assert same == [True, True, True], (name, k)
    first, last = steps[0], steps[-1]
    assert first[1]["no_history"] == W * H and np.array_equal(_bits(first[2].colour), _bits(first[3]))
    hits = W * H - last[1]["miss"]
    if name == "looking-away":
        assert last[1]["behind"] == hits > 0 and last[1]["taken"] == 0
        assert np.array_equal(_bits(last[2].colour), _bits(last[3])) and (last[2].count == SPP).all()
    if name == "degenerate-previous":
        assert T.reciprocal_basis(CASES[name][0][0]) is None and last[1]["no_history"] == W * H
        assert np.array_equal(_bits(last[2].colour), _bits(last[3])) and (last[2].count == SPP).all()
    if name == "same":
        assert last[1]["taken"] == hits and last[1]["partial"] > 0
    if name == "cap-0":  # the history is the current view, bit for bit
        assert last[1]["taken"] == 0 and np.array_equal(_bits(last[2].colour), _bits(last[3]))
        assert (last[2].count == SPP).all()
    if name == "cap-3":  # a cap that bites: without it the third view would weigh up to 8 samples of history
        assert last[1]["taken"] > 0 and last[2].count.max() == 3.0 + SPP
        assert steps[1][2].count.max() == 3.0 + SPP
    if name == "three-views":
        assert last[2].count.max() > 2 * SPP  # a pixel seen in all three
    if name in MOVING:  # neither nothing nor everything is taken
        for _same_, counts, _hist, _img in steps[1:]:
            hits = W * H - counts["miss"]
            assert counts["taken"] >= hits / 2 and hits - counts["taken"] >= hits / 100, counts
            for rule in ("depth", "normal", "albedo", "prev_miss"):
                assert counts[rule] > 0, (rule, counts)


def _with_special(img, mom, at_the_end):
    """test_display.py's special values in the first (or last) texels of the image and, shifted, of the moments."""
    special = np.array(SPECIAL, np.float32)
    sl = slice(-len(SPECIAL), None) if at_the_end else slice(0, len(SPECIAL))
    img, mom = img.copy(), mom.copy()
    img.reshape(-1)[sl] = special
    mom.reshape(-1)[sl] = np.roll(special, -2)
    return img, mom


@functools.lru_cache(maxsize=None)
def _special_case():
    """The special values enter the history through the first accumulate (first texels); the second view, from the
    same pose so that its taps land on them, carries its own in its last texels; the third has moved."""
    pt = _tracer()
    hist, steps = None, []
    for k, cam in enumerate((A, A, MOVED)):
        img, mom, g0, g1, view = _render(pt, cam, 1 + 16 * k)
        if k < 2:
            img, mom = _with_special(img, mom, at_the_end=k == 1)
            pt.write_image(img)
            pt.write_moments(mom, SPP)
        pt.accumulate_history(max_history=32.0, **TOL)
        hist, counts = T.accumulate(img, mom, g0, g1, SPP, view, hist, 32.0, **TOL)
        steps.append((_same(pt, hist), counts, hist, img))
    pt.close()
    return steps


def test_special_values(gpu):
    steps = _special_case()
    for k, (same, counts, hist, img) in enumerate(steps):
        print(f"special view {k}: bit-exact {same}; {counts}")
        assert same == [True, True, True], k
    assert not np.isfinite(steps[0][2].colour).all() and not np.isfinite(steps[0][2].moments).all()  # they entered
    assert steps[1][1]["bad_history"] > 0 and steps[1][1]["not_finite"] > 0
    # a pixel whose own colour is not finite keeps it and starts again; nothing else of the history is touched by one
    hist, img = steps[1][2], steps[1][3]
    bad = ~(np.isfinite(img[..., :3]).all(-1))
    assert bad.any() and np.array_equal(_bits(hist.colour[bad]), _bits(img[bad])) and (hist.count[bad] == SPP).all()
    assert np.isfinite(hist.colour[~bad]).all()
    assert np.isfinite(steps[2][2].colour[steps[2][2].count > SPP]).all()


def test_every_branch_and_rule_fires(gpu):
    seen = dict.fromkeys(T.BRANCHES + T.RULES, 0)
    for steps in [_case(name) for name in CASES] + [_special_case()]:
        for _same_, counts, _hist, _img in steps:
            for k, v in counts.items():
                seen[k] += v
    print(seen)
    missing = [k for k, v in seen.items() if v == 0]
    assert not missing, missing


def test_denoise_history(gpu):
    pt = _tracer()
    hist = None
    for k, cam in enumerate((A, MOVED)):
        img, mom, g0, g1, view = _render(pt, cam, 1 + 16 * k)
        pt.accumulate_history(max_history=32.0, **TOL)
        hist, _counts = T.accumulate(img, mom, g0, g1, SPP, view, hist, 32.0, **TOL)
    assert _same(pt, hist) == [True, True, True]
    fixed_before, guided_before = pt.denoise(), pt.denoise_guided()
    V = T.history_variance(hist)
    assert np.isfinite(V).all() and (V > 0).any()
    params = {"5": {}, "2-tight": dict(iterations=2, sigma_variance=0.5, sigma_depth=0.01, sigma_albedo=0.02,
                                       normal_power_log2=8), "8": dict(iterations=8)}
    for moved_on in (False, True):
        if moved_on:  # the live guides go stale; the history has its own
            pt._set_camera(A)
            assert pt.get_option("guides_valid") == 0.0 and pt.get_option("history_valid") == 1.0
            with pytest.raises(N.NativeError) as e:
                pt.denoise_guided()
            assert e.value.code == N.PT_ERR_STATE
        for case, p in params.items():
            want = T.denoise_history(hist, **p)
            assert not np.array_equal(_bits(want), _bits(hist.colour))
            for lds in (0, 1):
                pt.set_option("denoise_lds", lds)
                got = pt.denoise_history(**p)
                same = _bits(got) == _bits(want)
                print(f"{case} lds={lds} moved_on={moved_on}: bit-exact={same.mean():.5f} "
                      f"history_denoise_ms={pt.get_option('history_denoise_ms'):.3f} "
                      f"history_variance_ms={pt.get_option('history_variance_ms'):.3f}")
                assert same.all(), (case, lds, np.argwhere(~same)[:5])
                assert pt.get_option("history_denoise_ms") > 0.0 and pt.get_option("history_variance_ms") > 0.0
        pt.set_option("denoise_lds", 1)
        lin = pt.denoise_history()
        assert np.array_equal(_bits(pt.denoise_history(output="display")), _bits(O.display(lin)))
        srgb = pt.denoise_history(output="srgb8")
        assert srgb.dtype == np.uint8 and srgb.shape == (H, W, 4) and np.array_equal(srgb, O.display(lin, srgb8=True))
        if not moved_on:  # the other two filters answer as before, and the view is as it was
            assert np.array_equal(_bits(pt.denoise()), _bits(fixed_before))
            assert np.array_equal(_bits(pt.denoise_guided()), _bits(guided_before))
        assert np.array_equal(_bits(pt.read_image()), _bits(img)) and np.array_equal(_bits(pt.read_moments()), _bits(mom))
        assert _same(pt, hist) == [True, True, True]
    pt.close()


def test_it_helps(gpu):
    """C3 at 96x54, 8 bounces: eight views of 4 spp, the eye stepping along x
    towards a fixed target, each on frames of its own (render_view), against
    the final view's 1024-frame image from frame 5000.  DESIGN.md 3.30 has
    the numbers it prints: raw 0.1061, history 0.0509, denoise_guided of the
    raw view 0.0669, denoise_history 0.0508."""
    w, h, spp, views = 96, 54, 4, 8
    pt = _tracer("c3", w, h, bounces=8)
    eyes = [(G.EYE[0] - 0.05 * (views - 1 - k), G.EYE[1], G.EYE[2]) for k in range(views)]
    for eye in eyes:
        pt.render_view(spp, look_at_camera(eye, G.TARGET))
    assert pt.get_option("history_views") == views and pt.get_option("moment_frames") == spp
    assert pt.constants.frame == views * spp
    raw, raw_guided = pt.read_image(), pt.denoise_guided()
    hist, hist_guided = pt.read_history()[0], pt.denoise_history()
    count = pt.read_history()[2]
    temporal_ms = pt.get_option("temporal_ms")
    pt.clear()
    pt.dispatch(G.constants(w, h, frame=5000, last_clear=0), 1024)
    clean = pt.read_image()
    pt.close()
    assert np.isfinite(clean).all() and np.isfinite(hist).all()

    def rms(a):
        return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - clean[..., :3].astype(np.float64)) ** 2)))

    print(f"C3 {w}x{h} {views} views of {spp} spp, eye step 0.05: rms vs 1024 spp of the final view: raw {rms(raw):.4f}, "
          f"history {rms(hist):.4f}, denoise_guided(raw) {rms(raw_guided):.4f}, denoise_history {rms(hist_guided):.4f}; "
          f"samples per pixel in the history: mean {count.mean():.1f}, max {count.max():.1f}; temporal_ms={temporal_ms:.4f}")
    assert rms(hist) < rms(raw)
    assert rms(hist_guided) < rms(raw_guided)
