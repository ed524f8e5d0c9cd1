"""GPU: every image-space product at the sizes where a block, a tile or a
halo ends (postref.SIZES) -- the guides, the pixel queries, the variance
plane, the fixed and the variance-guided filter in the direct and the
LDS-staged form, the display pass, temporal accumulation and the history's
filter -- bit for bit against postref's expectations, which come from the
CPU references alone (pinned by test_post_ref.py, which also shows that none
of these comparisons passes vacuously).  Every comparison is view(np.uint32)
equality; the context's image and moments are first shown to be the CPU's.
c2 under the reference's fixed view at 3 frames and 4 bounces, with
test_display.py's special values from 64 texels on; the temporal runs on c3
at 4 frames per view."""
import numpy as np
import pytest

import gpuharness as G
import postref as PR

pytestmark = pytest.mark.gpu

SIZES = list(PR.SIZES)
IDS = [f"{w}x{h}" for w, h in SIZES]


def _context(cfg):
    """A context that holds the configuration's image and moments: rendered,
    shown to be the CPU's, then (special) overwritten with the written arrays."""
    w, h = cfg.w, cfg.h
    pt = G.tracer(PR.scene(cfg.scene)[0], w, h, cfg.bounces, extra=dict(moments=1))
    pt.dispatch(G.constants(w, h, cfg.frame0, 0), cfg.n)
    A, M = PR.image(cfg._replace(special=False))
    G.assert_same(pt.read_image(), A, f"{w}x{h}: the rendered image")
    G.assert_same(pt.read_moments(), M, f"{w}x{h}: the rendered moments")
    if cfg.special:
        A, M = PR.image(cfg)
        pt.write_image(A)
        pt.write_moments(M, cfg.n)
    pt.render_guides()
    return pt


def _queries(pt, cfg, what, with_picks):
    G.assert_queries(pt, PR.scene(cfg.scene), PR.guides(cfg), PR.picks(cfg) if with_picks else None, what)


@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_guides_and_queries(gpu, w, h):
    cfg = PR.size_config(w, h)
    pt = _context(cfg)
    g0, g1 = pt.read_guides()
    G.assert_same(g0, PR.guides(cfg)[0], f"{w}x{h}: g0")
    G.assert_same(g1, PR.guides(cfg)[1], f"{w}x{h}: g1")
    _queries(pt, cfg, f"{w}x{h}", w * h <= PR.PICK_TEXELS)
    # a list of pixels: the corners, in reverse
    xy = np.array([(w - 1, h - 1), (0, h - 1), (w - 1, 0), (0, 0)], np.int32)
    got = pt.pick_pixels(xy)
    G.assert_same(got.t, PR.guides(cfg)[0][xy[:, 1], xy[:, 0], 3], f"{w}x{h}: pick_pixels of the corners")
    pt.close()


@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_variance_and_filters(gpu, w, h):
    cfg = PR.size_config(w, h)
    pt = _context(cfg)
    A, M = PR.image(cfg)
    G.assert_same(pt.variance(), PR.variance(cfg), f"{w}x{h}: variance")
    for lds in (0, 1):
        pt.set_option("denoise_lds", lds)
        for it in PR.FIXED_ITERATIONS:
            G.assert_same(pt.denoise(iterations=it), PR.denoise(cfg, iterations=it), f"{w}x{h}: denoise, {it} iterations, lds {lds}")
        for it in PR.GUIDED_ITERATIONS:
            G.assert_same(pt.denoise_guided(iterations=it), PR.denoise_guided(cfg, iterations=it),
                          f"{w}x{h}: denoise_guided, {it} iterations, lds {lds}")
        G.assert_same(pt.variance(), PR.variance(cfg), f"{w}x{h}: variance after the guided filter, lds {lds}")
    if (w, h) == (1, 1):  # no neighbour: the colour is the input's, bit for bit
        G.assert_same(pt.denoise(iterations=8), A, "1x1: denoise against its input")
        G.assert_same(pt.denoise_guided(iterations=8), A, "1x1: denoise_guided against its input")
    G.assert_same(pt.read_image(), A, f"{w}x{h}: the image after the filters")
    G.assert_same(pt.read_moments(), M, f"{w}x{h}: the moments after the filters")
    pt.close()


@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_display(gpu, w, h):
    cfg = PR.size_config(w, h)
    pt = _context(cfg)
    rgba, srgb = PR.display(PR.image(cfg)[0])
    G.assert_same(pt.display(), rgba, f"{w}x{h}: display")
    G.assert_same(pt.display(srgb8=True), srgb, f"{w}x{h}: display srgb8")
    for it, lds in ((2, 1), (5, 0), (2, 0), (5, 1)):  # the result in either buffer, through the display pass
        pt.set_option("denoise_lds", lds)
        rgba, srgb = PR.display(PR.denoise(cfg, iterations=it))
        G.assert_same(pt.denoise(iterations=it, output="display"), rgba, f"{w}x{h}: denoise to display, {it} iterations")
        G.assert_same(pt.denoise(iterations=it, output="srgb8"), srgb, f"{w}x{h}: denoise to srgb8, {it} iterations")
    rgba, srgb = PR.display(PR.denoise_guided(cfg, iterations=5))
    G.assert_same(pt.denoise_guided(output="display"), rgba, f"{w}x{h}: denoise_guided to display")
    G.assert_same(pt.denoise_guided(output="srgb8"), srgb, f"{w}x{h}: denoise_guided to srgb8")
    G.assert_same(pt.display(), PR.display(PR.image(cfg)[0])[0], f"{w}x{h}: display after the filters' display passes")
    pt.close()


@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_temporal(gpu, w, h):
    """The views (A, A, MOVED) of test_gpu_temporal.py's special-value case;
    MOVED as it is: under it the third view takes history at every size from
    16x16 on (529 of 549 hits at 17x33, 87 of 103 at 64x4: test_post_ref.py
    prints the counts), and refuses some from 64 texels on.  The image and
    moments of each view are the fixed camera's render (postref.temporal_chain
    says why), the guides and the reprojection the view's.  From 64 texels
    on the run is repeated with the special values written as that case
    writes them: into the first view's image and moments, so that they enter
    the history, and elsewhere into the second's (postref.temporal_chain)."""
    for special in ((False, True) if w * h >= 64 else (False,)):
        _temporal_run(w, h, PR.temporal_chain(w, h, special), " with the special values" if special else "")


def _temporal_run(w, h, chain, tag):
    pt = G.tracer(PR.scene("c3")[0], w, h, 4, extra=dict(moments=1))
    for k, (cfg, cap) in enumerate(chain):
        what = f"{w}x{h}{tag} view {k} ({cfg.view})"
        pt.reset_camera()
        pt.clear()
        pt.dispatch(G.constants(w, h, cfg.frame0, 0), cfg.n)
        A, M = PR.image(cfg._replace(special=False))
        G.assert_same(pt.read_image(), A, f"{what}: the rendered image")
        G.assert_same(pt.read_moments(), M, f"{what}: the rendered moments")
        if cfg.special:  # the written arrays: the expectation is formed from them
            A, M = PR.image(cfg)
            pt.write_image(A)
            pt.write_moments(M, cfg.n)
        pt._set_camera(PR.CAMERAS[cfg.view])
        pt.render_guides()
        g0, g1 = pt.read_guides()
        G.assert_same(g0, PR.guides(cfg)[0], f"{what}: g0")
        G.assert_same(g1, PR.guides(cfg)[1], f"{what}: g1")
        pt.accumulate_history(max_history=cap, **PR.TOL)
        hist, counts = PR.history(chain[:k + 1])
        print(f"{what}: {counts}")
        for name, got, want in zip(("colour", "moments", "count"), pt.read_history(), PR.history_planes(hist)):
            G.assert_same(got, want, f"{what}: history {name}")
        assert pt.get_option("history_views") == k + 1
    want = PR.denoise_history(hist, iterations=5)
    for lds in (0, 1):
        pt.set_option("denoise_lds", lds)
        G.assert_same(pt.denoise_history(iterations=5), want, f"{w}x{h}{tag}: denoise_history, lds {lds}")
    for name, got, want in zip(("colour", "moments", "count"), pt.read_history(), PR.history_planes(hist)):
        G.assert_same(got, want, f"{w}x{h}{tag}: history {name} after its filter")
    pt.close()
