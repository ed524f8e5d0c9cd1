"""GPU: one long-lived context through postref's walk -- sizes down and up
and sideways, scenes, a value edit, camera moves with the history carried
along, a clear, a resize, tiles, the three users of the shared variance
buffers in every order, the moments option off and on, a lens -- every
image-space product bit for bit against postref after every step, on the
buffers the step before left behind, and every refusal where the flags say a
product is stale, before it is rendered again.  The flags themselves are
followed call by call against postref.Flags.  test_post_ref.py shows, without
a GPU, that the walk reaches the transitions it claims and that a stale buffer
would fail every one of them.  On binned_jit and on simple, the two kernels
that fold moments, in the scripted order and in one seeded permutation."""
import itertools
import time

import pytest

import gpuharness as G
import postref as PR
from compute_path_tracer_amd import _native as N

pytestmark = pytest.mark.gpu

STATE, UNSUPPORTED = N.PT_ERR_STATE, N.PT_ERR_UNSUPPORTED
PLANES = ("colour", "moments", "count")


def _flags_agree(pt, flags, where):
    got = tuple(pt.get_option(k) == 1.0 for k in ("guides_valid", "history_valid", "moments_valid"))
    assert got == (flags.guides, flags.history, flags.moments), f"{where}: flags (guides, history, moments) {got}, " \
        f"model {(flags.guides, flags.history, flags.moments)}"
    views = pt.get_option("history_views")  # 1 after a drop, one more otherwise
    assert views == flags.views, f"{where}: history_views {views}, model {flags.views}"


def _queries(pt, cfg, what, with_picks):
    G.assert_queries(pt, PR.scene(cfg.scene), PR.guides(cfg), PR.picks(cfg) if with_picks else None, what)


def _make(pt, call, step, kernel, flags, where, left=None):
    """One of postref.calls()'s calls on the context, the model following.
    left: the Expect of the step before, whose guides a pt_set_tiles keeps."""
    if call == "remake_pipeline":
        pt.remake_pipeline(PR.scene(step.scene)[0])
    elif call == "set_data":
        pt.set_data(PR.scene(step.scene)[1])
        G.ready(pt, G.KERNELS[kernel])
    elif call == "resize":
        pt.update(resized=True, window=(step.w, step.h))
    elif call == "set_tiles":
        pt.set_tiles(*step.tiles)
    elif call == "set_camera":
        pt._set_camera(PR.CAMERAS[step.camera])
    elif call == "set_moments":
        pt.set_option("moments", step.moments)
    flags.on(call)
    _flags_agree(pt, flags, f"{where}, after {call}")
    if call == "set_tiles" and flags.guides and left is not None:
        # kept, and not only by the flag: the planes the step before rendered, the pixel queries beside them
        # (scene and size are that step's: a change of either came first and would have dropped the guides;
        # the camera is still that step's: postref.calls() sets it after the tiles)
        g0, g1 = pt.read_guides()
        G.assert_same(g0, left.products["g0"], f"{where}: g0 after set_tiles")
        G.assert_same(g1, left.products["g1"], f"{where}: g1 after set_tiles")
        _queries(pt, left.step.cfg, f"{where}, after set_tiles", left.step.w * left.step.h <= 400)
    if call == "set_moments" and step.moments and flags.guides:
        # back on, the guides still valid: the moments are what is missing, until a render from a clear
        code, msg = G.refused(pt.denoise_guided)
        assert code == STATE and "no variance" in msg, f"{where}: {msg}"
        if step.tiles == (0, 1):
            code, msg = G.refused(pt.accumulate_history)
            assert code == STATE and "no variance" in msg, f"{where}: {msg}"


def _history_is(pt, hist, what):
    for name, got, want in zip(PLANES, pt.read_history(), PR.history_planes(hist)):
        G.assert_same(got, want, f"{what}: history {name}")


def _refusals(pt, e, it, where):
    """After the transition and the clear, before anything is rendered again."""
    f, s = e.before, e.step
    assert not f.guides and not f.moments  # (the clear)
    for fn in (pt.read_guides, pt.denoise, pt.denoise_guided, pt.variance, pt.read_moments):
        assert G.refused(fn)[0] == STATE, f"{where}: {fn.__name__} on stale inputs"
    assert G.refused(pt.accumulate_history)[0] == (STATE if s.tiles == (0, 1) else UNSUPPORTED), where
    if f.history:  # it stays through the clear, bit for bit, and filters under its own guides
        _history_is(pt, e.history_before, f"{where}, before the render")
        G.assert_same(pt.denoise_history(iterations=it), PR.denoise_history(e.history_before, iterations=it),
                      f"{where}: denoise_history before the render")
    else:
        for fn in (pt.read_history, pt.denoise_history):
            assert G.refused(fn)[0] == STATE, f"{where}: {fn.__name__} without a history"


def _products(pt, e, where):
    """Every product of the step against postref's."""
    s, p, cfg = e.step, e.products, e.step.cfg
    it = PR.iterations(e.k)
    pt.set_option("denoise_lds", PR.lds(e.k))
    G.assert_same(pt.read_image(), p["A"], f"{where}: the image")
    g0, g1 = pt.read_guides()
    G.assert_same(g0, p["g0"], f"{where}: g0")
    G.assert_same(g1, p["g1"], f"{where}: g1")
    _queries(pt, cfg, where, s.w * s.h <= 400)
    G.assert_same(pt.denoise(iterations=it), p["fixed"], f"{where}: denoise, {it} iterations")
    if s.moments:
        G.assert_same(pt.read_moments(), p["M"], f"{where}: the moments")
        G.assert_same(pt.variance(), p["V"], f"{where}: variance")
        G.assert_same(pt.denoise_guided(iterations=it), p["guided"], f"{where}: denoise_guided, {it} iterations")
    else:
        for fn in (pt.read_moments, pt.variance, pt.denoise_guided):
            code, msg = G.refused(fn)
            assert code == STATE, f"{where}: {fn.__name__} with moments off: {msg}"
    rgba, srgb = PR.display(p["A"])
    G.assert_same(pt.display(), rgba, f"{where}: display")
    G.assert_same(pt.display(srgb8=True), srgb, f"{where}: display srgb8")
    rgba, srgb = PR.display(p["fixed"])
    G.assert_same(pt.denoise(iterations=it, output="display"), rgba, f"{where}: denoise to display")
    G.assert_same(pt.denoise(iterations=it, output="srgb8"), srgb, f"{where}: denoise to srgb8")
    # the history
    if PR.accumulates(s):
        pt.accumulate_history(max_history=s.cap, **PR.TOL)
    else:
        code, msg = G.refused(pt.accumulate_history, max_history=s.cap, **PR.TOL)
        assert code == (UNSUPPORTED if s.tiles != (0, 1) else STATE), f"{where}: accumulate_history: {msg}"
    if e.history is not None:
        _history_is(pt, e.history, where)
        G.assert_same(pt.denoise_history(iterations=it), p["hfiltered"], f"{where}: denoise_history, {it} iterations")
        G.assert_same(pt.denoise_history(iterations=it, output="srgb8"), PR.display(p["hfiltered"])[1],
                      f"{where}: denoise_history to srgb8")
    else:
        assert G.refused(pt.read_history)[0] == STATE, where
    if s.orders:
        _var_users(pt, e, it, where)
    # nothing above wrote the image, the moments or the guides
    G.assert_same(pt.read_image(), p["A"], f"{where}: the image after the products")
    G.assert_same(pt.read_guides()[0], p["g0"], f"{where}: g0 after the products")


def _var_users(pt, e, it, where):
    """pt_read_variance, pt_denoise_guided and pt_denoise_history share mom.var: every order of the three, each
    call compared; then the fixed filter (which shares the colour buffers) between two guided calls."""
    p = e.products
    users = {"variance": (pt.variance, {}, p["V"]), "denoise_guided": (pt.denoise_guided, dict(iterations=it), p["guided"]),
             "denoise_history": (pt.denoise_history, dict(iterations=it), p["hfiltered"])}
    for order in itertools.permutations(users):
        for name in order:
            fn, kw, want = users[name]
            G.assert_same(fn(**kw), want, f"{where}: {name} in the order {order}")
    fn, kw, want = users["denoise_guided"]
    G.assert_same(fn(**kw), want, f"{where}: denoise_guided before denoise")
    G.assert_same(pt.denoise(iterations=it + 1), PR.denoise(e.step.cfg, iterations=it + 1), f"{where}: denoise between")
    G.assert_same(fn(**kw), want, f"{where}: denoise_guided after denoise")


def _open(step, kernel):
    """A fresh context in the step's configuration."""
    prog, data, _rows = PR.scene(step.scene)
    pt = G.tracer(prog, step.w, step.h, PR.BOUNCES, kernel, extra=dict(moments=1))
    if PR.program_of(step.scene) != step.scene:
        pt.set_data(data)
    return pt


def _render(pt, step):
    pt.dispatch(G.constants(step.w, step.h, step.frame0, 0), step.n)
    pt.render_guides()


def _read_all(pt, step, it):
    """Every read-back of a context that holds the step's render and one accumulate from no history."""
    out = {"image": pt.read_image(), "display": pt.display(), "srgb8": pt.display(srgb8=True),
           "fixed": pt.denoise(iterations=it), "t": pt.id_image().t, "shape": pt.id_image().shape}
    out["g0"], out["g1"] = pt.read_guides()
    if step.moments:
        out.update(moments=pt.read_moments(), variance=pt.variance(), guided=pt.denoise_guided(iterations=it))
    if PR.accumulates(step):
        out.update(zip(PLANES, pt.read_history()), hfiltered=pt.denoise_history(iterations=it))
    return out


def _run_walk(kernel, seed):
    order = "scripted" if seed is None else f"seed {seed}"
    steps = PR.walk(seed)
    t_ref = time.perf_counter()
    ex = PR.expectations(steps)
    t0 = time.perf_counter()
    pt = _open(steps[0], kernel)
    flags = PR.Flags()
    prev = left = None
    kept = 0  # the times a set_tiles found guides to keep
    for e in ex:
        s = e.step
        where = f"{kernel}, {order}: '{s.label}' after '{prev.label if prev else 'a fresh context'}'"
        for call in e.calls:
            kept += call == "set_tiles" and flags.guides and left is not None
            _make(pt, call, s, kernel, flags, where, left)
        pt.clear()
        flags.on("clear")
        _flags_agree(pt, flags, f"{where}, after the clear")
        assert (flags.guides, flags.history, flags.moments) == (e.before.guides, e.before.history, e.before.moments)
        _refusals(pt, e, PR.iterations(e.k), where)
        _render(pt, s)
        flags.on("dispatch_moments" if s.moments else "dispatch")
        flags.on("render_guides")
        _flags_agree(pt, flags, f"{where}, after the render")
        _products(pt, e, where)
        if PR.accumulates(s):
            flags.on("accumulate")
        _flags_agree(pt, flags, f"{where}, after the products")
        prev, left = s, e
    walked = time.perf_counter() - t0
    assert kept >= 2, f"{kernel}, {order}: set_tiles met valid guides {kept} times"
    # a fresh context given the final configuration: every read-back the same
    final, it = steps[-1], PR.iterations(len(steps))
    fresh = _open(final, kernel)
    for call in PR.calls(None, final):
        _make(fresh, call, final, kernel, PR.Flags(), f"{kernel}, {order}: the fresh context")
    for c in (pt, fresh):
        c.clear()
        _render(c, final)
        c.reset_history()
        if PR.accumulates(final):
            c.accumulate_history(max_history=final.cap, **PR.TOL)
    a, b = _read_all(pt, final, it), _read_all(fresh, final, it)
    fresh.close()
    pt.close()
    print(f"{kernel}, {order}: {len(steps)} steps in {walked:.2f} s after {t0 - t_ref:.2f} s of reference, "
          f"{time.perf_counter() - t0:.2f} s with the fresh context")
    assert a.keys() == b.keys()
    for name in a:
        G.assert_same(b[name], a[name], f"{kernel}, {order}: fresh context against the walked one after '{prev.label}': {name}")


@pytest.mark.parametrize("kernel", PR.KERNELS)
def test_walk_scripted(gpu, kernel):
    _run_walk(kernel, None)


@pytest.mark.parametrize("kernel", PR.KERNELS)
def test_walk_permuted(gpu, kernel):
    _run_walk(kernel, PR.SEED)
