"""The expectations of test_gpu_post_sizes.py and test_gpu_post_reuse.py,
host side (no GPU): denoiseref.atrous and momentref.guided against a plain
per-pixel, per-tap scalar restatement of DESIGN.md 3.26 / 3.28 at sizes below
the step, where the references' border slices had no pin; postref's image
against the oracle's own; the conditions that keep the edge-size comparisons
from passing vacuously; and, of the walk, that it reaches the transitions it
claims and that every product of every step differs from what the step before
left in memory in at least a tenth of its floats, in both orders.
Comparisons between two CPU results are by bits, a NaN equal to a NaN
whatever its payload (gpuharness.same_or_nan, first_difference): numpy's
elementwise form and the scalar loop need not produce the same NaN.  Every
comparison with the GPU, in the two GPU files, is strict bit equality."""
import numpy as np
import pytest

import denoiseref as D
import gpuharness as G
import momentref as MR
import postref as PR
from gpuharness import bits as _bits
from oracle import oracle as O

F = np.float32
H = (F(0.375), F(0.25), F(0.0625))
H3 = (F(0.5), F(0.25))
INF = F(np.inf)


# -- the scalar restatement ------------------------------------------------------------
def _finite3(c):
    return bool(np.isfinite(c[0]) and np.isfinite(c[1]) and np.isfinite(c[2]))


def _sq3(a, b):
    x, y, z = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return (x * x + y * y) + z * z


def scalar_kc(v, x, y, sv2):
    """the colour constant of pixel (x, y) from the variance plane's 3x3 neighbourhood."""
    h, w = v.shape
    sg, sw3 = F(0.0), F(0.0)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            qx, qy = x + dx, y + dy
            if qx < 0 or qy < 0 or qx >= w or qy >= h:
                continue
            vq = v[qy, qx]
            if not np.isfinite(vq):
                continue
            w3 = H3[abs(dy)] * H3[abs(dx)]
            sw3 = sw3 + w3
            sg = sg + w3 * vq
    g = sg / sw3 if sw3 > F(0.0) else INF
    return F(1.0) / (sv2 * g + F(1e-10))


def scalar_iteration(c, g0, g1, i, kc, kz, ka, npow, v=None, sv2=None):
    """One iteration (from 0) of DESIGN.md 3.26's loop, pixel by pixel and tap
    by tap in f32 scalars; with a variance plane `v`, 3.28's: kc per pixel
    from scalar_kc, the variance filtered beside the colour."""
    h, w = c.shape[:2]
    s = 1 << i
    out = c.copy()
    vout = None if v is None else v.copy()
    one, zero = F(1.0), F(0.0)
    for y in range(h):
        for x in range(w):
            cp = c[y, x]
            if not _finite3(cp):
                continue  # out = c_p, v_out = v_p
            kcp = kc if v is None else scalar_kc(v, x, y, sv2)
            hit_p = g1[y, x, 3]
            sw, sv, sc = zero, zero, [zero, zero, zero]
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qx, qy = x + s * dx, y + s * dy
                    if qx < 0 or qy < 0 or qx >= w or qy >= h:
                        continue
                    cq = c[qy, qx]
                    if not _finite3(cq):
                        continue
                    if dx == 0 and dy == 0:
                        wgt = H[0] * H[0]
                    else:
                        if g1[qy, qx, 3] != hit_p:
                            continue
                        wgt = H[abs(dy)] * H[abs(dx)]
                        den = one + _sq3(cq, cp) * kcp
                        if hit_p != zero:
                            den = den * (one + _sq3(g1[qy, qx], g1[y, x]) * ka)
                            dz = g0[qy, qx, 3] - g0[y, x, 3]
                            den = den * (one + (dz * dz) * kz)
                            n_p, n_q = g0[y, x], g0[qy, qx]
                            nd = (n_p[0] * n_q[0] + n_p[1] * n_q[1]) + n_p[2] * n_q[2]
                            nd = nd if nd > zero else zero  # (max drops a NaN)
                            for _ in range(npow):
                                nd = nd * nd
                            wgt = wgt * nd
                        wgt = wgt / den
                        if not wgt > zero:
                            continue
                    sw = sw + wgt
                    for k in range(3):
                        sc[k] = sc[k] + wgt * cq[k]
                    if v is not None:
                        sv = sv + (wgt * wgt) * v[qy, qx]
            for k in range(3):
                out[y, x, k] = sc[k] / sw
            if v is not None:
                vout[y, x] = sv / (sw * sw)
    return out if v is None else (out, vout)


def scalar_atrous(img, g0, g1, iterations, sigma_color=2.0, sigma_depth=0.05, sigma_albedo=0.1, normal_power_log2=5):
    kc, kz, ka = D.constants(iterations, sigma_color, sigma_depth, sigma_albedo)
    c = np.array(img, np.float32)
    with np.errstate(all="ignore"):
        for i in range(iterations):
            c = scalar_iteration(c, g0, g1, i, kc[i], kz[i], ka, normal_power_log2)
    return c


def scalar_guided(img, V, g0, g1, iterations, sigma_variance=2.0, sigma_depth=0.05, sigma_albedo=0.1,
                  normal_power_log2=5):
    _kc, kz, ka = D.constants(iterations, 0.0, sigma_depth, sigma_albedo)
    sv2 = F(sigma_variance) * F(sigma_variance)
    c, v = np.array(img, np.float32), np.array(V, np.float32)
    with np.errstate(all="ignore"):
        for i in range(iterations):
            c, v = scalar_iteration(c, g0, g1, i, None, kz[i], ka, normal_power_log2, v, sv2)
    return c, v


def _random_input(w, h, seed):
    """Random colour and variance with a few non-finite texels; guides with a
    hit / miss mix: unit normals, depths near 3, albedos from a palette of three."""
    rng = np.random.default_rng(seed)
    c = rng.random((h, w, 4)).astype(np.float32)
    c[..., 3] = 1.0
    v = (rng.random((h, w)) * 0.05).astype(np.float32)
    v[rng.random((h, w)) < 0.2] = 0.0
    hit = rng.random((h, w)) < 0.6
    if w * h > 1:
        hit.reshape(-1)[0], hit.reshape(-1)[-1] = True, False
    n = rng.normal(size=(h, w, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    n = np.where(rng.random((h, w, 1)) < 0.5, n, np.array([0.0, 0.6, -0.8]))  # half of them share a normal
    palette = np.array([[0.8, 0.2, 0.2], [0.8, 0.25, 0.2], [0.1, 0.9, 0.3]])
    g0 = np.zeros((h, w, 4), np.float32)
    g1 = np.zeros((h, w, 4), np.float32)
    g0[..., :3] = np.where(hit[..., None], n, 0.0)
    g0[..., 3] = np.where(hit, 3.0 + 0.1 * rng.random((h, w)), 101.0 + rng.random((h, w)))
    g1[..., :3] = np.where(hit[..., None], palette[rng.integers(0, 3, (h, w))], 0.0)
    g1[..., 3] = hit
    flat, vflat = c.reshape(-1, 4), v.reshape(-1)
    if w * h >= 6:  # a NaN, an infinity and a negative infinity in the colour; an infinite and a NaN variance
        at = rng.choice(w * h, 5, replace=False)
        flat[at[0], 0], flat[at[1], 1], flat[at[2], 2] = np.nan, np.inf, -np.inf
        vflat[at[3]], vflat[at[4]] = np.inf, np.nan
    return c, v, g0, g1


REF_SIZES = [(1, 1), (1, 7), (7, 1), (3, 2), (17, 9)]


@pytest.mark.parametrize("w,h", REF_SIZES, ids=[f"{w}x{h}" for w, h in REF_SIZES])
def test_references_equal_the_scalar_restatement(w, h):
    """Steps 1, 2, 4 and 8: from the second on at or beyond every size but 17x9."""
    for seed in (1, 2):
        c, v, g0, g1 = _random_input(w, h, 100 * w + h + seed)
        for iterations in (1, 4):
            want = scalar_atrous(c, g0, g1, iterations)
            got = D.atrous(c, g0, g1, iterations=iterations)
            assert G.first_difference(got, want) is None, (w, h, seed, iterations, G.first_difference(got, want))
            want, want_v = scalar_guided(c, v, g0, g1, iterations)
            got, got_v = MR.guided(c, v, g0, g1, iterations=iterations, with_variance=True)
            assert G.first_difference(got, want) is None, (w, h, seed, iterations, G.first_difference(got, want))
            assert G.same_or_nan(got_v, want_v).all(), (w, h, seed, iterations, np.argwhere(~G.same_or_nan(got_v, want_v))[:3])
        if w * h > 1:
            assert not np.array_equal(_bits(D.atrous(c, g0, g1, iterations=4)), _bits(c))


def test_smooth3_equals_the_scalar_restatement():
    for w, h in REF_SIZES:
        _c, v, _g0, _g1 = _random_input(w, h, 7 * w + h)
        sv2 = F(2.0) * F(2.0)
        with np.errstate(all="ignore"):
            want = np.array([[scalar_kc(v, x, y, sv2) for x in range(w)] for y in range(h)], np.float32)
            got = (F(1.0) / (sv2 * MR.smooth3(v) + MR.EPS)).astype(np.float32)
        assert G.same_or_nan(got, want).all(), (w, h)


# -- postref's own products ---------------------------------------------------------
def test_image_is_the_oracles():
    """frames_fold of single frames against the oracle's own accumulation: whole, and the tiles of one rank."""
    cfg = PR.Config("c2", 24, 16)
    A, M = PR.image(cfg)
    st = O.Settings(0, 4, 1.0, 1.0, 0)
    osc = O.OracleScene(PR.scene("c2")[2])
    assert G.first_difference(A, osc.render(24, 16, O.Constants(0.0, 1, G.aspect(24, 16), 0), st, 3)) is None
    assert PR.image(cfg)[0] is A and not A.flags.writeable  # cached, read-only
    folded = MR.folded("c2", 24, 16, 3, 4)
    assert np.array_equal(_bits(M), _bits(folded[1])) and np.array_equal(_bits(PR.variance(cfg)), _bits(folded[2]))
    part = PR.image(cfg._replace(w=40, h=24, frame0=17, tiles=(1, 3)))[0]
    want = osc.render(40, 24, O.Constants(0.0, 17, G.aspect(40, 24), 0), st, 3, rank=1, nranks=3)
    assert G.first_difference(part, want) is None
    own = PR.owned(40, 24, (1, 3))
    assert own.any() and not own.all() and not _bits(part[~own]).any()
    lit = cfg._replace(scene="c3")
    assert G.pixels_changed(PR.image(lit._replace(frame0=17))[0], PR.image(lit)[0]) > 24 * 16 // 4  # other frames, another image
    sA, sM = PR.image(cfg._replace(special=True))
    k = len(PR.SPECIAL)
    assert np.array_equal(_bits(sA.reshape(-1)[:k]), _bits(np.array(PR.SPECIAL, np.float32)))
    assert np.array_equal(_bits(sA.reshape(-1)[k:]), _bits(A.reshape(-1)[k:]))
    assert np.array_equal(_bits(sM.reshape(-1)[k:]), _bits(M.reshape(-1)[k:]))


def test_the_edited_scene_moves_a_shape():
    prog, data, rows = PR.scene("c3-moved")
    base = PR.scene("c3")
    assert prog.n_ops == base[0].n_ops and data.shape == base[1].shape and not np.array_equal(data, base[1])
    a, b = PR.guides(PR.Config("c3", 20, 12)), PR.guides(PR.Config("c3-moved", 20, 12))
    assert (_bits(a[0]) != _bits(b[0])).any(-1).mean() > 0.1


# -- the edge sizes: nothing passes vacuously ------------------------------------------
@pytest.mark.parametrize("w,h", list(PR.SIZES), ids=[f"{w}x{h}" for w, h in PR.SIZES])
def test_edge_sizes_are_not_vacuous(w, h):
    cfg = PR.size_config(w, h)
    A, M = PR.image(cfg)
    g0, g1 = PR.guides(cfg)
    V = PR.variance(cfg)
    hit = g1[..., 3]
    print(f"{w}x{h}: hit share {hit.mean():.2f}; V zero / positive / not finite "
          f"{int((V == 0).sum())} / {int((V > 0).sum())} / {int((~np.isfinite(V)).sum())}")
    if w * h >= 64:
        assert cfg.special and 0 < hit.sum() < w * h
        assert (V == 0).any() and (V > 0).any() and not np.isfinite(V).all()
        for it in PR.FIXED_ITERATIONS:
            assert not np.array_equal(_bits(PR.denoise(cfg, iterations=it)[..., :3]), _bits(A[..., :3])), it
        for it in PR.GUIDED_ITERATIONS:
            assert not np.array_equal(_bits(PR.denoise_guided(cfg, iterations=it)[..., :3]), _bits(A[..., :3])), it
    if (w, h) == (1, 1):  # nothing changed is the right answer here, and only here
        for it in PR.FIXED_ITERATIONS:
            assert np.array_equal(_bits(PR.denoise(cfg, iterations=it)), _bits(A))
        for it in PR.GUIDED_ITERATIONS:
            assert np.array_equal(_bits(PR.denoise_guided(cfg, iterations=it)), _bits(A))
    # successive iteration counts give different results wherever a neighbour exists: both result buffers tell
    if w * h >= 64:
        assert not np.array_equal(_bits(PR.denoise(cfg, iterations=1)), _bits(PR.denoise(cfg, iterations=2)))
    chain = PR.temporal_chain(w, h)
    for k in range(len(chain)):
        hist, counts = PR.history(chain[:k + 1])
        hits = w * h - counts["miss"] if k else int((PR.guides(chain[0][0])[1][..., 3] != 0).sum())
        print(f"{w}x{h} view {k} ({PR.TEMPORAL_VIEWS[k]}): hits {hits}; {counts}")
        assert sum(counts[b] for b in PR.T.BRANCHES[:-1]) == w * h
        if k == 0:
            assert counts["no_history"] == w * h
        if w * h >= 64 and k == 1:
            assert counts["taken"] == hits > 0
        if w * h >= 64 and k == 2:
            assert 0 < counts["taken"] < hits
        if w * h >= 16 * 16 and k == 2:
            assert counts["taken"] > 0


@pytest.mark.parametrize("w,h", [s for s in PR.SIZES if s[0] * s[1] >= 64], ids=[f"{w}x{h}" for w, h in PR.SIZES if w * h >= 64])
def test_edge_sizes_temporal_special_values(w, h):
    """The special values enter the history through the first view, meet the
    second view's taps, and the second view's own are refused as not finite."""
    chain = PR.temporal_chain(w, h, special=True)
    (_, first), (_, last) = chain[0][0].special, chain[1][0].special
    hit = PR.guides(chain[0][0])[1][..., 3].reshape(-1) != 0
    assert hit[first:first + 4].all() and hit[last:last + 4].all() and last >= first + 4 and not chain[2][0].special
    h0, _c0 = PR.history(chain[:1])
    h1, c1 = PR.history(chain[:2])
    h2, c2 = PR.history(chain)
    print(f"{w}x{h} with the special values: view 1 {c1}; view 2 {c2}")
    assert not np.isfinite(h0.colour).all() and not np.isfinite(h0.moments).all()
    assert c1["bad_history"] > 0 and c1["not_finite"] > 0 and c1["taken"] > 0 and c2["taken"] > 0
    # a pixel whose own colour is not finite keeps it and starts again
    bad = ~np.isfinite(PR.image(chain[1][0])[0][..., :3]).all(-1)
    assert bad.any() and (h1.count[bad] == chain[1][0].n).all() and not np.isfinite(h1.colour[bad]).all()


# -- the walk ------------------------------------------------------------------------
ORDERS = [None, PR.SEED]


def test_walk_shape():
    steps = PR.walk()
    assert len({s.label for s in steps}) == len(steps) and len({s.frame0 for s in steps}) == len(steps)
    assert all(s.w * s.h <= 72 * 40 and 2 <= s.n <= 4 for s in steps)
    # the Python path tracer renders the posed views: keep them small
    assert all(s.w * s.h <= 160 for s in steps if s.camera != "default")
    perm = PR.walk(PR.SEED)
    assert sorted(s.label for s in perm) == sorted(s.label for s in steps) and perm != steps
    assert perm == PR.walk(PR.SEED)
    key = lambda u: tuple(s.label for s in u)  # noqa: E731
    assert sorted(map(key, PR.units(perm))) == sorted(map(key, PR.units(steps)))
    for order in (steps, perm):  # odd and even counts, and both forms, follow each other at least twice
        for f in (PR.iterations, PR.lds):
            vals = [f(k) for k in range(len(order))]
            flips = [(a, b) for a, b in zip(vals, vals[1:]) if a != b]
            assert len(set(vals)) == 2 and all(flips.count(p) >= 2 for p in set(flips)) and len(set(flips)) == 2
        combos = {(PR.iterations(k) & 1, PR.lds(k)) for k in range(len(order))}
        assert len(combos) == 4


def test_walk_transitions_present():
    got = PR.transitions(PR.walk())
    assert set(PR.CLAIMS) <= got, sorted(set(PR.CLAIMS) - got)
    assert set(PR.CLAIMS) <= {s.label[0] for s in PR.walk()}
    # a permutation keeps the groups whole: what happens inside one stays
    assert set("bcdef") <= PR.transitions(PR.walk(PR.SEED))


def test_flags_along_the_walk():
    """The asymmetries of the flags, where the scripted walk meets them."""
    ex = {e.step.label: e for e in PR.expectations(PR.walk())}
    e = ex["a: 40x72: the same texel count, another stride"]
    assert e.calls == ["resize"] and e.history_before is None and e.counts["no_history"] == 40 * 72
    e = ex["c: clear at the same size: the history stays"]
    assert e.calls == [] and not e.before.guides and e.before.history and e.counts["taken"] > 0
    assert e.history_before is ex["c: the eye moved and the view panned, cap 3"].history
    e = ex["c: a resize drops the history"]
    assert not e.before.history and e.counts["no_history"] == 12 * 8
    e = ex["d: tiles of rank 1 of 3"]
    assert e.calls == ["set_tiles"] and e.before.history and e.counts is None and e.history is e.history_before
    e = ex["d: all tiles again"]
    assert e.before.history and e.counts["taken"] > 0
    e = ex["f: moments off"]
    assert e.counts is None and "V" not in e.products and e.history is not None
    e = ex["c: the eye moved and the view panned, cap 3"]
    assert e.history.count.max() == 3.0 + e.step.n and e.counts["taken"] > 0
    e = ex["f: a lens camera"]  # the guides are the pinhole's, the render is not
    pin = PR.Config("c3", 12, 8, "A", e.step.frame0, e.step.n)
    assert np.array_equal(_bits(e.products["g0"]), _bits(PR.guides(pin)[0]))
    assert G.pixels_changed(e.products["A"], PR.image(pin)[0]) >= 4


@pytest.mark.parametrize("seed", ORDERS, ids=["scripted", "permuted"])
def test_every_transition_could_fail_on_a_stale_buffer(seed):
    """Of each product, the flat prefix the step before left against the new
    expectation over as many floats: at least a tenth of them differ."""
    rows = list(PR.stale_shares(PR.expectations(PR.walk(seed))))
    assert {r[0] for r in rows} == set(PR.STALE)
    worst = min(rows, key=lambda r: r[3])
    print(f"{len(rows)} comparisons; smallest share of differing floats: {worst[3]:.3f} ({worst[0]} of '{worst[1]}' after '{worst[2]}')")
    short = [r for r in rows if r[3] < 0.1]
    assert not short, short
