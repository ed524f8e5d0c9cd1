"""Pins tests/temporalref.py on the CPU: guides from
denoiseref.guides on c2 at 24x14, synthetic colours.  The whole-image numpy
form agrees bit for bit with a scalar restatement of the contract's
pseudocode, a view reprojects onto itself, every branch and every skip rule
fires, the cap bounds the count, and the special values do what the contract
says."""
import functools

import numpy as np

import denoiseref as D
import gpuharness as G
import momentref as MR
import pyref as P
import temporalref as T
from compute_path_tracer_amd import scenes
from compute_path_tracer_amd.path_tracer import look_at_camera
from test_display import SPECIAL

F = np.float32
W, H = 24, 14
ASPECT = G.aspect(W, H)
CAMERAS = {"A": look_at_camera(G.EYE, G.TARGET), "B": look_at_camera((2.3, 1.4, -2.4), G.TARGET), "fixed": None,
           "posed": look_at_camera((0.4, 0.3, -3.0), G.TARGET), "away": look_at_camera(G.EYE, (4, 3, -5))}
TOL = dict(depth_tolerance=0.05, normal_cos=0.9, albedo_tolerance=0.1)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def view(name):
    return T.View(CAMERAS[name], ASPECT, 1.0)


@functools.lru_cache(maxsize=None)
def guides(name):
    g = D.guides(scenes.SCENES["c2"]().rows(), W, H, ASPECT, 1.0, CAMERAS[name])
    for a in g:
        a.setflags(write=False)
    return g


def colours(seed):
    """A synthetic image and moments: A in [0, 1), M >= A * A, alpha 1."""
    rng = np.random.default_rng(seed)
    A = rng.random((H, W, 4), np.float32)
    M = A * A + rng.random((H, W, 4), np.float32) * F(0.25)
    A[..., 3] = M[..., 3] = F(1.0)
    return A, M


def first(name, seed=1, n=4):
    A, M = colours(seed)
    return T.accumulate(A, M, *guides(name), n, view(name), None, 32.0, **TOL)[0]


def scalar_accumulate(A, M, g0, g1, n_cur, v, hist, max_history, depth_tolerance, normal_cos, albedo_tolerance):
    """The contract's pseudocode, pixel by pixel in float32 scalars over pyref.camera_ray."""
    def ray(vw, x, y):
        cam = P.camera_fields(vw.camera)
        if cam is not None:
            cam = cam[:4] + (F(0.0), cam[5])
        ux = ((F(x) / F(W)) * F(2.0) - F(1.0)) * F(vw.aspect)
        uy = (F(y) / F(H)) * F(2.0) - F(1.0)
        return P.camera_ray(cam, ux, uy, F(vw.fov), None)

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    def fin3(c):
        return bool(np.isfinite(c[:3]).all())

    po, ir, iu, ifw = T.reciprocal_basis(hist.view.camera)
    nc, one = F(n_cur), F(1.0)
    at2 = F(albedo_tolerance) * F(albedo_tolerance)
    Hc, Hm, Hn = A.copy(), M.copy(), np.full((H, W), nc, np.float32)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                if g1[y, x, 3] == 0 or not fin3(A[y, x]) or not fin3(M[y, x]) or not np.isfinite(g0[y, x, 3]):
                    continue
                ro, rd = ray(v, x, y)
                X = [ro[k] + rd[k] * g0[y, x, 3] for k in range(3)]
                d = [X[k] - po[k] for k in range(3)]
                a, b, c = dot(d, ir), dot(d, iu), dot(d, ifw)
                if not c > 0:
                    continue
                fx = ((((a / c) * F(hist.view.fov)) / F(hist.view.aspect)) + one) * F(0.5) * F(W)
                fy = (((b / c) * F(hist.view.fov)) + one) * F(0.5) * F(H)
                if not (fx > -1 and fx < F(W) and fy > -1 and fy < F(H)):
                    continue
                x0, y0 = int(np.floor(fx)), int(np.floor(fy))
                tx, ty = fx - F(x0), fy - F(y0)
                te = F(np.sqrt(dot(d, d)))
                sw, sn, sh, sm = F(0.0), F(0.0), [F(0.0)] * 3, [F(0.0)] * 3
                for j in (0, 1):
                    for i in (0, 1):
                        qx, qy = x0 + i, y0 + j
                        if qx < 0 or qy < 0 or qx >= W or qy >= H or hist.g1[qy, qx, 3] == 0:
                            continue
                        if not (hist.count[qy, qx] > 0 and fin3(hist.colour[qy, qx]) and fin3(hist.moments[qy, qx])):
                            continue
                        qo, qd = ray(hist.view, qx, qy)
                        e = [(qo[k] + qd[k] * hist.g0[qy, qx, 3]) - X[k] for k in range(3)]
                        if not abs(dot(e, g0[y, x])) <= F(depth_tolerance) * te:
                            continue
                        if not dot(g0[y, x], hist.g0[qy, qx]) >= F(normal_cos):
                            continue
                        ea = [hist.g1[qy, qx, k] - g1[y, x, k] for k in range(3)]
                        if not (ea[0] * ea[0] + ea[1] * ea[1]) + ea[2] * ea[2] <= at2:
                            continue
                        w = (tx if i else one - tx) * (ty if j else one - ty)
                        if not w > 0:
                            continue
                        sw = sw + w
                        sh = [sh[k] + w * hist.colour[qy, qx, k] for k in range(3)]
                        sm = [sm[k] + w * hist.moments[qy, qx, k] for k in range(3)]
                        sn = sn + w * hist.count[qy, qx]
                if not sw > 0:
                    continue
                hn = min(sn / sw, F(max_history))
                if not hn > 0:
                    continue
                n = hn + nc
                wgt = nc / n
                omw = one - wgt
                for k in range(3):
                    Hc[y, x, k] = (sh[k] / sw) * omw + A[y, x, k] * wgt
                    Hm[y, x, k] = (sm[k] / sw) * omw + M[y, x, k] * wgt
                Hn[y, x] = n
    return Hc, Hm, Hn


def test_numpy_form_is_the_pseudocode():
    for prev, cur, cap in (("A", "A", 32.0), ("A", "B", 32.0), ("fixed", "posed", 6.0), ("B", "fixed", 32.0)):
        hist = first(prev)
        A, M = colours(2)
        got, counts = T.accumulate(A, M, *guides(cur), 3, view(cur), hist, cap, **TOL)
        want = scalar_accumulate(A, M, *guides(cur), 3, view(cur), hist, cap, **TOL)
        for g, w_ in zip(got[:3], want):
            assert np.array_equal(_bits(g), _bits(w_)), (prev, cur)
        assert counts["taken"] > 0 and np.array_equal(_bits(got.g0), _bits(guides(cur)[0])) and got.view == view(cur)
        assert sum(counts[k] for k in T.BRANCHES[:-1]) == W * H


def test_first_accumulate_and_degenerate_basis_copy_the_view():
    A, M = colours(3)
    hist, counts = T.accumulate(A, M, *guides("A"), 5, view("A"), None, 32.0, **TOL)
    assert counts["no_history"] == W * H and counts["taken"] == 0
    assert np.array_equal(_bits(hist.colour), _bits(A)) and np.array_equal(_bits(hist.moments), _bits(M))
    assert (hist.count == 5).all()
    flat = look_at_camera(G.EYE, G.TARGET)
    for k in range(3):
        flat.up[k] = flat.right[k]  # two equal basis vectors: determinant 0
    assert T.reciprocal_basis(flat) is None
    bad = hist._replace(view=T.View(flat, ASPECT, 1.0))
    again, counts = T.accumulate(A, M, *guides("A"), 5, view("A"), bad, 32.0, **TOL)
    assert counts["no_history"] == W * H and np.array_equal(_bits(again.colour), _bits(A))


def test_reciprocal_basis():
    o, ir, iu, ifw = T.reciprocal_basis(None)
    assert o.tolist() == [0, 0, -3] and ir.tolist() == [1, 0, 0] and iu.tolist() == [0, 1, 0] and ifw.tolist() == [0, 0, 1]
    cam = CAMERAS["B"]
    o, ir, iu, ifw = T.reciprocal_basis(cam)
    basis = np.array([list(cam.right), list(cam.up), list(cam.forward)], np.float64)
    assert np.allclose(np.array([ir, iu, ifw], np.float64) @ basis.T, np.eye(3), atol=1e-6)
    skew = look_at_camera(G.EYE, G.TARGET)
    for k in range(3):
        skew.right[k] = 2.0 * skew.right[k] + 0.5 * skew.forward[k]  # pt_set_camera asks for no orthonormal basis
    o, ir, iu, ifw = T.reciprocal_basis(skew)
    basis = np.array([list(skew.right), list(skew.up), list(skew.forward)], np.float64)
    assert np.allclose(np.array([ir, iu, ifw], np.float64) @ basis.T, np.eye(3), atol=1e-6)


def test_a_view_reprojects_onto_itself():
    """The projection of a view's own hit points lands on the pixel; with a constant history every hit pixel mixes
    that constant with its own colour at the counts' weights."""
    g0, g1 = guides("A")
    hitm = g1[..., 3] != 0
    X = T.hit_points(view("A"), g0)
    po, ir, iu, ifw = T.reciprocal_basis(CAMERAS["A"])
    d = (X - po).astype(np.float64)
    a, b, c = d @ ir.astype(np.float64), d @ iu.astype(np.float64), d @ ifw.astype(np.float64)
    fx = (a / c / ASPECT + 1) * 0.5 * W
    fy = (b / c + 1) * 0.5 * H
    ys, xs = np.mgrid[0:H, 0:W]
    off = max(np.abs(fx - xs)[hitm].max(), np.abs(fy - ys)[hitm].max())
    print(f"self-reprojection at {W}x{H}: at most {off:.2e} px off the pixel")
    assert off < 2e-5
    A, M = colours(4)
    half = np.full((H, W, 4), 0.5, np.float32)
    hist = T.History(half, half.copy(), np.full((H, W), 16.0, np.float32), g0, g1, view("A"))
    got, counts = T.accumulate(A, M, g0, g1, 4, view("A"), hist, 32.0, **TOL)
    assert counts["taken"] == int(hitm.sum()) and counts["outside"] == 0 and counts["behind"] == 0
    wgt = F(4.0) / F(20.0)  # (a count of 16 and weights of 0.5 scale the sums exactly)
    want = np.where(hitm[..., None], F(0.5) * (F(1.0) - wgt) + A[..., :3] * wgt, A[..., :3])
    assert np.array_equal(_bits(got.colour[..., :3]), _bits(want))
    assert (got.count[hitm] == 20).all() and (got.count[~hitm] == 4).all()
    assert np.array_equal(_bits(got.colour[..., 3]), _bits(A[..., 3]))


def test_branches_rules_and_the_cap():
    seen = dict.fromkeys(T.BRANCHES + T.RULES, 0)
    for prev, cur in (("A", "A"), ("A", "B"), ("fixed", "posed"), ("away", "A")):
        hist = first(prev)
        if prev == "A" and cur == "B":  # a stale count and a non-finite history texel on hit pixels
            hist.count[H // 2, W // 2] = 0.0
            hist.colour[H // 2, W // 2 + 1, 1] = np.inf
        A, M = colours(5)
        got, counts = T.accumulate(A, M, *guides(cur), 4, view(cur), hist, 32.0, **TOL)
        print(prev, "->", cur, counts)
        hits = int((guides(cur)[1][..., 3] != 0).sum())
        assert counts["miss"] == W * H - hits
        if prev == "away":
            assert counts["behind"] == hits and counts["taken"] == 0
            assert np.array_equal(_bits(got.colour), _bits(A)) and (got.count == 4).all()
        else:
            assert counts["taken"] >= hits // 2
        for k, v in counts.items():
            seen[k] += v
    A, M = colours(6)
    A[0, 0, 0] = np.nan  # (0, 0) is a miss in every view: put a hit pixel's colour out of range too
    yx = tuple(np.argwhere(guides("B")[1][..., 3] != 0)[0])
    M[yx + (2,)] = np.inf
    _got, counts = T.accumulate(A, M, *guides("B"), 4, view("B"), first("A"), 32.0, **TOL)
    seen["not_finite"] += counts["not_finite"]
    assert counts["not_finite"] == 1
    # (at this size the depth and normal rules take every tap across two shapes first: the albedo rule alone)
    _got, counts = T.accumulate(A, M, *guides("B"), 4, view("B"), first("A"), 32.0, depth_tolerance=10.0, normal_cos=-1.0,
                                albedo_tolerance=0.1)
    assert counts["depth"] == 0 and counts["normal"] == 0
    seen["albedo"] += counts["albedo"]
    missing = [k for k, v in seen.items() if v == 0 and k != "no_history"]
    assert not missing, missing
    # the cap: 0 leaves the current view, a small one bounds the count
    hist = first("A", n=32)  # (a power of two: the gathered count is 32 exactly)
    A, M = colours(7)
    zero, counts = T.accumulate(A, M, *guides("B"), 4, view("B"), hist, 0.0, **TOL)
    assert counts["taken"] == 0 and np.array_equal(_bits(zero.colour), _bits(A)) and (zero.count == 4).all()
    capped, counts = T.accumulate(A, M, *guides("B"), 4, view("B"), hist, 6.0, **TOL)
    free, _ = T.accumulate(A, M, *guides("B"), 4, view("B"), hist, 1000.0, **TOL)
    assert counts["taken"] > 0 and capped.count.max() == 10.0 and free.count.max() == 36.0
    assert not np.array_equal(_bits(capped.colour), _bits(free.colour))


def test_special_values_enter_and_are_left_out():
    special = np.array(SPECIAL, np.float32)
    A, M = colours(8)
    A.reshape(-1)[:len(SPECIAL)] = special
    M.reshape(-1)[:len(SPECIAL)] = np.roll(special, -2)
    assert not np.isfinite(A).all()
    g0 = np.zeros((H, W, 4), np.float32)  # a synthetic wall facing the fixed camera, so every texel is a hit
    g0[..., 2], g0[..., 3] = -1.0, 3.0
    g1 = np.full((H, W, 4), 0.5, np.float32)
    g1[..., 3] = 1.0
    v = T.View(None, ASPECT, 1.0)
    ro, rd = T.rays(v, W, H)
    g0[..., 3] = (F(3.0) / rd[..., 2]).astype(np.float32)  # the plane z = 0 seen from (0, 0, -3)
    hist, _ = T.accumulate(A, M, g0, g1, 4, v, None, 32.0, **TOL)
    assert np.array_equal(_bits(hist.colour), _bits(A))  # that is how they enter
    A2, M2 = colours(9)
    got, counts = T.accumulate(A2, M2, g0, g1, 4, v, hist, 32.0, **TOL)
    assert counts["bad_history"] > 0 and np.isfinite(got.colour).all() and np.isfinite(got.moments).all()
    bad = ~(np.isfinite(A[..., :3]).all(-1) & np.isfinite(M[..., :3]).all(-1))
    assert bad.any() and (got.count[bad] <= 8).all() and counts["taken"] + counts["no_valid_tap"] == W * H
    A3 = A2.copy()
    A3[3, 5, 1] = -np.inf
    got, counts = T.accumulate(A3, M2, g0, g1, 4, v, hist, 32.0, **TOL)
    assert counts["not_finite"] == 1 and got.count[3, 5] == 4 and np.array_equal(_bits(got.colour[3, 5]), _bits(A3[3, 5]))


def test_history_variance_and_filter():
    one = np.ones((1, 2, 4), np.float32)
    hist = T.History(one * F(2.0), one * F(5.0), np.array([[2.0, 5.0]], np.float32), one, one, T.View(None, 1.0, 1.0))
    assert T.history_variance(hist).tolist() == [[3.0, 0.75]]  # (5 - 4) / (n - 1) per channel, summed
    hist = first("A")
    A, M = colours(10)
    hist, _ = T.accumulate(A, M, *guides("B"), 4, view("B"), hist, 32.0, **TOL)
    V = T.history_variance(hist)
    assert np.isfinite(V).all() and (V >= 0).all() and (V > 0).any()
    want = MR.guided(hist.colour, V, hist.g0, hist.g1)
    assert np.array_equal(_bits(T.denoise_history(hist)), _bits(want))
    assert not np.array_equal(_bits(want), _bits(hist.colour))
